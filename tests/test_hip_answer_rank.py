"""The VQA answer ranking and loop on a real MI355X: xfm_answer_shortlist and xfm_answer_rerank against torch, rank_answer(fused=True)
against the ATen path, the answer decoder with `encoder_batch_index` against the tiled call, and xfm_amd.vqa_loop against the reference's
loop (tests/golden/vqa_loop_small.npz).

Tolerances:
  PROB_TOL    shortlist probabilities, relative.  The reference is softmax -> index_select in fp64, rounded to fp32.  torch's OWN fp32
              softmax on the very inputs of these cases (vqa_loop_util.shortlist_case, CPU) is within 7.2e-8, 1.3e-7, 3.7e-7, 4.3e-7,
              1.9e-7 and 3.7e-7 of it over the six cases' shortlisted entries; the bound is twice the worst: 2 x 4.315e-7.
  RERANK_TOL  re-rank probabilities, relative, against the ATen lines in fp32.  Both sides form s = log(p) - loss in fp32 with |s| < 64,
              ulp(s) <= 2^-18 = 3.8e-6; two correct logf differ by an ulp of log(p) (<= 2^-21), which can move the rounded s by one ulp(s),
              i.e. exp() by 3.8e-6 relative, once in the numerator and once (opposite sign at worst) through the sum: 7.6e-6, plus
              < 1e-6 for expf / the sum / the division -> 1e-5.
  module      2e-3 on rank_answer's probabilities (tests/test_hip_modules.py::test_vqa_model_vs_golden), rtol = atol = 3e-3 on the
              decoder's per-sequence losses (::test_causal_lm_answer_decoder_vs_golden), 2e-3 relative on the loop's losses
              (tests/test_hip_imagenet_loop.py LOSS_TOL)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load, state_from_spec  # noqa: E402
from vqa_loop_util import SHORTLIST_CASES, eval_loader, fixture, loop_config, shortlist_case, shortlist_reference, train_batches  # noqa: E402
from xfm_amd import pretrain_loop as PL  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402
from xfm_amd import vqa_loop as VL  # noqa: E402

PROB_TOL = 2 * 4.315e-7
RERANK_TOL = 1e-5
MODULE_PROB_TOL, DECODER_TOL, LOSS_TOL = 2e-3, 3e-3, 2e-3


def _fx():
    from xfm_amd import functional as Fx
    return Fx


# ------------------------------------------------------------------------------------------------------------- shortlist
@pytest.mark.parametrize("case", SHORTLIST_CASES, ids=lambda c: "Q{}_V{}_ld{}_A{}_k{}_{}".format(*c))
def test_answer_shortlist_matches_torch(case, monkeypatch):
    Q, V, ld, A, k, kind = case
    logits, first = shortlist_case(*case)
    ref_p, ref_i, p_all = shortlist_reference(logits, V, first, k)
    # the order of DISTINCT probabilities is decided far above the arithmetic's error (else "indices match exactly" would test rounding)
    d = (ref_p[:, :-1] - ref_p[:, 1:]) / ref_p[:, :-1]
    assert not bool(((d > 0) & (d < 1e-3)).any())
    if kind == "ties":   # the cut falls inside a group of equal probabilities in every row
        s = torch.sort(p_all, dim=1, descending=True).values
        assert bool((s[:, k - 1] == s[:, k]).all())
    if kind == "aligned":   # 16-byte granules up to column V & ~3, then a scalar tail
        dev = torch.empty(Q, ld, device="cuda")
        dev.copy_(logits)
        assert dev.data_ptr() % 16 == 0 and ld % 4 == 0 and V % 4 != 0
    elif ld != V:        # an odd base as well: the rows start one float into the allocation
        buf = torch.empty(Q * ld + 1, device="cuda")
        dev = buf[1:].view(Q, ld)
        dev.copy_(logits)
        assert dev.data_ptr() % 16 != 0 or ld % 4 != 0
    else:
        dev = logits.cuda()
    prob, cand = _fx().answer_shortlist(dev, V, first.cuda(), k)
    assert prob.shape == cand.shape == (Q, k) and cand.dtype == torch.int64
    rel = float(((prob.cpu() - ref_p).abs() / ref_p).max())
    print(case, "max relative error", rel)
    assert torch.equal(cand.cpu(), ref_i), (cand.cpu()[:, :12].tolist(), ref_i[:, :12].tolist())
    assert rel <= PROB_TOL, rel
    monkeypatch.setenv("XFM_DETERMINISTIC", "1")
    prob_d, cand_d = _fx().answer_shortlist(dev, V, first.cuda(), k)
    assert torch.equal(prob_d, prob) and torch.equal(cand_d, cand)


def test_answer_shortlist_argument_errors_launch_nothing():
    from xfm_amd import _lib
    Fx = _fx()
    lib = _lib.load()
    logits = torch.randn(2, 40, device="cuda")
    first = torch.arange(16, device="cuda")
    big = torch.zeros(Fx.ANSWER_MAX_A + 1, dtype=torch.int64, device="cuda")
    prob = torch.full((2, Fx.ANSWER_MAX_K + 1), 7.0, device="cuda")
    cand = torch.full((2, Fx.ANSWER_MAX_K + 1), 7, dtype=torch.int64, device="cuda")
    for A, k, tok in ((16, 17, first), (16, 0, first), (Fx.ANSWER_MAX_A + 1, 8, big), (Fx.ANSWER_MAX_A, Fx.ANSWER_MAX_K + 1, big)):
        rc = lib.xfm_answer_shortlist(logits.data_ptr(), 40, 2, 40, tok.data_ptr(), A, k, prob.data_ptr(), cand.data_ptr(), None)
        assert rc == -1 and b"answer_shortlist" in lib.xfm_last_error(), (A, k)
    with pytest.raises(_lib.XfmHipError, match="answer_shortlist"):
        Fx.answer_shortlist(logits, 40, first, 17)
    torch.cuda.synchronize()
    assert float(prob.min()) == 7.0 and int(cand.min()) == 7


# ------------------------------------------------------------------------------------------------------------- re-rank
def _rerank_case(Q, k, seed=0):
    """Scores on a lattice (seq_loss = 5 + 0.25 i, prob = 2^-(1 + i % 4)): distinct scores are >= 0.057 nats apart, so the order of distinct
    values is decided; (row 0) one zero probability; (last row) two entries with equal probability AND equal loss: an exact tie."""
    g = torch.Generator().manual_seed(77 + seed + 1000 * k)
    loss = torch.stack([5.0 + 0.25 * torch.randperm(k, generator=g).float() for _ in range(Q)])
    prob = torch.stack([0.5 ** (1 + torch.randperm(k, generator=g) % 4).float() for _ in range(Q)])
    cand = torch.stack([torch.randperm(4 * k + 3, generator=g)[:k] for _ in range(Q)])
    if k >= 8:
        prob[0, 3] = 0.0
        a, b = 1, k - 2
        prob[Q - 1, b], loss[Q - 1, b] = prob[Q - 1, a], loss[Q - 1, a]
    return prob, loss.reshape(-1), cand


def _rerank_aten(prob, loss, cand):
    """model_generation.py:194-200 as the module's ATen path runs them, with the stable sort that pins the tie order."""
    Q, k = prob.shape
    log_probs_sum = torch.cat([prob.view(-1, 1).log(), -loss.view(-1, 1)], dim=1).sum(1).view(Q, k)
    p = torch.softmax(log_probs_sum, dim=-1)
    s = torch.sort(p, dim=1, descending=True, stable=True)
    return torch.gather(cand, 1, s.indices), s.values


@pytest.mark.parametrize("Q,k", [(1, 1), (3, 8), (32, 128)])
def test_answer_rerank_matches_aten(Q, k, monkeypatch):
    prob, loss, cand = (t.cuda() for t in _rerank_case(Q, k))
    ref_ids, ref_p = _rerank_aten(prob, loss, cand)
    result = torch.full((Q + 5,), -9, dtype=torch.int64, device="cuda")
    ids, p = _fx().answer_rerank(prob, loss, cand, result, 3)
    assert torch.equal(ids, ref_ids), (ids[:2].tolist(), ref_ids[:2].tolist())
    rel = float(((p - ref_p).abs() / ref_p.clamp_min(1e-30)).max())
    print((Q, k), "max relative error", rel)
    assert rel <= RERANK_TOL, rel
    assert result[:3].tolist() == [-9] * 3 and result[3 + Q:].tolist() == [-9] * 2     # the neighbours of the written range
    assert torch.equal(result[3:3 + Q], ref_ids[:, 0])
    if k >= 8:
        assert float(p[0, -1]) == 0.0 and int(ids[0, -1]) == int(cand[0, 3])          # the zero probability: score -inf, last
        pos = {int(c): j for j, c in enumerate(ids[Q - 1].tolist())}
        a, b = int(cand[Q - 1, 1]), int(cand[Q - 1, k - 2])
        assert pos[b] == pos[a] + 1 and float(p[Q - 1, pos[a]]) == float(p[Q - 1, pos[b]])   # the tie: earlier position first
    monkeypatch.setenv("XFM_DETERMINISTIC", "1")
    ids_d, p_d = _fx().answer_rerank(prob, loss, cand)
    assert torch.equal(ids_d, ids) and torch.equal(p_d, p)


# ------------------------------------------------------------------------------------------------------------- modules
def _model_cfg(meta):
    return {"use_beit_v2": True, "image_res": meta.get("image_res", 224), "patch_size": 16, "local_attn_depth": -1, "text_encoder": "roberta-base",
            "text_num_hidden_layers": meta["text_layers"], "text_fusion_start_at": meta["text_layers"],
            "fusion_num_hidden_layers": meta["fusion_layers"], "fusion_fusion_start_at": 0, "embed_dim": 256, "temp": 0.07,
            "learnable_temp": True, "max_temp": 0.5, "min_temp": 0.001, "vision_depth": meta.get("vit_depth", 12),
            "pad_token_id": meta["pad_token_id"], "decoder_fusion_start_at": meta["dec_fusion_start"], "num_dec_layers": meta["dec_layers"]}


def test_rank_answer_fused_against_the_aten_path():
    from xfm_amd.model_generation import XFMForVQA
    z, meta = load("vqa_small")
    m = XFMForVQA(_model_cfg(meta))
    m.load_state_dict(state_from_spec(meta["spec"]), strict=True)
    m.cuda().finalize().eval()
    x = syn.vqa_inputs(image_res=meta.get("image_res", 224))
    q, c = (x.q_ids.cuda(), x.q_atts.cuda()), (x.c_ids.cuda(), x.c_atts.cuda())
    with torch.no_grad():
        ids0, p0 = m(x.image.cuda(), q, c, k=x.topk, train=False)
        result = torch.full((5,), -1, dtype=torch.int64, device="cuda")
        ids1, p1 = m(x.image.cuda(), q, c, k=x.topk, train=False, fused=True, result=result, result_offset=1)
    print("aten", ids0.tolist(), p0.tolist(), "fused", ids1.tolist(), p1.tolist())
    for r in range(ids0.shape[0]):
        assert sorted(ids0[r].tolist()) == sorted(ids1[r].tolist())
        assert int(ids1[r, 0]) == int(ids0[r, int(p0[r].argmax())])
        by_id = {int(i): float(p) for i, p in zip(ids0[r], p0[r])}
        assert all(abs(float(p) - by_id[int(i)]) < MODULE_PROB_TOL for i, p in zip(ids1[r], p1[r]))
    assert result.tolist() == [-1] + ids1[:, 0].tolist() + [-1]


def test_answer_decoder_with_encoder_batch_index_against_the_tiled_call():
    from xfm_amd.xroberta import RobertaConfig, RobertaForCausalLM
    z, meta = load("causal_lm_2L")
    B, S = meta["B"], meta["S"]
    m = RobertaForCausalLM(RobertaConfig(num_hidden_layers=meta["layers"], fusion_layer=0, encoder_width=768))
    m.load_state_dict(state_from_spec(meta["spec"]), strict=True)
    m.cuda().finalize().eval()
    ids, atts, enc_atts = (torch.tensor(meta[k]).cuda() for k in ("ids", "atts", "enc_atts"))
    enc = syn.gaussian("causal.question_states", (B, S, 768), 0.7).cuda()
    index = torch.tensor([0, 0, 0, 1, 1, 1][:B], device="cuda")
    labels = ids.masked_fill(ids == 1, -100)
    with torch.no_grad():
        tiled = m(ids, attention_mask=atts, encoder_hidden_states=enc[index], encoder_attention_mask=enc_atts[index], labels=labels,
                  return_dict=True, reduction="none")
        shared = m(ids, attention_mask=atts, encoder_hidden_states=enc[:2].contiguous(), encoder_attention_mask=enc_atts[:2].contiguous(),
                   labels=labels, return_dict=True, reduction="none", encoder_batch_index=index)
    print("tiled", tiled.loss.tolist(), "shared", shared.loss.tolist())
    assert torch.allclose(shared.loss.float(), tiled.loss.float(), rtol=DECODER_TOL, atol=DECODER_TOL)


# ------------------------------------------------------------------------------------------------------------- loop
@pytest.fixture(scope="module")
def gold():
    z, meta = fixture()
    return z, meta, state_from_spec(meta["spec"])


def _build(gold, train):
    """The fixture model on the GPU; for training behind RCCLDDPAccelerator with the four-group optimizer and the linear schedule.  Dropout
    and drop-path are off, as in the fixture (the reference model stayed in eval mode)."""
    from xfm_amd.accelerators import RCCLDDPAccelerator
    from xfm_amd.model_generation import XFMForVQA
    z, meta, sd = gold
    cfg = loop_config(meta, text_config={"hidden_dropout_prob": 0.0, "attention_probs_dropout_prob": 0.0})
    m = XFMForVQA(cfg)
    m.load_state_dict(sd, strict=True)
    m.cuda()
    for blk in m.vision_encoder.blocks:
        blk.drop_path_prob = 0.0
    if not train:
        return cfg, m.finalize().eval(), None, None, None
    opt = PL.create_optimizer(PL.AttrDict(cfg["optimizer"]), m)
    sch = PL.AttrDict(cfg["schedular"])
    sch["step_per_epoch"] = len(meta["train_seeds"])
    scheduler = PL.create_scheduler(sch, opt)
    losses = []

    class Recording(RCCLDDPAccelerator):
        def backward_step(self, loss, optimizer, sync=None):
            losses.append(loss.detach())
            return super().backward_step(loss, optimizer, sync=sync)

    acc = Recording({"RNG_SEED": 3, "CLIP_GRAD_NORM": 0.0, "GRAD_ACCUMULATE_STEPS": 1})
    wrapped, opt, scheduler = acc.set_up(m, opt, scheduler, 0, 1, 0)
    return cfg, wrapped, opt, scheduler, (acc, losses)


def test_evaluation_against_the_reference_with_one_device_read(gold, monkeypatch):
    z, meta, _ = gold
    cfg, m, _, _, _ = _build(gold, train=False)
    loader = eval_loader(z, meta)
    reads, fused_calls = [], []
    real = VL._read
    monkeypatch.setattr(VL, "_read", lambda t: (reads.append(tuple(t.shape)), real(t))[1])
    orig = m.rank_answer
    monkeypatch.setattr(m, "rank_answer", lambda *a, **kw: (fused_calls.append(kw.get("fused")), orig(*a, **kw))[1])
    records = VL.evaluation(m, loader, torch.device("cuda"), cfg)
    print("records", records, "reference", meta["records"])
    assert reads == [(meta["eval_B"],)] and fused_calls == [True, True]
    assert records == meta["records"]
    # the shortlist and the re-rank themselves against the reference's (margins recorded by the generator: 8th / 9th first-token
    # probabilities >= 30 % apart, the winner ahead by >= 0.2 in probability)
    image, question, _ = eval_loader(z, meta, splits=(meta["eval_B"],))[0]
    cands = tuple(t.cuda() for t in loader.dataset.answer_input)
    with torch.no_grad():
        ids, probs = m(image.cuda(), tuple(t.cuda() for t in question), cands, k=cfg["k_test"], train=False, fused=True)
    ref_ids = z["eval/topk_ids"]
    for r in range(meta["eval_B"]):
        assert sorted(ids[r].tolist()) == sorted(z["eval/shortlist"][r].tolist())
        assert int(ids[r, 0]) == int(ref_ids[r, 0]) and abs(float(probs[r, 0]) - float(z["eval/topk_probs"][r, 0])) < MODULE_PROB_TOL


def test_two_training_iterations_against_the_reference(gold):
    z, meta, _ = gold
    cfg, wrapped, opt, scheduler, (acc, losses) = _build(gold, train=True)
    VL.train_one_epoch(wrapped, train_batches(meta), opt, 0, torch.device("cuda"), scheduler, cfg, acc)
    got = [float(l) for l in losses]
    ref = z["train/loss"].tolist()[:2]
    print("losses", got, "reference", ref)
    assert len(got) == 2
    assert [g["lr"] for g in opt.param_groups] == z["train/lr"][2].tolist()   # after two scheduler steps
    for g, w in zip(got, ref):
        assert abs(g - w) <= LOSS_TOL * abs(w), (got, ref)


# ------------------------------------------------------------------------------------------------------------- script
def test_vqa_script_main_trains_evaluates_and_writes_result_files(gold, tmp_path):
    """VQA.py's main() as `run.py --task vqa` starts it, at the fixture's shallow shape with synthetic loaders: two training iterations, the
    log line, the checkpoint, an evaluation pass through the accelerator's wrapped model; then the `--evaluate` form on a fresh model."""
    import json
    from types import SimpleNamespace as NS

    import VQA as script
    _, meta, _ = gold
    cfg = loop_config(meta, synthetic=True, train_dataset_size=2 * meta["B"], test_dataset_size=8, batch_size_test=4, answer_list_size=24,
                      answer_len=meta["answer_len"], max_tokens=meta["max_tokens"], max_answers=meta["max_answers"], print_freq=1)
    cfg["schedular"]["epochs"] = 1
    out = tmp_path / "vqa"
    (out / "result").mkdir(parents=True)
    args = NS(checkpoint="", bs=-1, seed=42, evaluate=False, output_dir=str(out), result_dir=str(out / "result"))
    script.main(args, dict(cfg))
    assert [json.loads(l)["epoch"] for l in (out / "log.txt").read_text().splitlines()] == [0]
    assert (out / "model_state_epoch_0.th").exists() and (out / "training_state_latest.th").exists()
    args.evaluate = True
    script.main(args, dict(cfg))
    names = set(script.SyntheticTestSet(8, 24, 0, answer_len=meta["answer_len"]).answer_list)
    for f in ("vqa_result_epoch0.json", "vqa_eval.json"):
        records = json.loads((out / "result" / f).read_text())
        assert [r["question_id"] for r in records] == list(range(8)) and all(r["answer"] in names for r in records), (f, records)
