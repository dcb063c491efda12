"""Host side of the VQA fine-tune / evaluation loop (xfm_amd.vqa_loop) without a GPU: the schedule and the optimizer groups value for value,
the loop on the CPU model path (oracle forward, HF-rule AdamW stepping) against tests/golden/vqa_loop_small.npz -- the REFERENCE's loop,
see tools/oracle/gen_vqa_loop.py -- calculate_acc, the launcher's command line, and the ABI of the two answer-ranking kernels.

Parameter probes after the steps are NOT compared across implementations (Adam's first updates are sign-like: a 1e-7 gradient difference
on a near-zero entry flips a full lr); the loss trajectory carries the update instead."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

from vqa_loop_util import eval_loader, fixture, loop_config, oracle_model, train_batches
from xfm_amd import pretrain_loop as PL
from xfm_amd import vqa_loop as VL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, ref):
    """tests/test_oracle_golden.py's rule (golden_util.check): |err| <= 2e-5 + 2e-4 * rms of the reference."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rms = float(np.sqrt((ref * ref).mean()))
    err = float(np.abs(got - ref).max())
    assert err <= 2e-5 + 2e-4 * rms, (err, rms, got, ref)


@pytest.fixture(scope="module")
def gold():
    z, meta = fixture()
    return z, meta, oracle_model(meta)


class _HFStep:
    """backward / step without an arena, stepping with the transformers AdamW rule that optim.py's optimizer stands for (eps before the bias
    correction, decay after the update): what xfm_adamw runs on the GPU."""

    def __init__(self):
        self.losses, self.t = [], {}

    def backward_step(self, loss, optimizer):
        self.losses.append(float(loss.detach()))
        loss.backward()

    @torch.no_grad()
    def optimizer_step(self, optimizer, model):
        for g in optimizer.param_groups:
            b1, b2 = g["betas"]
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = optimizer.state[p]
                if not st:
                    st["step"], st["exp_avg"], st["exp_avg_sq"] = 0, torch.zeros_like(p), torch.zeros_like(p)
                st["step"] += 1
                st["exp_avg"].mul_(b1).add_(p.grad, alpha=1 - b1)
                st["exp_avg_sq"].mul_(b2).addcmul_(p.grad, p.grad, value=1 - b2)
                step_size = g["lr"] * math.sqrt(1 - b2 ** st["step"]) / (1 - b1 ** st["step"])
                p.addcdiv_(st["exp_avg"], st["exp_avg_sq"].sqrt().add_(g["eps"]), value=-step_size)
                if g["weight_decay"] > 0:
                    p.add_(p, alpha=-g["lr"] * g["weight_decay"])


def _optimizer(meta, model):
    opt = PL.create_optimizer(PL.AttrDict(meta["optimizer"]), model)
    sch = PL.AttrDict(meta["schedular"])
    sch["step_per_epoch"] = len(meta["train_seeds"])
    return opt, PL.create_scheduler(sch, opt), sch


def test_schedule_and_groups_match_the_reference_value_for_value(gold):
    z, meta, model = gold
    opt, scheduler, sch = _optimizer(meta, model)
    assert (sch["num_warmup_steps"], sch["num_training_steps"]) == (meta["num_warmup_steps"], meta["num_training_steps"]) == (1, 4)
    assert [len(g["params"]) for g in opt.param_groups] == meta["groups"]
    names = {id(p): n for n, p in model.named_parameters()}
    assert [names[id(g["params"][0])] if g["params"] else None for g in opt.param_groups] == meta["group_first"]
    assert [g["weight_decay"] for g in opt.param_groups] == [0.01, 0.0, 0.01, 0.0]
    assert tuple(opt.param_groups[0]["betas"]) == tuple(meta["betas"]) and opt.param_groups[0]["eps"] == meta["eps"]
    ref = z["train/lr"]
    assert ref.dtype == np.float64 and ref.shape == (4, 4)
    got = []
    for _ in range(4):
        got.append([g["lr"] for g in opt.param_groups])
        opt.step()
        scheduler.step()
    assert np.array_equal(np.asarray(got), ref), (got, ref.tolist())
    assert got[0] == [0.0] * 4 and got[1] == [1e-4, 1e-4, 2e-4, 2e-4]   # warm-up from 0, the peak, lr_mult = 2 on groups 2 and 3


def test_loop_on_the_cpu_model_path_reproduces_the_reference(gold, tmp_path):
    z, meta, _ = gold
    model = oracle_model(meta)
    cfg = loop_config(meta, start_eval=1)
    # the evaluation pass at the formula weights: the fixture's records, shortlist and re-rank
    loader = eval_loader(z, meta)
    records = VL.evaluation(model, loader, "cpu", cfg)
    assert records == meta["records"]
    assert all(set(r) == {"question_id", "answer"} for r in records)
    with torch.no_grad():
        image, question, _ = eval_loader(z, meta, splits=(5,))[0]
        ids, probs = model(image, question, loader.dataset.answer_input, k=cfg["k_test"], train=False)
    assert ids.tolist() == z["eval/topk_ids"].tolist()
    _close(probs.numpy(), z["eval/topk_probs"])
    assert meta["margin_8_9"] > 0.3 and meta["winner_margin"] > 0.2
    # 2 epochs x 2 iterations through train(): losses, the schedule, log.txt, the checkpoints, the result file of epoch 1
    opt, scheduler, _ = _optimizer(meta, model)
    acc = _HFStep()
    saved = []

    class Ckpt:
        def save_checkpoint(self, model_state, epoch, training_states, step=-1):
            saved.append((epoch, sorted(model_state), len(training_states["state"])))

    results = VL.train(model, train_batches(meta), loader, opt, "cpu", scheduler, cfg, acc, Ckpt(), str(tmp_path), str(tmp_path / "result"))
    print("losses", acc.losses, "reference", z["train/loss"].tolist())
    _close(acc.losses, z["train/loss"])
    assert [g["lr"] for g in opt.param_groups] == [0.0] * 4   # the linear decay ended
    assert saved == [(0, ["config", "model"], meta["stepped"]), (1, ["config", "model"], meta["stepped"])]
    lines = [json.loads(l) for l in open(tmp_path / "log.txt")]
    assert [l["epoch"] for l in lines] == [0, 1] and lines[0]["train_loss"] == "{:.5f}".format(np.mean(acc.losses[:2]))
    assert results == [str(tmp_path / "result" / "vqa_result_epoch1.json")]
    out = json.load(open(results[0]))
    assert [r["question_id"] for r in out] == meta["question_ids"] and all(r["answer"] in meta["answer_list"] for r in out)
    assert VL.calculate_acc(results[0], loader.dataset) is None   # a test split: annotations without answers (VQA.py:105-109)


def test_calculate_acc_hand_worked(tmp_path, capsys):
    from types import SimpleNamespace as NS
    path = VL.save_result([{"question_id": 7, "answer": "yes"}, {"question_id": 8, "answer": " two "}, {"question_id": 9, "answer": "red"},
                           {"question_id": 7, "answer": "no"}], str(tmp_path), "vqa_eval")
    assert path == str(tmp_path / "vqa_eval.json")
    ds = NS(ann=[{"question_id": 7, "answer": "yes "}, {"question_id": 8, "answer": "two"}, {"question_id": 9, "answer": "blue"}])
    assert VL.calculate_acc(path, ds) == 0.5
    assert "n_questions: 4, n_correct: 2" in capsys.readouterr().out
    assert VL.calculate_acc(path, NS(ann=[{"question_id": 7, "answer": "yes"}, {"question_id": 8}])) is None


def test_accumulate_steps_above_one_raises(gold):
    z, meta, model = gold
    opt, scheduler, _ = _optimizer(meta, model)
    with pytest.raises(NotImplementedError, match="accumulate_steps == 2"):
        VL.train_one_epoch(model, [], opt, 0, "cpu", scheduler, loop_config(meta, accumulate_steps=2), _HFStep())
    with pytest.raises(NotImplementedError, match="VQA.py:53-57"):
        VL.train(model, [], [], opt, "cpu", scheduler, loop_config(meta, accumulate_steps=2), _HFStep(), None, ".", ".")


def test_fused_on_cpu_raises():
    from xfm_amd.model_generation import XFMForVQA
    qs, atts = torch.zeros(2, 4, 768), torch.ones(2, 4, dtype=torch.long)
    ids, a_atts = torch.zeros(3, 4, dtype=torch.long), torch.ones(3, 4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="fused=True"):
        XFMForVQA.rank_answer(None, qs, atts, ids, a_atts, 2, fused=True)
    import inspect
    for fn in (XFMForVQA.rank_answer, XFMForVQA.forward):
        assert inspect.signature(fn).parameters["fused"].default is False
    from xfm_amd.xbert import BertLMHeadModel
    from xfm_amd.xroberta import RobertaForCausalLM
    for cls in (RobertaForCausalLM, BertLMHeadModel):
        assert inspect.signature(cls.forward).parameters["encoder_batch_index"].default is None


def test_launcher_command_line_and_synthetic_loaders():
    import run as R
    a = R.parse(["--task", "vqa", "--dist", "gpu0", "--output_dir", "out/vqa", "--bs", "48"])
    cmd, nproc, vis, sa = R.task_command(a, 8)
    assert (nproc, vis) == (1, "0") and any(str(c).endswith("VQA.py") for c in cmd)
    assert sa[sa.index("--config") + 1].endswith("configs/VQA_synthetic.yaml")
    assert sa[sa.index("--bs") + 1] == 48 and sa[sa.index("--seed") + 1] == 42 and sa[sa.index("--output_dir") + 1] == "out/vqa"
    assert "--evaluate" not in sa and "--checkpoint" not in sa and "--epoch" not in sa
    a.evaluate, a.checkpoint = True, "ckpt.th"
    sa = R.task_command(a, 8)[3]
    assert "--evaluate" in sa and sa[sa.index("--checkpoint") + 1] == "ckpt.th"
    import VQA as script
    with pytest.raises(NotImplementedError, match="file-backed"):
        script.synthetic_loaders({"synthetic": False}, 0)
    with open(os.path.join(ROOT, "configs", "VQA_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["accumulate_steps"] == 1 and cfg["k_test"] == 128 and cfg["batch_size_test"] == 32 and cfg["start_eval"] < cfg["schedular"]["epochs"]
    cfg.update(image_res=32, batch_size_train=3, train_dataset_size=7, batch_size_test=4, test_dataset_size=8, answer_list_size=40)
    train_loader, test_loader = script.synthetic_loaders(cfg, seed=42)
    assert len(train_loader) == 3 and len(test_loader) == 2   # ceil(7 / 3) as VQA.py:219; 8 // 4
    image, (q_ids, q_atts), (a_ids, a_atts), weights, n = next(iter(train_loader))
    assert image.shape == (3, 3, 32, 32) and q_ids.shape == q_atts.shape == (3, 40) and a_ids.shape[0] == sum(n) == weights.numel()
    qids = [int(q) for _, _, qid in test_loader for q in qid]
    assert qids == list(range(8))
    ids, atts = test_loader.dataset.answer_input
    assert ids.shape == (40, 8) and len(test_loader.dataset.answer_list) == 40 and int(ids[:, 0].max()) == 0
    first = ids[:, 1].tolist()
    assert len(set(first)) < len(first)   # several candidates share a first token
    assert all(int(ids[i, int(atts[i].sum()) - 1]) == 2 for i in range(40))   # every row ends in </s>


def test_abi_and_new_symbols():
    """The two entry points of the answer ranking exist at ABI 14, and refuse bad arguments before anything is launched (host-only checks:
    the dummy non-NULL pointers are not read)."""
    from xfm_amd import _lib
    from xfm_amd import functional as Fx
    assert _lib.ABI_VERSION >= 14
    lib = _lib.load()
    assert lib.xfm_abi_version() == _lib.ABI_VERSION
    for name in ("xfm_answer_shortlist", "xfm_answer_rerank"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    with open(os.path.join(ROOT, "include", "xfm_hip.h")) as f:
        hdr = f.read()
    assert f"#define XFM_ANSWER_MAX_A {Fx.ANSWER_MAX_A}" in hdr and f"#define XFM_ANSWER_MAX_K {Fx.ANSWER_MAX_K}" in hdr
    assert Fx.ANSWER_MAX_A >= 8192 and Fx.ANSWER_MAX_K >= 256
    assert "ascending candidate index" in hdr.lower()
    assert Fx.answer_rank_ok(8192, 256) and Fx.answer_rank_ok(3128, 128) and Fx.answer_rank_ok(1, 1)
    assert not Fx.answer_rank_ok(Fx.ANSWER_MAX_A + 1, 8) and not Fx.answer_rank_ok(4096, Fx.ANSWER_MAX_K + 1) and not Fx.answer_rank_ok(4, 5)
    P = 0x10000
    for bad in (dict(k=0), dict(k=8), dict(A=Fx.ANSWER_MAX_A + 1), dict(A=4096, k=Fx.ANSWER_MAX_K + 1), dict(ld=9), dict(Q=0)):
        kw = dict(ld=10, Q=2, V=10, A=7, k=3)
        kw.update(bad)
        rc = lib.xfm_answer_shortlist(P, kw["ld"], kw["Q"], kw["V"], P, kw["A"], kw["k"], P, P, None)
        assert rc == -1 and b"answer_shortlist" in lib.xfm_last_error(), bad
    assert lib.xfm_answer_shortlist(None, 10, 2, 10, P, 7, 3, P, P, None) == -1
    for bad in (dict(k=0), dict(k=Fx.ANSWER_MAX_K + 1), dict(Q=0), dict(off=-1)):
        kw = dict(Q=2, k=3, off=0)
        kw.update(bad)
        rc = lib.xfm_answer_rerank(P, P, P, kw["Q"], kw["k"], P, P, P, kw["off"], None)
        assert rc == -1 and b"answer_rerank" in lib.xfm_last_error(), bad
    assert lib.xfm_answer_rerank(P, None, P, 2, 3, P, P, None, 0, None) == -1
