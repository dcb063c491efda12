"""The VQ-KD tokenizer and the token branch of the MIM loss on a real MI355X against tests/golden/vqkd_small.npz (the reference's own
modules, tools/oracle/gen_vqkd.py).

  features      the tokenizer's quantizer input per image against the reference's fp32 features: the module rule of test_hip_modules.py --
                rel-L2 <= max(tol, 1.3 x floor), 1 - cos <= max(1 - cos_tol, 1.7 x the floor's) with the reference's bf16-autocast floor.
  composition   the returned indices are the fp64 argmin over the tokenizer's OWN returned features (the rule of tests/vq_util.py), and the
                eval-mode EMA of cluster_size is (1 - decay) x their histogram.
  reference     every patch the feature error cannot flip (gap > 4 |delta| + the kernel's bound, delta measured here) carries the
                reference's index; at least 70 % of the patches must be such (the generator showed 87 % against 1.3 x the autocast error).
  MIM branch    get_mim_loss with the fixture's tokens in place of vqkd.get_codebook_indices: loss_mim to the pre-training fixtures' 3e-3,
                lm_head and vision-tower gradients through _check_grads with the floor.
  flag          XFM with use_vision_tokenizer constructs (the parent commit raises NotImplementedError); without the flag the state_dict
                keys are those of the reference fixture, with it they gain lm_head.* and the kept vqkd.* keys only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load, state_from_spec  # noqa: E402
from test_hip_modules import COS_TOL, FLOOR_COS, FLOOR_ERR, OUT_TOL, _check_grads, _pretrain_cfg  # noqa: E402
from vq_util import check_indices, decided_patches, unit64, vq_ref64, vqkd_images, vqkd_state  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402

TOKENIZER = "vqkd_encoder_base_decoder_3x768x12_clip"


@pytest.fixture(scope="module")
def tok_case():
    from xfm_amd.model_vqkd import vqkd_encoder_base_decoder_3x768x12_clip
    z, meta = load("vqkd_small")
    tok = vqkd_encoder_base_decoder_3x768x12_clip(pretrained=True, as_tokenzer=True, img_size=meta["image_res"], n_code=meta["n_code"],
                                                  code_dim=meta["code_dim"], encoder_depth=meta["encoder_depth"])
    sd = vqkd_state(meta["spec"])
    assert any(k.startswith("decoder.") for k in sd) and any(k.startswith("decode_task_layer.") for k in sd)
    tok.load_state_dict(sd, strict=True)   # decoder.* / decode_task_layer.* accepted, not kept
    tok.cuda().finalize()
    image = vqkd_images(meta).cuda()
    with torch.no_grad():
        feat = tok.encode_features(tok.pre_process(image))
    return z, meta, tok, image, feat, sd["quantize.embedding.weight"].float()


def test_tokenizer_features_against_the_reference(tok_case):
    z, meta, tok, image, feat, code = tok_case
    ref = torch.from_numpy(z["feat"]).double()
    assert feat.dtype == torch.float32 and tuple(feat.shape) == tuple(ref.shape) == (meta["B"], 196, meta["code_dim"])
    for b in range(meta["B"]):
        a, r = feat[b].double().cpu().reshape(-1), ref[b].reshape(-1)
        err, cos = float((a - r).norm() / r.norm()), float((a @ r) / (a.norm() * r.norm()))
        fe, fc = (float(v) for v in z["floor"][b])
        print(f"image {b}: rel-L2 {err:.4f} (floor {fe:.4f})  1 - cos {1 - cos:.2e} (floor {1 - fc:.2e})")
        assert err <= max(OUT_TOL, FLOOR_ERR * fe) and 1.0 - cos <= max(1.0 - COS_TOL, FLOOR_COS * (1.0 - fc)), (b, err, cos)


def test_tokens_are_the_argmin_of_the_returned_features(tok_case):
    z, meta, tok, image, feat, code = tok_case
    tok.quantize.cluster_size.zero_()
    idx = tok.get_codebook_indices(image)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (meta["B"], 196) and tok.get_number_of_tokens() == meta["n_code"]
    flat = feat.reshape(-1, meta["code_dim"]).cpu()
    und = check_indices(idx.reshape(-1), vq_ref64(flat, code), "tokens against the tokenizer's own features")
    print("undecided patches", und)
    want = (1.0 - tok.quantize.decay) * torch.bincount(idx.reshape(-1).cpu(), minlength=meta["n_code"]).double()
    assert float((tok.quantize.cluster_size.double().cpu() - want).abs().max()) <= 1e-5
    # encode() is the same pass with z_q and the loss on top (eval mode: the reference's arithmetic on the indices)
    zq, ind, loss = tok.encode(tok.pre_process(image))
    assert torch.equal(ind.view(idx.shape), idx) and tuple(zq.shape) == (meta["B"], meta["code_dim"], 14, 14)
    zn = torch.nn.functional.normalize(feat, dim=-1)
    picked = code.cuda()[idx]
    assert float((zq.permute(0, 2, 3, 1).reshape(picked.shape) - picked).abs().max()) <= 1e-6
    assert abs(float(loss) - float((picked - zn).pow(2).mean())) <= 1e-6
    assert not tok.training and all(not p.requires_grad for p in tok.parameters())
    tok.train()
    assert not tok.training, "the tokenizer stays in eval mode"


def test_tokens_against_the_reference_where_decided(tok_case):
    z, meta, tok, image, feat, code = tok_case
    idx = tok.get_codebook_indices(image).reshape(-1).cpu()
    ref_feat = torch.from_numpy(z["feat"]).reshape(-1, meta["code_dim"])
    delta = (unit64(feat.reshape(-1, meta["code_dim"]).cpu()) - unit64(ref_feat)).norm(dim=1)
    ref, decided = decided_patches(ref_feat, code, delta)
    ref_idx = torch.from_numpy(z["index"]).reshape(-1)
    share = float(decided.double().mean())
    print(f"decided {share:.3f}; equal overall {float((idx == ref_idx).double().mean()):.3f}; mean |delta| {float(delta.mean()):.4f}")
    assert torch.equal(ref_idx[decided], ref["index"][decided]), "the fixture's indices leave the fp64 restatement on decided patches"
    assert share >= 0.70, share
    assert torch.equal(idx[decided], ref_idx[decided]), (idx[decided] != ref_idx[decided]).nonzero().flatten()[:8].tolist()


def _mim_cfg(meta, flag=True):
    cfg = _pretrain_cfg(meta)
    if flag:
        cfg.update(use_vision_tokenizer=True, tokenizer_model=TOKENIZER, tokenizer_weight=None, codebook_size=meta["n_code"],
                   codebook_dim=meta["code_dim"], tokenizer_depth=meta["encoder_depth"])
    return cfg


def test_mim_loss_token_branch_against_the_reference():
    from xfm_amd.model_pretrain import XFM
    z, meta = load("vqkd_small")
    m = XFM(_mim_cfg(meta))
    sd = state_from_spec(meta["mim_spec"])
    sd.update({"vqkd." + k: v for k, v in vqkd_state(meta["spec"]).items()})
    m.load_state_dict(sd, strict=True)
    m.cuda().finalize().eval()
    tokens = torch.from_numpy(z["mim/tokens"]).cuda()
    m.vqkd.get_codebook_indices = lambda x, **kw: tokens
    Bm = meta["mim_B"]
    img = syn.pretrain_batch(Bm, seed=meta["mim_seed"])["image"].cuda()
    masks = torch.from_numpy(z["mim/ids_mask"])
    assert torch.equal(masks, syn.mim_block_mask(Bm, 14, 75, seed=meta["mim_seed"]).bool())
    emb, _, ids_mask = m.get_vision_embeds(img, do_mask=True, ids_mask=masks)
    loss = m.get_mim_loss(emb, img, ids_mask)
    ref = float(z["mim/loss_mim"])
    print(f"loss_mim {float(loss):.6f} reference {ref:.6f} (its bf16 autocast: {float(z['mim/floor_loss_mim']):.6f})")
    assert abs(float(loss) - ref) <= 3e-3 * max(abs(ref), 1.0)
    loss.backward()
    _check_grads(z, "mim/grad", m, min_rms=1e-6, floor="mim/floor")
    assert any(k.startswith("mim/grad/lm_head.") for k in z.files) and any(k.startswith("mim/grad/vision_encoder.") for k in z.files)
    for n, p in m.vqkd.named_parameters():
        assert not p.requires_grad and getattr(p, "_xfm_arena", None) is not m._arena, n
    for n, p in m.named_parameters():
        if n in set(meta["mim_unused"]):
            assert float(p._xfm_grad.abs().max()) == 0.0, f"{n} must receive no gradient"


def test_mim_step_runs_the_tokenizer_end_to_end():
    """forward_multimodal with the flag: the images themselves are the MIM target (model_pretrain.py:70-72), the tokenizer runs under
    no_grad, the loss is finite and its gradient reaches lm_head."""
    from xfm_amd.model_pretrain import XFM
    z, meta = load("vqkd_small")
    m = XFM(_mim_cfg(meta))
    sd = state_from_spec(meta["mim_spec"])
    sd.update({"vqkd." + k: v for k, v in vqkd_state(meta["spec"]).items()})
    m.load_state_dict(sd, strict=True)
    m.cuda().finalize().eval()
    Bm = meta["mim_B"]
    b = {k: v.cuda() for k, v in syn.pretrain_batch(Bm, seed=meta["mim_seed"]).items()}
    masks = torch.from_numpy(z["mim/ids_mask"])
    losses = m(b["image"], b["text_ids"], b["text_atts"], text_ids_masked=b["text_ids_masked"], masked_pos=b["masked_pos"],
               masked_ids=b["masked_ids"], ret_mim_loss=True, data_source="image", ids_mask=masks)
    own = m.vqkd.get_codebook_indices(b["image"])
    ref_tok = torch.from_numpy(z["mim/tokens"])
    print("tokens equal to the reference's:", float((own.cpu() == ref_tok).double().mean()))
    assert torch.isfinite(losses["loss_mim"]) and float(losses["loss_mim"]) > 0
    losses["loss_mim"].backward()
    assert float(m.lm_head.weight._xfm_grad.abs().max()) > 0


def test_flag_constructs_and_leaves_the_keys_alone():
    from xfm_amd.model_pretrain import XFM
    _, meta = load("vqkd_small")
    zp, meta_p = load("pretrain_small")
    plain = XFM(_mim_cfg(meta_p, flag=False))
    assert not plain.use_vision_tokenizer and not hasattr(plain, "vqkd") and not hasattr(plain, "lm_head")
    assert set(plain.state_dict().keys()) == set(meta_p["spec"].keys())
    with_tok = XFM(_mim_cfg(dict(meta_p, **{k: meta[k] for k in ("n_code", "code_dim", "encoder_depth")})))   # the parent commit raises here
    extra = set(with_tok.state_dict().keys()) - set(plain.state_dict().keys())
    kept = {"vqkd." + k for k in meta["spec"] if not k.startswith(("decoder.", "decode_task_layer."))}
    assert set(plain.state_dict().keys()) <= set(with_tok.state_dict().keys())
    assert extra == kept | {"lm_head.weight", "lm_head.bias"}, sorted(extra ^ (kept | {"lm_head.weight", "lm_head.bias"}))[:10]
    assert tuple(with_tok.lm_head.weight.shape) == (meta["n_code"], 768)
