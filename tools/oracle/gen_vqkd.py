"""Generate tests/golden/vqkd_small.npz from the REAL reference (behind ref_shim, as gen_golden.py does).

Run in the build container only:   python tools/oracle/gen_vqkd.py

ref_shim.install() stubs `models.model_vqkd` (the flag was never set).  Here the stub is replaced by the real module: the reference's own
models/vqkd_vit.py, models/norm_ema_quantizer.py and models/model_vqkd.py are imported as they stand, behind the timm stubs of ref_shim and
a stub of `models.vqkd_teacher` (CLIP / DINO teachers: only needed to train the tokenizer; `as_tokenzer=True` builds none).  The real
constructor function is then bound into models.xfm, which had imported the stub.  install() stays as it is for the other generators.

Tokenizer part.  vqkd_encoder_base_decoder_3x768x12_clip(as_tokenzer=True) with a 2-block encoder (get_model_default_params re-bound for
the construction, as gen_golden.shallow_vit does for the vision tower; the 3 x 768 x 12 decoder is built because the constructor builds
it), n_code / code_dim from META.  Weights: syn.formula_state_dict on the module's own state_dict, the codebook rows l2-normalised in fp32
afterwards and `initted` set (tests/vq_util.vqkd_state repeats that), saved to a temporary .pth and loaded through the reference's own
as_tokenzer path.  B = 3 formula images in [0, 1).  Stored: the fp32 reference's pre-normalisation features [3, 196, code_dim] (the input
of the quantizer), its indices, per patch its top-2 gap in d (fp64 restatement on those features -- the reference's own argmin must and
does agree wherever the gap exceeds the fp32 bound), the same features and indices under torch.autocast("cpu", bfloat16), and per image
[rel-L2, cosine] of the autocast features against the fp32 ones (the floor, as amp_floor is for gradients).

Asserted here: with delta = 1.3 x the autocast error of a patch's normalised feature, a patch is decided when its gap exceeds 4 |delta| plus
the kernel's fp32 bound; at least 80 % of the patches are decided.  The reference's autocast moves a normalised feature by about 1.1 %, so
4 |delta| is about 0.056 -- the MEDIAN top-2 gap of 1024 random unit codes in 32 dimensions, which leaves 52 % decided.  Fewer codes
alone do not help at 32 dimensions (256: 60 %, 64: 68 %, 16: 71 %); fewer dimensions spread the codes' scores: (n_code, code_dim) =
(32, 8) gives 81 %, (16, 8) gives 87 %, which is what META holds (the kernel's own tests cover the large shapes).

MIM branch.  The reference XFM (models/model_pretrain.py) with use_vision_tokenizer, 2 vision blocks + 2 text + 2 fusion layers, formula
weights, its vqkd loaded from the same checkpoint; a fixed ids_mask; get_vision_embeds(do_mask) -> get_mim_loss(image_embeds_masked, image,
ids_mask) as model_pretrain.py:69-72 calls it.  Stored: ids_mask, the reference's token indices, loss_mim, the gradients of lm_head.* and
of the vision tower (probes), and their bf16-autocast floor (the tokens held at their fp32 values, so the floor is that of the head and the
tower, not of a flipped token)."""
import importlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))

import gen_golden as G  # noqa: E402
import ref_shim  # noqa: E402
from xfm_amd import synthetic as syn  # noqa: E402

META = {"B": 3, "image_res": 224, "image_seed": 77, "encoder_depth": 2, "n_code": 16, "code_dim": 8, "delta_factor": 1.3,
        "min_decided": 0.8, "mim_B": 2, "mim_seed": 1234, "text_layers": 2, "fusion_layers": 2}


def reference_vqkd():
    """The real models.model_vqkd in place of ref_shim's stub."""
    ref_shim.install()
    ref_shim._stub("models.vqkd_teacher", clip=None, get_dino_vit_base=None)
    sys.modules.pop("models.model_vqkd", None)
    mod = importlib.import_module("models.model_vqkd")
    import models.xfm as X
    X.vqkd_encoder_base_decoder_3x768x12_clip = mod.vqkd_encoder_base_decoder_3x768x12_clip
    defaults = mod.get_model_default_params
    mod.get_model_default_params = lambda: dict(defaults(), depth=META["encoder_depth"])   # (the decoder's depth is set after this call)
    return mod


def tokens_of(tok, image):
    """get_codebook_indices as the reference runs it, with the quantizer's input captured -> (indices [B, N], features fp32 [B, N, C])."""
    got = {}
    h = tok.encode_task_layer.register_forward_hook(lambda mod, inp, out: got.__setitem__("f", out.detach().float().clone()))
    try:
        with torch.no_grad():
            idx = tok.get_codebook_indices(image)
    finally:
        h.remove()
    return idx, got["f"]


def main():
    import vq_util as V
    mod = reference_vqkd()
    L = dict(META)
    torch.manual_seed(0)
    # ---- the checkpoint: formula weights on the reference module's own state_dict
    enc, dec = mod.get_model_default_params(), mod.get_model_default_params()
    enc.update(img_size=L["image_res"], num_classes=0)
    dec.update(img_size=L["image_res"] // 16, patch_size=1, in_chans=L["code_dim"], num_classes=0, depth=3)
    blank = mod.VQKD(enc, dec, L["n_code"], L["code_dim"], teacher_model_type='None', decoder_out_dim=512)
    spec = G.spec_of(blank)
    sd = V.vqkd_state(spec)
    ckpt = os.path.join(tempfile.mkdtemp(prefix="xfm_vqkd_"), "tokenizer.pth")
    torch.save({"model": sd}, ckpt)
    tok = mod.vqkd_encoder_base_decoder_3x768x12_clip(pretrained=True, pretrained_weight=ckpt, as_tokenzer=True, img_size=L["image_res"],
                                                      n_code=L["n_code"], code_dim=L["code_dim"]).eval()
    assert len(tok.encoder.blocks) == L["encoder_depth"] and len(tok.decoder.blocks) == 3
    image = V.vqkd_images(L)
    idx32, f32 = tokens_of(tok, image)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        idx16, f16 = tokens_of(tok, image)
    B, N, C = f32.shape
    code = sd["quantize.embedding.weight"]
    flat32, flat16 = f32.reshape(-1, C), f16.reshape(-1, C)
    delta = L["delta_factor"] * (V.unit64(flat16) - V.unit64(flat32)).norm(dim=1)
    ref, decided = V.decided_patches(flat32, code, delta)
    clear = ref["gap"] > 2.0 * ref["B"]
    assert torch.equal(idx32.reshape(-1)[clear], ref["index"][clear]), "the reference's argmin leaves the fp64 restatement"
    share = float(decided.double().mean())
    flips = int((idx16.reshape(-1) != idx32.reshape(-1)).sum())
    assert not bool((decided & (idx16.reshape(-1) != idx32.reshape(-1))).any()), "a decided patch flipped under autocast"
    floor = []
    for b in range(B):
        a, r = f16[b].double().reshape(-1), f32[b].double().reshape(-1)
        floor.append([float((a - r).norm() / r.norm()), float((a @ r) / (a.norm() * r.norm()))])
    print(f"decided {share:.3f} of {B * N} patches; autocast flips {flips}; distinct codes {len(set(idx32.reshape(-1).tolist()))}; "
          f"floor {floor}", flush=True)
    assert share >= L["min_decided"], share
    out = {"feat": f32.numpy(), "index": idx32.numpy(), "gap": ref["gap"].reshape(B, N).numpy(), "feat_bf16_autocast": f16.numpy(),
           "index_bf16_autocast": idx16.numpy(), "floor": np.asarray(floor)}
    L["decided_share"], L["autocast_flips"] = share, flips

    # ---- the MIM branch of the pre-training model
    from models.model_pretrain import XFM
    ref_shim.init_single_process_group()
    cfg = ref_shim.pretrain_config(text_layers=L["text_layers"], fusion_layers=L["fusion_layers"],
                                   overrides={"use_vision_tokenizer": True, "tokenizer_model": "vqkd_encoder_base_decoder_3x768x12_clip",
                                              "tokenizer_weight": ckpt, "codebook_size": L["n_code"], "codebook_dim": L["code_dim"]})
    with G.shallow_vit():
        m = XFM(cfg, load_vision_params=False, load_text_params=False)
    full = {k: v for k, v in m.state_dict().items() if not k.startswith("vqkd.")}
    m.load_state_dict(dict(syn.formula_state_dict(full), **{"vqkd." + k: v for k, v in sd.items()}), strict=True)
    m.eval()
    Bm = L["mim_B"]
    img = syn.pretrain_batch(Bm, seed=L["mim_seed"])["image"]
    masks = syn.mim_block_mask(Bm, 14, 75, seed=L["mim_seed"])
    with torch.no_grad():
        tokens = m.vqkd.get_codebook_indices(img)
    m.vqkd.get_codebook_indices = lambda x, **kw: tokens   # (held for the autocast pass: the floor is the head's and the tower's)

    def loss_fn():
        m.vision_encoder.generator = G.FixedMasks(masks, 14)
        emb, _, ids_mask = m.get_vision_embeds(img, do_mask=True)
        assert torch.equal(ids_mask.cpu().bool(), masks.bool())
        return m.get_mim_loss(emb, img, ids_mask)

    loss = loss_fn()
    loss.backward()
    out["mim/ids_mask"], out["mim/tokens"], out["mim/loss_mim"] = masks.numpy().astype(bool), tokens.numpy(), np.asarray(float(loss))
    G.grads_of(m, out, prefix="mim/grad")
    unused = [n for n, p in m.named_parameters() if p.grad is None and not n.startswith("vqkd.")]
    l16 = G.amp_floor(m, loss_fn, out, prefix="mim/floor")
    out["mim/floor_loss_mim"] = np.asarray(l16)
    print("loss_mim", float(loss), "under autocast", l16, flush=True)
    mim_spec = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in full.items()}   # (vqkd.* is `spec` under the prefix)
    meta = dict(L, spec=spec, mim_spec=mim_spec, mim_unused=unused, vit_depth=G.SHALLOW)
    G.save("vqkd_small", out, meta)
    for f in os.listdir(G.OUT):
        if f.startswith("vqkd_small"):
            assert os.path.getsize(os.path.join(G.OUT, f)) < 1024 * 1024, f
    print(json.dumps({k: v for k, v in meta.items() if "spec" not in k and k != "mim_unused"}))


if __name__ == "__main__":
    main()
