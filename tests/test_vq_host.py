"""Host side of the VQ-KD tokenizer without a GPU: ABI 20 and the header text of xfm_vq_assign, its argument checks (nothing is launched:
the dummy non-NULL pointers are never dereferenced), the fp64 restatement of tests/vq_util.py against the reference's three ATen lines
(norm_ema_quantizer.py:153-162) on the CPU, the margins the GPU cases rely on, the state_dict keys of the tokenizer modules against the spec
of the reference's own module (tests/golden/vqkd_small.npz), and that fixture's own conditions."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from vq_util import GRID, U, WIDTHS, UNDECIDED_CAP, decided_patches, make_case, unit64, vq_ref64, vqkd_images, vqkd_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xfm_hip.h")
P16 = 4096   # a 16-byte aligned dummy pointer


def test_abi_20_header_and_binding_agree():
    from xfm_amd import _lib
    assert _lib.ABI_VERSION >= 20
    lib = _lib.load()
    assert lib.xfm_abi_version() == _lib.ABI_VERSION
    hdr = open(HEADER).read()
    assert f"#define XFM_ABI_VERSION {_lib.ABI_VERSION}" in hdr
    assert "xfm_vq_assign" in _lib.SIGNATURES and lib.xfm_vq_assign is not None and "int xfm_vq_assign(" in hdr
    for text in ("norm_ema_quantizer.py:153", "norm_ema_quantizer.py:158-162", "norm_ema_quantizer.py:168-172", "ABI 20",
                 "EQUAL SCORES GO TO THE LOWEST CODE INDEX", "NOT assumed to be unit-norm", "no workspace", "XFM_DETERMINISTIC"):
        assert text in hdr, text
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = plain[plain.index("int xfm_vq_assign("):]
    assert len(proto[:proto.index(")")].split(",")) == len(_lib.SIGNATURES["xfm_vq_assign"][1]) == 10


def test_vq_assign_argument_errors_launch_nothing():
    from xfm_amd import _lib
    lib = _lib.load()
    base = dict(z=P16, z_ld=32, M=64, K=32, code=P16, code_ld=32, n=100, index=P16, counts=None)

    def call(**over):
        k = dict(base)
        k.update(over)
        return lib.xfm_vq_assign(k["z"], k["z_ld"], k["M"], k["K"], k["code"], k["code_ld"], k["n"], k["index"], k["counts"], None)
    for over in (dict(z=None), dict(code=None), dict(index=None), dict(M=0), dict(M=-3), dict(n=0), dict(n=-1), dict(z_ld=28), dict(code_ld=31),
                 dict(z_ld=0), dict(z=P16 + 4), dict(z=P16 + 8), dict(code=P16 + 4), dict(code=P16 + 12), dict(z_ld=34), dict(code_ld=33),
                 dict(code_ld=38)):
        assert call(**over) == -1 and b"vq_assign" in lib.xfm_last_error(), over
    for over in (dict(K=0), dict(K=2), dict(K=30), dict(K=33), dict(K=68, z_ld=68, code_ld=68), dict(K=128, z_ld=128, code_ld=128), dict(K=-4)):
        assert call(**over) == -3 and b"vq_assign" in lib.xfm_last_error(), over


def test_python_wrapper_refuses_cpu_tensors():
    from xfm_amd import _lib
    from xfm_amd import functional as Fx
    with pytest.raises(_lib.XfmHipError):
        Fx.vq_assign(torch.zeros(4, 32), torch.zeros(8, 32))


def _aten_lines(z, weight):
    """norm_ema_quantizer.py:153-162 on a flattened z, as written there (fp32 ATen)."""
    z_flattened = F.normalize(z, p=2, dim=-1)
    d = z_flattened.pow(2).sum(dim=1, keepdim=True) + weight.pow(2).sum(dim=1) - 2 * torch.einsum('bd,nd->bn', z_flattened, weight)
    return torch.argmin(d, dim=1), d


@pytest.mark.parametrize("M,n_code,K,kind", [(M, n, 32, "unit") for M, n in GRID] + [w + ("unit",) for w in WIDTHS] + [(200, 257, 32, "norms")])
def test_fp64_restatement_against_the_reference_lines(M, n_code, K, kind):
    """The restatement is the reference's arithmetic: d agrees to ATen's own fp32 error -- the kernel's bound (another summation order of
    the same K-term sums) plus the three-term sum that ATen does form, 4 u (|zn|^2 + |e|^2 + 2 |zn||e|) -- and the argmin is equal on every
    row whose gap exceeds twice that.  The cap on undecided rows holds for every GPU case."""
    z, code, ref = make_case(M, n_code, K, kind)
    idx, d32 = _aten_lines(z, code)
    en = code.double().norm(dim=1)[None, :]
    slack = ref["B"][:, None] + 4 * U * (1.0 + en * en + 2.0 * en)
    assert bool(((d32.double() - ref["d"]).abs() <= slack).all())
    decided = ref["gap"] > 2.0 * slack.max(dim=1).values
    assert torch.equal(idx[decided], ref["index"][decided])
    assert int((ref["gap"] <= 2.0 * ref["B"]).sum()) <= UNDECIDED_CAP * M
    assert float(decided.double().mean()) >= 0.99 or M < 100


def test_restatement_rules_on_hand_cases():
    """Ties go to the first index, an all-zero row scores |e|^2, and |e|^2 decides between codes at the same angle."""
    code = torch.tensor([[2.0, 0, 0, 0], [0.5, 0, 0, 0], [0, 1.0, 0, 0], [0.5, 0, 0, 0]])
    z = torch.tensor([[3.0, 0, 0, 0], [0, 0, 0, 0], [0, 2.0, 0, 0]])
    ref = vq_ref64(z, code)
    # row 0: d = 1 + 4 - 4 = 1 against 1 + 0.25 - 1 = 0.25 (codes 1 and 3, tied: 1); row 1: |e|^2 -> 0.25 (code 1); row 2: code 2 (d = 0)
    assert ref["index"].tolist() == [1, 1, 2] and ref["d"][0].tolist() == [1.0, 0.25, 2.0, 0.25] and ref["gap"].tolist() == [0.0, 0.0, 1.25]
    assert _aten_lines(z, code)[0].tolist() == [1, 1, 2]


# ---------------------------------------------------------------------------------------------------------------- modules and fixture
def _tokenizer(meta):
    from xfm_amd.model_vqkd import vqkd_encoder_base_decoder_3x768x12_clip
    return vqkd_encoder_base_decoder_3x768x12_clip(pretrained=True, as_tokenzer=True, img_size=meta["image_res"], n_code=meta["n_code"],
                                                   code_dim=meta["code_dim"], encoder_depth=meta["encoder_depth"])


def test_tokenizer_state_dict_keys_match_the_reference():
    from golden_util import load
    from xfm_amd.norm_ema_quantizer import NormEMAVectorQuantizer
    _, meta = load("vqkd_small")
    spec = meta["spec"]
    tok = _tokenizer(meta)
    ours = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in tok.state_dict().items()}
    dropped = {k for k in spec if k.startswith(("decoder.", "decode_task_layer."))}
    assert dropped and {k: v for k, v in spec.items() if k not in dropped} == ours
    assert {k.split(".")[0] for k in ours} == {"encoder", "encode_task_layer", "quantize"}
    q = NormEMAVectorQuantizer(meta["n_code"], meta["code_dim"], beta=1.0, kmeans_init=True)
    assert {"quantize." + k: list(v.shape) for k, v in q.state_dict().items()} == {k: v[0] for k, v in spec.items() if k.startswith("quantize.")}
    assert set(q.state_dict()) == {"embedding.weight", "embedding.cluster_size", "embedding.embed_avg", "embedding.initted", "cluster_size"}
    assert all(not p.requires_grad for p in tok.parameters()) and not tok.training
    assert tok.load_state_dict(vqkd_state(spec), strict=True).missing_keys == []   # decoder.* / decode_task_layer.* accepted, not kept
    assert float((tok.quantize.embedding.weight.norm(dim=1) - 1).abs().max()) < 1e-6 and float(tok.quantize.embedding.initted) == 1.0


def test_quantizer_refuses_what_is_out_of_scope():
    from xfm_amd.model_vqkd import VQKD, vqkd_encoder_base_decoder_3x768x12_clip
    from xfm_amd.norm_ema_quantizer import NormEMAVectorQuantizer
    q = NormEMAVectorQuantizer(16, 8, beta=1.0)
    with pytest.raises(NotImplementedError, match="training"):
        q.train().assign(torch.zeros(4, 8))
    q = NormEMAVectorQuantizer(16, 8, beta=1.0, kmeans_init=True).eval()
    with pytest.raises(NotImplementedError, match="k-means"):
        q.assign(torch.zeros(4, 8))
    with pytest.raises(NotImplementedError):
        vqkd_encoder_base_decoder_3x768x12_clip(as_tokenzer=False)
    with pytest.raises(NotImplementedError, match="process_type"):
        VQKD(dict(img_size=224, patch_size=16, embed_dim=768, depth=1, num_heads=12), process_type="dall-e")


def test_pre_process_is_the_reference_rule_without_a_host_read():
    from golden_util import load
    _, meta = load("vqkd_small")
    tok = _tokenizer(dict(meta, encoder_depth=1))
    x = vqkd_images(meta)[:1]
    assert float(x.max()) <= 1.0
    assert torch.equal(tok.pre_process(x), x * 255. / 127.5 - 1.0)          # model_vqkd.py:129-131, the [0, 1] branch
    big = x * 3.0 + 0.5
    assert float(big.max()) > 1.0 and torch.equal(tok.pre_process(big), big / 127.5 - 1.0)
    tok.process_type = "imagenet_norm"
    mean, std = torch.tensor([0.485, 0.456, 0.406])[None, :, None, None], torch.tensor([0.229, 0.224, 0.225])[None, :, None, None]
    assert torch.equal(tok.pre_process(x), (x - mean) / std)


def test_fixture_conditions():
    """What tools/oracle/gen_vqkd.py asserted, again from the stored arrays: the reference's indices are the fp64 argmin of its features
    wherever the gap is clear of the fp32 bound, the stored gaps are those, at least 80 % of the patches are decided against 1.3 x the
    reference's own autocast error, no decided patch flipped under autocast, and the floor is the stored features'."""
    from golden_util import load
    z, meta = load("vqkd_small")
    B, C, n = meta["B"], meta["code_dim"], meta["n_code"]
    code = vqkd_state({k: v for k, v in meta["spec"].items() if k == "quantize.embedding.weight"})["quantize.embedding.weight"]
    assert tuple(code.shape) == (n, C) and z["feat"].shape == (B, 196, C) and z["index"].shape == (B, 196) and z["index"].max() < n
    f32, f16 = torch.from_numpy(z["feat"]).reshape(-1, C), torch.from_numpy(z["feat_bf16_autocast"]).reshape(-1, C)
    i32, i16 = torch.from_numpy(z["index"]).reshape(-1), torch.from_numpy(z["index_bf16_autocast"]).reshape(-1)
    delta = meta["delta_factor"] * (unit64(f16) - unit64(f32)).norm(dim=1)
    ref, decided = decided_patches(f32, code, delta)
    clear = ref["gap"] > 2.0 * ref["B"]
    assert torch.equal(i32[clear], ref["index"][clear]) and float(clear.double().mean()) > 0.99
    assert float((ref["gap"] - torch.from_numpy(z["gap"]).reshape(-1)).abs().max()) < 1e-12
    share = float(decided.double().mean())
    assert share >= meta["min_decided"] and abs(share - meta["decided_share"]) < 1e-9
    assert not bool((decided & (i16 != i32)).any())
    for b in range(B):
        a, r = torch.from_numpy(z["feat_bf16_autocast"][b]).double().reshape(-1), torch.from_numpy(z["feat"][b]).double().reshape(-1)
        assert abs(float((a - r).norm() / r.norm()) - float(z["floor"][b, 0])) < 1e-9
    assert z["mim/ids_mask"].shape == (meta["mim_B"], 196) and z["mim/ids_mask"].sum(1).tolist() == [75] * meta["mim_B"]
    assert z["mim/tokens"].shape == (meta["mim_B"], 196) and float(z["mim/loss_mim"]) > 0
    assert "mim/grad/lm_head.weight/probe" in z.files and "mim/floor/lm_head.weight" in z.files


def test_flag_constructs_the_tokenizer_and_the_token_head():
    """XFM with use_vision_tokenizer: the parent commit raises NotImplementedError here.  The tokenizer's parameters stay out of the
    model's arena and out of the optimizer's groups."""
    from golden_util import load
    from xfm_amd.model_pretrain import XFM
    from xfm_amd.pretrain_loop import optimizer_groups
    _, meta = load("vqkd_small")
    cfg = {"use_beit_v2": True, "image_res": 224, "patch_size": 16, "local_attn_depth": -1, "text_encoder": "roberta-base",
           "text_num_hidden_layers": 1, "text_fusion_start_at": 1, "fusion_num_hidden_layers": 1, "fusion_fusion_start_at": 0, "embed_dim": 256,
           "temp": 0.07, "learnable_temp": True, "max_temp": 0.5, "min_temp": 0.001, "vision_depth": 1}
    plain = XFM(dict(cfg))
    m = XFM(dict(cfg, use_vision_tokenizer=True, tokenizer_model="vqkd_encoder_base_decoder_3x768x12_clip", tokenizer_weight=None,
                 codebook_size=meta["n_code"], codebook_dim=meta["code_dim"], tokenizer_depth=1))
    assert m.use_vision_tokenizer and not m.vqkd.training and tuple(m.lm_head.weight.shape) == (meta["n_code"], 768)
    extra = set(m.state_dict()) - set(plain.state_dict())
    assert set(plain.state_dict()) <= set(m.state_dict()) and all(k.startswith(("vqkd.", "lm_head.")) for k in extra)
    m.train()
    assert m.training and not m.vqkd.training and not m.vqkd.quantize.training
    names = {n for g in optimizer_groups(m) for n in g}
    assert "lm_head.weight" in names and not any(n.startswith("vqkd.") for n in names)
    m.finalize(torch.device("cpu"))
    own = {id(p) for p in m._arena.params}
    assert id(m.lm_head.weight) in own and not any(id(p) in own for p in m.vqkd.parameters())
    with pytest.raises(ValueError):
        XFM(dict(cfg, use_vision_tokenizer=True, tokenizer_model="other", codebook_size=16, codebook_dim=8))
