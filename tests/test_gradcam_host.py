"""Host side of the Grad-CAM grounding feature without a GPU: ABI 19 and the argument checks of xfm_xattn_gradcam / xfm_cam_box_rank (nothing
is launched: the dummy non-NULL pointers are never dereferenced), the torch restatement of cam / P / dP against the fp64 definition, the
host form of the box ranking against the restatement of tests/gradcam_util.py and a hand-worked bicubic box sum, and the margins that the
GPU tests rely on (asserted for every ref, here too, so that a GPU run never meets an undecided case)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gradcam_util import (BOX_P, MODES, SHAPES, box_rank_case, box_rank_expect, gradcam_ref, interp_score_bound, interp_scores,
                          kernel_score_bound, make_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xfm_hip.h")
P16 = 4096   # a 16-byte aligned dummy pointer


def test_abi_19_header_and_binding_agree():
    from xfm_amd import _lib
    assert _lib.ABI_VERSION >= 19
    lib = _lib.load()
    assert lib.xfm_abi_version() == _lib.ABI_VERSION
    hdr = open(HEADER).read()
    assert f"#define XFM_ABI_VERSION {_lib.ABI_VERSION}" in hdr
    for sym in ("xfm_xattn_gradcam", "xfm_cam_box_rank"):
        assert sym in _lib.SIGNATURES and getattr(lib, sym) is not None and f"int {sym}(" in hdr
    assert "Grounding.py:109-115" in hdr and "utils.py:183-216" in hdr and "counted as WRONG" in hdr
    assert f"#define XFM_CAM_MAX_P {_lib.CAM_MAX_P}" in hdr and f"#define XFM_CAM_MAX_DETS {_lib.CAM_MAX_DETS}" in hdr
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    end = plain.index("} xfm_gradcam_args;")
    body = plain[plain.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    fields = [re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip())[0] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert fields == [f[0] for f in _lib.GradcamArgs._fields_]
    proto = plain[plain.index("int xfm_cam_box_rank("):]
    assert len(proto[:proto.index(")")].split(",")) == len(_lib.SIGNATURES["xfm_cam_box_rank"][1])


def _gargs(_lib, **over):
    kw = dict(q=P16, q_rs=128, dout=P16, do_rs=128, k=P16, k_rs=256, v=P16, v_rs=256, lse=P16, stat_ld=64, q_start=0, q_len=0, kv_src=0,
              n_src=2, B=2, H=2, Sq=64, Sk=37, scale=0.125, t_div=64, cam=P16, p_out=0, dp_out=0)
    kw.update(over)
    return _lib.GradcamArgs(**kw)


def test_xattn_gradcam_argument_errors_launch_nothing():
    from xfm_amd import _lib
    lib = _lib.load()
    assert lib.xfm_xattn_gradcam(None, None) == -1
    for over in (dict(cam=0), dict(q=0), dict(dout=0), dict(k=0), dict(v=0), dict(lse=0), dict(B=0), dict(B=65536), dict(H=0), dict(Sq=0),
                 dict(Sk=1), dict(q_rs=64), dict(do_rs=120), dict(k_rs=132), dict(v_rs=127), dict(q=P16 + 8), dict(dout=P16 + 2), dict(k=P16 + 4),
                 dict(v=P16 + 8), dict(lse=P16 + 4), dict(stat_ld=60), dict(stat_ld=66), dict(q_start=P16), dict(n_src=0), dict(t_div=0),
                 dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan"))):
        rc = lib.xfm_xattn_gradcam(ctypes.byref(_gargs(_lib, **over)), None)
        assert rc == -1 and b"xattn_gradcam" in lib.xfm_last_error(), over
    for over in (dict(Sq=65, stat_ld=68), dict(Sq=128, stat_ld=128)):
        rc = lib.xfm_xattn_gradcam(ctypes.byref(_gargs(_lib, **over)), None)
        assert rc == -3 and b"xattn_gradcam" in lib.xfm_last_error(), over


def test_cam_box_rank_argument_errors_launch_nothing():
    from xfm_amd import _lib
    lib = _lib.load()
    base = dict(cam=P16, p=6, hw=P16, det=P16, st=P16, md=4, rb=P16, sp=P16, n=3, alpha=0.5, out=P16, off=0, counts=P16)

    def call(**over):
        k = dict(base)
        k.update(over)
        return lib.xfm_cam_box_rank(k["cam"], k["p"], k["hw"], k["det"], k["st"], k["md"], k["rb"], k["sp"], k["n"], k["alpha"], k["out"], k["off"],
                                    k["counts"], None)
    for over in (dict(cam=None), dict(hw=None), dict(det=None), dict(st=None), dict(rb=None), dict(sp=None), dict(out=None), dict(counts=None),
                 dict(n=0), dict(n=-2), dict(p=0), dict(off=-1), dict(md=-1), dict(alpha=float("nan")), dict(alpha=float("inf"))):
        assert call(**over) == -1 and b"cam_box_rank" in lib.xfm_last_error(), over
    for over in (dict(p=_lib.CAM_MAX_P + 1), dict(md=_lib.CAM_MAX_DETS + 1)):
        assert call(**over) == -3 and b"cam_box_rank" in lib.xfm_last_error(), over


def test_python_wrappers_refuse_cpu_tensors():
    from xfm_amd import _lib
    from xfm_amd import functional as Fx
    z = torch.zeros(64, 128, dtype=torch.bfloat16)
    with pytest.raises(_lib.XfmHipError):
        Fx.xattn_gradcam(z, z, z, z, torch.zeros(1, 2, 64), 1, 2, 64, 64, 0.125, 64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["s37", "s197"])
def test_torch_restatement_matches_the_fp64_definition(name, mode):
    """gradcam_torch (fp32 ATen, the fallback for CPU tensors and Sq > 64) against the fp64 definition.  The fp32 matmuls of ATen are not
    the kernel's: held to 4 x the kernel's derived bound plus 2e-6 of the largest value (fp32 dot products of 64 terms in any order)."""
    from xfm_amd import gradcam as G
    c = make_case(name, mode)
    ref = gradcam_ref(c)
    B, H, Sq, Sk, D = c["B"], c["H"], c["Sq"], c["Sk"], c["D"]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)   # noqa: E731
    cam, P, dP = G.gradcam_torch(c["q"], c["dout"], c["kv"][:, :D], c["kv"][:, D:], ref["lse32"].nan_to_num(0.0), B, H, Sq, Sk, 0.125, c["t_div"],
                                 q_start=i32(c["start"]) if mode == "packed" else None, q_len=i32(c["lens"]) if mode != "dense" else None,
                                 kv_src=None if c["kv_src"] is None else i32(c["kv_src"]))
    for got, want, bound in ((P, ref["P"], ref["bP"]), (dP, ref["dP"], ref["bdP"]), (cam, ref["cam"], ref["bcam"])):
        assert got.dtype == torch.float32 and got.shape == want.shape
        err = (got.double() - want).abs()
        assert bool((err <= 4 * bound + 2e-6 * float(want.abs().max())).all()), float((err - 4 * bound).max())
    for b, n in enumerate(c["lens"]):
        if n < Sq:
            assert float(P[b, :, n:].abs().max()) == 0.0 and float(dP[b, :, n:].abs().max()) == 0.0
    # attention_gradcam on CPU tensors takes the same restatement
    cam2, P2, dP2 = G.attention_gradcam(c["q"], c["dout"], c["kv"][:, :D], c["kv"][:, D:], ref["lse32"].nan_to_num(0.0), B, H, Sq, Sk, 0.125, c["t_div"],
                                        q_pack=(i32(c["start"]), i32(c["lens"])) if mode == "packed" else None,
                                        q_len=i32(c["lens"]) if mode == "dense_len" else None,
                                        kv_src=None if c["kv_src"] is None else i32(c["kv_src"]), p_out=True)
    assert torch.equal(cam2, cam) and torch.equal(P2, P) and dP2 is None


def test_hand_worked_bicubic_box_sum():
    """p = 2 onto a 4 x 4 image: source coordinates -0.25, 0.25, 0.75, 1.25; every tap weight is a dyadic fraction, exact in fp32:
    cc1(0.25) = 0.87890625, cc1(0.75) = 0.26171875, cc2(1.25) = -0.10546875, cc2(1.75) = -0.03515625.  After clamping the tap indices the
    four output rows weigh the inputs (1.10546875, -0.10546875), (0.7734375, 0.2265625), (0.2265625, 0.7734375), (-0.10546875, 1.10546875).
    Box (x, y, w, h) = (0, 1, 2, 2): rows 1:3 give a = (1, 1), columns 0:2 give b = (1.87890625, 0.12109375);
    cam = [[1, 2], [3, 4]]: a^T cam b = 2.12109375 + 6.12109375 = 8.2421875, area^0.5 = 2: score 4.12109375."""
    from xfm_amd import gradcam as G
    idx, w = G.cubic_tap_weights(4, 2)
    rows = np.zeros((4, 2))
    for y in range(4):
        for j in range(4):
            rows[y, idx[y, j]] += float(w[y, j])
    assert np.array_equal(rows, np.array([[1.10546875, -0.10546875], [0.7734375, 0.2265625], [0.2265625, 0.7734375], [-0.10546875, 1.10546875]]))
    cam = np.array([[[1.0, 2.0], [3.0, 4.0]]], dtype=np.float32)
    dets = [np.array([[0.0, 0.0, 1.0, 1.0], [0.0, 1.0, 2.0, 2.0], [0.0, 1.0, 2.0, 2.0], [4.0, 0.0, 2.0, 2.0]])]
    out, counts = G.cam_box_rank_host(cam, np.array([[4, 4]]), dets, np.array([[0.0, 1.0, 2.0, 3.0]]), np.array([1]), 0.5)
    # box 0 = the pixel (0, 0): about 0.68; box 1 wins, its twin (box 2) does not replace it; box 3's slice is empty
    assert out[0, 0] == 1.0 and out[0, 1] == 4.12109375
    assert out[0, 2] == pytest.approx(4.0 / 6.0, abs=1e-15) and counts.tolist() == [[0, 0], [1, 1], [0, 0]]
    si = interp_scores(cam[0], (4, 4), dets[0], 0.5)
    assert abs(si[1] - 4.12109375) <= 1e-6 and si[3] == 0.0


@pytest.mark.parametrize("p", BOX_P)
def test_host_box_rank_reproduces_the_restatement(p):
    """cam_box_rank_host (the CPU form of grounding_eval) against the restatement: indices, IoUs and counts exactly, scores to the fp64
    summation bound; the margins that make the indices decidable hold for every ref; F.interpolate + the reference's loop agree."""
    from xfm_amd import gradcam as G
    case = box_rank_case(p)
    want = box_rank_expect(case, lambda m, hw, pp: max(kernel_score_bound(m, hw, pp), interp_score_bound(m)))
    out, counts = G.cam_box_rank_host(case["cam"], case["hw"], case["dets"], case["ref_box"], case["split"], case["alpha"])
    want_counts = np.zeros((3, 2), dtype=np.int64)
    for i, (sc, mg, pick, best, iou) in enumerate(want):
        assert int(out[i, 0]) == pick and out[i, 2] == iou
        assert abs(out[i, 1] - best) <= (kernel_score_bound(mg[pick], case["hw"][i], p) if pick >= 0 else 0.0)
        want_counts[case["split"][i], 1] += 1
        want_counts[case["split"][i], 0] += int(pick >= 0 and iou >= 0.5)
    assert np.array_equal(counts, want_counts)
    assert want[4][2] == -1 and want[3][2] == 1
    i = 0   # the small image: the reference's own recipe on the CPU (the 480 x 640 one runs in the GPU test)
    si = interp_scores(case["cam"][i], case["hw"][i], case["dets"][i], case["alpha"])
    for d in range(len(si)):
        assert abs(si[d] - want[i][0][d]) <= interp_score_bound(want[i][1][d])


def test_grounding_eval_on_cpu_tensors():
    """grounding_eval's CPU path: the accuracy dict of utils.py:218 from the host form; negative coordinates and a wrong count are refused."""
    from types import SimpleNamespace as NS
    from xfm_amd import gradcam as G
    case = box_rank_case(6)
    refs = NS(ref_box=case["ref_box"], ref_size=np.stack([case["hw"][:, 1], case["hw"][:, 0]], axis=1), ref_split=case["split"])
    acc, rows = G.grounding_eval(torch.from_numpy(case["cam"]), refs, case["dets"], alpha=0.5, return_rows=True)
    want = box_rank_expect(case, lambda m, hw, pp: interp_score_bound(m))
    assert [int(r[0]) for r in rows] == [w[2] for w in want]
    hits = {s: [int(w[2] >= 0 and w[4] >= 0.5) for w, sp in zip(want, case["split"]) if sp == s] for s in range(3)}
    assert acc == {"val_d": sum(hits[0]) / len(hits[0]), "testA_d": sum(hits[1]) / len(hits[1]), "testB_d": sum(hits[2]) / len(hits[2])}
    bad = [d.copy() for d in case["dets"]]
    bad[0][0, 0] = -1.0
    with pytest.raises(ValueError):
        G.grounding_eval(torch.from_numpy(case["cam"]), refs, bad)
    with pytest.raises(ValueError):
        G.grounding_eval(torch.from_numpy(case["cam"]), refs, case["dets"][:3])


# ---------------------------------------------------------------------------------------------------------------- the fixture
def _oracle_gradcam():
    """The fixture's batch on the CPU oracle path (oracle/xfm_oracle.py: fp32 ATen), the cross-attention of fusion layer block_num taken
    apart into (q, dO, k, v, lse) the way the HIP layer holds them, and the torch restatement of the kernel on those."""
    import math

    from golden_util import load, state_from_spec
    from oracle import xfm_oracle as O
    from xfm_amd import gradcam as G
    from xfm_amd import synthetic as syn
    z, meta = load("gradcam_small")
    Pm = state_from_spec(meta["spec"])
    image = syn.grounding_eval_batch(meta["B"], seed=meta["batch_seed"], image_res=meta["image_res"], max_tokens=meta["max_tokens"],
                                     min_len=meta["min_len"])[0]
    ids, atts = torch.from_numpy(z["text_ids"]), torch.from_numpy(z["text_atts"])
    blk, L, heads = meta["block_num"], meta["fusion_layers"], 12
    with torch.no_grad():
        enc = O.beit_forward(Pm, "vision_encoder.", image, depth=meta["vit_depth"])
        pre = "fusion_encoder.roberta."
        x = O.roberta_embeddings(Pm, pre + "embeddings.", ids)
        add_mask = O.extended_attention_mask(atts)
        for i in range(blk):
            x = O.roberta_layer(Pm, f"{pre}encoder.layer.{i}.", x, add_mask, enc, None, True)
        lp = f"{pre}encoder.layer.{blk}."
        y1 = O.roberta_attention(Pm, lp + "attention.", x, add_mask)
        B, T, C = y1.shape
        N, d = enc.shape[1], C // heads
        q = O._lin(Pm, lp + "crossattention.self.query", y1)
        k, v = O._lin(Pm, lp + "crossattention.self.key", enc), O._lin(Pm, lp + "crossattention.self.value", enc)
        qh, kh, vh = (t.view(B, -1, heads, d).permute(0, 2, 1, 3) for t in (q, k, v))
        s = (qh / math.sqrt(d)) @ kh.transpose(-1, -2)
        lse = torch.logsumexp(s, dim=-1)
        ctx = (s.softmax(dim=-1) @ vh).permute(0, 2, 1, 3).reshape(B, T, C)
    ctx.requires_grad_(True)
    y = O._ln(Pm, lp + "crossattention.output.LayerNorm", O._lin(Pm, lp + "crossattention.output.dense", ctx) + y1, 1e-5)
    h = O.gelu_erf(O._lin(Pm, lp + "intermediate.dense", y))
    x = O._ln(Pm, lp + "output.LayerNorm", O._lin(Pm, lp + "output.dense", h) + y, 1e-5)
    for i in range(blk + 1, L):
        x = O.roberta_layer(Pm, f"{pre}encoder.layer.{i}.", x, add_mask, enc, None, True)
    O.build_mlp_forward(Pm, "itm_head.", x[:, 0, :])[:, 1].sum().backward()
    lens = atts.sum(1).to(torch.int32)
    cam, P, dP = G.gradcam_torch(q.reshape(B * T, C), ctx.grad.reshape(B * T, C), k.reshape(B * N, C), v.reshape(B * N, C), lse, B, heads, T, N,
                                 1.0 / math.sqrt(d), T, q_len=lens)
    return z, meta, cam, P, dP


def test_torch_restatement_on_the_oracle_path_matches_the_fixture():
    """cam, P and dP against the reference's values: the oracle's standing bound, 2e-5 absolute + 2e-4 of the reference's rms."""
    z, meta, cam, P, dP = _oracle_gradcam()
    p = meta["image_res"] // meta["patch"]
    for name, got, want in (("cam", cam.view(-1, p, p), z["cam"]), ("P", P, z["P"]), ("dP", dP, z["dP"])):
        want = torch.from_numpy(want).double()
        assert tuple(got.shape) == tuple(want.shape), name
        rms = float(want.pow(2).mean().sqrt())
        err = float((got.double() - want).abs().max())
        assert err <= 2e-5 + 2e-4 * rms, (name, err, rms)
    for b, n in enumerate(meta["lens"]):
        assert float(P[b, :, n:].abs().sum()) == 0.0 and float(dP[b, :, n:].abs().sum()) == 0.0


def test_cpu_grounding_eval_reproduces_the_fixture_exactly():
    """Indices, IoUs and accuracies of the reference's own grounding_eval, from the fixture's cams on the CPU; and the margins the
    generator asserted (winner >= 1.3 x runner-up, every IoU 0.05 away from 0.5, a positive score for every ref)."""
    from types import SimpleNamespace as NS

    from golden_util import load
    from xfm_amd import gradcam as G
    z, meta = load("gradcam_small")
    B = meta["B"]
    start = np.concatenate([[0], np.cumsum(z["det_count"])])
    dets = [z["dets"][start[k]:start[k + 1]] for k in range(B)]
    assert all(3 <= len(d) <= 6 for d in dets) and sorted(meta["lens"])[0] == 3
    refs = NS(ref_box=z["ref_box"], ref_size=z["ref_size"], ref_split=z["ref_split"])
    acc, rows = G.grounding_eval(torch.from_numpy(z["cam"]), refs, dets, alpha=meta["alpha"], return_rows=True)
    assert [int(v) for v in rows[:, 0]] == z["chosen"].tolist()
    assert np.array_equal(rows[:, 2], z["iou"]) and np.array_equal(rows[:, 1], z["score"])
    assert acc == meta["acc"]
    hw = np.stack([z["ref_size"][:, 1], z["ref_size"][:, 0]], axis=1).astype(np.int64)
    for k in range(B):
        sc = np.array([G.cam_box_rank_host(z["cam"][k:k + 1], hw[k:k + 1], [d[None]], np.zeros((1, 4)), [0], meta["alpha"])[0][0, 1] for d in dets[k]])
        top = np.sort(sc)[::-1]
        assert top[0] > 0 and top[0] >= meta["win_ratio"] * top[1] and abs(z["iou"][k] - 0.5) >= meta["iou_margin"]
    # the same cams under the reference's bf16 autocast choose the same boxes: the margin is one the 16-bit towers cannot flip
    acc16, rows16 = G.grounding_eval(torch.from_numpy(z["cam_bf16_autocast"]), refs, dets, alpha=meta["alpha"], return_rows=True)
    assert [int(v) for v in rows16[:, 0]] == z["chosen"].tolist() and acc16 == acc


def test_config_and_script_parse():
    import importlib
    import yaml
    with open(os.path.join(ROOT, "configs", "Grounding_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["synthetic"] is True and cfg["image_res"] == 384 and cfg["patch_size"] == 16 and cfg["block_num"] == 8
    assert cfg["fusion_num_hidden_layers"] == 12 and cfg["batch_size"] == 32 and 0 <= cfg["block_num"] < cfg["fusion_num_hidden_layers"]
    script = importlib.import_module("Grounding")
    a = script.parse_args(["--evaluate", "--block_num", "3"])
    assert a.evaluate and a.block_num == 3 and a.gradcam_mode == "itm" and a.config.endswith("configs/Grounding_synthetic.yaml")
    with pytest.raises(NotImplementedError, match="--evaluate"):
        script.main(script.parse_args([]), cfg)
    with pytest.raises(NotImplementedError, match="itc"):
        script.main(script.parse_args(["--evaluate", "--gradcam_mode", "itc"]), cfg)
    with pytest.raises(NotImplementedError, match="synthetic"):
        script.synthetic_loader(dict(cfg, synthetic=False), 1)
    from xfm_amd import synthetic as syn
    refs = syn.grounding_refs(6, seed=9)
    dets = syn.grounding_dets(refs, seed=9)
    assert len(dets) == 6 and all(d.dtype == np.float64 and d.shape[1] == 4 and 3 <= len(d) <= 8 and (d >= 0).all() for d in dets)
    for r, d in enumerate(dets):
        W, H = refs.ref_size[r].tolist()
        assert (d[:, 0] < W).all() and (d[:, 1] < H).all() and (d[:, 2:] > 0).all()


def test_module_contract_defaults():
    """save_attention is False by default on every cross-attention of both tower flavours; the getters start empty."""
    from xfm_amd.xbert import BertConfig, BertModel
    from xfm_amd.xroberta import RobertaSelfAttention
    m = BertModel(BertConfig(num_hidden_layers=2, fusion_layer=1, vocab_size=64, max_position_embeddings=16))
    att = m.encoder.layer[1].crossattention.self
    assert isinstance(att, RobertaSelfAttention) and att.save_attention is False
    assert att.get_attention_map() is None and att.get_attn_gradients() is None
    att.save_attention_map("P")
    att.save_attn_gradients("dP")
    assert att.get_attention_map() == "P" and att.get_attn_gradients() == "dP"
    assert not hasattr(m.encoder.layer[0], "crossattention")
