"""The Grad-CAM kernels on a real MI355X: xfm_xattn_gradcam and xfm_cam_box_rank against the fp64 restatements and derived bounds of
tests/gradcam_util.py (its header has the derivations; no bound is fitted to the kernels' output).

  kernel in isolation    every operand a strided slice of a poisoned parent; cam, P and dP of the three shapes of the issue, dense rows,
                         dense rows with lengths and packed rows, a kv_src that is a permutation and one that shares a source; every
                         combination of the three optional outputs gives the same bits as the launch with all three; two launches give
                         equal bits; equal bits under XFM_DETERMINISTIC=1 (a fresh child process).
  with the real lse      the same kernel on the lse xfm_attn_fwd left: the same bound plus P times the forward's own lse bound.
  box ranking            scores against the fp64 restatement (same fp32 taps) and against F.interpolate + the reference's loop; indices, IoU
                         flags and counts EQUAL: gradcam_util.box_rank_expect asserts for every ref that its margin exceeds the bound."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gemm_strided_util import SENTINEL, assert_outside_untouched, check_f32  # noqa: E402
from gradcam_util import (BOX_P, MODES, SHAPES, GradcamBuffers, box_rank_case, box_rank_expect, fwd_lse_bound, gradcam_digests,  # noqa: E402
                          gradcam_ref, interp_score_bound, interp_scores, kernel_score_bound, make_case, run_box_rank)

DEV = "cuda"


def _lib():
    from xfm_amd import _lib
    return _lib


def _launch(bufs, cam, p, dp, **over):
    lib = _lib().load()
    a = bufs.args(_lib(), cam, p, dp, **over)
    rc = lib.xfm_xattn_gradcam(ctypes.byref(a), None)
    assert rc == 0, lib.xfm_last_error()
    torch.cuda.synchronize()


def _shaped(c, cam, p, dp):
    B, H, Sq, Sk = c["B"], c["H"], c["Sq"], c["Sk"]
    return cam.cpu().view(B, Sk - 1), p.cpu().view(B, H, Sq, Sk), dp.cpu().view(B, H, Sq, Sk)


# ---------------------------------------------------------------------------------------------------------------- xfm_xattn_gradcam
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_gradcam_kernel_matches_the_fp64_restatement(name, mode):
    c = make_case(name, mode)
    ref = gradcam_ref(c)
    bufs = GradcamBuffers(c, ref["lse32"], DEV)
    (cam, cam_par), (p, p_par), (dp, dp_par) = bufs.outputs(True, True, True)
    _launch(bufs, cam, p, dp)
    gc, gp, gdp = _shaped(c, cam, p, dp)
    rp = check_f32(gp, ref["P"], ref["bP"], f"{name}/{mode} P")
    rd = check_f32(gdp, ref["dP"], ref["bdP"], f"{name}/{mode} dP")
    rc = check_f32(gc, ref["cam"], ref["bcam"], f"{name}/{mode} cam")
    print(f"{name}/{mode}: worst err / bound  P {rp:.3f}  dP {rd:.3f}  cam {rc:.3f}")
    for b, n in enumerate(c["lens"]):   # rows past an entry's length: exact zeros in both maps
        assert float(gp[b, :, n:].abs().max() if n < c["Sq"] else 0.0) == 0.0 and float(gdp[b, :, n:].abs().max() if n < c["Sq"] else 0.0) == 0.0
    for par, view in ((cam_par, cam), (p_par, p), (dp_par, dp)):
        assert_outside_untouched(par, view, SENTINEL, "output parent")
    # every combination of the optional outputs: the bits of the launch with all three; a second launch: the same bits
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
        (cam2, cp2), (p2, pp2), (dp2, dp2p) = bufs.outputs(*[bool(w) for w in want])
        _launch(bufs, cam2, p2, dp2)
        for got, first, par in ((cam2, cam, cp2), (p2, p, pp2), (dp2, dp, dp2p)):
            if got is not None:
                assert torch.equal(got.view(torch.int32), first.view(torch.int32)), (name, mode, want)
                assert_outside_untouched(par, got, SENTINEL, "output parent")


def test_gradcam_kernel_entry_without_a_source_is_zeros():
    c = make_case("s37", "dense_len")
    ref2 = gradcam_ref(c, bad_src=(1, 2))   # (their lse rows stay NaN: nothing of such an entry is read)
    bufs = GradcamBuffers(c, ref2["lse32"], DEV)
    bufs.kv_src = torch.tensor([2, 7, -1], dtype=torch.int32, device=DEV)
    (cam, _), (p, _), (dp, _) = bufs.outputs(True, True, True)
    _launch(bufs, cam, p, dp)
    gc, gp, gdp = _shaped(c, cam, p, dp)
    check_f32(gp, ref2["P"], ref2["bP"], "P")
    check_f32(gc, ref2["cam"], ref2["bcam"], "cam")
    assert float(gp[1:].abs().max()) == 0.0 and float(gdp[1:].abs().max()) == 0.0 and float(gc[1:].abs().max()) == 0.0


@pytest.mark.parametrize("name", list(SHAPES))
def test_gradcam_kernel_on_the_forwards_own_lse(name):
    """xfm_attn_fwd (grouped route, packed query rows) leaves the lse; the Grad-CAM kernel reads it as it stands."""
    from xfm_amd import functional as Fx
    c = make_case(name, "packed")
    ref = gradcam_ref(c)
    bufs = GradcamBuffers(c, ref["lse32"], DEV)
    B, H, Sq, Sk = c["B"], c["H"], c["Sq"], c["Sk"]
    src = torch.arange(B, dtype=torch.int32, device=DEV) if bufs.kv_src is None else bufs.kv_src
    groups = Fx.kv_groups(src, c["n_src"])
    _, lse = Fx.attn_fwd(bufs.q, bufs.k, bufs.v, B, H, Sq, Sk, 0.125, groups=groups, q_pack=(bufs.q_start, bufs.q_len))
    torch.cuda.synchronize()
    b_lse = fwd_lse_bound(c, ref)
    for b, n in enumerate(c["lens"]):
        check_f32(lse[b, :, :n].cpu(), ref["lse"][b, :, :n], b_lse[b, :, :n], "lse of the forward")
    # the reference is the exact softmax (the fp64 lse); the lse the kernel is given lies within b_lse of it, which moves P by at most
    # P (exp(b_lse) - 1) on top of the kernel's own bound
    exact = gradcam_ref(c, lse_given=ref["lse"])
    bufs.lse = lse
    (cam, _), (p, _), (dp, _) = bufs.outputs(True, True, True)
    _launch(bufs, cam, p, dp)
    gc, gp, gdp = _shaped(c, cam, p, dp)
    moved = exact["P"] * torch.expm1(b_lse)[..., None]
    rp = check_f32(gp, exact["P"], exact["bP"] + moved, f"{name} P on the forward's lse")
    check_f32(gdp, exact["dP"], exact["bdP"], f"{name} dP")
    bcam = exact["bcam"] + (moved * exact["dP"].clamp(min=0)).sum(dim=(1, 2))[:, 1:] / float(H * c["t_div"])
    rc = check_f32(gc, exact["cam"], bcam, f"{name} cam on the forward's lse")
    print(f"{name}: worst err / bound on the forward's lse  P {rp:.3f}  cam {rc:.3f}")


def test_gradcam_same_bits_under_xfm_deterministic():
    """A fresh child process with XFM_DETERMINISTIC=1 against this process without it: every output of both kernels, bit for bit."""
    env = dict(os.environ, XFM_DETERMINISTIC="1")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "gradcam_util.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    child = [line for line in r.stdout.splitlines() if line.startswith("GRADCAM ")][-1].split()[1:]
    saved = os.environ.pop("XFM_DETERMINISTIC", None)
    try:
        own = gradcam_digests()
    finally:
        if saved is not None:
            os.environ["XFM_DETERMINISTIC"] = saved
    assert len(own) == 3 * len(SHAPES) * len(MODES) + 2 * len(BOX_P) and child == own, (child, own)


def test_gradcam_argument_errors_launch_nothing():
    c = make_case("s37", "packed")
    ref = gradcam_ref(c)
    bufs = GradcamBuffers(c, ref["lse32"], DEV)
    (cam, cam_par), (p, p_par), (dp, dp_par) = bufs.outputs(True, True, True)
    lib = _lib().load()
    a = bufs.args(_lib(), None, None, None)
    assert lib.xfm_xattn_gradcam(ctypes.byref(a), None) == -1 and b"no output" in lib.xfm_last_error()
    bad_arg = [dict(q=0), dict(dout=0), dict(k=0), dict(v=0), dict(lse=0), dict(B=0), dict(B=70000), dict(H=0),
               dict(Sq=0), dict(Sk=1), dict(q_rs=64), dict(k_rs=c["D"] + 4), dict(q=bufs.q.data_ptr() + 2), dict(lse=bufs.lse.data_ptr() + 4),
               dict(stat_ld=c["Sq"] - 4), dict(stat_ld=c["Sq"] + 2), dict(q_len=0), dict(n_src=0), dict(t_div=0), dict(scale=0.0),
               dict(scale=float("inf"))]
    for over in bad_arg:
        a = bufs.args(_lib(), cam, p, dp, **over)
        assert lib.xfm_xattn_gradcam(ctypes.byref(a), None) == -1 and b"xattn_gradcam" in lib.xfm_last_error(), over
    a = bufs.args(_lib(), cam, p, dp, Sq=65, stat_ld=68)
    assert lib.xfm_xattn_gradcam(ctypes.byref(a), None) == -3 and b"xattn_gradcam" in lib.xfm_last_error()
    assert lib.xfm_xattn_gradcam(None, None) == -1
    torch.cuda.synchronize()
    for par, view in ((cam_par, cam), (p_par, p), (dp_par, dp)):   # nothing ran: the outputs still hold their NaN, the borders their poison
        assert bool(torch.isnan(view).all())
        assert_outside_untouched(par, view, SENTINEL, "output parent")


# ---------------------------------------------------------------------------------------------------------------- xfm_cam_box_rank
@pytest.mark.parametrize("p", BOX_P)
def test_cam_box_rank_matches_the_restatement_and_interpolate(p):
    case = box_rank_case(p)
    want = box_rank_expect(case, lambda m, hw, pp: max(kernel_score_bound(m, hw, pp), interp_score_bound(m)))
    out, counts, kept = run_box_rank(case, DEV, calls=2, out_offset=3)
    assert kept
    want_counts = np.zeros((3, 2), dtype=np.int64)
    worst_k = worst_i = 0.0
    for i, (sc, mg, pick, best, iou) in enumerate(want):
        hw, dets = case["hw"][i], case["dets"][i]
        assert int(out[i, 0]) == pick, (p, i, out[i], pick)
        if pick >= 0:
            bk = kernel_score_bound(mg[pick], hw, p)
            assert abs(out[i, 1] - best) <= bk, (p, i, out[i, 1], best, bk)
            worst_k = max(worst_k, abs(out[i, 1] - best) / bk)
            assert abs(out[i, 2] - iou) <= 2.0 ** -50 and (out[i, 2] >= 0.5) == (iou >= 0.5)
        else:
            assert out[i, 1] == 0.0 and out[i, 2] == 0.0
        # the reference's own recipe: the interpolated map on the CPU, the Python loop
        si = interp_scores(case["cam"][i], hw, dets, case["alpha"])
        for d in range(len(dets)):
            bi = interp_score_bound(mg[d])
            assert abs(si[d] - sc[d]) <= bi, (p, i, d, si[d], sc[d], bi)
            worst_i = max(worst_i, abs(si[d] - sc[d]) / bi if bi > 0 else 0.0)
        pick_i = -1
        best_i = 0.0
        for d in range(len(dets)):
            if si[d] > best_i:
                best_i, pick_i = si[d], d
        assert pick_i == pick, (p, i, pick_i, pick)
        s = int(case["split"][i])
        want_counts[s, 1] += 1
        want_counts[s, 0] += int(pick >= 0 and iou >= 0.5)
    print(f"p={p}: worst err / bound  kernel score {worst_k:.3f}  interpolate vs restatement {worst_i:.3f}; counts {counts.tolist()}")
    assert np.array_equal(counts, 2 * want_counts)   # two calls accumulate into one buffer
    assert want[4][2] == -1 and want[3][2] == 1 and len(case["dets"][1]) == 256 and len(case["dets"][2]) == 1


def test_cam_box_rank_argument_errors_launch_nothing():
    from xfm_amd import functional as Fx
    lib = _lib().load()
    case = box_rank_case(6)
    n = 5
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    start = np.zeros(n + 1, dtype=np.int32)
    start[1:] = np.cumsum([len(d) for d in case["dets"]])
    cam, hw, det, st, rb, sp = t(case["cam"]), t(case["hw"]), t(np.concatenate(case["dets"])), t(start), t(case["ref_box"]), t(case["split"])
    out = torch.full((n, 3), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((3, 2), 5, dtype=torch.int64, device=DEV)
    base = dict(cam=cam.data_ptr(), p=6, hw=hw.data_ptr(), det=det.data_ptr(), st=st.data_ptr(), md=256, rb=rb.data_ptr(), sp=sp.data_ptr(), n=n,
                alpha=0.5, out=out.data_ptr(), off=0, counts=counts.data_ptr())

    def call(**over):
        k = dict(base)
        k.update(over)
        return lib.xfm_cam_box_rank(k["cam"], k["p"], k["hw"], k["det"], k["st"], k["md"], k["rb"], k["sp"], k["n"], k["alpha"], k["out"], k["off"],
                                    k["counts"], None)
    for over in (dict(cam=None), dict(hw=None), dict(det=None), dict(st=None), dict(rb=None), dict(sp=None), dict(out=None), dict(counts=None),
                 dict(n=0), dict(p=0), dict(off=-1), dict(md=-1), dict(alpha=float("nan")), dict(alpha=float("inf"))):
        assert call(**over) == -1 and b"cam_box_rank" in lib.xfm_last_error(), over
    for over in (dict(p=33), dict(md=257)):
        assert call(**over) == -3 and b"cam_box_rank" in lib.xfm_last_error(), over
    with pytest.raises(_lib().XfmHipError, match="cam_box_rank"):
        Fx.cam_box_rank(cam, hw, det, st, 300, rb, sp, 0.5, counts, out, 0)
    torch.cuda.synchronize()
    assert counts.tolist() == [[5, 5]] * 3 and float(out.min()) == 7.0 == float(out.max())


# ---------------------------------------------------------------------------------------------------------------- the module contract
# Bounds: the project's standing rule of tests/test_hip_modules.py, no new number -- a forward quantity (P) to OUT_TOL, a gradient (dP, the
# cams) to GRAD_TOL, cosine COS_TOL; a cam may exceed GRAD_TOL only up to FLOOR_ERR x the fixture's bf16-autocast floor for that ref
# (cosine: FLOOR_COS x).  Fused against unfused: the same kernels produce q2, kv, lse2 and dc2 on both routes, so the two differ by the
# order of the sums alone -- the kernel's cam bound of gradcam_util, evaluated on the maps the unfused route saved.
def _fixture_model():
    from golden_util import load
    from test_hip_modules import _load_into, _pretrain_cfg
    from xfm_amd import synthetic as syn
    from xfm_amd.model_retrieval import XFMForRetrieval
    z, meta = load("gradcam_small")
    m = XFMForRetrieval(_pretrain_cfg(meta))
    _load_into(m, meta["spec"])
    m.cuda().finalize().eval()
    image = syn.grounding_eval_batch(meta["B"], seed=meta["batch_seed"], image_res=meta["image_res"], max_tokens=meta["max_tokens"],
                                     min_len=meta["min_len"])[0]
    ids, atts = torch.from_numpy(z["text_ids"]), torch.from_numpy(z["text_atts"])
    return z, meta, m, image.cuda(), ids.cuda(), atts.cuda()


def _rel_cos(got, ref):
    got, ref = got.double().reshape(-1).cpu(), ref.double().reshape(-1)
    return float((got - ref).norm() / ref.norm()), float((got @ ref) / (got.norm() * ref.norm()))


@pytest.fixture(scope="module")
def fixture_run():
    """The fixture's model and batch, the unfused pass (which leaves the maps) and the fused one, computed once."""
    from xfm_amd import gradcam as G
    z, meta, m, image, ids, atts = _fixture_model()
    # fused first.  The arena hands every parameter its .grad view when it is built, so "no gradient appeared" reads here: no
    # parameter is marked live, every .grad is still the arena's own view, and the gradient buffer keeps the poison written before the call
    arena = m._arena
    assert not any(arena.live)
    live_ver = arena.live_ver
    arena.grad.fill_(7.0)
    fused = G.cross_attention_gradcam(m, image, ids, atts, meta["block_num"], fused=True)
    torch.cuda.synchronize()
    untouched = (not any(arena.live) and arena.live_ver == live_ver and all(p.grad is p._xfm_grad for p in m.parameters())
                 and bool((arena.grad == 7.0).all()))
    arena.grad.zero_()
    att = m.fusion_encoder.roberta.encoder.layer[meta["block_num"]].crossattention.self
    att.save_attention = True
    image_embeds, image_atts = m.get_vision_embeds(image)
    cls = m.get_cross_embeds(image_embeds, image_atts, text_ids=ids, text_atts=atts)[:, 0, :]
    m.itm_head(cls)[:, 1].sum().backward()
    P, dP = att.get_attention_map().clone(), att.get_attn_gradients().clone()
    att.save_attention = False
    m.zero_grad()
    unfused = G.cross_attention_gradcam(m, image, ids, atts, meta["block_num"], fused=False)
    torch.cuda.synchronize()
    return dict(z=z, meta=meta, m=m, image=image, ids=ids, atts=atts, fused=fused, unfused=unfused, P=P, dP=dP, untouched=untouched)


def test_attention_maps_match_the_fixture(fixture_run):
    from test_hip_modules import COS_TOL, GRAD_TOL, OUT_TOL
    r = fixture_run
    z, lens = r["z"], r["meta"]["lens"]
    assert r["P"].dtype == torch.float32 and tuple(r["P"].shape) == z["P"].shape == tuple(r["dP"].shape)
    for b, n in enumerate(lens):
        ep, cp = _rel_cos(r["P"][b, :, :n], torch.from_numpy(z["P"][b, :, :n]))
        ed, cd = _rel_cos(r["dP"][b, :, :n], torch.from_numpy(z["dP"][b, :, :n]))
        print(f"ref {b} (len {n}): P rel-L2 {ep:.3e} cos {cp:.6f}   dP rel-L2 {ed:.3e} cos {cd:.6f}")
        assert ep <= OUT_TOL and cp >= COS_TOL, (b, ep, cp)
        assert ed <= GRAD_TOL and cd >= COS_TOL, (b, ed, cd)
        assert float(r["P"][b, :, n:].abs().sum()) == 0.0 and float(r["dP"][b, :, n:].abs().sum()) == 0.0   # rows past the length: zeros


@pytest.mark.parametrize("which", ["fused", "unfused"])
def test_gradcam_matches_the_fixture_per_ref(fixture_run, which):
    from test_hip_modules import COS_TOL, FLOOR_COS, FLOOR_ERR, GRAD_TOL
    r = fixture_run
    z = r["z"]
    cam = r[which]
    assert cam.dtype == torch.float32 and tuple(cam.shape) == z["cam"].shape
    worst = 0.0
    for b in range(cam.shape[0]):
        err, cos = _rel_cos(cam[b], torch.from_numpy(z["cam"][b]))
        f_err, f_cos = float(z["floor"][b, 0]), float(z["floor"][b, 1])
        print(f"{which} ref {b}: rel-L2 {err:.3e} (floor {f_err:.3e}) cos {cos:.6f} (floor {f_cos:.6f})")
        assert err <= max(GRAD_TOL, FLOOR_ERR * f_err), (which, b, err, f_err)
        assert 1.0 - cos <= max(1.0 - COS_TOL, FLOOR_COS * (1.0 - f_cos)), (which, b, cos, f_cos)
        worst = max(worst, err)
    print(f"{which}: worst rel-L2 {worst:.3e}")


def test_fused_and_unfused_agree_to_the_kernel_bound(fixture_run):
    from gradcam_util import U32
    r = fixture_run
    P, dP = r["P"].double().cpu(), r["dP"].double().cpu()
    B, H, T, Sk = P.shape
    # the maps are the kernel's own fp32 outputs: the fused sum and the ATen product / means differ by their (H T + 2)-term summation
    # and the unfused route's extra roundings (the product, the two means): (N + 4) u32 relative to the sum of the terms
    term = (P * dP.clamp(min=0))[..., 1:].sum(dim=(1, 2)) / (H * T)
    bound = (H * T + 4) * U32 * term
    err = (r["fused"].double().cpu().reshape(B, -1) - r["unfused"].double().cpu().reshape(B, -1)).abs()
    print(f"fused vs unfused: worst err / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())


def test_fused_call_touches_no_parameter_gradient(fixture_run):
    assert fixture_run["untouched"]


def test_save_attention_false_leaves_ordinary_passes_bit_equal(monkeypatch):
    """Outputs and gradients of an ordinary forward / backward: a run made before any map was ever requested against a run after maps
    were requested and switched off again.  XFM_DETERMINISTIC=1 (the default build sums some gradients with float atomics); a baseline
    pair of runs says which tensors repeat bit for bit at all: every tensor of the fusion tower and of the head must, and those are compared."""
    from xfm_amd import gradcam as G
    monkeypatch.setenv("XFM_DETERMINISTIC", "1")
    z, meta, m, image, ids, atts = _fixture_model()

    def run():
        m.zero_grad()
        image_embeds, image_atts = m.get_vision_embeds(image)
        seq = m.get_cross_embeds(image_embeds, image_atts, text_ids=ids, text_atts=atts)
        m.itm_head(seq[:, 0, :])[:, 1].sum().backward()
        torch.cuda.synchronize()
        live = {n for n, p in m.named_parameters() if m._arena.live[m._arena._unit_of[id(p)]]}
        return seq.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if n in live}
    seq0, g0 = run()
    seq0b, g0b = run()
    assert torch.equal(seq0.view(torch.int16), seq0b.view(torch.int16)) and g0.keys() == g0b.keys() and len(g0) > 50
    repeat = {n for n in g0 if torch.equal(g0[n], g0b[n])}
    assert all(n in repeat for n in g0 if n.startswith(("fusion_encoder.", "itm_head."))), sorted(set(g0) - repeat)[:5]
    G.cross_attention_gradcam(m, image, ids, atts, meta["block_num"], fused=False)
    G.cross_attention_gradcam(m, image, ids, atts, meta["block_num"], fused=True)
    att = m.fusion_encoder.roberta.encoder.layer[meta["block_num"]].crossattention.self
    assert att.save_attention is False and att.get_attention_map() is None
    seq1, g1 = run()
    assert torch.equal(seq0.view(torch.int16), seq1.view(torch.int16))
    assert g0.keys() == g1.keys()
    for n in repeat:
        assert torch.equal(g0[n], g1[n]), n
    print(f"{len(repeat)} of {len(g0)} gradient tensors repeat bit for bit between two plain runs; all of those are unchanged")


def test_training_mode_raises():
    from xfm_amd import gradcam as G
    z, meta, m, image, ids, atts = _fixture_model()
    m.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        G.cross_attention_gradcam(m, image, ids, atts, meta["block_num"])
    att = m.fusion_encoder.roberta.encoder.layer[meta["block_num"]].crossattention.self
    att.save_attention = True
    with pytest.raises(RuntimeError, match="eval mode"):
        image_embeds, image_atts = m.get_vision_embeds(image)
        m.get_cross_embeds(image_embeds, image_atts, text_ids=ids, text_atts=atts)


def test_val_and_grounding_eval_reproduce_the_fixture_with_one_read(fixture_run, monkeypatch):
    from types import SimpleNamespace as NS
    from xfm_amd import gradcam as G
    r = fixture_run
    z, meta = r["z"], r["meta"]
    reads = []
    real = G._read
    monkeypatch.setattr(G, "_read", lambda t: (reads.append(1), real(t))[1])
    B = meta["B"]
    loader = [(r["image"][:2].cpu(), (r["ids"][:2].cpu(), r["atts"][:2].cpu()), torch.tensor(meta["ref_ids"][:2])),
              (r["image"][2:].cpu(), (r["ids"][2:].cpu(), r["atts"][2:].cpu()), torch.tensor(meta["ref_ids"][2:]))]
    cams, ref_ids = G.val(r["m"], loader, torch.device("cuda"), meta["block_num"], meta["image_res"] // meta["patch"])
    assert cams.is_cuda and tuple(cams.shape) == z["cam"].shape and ref_ids == meta["ref_ids"] and not reads
    start = np.concatenate([[0], np.cumsum(z["det_count"])])
    dets = [z["dets"][start[k]:start[k + 1]] for k in range(B)]
    refs = NS(ref_box=z["ref_box"], ref_size=z["ref_size"], ref_split=z["ref_split"])
    acc, rows = G.grounding_eval(cams, refs, dets, alpha=meta["alpha"], return_rows=True)
    assert len(reads) == 1
    assert [int(v) for v in rows[:, 0]] == z["chosen"].tolist()
    assert [v >= 0.5 for v in rows[:, 2]] == [v >= 0.5 for v in z["iou"]] and np.abs(rows[:, 2] - z["iou"]).max() < 1e-12
    assert acc == meta["acc"]
    acc2 = G.grounding_eval(cams, refs, dets, alpha=meta["alpha"])
    assert acc2 == acc and len(reads) == 2


def test_grounding_script_runs_on_the_synthetic_config(tmp_path, capsys):
    """Grounding.py --evaluate on configs/Grounding_synthetic.yaml, towers cut to 2 + 2 + 2 layers and 96 px so that the test stays short."""
    import importlib
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = importlib.import_module("Grounding")
    with open(os.path.join(root, "configs", "Grounding_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(image_res=96, text_num_hidden_layers=2, text_fusion_start_at=2, fusion_num_hidden_layers=2, vision_depth=2, batch_size=4,
               test_dataset_size=8, max_tokens=12)
    args = script.parse_args(["--evaluate", "--block_num", "1", "--output_dir", str(tmp_path)])
    acc = script.main(args, cfg)
    assert set(acc) == {"val_d", "testA_d", "testB_d"} and all(0.0 <= v <= 1.0 for v in acc.values())
    assert "Start evaluating" in capsys.readouterr().out
    with pytest.raises(NotImplementedError):
        script.main(script.parse_args(["--output_dir", str(tmp_path)]), cfg)
    with pytest.raises(NotImplementedError):
        script.main(script.parse_args(["--evaluate", "--gradcam_mode", "itc", "--output_dir", str(tmp_path)]), cfg)


def test_saving_last_layer_runs_all_its_rows_on_packed_grouped_passes():
    """Packed rows, an encoder_batch_index (the grouped cross-attention) and `output_rows`: a last layer that saves its maps is not run on
    the selected rows alone -- the result equals the full tower read at those rows bit for bit -- and its map is a softmax on every real
    token row (rows sum to 1 to fp32 rounding of Sk terms), zero past each sequence's length, with the sequences in the pack's order."""
    from test_hip_packing import _lens, _roberta
    from xfm_amd.packing import image_major_layout, pack_rows
    torch.manual_seed(0)
    m = _roberta(2, 0).cuda().finalize().eval()
    B, U, T, N, M = 6, 3, 30, 197, 4
    ln = _lens(B, T, 8, lo=6)
    g = torch.Generator().manual_seed(5)
    seq_img = torch.randint(0, U, (B,), generator=g)
    n_cls = 3
    pos = torch.stack([torch.randint(0, int(ln[n_cls + j]), (M,), generator=g) for j in range(B - n_cls)])
    sel_off = list(range(n_cls)) + [n_cls + j * M for j in range(B - n_cls)]
    sel_len = [1] * n_cls + [M] * (B - n_cls)
    pack, order, pos_of, meta, _ = image_major_layout(ln.tolist(), seq_img.tolist(), U, T, "cuda", extra=(seq_img.tolist(), sel_off, sel_len))
    keep = torch.arange(T)[None, :] < ln[:, None]
    x = ((torch.randn(B, T, 768, generator=g) * 0.7) * keep[..., None]).to(torch.bfloat16).cuda()
    img = (torch.randn(U, N, 768, generator=g) * 0.7).to(torch.bfloat16).cuda()
    from xfm_amd.xfm import _ones_mask
    iatts = _ones_mask(img)   # (the towers' own all-ones mask: image keys are never masked on this path; a real key mask raises)
    start_of = pack.start.index_select(0, torch.tensor(pos_of, device="cuda"))
    rows = torch.cat([start_of[:n_cls], (start_of[n_cls:, None] + pos.cuda().to(torch.int32)).reshape(-1)]).to(torch.int32)
    xr = pack_rows(x[torch.tensor(order)], pack)
    kw = dict(encoder_embeds=xr, attention_mask=None, encoder_hidden_states=img, encoder_attention_mask=iatts,
              encoder_batch_index=meta[1].contiguous(), pack=pack)
    att = m.roberta.encoder.layer[1].crossattention.self
    att.save_attention = True
    with torch.no_grad():
        full = m.bert(**kw).last_hidden_state.index_select(0, rows.long())
        P_full = att.get_attention_map().clone()
        sel = m.bert(output_rows=(rows, meta[2].contiguous(), meta[3].contiguous(), M), **kw).last_hidden_state
        P_sel = att.get_attention_map().clone()
        with pytest.raises(NotImplementedError, match="masked image keys"):
            m.bert(**dict(kw, encoder_attention_mask=torch.ones(U, N, dtype=torch.long, device="cuda")))
    att.save_attention = False
    assert sel.shape == (rows.numel(), 768) and torch.equal(sel.view(torch.int16), full.view(torch.int16))
    assert tuple(P_full.shape) == (B, 12, T, N) and torch.equal(P_full, P_sel)
    lens = pack.lens.cpu().tolist()
    for b, n in enumerate(lens):
        s = P_full[b, :, :n].double().sum(-1)
        # (a sanity bound, not a precision test -- those are above: Sk roundings of the sum plus the forward's lse error, which for
        # scores of this size is below 1e-4 by attention_util's count; 1e-3 leaves an order of room)
        assert float((s - 1.0).abs().max()) <= 1e-3, (b, float((s - 1.0).abs().max()))
        assert float(P_full[b, :, n:].abs().sum()) == 0.0
