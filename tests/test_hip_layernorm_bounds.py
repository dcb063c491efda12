"""The LayerNorm family (layernorm.hip) under elementwise fp64 bounds, at every width it dispatches on.

tests/test_hip_kernels.py compares these kernels with fp32 torch at 1e-2 of the tensor's largest value, at D = 768 / 1536 / 3072 / 6144 and a
few hundred rows.  Here every narrow width (256 ... 1536) runs in every mode (PLAIN fp32 / bf16 input, POST with a bf16 or an fp32 residual
stream, LS) and every wide one (2048, 3072, 8192: the last fills the kernels' register tile) in PLAIN, forward and backward, at a row count
below a block's four waves or just past it (1, 2, 3, 5), at 261 rows, and at 8200 rows (past the forward's 2048-block grid and the backward's
block cap, so the grid-stride loops and the grouped fold of the column sums run).  Every element of every output -- y, its fp32 twin, mean,
rstd, z / x', dx, dh, dres, the stream, dgamma, dbeta, dbias, dls -- is held to the bound rowwise_util derives from the operands (its header
has the counts), and rows come from six families (rowwise_util.family_rows: mean 100 / spread 1, spread 1e-4 and 1e4, a constant row, a row
with one non-zero element, next to randn * 2).  Inputs sit in NaN-filled parents with rows before and after them, outputs in 7.0-filled
ones whose outside must keep its bits; the workspace is exactly as large as the library asks for.  The backward takes fp32 statistics
computed here, so each direction is checked on its own.  Offsets are whole rows (the kernels do not check alignment).

Every check prints `rowwise-ratio gpu <kernel> <mode> <width> <quantity> <worst err / bound>` (pytest -s); profiles/tests_rowwise_bounds.md
holds the table."""
import ctypes
import functools

import pytest
import torch

import rowwise_util as R
from rowwise_util import BF16, F32, U32

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODE_ID = {"plain32": 0, "plain16": 0, "post16": 1, "post32": 1, "ls": 2}
XFM_E_ARG = -1


def _lib():
    from xfm_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _report(kernel, mode, width, what, ratio):
    print(f"rowwise-ratio gpu {kernel} {mode} {width} {what} {ratio:.3g}")


@functools.lru_cache(maxsize=4)
def _case(D, mode, rows):
    return R.ln_case(D, mode, rows)


def _dev(c):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}


def _cases():
    out = [(D, m, rows) for D in R.LN_NARROW for m in R.LN_MODES for rows in (R.small_rows(D, m), R.ROWS_BIG)]
    out += [(D, m, rows) for D in R.LN_WIDE for m in ("plain32", "plain16") for rows in (R.small_rows(D, m), R.ROWS_BIG)]
    return out + [(256, "plain32", R.ROWS_GRID), (256, "ls", R.ROWS_GRID)]


# -------------------------------------------------------------------------------------------------------------------------- forward
def _fwd(c, gelu=False, drop=(0, 1.0, 0, 0), h=None, res=None):
    """one xfm_layernorm_fwd call on case c (CPU tensors) -> (rc, Outs, inputs kept alive)"""
    L = _lib()
    D, rows, mode = c["D"], c["rows"], c["mode"]
    o, keep = R.Outs(DEV), []

    def inp(t):
        keep.append(R.poisoned_in(t, DEV))
        return keep[-1].data_ptr()

    a = L.LnFwdArgs(w=inp(c["w"]), b=inp(c["b"]), rows=rows, rows_per_sample=c["rps"], eps=R.EPS, gelu=int(gelu),
                    drop_thresh=drop[0], drop_scale=drop[1], seed_lo=drop[2], seed_hi=drop[3])
    a.y, a.y32 = o.add("y", (rows, D), BF16), o.add("y32", (rows, D), F32)
    a.mean, a.rstd = o.add("mean", (rows,), F32), o.add("rstd", (rows,), F32)
    if mode == "plain32":
        a.x32 = inp(c["x"])
    elif mode == "plain16":
        a.x16 = inp(c["x"])
    elif mode.startswith("post"):
        a.h = inp(c["h"] if h is None else h)
        r = c["res"] if res is None else res
        if r.dtype == F32:
            a.res32, a.z32_out = inp(r), o.add("z32", (rows, D), F32)
        else:
            a.res, a.z_out = inp(r), o.add("z", (rows, D), BF16)
    else:
        a.x32, a.h, a.ls_gamma = inp(c["x"]), inp(c["h"]), inp(c["ls_gamma"])
        if c["row_scale"] is not None:
            a.row_scale = inp(c["row_scale"])
        a.x_out = o.add("x_out", (rows, D), F32)
    rc = L.load().xfm_layernorm_fwd(ctypes.byref(a), D, MODE_ID[mode], _stream())
    torch.cuda.synchronize()
    return rc, o, keep


def _check_fwd(c, o, gelu, keep_mask=None, drop_scale=1.0, tag=""):
    D, mode = c["D"], c["mode"]
    g = _dev(c)
    X, x_err = R.ln_row(g, keep_mask, drop_scale)
    ref = R.ln_fwd_ref(X, g["w"], g["b"], R.EPS, x_err, gelu)
    o.check_outside()
    k = "ln_fwd_wide" if D > 1536 else "ln_fwd"
    t = tag + ("gelu" if gelu else "y")
    if mode == "post16":
        _report(k, mode, D, tag + "z16", R.check_bf16(o["z"], X, x_err, "z"))
    elif mode == "post32":
        _report(k, mode, D, tag + "z32", R.check_f32(o["z32"], X, x_err, "z32"))
    elif mode == "ls":
        _report(k, mode, D, tag + "x_out", R.check_f32(o["x_out"], X, x_err, "x_out"))
    _report(k, mode, D, tag + "mean", R.check_f32(o["mean"], *ref["mean"], "mean"))
    _report(k, mode, D, tag + "rstd", R.check_f32(o["rstd"], *ref["rstd"], "rstd"))
    assert bool(torch.isfinite(o["y32"]).all()), "y32 not finite"
    _report(k, mode, D, t + "32", R.check_f32(o["y32"], *ref["y"], "y32"))
    _report(k, mode, D, t + "16", R.check_bf16(o["y"], *ref["y"], "y"))


@pytest.mark.parametrize("D,mode,rows", _cases())
def test_ln_forward_within_bounds(D, mode, rows):
    c = _case(D, mode, rows)
    for gelu in (False, True):
        rc, o, _ = _fwd(c, gelu)
        _lib().check(rc, "layernorm_fwd")
        _check_fwd(c, o, gelu)


# ------------------------------------------------------------------------------------------------------------------------- backward
def _bwd(c, xs, mean, rstd, parts, gelu_b=False, accum=False, dx16=False, drop=(0, 1.0, 0, 0)):
    """one xfm_layernorm_bwd call -> (rc, Outs, ws parent, ws view).  parts: which of dy2 / dy32 join dy1."""
    L = _lib()
    lib = L.load()
    D, rows, mode = c["D"], c["rows"], c["mode"]
    o, keep = R.Outs(DEV), []

    def inp(t):
        keep.append(R.poisoned_in(t, DEV))
        return keep[-1].data_ptr()

    a = L.LnBwdArgs(dy1=inp(c["dy1"]), mean=inp(mean), rstd=inp(rstd), w=inp(c["w"]), rows=rows, rows_per_sample=c["rps"],
                    drop_thresh=drop[0], drop_scale=drop[1], seed_lo=drop[2], seed_hi=drop[3])
    if "dy2" in parts:
        a.dy2 = inp(c["dy2"])
    if "dy32" in parts:
        a.dy32 = inp(c["dy32"])
    if xs.dtype == F32:
        a.x32 = inp(xs)
    else:
        a.x16 = inp(xs)
    if gelu_b:
        a.gelu_b = inp(c["b"])
    dgamma, dbeta = o.add("dgamma", (D,), F32, torch.full((D,), 0.5)), o.add("dbeta", (D,), F32, torch.full((D,), 0.25))
    dbias = dls = 0
    if mode.startswith("plain"):
        a.dx32 = o.add("dx32", (rows, D), F32, c["dx0"] if accum else None)
        a.dx_accum = int(accum)
        if dx16:
            a.dx16 = o.add("dx16", (rows, D), BF16)
    elif mode.startswith("post"):
        a.dh = o.add("dh", (rows, D), BF16)
        dbias = o.add("dbias", (D,), F32, torch.full((D,), 0.5))
        if mode == "post16":
            a.dres = o.add("dres", (rows, D), BF16)
        else:
            a.dres32 = o.add("dres32", (rows, D), F32)
    else:
        a.dh, a.dstream = o.add("dh", (rows, D), BF16), o.add("dstream", (rows, D), F32, c["dx0"])
        a.h, a.ls_gamma = inp(c["h"]), inp(c["ls_gamma"])
        if c["row_scale"] is not None:
            a.row_scale = inp(c["row_scale"])
        dbias, dls = o.add("dbias", (D,), F32, torch.full((D,), 0.5)), o.add("dls", (D,), F32, torch.full((D,), 0.5))
    nb = lib.xfm_layernorm_bwd_workspace(rows, D, MODE_ID[mode])
    assert nb % 4 == 0
    wsv, wsp = R.embed_vec(torch.zeros(nb // 4, dtype=F32, device=DEV), 64, 64, R.SENTINEL)
    rc = lib.xfm_layernorm_bwd(ctypes.byref(a), D, MODE_ID[mode], dgamma, dbeta, dbias, dls, wsv.data_ptr(), nb, _stream())
    torch.cuda.synchronize()
    return rc, o, wsp, wsv


def _check_bwd(c, o, ws, xs, mean, rstd, parts, gelu_b=False, accum=False, keep_mask=None, drop_scale=1.0, tag=""):
    D, rows, mode = c["D"], c["rows"], c["mode"]
    g = _dev(c)
    k = "ln_bwd_wide" if D > 1536 else "ln_bwd"
    o.check_outside()
    R.assert_outside_untouched(ws[0], ws[1], R.SENTINEL, "workspace")
    ref = R.ln_bwd_ref([g["dy1"]] + [g[p] for p in parts], xs.to(DEV), mean.to(DEV), rstd.to(DEV), g["w"], g["b"] if gelu_b else None)
    dx, bdx = ref["dx"]
    DY, e_dy = ref["dy"]
    xh = ref["xh"]
    adds = rows if D > 1536 else 1
    _report(k, mode, D, tag + "dgamma", R.check_f32(o["dgamma"], *R.colsum_bound(DY * xh, e_dy * xh.abs(), 0.5, adds), "dgamma"))
    _report(k, mode, D, tag + "dbeta", R.check_f32(o["dbeta"], *R.colsum_bound(DY, e_dy, 0.25, adds), "dbeta"))
    if mode.startswith("plain"):
        if accum:
            d0 = g["dx0"].double()
            _report(k, mode, D, tag + "dx32+", R.check_f32(o["dx32"], dx + d0, bdx + U32 * d0.abs(), "dx32 accumulated"))
        else:
            _report(k, mode, D, tag + "dx32", R.check_f32(o["dx32"], dx, bdx, "dx32"))
        if "dx16" in o:
            _report(k, mode, D, tag + "dx16", R.check_bf16(o["dx16"], dx, bdx, "dx16"))
        return
    if mode.startswith("post"):
        dh_ref, dh_b = dx, bdx
        if keep_mask is not None:
            s = float(torch.tensor(drop_scale, dtype=F32))
            dh_ref = torch.where(keep_mask, dx * s, torch.zeros_like(dx))
            dh_b = torch.where(keep_mask, bdx * s + U32 * dh_ref.abs(), torch.zeros_like(dx))
        _report(k, mode, D, tag + "dh16", R.check_bf16(o["dh"], dh_ref, dh_b, "dh"))
        if mode == "post16":
            _report(k, mode, D, tag + "dres16", R.check_bf16(o["dres"], dx, bdx, "dres"))
        else:
            _report(k, mode, D, tag + "dres32", R.check_f32(o["dres32"], dx, bdx, "dres32"))
    else:
        d0 = g["dx0"].double()
        o_ref = dx + d0
        b_o = bdx + U32 * o_ref.abs()
        _report(k, mode, D, tag + "dstream", R.check_f32(o["dstream"], o_ref, b_o, "dstream"))
        s = R.row_scale_of(g["row_scale"], rows, c["rps"], DEV)
        sg = s * g["ls_gamma"].double()
        _report(k, mode, D, tag + "dh16", R.check_bf16(o["dh"], sg * o_ref, sg.abs() * b_o + 3 * U32 * (sg * o_ref).abs(), "dh"))
        _report(k, mode, D, tag + "dls", R.check_f32(o["dls"], *R.colsum_bound(s * g["h"].double() * o["dstream"].double(), None, 0.5), "dls"))
    # dbias sums the kernel's own bf16 dh, as stored
    _report(k, mode, D, tag + "dbias", R.check_f32(o["dbias"], *R.colsum_bound(o["dh"], None, 0.5), "dbias"))


def _bwd_variants(mode):
    """(dy parts, gelu_b, dx_accum, dx16) of the calls a mode gets"""
    if mode.startswith("plain"):
        return [((), False, False, False), (("dy2", "dy32"), False, True, True), ((), True, False, True)]
    return [((), False, False, False), (("dy32",) if mode == "post32" else ("dy2",), False, False, False)]


@pytest.mark.parametrize("D,mode,rows", _cases())
def test_ln_backward_within_bounds(D, mode, rows):
    c = _case(D, mode, rows)
    xs = R.ln_stored(c)
    mean, rstd = R.ln_stats(xs)
    for i, (parts, gelu_b, accum, dx16) in enumerate(_bwd_variants(mode)):
        rc, o, wsp, wsv = _bwd(c, xs, mean, rstd, parts, gelu_b, accum, dx16)
        _lib().check(rc, "layernorm_bwd")
        _check_bwd(c, o, (wsp, wsv), xs, mean, rstd, parts, gelu_b, accum, tag=f"v{i}:")


# ---------------------------------------------------------------------------------------------------------------- POST with dropout
def test_ln_post_dropout_mask_is_a_function_of_seed_row_column():
    """p = 0.1: the mask is read off a first call with h = 1, res = 0 (z = keep / (1 - p)) and then used in the fp64 reference of a second call
    with the same seed on random data, forward and backward: it may depend on (seed, row, column) only."""
    from xfm_amd import functional as Fx
    D, rows = 768, R.ROWS_BIG
    c = _case(D, "post16", rows)
    drop = Fx.drop_params(0.1, 0x1234567890ABCDEF)
    rc, o, _ = _fwd(c, drop=drop, h=torch.ones((rows, D), dtype=BF16), res=torch.zeros((rows, D), dtype=BF16))
    _lib().check(rc, "layernorm_fwd")
    z = o["z"].float()
    keep = z != 0
    frac = float(keep.double().mean())
    assert abs(frac - 0.9) < 0.01, frac
    assert float((z[keep] - 1.0 / 0.9).abs().max()) <= 1.0 / 0.9 * R.U16
    rc, o, _ = _fwd(c, drop=drop)
    _lib().check(rc, "layernorm_fwd")
    _check_fwd(c, o, False, keep, drop[1], tag="drop:")
    xs = o["z"].cpu()   # the backward reads the z this forward stored
    mean, rstd = R.ln_stats(xs)
    rc, ob, wsp, wsv = _bwd(c, xs, mean, rstd, ("dy2",), drop=drop)
    _lib().check(rc, "layernorm_bwd")
    _check_bwd(c, ob, (wsp, wsv), xs, mean, rstd, ("dy2",), keep_mask=keep, drop_scale=drop[1], tag="drop:")


# ------------------------------------------------------------------------------------------------------------------ rejected widths
@pytest.mark.parametrize("D,mode", [(640, "plain32"), (640, "plain16"), (9216, "plain32"), (9216, "plain16"), (2048, "post16"),
                                    (2048, "post32"), (2048, "ls")])
def test_ln_rejected_widths_touch_nothing(D, mode):
    c = R.ln_case(D, mode, 3)
    rc, o, _ = _fwd(c)
    assert rc == XFM_E_ARG, rc
    assert b"unsupported width" in _lib().load().xfm_last_error()
    o.check_unchanged()
    xs = R.ln_stored(c)
    mean, rstd = R.ln_stats(xs)
    rc, o, wsp, wsv = _bwd(c, xs, mean, rstd, ())
    assert rc == XFM_E_ARG, rc
    assert b"unsupported width" in _lib().load().xfm_last_error()
    o.check_unchanged()
    R.assert_outside_untouched(wsp, wsv, R.SENTINEL, "workspace")
    assert float(wsv.abs().max()) == 0.0
