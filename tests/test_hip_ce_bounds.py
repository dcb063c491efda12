"""The cross-entropy family (cross_entropy.hip) under elementwise fp64 bounds: ce_fwd / ce_bwd (one-hot), the label form and the dense form.

The existing tests hold dlogits to 1e-2 of the tensor's largest entry -- the label's, about `scale` -- while at V = 50265 every other entry is
some 1e-5 of that: a zeroed last column, a wrong scalar tail, a chunk read from its neighbour all pass.  Here every element of dlogits is
held to rowwise_util.ce_bwd_ref's bound (from the lse and tsum handed to the kernel, so the backward is checked on its own), at shapes that
put V on and next to every boundary of the kernels: V = 50265 / ld 50304, V = 1001 and 1003 (a scalar tail of 1 and 3 columns, ld = V + 7 and
V + 1), V = 8 = ld, V = 5, V = 3 = ld (no 16-byte load at all) and V = 4096, where the four-way unrolled forward loop stops one granule short.
Rows: one scaled by 30, one whose largest logit is 100 above the rest (its other entries flush), the last one ignored.  The logits' padding
columns [V, ld) are NaN in one run and +1e30 in another (fmaxf drops a NaN, so NaN alone cannot show a read in the max pass), the rows
around them NaN; dlogits' padding [V, ldd) must be exactly zero and the 7.0 around every output must keep its bits.  The forward is checked
with the row maximum planted 20 above the rest at column 0, V - 1, V & ~3, (V & ~3) - 1 and the label in turn: a lost column moves lse by
O(1) against a bound of 1e-7 (V + 90).

Every check prints `rowwise-ratio gpu <kernel> <form> <V> <quantity> <worst err / bound>` (pytest -s)."""
import functools

import pytest
import torch

import rowwise_util as R
from rowwise_util import BF16, F32, U32

pytestmark = pytest.mark.gpu

DEV = "cuda"
PADS = {"nan": float("nan"), "1e30": 1e30}


def _lib():
    from xfm_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _report(kernel, form, V, what, ratio):
    print(f"rowwise-ratio gpu {kernel} {form} {V} {what} {ratio:.3g}")


def _padded(x, ld, pad):
    """x [R, V] as the first V columns of a [R, ld] view (columns [V, ld) = pad) of a parent with 4 NaN rows before and 3 after"""
    Rr, V = x.shape
    t = torch.full((Rr, ld), pad, dtype=F32, device=DEV)
    t[:, :V] = x.to(DEV)
    return R.embed(t, ld, 0, 4, 3, R.NAN)[0]


def _vec(t):
    return R.poisoned_in(t, DEV)


@functools.lru_cache(maxsize=2)
def _case(Rr, V):
    return R.ce_case(Rr, V)


def _dev(c):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}


# ------------------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("pad", list(PADS))
@pytest.mark.parametrize("form", R.CE_FORMS)
@pytest.mark.parametrize("Rr,V,ld", R.CE_SHAPES)
def test_ce_backward_within_bounds(Rr, V, ld, form, pad):
    lib = _lib().load()
    c = _case(Rr, V)
    g = _dev(c)
    ldd = (ld + 7) // 8 * 8
    x = _padded(c["x"], ld, PADS[pad])
    t, tsum, valid = R.ce_target(g, form, V)
    lse = torch.logsumexp(g["x"].double(), 1).float()       # the statistics handed to the kernel
    lse_v, tsum_v = _vec(lse), _vec(tsum.float())
    labels, labels_b, lam = g["labels"], g["labels_b"], _vec(c["lam"])
    tv = _padded(c["t"], ld, float("nan")) if form == "dense" else None
    for sname in ("scale1", "scaleR"):
        sc = _vec(c[sname])
        per_row = int(sname == "scaleR")
        o = R.Outs(DEV)
        d = o.add("dlogits", (Rr, ldd), BF16)
        if form == "onehot":
            rc = lib.xfm_ce_bwd(x.data_ptr(), ld, Rr, V, labels.data_ptr(), lse_v.data_ptr(), sc.data_ptr(), per_row, d, ldd, _stream())
        elif form == "label":
            rc = lib.xfm_ce_smooth_bwd(x.data_ptr(), ld, Rr, V, labels.data_ptr(), labels_b.data_ptr(), lam.data_ptr(), R.CE_ON, c["off"],
                                       lse_v.data_ptr(), sc.data_ptr(), per_row, d, ldd, _stream())
        else:
            rc = lib.xfm_ce_soft_bwd(x.data_ptr(), ld, tv.data_ptr(), ld, Rr, V, lse_v.data_ptr(), tsum_v.data_ptr(), sc.data_ptr(), per_row, d,
                                     ldd, _stream())
        _lib().check(rc, "ce backward")
        torch.cuda.synchronize()
        o.check_outside()
        got = o["dlogits"]
        ref, b32 = R.ce_bwd_ref(g["x"], lse, t, tsum, g[sname], valid)
        _report("ce_bwd", form, V, f"{sname}:{pad}", R.check_bf16(got[:, :V], ref, b32, f"dlogits ({sname}, padding {pad})"))
        assert bool((got[:, V:].view(torch.int16) == 0).all()), "dlogits padding columns [V, ldd) are not +0"
        if valid is not None:
            assert bool((got[~valid].view(torch.int16) == 0).all()), "an ignored row's dlogits are not +0"


# -------------------------------------------------------------------------------------------------------------------------- forward
def _planted(c, V, where):
    """the case's logits with each row's maximum, 20 above the rest, planted at column `where` (an int, or "label": each row's own label)"""
    x = c["x"].clone()
    if where is None:
        return x
    top = x.max(1).values + 20.0
    cols = c["labels"].clamp(min=0) if where == "label" else torch.full((x.shape[0],), where)
    x[torch.arange(x.shape[0]), cols] = top
    return x


@pytest.mark.parametrize("pad", list(PADS))
@pytest.mark.parametrize("Rr,V,ld", R.CE_SHAPES)
def test_ce_forward_planted_maximum(Rr, V, ld, pad):
    lib = _lib().load()
    c = _case(Rr, V)
    g = _dev(c)
    labels, labels_b, lam = g["labels"], g["labels_b"], _vec(c["lam"])
    tv = _padded(c["t"], ld, float("nan"))
    places = [None] + [w for w in (0, V - 1, V & ~3, (V & ~3) - 1) if 0 <= w < V] + ["label"]
    for where in places:
        xc = _planted(c, V, where)
        x = _padded(xc, ld, PADS[pad])
        xg = xc.to(DEV)
        for form in R.CE_FORMS:
            t, tsum, valid = R.ce_target(g, form, V)
            o = R.Outs(DEV)
            lse_p, loss_p = o.add("lse", (Rr,), F32), o.add("loss", (Rr,), F32)
            if form == "onehot":
                rc = lib.xfm_ce_fwd(x.data_ptr(), ld, Rr, V, labels.data_ptr(), lse_p, loss_p, _stream())
            elif form == "label":
                rc = lib.xfm_ce_smooth_fwd(x.data_ptr(), ld, Rr, V, labels.data_ptr(), labels_b.data_ptr(), lam.data_ptr(), R.CE_ON, c["off"],
                                           lse_p, loss_p, _stream())
            else:
                rc = lib.xfm_ce_soft_fwd(x.data_ptr(), ld, tv.data_ptr(), ld, Rr, V, lse_p, o.add("tsum", (Rr,), F32), loss_p, _stream())
            _lib().check(rc, "ce forward")
            torch.cuda.synchronize()
            o.check_outside()
            lse, b_lse, loss, b_loss = R.ce_fwd_ref(xg, t, t.sum(1) if form == "dense" else tsum, valid)
            what = f"{where}:{pad}"
            _report("ce_fwd", form, V, "lse:" + what, R.check_f32(o["lse"], lse, b_lse, f"lse ({form}, maximum at {where})"))
            _report("ce_fwd", form, V, "loss:" + what, R.check_f32(o["loss"], loss, b_loss, f"loss rows ({form}, maximum at {where})"))
            if form == "dense":
                ts = t.sum(1)
                _report("ce_fwd", form, V, "tsum:" + what, R.check_f32(o["tsum"], ts, U32 * (V + 8) * t.abs().sum(1), "tsum"))
