"""The embedding + LayerNorm kernels (embedding.hip: emb_fwd_kernel<3 / 4>, emb_bwd_kernel<3 / 4>) under elementwise fp64 bounds.

tests/test_hip_kernels.py runs them at D = 768, T = 30 and at most 1440 rows and accepts y at 1e-2 of the tensor's largest value.  The cases
here (token_rows_util.EMB_CASES; tests/test_token_rows_host.py asserts that each has the property it is named for) cover D = 1024, rows
longer than one 64-token ballot with pads at the head, the tail and across position 64, an all-pad row, fewer than 16 rows, row counts past
the backward's and the forward's grid caps with a vocabulary small enough for hundreds of hits a table row, pos_mode 1, a row_map with
skipped rows, the fp32 gradient twin, and dropout.  The forward and the atomic backward go through the C ABI, so every output sits in a
7.0-filled parent whose outside must keep its bits and every input in a NaN-filled one; the backward takes fp32 statistics computed here
(NaN on rows the row_map skips).  The ordered backward (XFM_DETERMINISTIC=1: dz_out + rows_segment_sum) runs through
functional.embed_ln_bwd against the same bounds and must repeat bit for bit.

Every check prints `token-ratio gpu <kernel> <case> <width> <quantity> <worst err / bound>` (pytest -s); profiles/tests_token_rows_bounds.md
holds the table."""
import ctypes
import functools

import pytest
import torch

import token_rows_util as T
from token_rows_util import BF16, EPS, F32, I32, PAD

pytestmark = pytest.mark.gpu

DEV = "cuda"
NO_DROP = (0, 1.0, 0, 0)


def _lib():
    from xfm_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


rep = T.reporter("gpu")


@functools.lru_cache(maxsize=2)
def _case(name):
    return T.emb_case(name)


class _Call:
    """the inputs of one call as views of NaN-filled parents, by name in `t` (ids and row_map as they are: an integer has no poison that
    is safe to read), and the EmbedArgs that points at them"""

    def __init__(self, c, drop, w=None, b=None):
        self.c = c
        self.t = {"ids": c["ids"].to(DEV).contiguous(), "row_map": None if c["row_map"] is None else c["row_map"].to(DEV).contiguous()}
        for k, v in (("word", c["word"]), ("pos", c["pos"]), ("typ", c["typ"]), ("w", c["w"] if w is None else w), ("b", c["b"] if b is None else b)):
            self.inp(k, v)
        t = self.t
        self.args = _lib().EmbedArgs(pos_mode=c["pos_mode"], ids=t["ids"].data_ptr(), word=t["word"].data_ptr(), pos=t["pos"].data_ptr(),
                                     type=t["typ"].data_ptr(), w=t["w"].data_ptr(), b=t["b"].data_ptr(), B=c["B"], T=c["T"], pad_id=PAD,
                                     eps=EPS, drop_thresh=drop[0], drop_scale=drop[1], seed_lo=drop[2], seed_hi=drop[3])
        if t["row_map"] is not None:
            self.args.row_map = t["row_map"].data_ptr()

    def inp(self, name, v):
        self.t[name] = T.poisoned_in(v, DEV)
        return self.t[name].data_ptr()


def _fwd(c, drop=NO_DROP, w=None, b=None):
    call = _Call(c, drop, w, b)
    a, o = call.args, T.Outs(DEV)
    D, rows, orows = c["D"], c["rows"], c["out_rows"]
    a.y, a.y32 = o.add("y", (orows, D), BF16), o.add("y32", (orows, D), F32)
    a.mean, a.rstd, a.pos_ids = o.add("mean", (rows,), F32), o.add("rstd", (rows,), F32), o.add("pos_ids", (rows,), F32)
    rc = _lib().load().xfm_embed_ln_fwd(ctypes.byref(a), D, _stream())
    torch.cuda.synchronize()
    _lib().check(rc, "embed_ln_fwd")
    o.check_outside()
    return {"y": o["y"], "y32": o["y32"], "mean": o["mean"], "rstd": o["rstd"], "pos_ids": o["pos_ids"].view(I32)}


def _bwd_outs(c):
    o = T.Outs(DEV)
    V, D = c["word"].shape
    ptr = {"dword": o.add("dword", (V, D), F32, c["dword0"]), "dpos": o.add("dpos", tuple(c["dpos0"].shape), F32, c["dpos0"])}
    for q in ("dgamma", "dbeta", "dtype"):
        ptr[q] = o.add(q, (D,), F32, c[q + "0"])
    return o, ptr


def _bwd(c, stats, use_dy32, drop=NO_DROP, dz_out=False):
    """one xfm_embed_ln_bwd call through the C ABI, the workspace exactly as large as the library asks for"""
    lib = _lib().load()
    call = _Call(c, drop)
    a = call.args
    D, rows = c["D"], c["rows"]
    mean, rstd, pid32 = stats
    a.mean, a.rstd = call.inp("mean", mean), call.inp("rstd", rstd)
    pid = pid32.to(DEV)
    a.pos_ids, a.dy = pid.data_ptr(), call.inp("dy", c["dy"])
    if use_dy32:
        a.dy32 = call.inp("dy32", c["dy32"])
    o, ptr = _bwd_outs(c)
    a.dword, a.dpos = ptr["dword"], ptr["dpos"]
    if dz_out:
        a.dz_out = o.add("dz", (rows, D), F32)
    nb = lib.xfm_embed_ln_bwd_workspace(rows, D)
    assert nb == 3 * T.emb_bwd_grid(rows) * D * 4
    wsv, wsp = T.embed_vec(torch.zeros(nb // 4, dtype=F32, device=DEV), 64, 64, T.SENTINEL)
    rc = lib.xfm_embed_ln_bwd(ctypes.byref(a), D, ptr["dgamma"], ptr["dbeta"], ptr["dtype"], wsv.data_ptr(), nb, _stream())
    torch.cuda.synchronize()
    _lib().check(rc, "embed_ln_bwd")
    o.check_outside()
    T.assert_outside_untouched(wsp, wsv, T.SENTINEL, "workspace")
    return o


def _bwd_ordered(c, stats, use_dy32, drop=NO_DROP):
    """functional.embed_ln_bwd (the caller sets XFM_DETERMINISTIC=1) on the same poisoned layout"""
    from xfm_amd import functional as Fx
    mean, rstd, pid32 = stats
    t = {k: T.poisoned_in(c[k], DEV) for k in ("word", "pos", "typ", "w", "b", "dy")}
    dy32 = T.poisoned_in(c["dy32"], DEV) if use_dy32 else None
    rm = None if c["row_map"] is None else c["row_map"].to(DEV)
    o, _ = _bwd_outs(c)
    Fx.embed_ln_bwd(t["dy"], c["ids"].to(DEV).contiguous(), t["word"], t["pos"], t["typ"], t["w"], t["b"], EPS, PAD, T.poisoned_in(mean, DEV),
                    T.poisoned_in(rstd, DEV), pid32.to(DEV), o["dword"], o["dpos"], o["dtype"], o["dgamma"], o["dbeta"], drop=drop,
                    pos_mode=c["pos_mode"], row_map=rm, dy32=dy32)
    torch.cuda.synchronize()
    o.check_outside()
    return o


def _got(o):
    return {q: o[q] for q in ("dword", "dpos", "dgamma", "dbeta", "dtype")}


@pytest.mark.parametrize("name", sorted(T.EMB_CASES))
def test_embedding_forward_within_bounds(name):
    c = _case(name)
    T.check_emb_fwd(T.dev(c, DEV), _fwd(c), rep)


@pytest.mark.parametrize("name", sorted(T.EMB_CASES))
def test_embedding_backward_atomic_and_ordered_within_bounds(name, monkeypatch):
    c = _case(name)
    g = T.dev(c, DEV)
    stats = T.emb_stats(c)
    sd = tuple(s.to(DEV) for s in stats)
    lr = T.emb_live(g)[0]
    monkeypatch.setenv("XFM_DETERMINISTIC", "0")
    for use32 in (False, True):
        ref = T.emb_bwd_ref(g, *sd, use32)
        tag = "dy32:" if use32 else ""
        T.check_emb_bwd(g, _got(_bwd(c, stats, use32)), ref, rep, tag=tag + "atomic:")
        # dz_out: the per-token gradient is stored by unpacked row, skipped rows and both tables keep every bit
        o = _bwd(c, stats, use32, dz_out=True)
        rep("emb_bwd", name, c["D"], tag + "dz", T.check_f32(o["dz"][lr], *ref["dz"], "dz"), "f32")
        if c["row_map"] is not None:
            dead = g["row_map"] < 0
            T.check_equal(o["dz"][dead], torch.full((int(dead.sum()), c["D"]), T.SENTINEL, device=DEV), "dz rows of skipped tokens")
        T.check_equal(o["dword"].contiguous(), g["dword0"], "dword with dz_out")
        T.check_equal(o["dpos"].contiguous(), g["dpos0"], "dpos with dz_out")
        for q in ("dgamma", "dbeta", "dtype"):
            rep("emb_bwd", name, c["D"], tag + "dz_out:" + q, T.check_f32(o[q], *ref[q], q), "f32")
    monkeypatch.setenv("XFM_DETERMINISTIC", "1")
    first = _got(_bwd_ordered(c, stats, True))
    T.check_emb_bwd(g, first, ref, rep, tag="dy32:ordered:")
    again = _got(_bwd_ordered(c, stats, True))
    for q in first:
        assert T.bits_equal(first[q].contiguous(), again[q].contiguous()), f"{q}: the ordered form differs between two calls"


def test_embedding_dropout_one_mask_forward_backward_with_and_without_row_map(monkeypatch):
    """p = 0.1 on 780 x 768 elements.  The mask is read off a forward with w = 0, b = 1 (y32 = keep ? scale : 0 exactly), once with the
    row_map and once without: it is keyed by the unpacked row, so both give one mask.  The forward and both backward forms on real data
    must then have used exactly that mask; its kept fraction lies within 5 binomial standard deviations of 0.9."""
    from xfm_amd import functional as Fx
    c = _case(T.DROP_CASE)
    g = T.dev(c, DEV)
    D, rows = c["D"], c["rows"]
    drop = Fx.drop_params(T.DROP_P, T.DROP_SEED)
    scale = torch.tensor(drop[1], dtype=F32, device=DEV)
    zero_w, one_b = torch.zeros(D), torch.ones(D)
    flat = dict(c, row_map=None, out_rows=rows, dy=T.randn((rows, D), 1.0, 1).to(BF16))
    probe = _fwd(flat, drop, zero_w, one_b)["y32"]
    assert bool(((probe == 0) | (probe == scale)).all()), "the probe's y32 is not keep ? scale : 0"
    keep = probe != 0
    frac = T.check_keep_fraction(keep, T.DROP_P)
    print(f"token-keep-rate gpu emb {rows}x{D} p={T.DROP_P} {frac:.5f}")
    lr, orow = T.emb_live(g)
    packed = _fwd(c, drop, zero_w, one_b)["y32"]
    assert torch.equal(packed[orow] != 0, keep[lr]), "the mask depends on the row_map"
    T.check_keep_fraction(keep[lr], T.DROP_P)
    other = _fwd(flat, Fx.drop_params(T.DROP_P, T.DROP_SEED + 1), zero_w, one_b)["y32"] != 0
    assert not torch.equal(other, keep), "the mask does not depend on the seed"
    T.check_emb_fwd(g, _fwd(c, drop), rep, keep, drop[1], tag="drop:")
    stats = T.emb_stats(c)
    ref = T.emb_bwd_ref(g, *(s.to(DEV) for s in stats), True, keep, drop[1])
    monkeypatch.setenv("XFM_DETERMINISTIC", "0")
    T.check_emb_bwd(g, _got(_bwd(c, stats, True, drop)), ref, rep, tag="drop:atomic:")
    o = _bwd(c, stats, True, drop, dz_out=True)
    rep("emb_bwd", c["name"], D, "drop:dz", T.check_f32(o["dz"][lr], *ref["dz"], "dz"), "f32")
    monkeypatch.setenv("XFM_DETERMINISTIC", "1")
    T.check_emb_bwd(g, _got(_bwd_ordered(c, stats, True, drop)), ref, rep, tag="drop:ordered:")
