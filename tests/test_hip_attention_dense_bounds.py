"""The dense attention routes -- no mask, no dropout, no packing: where training spends its attention time -- under elementwise fp64 bounds
inside poisoned buffers, as tests/test_hip_attention_bounds.py holds the masked ones.

Every case of attention_util.dense_specs() names the route it is meant to reach; attention_util.dense_plan restates the library's choice and
the observable part of it is pinned here: xfm_attn_bwd_workspace must report `planes` [H, Sq, bias_ld] fp32 planes for every variant.  Per
spec the forward runs through xfm_attn_fwd (row-major bias, and the tiled copy of xfm_bias_tile on the ViT forward), writing o, lse and the
low half o_lo; the backward runs from an fp32 lse computed here through xfm_attn_bwd in every variant the route has:
    (base)    transposed bias copy and a workspace offered
    gather    neither (the dK/dV kernels' strided gather or the general dK/dV; atomics, or one slice in place)
    tiled     the accumulator-layout copies (the long kernels, square shapes)
    pre1      XFM_ATTN_SHORT_PRE=1 without o_lo: must change no bit of delta, dq, dk, dv
    pre+lo    XFM_ATTN_SHORT_PRE=1 with o_lo: delta = dO . (O + O_lo)                   (the short dQ kernel)
    lo        o_lo present: the same delta                                             (the long dQ kernel)
    det       XFM_DETERMINISTIC=1: one plane per slice of the short dQ kernel, equal bits on two launches
    vit3      XFM_ATTN_VIT_BWD=3: the opt-in single pass (13-tile shapes, tiled bias): delta = dO . O with the bf16 O
    vit4      XFM_ATTN_VIT_BWD=4: the single pass without its bias-gradient sums + the bias-gradient kernel of the long route
and every element of o, lse, o + o_lo, delta, dq, dk, dv, dbias is held to the bound attention_util derives for the kernels the variant runs
(its header has the counts per family).  Operands are column slices of NaN-filled parents, bias rows end in NaN padding, outputs sit in
7.0-filled parents, dbias starts at 0.5 with its columns [Sk, ld) bit-unchanged, the statistics' padding is NaN before the backward, the
workspace is exactly as large as the library asks for.

Equal bits, from the code: the ViT forward forms fl(bias fl(1 / scale)) whichever copy it reads (o, lse, o_lo: row-major == tiled); no dQ
kernel reads the transposed copy or the workspace (dq, delta: base == gather); the general dK/dV kernel gathers the values the transposed
copy holds, and the short one never reads it (dk, dv: base == gather where both run the same dK/dV kernel); the long kernels form
fma(bias / scale, c2, .) from the tiled copy and fma(bias, log2 e, .) from the row-major one: NOT equal, each within the bound.  The
bias-gradient kernel of the long route has no atomics, in place or in planes: equal bits on two launches.

Every check prints `attn-ratio gpu <route> <shape> <case> <quantity> <worst err / bound>` (pytest -s); profiles/tests_attention_dense_bounds.md
holds the table."""
import ctypes
import functools

import pytest
import torch

import attention_util as A
from attention_util import BF16, F32, SCALE

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPECS = A.dense_specs()
KNOBS = ("XFM_ATTN_VIT_BWD", "XFM_ATTN_SHORT_PRE", "XFM_DETERMINISTIC")


def _mod():
    from xfm_amd import _lib
    return _lib


def _lib():
    return _mod().load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _report(sp, what, ratio):
    print(A.ratio_line(sp, what, ratio))
    return ratio


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


@functools.lru_cache(maxsize=2)
def _case(sp):
    return A.make_case(sp)


def _tiles(buf):
    """(tiled, tiled_t) of buf.bias by xfm_bias_tile, each on a 16-byte boundary inside a 7.0-filled parent"""
    sp = buf.sp
    T = A.cdiv(sp.Sq, 16)
    tiled, _ = A.embed_vec(torch.full((sp.H * T * T * 256,), A.SENTINEL, dtype=F32, device=DEV), 8, 8, A.SENTINEL)
    tiled_t, _ = A.embed_vec(torch.full((sp.H * (T + 1) * T * 256,), A.SENTINEL, dtype=F32, device=DEV), 8, 8, A.SENTINEL)
    rc = _lib().xfm_bias_tile(buf.bias.data_ptr(), sp.H, sp.Sq, buf.bias.stride(0), SCALE, tiled.data_ptr(), tiled_t.data_ptr(), _stream())
    assert rc == 0, _lib().xfm_last_error()
    return tiled, tiled_t


def _args(buf, o, lse, tiles=None):
    sp = buf.sp
    a = _mod().AttnArgs(q=buf.q.data_ptr(), q_rs=buf.q.stride(0), k=buf.k.data_ptr(), k_rs=buf.k.stride(0), v=buf.v.data_ptr(),
                        v_rs=buf.v.stride(0), o=o.data_ptr(), o_rs=o.stride(0), lse=lse.data_ptr(), stat_ld=buf.ld_stat,
                        bias=_ptr(buf.bias), bias_ld=0 if buf.bias is None else buf.bias.stride(0),
                        B=sp.B, H=sp.H, Sq=sp.Sq, Sk=sp.Sk, scale=SCALE, drop_scale=1.0)
    if tiles is not None:
        a.bias_tiled, a.bias_t_tiled = tiles[0].data_ptr(), tiles[1].data_ptr()
    return a


def _fwd(buf, tiles=None):
    """one xfm_attn_fwd call -> (o, o_lo, lse)"""
    buf.begin()
    n = buf.sp.B * buf.sp.Sq
    o, o_lo, lse = buf.out16("o", n), buf.out16("o_lo", n), buf.stat("lse")
    a = _args(buf, o, lse, tiles)
    a.o_lo = o_lo.data_ptr()
    rc = _lib().xfm_attn_fwd(ctypes.byref(a), _stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib().xfm_last_error()
    buf.check_outside()
    return o, o_lo, lse


def _bwd(buf, lse32, o, o_lo, use_bias_t, tiles, use_ws, planes):
    """one xfm_attn_bwd call from the given statistics -> dict of the outputs"""
    sp = buf.sp
    buf.begin()
    lse_in = buf.stat("lse_in", given=lse32)
    out = {"delta": buf.stat("delta", nan_padding=True), "dq": buf.out16("dq", sp.B * sp.Sq), "dk": buf.out16("dk", sp.B * sp.Sk),
           "dv": buf.out16("dv", sp.B * sp.Sk)}
    a = _args(buf, o, lse_in, tiles)
    a.o_lo = _ptr(o_lo)
    a.dout, a.do_rs = buf.do.data_ptr(), buf.do.stride(0)
    a.dq, a.dq_rs, a.dk, a.dk_rs = out["dq"].data_ptr(), out["dq"].stride(0), out["dk"].data_ptr(), out["dk"].stride(0)
    a.dv, a.dv_rs, a.delta = out["dv"].data_ptr(), out["dv"].stride(0), out["delta"].data_ptr()
    if buf.bias is not None:
        out["dbias"] = buf.dbias()
        a.dbias = out["dbias"].data_ptr()
        if use_bias_t:
            a.bias_t, a.bias_t_ld = buf.bias_t.data_ptr(), buf.bias_t.stride(0)
    need = _lib().xfm_attn_bwd_workspace(ctypes.byref(a))
    ld = 0 if buf.bias is None else buf.bias.stride(0)
    assert need == planes * sp.H * sp.Sq * ld * 4, f"workspace of {need} bytes, the restated plan has {planes} planes"
    if use_ws and need > 0:
        a.dbias_ws = buf.workspace(need).data_ptr()
    rc = _lib().xfm_attn_bwd(ctypes.byref(a), _stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib().xfm_last_error()
    buf.check_outside()
    return out


def _variants(sp):
    """(tag, bias_t, tiled, o_lo, workspace offered, knobs, launches)"""
    rt = sp.want
    v = [("", True, False, False, True, {}, 2 if rt.dq == "long" else 1)]      # the long route: no atomics anywhere, launched twice
    if sp.bias:
        v.append(("gather", False, False, False, False, {}, 1))
        if sp.Sq == sp.Sk and rt.dq == "long":
            v.append(("tiled", True, True, False, True, {}, 1))
    if rt.dq == "short":
        v.append(("pre1", True, False, False, True, {"XFM_ATTN_SHORT_PRE": "1"}, 1))
        v.append(("pre+lo", True, False, True, True, {"XFM_ATTN_SHORT_PRE": "1"}, 1))
        if sp.bias and rt.slices > 1 and sp.route == "short_slices":
            v.append(("det", True, False, False, True, {"XFM_DETERMINISTIC": "1"}, 2))
    if rt.dq == "long":
        v.append(("lo", True, False, True, True, {}, 1))
    if rt.fwd == "vit13":      # the opt-in single pass: 13 tiles, the bias through its tiled copies only
        v.append(("vit3", True, True, False, True, {"XFM_ATTN_VIT_BWD": "3"}, 1))
        if sp.bias:
            v.append(("vit4", True, True, False, True, {"XFM_ATTN_VIT_BWD": "4"}, 2))
    return v


def _plan(sp, use_bias_t, tiled, with_lo, use_ws, knobs):
    return A.dense_plan(sp, bias_t=use_bias_t, tiled=tiled, o_lo=with_lo, have_ws=use_ws, vit_mode=int(knobs.get("XFM_ATTN_VIT_BWD", "0")),
                        pre=knobs.get("XFM_ATTN_SHORT_PRE") == "1", det=knobs.get("XFM_DETERMINISTIC") == "1")


@pytest.mark.parametrize("sp", SPECS, ids=A.spec_id)
def test_dense_attention_within_bounds(sp, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    assert A.dense_plan(sp) == sp.want, "the spec no longer reaches the route it names"
    c = A.to_device(_case(sp), DEV)
    buf = A.AttnBuffers(c, DEV)
    fam_f = A.dense_families(sp.want)[0]
    fr = A.dense_fwd_ref(c, fam_f)
    tiles = _tiles(buf) if sp.bias and sp.Sq == sp.Sk and (fam_f == "vit" or sp.want.dq == "long") else None
    runs = {}
    for tag, tl in [("", None)] + ([(":tiled", tiles)] if tiles is not None and fam_f == "vit" else []):
        o, o_lo, lse = _fwd(buf, tl)
        _report(sp, "o" + tag, A.check_bf16(o, *fr["o"], "o"))
        _report(sp, "lse" + tag, A.check_f32(lse[:, :sp.Sq], *fr["lse"], "lse"))
        _report(sp, "o+o_lo" + tag, A.check_o_lo(o, o_lo, *fr["o"]))
        runs[tag] = (o.clone(), o_lo.clone(), lse[:, :sp.Sq].clone())
    if ":tiled" in runs:
        for name, x, y in zip(("o", "o_lo", "lse"), runs[""], runs[":tiled"]):
            assert torch.equal(_bits(x), _bits(y)), f"{name}: the row-major and the tiled bias gave different bits"
    if not sp.bwd:
        return
    o, o_lo, _ = runs[""]
    # the buffers the backward reads o / o_lo from: NaN-filled parents of their own, the slices on 16-byte boundaries
    o_in, _ = A.embed(o, o.shape[1] + 16, 8, 4, 3, A.NAN)
    lo_in, _ = A.embed(o_lo, o.shape[1] + 16, 8, 4, 3, A.NAN)
    lse32 = fr["lse"][0].float()
    refs, got = {}, {}
    for tag, use_bias_t, tiled, with_lo, use_ws, knobs, launches in _variants(sp):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, val in knobs.items():
            monkeypatch.setenv(k, val)
        rt = _plan(sp, use_bias_t, tiled, with_lo, use_ws, knobs)
        planes = _plan(sp, use_bias_t, tiled, with_lo, True, knobs).planes     # what the library asks for, taken or not
        assert (rt.dq == "vit3") == ("XFM_ATTN_VIT_BWD" in knobs), "the single pass must take the 13-tile shapes it is asked for, and only those"
        _, fam_q, fam_k = A.dense_families(rt)
        from_out = (with_lo and rt.dq in ("short_pre", "long")) or rt.dq == "vit3"
        key = (fam_q, fam_k, A.dense_flushes(sp, rt), from_out and rt.dq, rt.dbias)
        if key not in refs:
            given = None
            if from_out:      # the single pass: dO . O with the bf16 O alone
                given = A.delta_out_ref(c, o, torch.zeros_like(o_lo) if rt.dq == "vit3" else o_lo,
                                        A.C_DELTA_DOT if rt.dq == "short_pre" else A.C_DELTA_CHAIN)
            refs[key] = A.dense_bwd_ref(c, lse32, fam_q, fam_k, key[2], given, fam_b="long" if rt.dq == "vit3" and rt.dbias == "blocks" else None,
                                        delta_in_acc=rt.dq == "vit3")
        br = refs[key]
        sfx = ":" + tag if tag else ""
        for launch in range(launches):
            out = _bwd(buf, lse32, o_in, lo_in if with_lo else None, use_bias_t, tiles if tiled and sp.bias else None, use_ws, planes)
            _report(sp, "delta" + sfx, A.check_f32(out["delta"][:, :sp.Sq], *br["delta"], "delta"))
            for name in ("dq", "dk", "dv"):
                _report(sp, name + sfx, A.check_bf16(out[name], *br[name], name))
            if sp.bias:
                _report(sp, "dbias" + sfx, A.check_f32(out["dbias"][:, :sp.Sk], *br["dbias"], "dbias"))
            kept = {k: v.clone() for k, v in out.items()}
            if launch == 1:      # no atomics anywhere on this variant's path to the named outputs
                same = ("delta", "dq", "dk", "dv") + (("dbias",) if rt.dbias in ("blocks", "short_planes") else ())
                for name in same:
                    assert torch.equal(_bits(kept[name]), _bits(got[tag][0][name])), f"{name} ({tag or 'base'}): two launches gave different bits"
            got[tag] = (kept, rt)
    base, base_rt = got[""]
    for tag, names in (("gather", ("delta", "dq")), ("pre1", ("delta", "dq", "dk", "dv")), ("det", ("delta", "dq", "dk", "dv"))):
        if tag in got:
            other, rt = got[tag]
            if tag == "gather" and rt.dkv == base_rt.dkv and rt.dkv in ("short", "general"):
                names = names + ("dk", "dv")
            for name in names:
                assert torch.equal(_bits(base[name]), _bits(other[name])), f"{name}: base and {tag} gave different bits"


def test_every_dense_route_is_reached():
    """The union of the routes the variants of the suite reach, by the restatement the workspace sizes pin."""
    seen = set()
    for sp in SPECS:
        c, grid, last = A.vit_map(sp.B, sp.H)
        if sp.route == "vit_walk":
            assert c == 2 and 0 < last < c, "a walking spec must give two items a workgroup and a shorter last workgroup"
        seen.add(("fwd", sp.want.fwd))
        if not sp.bwd:
            continue
        for tag, use_bias_t, tiled, with_lo, use_ws, knobs, _ in _variants(sp):
            rt = _plan(sp, use_bias_t, tiled, with_lo, use_ws, knobs)
            seen |= {("dq", rt.dq, A.attn_short_dq_np(sp.Sk) if rt.dq.startswith("short") else 0), ("dkv", rt.dkv), ("dbias", rt.dbias, rt.planes > 0)}
            if rt.dq == "sums":
                seen.add(("sums nb", rt.nb))
    want = {("fwd", "vit13"), ("fwd", "vit_rt"), ("fwd", "plain_res"), ("fwd", "plain_stream"),
            ("dq", "short", 4), ("dq", "short", 7), ("dq", "short", 8), ("dq", "short_pre", 4), ("dq", "short_pre", 7), ("dq", "short_pre", 8),
            ("dq", "sums", 0), ("dq", "long", 0), ("dq", "vit3", 0), ("dkv", "vit3"), ("dkv", "short"), ("dkv", "general"), ("dkv", "long"),
            ("dbias", "atomics", False), ("dbias", "sums", False), ("dbias", "short_planes", True), ("dbias", "blocks", True),
            ("dbias", "blocks", False), ("sums nb", 1), ("sums nb", 2), ("sums nb", 4)}
    assert want <= seen, sorted(want - seen, key=str)
