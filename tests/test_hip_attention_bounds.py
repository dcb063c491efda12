"""The attention routes that take a key mask, a causal mask or dropout, under elementwise fp64 bounds.

tests/test_hip_kernels.py runs the dense kernels at twenty-odd shapes and these routes at a handful, all at max |err| / max |ref| <= 1e-2 or
2e-2: causal at one 30 x 30 shape, key masks as a tail with entry 0 unmasked, dropout against a reference once.  Here every case of
attention_util.specs() -- per shape every key-mask family (ragged tail with entry 0 masked, every third key, a wholly masked first chunk, a
single kept key in the last chunk, a batch entry with every key masked), causal alone, with a tail and with a tail and dropout, dropout at
0.1 and 0.5, steep scores,
with and without a bias -- runs the forward, then the backward from an fp32 lse computed here, through xfm_attn_fwd / xfm_attn_bwd directly,
and every element of o, lse, delta, dq, dk, dv and dbias is held to the bound attention_util derives from the operands (its header has the
counts).  The shapes are the smallest that reach each route (attention_util.SHAPES says which and why).  q, k, v sit in one NaN-filled
parent, the outputs in 7.0-filled ones whose outside must keep its bits; the padding of lse and delta is NaN before the backward; dbias
starts at 0.5; the bias-gradient workspace is exactly as large as the library asks for.  With a bias the backward runs twice: with the
transposed bias copy and (past 256 keys) the workspace, and without either (the dK/dV kernel's strided gather, float atomics).

The dropout keep mask is read off forward calls with q = 0 and V = a 64 x 64 identity at one key chunk (o is then mask / (Sk (1 - p))), one
call per chunk, on the route under test; that mask drives the reference of the forward on random data with key masks and the causal mask
on (holes + p0.1 everywhere, causal + tail + p0.1 on every square), of dQ and of dK/dV (which recomputes the row key per element), and
must be the same on the packed, general and grouped routes.

Every check prints `attn-ratio gpu <route> <shape> <case> <quantity> <worst err / bound>` (pytest -s); profiles/tests_attention_bounds.md holds
the table."""
import ctypes
import functools
import math

import pytest
import torch

import attention_util as A
from attention_util import BF16, F32, SCALE

pytestmark = pytest.mark.gpu

DEV = "cuda"
XFM_E_ARG = -1
SPECS = A.specs()


def _lib():
    from xfm_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _drop(p, seed=A.SEED):
    from xfm_amd import functional as Fx
    return Fx.drop_params(p, seed)


def _report(sp, what, ratio):
    print(A.ratio_line(sp, what, ratio))


@functools.lru_cache(maxsize=4)
def _case(sp):
    return A.make_case(sp)


# ------------------------------------------------------------------------------------------------------------------------- the calls
def _args(buf, o, lse, drop):
    sp = buf.sp
    return _lib().AttnArgs(q=buf.q.data_ptr(), q_rs=buf.q.stride(0), k=buf.k.data_ptr(), k_rs=buf.k.stride(0), v=buf.v.data_ptr(),
                           v_rs=buf.v.stride(0), o=o.data_ptr(), o_rs=o.stride(0), lse=lse.data_ptr(), stat_ld=buf.ld_stat,
                           bias=_ptr(buf.bias), bias_ld=0 if buf.bias is None else buf.bias.stride(0), key_keep=_ptr(buf.keep),
                           B=sp.B, H=sp.H, Sq=sp.Sq, Sk=sp.Sk, scale=SCALE, causal=int(sp.causal),
                           drop_thresh=drop[0], drop_scale=drop[1], seed_lo=drop[2], seed_hi=drop[3],
                           kv_index=_ptr(buf.kv_index), grp_start=_ptr(buf.grp_start), grp_rows=_ptr(buf.grp_rows),
                           n_groups=sp.U if sp.grouped else 0)


def _fwd(buf, drop):
    """one xfm_attn_fwd call -> (rc, o, lse)"""
    buf.begin()
    o, lse = buf.out16("o", buf.sp.B * buf.sp.Sq), buf.stat("lse")
    a = _args(buf, o, lse, drop)
    rc = _lib().load().xfm_attn_fwd(ctypes.byref(a), _stream())
    torch.cuda.synchronize()
    return rc, o, lse


def _bwd(buf, drop, lse32, o, use_bias_t, use_ws):
    """one xfm_attn_bwd call from the given statistics -> (rc, dict of the outputs)"""
    sp = buf.sp
    buf.begin()
    lse_in = buf.stat("lse_in", given=lse32)      # check_outside compares its whole parent with a copy taken here
    n = sp.U if sp.grouped else sp.B
    out = {"delta": buf.stat("delta", nan_padding=True), "dq": buf.out16("dq", sp.B * sp.Sq), "dk": buf.out16("dk", n * sp.Sk),
           "dv": buf.out16("dv", n * sp.Sk)}
    a = _args(buf, o, lse_in, drop)
    a.dout, a.do_rs = buf.do.data_ptr(), buf.do.stride(0)
    a.dq, a.dq_rs, a.dk, a.dk_rs = out["dq"].data_ptr(), out["dq"].stride(0), out["dk"].data_ptr(), out["dk"].stride(0)
    a.dv, a.dv_rs, a.delta = out["dv"].data_ptr(), out["dv"].stride(0), out["delta"].data_ptr()
    if buf.bias is not None:
        out["dbias"] = buf.dbias()
        a.dbias = out["dbias"].data_ptr()
        if use_bias_t:
            a.bias_t, a.bias_t_ld = buf.bias_t.data_ptr(), buf.bias_t.stride(0)
    need = _lib().load().xfm_attn_bwd_workspace(ctypes.byref(a))
    # per-entry planes for a masked problem's bias gradient past 256 keys (attn_bwd_plan: DB_ENTRY_WS), nothing otherwise
    assert need == (sp.B * sp.H * sp.Sq * buf.bias.stride(0) * 4 if buf.bias is not None and sp.Sk > 256 else 0), need
    if use_ws and need > 0:
        a.dbias_ws = buf.workspace(need).data_ptr()
    rc = _lib().load().xfm_attn_bwd(ctypes.byref(a), _stream())
    torch.cuda.synchronize()
    return rc, out


# ------------------------------------------------------------------------------------------------------------------ the dropout mask
def _mask_spec(sp):
    """the call that exposes sp's dropout stream: same route, shape and sources; no key mask, no causal mask"""
    return sp._replace(mask=None, causal=False, score="randn", name=f"mask-p{sp.p}")


@functools.lru_cache(maxsize=64)
def _read_mask(msp, seed=A.SEED):
    """bool [B, H, Sq, Sk] on the GPU: q = 0 (every score 0, every probability 1 / Sk; a zero bias where the route is reached through one)
    and V = the 64 x 64 identity at keys [64 c, 64 c + 64), zero elsewhere: o[b, qi, h, d] = keep(b, h, qi, 64 c + d) / (Sk (1 - p))."""
    B, H, Sq, Sk = msp.B, msp.H, msp.Sq, msp.Sk
    c = A.make_case(msp)
    c["q"] = torch.zeros_like(c["q"])
    if c["bias"] is not None:
        c["bias"] = torch.zeros_like(c["bias"])
    M = torch.zeros((B, H, Sq, Sk), dtype=torch.bool, device=DEV)
    want = 1.0 / (Sk * (1.0 - msp.p))
    for kc in range(A.chunks(Sk)):
        n = min(64, Sk - 64 * kc)
        c["v"] = torch.zeros_like(c["v"])
        c["v"][:, 64 * kc:64 * kc + n] = torch.eye(64, dtype=BF16)[:n].expand(msp.U, H, n, 64).permute(0, 2, 1, 3)
        buf = A.AttnBuffers(c, DEV)
        rc, o, _ = _fwd(buf, _drop(msp.p, seed))
        assert rc == 0
        buf.check_outside()
        got = o.float().reshape(B, Sq, H, 64).permute(0, 2, 1, 3)[..., :n]
        kept = got != 0
        assert bool(((got - want).abs() <= 2.0 ** -7 * want)[kept].all()), "a kept probability is not 1 / (Sk (1 - p))"
        M[..., 64 * kc:64 * kc + n] = kept
    return M


def _mask_of(sp):
    return None if sp.p == 0.0 else _read_mask(_mask_spec(sp))


# -------------------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("sp", SPECS, ids=A.spec_id)
def test_attention_within_bounds(sp):
    c = A.to_device(_case(sp), DEV)
    M = _mask_of(sp)
    drop = _drop(sp.p)
    buf = A.AttnBuffers(c, DEV)
    rc, o, lse = _fwd(buf, drop)
    assert rc == 0, _lib().load().xfm_last_error()
    fr = A.fwd_ref(c, M)
    buf.check_outside()
    _report(sp, "o", A.check_bf16(o, *fr["o"], "o"))
    _report(sp, "lse", A.check_f32(lse[:, :sp.Sq], *fr["lse"], "lse"))
    lse32 = fr["lse"][0].float()
    br = A.bwd_ref(c, lse32, M)
    variants = [("", True, True), (":gather", False, False)] if sp.bias else [("", False, False)]
    for tag, use_bias_t, use_ws in variants:
        rc, out = _bwd(buf, drop, lse32, o, use_bias_t, use_ws)
        assert rc == 0, _lib().load().xfm_last_error()
        buf.check_outside()
        _report(sp, "delta" + tag, A.check_f32(out["delta"][:, :sp.Sq], *br["delta"], "delta"))
        for name in ("dq", "dk", "dv"):
            _report(sp, name + tag, A.check_bf16(out[name], *br[name], name))
        if sp.bias:
            _report(sp, "dbias" + tag, A.check_f32(out["dbias"][:, :sp.Sk], *br["dbias"], "dbias"))
    if sp.route == "kvindex":      # the per-row dK / dV folded onto their sources
        for name in ("dk", "dv"):
            src = out[name].contiguous()
            dst, parent = A.embed(torch.full((sp.U * sp.Sk, sp.H * 64), A.SENTINEL, dtype=BF16, device=DEV), sp.H * 64, 0, 4, 3, A.SENTINEL)
            rc = _lib().load().xfm_rows_index_sum(src.data_ptr(), buf.kv_index.data_ptr(), sp.B, sp.U, sp.Sk * sp.H * 64, dst.data_ptr(), _stream())
            torch.cuda.synchronize()
            assert rc == 0
            A.assert_outside_untouched(parent, dst, A.SENTINEL, name + " fold")
            ref, b32 = A.fold_ref(src.reshape(sp.B, -1), c["idx"], sp.U)
            _report(sp, name + ":fold", A.check_bf16(dst.reshape(sp.U, -1), ref, b32, name + " fold"))


# ---------------------------------------------------------------------------------------------------------------------------- dropout
def _route_spec(route, B, H, Sq, Sk, p, bias=False, idx=None, grouped=False):
    return A.Spec(route, B, H, Sq, Sk, B, idx, grouped, None, False, p, "randn", bias, f"mask-p{p}")


@pytest.mark.parametrize("B,Sq,Sk,p", [(3, 30, 50, 0.1), (2, 30, 130, 0.1), (2, 40, 300, 0.5)])
def test_dropout_mask_is_a_function_of_seed_row_and_key(B, Sq, Sk, p):
    """The keep decision of score (b, h, qi, kj) is the same on every route that reaches the shape: the general kernels (B = 3 at 30 x 50
    through a zero bias, which keeps them off the packed route), the packed forward (30 x 50), the grouped kernels with every row its own
    source (resident at 130 keys, streamed at 300).  The grouped calls give row b the source (b + 1) % B, so a row's place in the group
    list differs from its number: a stream keyed by the group or by the place in it, not by the query row, shows here.  Its rate lies
    within 4 sqrt(p (1 - p) / n) of 1 - p, two calls with one seed give equal bits, another seed gives another mask."""
    H = 2
    rotated = tuple((b + 1) % B for b in range(B))
    general = _read_mask(_route_spec("small", B, H, Sq, Sk, p, bias=Sk <= 64))
    others = {"grouped": _read_mask(_route_spec("grouped", B, H, Sq, Sk, p, idx=rotated, grouped=True)),
              "grouped, rows in order": _read_mask(_route_spec("grouped", B, H, Sq, Sk, p, idx=tuple(range(B)), grouped=True))}
    if Sk <= 64:
        others["packed"] = _read_mask(_route_spec("packed", B, H, Sq, Sk, p))
    for name, m in others.items():
        diff = int((m != general).sum())
        assert diff == 0, f"{name} route: {diff} of {m.numel()} keep decisions differ from the general kernels'"
    n = general.numel()
    rate = float(general.double().mean())
    print(f"attn-keep-rate gpu {B}x{H}x{Sq}x{Sk} p={p} {rate:.5f} ({(rate - (1 - p)) / math.sqrt(p * (1 - p) / n):+.2f} sigma)")
    assert abs(rate - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n), rate
    other_seed = _read_mask(_route_spec("grouped", B, H, Sq, Sk, p, idx=tuple(range(B)), grouped=True), A.SEED + 0x100000001)
    assert not torch.equal(other_seed, general)


@pytest.mark.parametrize("route,shape", [("packed", "3x2x30x30"), ("resident", "2x2x70x130"), ("grouped_stream", "5x2x40x300")])
def test_dropout_same_seed_same_bits(route, shape):
    sp = next(s for s in SPECS if s.route == route and A.shape_of(s) == shape and s.name == "holes+p0.1")
    c = A.to_device(_case(sp), DEV)
    runs = []
    for _ in range(2):
        buf = A.AttnBuffers(c, DEV)
        rc, o, lse = _fwd(buf, _drop(sp.p))
        assert rc == 0
        runs.append((o.clone(), lse[:, :sp.Sq].clone()))
    assert torch.equal(runs[0][0].view(torch.int16), runs[1][0].view(torch.int16)) and torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------------------------------------------------------------- rejections
@pytest.mark.parametrize("what", ["causal", "bias", "Sq>64"])
def test_grouped_rejections_touch_nothing(what):
    """The grouped kernels take no causal mask, no bias and at most 64 queries a row: xfm_attn_fwd / xfm_attn_bwd must say so (XFM_E_ARG) and
    write nothing."""
    sp = A.Spec("grouped", 5, 2, 70 if what == "Sq>64" else 30, 130, 2, (1, 0, 1, 1, 0), True, "holes", what == "causal", 0.0, "randn",
                what == "bias", "rejected-" + what)
    c = A.to_device(A.make_case(sp), DEV)
    buf = A.AttnBuffers(c, DEV)
    rc, o, lse = _fwd(buf, _drop(0.0))
    assert rc == XFM_E_ARG
    buf.check_outside()
    assert bool((o == A.SENTINEL).all()) and bool((lse == A.SENTINEL).all())
    lse32 = torch.zeros((sp.B * sp.H, sp.Sq), dtype=F32, device=DEV)
    rc, out = _bwd(buf, _drop(0.0), lse32, o, False, False)
    assert rc == XFM_E_ARG
    buf.check_outside()
    for name in ("dq", "dk", "dv"):
        assert bool((out[name] == A.SENTINEL).all()), name
    assert bool((out["delta"][:, :sp.Sq] == A.SENTINEL).all())
    if "dbias" in out:
        assert bool((out["dbias"] == A.DBIAS_INIT).all())

