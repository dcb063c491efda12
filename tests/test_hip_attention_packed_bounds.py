"""Unpadded token rows, o_lo on masked problems and the split backward, under elementwise fp64 bounds.

xfm_rlayer_fwd / bwd (csrc/encoder.hip) call the attention kernels with q_start / q_len / k_start / k_len (self-attention: both pairs;
range-mode and grouped cross-attention: the query pair), with o_lo on masked, dropped and grouped problems, and with the backward split
into bwd_phase = 1 and bwd_phase = 2; tests/test_hip_attention_bounds.py and tests/test_hip_attention_dense_bounds.py run none of the
three, and tests/test_hip_packing.py holds the packed step to a norm-relative 2e-3 / 5e-3 of the padded one.  Here every case of
attention_util.ragged_specs() goes through xfm_attn_fwd / xfm_attn_bwd directly, its entries' live rows scattered (starts not monotone,
slack rows between) inside NaN-filled inputs and sentinel-filled outputs:

    forward with o_lo requested: o, lse, o + o_lo; then, from an fp32 lse computed here (NaN in the columns [q_len, stat_ld)),
    p0        bwd_phase = 0 without o_lo           delta = sum_j P dP
    p0:lo     bwd_phase = 0 with o_lo              delta = dO . (O + O_lo)  (delta_from_out in all three dQ kernels: C_DELTA_CHAIN)
    split     bwd_phase = 1, then bwd_phase = 2 on the delta the first call left, without and with o_lo

and every element of delta, dq, dk, dv is held to the bound of the per-entry reference (attention_util, "ragged rows").  After every call
the outside of every parent, the statistics' padding AND dead columns [q_len[b], Sq), and the slack rows of o, o_lo, dq, dk, dv must have
kept their bits.  The split run must equal the phase-0 run of the same variant bit for bit on every route: attn_bwd_plan
(csrc/attention.hip) picks p.dq and p.dkv from the same predicates whatever the phase (run_dq / run_dkv only drop one of them), no kernel
reads bwd_phase, and none of these routes sums with atomics; phase 1 must leave dk / dv at the sentinel, phase 2 dq at the sentinel and
delta unchanged.

The dropout keep mask is read off ragged forward calls (q = 0, V = the identity at one key chunk: o = keep / (k_len[b] (1 - p))) and must
equal, on every live (b, h, qi, kj), the mask the same route gives for the dense padded shape: the counters stay laid out for the padded
Sq.  Every check prints `attn-ratio gpu <route> <shape> <case> <quantity> <ratio>`; profiles/tests_attention_packed_bounds.md has the table."""
import ctypes
import functools

import pytest
import torch

import attention_util as A
from attention_util import BF16, F32, SCALE

pytestmark = pytest.mark.gpu

DEV = "cuda"
XFM_E_ARG = -1
SPECS = A.ragged_specs()
CHECK = {"o": A.check_bf16, "lse": A.check_f32, "delta": A.check_f32, "dq": A.check_bf16, "dk": A.check_bf16, "dv": A.check_bf16}
SIDE = {"o": "q", "o_lo": "q", "lse": "stat", "delta": "stat", "dq": "q", "dk": "k", "dv": "k"}


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


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _check(buf, name, got, pair, tag=""):
    """the checker of `name` on what the kernels own; prints the ratio"""
    sp = buf.sp
    live = buf.live[SIDE[name]]
    g = got[:, :sp.Sq] if SIDE[name] == "stat" else got
    print(A.ratio_line(sp, name + tag, CHECK[name](g[live], pair[0][live], pair[1][live], name)))


@functools.lru_cache(maxsize=4)
def _case(sp):
    return A.make_ragged_case(sp)


# ------------------------------------------------------------------------------------------------------------------------- the calls
def _args(buf, o, o_lo, lse, drop):
    sp = buf.sp
    return _lib().AttnArgs(q=buf.q.data_ptr(), q_rs=buf.q.stride(0), k=buf.k.data_ptr(), k_rs=buf.k.stride(0), v=buf.v.data_ptr(),
                           v_rs=buf.v.stride(0), o=o.data_ptr(), o_rs=o.stride(0), o_lo=_ptr(o_lo), lse=lse.data_ptr(), stat_ld=buf.ld_stat,
                           key_keep=_ptr(buf.keep), B=sp.B, H=sp.H, Sq=sp.Sq, Sk=sp.Sk, scale=SCALE, causal=int(sp.causal),
                           drop_thresh=drop[0], drop_scale=drop[1], seed_lo=drop[2], seed_hi=drop[3],
                           grp_start=_ptr(buf.grp_start), grp_rows=_ptr(buf.grp_rows), n_groups=sp.U if sp.grouped else 0,
                           q_start=_ptr(buf.q_start), q_len=_ptr(buf.q_len), k_start=_ptr(buf.k_start), k_len=_ptr(buf.k_len))


def _fwd(buf, drop, with_lo=True, edit=None):
    """one xfm_attn_fwd call -> (rc, o, o_lo, lse); o and o_lo share one row stride (o_rs), as the library addresses them"""
    buf.begin()
    o, lse = buf.rows_out("o", "q"), buf.stat("lse")
    o_lo = buf.rows_out("o_lo", "q") if with_lo else None
    a = _args(buf, o, o_lo, lse, drop)
    if edit is not None:
        edit(a)
    rc = _lib().load().xfm_attn_fwd(ctypes.byref(a), _stream())
    torch.cuda.synchronize()
    return rc, o, o_lo, lse


def _bwd(buf, drop, lse32, o_in, lo_in, phase=0, carry=None, edit=None):
    """one xfm_attn_bwd call from the given statistics -> (rc, dict of the outputs).  carry: the outputs of the phase-1 call whose delta a
    phase-2 call reads (its delta stays registered, so check_outside still guards its padding and dead columns)"""
    buf.begin()
    lse_in = buf.stat("lse_in", given=lse32)
    out = {"dq": buf.rows_out("dq", "q"), "dk": buf.rows_out("dk", "k"), "dv": buf.rows_out("dv", "k")}
    if carry is None:
        out["delta"] = buf.stat("delta", nan_padding=True)
    else:
        out["delta"] = carry["delta"]
        buf.outs.update({k: v for k, v in carry["reg"].items()})
        buf.dead["delta"] = (carry["delta"], True)
    out["reg"] = {k: buf.outs[k] for k in ("delta", "delta:padding")}
    a = _args(buf, o_in, lo_in, lse_in, drop)
    a.dout, a.do_rs = buf.do.data_ptr(), buf.do.stride(0)
    a.dq, a.dq_rs, a.dk, a.dk_rs = out["dq"].data_ptr(), out["dq"].stride(0), out["dk"].data_ptr(), out["dk"].stride(0)
    a.dv, a.dv_rs, a.delta, a.bwd_phase = out["dv"].data_ptr(), out["dv"].stride(0), out["delta"].data_ptr(), phase
    if edit is not None:
        edit(a)
    assert _lib().load().xfm_attn_bwd_workspace(ctypes.byref(a)) == 0
    rc = _lib().load().xfm_attn_bwd(ctypes.byref(a), _stream())
    torch.cuda.synchronize()
    return rc, out


# ------------------------------------------------------------------------------------------------------------------ the dropout mask
@functools.lru_cache(maxsize=64)
def _read_mask(msp, seed=A.SEED):
    """bool [B, H, Sq, Sk] on the GPU, False outside the live corner of every entry: q = 0 and V = the 64 x 64 identity at keys
    [64 c, 64 c + 64): o[row of (b, qi), h, d] = keep(b, h, qi, 64 c + d) / (k_len[b] (1 - p))."""
    B, H, Sq, Sk = msp.B, msp.H, msp.Sq, msp.Sk
    lay = A.ragged_layout(msp)
    c = A.make_ragged_case(msp)
    c["q"] = torch.zeros_like(c["q"])
    M = torch.zeros((B, H, Sq, Sk), dtype=torch.bool, device=DEV)
    for kc in range(A.chunks(Sk)):
        n = min(64, Sk - 64 * kc)
        c["v"] = torch.zeros_like(c["v"])
        c["v"][:, 64 * kc:64 * kc + n] = torch.eye(64, dtype=BF16)[:n].expand(msp.U, H, n, 64).permute(0, 2, 1, 3)
        buf = A.RaggedBuffers(c, DEV)
        rc, o, _, _ = _fwd(buf, _drop(msp.p, seed), with_lo=False)
        assert rc == 0, _lib().load().xfm_last_error()
        buf.check_outside()
        for b in range(B):
            ql, kl = lay.q_len[b], lay.k_len[int(c["idx"][b])]
            m = min(n, kl - 64 * kc)
            if m <= 0:
                continue
            got = o[lay.q_start[b]:lay.q_start[b] + ql].float().reshape(ql, H, 64).permute(1, 0, 2)[..., :m]
            want = 1.0 / (kl * (1.0 - msp.p))
            kept = got != 0
            assert bool(((got - want).abs() <= 2.0 ** -7 * want)[kept].all()), "a kept probability is not 1 / (k_len (1 - p))"
            M[b, :, :ql, 64 * kc:64 * kc + m] = kept
    return M


def _mask_of(sp):
    """the keep mask of sp's route and layout, which must be the dense padded shape's on every live score"""
    if sp.p == 0.0:
        return None
    msp = sp._replace(mask=None, causal=False, score="randn", name=f"mask-p{sp.p}")
    M = _read_mask(msp)
    if sp.q_len is not None:
        dense = _read_mask(msp._replace(q_len=None, k_len=None, layout="dense"))
        lay = A.ragged_layout(sp)
        for b in range(sp.B):
            ql, kl = lay.q_len[b], lay.k_len[int(_case(sp)["idx"][b])]
            diff = int((M[b, :, :ql, :kl] != dense[b, :, :ql, :kl]).sum())
            assert diff == 0, f"entry {b}: {diff} keep decisions differ from the dense padded call's: the counters are not laid out for the padded Sq"
            assert not bool(M[b, :, ql:].any()) and not bool(M[b, :, :, kl:].any())
    return M


# -------------------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("sp", SPECS, ids=A.spec_id)
def test_ragged_attention_within_bounds(sp):
    c = A.to_device(_case(sp), DEV)
    M = _mask_of(sp)
    drop = _drop(sp.p)
    buf = A.RaggedBuffers(c, DEV)
    rc, o, o_lo, lse = _fwd(buf, drop)
    assert rc == 0, _lib().load().xfm_last_error()
    buf.check_outside()
    fr = A.ragged_fwd_ref(c, M)
    _check(buf, "o", o, fr["o"])
    _check(buf, "lse", lse, fr["lse"])
    live = buf.live["q"]
    print(A.ratio_line(sp, "o+o_lo", A.check_o_lo(o[live], o_lo[live], fr["o"][0][live], fr["o"][1][live])))
    # the halves the backward reads: NaN-filled parents of their own (slack rows NaN too), the slices on 16-byte boundaries, one stride
    nan_rows = (~live)[:, None]
    o_in, _ = A.embed(torch.where(nan_rows, torch.full_like(o, A.NAN), o), o.shape[1] + 16, 8, 4, 3, A.NAN)
    lo_in, _ = A.embed(torch.where(nan_rows, torch.full_like(o, A.NAN), o_lo), o.shape[1] + 16, 8, 4, 3, A.NAN)
    lse32 = A.ragged_lse32(fr, sp)
    for tag, lo in (("", None), (":lo", lo_in)):
        br = A.ragged_bwd_ref(c, lse32, M, *((o, o_lo) if lo is not None else ()))
        rc, p0 = _bwd(buf, drop, lse32, o_in, lo)
        assert rc == 0, _lib().load().xfm_last_error()
        buf.check_outside()
        for name in ("delta", "dq", "dk", "dv"):
            _check(buf, name, p0[name], br[name], tag)
        rc, p1 = _bwd(buf, drop, lse32, o_in, lo, phase=1)
        assert rc == 0, _lib().load().xfm_last_error()
        buf.check_outside()
        for name in ("dk", "dv"):
            assert bool((p1[name] == A.SENTINEL).all()), f"phase 1 wrote {name}"
        delta1 = p1["delta"].clone()
        rc, p2 = _bwd(buf, drop, lse32, o_in, lo, phase=2, carry=p1)
        assert rc == 0, _lib().load().xfm_last_error()
        buf.check_outside()
        assert bool((p2["dq"] == A.SENTINEL).all()), "phase 2 wrote dq"
        assert torch.equal(_bits(p2["delta"]), _bits(delta1)), "phase 2 changed delta"
        for name, t in (("delta", p1["delta"]), ("dq", p1["dq"]), ("dk", p2["dk"]), ("dv", p2["dv"])):
            _check(buf, name, t, br[name], tag + ":split")
            assert torch.equal(_bits(t), _bits(p0[name])), f"{name}{tag}: the split backward and bwd_phase = 0 gave different bits"


# ------------------------------------------------------------------------------------------------------------------------- rejections
def _null(*names):
    def edit(a):
        for n in names:
            setattr(a, n, None)
    return edit


def _expect_rejected(sp, edit, extra=None):
    """xfm_attn_fwd and xfm_attn_bwd both answer XFM_E_ARG and write nothing"""
    c = A.to_device(A.make_ragged_case(sp), DEV)
    buf = A.RaggedBuffers(c, DEV)
    if extra is not None:
        extra(buf)
    rc, o, o_lo, lse = _fwd(buf, _drop(0.0), edit=edit)
    assert rc == XFM_E_ARG
    buf.check_outside()
    assert bool((o == A.SENTINEL).all()) and bool((o_lo == A.SENTINEL).all()) and bool((lse == A.SENTINEL).all())
    lse32 = torch.zeros((sp.B * sp.H, sp.Sq), dtype=F32, device=DEV)
    rc, out = _bwd(buf, _drop(0.0), lse32, o, None, edit=edit)
    assert rc == XFM_E_ARG
    buf.check_outside()
    for name in ("dq", "dk", "dv"):
        assert bool((out[name] == A.SENTINEL).all()), name
    live = buf.live["stat"]
    assert bool((out["delta"][:, :sp.Sq][live] == A.SENTINEL).all())


@pytest.mark.parametrize("what", ["q_start without q_len", "k_len without k_start", "bias", "kv_index", "grouped k_start"])
def test_packed_rejections_touch_nothing(what):
    """A start without its len, packed rows with a bias or with kv_index (attn_check), and grouped mode with a packed key side
    (attn_check_grouped: the grouped kernels address source g's keys as rows g Sk .. + Sk and would ignore the pair) are refused on the
    host, before any launch."""
    self_sp = next(s for s in SPECS if s.route == "resident" and s.name.startswith("holes:"))
    keep = []      # (device arrays the edited arguments point at)
    if what == "q_start without q_len":
        _expect_rejected(self_sp, _null("q_len"))
    elif what == "k_len without k_start":
        _expect_rejected(self_sp, _null("k_start"))
    elif what == "bias":
        def edit(a):
            keep.append(torch.zeros((self_sp.H * self_sp.Sq, 132), dtype=F32, device=DEV))
            a.bias, a.bias_ld = keep[-1].data_ptr(), 132
        _expect_rejected(self_sp, edit)
    elif what == "kv_index":
        def edit(a):
            keep.append(torch.zeros(self_sp.B, dtype=torch.int32, device=DEV))
            a.kv_index = keep[-1].data_ptr()
        _expect_rejected(self_sp, edit)
    else:
        sp = next(s for s in SPECS if s.route == "grouped" and s.name.startswith("holes:q") and s.U == 2)

        def edit(a):      # a pair that restates the dense key rows: still refused, the kernels would not read it
            keep.append(torch.tensor([0, sp.Sk], dtype=torch.int32, device=DEV))
            keep.append(torch.tensor([sp.Sk, sp.Sk], dtype=torch.int32, device=DEV))
            a.k_start, a.k_len = keep[0].data_ptr(), keep[1].data_ptr()
        _expect_rejected(sp, edit)
