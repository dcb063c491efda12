"""Host-side proof that attention_util's bounds hold for a correct fp32 evaluation and bite for a wrong one (CPU, no GPU).

1. The fp64 reference agrees with torch autograd on the same formula in fp64 (no dropout): o, dq, dk, dv, dbias to 1e-12 relative.
2. A plain fp32 emulation of the kernels' arithmetic -- online softmax over 64-key chunks, P and dS rounded to bf16 before the second
   product, the backward from a given fp32 lse with delta = sum P dP -- stays within every bound for every case of attention_util.specs(),
   and prints `attn-ratio host <quantity> <family> <ratio>` (pytest -s; family = route-shape-case).  No ratio may pass 0.9: one that does means the
   derivation misses a rounding.
3. Planted faults, applied to the emulation's masks or outputs, land past the bound.
4. test_max_norm_check_misses_what_the_bound_catches: why the bounds exist."""
import functools

import pytest
import torch

import attention_util as A
from attention_util import BF16, F32, SCALE

HOST_MAX = 0.9
SPECS = A.specs()


def _report(sp, what, ratio, limit=HOST_MAX):
    print(f"attn-ratio host {what} {A.spec_id(sp)} {ratio:.3g}")
    assert ratio <= limit, f"{A.spec_id(sp)} {what}: a correct fp32 evaluation at {ratio:.3g} of the bound: the derivation misses a rounding"


def _fails(fn, match="past the bound"):
    with pytest.raises(AssertionError, match=match):
        fn()


def host_mask(sp, seed=7):
    """a Bernoulli keep mask (the kernels' own stream is read off the GPU in tests/test_hip_attention_bounds.py)"""
    if sp.p == 0.0:
        return None
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand((sp.B, sp.H, sp.Sq, sp.Sk), generator=g) >= sp.p


@functools.lru_cache(maxsize=8)
def _case(sp):
    return A.make_case(sp)


# ------------------------------------------------------------------------------------------------------------------- fp32 emulation
def _h32(t):
    return t.permute(0, 2, 1, 3).float()


def emul_scores(c, keep=None, causal_shift=0, leak=None, twice=False, bias=None):
    """fp32 [B, H, Sq, Sk] as score_masked forms them.  Faults: keep (another key mask, [B, Sk] per query row), causal_shift (masked when
    kj > qi + shift), leak (b, h, qi, kj: that score gets no mask term), twice (-10000 per reason), bias (another bias)."""
    sp = c["sp"]
    s = (_h32(c["q"]) @ _h32(c["k"][c["idx"]]).transpose(-1, -2)) * SCALE
    bias = c["bias"] if bias is None else bias
    if bias is not None:
        s = s + bias[:, :, :sp.Sk].unsqueeze(0)
    km = torch.zeros((sp.B, 1, 1, sp.Sk), dtype=torch.bool)
    if c["keep"] is not None:
        km = ((c["keep"][c["idx"]] if keep is None else keep) == 0)[:, None, None, :]
    cm = torch.zeros((1, 1, sp.Sq, sp.Sk), dtype=torch.bool)
    if sp.causal:
        cm = (torch.arange(sp.Sk)[None, :] > torch.arange(sp.Sq)[:, None] + causal_shift)[None, None]
    if twice:
        add = km.float() * A.MASK_NEG + cm.float() * A.MASK_NEG
    else:
        add = (km | cm).float() * A.MASK_NEG
    add = add.expand(sp.B, sp.H, sp.Sq, sp.Sk).clone()
    if leak is not None:
        add[leak] = 0.0
    return s + add


def emul_fwd(c, M=None, ps=None, **faults):
    """-> (o bf16 [B*Sq, H*64], lse fp32 [B*H, Sq])"""
    sp = c["sp"]
    s = emul_scores(c, **faults)
    V = _h32(c["v"][c["idx"]])
    ps = A.drop_scale32(sp.p) if ps is None else ps
    m = torch.full(s.shape[:3], -1.0e30)
    l = torch.zeros(s.shape[:3])
    acc = torch.zeros(s.shape[:3] + (64,))
    for k0 in range(0, sp.Sk, 64):
        sc = s[..., k0:k0 + 64]
        m_new = torch.maximum(m, sc.max(-1).values)
        alpha = torch.exp(m - m_new)
        p = torch.exp(sc - m_new.unsqueeze(-1))
        l = l * alpha + p.sum(-1)
        if M is not None:
            p = torch.where(M[..., k0:k0 + 64], p * ps, torch.zeros(()))
        acc = acc * alpha.unsqueeze(-1) + p.to(BF16).float() @ V[:, :, k0:k0 + 64]
        m = m_new
    o = (acc * (1.0 / l).unsqueeze(-1)).to(BF16)
    return o.permute(0, 2, 1, 3).reshape(sp.B * sp.Sq, sp.H * 64), (m + torch.log(l)).reshape(sp.B * sp.H, sp.Sq)


def emul_bwd(c, lse32, M=None, M_dkv=None, ps=None, dbias_init=A.DBIAS_INIT, **faults):
    """-> dict of delta, dq, dk, dv (per query row; per source when grouped), dbias.  M_dkv: the mask the dK/dV side draws (default M)."""
    sp = c["sp"]
    B, H, Sq, Sk = sp.B, sp.H, sp.Sq, sp.Sk
    s = emul_scores(c, **faults)
    Q, K, V, DO = _h32(c["q"]), _h32(c["k"][c["idx"]]), _h32(c["v"][c["idx"]]), _h32(c["do"])
    ps = A.drop_scale32(sp.p) if ps is None else ps
    P = torch.exp(s - lse32.reshape(B, H, Sq, 1))
    dp0 = DO @ V.transpose(-1, -2)
    one = torch.ones(())
    f = one if M is None else torch.where(M, ps * one, 0 * one)
    fk = f if M_dkv is None else torch.where(M_dkv, ps * one, 0 * one)
    dp = dp0 * f
    delta = (P * dp).sum(-1)
    ds = P * (dp - delta.unsqueeze(-1))
    dq = ((ds.to(BF16).float() @ K) * SCALE).to(BF16)
    ds_k = P * (dp0 * fk - delta.unsqueeze(-1))
    dk = (ds_k.to(BF16).float().transpose(-1, -2) @ Q) * SCALE
    dv = (P * fk).to(BF16).float().transpose(-1, -2) @ DO
    if sp.grouped:
        dk, dv = (torch.zeros((sp.U,) + t.shape[1:]).index_add_(0, c["idx"], t) for t in (dk, dv))
    rows = lambda t, S: t.permute(0, 2, 1, 3).reshape(t.shape[0] * S, H * 64)   # noqa: E731
    out = {"delta": delta.reshape(B * H, Sq), "dq": rows(dq, Sq), "dk": rows(dk.to(BF16), Sk), "dv": rows(dv.to(BF16), Sk)}
    if c["bias"] is not None:
        out["dbias"] = (dbias_init + ds.sum(0)).reshape(H * Sq, Sk)
    return out


CHECK = {"delta": A.check_f32, "dq": A.check_bf16, "dk": A.check_bf16, "dv": A.check_bf16, "dbias": A.check_f32}


# ----------------------------------------------------------------------------------------------------------------------- 1. autograd
@pytest.mark.parametrize("sp", [s for s in SPECS if s.p == 0.0], ids=A.spec_id)
def test_reference_agrees_with_autograd(sp):
    c = _case(sp)
    B, H, Sq, Sk = sp.B, sp.H, sp.Sq, sp.Sk
    leaf = lambda t: t.double().clone().requires_grad_(True)   # noqa: E731
    q, k, v = leaf(c["q"]), leaf(c["k"]), leaf(c["v"])
    bias = leaf(c["bias"]) if sp.bias else None
    s = SCALE * (q.permute(0, 2, 1, 3) @ k[c["idx"]].permute(0, 2, 3, 1))
    if sp.bias:
        s = s + bias[:, :, :Sk]
    s = s + A.MASK_NEG * A.masked_of(c).double()
    o = (s.softmax(-1) @ v[c["idx"]].permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(B * Sq, H * 64)
    o.backward(c["do"].double().reshape(B * Sq, H * 64))
    fr = A.fwd_ref(c)
    br = A.bwd_ref(c, fr["lse"][0])      # the exact lse: the backward is then the gradient of the forward
    per_src = sp.grouped or sp.idx is None

    def rel(got, ref):
        return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))

    assert rel(fr["o"][0], o.detach()) <= 1e-12
    assert rel(br["dq"][0], q.grad.reshape(B * Sq, H * 64)) <= 1e-12
    for name, g in (("dk", k.grad), ("dv", v.grad)):
        got = br[name][0]
        if not per_src:      # per query row: fold as the row-fold kernel does
            got = torch.zeros((sp.U, Sk * H * 64), dtype=torch.float64).index_add_(0, c["idx"], got.reshape(B, -1))
        assert rel(got.reshape(-1), g.reshape(-1)) <= 1e-12, name
    if sp.bias:
        assert rel(br["dbias"][0] - A.DBIAS_INIT, bias.grad[:, :, :Sk].reshape(H * Sq, Sk)) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------- 2. emulation
@pytest.mark.parametrize("sp", SPECS, ids=A.spec_id)
def test_emulation_within_bounds(sp):
    c = _case(sp)
    M = host_mask(sp)
    fr = A.fwd_ref(c, M)
    o, lse = emul_fwd(c, M)
    _report(sp, "o", A.check_bf16(o, *fr["o"], "o"))
    _report(sp, "lse", A.check_f32(lse, *fr["lse"], "lse"))
    lse32 = fr["lse"][0].float()
    br = A.bwd_ref(c, lse32, M)
    got = emul_bwd(c, lse32, M)
    for name, t in got.items():
        _report(sp, name, CHECK[name](t, *br[name], name))


# -------------------------------------------------------------------------------------------------------------------------- 3. faults
def _spec(route, shape, name):
    return next(s for s in SPECS if s.route == route and A.shape_of(s) == shape and s.name == name)


def _fault_ratio(sp, what, fn):
    """the fault must fail the check; prints by how much (the checker's message carries err / bound)"""
    with pytest.raises(AssertionError, match="past the bound") as e:
        fn()
    ratio = float(str(e.value).rsplit("=", 1)[1])
    print(f"attn-fault host {A.spec_id(sp)} {what} {ratio:.3g}")
    assert ratio > 1.0


@pytest.mark.parametrize("shape", ["2x2x30x30", "2x2x65x65", "2x2x300x300", "2x2x20x50"])
def test_fault_causal_off_by_one(shape):
    sp = _spec("causal", shape, "causal")
    c = _case(sp)
    fr = A.fwd_ref(c)
    o, lse = emul_fwd(c, causal_shift=1)
    _fault_ratio(sp, "causal+1:o", lambda: A.check_bf16(o, *fr["o"], "o"))
    _fault_ratio(sp, "causal+1:lse", lambda: A.check_f32(lse, *fr["lse"], "lse"))
    lse32 = fr["lse"][0].float()
    br = A.bwd_ref(c, lse32)
    got = emul_bwd(c, lse32, causal_shift=1)
    for name in ("dq", "dk", "dv"):
        _fault_ratio(sp, "causal+1:" + name, lambda: CHECK[name](got[name], *br[name], name))


def _leak(c):
    """one masked key of one row: (b, h, qi) = (1, 1, 17) and the key, of those entry 1's mask hides, whose unmasked score is nearest 0,
    the scores' mean -- a typical key (it takes about 1 / 200 of the row).  A key 1.5 below the mean moves o by less than its bound and
    is caught by lse alone."""
    hidden = (c["keep"][c["idx"][1]] == 0).nonzero().flatten()
    s = A.scores_ref(c)[0][1, 1, 17, hidden] - A.MASK_NEG
    return (1, 1, 17, int(hidden[s.abs().argmin()]))


@pytest.mark.parametrize("family", ["holes", "tail"])
def test_fault_one_masked_key_visible(family):
    sp = _spec("streamed", "2x2x40x300", family)
    c = _case(sp)
    fr = A.fwd_ref(c)
    o, lse = emul_fwd(c, leak=_leak(c))
    _fault_ratio(sp, "leak:o", lambda: A.check_bf16(o, *fr["o"], "o"))
    _fault_ratio(sp, "leak:lse", lambda: A.check_f32(lse, *fr["lse"], "lse"))
    lse32 = fr["lse"][0].float()
    br = A.bwd_ref(c, lse32)
    got = emul_bwd(c, lse32, leak=_leak(c))
    if family == "holes":      # (the tail family's typical hidden key moves dq by less than its bound: the forward catches it)
        _fault_ratio(sp, "leak:dq", lambda: A.check_bf16(got["dq"], *br["dq"], "dq"))


def test_fault_key_mask_of_the_previous_entry():
    sp = _spec("resident", "2x2x70x130", "tail")
    c = _case(sp)
    fr = A.fwd_ref(c)
    wrong = c["keep"][c["idx"]].roll(1, 0)
    o, lse = emul_fwd(c, keep=wrong)
    _fault_ratio(sp, "keep[b-1]:o", lambda: A.check_bf16(o, *fr["o"], "o"))
    _fault_ratio(sp, "keep[b-1]:lse", lambda: A.check_f32(lse, *fr["lse"], "lse"))
    lse32 = fr["lse"][0].float()
    br = A.bwd_ref(c, lse32)
    got = emul_bwd(c, lse32, keep=wrong)
    _fault_ratio(sp, "keep[b-1]:dk", lambda: A.check_bf16(got["dk"], *br["dk"], "dk"))


@pytest.mark.parametrize("route,shape", [("packed", "3x2x30x30"), ("streamed", "2x2x40x300"), ("grouped", "5x2x30x130")])
def test_fault_dropout(route, shape):
    sp = _spec(route, shape, "holes+p0.1")
    c = _case(sp)
    M = host_mask(sp)
    fr = A.fwd_ref(c, M)
    lse32 = fr["lse"][0].float()
    br = A.bwd_ref(c, lse32, M)
    # one dropped score (of a kept key, in a row of the last batch entry) kept by the dK/dV side only
    b, h, qi = sp.B - 1, 1, 5
    src = int(c["idx"][b])
    cand = (~M[b, h, qi]) & (c["keep"][src] != 0)
    kj = int(cand.nonzero()[0])
    Mk = M.clone()
    Mk[b, h, qi, kj] = True
    got = emul_bwd(c, lse32, M, M_dkv=Mk)
    A.check_bf16(got["dq"], *br["dq"], "dq")
    _fault_ratio(sp, "dkv keeps a dropped score:dk|dv",
                 lambda: (A.check_bf16(got["dv"], *br["dv"], "dv"), A.check_bf16(got["dk"], *br["dk"], "dk")))
    # scale 1 instead of 1 / (1 - p)
    o, _ = emul_fwd(c, M, ps=1.0)
    _fault_ratio(sp, "drop scale 1:o", lambda: A.check_bf16(o, *fr["o"], "o"))
    got = emul_bwd(c, lse32, M, ps=1.0)
    for name in ("dq", "dk", "dv"):
        _fault_ratio(sp, "drop scale 1:" + name, lambda: CHECK[name](got[name], *br[name], name))


def test_fault_mask_added_twice():
    """a key both masked and causally hidden must get -10000 once: in the all-masked entry the row is then a softmax over EVERY key"""
    sp = _spec("causal", "2x2x65x65", "causal+all")
    c = _case(sp)
    fr = A.fwd_ref(c)
    o, lse = emul_fwd(c)
    A.check_bf16(o, *fr["o"], "o")
    A.check_f32(lse, *fr["lse"], "lse")
    o, lse = emul_fwd(c, twice=True)
    _fault_ratio(sp, "mask twice:o", lambda: A.check_bf16(o, *fr["o"], "o"))
    _fault_ratio(sp, "mask twice:lse", lambda: A.check_f32(lse, *fr["lse"], "lse"))
    lse32 = fr["lse"][0].float()
    br = A.bwd_ref(c, lse32)
    got = emul_bwd(c, lse32, twice=True)
    _fault_ratio(sp, "mask twice:dv", lambda: A.check_bf16(got["dv"], *br["dv"], "dv"))


def test_fault_bias_of_the_other_head_and_dbias_overwritten():
    sp = _spec("resident", "2x2x70x130", "holes+bias")
    c = _case(sp)
    fr = A.fwd_ref(c)
    wrong = c["bias"][[0, 0]]
    o, lse = emul_fwd(c, bias=wrong)
    _fault_ratio(sp, "bias[h-1]:o", lambda: A.check_bf16(o, *fr["o"], "o"))
    _fault_ratio(sp, "bias[h-1]:lse", lambda: A.check_f32(lse, *fr["lse"], "lse"))
    lse32 = fr["lse"][0].float()
    br = A.bwd_ref(c, lse32)
    got = emul_bwd(c, lse32, bias=wrong)
    _fault_ratio(sp, "bias[h-1]:dq", lambda: A.check_bf16(got["dq"], *br["dq"], "dq"))
    _fault_ratio(sp, "bias[h-1]:dbias", lambda: A.check_f32(got["dbias"], *br["dbias"], "dbias"))
    got = emul_bwd(c, lse32, dbias_init=0.0)
    _fault_ratio(sp, "dbias = instead of +=:dbias", lambda: A.check_f32(got["dbias"], *br["dbias"], "dbias"))


def test_fault_one_bit_outside_a_view():
    sp = _spec("small", "1x2x30x30", "holes")
    buf = A.AttnBuffers(_case(sp), "cpu")
    o, lse, delta = buf.out16("o", sp.B * sp.Sq), buf.stat("lse"), buf.stat("delta", nan_padding=True)
    o.fill_(0.25)
    lse[:, :sp.Sq] = 1.0
    delta[:, :sp.Sq] = 1.0
    buf.check_outside()
    for name, (r, col), it in (("o", (4, 3), torch.int16), ("o", (3, 40), torch.int16), ("lse", (3, 5), torch.int32),
                               ("lse", (4, sp.Sq), torch.int32), ("delta", (5, sp.Sq + 1), torch.int32)):
        parent = buf.outs[name][0]
        parent.view(it)[r, col] ^= 1
        with pytest.raises(AssertionError, match="written"):
            buf.check_outside()
        parent.view(it)[r, col] ^= 1
    buf.check_outside()
    # the statistics handed to the backward are an input: a value, its NaN padding and the NaN rows around it
    buf.stat("lse_in", given=torch.ones((sp.B * sp.H, sp.Sq)))
    buf.check_outside()
    parent = buf.given["lse_in"][0]
    for r, col in ((4, 2), (4, sp.Sq), (2, 1)):
        parent.view(torch.int32)[r, col] ^= 1
        with pytest.raises(AssertionError, match="written"):
            buf.check_outside()
        parent.view(torch.int32)[r, col] ^= 1
    buf.check_outside()


# ---------------------------------------------------------------------------------------------------------------- 4. why the bounds
def test_max_norm_check_misses_what_the_bound_catches():
    """why these bounds exist, kept as a test: one masked key leaking into one query row at Sk = 300 passes max |err| / max |ref| <= 2e-2,
    the measure of tests/test_hip_kernels.py, on o and on dq; the elementwise bound catches it on both sides of the call"""
    sp = _spec("streamed", "2x2x40x300", "holes")
    c = _case(sp)
    fr = A.fwd_ref(c)
    o, lse = emul_fwd(c, leak=_leak(c))
    assert A.max_norm_err(o, fr["o"][0]) <= 2e-2
    _fails(lambda: A.check_bf16(o, *fr["o"], "o"))
    lse32 = fr["lse"][0].float()
    br = A.bwd_ref(c, lse32)
    got = emul_bwd(c, lse32, leak=_leak(c))
    assert A.max_norm_err(got["dq"], br["dq"][0]) <= 2e-2
    _fails(lambda: A.check_bf16(got["dq"], *br["dq"], "dq"))
    assert bool(torch.isfinite(fr["o"][1]).all()) and bool(torch.isfinite(br["dq"][1]).all())
    assert o.dtype == BF16 and lse.dtype == F32
