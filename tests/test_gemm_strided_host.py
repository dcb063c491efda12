"""The strided-GEMM checker (gemm_strided_util) has teeth, shown on the CPU: a plain fp32 stand-in "kernel" that reads the operand
views and writes the output view passes every check in both layouts of tests/test_hip_gemm_strided.py, and each broken stand-in --
one k-term dropped, a read one column left of the view, a read of row M of the parent, a sentinel right of column N overwritten, two B
rows swapped, the parent's ld taken for K -- fails."""
import pytest
import torch

import gemm_strided_util as U

BF16, F32 = torch.bfloat16, torch.float32
SHAPES = [(300, 200, 128), (83, 128, 256), (1100, 1001, 64)]
LAYOUTS = ["tight", "block"]


def _rand(shape, scale, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _embed_in(t, layout, pad):
    """tight: the view starts 8 elements into rows of cols + pad, 3 poisoned rows before and 5 after; block: the middle third of a
    3 * cols wide parent."""
    C = t.shape[1]
    return U.embed(t, C + pad, 8, 3, 5, U.NAN) if layout == "tight" else U.embed(t, 3 * C, C, 3, 5, U.NAN)


def _embed_out(M, N, dtype, layout, init=U.SENTINEL):
    t = torch.full((M, N), init, dtype=dtype)
    return U.embed(t, (N + 7) // 8 * 8 + 16, 8, 3, 5, U.SENTINEL) if layout == "tight" else U.embed(t, 3 * N, N, 3, 5, U.SENTINEL)


_CASES = {}


def _case(shape, layout):
    """Operands, their views and the fp64 reference of one (shape, layout), made once and never written."""
    key = (shape, layout)
    if key not in _CASES:
        M, N, K = shape
        a, b, bias = _rand((M, K), 1.0, BF16, 1), _rand((N, K), 0.05, BF16, 2), _rand((N,), 0.5, F32, 3)
        (av, ap), (bv, bp) = _embed_in(a, layout, 24), _embed_in(b, layout, 40)
        biasv, _ = U.embed_vec(bias, 5, 3, U.NAN)
        _CASES[key] = (av, ap, bv, bp, biasv) + U.nt_bound(a, b, bias)
    return _CASES[key]


def _nt(av, bv, biasv, cv):
    """the stand-in kernel: fp32 product of the views, written into the output view (rounded once when that is bf16)"""
    cv.copy_(av.float() @ bv.float().t() + biasv)


def _checks(cv, cp, ref, b32, what):
    U.assert_outside_untouched(cp, cv, U.SENTINEL, what)
    return (U.check_f32 if cv.dtype == F32 else U.check_bf16)(cv, ref, b32, what)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_plain_standin_passes_with_margin(shape, layout):
    """The fp32 stand-in sits under 2 % of b32 (its error is a few fp32 roundings, the bound allows K + 2 truncations), the bf16 one
    under 1.0 of its bound (the one rounding the bound grants is attained)."""
    M, N, K = shape
    av, ap, bv, bp, biasv, ref, b32 = _case(shape, layout)
    cv, cp = _embed_out(M, N, F32, layout)
    _nt(av, bv, biasv, cv)
    assert _checks(cv, cp, ref, b32, "fp32 stand-in") < 0.02
    cv, cp = _embed_out(M, N, BF16, layout)
    _nt(av, bv, biasv, cv)
    assert _checks(cv, cp, ref, b32, "bf16 stand-in") < 1.0
    # accumulate epilogue: C0 = 0.5 in the view, 7.0 around it
    cv, cp = _embed_out(M, N, F32, layout, init=0.5)
    cv += av.float() @ bv.float().t() + biasv
    ref_acc, b32_acc = U.nt_bound(av, bv, biasv, 0.5)
    assert _checks(cv, cp, ref_acc, b32_acc, "fp32 accumulate stand-in") < 0.02


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_tn_standin_passes(shape, layout):
    M, N, K = shape
    dy, x = _rand((M, N), 1.0, BF16, 10), _rand((M, K), 1.0, BF16, 11)
    (dyv, _), (xv, _) = _embed_in(dy, layout, 24), _embed_in(x, layout, 40)
    dwv, dwp = U.embed(torch.full((N, K), 0.5), K + 12, 4, 3, 5, U.SENTINEL)
    dbv, dbp = U.embed_vec(torch.full((N,), 0.25), 5, 3, U.SENTINEL)
    dwv += dyv.float().t() @ xv.float()
    dbv += dyv.float().sum(0)
    ref_w, bw, ref_b, bb = U.tn_bound(dy, x, 0.5, 0.25)
    assert U.check_f32(dwv, ref_w, bw, "dW stand-in") < 0.05
    assert U.check_f32(dbv, ref_b, bb, "dbias stand-in") < 0.05
    U.assert_outside_untouched(dwp, dwv, U.SENTINEL, "dW")
    U.assert_outside_untouched(dbp, dbv, U.SENTINEL, "dbias")
    # one row of M dropped
    dwv.fill_(0.5)
    dwv += dyv[:-1].float().t() @ xv[:-1].float()
    with pytest.raises(AssertionError, match="past the bound"):
        U.check_f32(dwv, ref_w, bw, "dW, one m-term dropped")


def _sub(parent, r0, c0, R, C):
    return parent[r0:r0 + R, c0:c0 + C]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_broken_standins_fail(shape, layout, dtype):
    M, N, K = shape
    av, ap, bv, bp, biasv, ref, b32 = _case(shape, layout)
    ra, _, ca, _ = U._region(ap, av)

    def run(a_read, b_read, what, spoil=None):
        cv, cp = _embed_out(M, N, dtype, layout)
        _nt(a_read, b_read, biasv, cv)
        if spoil is not None:
            spoil(cv, cp)
        _checks(cv, cp, ref, b32, what)

    run(av, bv, "sound")   # (the same path passes when nothing is broken)
    with pytest.raises(AssertionError, match="past the bound"):
        run(av[:, :K - 1], bv[:, :K - 1], "one k-term dropped")
    with pytest.raises(AssertionError, match="past the bound"):
        run(_sub(ap, ra, ca - 1, M, K), bv, "read one column left of the view")
    with pytest.raises(AssertionError, match="past the bound"):
        run(_sub(ap, ra + 1, ca, M, K), bv, "read of row M of the parent")
    with pytest.raises(AssertionError, match="outside the view"):
        def spoil(cv, cp):
            r0, _, _, c1 = U._region(cp, cv)
            cp[r0 + M // 2, c1] = 0.0
        run(av, bv, "sentinel right of column N overwritten", spoil)
    with pytest.raises(AssertionError, match="past the bound"):
        swapped = bv.clone()
        swapped[[N // 2, N // 2 + 1]] = bv[[N // 2 + 1, N // 2]]
        run(av, swapped, "B rows i and i + 1 swapped")
    with pytest.raises(AssertionError, match="past the bound"):
        flat = ap.reshape(-1)[av.storage_offset():av.storage_offset() + M * K].reshape(M, K)   # rows K apart instead of ld apart
        run(flat, bv, "ld of the parent taken for K")


def test_dropped_k_term_breaks_most_elements():
    """One of K = 128 terms dropped is no rare-element event for the elementwise bound: it breaks it in nearly every fp32 element and
    in most bf16 ones (those where the dropped term outweighs the output's own rounding)."""
    av, ap, bv, bp, biasv, ref, b32 = _case((300, 200, 128), "tight")
    got = av[:, :127].float() @ bv[:, :127].float().t() + biasv
    err = (got.double() - ref).abs()
    assert float((err > b32).double().mean()) > 0.95
    got16 = got.to(BF16)
    err16 = (got16.double() - ref).abs()
    assert float((err16 > U.U16 * (ref.abs() + b32) + b32).double().mean()) > 0.8


def test_sentinel_check_compares_bits_and_int_operands_are_exact():
    v, p = U.embed(torch.zeros((4, 6), dtype=F32), 16, 8, 1, 1, U.NAN)
    U.assert_outside_untouched(p, v, U.NAN)          # NaN fill compares equal to itself through the integer view
    p[0, 0] = 7.0
    with pytest.raises(AssertionError, match=r"parent\[0, 0\]"):
        U.assert_outside_untouched(p, v, U.NAN)
    v, p = U.embed_vec(torch.zeros(5), 3, 2, U.SENTINEL)
    U.assert_outside_untouched(p, v, U.SENTINEL)
    p[8] = 7.5
    with pytest.raises(AssertionError, match=r"parent\[0, 8\]"):
        U.assert_outside_untouched(p, v, U.SENTINEL)
    a, b = U.int_operands((70, 128), 7, 13), U.int_operands((50, 128), 5, 11)
    assert float(a.min()) == -6 and float(a.max()) == 6 and float(b.min()) == -5 and float(b.max()) == 5
    ref, _ = U.nt_bound(a, b)
    U.check_exact(a.float() @ b.float().t(), ref, "integer product")
    with pytest.raises(AssertionError, match="differ from the exact product"):
        U.check_exact(a[:, :127].float() @ b[:, :127].float().t(), ref, "integer product, k-term dropped")
    with pytest.raises(AssertionError, match=r"worst at \(3, 4\)"):
        got = (a.float() @ b.float().t())
        got[3, 4] = float("nan")
        U.check_f32(got, ref, torch.ones_like(ref), "a NaN fails")
