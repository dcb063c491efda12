"""The GELU / dGELU epilogue checks (gemm_epilogue_util) are neither vacuous nor too tight, shown on the CPU: an fp32 emulation of
gemm_common.h::gemm_epilogue (rowwise_util.gelu_parts32 for common.h's polynomial; 8-column chunks, an aux with its own row stride)
passes every check of tests/test_hip_gemm_epilogue_bounds.py at (300, 203, 64) and (5, 3, 64) with every ratio below 1, the grid
family covers [-6, 6], and each planted fault -- the tanh forms of GELU and GELU', an Abramowitz-Stegun coefficient off in its third
digit, u without its x pdf term past |x| = 3, the dGELU taking aux chunk 0 for the partial last chunk or reading aux with ldc for
ldaux, the neighbouring column's bias in the last partial chunk -- fails at least one of them.  The worst ratios are printed
(pytest -s) as `gemm-epi-ratio cpu <shape> <family> <quantity> <ratio>` lines; profiles/tests_gemm_epilogue_bounds.md sets them next to
the MI355X's and next to the 0.75 that the other host twins keep their fp32 emulations under."""
import math

import pytest
import torch

import gemm_epilogue_util as E
from gemm_epilogue_util import BF16
from rowwise_util import gelu_parts32

SHAPES = [(300, 203, 64), (5, 3, 64)]
OLD_SHAPES = [(300, 200, 128), (5, 3, 64)]      # what the suite had for the small tiles: N % 8 == 0, or one partial chunk that is chunk 0
FAULTS = ("tanh_gelu", "tanh_grad", "coefficient", "u_without_x_pdf", "aux_chunk0", "aux_ldc", "neighbour_bias")


def _report(shape, family, what, ratio, limit=1.0):
    print(f"gemm-epi-ratio cpu {'x'.join(str(s) for s in shape)} {family} {what} {ratio:.3g}")
    assert ratio < limit, f"{shape} {family} {what}: emulation at {ratio:.3g} of the bound"


# ------------------------------------------------------------------------------------------------------------------- fp32 emulation
def _fma(x, y, z):
    """fp32 fma: the product is exact in fp64, one rounding of the sum (to fp64 first: a double rounding in 2^-29 of the cases)"""
    return (x.double() * y.double() + z.double()).float()


def _last_partial_chunk(N):
    """columns of the partial 8-column chunk (empty when N % 8 == 0)"""
    return range(N // 8 * 8, N)


def emul_gelu(a, b, bias, fault=None):
    """(h, u) in fp32, before the bf16 store"""
    N = b.shape[0]
    bv = bias.float().clone()
    if fault == "neighbour_bias":
        for n in _last_partial_chunk(N):
            bv[n] = bias[n - 1] if n > 0 else bias[n + 1]
    x = (a.float() @ b.float().t() + bv).to(BF16).float()
    cdf, pdf = gelu_parts32(x, 0.7468556) if fault == "coefficient" else gelu_parts32(x)
    h, u = x * cdf, _fma(x, pdf, cdf)
    if fault in ("tanh_gelu", "tanh_grad"):
        c = math.sqrt(2.0 / math.pi)
        t = torch.tanh(c * (x + 0.044715 * x ** 3))
        if fault == "tanh_gelu":
            h = 0.5 * x * (1.0 + t)
        else:
            u = 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * c * (1.0 + 3 * 0.044715 * x * x)
    if fault == "u_without_x_pdf":
        u = torch.where(x.abs() > 3, cdf, u)
    return h, u


def emul_dgelu(a, b, aux, ldc, fault=None):
    """fp32 product before the bf16 store; aux: a [M, N] view with its own row stride"""
    M, N = aux.shape
    used = aux
    if fault == "aux_ldc":
        used = torch.as_strided(aux, (M, N), (ldc, 1))
    used = used.float().clone()
    if fault == "aux_chunk0":
        cols = _last_partial_chunk(N)
        if len(cols):
            used[:, cols.start:] = aux[:, :len(cols)].float()
    return (a.float() @ b.float().t()) * used


def _aux_view(aux):
    """aux inside a NaN-filled parent with ldaux = N + 8"""
    return E.embed(aux, aux.shape[1] + 8, 0, 1, 1, float("nan"))[0]


# ---------------------------------------------------------------------------------------------------- every check, with and without a fault
_CASES = {}


def _case(shape):
    """operands and fp64 references of a shape, made once, never written"""
    if shape not in _CASES:
        c = {}
        for fam, make in (("random", E.random_family), ("wide", E.wide_family)):
            ops = make(*shape)
            c[fam] = (ops, E.gelu_refs(*ops))
        ops = E.grid_family(*shape)
        c["grid"] = (ops, E.grid_refs(*ops))
        a, b, aux = E.dgelu_family(*shape)
        c["dgelu"] = ((a, b, _aux_view(aux)), E.dgelu_refs(a, b, aux))
        a, b, aux = E.dgelu_exact_family(*shape)
        c["exact"] = ((a, b, _aux_view(aux)), E.dgelu_refs(a, b, aux)[0])
        _CASES[shape] = c
    return _CASES[shape]


def run_checks(shape, fault=None, report=False):
    """The checks of the GPU file on the emulation; raises AssertionError at the first that fails.  With report, also the fp32-level
    ratios of the emulation (its error before the bf16 store over the fp32-level bound or over d)."""
    c, N = _case(shape), shape[1]
    for fam in ("random", "wide"):
        ops, refs = c[fam]
        h, u = emul_gelu(*ops, fault=fault)
        rh, ru = E.check_gelu(h.to(BF16), u.to(BF16), refs, f"{fam}")
        if report:
            _report(shape, fam, "h32", E._check(h, *refs["h"], "h fp32"))
            _report(shape, fam, "u32", E._check(u, *refs["u"], "u fp32"))
            _report(shape, fam, "h16", rh)
            _report(shape, fam, "u16", ru)
    ops, refs = c["grid"]
    h, u = emul_gelu(*ops, fault=fault)
    rh, ru = E.check_grid(h.to(BF16), u.to(BF16), refs, "grid")
    if report:
        keep = [n for n in range(N) if n not in refs["sat_pos"] + refs["sat_neg"]]
        _report(shape, "grid", "h32", E._check(h[:, keep], refs["h"][0][:, keep], refs["h"][1][:, keep], "grid h fp32"))
        _report(shape, "grid", "u32", E._check(u[:, keep], refs["u"][0][:, keep], refs["u"][1][:, keep], "grid u fp32"))
        _report(shape, "grid", "h16", rh)
        _report(shape, "grid", "u16", ru)
    (a, b, auxv), (ref, bound) = c["dgelu"]
    got = emul_dgelu(a, b, auxv, N, fault)
    r16 = E.check_bf16(got.to(BF16), ref, bound, "dgelu")
    if report:
        _report(shape, "dgelu", "c32", E._check(got, ref, bound, "dgelu fp32"))
        _report(shape, "dgelu", "c16", r16)
    (a, b, auxv), ref = c["exact"]
    E.check_dgelu_exact(emul_dgelu(a, b, auxv, N, fault).to(BF16), ref, "dgelu exact")


@pytest.mark.parametrize("shape", SHAPES)
def test_emulation_passes_every_check(shape):
    c = _case(shape)
    assert float(c["wide"][1]["pre"].abs().max()) >= 6.0
    assert float(c["random"][1]["pre"].abs().max()) < 4.0
    run_checks(shape, report=True)


def test_grid_family_covers_the_interval():
    """for N >= 200 at least 90 % of the values k / 32 in [-6, 6] occur as pre-activations (a condition on the operand recipe)"""
    for shape in ((300, 203, 64), (300, 200, 128), (300, 256, 128)):
        cov = E.grid_coverage(E.grid_refs(*E.grid_family(*shape))["x"])
        print(f"gemm-epi-coverage {shape} {cov:.3f}")
        assert cov >= 0.9, (shape, cov)


def test_gelu_parts_inside_both_intervals_on_the_whole_grid():
    """all 511 grid points x = k / 32, |k| <= 255, as a 1 x 511 problem with K = 64: x comes from the bias alone"""
    N = 2 * E.GRID_KMAX + 1
    a, b = torch.zeros((1, 64), dtype=BF16), torch.zeros((N, 64), dtype=BF16)
    bias = (torch.arange(N) - E.GRID_KMAX).float() / E.GRID
    x, _ = E.nt_bound(a, b, bias)
    g, gu, ax = E.gelu64(x), E.gelu_grad64(x), x.abs()
    dh, du = E.GELU_U * ax + E.U32 * g.abs(), E.GELU_U * (1 + ax) + E.U32 * gu.abs()
    h, u = emul_gelu(a, b, bias)
    rh, ru = E.check_interval(h.to(BF16), g, dh, "h"), E.check_interval(u.to(BF16), gu, du, "u")
    nz = x != 0    # d = 0 at x = 0 for h, where the emulation is exact
    r32h, r32u = float(((h.double() - g).abs()[nz] / dh[nz]).max()), float(((u.double() - gu).abs() / du).max())
    print(f"gemm-epi-ratio cpu grid511 h32 {r32h:.3g} u32 {r32u:.3g} h16 {rh:.3g} u16 {ru:.3g}")
    assert float(h[~nz].abs().max()) == 0.0 and r32h < 1.0 and r32u < 1.0
    for fault, which, at_least in (("tanh_gelu", "h", 72), ("tanh_grad", "u", 108)):
        hf, uf = emul_gelu(a, b, bias, fault)
        got, t, d = (hf, g, dh) if which == "h" else (uf, gu, du)
        lo, hi = E.bf16_rne(t - d), E.bf16_rne(t + d)
        G = got.to(BF16).double()
        outside = int((~((G >= lo) & (G <= hi))).sum())
        print(f"gemm-epi-grid511 {fault}: {outside} of {N} points outside the interval")
        assert outside >= at_least // 2, (fault, outside)


def _fails(shape, fault):
    try:
        run_checks(shape, fault)
    except AssertionError as e:
        return str(e).split(":")[0]
    return None


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_faults_are_caught(fault):
    """each fault fails at least one check at the new ragged shape"""
    which = _fails((300, 203, 64), fault)
    print(f"gemm-epi-fault {fault}: first failing check at 300x203x64: {which}")
    assert which is not None, f"{fault} passes every check"


# ----------------------------------------------------------------------------------------------------- what the older checks could see
def _max_norm_passes(got, ref, tol=1e-2):
    """tests/test_hip_kernels.py::_close: max error over the tensor's largest magnitude"""
    got, ref = got.float(), ref.float()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-6) <= tol


def _old_check_passes(shape, fault):
    """test_gemm_nt_gelu_and_dgelu's comparisons, on the emulation with a fault: the older scales, fp32 torch as the reference"""
    a, b, bias = E.random_family(*shape)
    pre = a.float() @ b.float().t() + bias
    x = pre.to(BF16).float()
    h, u = emul_gelu(a, b, bias, fault)
    ok = _max_norm_passes(h.to(BF16), torch.nn.functional.gelu(x)) and _max_norm_passes(u.to(BF16), E.gelu_grad64(x.double()).float())
    a, b, aux = E.dgelu_family(*shape)
    got = emul_dgelu(a, b, _aux_view(aux), shape[1], fault).to(BF16)
    return ok and _max_norm_passes(got, (a.float() @ b.float().t()) * aux.float())


def test_max_norm_check_misses_what_the_bounds_catch():
    """Why these checks exist, kept as a test.  Under max error <= 1e-2 max|ref| on the older scales, even at the new ragged shape, the
    two tanh forms, the wrong coefficient and the dropped x pdf term (|x| never passes 3 there) pass; the new checks fail all four.  At
    the shapes the small tiles had (N % 8 == 0, or 5 x 3 x 64 whose one partial chunk is chunk 0) the chunk-0 fault changes nothing and
    passes old and new checks alike, and the neighbour's bias has no partial chunk to act on at N = 200: (300, 203, 64) is what
    catches both."""
    new_shape = (300, 203, 64)
    passes_old = {f: _old_check_passes(new_shape, f) for f in FAULTS}
    print(f"gemm-epi-old-check at 300x203x64: {passes_old}")
    for f in ("tanh_gelu", "tanh_grad", "coefficient", "u_without_x_pdf"):
        assert passes_old[f], f
        assert _fails(new_shape, f) is not None, f
    for f in ("aux_chunk0", "aux_ldc", "neighbour_bias"):   # address faults: O(1) errors, visible to any check that runs the shape
        assert not passes_old[f], f
    at_old = {shape: {f: _fails(shape, f) is None for f in FAULTS} for shape in OLD_SHAPES}
    print(f"gemm-epi-new-checks passing at the older shapes: {at_old}")
    for shape in OLD_SHAPES:
        assert at_old[shape]["aux_chunk0"], shape
        assert not at_old[shape]["aux_ldc"], shape
    assert at_old[(300, 200, 128)]["neighbour_bias"] and not at_old[(5, 3, 64)]["neighbour_bias"]
    for f in ("tanh_gelu", "tanh_grad", "coefficient", "u_without_x_pdf"):
        assert not at_old[(300, 200, 128)][f], f


def test_interval_check_is_exact_about_roundings():
    """bf16_rne is bf16's rounding, and check_interval accepts exactly the roundings of [g - d, g + d]"""
    t = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * 8
    t32 = t.float().double()     # fp32-exact numbers: torch's own conversion rounds them once
    assert torch.equal(E.bf16_rne(t32), t32.float().to(BF16).double())
    g = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -12], dtype=torch.float64)     # just above the tie between 1 and 1 + 2^-7
    d = torch.tensor([2.0 ** -11], dtype=torch.float64)
    up, down = torch.tensor([1.0 + 2.0 ** -7], dtype=BF16), torch.tensor([1.0], dtype=BF16)
    assert E.check_interval(up, g, d) == 0.0
    assert 0.0 < E.check_interval(down, g, d) < 1.0         # g - d lies below the tie: 1.0 is the rounding of a value within d
    with pytest.raises(AssertionError, match="outside their interval"):
        E.check_interval(down, g, d / 4)
    with pytest.raises(AssertionError, match="outside their interval"):
        E.check_interval(torch.tensor([float("nan")], dtype=BF16), g, d)
