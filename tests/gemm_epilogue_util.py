"""fp64 references and elementwise bounds of the GELU / dGELU epilogues of xfm_gemm_nt (test infrastructure; any device): EPI_GELU, the
FFN-in GEMM that writes h = GELU(x) and u = GELU'(x), and EPI_DGELU, the FFN dgrad C = (dY . Wt^T) * u.  The checkers, nt_bound and the
poisoned parents are gemm_strided_util's, the fp64 GELU and its constants rowwise_util's; the operand builders at the end are shared by
the host and GPU tests.

The arithmetic (gemm_common.h::gemm_epilogue, common.h::gelu_parts), per element, acc the fp32 MFMA sum over K:
    v = acc + bias                          fp32;  nt_bound: |v - pre| <= b32 = (K + 2) u32 (|A| . |B|^T + |bias|)
    x = bf16(v)                             one bf16 rounding:  |x - pre| <= ex = 2^-8 (|pre| + b32) + b32
    (cdf, pdf) = gelu_parts(x)              erf by Abramowitz-Stegun 7.1.25 (|delta erf| <= 2.5e-5, so cdf is off by <= 1.25e-5), rcp and
                                            exp2 to one ulp, five fp32 operations
    h = bf16(x * cdf)                       u = bf16(fma(x, pdf, cdf))
    EPI_DGELU:  C = bf16(v * aux)           aux = the stored u, a bf16 input; no bias on the product path (v = acc)

General bound (any operands).  GELU_U = 2^-16 = 1.53e-5 is rowwise_util's allowance for an evaluation of Phi by gelu_parts: 1.25e-5 of
A-S, the rest for the one-ulp rcp / exp2 and the fp32 roundings inside the polynomial (each at most 2^-24 of a value <= 1).
    h   |x cdf - GELU(pre)| <= GELU_LIP ex + GELU_U |pre| + u32 |GELU(pre)|
        (GELU_LIP = 1.13 >= max |GELU'| carries the error of x through the function; cdf off by GELU_U, times |x|; the product's rounding)
    u   |fma(x, pdf, cdf) - GELU'(pre)| <= GELU_GRAD_LIP ex + GELU_U (1 + |pre|) + u32 |GELU'(pre)|
        (GELU_GRAD_LIP = 1 >= max |GELU''| = 2 phi(0) = 0.798; cdf off by GELU_U; pdf = 0.3989 exp2(..) is off by a few ulp of a value
        <= 0.4, which times |x| stays under GELU_U |pre| -- the form ln_bwd_ref charges; the fma's one rounding)
    Both are fp32-level bounds; the stored bf16 is held to check_bf16(got, ref, bound) (one more rounding of a value within it).
    dGELU   ref = (A . B^T) aux,  fp32-level bound b32 |aux| + u32 |ref|  (v within b32, one product), then check_bf16.

Exact-grid check.  ex is about 2^-8 |x|, far wider than what a wrong erf makes (the tanh form of GELU is off by up to 4.7e-4 absolute,
a third-digit error in an A-S coefficient by 2e-4): under the general bound alone such a kernel passes.  grid_family removes the rounding
of x: A in {-1, 0, 1}, B in {-1, 0, 1} / 32, bias = j_n / 32 with j_n = (37 n mod 401) - 200.  Every product is 0 or +-2^-5, every partial
sum a multiple of 2^-5 below 2^19 in any order: exact in fp32.  grid_refs asserts from the fp64 product that every pre-activation is
k / 32 with |k| <= 255, which is a bf16 value (8 significant bits), so the kernel's x IS the reference's.  What is left is the
evaluation at an exact argument:
    h   d = GELU_U |x| + u32 |GELU(x)|            u   d = GELU_U (1 + |x|) + u32 |GELU'(x)|
and the stored bf16 must be the rounding of SOME value within d of the truth.  Rounding to nearest-even is monotone, so that is
    bf16(g - d) <= got <= bf16(g + d)
(bf16_rne rounds the fp64 numbers to 8 significant bits, ties to even, without a detour over fp32).  The ratio printed for this check
is the share of d that the stored value needs: the distance from g to the set of reals that round to `got`, over d (0 when g itself
rounds to got).  For N >= 200 the family has to hit at least 90 % of the 385 values k / 32 in [-6, 6] (grid_coverage; asserted by the
host test, so the recipe above is what has to deliver it).

Saturation columns (sat_columns: N >= 12): six columns -- the second of the first chunk, the second of the second chunk, two in the
middle, the last two, which lie in the partial chunk of a ragged N -- get a zero row of B and a bias of +-8, +-16, +-128, so x is that
value in every row.  These are bf16 values outside the |k| <= 255 grid and exempt from that assertion only: +-8 go through the
interval check like every other element; at |x| >= 16 exp2(-0.72 x^2) is zero in fp32, so cdf is exactly 1 or 0 and pdf 0:
h == x and u == 1 for x > 0, h == 0 and u == 0 by value (the sign of the zero is the product's, not asserted) for x < 0.  No NaN anywhere.
(5 x 3 x 64 has three columns: no room for them, it is checked on the grid alone.)

Exact dGELU: int_operands A (|a| <= 6) and B (|b| <= 5), aux in {-2, -1, -0.5, 0, 0.5, 1, 2}: v is an integer below 2^24, the product
with a power of two (or zero) is exact, and the output must be bf16(ref), every element, compared by value (NaN fails; a zero's sign is
the product's in both)."""
import math

import torch

from gemm_strided_util import U16, U32, _check, check_bf16, embed, int_operands, nt_bound  # noqa: F401
from rowwise_util import GELU_LIP, GELU_U, gelu64, gelu_grad64

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GELU_GRAD_LIP = 1.0      # max |GELU''| = GELU''(0) = 2 phi(0) = 0.798
GRID = 32                # grid step 1 / 32
GRID_KMAX = 255          # |k| <= 255: 8 significant bits
SAT_VALUES = (8.0, -8.0, 16.0, -16.0, 128.0, -128.0)
DGELU_AUX_SET = (-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0)
INF = math.inf


# ---------------------------------------------------------------------------------------------------------------------- general bound
def gelu_refs(a, b, bias):
    """{"pre": pre, "h": (GELU(pre), bound), "u": (GELU'(pre), bound)} in fp64, fp32-level bounds (see the header)."""
    pre, b32 = nt_bound(a, b, bias)
    ap = pre.abs()
    ex = U16 * (ap + b32) + b32
    g, gu = gelu64(pre), gelu_grad64(pre)
    return {"pre": pre, "h": (g, GELU_LIP * ex + GELU_U * ap + U32 * g.abs()), "u": (gu, GELU_GRAD_LIP * ex + GELU_U * (1 + ap) + U32 * gu.abs())}


def check_gelu(h, u, refs, what=""):
    """the stored bf16 h and u against gelu_refs; -> (worst ratio of h, of u)"""
    return check_bf16(h, *refs["h"], f"{what} h"), check_bf16(u, *refs["u"], f"{what} u")


def dgelu_refs(a, b, aux):
    """(ref, fp32-level bound) in fp64 for C = (a . b^T) * aux"""
    v, b32 = nt_bound(a, b)
    A = aux.double()
    ref = v * A
    return ref, b32 * A.abs() + U32 * ref.abs()


def check_dgelu_exact(got, ref, what=""):
    """the exact family: got == bf16(ref) in every element (ref is an fp32-exact number: the conversion rounds once)"""
    assert got.dtype == BF16, got.dtype
    want = ref.to(F32).to(BF16)
    if not torch.equal(got, want):
        bad = ~(got == want)
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements differ from bf16(exact product), first at {idx}: "
                             f"got {float(got[idx])!r}, want {float(want[idx])!r}")


# ------------------------------------------------------------------------------------------------------------------------- exact grid
def bf16_rne(t):
    """fp64 -> the nearest number with 8 significant bits (ties to even), as fp64: bf16's rounding for every normal value"""
    bits = t.contiguous().view(torch.int64)    # on the bit pattern (sign and magnitude): exact on every device, unlike ldexp through pow
    bits = bits + ((1 << 44) - 1) + ((bits >> 45) & 1)       # 52 - 7 = 45 fraction bits go; a tie moves up only onto an even pattern
    return (bits & ~((1 << 45) - 1)).view(F64)


def _cell_distance(got, g):
    """distance from g to the reals that round to the bf16 `got` (both fp64): 0 inside got's rounding cell"""
    s = torch.where(got < 0, -torch.ones_like(g), torch.ones_like(g))
    H, G = got.abs().contiguous(), g * s
    bits = H.view(torch.int64)
    ulp = (torch.clamp(((bits >> 52) & 0x7FF) - 7, min=1) << 52).view(F64)    # H = 1.f 2^E: spacing 2^(E - 7)
    up = 0.5 * ulp
    down = torch.where((bits & ((1 << 52) - 1)) == 0, 0.25 * ulp, 0.5 * ulp)   # below a power of two the spacing halves
    zero = H == 0
    up, down = torch.where(zero, torch.zeros_like(up), up), torch.where(zero, torch.zeros_like(down), down)
    return torch.clamp(torch.maximum(H - down - G, G - H - up), min=0.0)


def check_interval(got, g, d, what=""):
    """bf16(g - d) <= got <= bf16(g + d) in every element (a NaN fails); -> the worst share of d needed (see the header)"""
    assert got.dtype == BF16 and got.shape == g.shape, (got.dtype, tuple(got.shape), tuple(g.shape))
    G = got.double()
    lo, hi = bf16_rne(g - d), bf16_rne(g + d)
    bad = ~((G >= lo) & (G <= hi))
    dist = _cell_distance(torch.nan_to_num(G, nan=INF, posinf=INF, neginf=-INF), g)
    ratio = torch.where(d > 0, dist / d, torch.where(dist == 0, torch.zeros_like(dist), torch.full_like(dist, INF)))
    ratio = torch.nan_to_num(ratio, nan=INF)
    nbad = int(bad.sum())
    if nbad:
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {nbad} of {g.numel()} elements outside their interval, first at {idx}: got {float(got[idx])!r}, "
                             f"truth {float(g[idx])!r}, interval [{float(lo[idx])!r}, {float(hi[idx])!r}], d = {float(d[idx]):.3g}")
    return float(ratio.max()) if ratio.numel() else 0.0


def sat_columns(N):
    """{column: x} of the saturation columns (none below N = 12)"""
    if N < 12:
        return {}
    return dict(zip((1, 9, N // 2, N // 2 + 1, N - 2, N - 1), SAT_VALUES))


def grid_refs(a, b, bias):
    """References of the grid family, fp64: asserts the grid property outside the saturation columns and returns x, (g, d) for h and u,
    and the column lists of the |x| >= 16 expectations."""
    N = b.shape[0]
    x, _ = nt_bound(a, b, bias)
    sat = sat_columns(N)
    plain = torch.ones(N, dtype=torch.bool, device=x.device)
    for c, v in sat.items():
        plain[c] = False
        assert bool((x[:, c] == v).all()), f"saturation column {c} is not {v} in every row"
    k = x[:, plain] * GRID
    assert bool((k == k.round()).all()) and float(k.abs().max()) <= GRID_KMAX, f"not on the grid: max |k| = {float(k.abs().max())}"
    ax = x.abs()
    g, gu = gelu64(x), gelu_grad64(x)
    return {"x": x, "h": (g, GELU_U * ax + U32 * g.abs()), "u": (gu, GELU_U * (1 + ax) + U32 * gu.abs()),
            "sat_pos": [c for c, v in sat.items() if v >= 16], "sat_neg": [c for c, v in sat.items() if v <= -16]}


def check_grid(h, u, refs, what=""):
    """h and u of the grid family: no NaN, the |x| >= 16 columns exact, every other element inside its interval; -> (ratio h, ratio u)"""
    assert not bool(h.isnan().any()) and not bool(u.isnan().any()), f"{what}: NaN in the output"
    x = refs["x"]
    rest = torch.ones(x.shape[1], dtype=torch.bool, device=x.device)
    for cols, want_u in ((refs["sat_pos"], 1.0), (refs["sat_neg"], 0.0)):
        for c in cols:
            rest[c] = False
            want_h = x[:, c] if want_u else torch.zeros_like(x[:, c])
            assert bool((h[:, c].double() == want_h).all()), f"{what}: h of saturation column {c} (x = {float(x[0, c])}) is not {'x' if want_u else '0'}"
            assert bool((u[:, c].double() == want_u).all()), f"{what}: u of saturation column {c} (x = {float(x[0, c])}) is not {want_u}"
    (g, dh), (gu, du) = refs["h"], refs["u"]
    return (check_interval(h[:, rest], g[:, rest], dh[:, rest], f"{what} h"), check_interval(u[:, rest], gu[:, rest], du[:, rest], f"{what} u"))


def grid_coverage(x):
    """share of the values k / 32 in [-6, 6] that occur among the pre-activations x"""
    k = (x * GRID).round().long().reshape(-1)
    k = k[k.abs() <= 6 * GRID]
    return int(torch.unique(k).numel()) / (2 * 6 * GRID + 1)


# ---------------------------------------------------------------------------------------- operands (shared by the host and GPU tests)
def _randn(shape, scale, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _randint(lo, hi, shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g)


def random_family(M, N, K, device="cpu"):
    """the scales of the older GEMM tests: A ~ 1, B ~ 0.05, bias ~ 0.5  (|pre| stays below about 3)"""
    return (_randn((M, K), 1.0, 1).to(BF16).to(device), _randn((N, K), 0.05, 2).to(BF16).to(device), _randn((N,), 0.5, 3).to(device))


def wide_family(M, N, K, device="cpu"):
    """B ~ 0.25, scaled up where the shape is too small for that to carry |A . B^T| to 7.5: with a bias ~ 0.5, |pre| reaches 6 (the
    callers assert it)"""
    a, b0 = _randn((M, K), 1.0, 11).to(BF16), _randn((N, K), 0.25, 12)
    top = float((a.double() @ b0.to(BF16).double().t()).abs().max())
    return a.to(device), (b0 * max(1.0, 7.5 / top)).to(BF16).to(device), _randn((N,), 0.5, 13).to(device)


def grid_family(M, N, K, device="cpu"):
    """A in {-1, 0, 1}, B in {-1, 0, 1} / 32, bias (37 n mod 401 - 200) / 32; the saturation columns with a zero row of B (see the header)"""
    a = _randint(-1, 2, (M, K), 21).to(BF16)
    b = (_randint(-1, 2, (N, K), 22).float() / GRID).to(BF16)
    bias = ((torch.arange(N) * 37) % 401 - 200).float() / GRID
    for c, v in sat_columns(N).items():
        b[c] = 0
        bias[c] = v
    return a.to(device), b.to(device), bias.to(device)


def dgelu_family(M, N, K, device="cpu"):
    """the random family's A and B with aux = true GELU' values of a standard normal argument, as the forward stores them"""
    a, b, _ = random_family(M, N, K, device)
    return a, b, gelu_grad64(_randn((M, N), 1.0, 4).double()).to(BF16).to(device)


def dgelu_exact_family(M, N, K, device="cpu"):
    """integer A and B, aux drawn from DGELU_AUX_SET"""
    vals = torch.tensor(DGELU_AUX_SET)
    aux = vals[_randint(0, len(DGELU_AUX_SET), (M, N), 31)].to(BF16)
    return int_operands((M, K), 7, 13, device), int_operands((N, K), 5, 11, device), aux.to(device)
