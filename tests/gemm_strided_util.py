"""Shared helpers of the strided-GEMM tests (test infrastructure; any device): operands embedded as views of poisoned parents, the
check that nothing outside an output view was written, and elementwise error bounds computed in fp64 from the operands.

Poison: an input's parent is NaN outside the view (a read from there reaches the result as NaN), an output's parent is 7.0 (a store
from there changes its bits).  Bounds (u32 = 2^-23 is twice fp32's unit roundoff, which also covers a truncating accumulator; 2^-8 is
bf16's unit roundoff, for the one rounding of a bf16 output):
    NT  C = A . B^T + bias (+ C0):   b32 = (K + 2) u32 (|A| . |B|^T + |bias| + |C0|)      fp32 out: |got - ref| <= b32
                                                                                           bf16 out: |got - ref| <= 2^-8 (|ref| + b32) + b32
    TN  dW = dW0 + dY^T . X:         (M + 64) u32 (|dY|^T . |X| + |dW0|);  dbias the same with sum_m |dY| + |db0|
(K + 2: K products summed, the bias and C0 added; M + 64: M products, the merges of the M-splits and dW0.)"""
import math

import torch

NAN, SENTINEL = float("nan"), 7.0
U32, U16 = 2.0 ** -23, 2.0 ** -8
_BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def embed(t, ld, col0, rows_before, rows_after, fill):
    """(view, parent): parent [rows_before + R + rows_after, ld] filled with `fill`, t [R, C] copied to its rows rows_before.., columns
    col0..; view is that slice."""
    R, C = t.shape
    assert col0 >= 0 and col0 + C <= ld, (col0, C, ld)
    parent = torch.full((rows_before + R + rows_after, ld), fill, dtype=t.dtype, device=t.device)
    view = parent[rows_before:rows_before + R, col0:col0 + C]
    view.copy_(t)
    return view, parent


def embed_vec(t, before, after, fill):
    """embed for a vector (bias, dbias): a slice of a longer filled one."""
    n = t.shape[0]
    parent = torch.full((before + n + after,), fill, dtype=t.dtype, device=t.device)
    view = parent[before:before + n]
    view.copy_(t)
    return view, parent


def _region(parent, view):
    """(r0, r1, c0, c1) of a view inside its parent (a vector is one row)."""
    off = view.storage_offset() - parent.storage_offset()
    if parent.dim() == 1:
        return 0, 1, off, off + view.shape[0]
    ld = parent.stride(0)
    assert view.stride(0) == ld and view.stride(1) == 1 and off >= 0
    r0, c0 = off // ld, off % ld
    return r0, r0 + view.shape[0], c0, c0 + view.shape[1]


def assert_outside_untouched(parent, view_region, fill, what=""):
    """Every element of `parent` outside the view(s) still has the fill's exact bits (compared through an integer view, so NaN fills and
    the sign of a zero count).  view_region: a view of parent, an (r0, r1, c0, c1) tuple, or a list of those."""
    regions = view_region if isinstance(view_region, (list, tuple)) and not isinstance(view_region[0], int) else [view_region]
    p2 = parent.view(1, -1) if parent.dim() == 1 else parent
    outside = torch.ones(p2.shape, dtype=torch.bool, device=parent.device)
    for rg in regions:
        r0, r1, c0, c1 = _region(parent, rg) if torch.is_tensor(rg) else rg
        outside[r0:r1, c0:c1] = False
    it = _BITS[parent.dtype]
    want = torch.full((), fill, dtype=parent.dtype, device=parent.device).view(it)
    bad = outside & (p2.view(it) != want)
    nbad = int(bad.sum())
    if nbad:
        r, c = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {nbad} elements outside the view were written, first at parent[{r}, {c}] = {float(p2[r, c])!r} (fill {fill})")


def int_operands(shape, mul, mod, device="cpu"):
    """Small-integer bf16 operands, ((arange * mul) % mod) - mod // 2 (the suite's (arange * 7) % 13 - 6 pattern): every product and every
    partial sum of a GEMM over them is an exact fp32 integer, so an fp32 output equals the fp64 product bit for bit."""
    n = math.prod(shape)
    return ((torch.arange(n, device=device).reshape(shape) * mul) % mod - mod // 2).to(torch.bfloat16)


def _f64(t):
    return t.double() if torch.is_tensor(t) else t


def _mag(t):
    return t.double().abs() if torch.is_tensor(t) else abs(float(t))


def nt_bound(a, b, bias=None, c0=None):
    """(ref, b32) in fp64 for C = a . b^T + bias + c0 (c0: tensor or number, the accumulate epilogue)."""
    A, B = a.double(), b.double()
    ref, mag = A @ B.t(), A.abs() @ B.abs().t()
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    if c0 is not None:
        ref, mag = ref + _f64(c0), mag + _mag(c0)
    return ref, (a.shape[1] + 2) * U32 * mag


def tn_bound(dy, x, dw0=0.0, db0=0.0):
    """(ref_w, bound_w, ref_b, bound_b) in fp64 for dW = dw0 + dy^T . x and dbias = db0 + sum_m dy."""
    Y, X = dy.double(), x.double()
    f = (dy.shape[0] + 64) * U32
    ref_w, mag_w = Y.t() @ X + _f64(dw0), Y.abs().t() @ X.abs() + _mag(dw0)
    ref_b, mag_b = Y.sum(0) + _f64(db0), Y.abs().sum(0) + _mag(db0)
    return ref_w, f * mag_w, ref_b, f * mag_b


def _check(got, ref, bound, what):
    """Every element: |got - ref| <= bound (a NaN fails).  The message names the worst index and its err / bound ratio."""
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    nbad = int(bad.sum())
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    worst = int(ratio.reshape(-1).argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), ratio.shape)) if ratio.dim() else ()
    wr = float(ratio.reshape(-1)[worst])
    assert nbad == 0, (f"{what}: {nbad} of {err.numel()} elements past the bound; worst at {idx}: got {float(got[idx])!r}, ref {float(ref[idx])!r}, "
                       f"err / bound = {wr:.3g}")
    return wr


def check_f32(got, ref, b32, what=""):
    """fp32 output against the fp64 reference; returns the worst err / bound ratio."""
    assert got.dtype == torch.float32, got.dtype
    return _check(got, ref, b32, what)


def check_bf16(got, ref, b32, what=""):
    """bf16 output: the fp32 bound plus one bf16 rounding of a value within it."""
    assert got.dtype == torch.bfloat16, got.dtype
    return _check(got, ref, U16 * (ref.abs() + b32) + b32, what)


def check_exact(got, ref, what=""):
    """fp32 output of integer operands: equal to the fp64 product, every element."""
    assert got.dtype == torch.float32, got.dtype
    if not torch.equal(got.double(), ref):
        bad = got.double() != ref
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements differ from the exact product, first at {idx}: "
                             f"got {float(got[idx])!r}, ref {float(ref[idx])!r}")
