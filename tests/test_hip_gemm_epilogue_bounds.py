"""The GELU / dGELU epilogues of xfm_gemm_nt (gemm_common.h::gemm_epilogue) under elementwise fp64 bounds, on every tile configuration.

tests/test_hip_kernels.py holds these epilogues to 1e-2 of the tensor's largest value on hints 0, 4 and 5, and
tests/test_hip_gemm_strided.py pins their strided bits to the contiguous call's; neither can see a wrong erf, and the small tiles never
met a ragged N whose partial 8-column chunk is not chunk 0.  Here (gemm_epilogue_util's header has the derivations):
    GELU    h and u under the general bound on two random families (the older scales; a wide one whose |pre| reaches 6), and on the exact
            grid family, where x = k / 32 is a bf16 value and the stored h and u must be roundings of values within
            2^-16 |x| (+ 2^-16 for u) of the truth -- with the saturation columns x = +-8, +-16, +-128.
            Every GELU call runs twice: aux contiguous (ldaux == ldc) and aux a view of a wider parent (ldaux != ldc).
    dGELU   under its bound with true GELU' values as aux, and bit for bit on integer operands with aux in {0, +-0.5, +-1, +-2}.
Operands are contiguous (the strided test covers the layouts).  Shapes: the small hints at (300, 200, 128), (5, 3, 64) and the ragged
(300, 203, 64) -- two column tiles, full chunks, then a partial chunk that is not chunk 0 --, one workgroup per 256 x 256 tile, the
persistent form with ragged M and N and the bias through LDS, and the tail split, whose second call offsets aux by rows_a * ldaux.
One `gemm-epi-ratio gpu ...` line per check (pytest -s); profiles/tests_gemm_epilogue_bounds.md keeps them next to the CPU emulation's
(tests/test_gemm_epilogue_host.py)."""
import ctypes
import functools

import pytest
import torch

import gemm_epilogue_util as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
SMALL_HINTS = [1, 2, 3, 4, 7, 8, 0]
CASES = ([(300, 200, 128, h) for h in SMALL_HINTS] + [(5, 3, 64, h) for h in SMALL_HINTS] + [(300, 203, 64, h) for h in SMALL_HINTS]
         + [(300, 256, 128, 5),      # one workgroup per 256 x 256 tile
            (16400, 1001, 64, 5),    # 260 tiles > CUs: persistent, ragged M and N, the bias through LDS
            (21800, 520, 64, 0)])    # tail split: rows_a rows on 256 x 256 tiles, the rest planned again
TAIL_SPLIT = (21800, 520, 64, 0)


def _fx():
    from xfm_amd import functional as Fx
    return Fx


def _plan(M, N, K, epi, hint):
    from xfm_amd import _lib as L
    cfg, rows_a = ctypes.c_int(), ctypes.c_int()
    L.check(L.load().xfm_gemm_nt_plan(M, N, K, epi, hint, ctypes.byref(cfg), ctypes.byref(rows_a)), "gemm_nt_plan")
    return cfg.value, rows_a.value


def _assert_route(M, N, K, hint, epi):
    """the configuration this case is here for: an explicit hint is taken as given and never split; hint 0 is a small tile at the small
    shapes and the tail split (rows_a > 0, then configuration 5) at its shape"""
    cfg, rows_a = _plan(M, N, K, epi, hint)
    if hint > 0:
        assert (cfg, rows_a) == (hint, 0), (cfg, rows_a)
    elif (M, N, K, hint) == TAIL_SPLIT:
        assert cfg == 5 and 0 < rows_a < M and rows_a % 256 == 0, (cfg, rows_a)
    else:
        assert cfg in (2, 3, 7, 8) and rows_a == 0, (cfg, rows_a)
    return cfg, rows_a


def _report(tag, what, ratio):
    print(f"gemm-epi-ratio gpu {tag} {what} {ratio:.3g}")
    assert ratio <= 1.0, (tag, what, ratio)


@functools.lru_cache(maxsize=1)
def _gelu_case(M, N, K):
    """Operands and fp64 references of a shape's three GELU families, made once, shared by its hints, never written."""
    c = {}
    for fam, make in (("random", E.random_family), ("wide", E.wide_family)):
        ops = make(M, N, K, DEV)
        c[fam] = (ops, E.gelu_refs(*ops))
    ops = E.grid_family(M, N, K, DEV)
    c["grid"] = (ops, E.grid_refs(*ops))
    assert float(c["wide"][1]["pre"].abs().max()) >= 6.0, "the wide family has to reach |pre| = 6"
    return c


@functools.lru_cache(maxsize=1)
def _dgelu_case(M, N, K):
    a, b, aux = E.dgelu_family(M, N, K, DEV)
    ai, bi, auxi = E.dgelu_exact_family(M, N, K, DEV)
    return (a, b, aux, E.dgelu_refs(a, b, aux)), (ai, bi, auxi, E.dgelu_refs(ai, bi, auxi)[0])


def _aux_out(M, N, strided):
    """the u output: contiguous (ldaux == ldc == N), or the first N columns of a 7.0-filled parent whose rows are N rounded up to 8,
    plus 8, long -- 16-byte row starts, ldaux != ldc.  -> (view, parent or None)"""
    if not strided:
        return torch.empty((M, N), dtype=BF16, device=DEV), None
    parent = torch.full((M, (N + 7) // 8 * 8 + 8), 7.0, dtype=BF16, device=DEV)
    return parent[:, :N], parent


@pytest.mark.parametrize("M,N,K,hint", CASES)
def test_gemm_nt_gelu_bounds(M, N, K, hint):
    Fx = _fx()
    cfg, rows_a = _assert_route(M, N, K, hint, Fx.EPI_GELU)
    c = _gelu_case(M, N, K)
    for strided in (False, True):
        tag = f"{M}x{N}x{K} hint {hint} cfg {cfg} rows_a {rows_a} ldaux {'!=' if strided else '=='} ldc"
        for fam in ("random", "wide", "grid"):
            (a, b, bias), refs = c[fam]
            u, parent = _aux_out(M, N, strided)
            h, _ = Fx.gemm_nt(a, b, bias, epi=Fx.EPI_GELU, aux=u, tile_hint=hint)
            assert h.stride(0) == N and (u.stride(0) != N) == strided
            if parent is not None:
                assert bool((parent[:, N:] == 7.0).all()), f"{tag} {fam}: columns right of the aux view were written"
            rh, ru = (E.check_grid if fam == "grid" else E.check_gelu)(h, u, refs, f"{tag} {fam}")
            _report(tag, f"{fam} h", rh)
            _report(tag, f"{fam} u", ru)


@pytest.mark.parametrize("M,N,K,hint", CASES)
def test_gemm_nt_dgelu_bounds(M, N, K, hint):
    Fx = _fx()
    cfg, rows_a = _assert_route(M, N, K, hint, Fx.EPI_DGELU)
    (a, b, aux, (ref, bound)), (ai, bi, auxi, refi) = _dgelu_case(M, N, K)
    tag = f"{M}x{N}x{K} hint {hint} cfg {cfg} rows_a {rows_a}"
    got = Fx.gemm_nt(a, b, None, epi=Fx.EPI_DGELU, aux=aux, tile_hint=hint)
    _report(tag, "dgelu", E.check_bf16(got, ref, bound, f"{tag} dgelu"))
    got = Fx.gemm_nt(ai, bi, None, epi=Fx.EPI_DGELU, aux=auxi, tile_hint=hint)
    E.check_dgelu_exact(got, refi, f"{tag} dgelu exact")
