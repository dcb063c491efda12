"""xfm_gemm_nt with tile_hint 6: the one-round 320 x 256 tile (csrc/nt320_gemm.hip) against the fp64 product of the same bf16 operands.

Bounds are those of the existing GEMM tests for the same epilogue (gemm_strided_util.nt_bound / check_f32 / check_bf16,
gemm_epilogue_util.gelu_refs / dgelu_refs).  Shapes: the smallest tile with 1, 2, 3 and 5 K-tiles (prologue and drain only; exactly the
two K-tiles of the LDS ring; the first reuse of a ring slot; an odd count that is no multiple of the ring), a one-row tile behind a
full one, several row tiles against all three column tiles, every epilogue, strided operands inside poisoned parents, bit identity
with configuration 5 and the fallback of a call the tile does not take."""
import ctypes
import functools

import pytest
import torch

import gemm_epilogue_util as G
import gemm_strided_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
HINT = 6


def _fx():
    from xfm_amd import functional as Fx
    return Fx


def _plan(M, N, K, epi, hint):
    from xfm_amd import _lib as L
    cfg, rows_a = ctypes.c_int(), ctypes.c_int()
    L.check(L.load().xfm_gemm_nt_plan(M, N, K, epi, hint, ctypes.byref(cfg), ctypes.byref(rows_a)), "gemm_nt_plan")
    return cfg.value, rows_a.value


def _full(shape, v, dtype):
    return torch.full(shape, v, dtype=dtype, device=DEV)


def _report(what, ratio):
    print(f"  {what}: worst err / bound = {ratio:.3g}")


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """Operands and fp64 references of a shape, made once, shared by the tests that use it, never written."""
    a, b, bias = G.random_family(M, N, K, DEV)
    aux = G.dgelu_family(M, N, K, DEV)[2]
    return dict(a=a, b=b, bias=bias, aux=aux, plain=U.nt_bound(a, b, bias), acc=U.nt_bound(a, b, bias, 0.5), gelu=G.gelu_refs(a, b, bias),
                dgelu=G.dgelu_refs(a, b, aux))


def _is_320(M, N, K):
    for epi in range(5):
        assert _plan(M, N, K, epi, HINT) == (6, 0), (M, N, K, epi)


@pytest.mark.parametrize("M,N,K", [(320, 256, 64), (320, 256, 128), (320, 256, 192), (320, 256, 320),
                                   (321, 768, 128), (639, 512, 192), (788, 768, 768), (1000, 768, 768)])
def test_nt320_plain_epilogue_vs_fp64(M, N, K):
    Fx, c = _fx(), _case(M, N, K)
    _is_320(M, N, K)
    got = Fx.gemm_nt(c["a"], c["b"], c["bias"], tile_hint=HINT)
    _report(f"{M}x{N}x{K} bf16", U.check_bf16(got, *c["plain"], f"{M}x{N}x{K} bf16"))
    # integer operands: the fp32 output is the exact product (a fragment fed to the wrong accumulator cannot hide in a bound)
    ai, bi = U.int_operands((M, K), 7, 13, DEV), U.int_operands((N, K), 5, 11, DEV)
    biasi = (torch.arange(N, device=DEV) % 5 - 2).float()
    U.check_exact(Fx.gemm_nt(ai, bi, biasi, epi=Fx.EPI_F32, tile_hint=HINT), U.nt_bound(ai, bi, biasi)[0], f"{M}x{N}x{K} integers")


@pytest.mark.parametrize("M,N,K", [(400, 256, 128), (788, 768, 768)])
def test_nt320_every_epilogue_vs_fp64(M, N, K):
    Fx, c = _fx(), _case(M, N, K)
    _is_320(M, N, K)
    a, b, bias, tag = c["a"], c["b"], c["bias"], f"{M}x{N}x{K}"
    _report(f"{tag} bias bf16", U.check_bf16(Fx.gemm_nt(a, b, bias, tile_hint=HINT), *c["plain"], f"{tag} bf16"))
    _report(f"{tag} f32", U.check_f32(Fx.gemm_nt(a, b, bias, epi=Fx.EPI_F32, tile_hint=HINT), *c["plain"], f"{tag} f32"))
    h, u = Fx.gemm_nt(a, b, bias, epi=Fx.EPI_GELU, tile_hint=HINT)
    rh, ru = G.check_gelu(h, u, c["gelu"], f"{tag} gelu")
    _report(f"{tag} gelu h", rh)
    _report(f"{tag} gelu u", ru)
    got = Fx.gemm_nt(a, b, None, epi=Fx.EPI_DGELU, aux=c["aux"], tile_hint=HINT)
    _report(f"{tag} dgelu", U.check_bf16(got, *c["dgelu"], f"{tag} dgelu"))
    got = Fx.gemm_nt(a, b, bias, epi=Fx.EPI_F32_ACC, out=_full((M, N), 0.5, F32), tile_hint=HINT)
    _report(f"{tag} acc", U.check_f32(got, *c["acc"], f"{tag} acc"))


@pytest.mark.parametrize("M,N,K", [(321, 768, 128), (788, 768, 768)])
def test_nt320_strided_operands_in_poisoned_buffers(M, N, K):
    """lda > K, ldb > K, ldc > N, ldaux != ldc, every view starts past row 0 and 8 columns in; inputs sit in NaN, outputs in 7.0.  The
    output parents go on behind the view for the padded rows M .. 320 ceil(M / 320) - 1 of the last row tile and five more: a store
    without its row guard lands there and changes a sentinel."""
    Fx, c = _fx(), _case(M, N, K)
    _is_320(M, N, K)
    tag = f"{M}x{N}x{K} strided"
    (av, _), (bv, _) = U.embed(c["a"], K + 24, 8, 3, 5, U.NAN), U.embed(c["b"], K + 40, 8, 3, 5, U.NAN)
    biasv, _ = U.embed_vec(c["bias"], 5, 3, U.NAN)
    pad = (M + 319) // 320 * 320 - M + 5   # rows behind the view: the padded rows of the last row tile and five more

    def out(dtype, init=U.SENTINEL, extra=0):
        return U.embed(_full((M, N), init, dtype), N + 16 + extra, 8, 3, pad, U.SENTINEL)

    for name, epi, dtype, init, (ref, b32) in (("bf16", Fx.EPI_BF16, BF16, U.SENTINEL, c["plain"]), ("f32", Fx.EPI_F32, F32, U.SENTINEL, c["plain"]),
                                               ("acc", Fx.EPI_F32_ACC, F32, 0.5, c["acc"])):
        cv, cp = out(dtype, init)
        Fx.gemm_nt(av, bv, biasv, epi=epi, out=cv, n=N, tile_hint=HINT)
        U.assert_outside_untouched(cp, cv, U.SENTINEL, f"{tag} {name}")
        _report(f"{tag} {name}", (U.check_bf16 if dtype == BF16 else U.check_f32)(cv, ref, b32, f"{tag} {name}"))
    (hv, hp), (uv, up) = out(BF16), out(BF16, extra=8)
    assert uv.stride(0) != hv.stride(0)
    Fx.gemm_nt(av, bv, biasv, epi=Fx.EPI_GELU, aux=uv, out=hv, n=N, tile_hint=HINT)
    U.assert_outside_untouched(hp, hv, U.SENTINEL, f"{tag} gelu")
    U.assert_outside_untouched(up, uv, U.SENTINEL, f"{tag} gelu aux")
    G.check_gelu(hv, uv, c["gelu"], f"{tag} gelu")
    xv, _ = U.embed(c["aux"], N + 24, 8, 3, 5, U.NAN)
    cv, cp = out(BF16)
    assert xv.stride(0) != cv.stride(0)
    Fx.gemm_nt(av, bv, None, epi=Fx.EPI_DGELU, aux=xv, out=cv, n=N, tile_hint=HINT)
    U.assert_outside_untouched(cp, cv, U.SENTINEL, f"{tag} dgelu")
    _report(f"{tag} dgelu", U.check_bf16(cv, *c["dgelu"], f"{tag} dgelu"))


@pytest.mark.parametrize("M,N,K", [(1000, 768, 768), (788, 768, 3072)])
def test_nt320_is_bit_identical_to_the_256_tile(M, N, K):
    """Every output element is accumulated over K in the same order by the same MFMA as in gemm_nt_256_kernel."""
    Fx, c = _fx(), _case(M, N, K)
    _is_320(M, N, K)
    assert _plan(M, N, K, 0, 5) == (5, 0)
    a, b, bias = c["a"], c["b"], c["bias"]
    for name, kw in (("bf16", dict(bias=bias)), ("f32", dict(bias=bias, epi=Fx.EPI_F32)), ("dgelu", dict(epi=Fx.EPI_DGELU, aux=c["aux"]))):
        assert torch.equal(Fx.gemm_nt(a, b, tile_hint=6, **kw), Fx.gemm_nt(a, b, tile_hint=5, **kw)), f"{M}x{N}x{K} {name}"
    h6, u6 = Fx.gemm_nt(a, b, bias, epi=Fx.EPI_GELU, tile_hint=6)
    h5, u5 = Fx.gemm_nt(a, b, bias, epi=Fx.EPI_GELU, tile_hint=5)
    assert torch.equal(h6, h5) and torch.equal(u6, u5), f"{M}x{N}x{K} gelu"
    acc6 = Fx.gemm_nt(a, b, bias, epi=Fx.EPI_F32_ACC, out=_full((M, N), 0.5, F32), tile_hint=6)
    acc5 = Fx.gemm_nt(a, b, bias, epi=Fx.EPI_F32_ACC, out=_full((M, N), 0.5, F32), tile_hint=5)
    assert torch.equal(acc6, acc5), f"{M}x{N}x{K} acc"


def test_nt320_hint_falls_back_where_the_tile_does_not_fit():
    """N % 256 != 0, and more tiles than one round: hint 6 is planned as hint 0 and the result is that call's."""
    Fx = _fx()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    over = 320 * (cus // 2 + 1)          # x 2 column tiles: one tile more than one workgroup per CU (two where the CU count is odd)
    for M, N, K in ((1000, 520, 64), (over, 512, 64)):
        assert _plan(M, N, K, 0, HINT) == _plan(M, N, K, 0, 0) and _plan(M, N, K, 0, HINT)[0] != 6, (M, N, K)
        a, b, bias = G.random_family(M, N, K, DEV)
        got = Fx.gemm_nt(a, b, bias, tile_hint=HINT)
        _report(f"{M}x{N}x{K} fallback", U.check_bf16(got, *U.nt_bound(a, b, bias), f"{M}x{N}x{K} fallback"))
        assert torch.equal(got, Fx.gemm_nt(a, b, bias, tile_hint=0))
    # the shape the tile was made for: plan queries only
    assert _plan(25216, 768, 768, 0, 6) == (6, 0)
    assert _plan(25216, 768, 768, 0, 0) == (5, 21760)
