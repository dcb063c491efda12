"""The bf16 MFMA GEMMs on strided, offset operands inside poisoned buffers, against the fp64 product of the same bf16 operands.

The model hands every GEMM views (wt[:, D:3*D], logits with a padded row stride, dw[D:3*D], the kv / dkv column blocks, slab offsets);
tests/test_hip_kernels.py only ever passes fresh contiguous operands.  Here every input lives in a NaN-filled parent and every output in
a 7.0-filled one (gemm_strided_util): a wrong leading dimension, a row assumed to start on a 128-byte boundary or a read outside the
view reaches the result as NaN or breaks the elementwise bound, a store outside the view changes a sentinel's bits.  Bounds are per
element and derived from the operands (gemm_strided_util's header); integer operands must come out exact.  Bit-identity to the call on
contiguous copies is asserted next to those, where the summation order is fixed.

Input layouts: "tight" = the view starts 8 elements (16 bytes) into rows of cols + 24 (A / dY) or cols + 40 (B / X) elements -- rows
start 16-byte but not 128-byte aligned -- with 3 poisoned rows before and 5 after; "block" = the middle third of a 3 * cols wide
parent (the qkv[:, D:2*D] / wt[:, D:2*D] shape).  Output layouts: "vec" = ldc % 8 == 0, ldc > N, the view 8 columns in (16-byte
stores at an edge); "scalar" (ragged N) = ldc = N + 2; ldaux = ldc + 8 or N + 4, never ldc."""
import ctypes
import functools

import pytest
import torch

import gemm_strided_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
LAYOUTS = ["tight", "block"]
NO_LIMIT = 2 ** 63 - 1


def _fx():
    from xfm_amd import functional as Fx
    return Fx


def _lib():
    from xfm_amd import _lib
    return _lib


def _rand(shape, scale, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def _in(t, layout, pad):
    C = t.shape[1]
    return U.embed(t, C + pad, 8, 3, 5, U.NAN) if layout == "tight" else U.embed(t, 3 * C, C, 3, 5, U.NAN)


def _out_layouts(N):
    return ["vec"] + (["scalar"] if N % 8 else [])


def _out(t, how, fill, extra=0):
    """t [M, N] (an output's initial content, or the aux input) as a view of a `fill`ed parent.  vec: ld = N rounded up to 8, + 16
    (+ extra), view 8 columns in.  scalar: ld = N + 2 (+ extra), the view one or two columns in, after as many rows as put its first
    element on a 16-byte boundary (what xfm_gemm_nt asks of the C pointer)."""
    M, N = t.shape
    if how == "vec":
        return U.embed(t, (N + 7) // 8 * 8 + 16 + extra, 8, 3, 5, fill)
    ld = N + 2 + extra
    per16 = 16 // t.element_size()
    for col0 in (1, 2, 0):
        for rb in range(1, 17):
            if (rb * ld + col0) % per16 == 0:
                return U.embed(t, ld, col0, rb, 5, fill)
    raise AssertionError(f"no aligned offset for ld {ld}")


def _full(shape, v, dtype):
    return torch.full(shape, v, dtype=dtype, device=DEV)


def _report(what, ratio):
    print(f"  {what}: worst err / bound = {ratio:.3g}")


# ---------------------------------------------------------------------------------------------------------------------- xfm_gemm_nt
@functools.lru_cache(maxsize=2)
def _nt_case(M, N, K):
    """Operands and fp64 references of a shape, made once, shared by its hints and layouts, never written."""
    a, b, bias = _rand((M, K), 1.0, BF16, 1), _rand((N, K), 0.05, BF16, 2), _rand((N,), 0.5, F32, 3)
    aux = _rand((M, N), 1.0, BF16, 4)   # plays gelu'(x) of the forward
    ai, bi = U.int_operands((M, K), 7, 13, DEV), U.int_operands((N, K), 5, 11, DEV)
    biasi = (torch.arange(N, device=DEV) % 5 - 2).float()
    return dict(a=a, b=b, bias=bias, aux=aux, plain=U.nt_bound(a, b, bias), acc=U.nt_bound(a, b, bias, 0.5),
                ai=ai, bi=bi, biasi=biasi, refi=U.nt_bound(ai, bi, biasi)[0])


@functools.lru_cache(maxsize=2)
def _nt_contiguous(M, N, K, hint):
    """What the same calls write on the contiguous operands: every epilogue, once per (shape, hint)."""
    Fx, c = _fx(), _nt_case(M, N, K)
    a, b, bias = c["a"], c["b"], c["bias"]
    out = {"bf16": Fx.gemm_nt(a, b, bias, tile_hint=hint),
           "f32": Fx.gemm_nt(a, b, bias, epi=Fx.EPI_F32, tile_hint=hint),
           "acc": Fx.gemm_nt(a, b, bias, epi=Fx.EPI_F32_ACC, out=_full((M, N), 0.5, F32), tile_hint=hint),
           "dgelu": Fx.gemm_nt(a, b, None, epi=Fx.EPI_DGELU, aux=c["aux"], tile_hint=hint)}
    out["gelu"], out["gelu_aux"] = Fx.gemm_nt(a, b, bias, epi=Fx.EPI_GELU, tile_hint=hint)
    return out


NT_SMALL_HINTS = [1, 2, 3, 4, 7, 8, 0]
NT_CASES = ([(300, 200, 128, h) for h in NT_SMALL_HINTS] + [(5, 3, 64, h) for h in NT_SMALL_HINTS]
            + [(300, 203, 64, h) for h in NT_SMALL_HINTS]   # ragged N on the small tiles: full chunks, then a partial one that is not chunk 0
            + [(16400, 1001, 64, 5),    # 260 tiles of 256 x 256 > CUs: the persistent form, ragged M and N
               (300, 256, 128, 5),      # one workgroup per tile
               (21800, 520, 64, 0)])    # tail split: the second call offsets A, C and aux by rows_a * ld


def _nt_plan(M, N, K, epi, hint):
    cfg, rows_a = ctypes.c_int(), ctypes.c_int()
    L = _lib()
    L.check(L.load().xfm_gemm_nt_plan(M, N, K, epi, hint, ctypes.byref(cfg), ctypes.byref(rows_a)), "gemm_nt_plan")
    return cfg.value, rows_a.value


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,N,K,hint", NT_CASES)
def test_gemm_nt_strided(M, N, K, hint, layout):
    Fx, c = _fx(), _nt_case(M, N, K)
    if (M, N, K, hint) == (21800, 520, 64, 0):
        for epi in range(5):
            assert _nt_plan(M, N, K, epi, hint)[1] > 0, "this shape is here for the tail split"
    (av, _), (bv, _) = _in(c["a"], layout, 24), _in(c["b"], layout, 40)
    biasv, _ = U.embed_vec(c["bias"], 5, 3, U.NAN)
    same = _nt_contiguous(M, N, K, hint)
    for how in _out_layouts(N):
        tag = f"{M}x{N}x{K} hint {hint} {layout}/{how}"
        # plain epilogues: the bound, the sentinels, the bits of the contiguous call
        for name, epi, dtype, init, (ref, b32) in (("bf16", Fx.EPI_BF16, BF16, U.SENTINEL, c["plain"]), ("f32", Fx.EPI_F32, F32, U.SENTINEL, c["plain"]),
                                                   ("acc", Fx.EPI_F32_ACC, F32, 0.5, c["acc"])):
            cv, cp = _out(_full((M, N), init, dtype), how, U.SENTINEL)
            Fx.gemm_nt(av, bv, biasv, epi=epi, out=cv, n=N, tile_hint=hint)
            U.assert_outside_untouched(cp, cv, U.SENTINEL, f"{tag} {name}")
            _report(f"{tag} {name}", (U.check_bf16 if dtype == BF16 else U.check_f32)(cv, ref, b32, f"{tag} {name}"))
            assert torch.equal(cv, same[name]), f"{tag} {name}: differs from the call on contiguous operands"
        # GELU forward: both outputs strided, ldaux != ldc
        hv, hp = _out(_full((M, N), U.SENTINEL, BF16), how, U.SENTINEL)
        uv, up = _out(_full((M, N), U.SENTINEL, BF16), how, U.SENTINEL, extra=8 if how == "vec" else 2)
        assert uv.stride(0) != hv.stride(0)
        Fx.gemm_nt(av, bv, biasv, epi=Fx.EPI_GELU, aux=uv, out=hv, n=N, tile_hint=hint)
        U.assert_outside_untouched(hp, hv, U.SENTINEL, f"{tag} gelu")
        U.assert_outside_untouched(up, uv, U.SENTINEL, f"{tag} gelu aux")
        assert torch.equal(hv, same["gelu"]) and torch.equal(uv, same["gelu_aux"]), f"{tag} gelu: differs from the call on contiguous operands"
        # GELU dgrad: aux-in strided with NaN around it
        xv, _ = _out(c["aux"], how, U.NAN, extra=8 if how == "vec" else 2)
        cv, cp = _out(_full((M, N), U.SENTINEL, BF16), how, U.SENTINEL)
        Fx.gemm_nt(av, bv, None, epi=Fx.EPI_DGELU, aux=xv, out=cv, n=N, tile_hint=hint)
        U.assert_outside_untouched(cp, cv, U.SENTINEL, f"{tag} dgelu")
        assert torch.equal(cv, same["dgelu"]), f"{tag} dgelu: differs from the call on contiguous operands"
    # integer operands: the fp32 output is the exact product
    (av, _), (bv, _) = _in(c["ai"], layout, 24), _in(c["bi"], layout, 40)
    biasv, _ = U.embed_vec(c["biasi"], 5, 3, U.NAN)
    cv, cp = _out(_full((M, N), U.SENTINEL, F32), "vec", U.SENTINEL)
    Fx.gemm_nt(av, bv, biasv, epi=Fx.EPI_F32, out=cv, n=N, tile_hint=hint)
    U.assert_outside_untouched(cp, cv, U.SENTINEL, f"{M}x{N}x{K} hint {hint} {layout} integers")
    U.check_exact(cv, c["refi"], f"{M}x{N}x{K} hint {hint} {layout} integers")


def test_gemm_nt_forced_256_refuses_operands_past_its_offsets():
    """lda = 2^21 at M = 2048: M * lda = 2^32 elements, past the 256 x 256 kernel's 32-bit offsets.  An explicit hint 5 is an error and
    launches nothing (the call sees only pointers and sizes: no large buffer)."""
    L = _lib()
    lib = L.load()
    M, N, K = 2048, 256, 64
    a, b = _full((8, K), 1.0, BF16), _full((N, K), 1.0, BF16)
    out = _full((M, N), U.SENTINEL, BF16)
    rc = lib.xfm_gemm_nt(a.data_ptr(), 1 << 21, b.data_ptr(), K, out.data_ptr(), N, None, None, 0, M, N, K, 0, 5, _fx()._stream())
    assert rc != 0 and b"32-bit" in lib.xfm_last_error()
    torch.cuda.synchronize()
    assert bool((out == U.SENTINEL).all())


def test_gemm_nt_auto_plan_steps_down_for_operands_past_the_256_kernel_offsets():
    """(2048, 5888, 64) is a 256 x 256 shape for the automatic plan (184 tiles).  With A a view into a 2048 x 2^21 parent (8 GiB, only
    the view is written) the plan has to take the operand size into account and run configuration 1, whose row offsets are 64-bit."""
    free, _ = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip(f"needs 12 GiB of free device memory, {free >> 30} GiB are free")
    Fx = _fx()
    M, N, K = 2048, 5888, 64
    assert _nt_plan(M, N, K, Fx.EPI_BF16, 0) == (5, 0)   # the plan of tight operands
    a, b, bias = _rand((M, K), 1.0, BF16, 1), _rand((N, K), 0.05, BF16, 2), _rand((N,), 0.5, F32, 3)
    parent = torch.empty((M, 1 << 21), dtype=BF16, device=DEV)
    av = parent[:, 8:8 + K]
    av.copy_(a)
    bv, _ = _in(b, "tight", 40)
    biasv, _ = U.embed_vec(bias, 5, 3, U.NAN)
    cv, cp = _out(_full((M, N), U.SENTINEL, BF16), "vec", U.SENTINEL)
    Fx.gemm_nt(av, bv, biasv, out=cv, n=N, tile_hint=0)
    U.assert_outside_untouched(cp, cv, U.SENTINEL, "large lda")
    ref, b32 = U.nt_bound(a, b, bias)
    _report("large lda bf16", U.check_bf16(cv, ref, b32, "large lda"))
    with pytest.raises(_lib().XfmHipError, match="32-bit"):
        Fx.gemm_nt(av, bv, biasv, out=cv, n=N, tile_hint=5)
    del parent, av
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------------------------- xfm_gemm_nt_ksplit
def _ksplit(a, b, bias, out, M, N, K):
    Fx, L = _fx(), _lib()
    lib = L.load()
    need = lib.xfm_gemm_nt_ksplit_workspace(M, N, K)
    ws = Fx.workspace(need, a.device) if need > 0 else None
    L.check(lib.xfm_gemm_nt_ksplit(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), int(out.dtype == BF16),
                                   bias.data_ptr(), M, N, K, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4,
                                   Fx._stream()), "gemm_nt_ksplit")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("K,sliced", [(8192, True), (4096, False)])
def test_gemm_nt_ksplit_strided(K, sliced, layout):
    M, N = 64, 128
    assert (_lib().load().xfm_gemm_nt_ksplit_workspace(M, N, K) > 0) == sliced
    a, b, bias = _rand((M, K), 1.0, BF16, 5), _rand((N, K), 0.05, BF16, 6), _rand((N,), 0.5, F32, 7)
    ref, b32 = U.nt_bound(a, b, bias)
    (av, _), (bv, _) = _in(a, layout, 24), _in(b, layout, 40)
    biasv, _ = U.embed_vec(bias, 5, 3, U.NAN)
    for dtype in (BF16, F32):
        tag = f"ksplit K {K} {layout} {dtype}"
        ov, op = _out(_full((M, N), U.SENTINEL, dtype), "vec", U.SENTINEL)
        _ksplit(av, bv, biasv, ov, M, N, K)
        U.assert_outside_untouched(op, ov, U.SENTINEL, tag)
        _report(tag, (U.check_bf16 if dtype == BF16 else U.check_f32)(ov, ref, b32, tag))
        oc = _full((M, N), U.SENTINEL, dtype)
        _ksplit(a, b, bias, oc, M, N, K)
        assert torch.equal(ov, oc), f"{tag}: differs from the call on contiguous operands"


# ---------------------------------------------------------------------------------------------------------------------- xfm_gemm_tn
TN_CASES = [(83, 128, 256, 1),        # ring kernel, ragged M
            (64, 136, 64, 1),         # register-staged kernel with N / K edges
            (2000, 256, 128, 3),      # split planes plus reduce
            (320, 256, 512, -3),      # 256 x 256 kernel
            (2000, 256, 128, -5),     # register-staged kernel
            (2000, 256, 128, -4),     # 256 x 256 kernel forbidden
            (8250, 768, 1536, 0)]     # ragged body plus tail: the second call offsets by M0 * ldy and M0 * ldx


@functools.lru_cache(maxsize=2)
def _tn_case(M, N, K):
    dy, x = _rand((M, N), 1.0, BF16, 10), _rand((M, K), 1.0, BF16, 11)
    return (dy, x) + U.tn_bound(dy, x, 0.5, 0.25)


def _tn_outputs(N, K, layout):
    dw0 = _full((N, K), 0.5, F32)
    dwv, dwp = U.embed(dw0, K + 12, 4, 3, 5, U.SENTINEL) if layout == "tight" else U.embed(dw0, 3 * K, K, 3, 5, U.SENTINEL)
    dbv, dbp = U.embed_vec(_full((N,), 0.25, F32), 5, 3, U.SENTINEL)
    return dwv, dwp, dbv, dbp


def _tn_plan(M, N, K, ldy, ldx, hint):
    kernel, splits, used = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    L = _lib()
    L.check(L.load().xfm_gemm_tn_plan(M, N, K, ldy, ldx, hint, NO_LIMIT if hint >= 0 else 0, kernel, splits, used), "gemm_tn_plan")
    return kernel.value, splits.value, used.value


def _tn_checks(tag, dwv, dwp, dbv, dbp, ref_w, bw, ref_b, bb):
    U.assert_outside_untouched(dwp, dwv, U.SENTINEL, f"{tag} dW")
    U.assert_outside_untouched(dbp, dbv, U.SENTINEL, f"{tag} dbias")
    _report(f"{tag} dW", U.check_f32(dwv, ref_w, bw, f"{tag} dW"))
    _report(f"{tag} dbias", U.check_f32(dbv, ref_b, bb, f"{tag} dbias"))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,N,K,hint", TN_CASES)
def test_gemm_tn_strided(M, N, K, hint, layout):
    Fx = _fx()
    dy, x, ref_w, bw, ref_b, bb = _tn_case(M, N, K)
    (dyv, _), (xv, _) = _in(dy, layout, 24), _in(x, layout, 40)
    kernel, splits, used = _tn_plan(M, N, K, dyv.stride(0), xv.stride(0), hint)
    if hint == 0:
        assert kernel == 0 and M % 64 != 0, "this shape is here for the 256 x 256 body plus the ragged tail"
    tag = f"tn {M}x{N}x{K} hint {hint} {layout}"
    dwv, dwp, dbv, dbp = _tn_outputs(N, K, layout)
    Fx.gemm_tn(dyv, xv, dwv, splits=hint, dbias=dbv)
    _tn_checks(tag, dwv, dwp, dbv, dbp, ref_w, bw, ref_b, bb)
    if hint == 1 or used > 0:   # an ordered merge: one split in place, or workspace planes summed by the reduce kernel
        dwc, dbc = _full((N, K), 0.5, F32), _full((N,), 0.25, F32)
        Fx.gemm_tn(dy, x, dwc, splits=hint, dbias=dbc)
        assert torch.equal(dwv, dwc), f"{tag}: dW differs from the call on contiguous operands"
        if hint == 1:   # (the M-splits meet in dbias through float atomics)
            assert torch.equal(dbv, dbc), f"{tag}: dbias differs from the call on contiguous operands"
    if hint in (1, -3):
        dyi, xi = U.int_operands((M, N), 7, 13, DEV), U.int_operands((M, K), 5, 11, DEV)
        (dyv, _), (xv, _) = _in(dyi, layout, 24), _in(xi, layout, 40)
        dwv, dwp, dbv, dbp = _tn_outputs(N, K, layout)
        Fx.gemm_tn(dyv, xv, dwv, splits=hint, dbias=dbv)
        ri_w, _, ri_b, _ = U.tn_bound(dyi, xi, 0.5, 0.25)
        U.assert_outside_untouched(dwp, dwv, U.SENTINEL, f"{tag} integers dW")
        U.assert_outside_untouched(dbp, dbv, U.SENTINEL, f"{tag} integers dbias")
        U.check_exact(dwv, ri_w, f"{tag} integers dW")
        U.check_exact(dbv, ri_b, f"{tag} integers dbias")


@pytest.mark.parametrize("M,N,K,hint", [(83, 128, 256, 1), (64, 136, 64, 1), (2000, 256, 128, 3)])
def test_gemm_tn_n_smaller_than_dy_columns(M, N, K, hint):
    """dW has fewer rows than dY has columns (n = N on a wider dY): the further columns, NaN here, stay out of dW and dbias."""
    Fx = _fx()
    dy, x, ref_w, bw, ref_b, bb = _tn_case(M, N, K)
    (dyv, dyp), (xv, _) = _in(dy, "tight", 24), _in(x, "tight", 40)
    wide = dyp[3:3 + M, 8:8 + N + 8]
    assert wide.data_ptr() == dyv.data_ptr() and bool(wide[:, N:].isnan().all())
    dwv, dwp, dbv, dbp = _tn_outputs(N, K, "tight")
    Fx.gemm_tn(wide, xv, dwv, n=N, splits=hint, dbias=dbv)
    _tn_checks(f"tn {M}x{N}x{K} hint {hint} n < columns", dwv, dwp, dbv, dbp, ref_w, bw, ref_b, bb)


def test_gemm_tn_batch_strided():
    """Three problems in one launch: the dY are the thirds of one [M, 3N] parent, the X and the dW column blocks of one strided parent
    each, the dbias slices of one vector."""
    Fx, lib = _fx(), _lib().load()
    M, N, K, nb = 1300, 256, 256, 3
    assert lib.xfm_gemm_tn_batch_workspace(nb, M, N, K) > lib.xfm_gemm_tn_workspace(M, N, K), "the batched launch has split planes of its own"
    dys, xs = [_rand((M, N), 1.0, BF16, 30 + i) for i in range(nb)], [_rand((M, K), 1.0, BF16, 40 + i) for i in range(nb)]
    dyp = _full((3 + M + 5, nb * N), U.NAN, BF16)
    xp = _full((3 + M + 5, nb * (K + 16) + 8), U.NAN, BF16)
    dwp = _full((3 + N + 5, nb * (K + 8) + 4), U.SENTINEL, F32)
    dbp = _full((nb * (N + 4) + 4,), U.SENTINEL, F32)
    dyv = [dyp[3:3 + M, i * N:(i + 1) * N] for i in range(nb)]
    xv = [xp[3:3 + M, 8 + i * (K + 16):8 + i * (K + 16) + K] for i in range(nb)]
    dwv = [dwp[3:3 + N, 4 + i * (K + 8):4 + i * (K + 8) + K] for i in range(nb)]
    dbv = [dbp[4 + i * (N + 4):4 + i * (N + 4) + N] for i in range(nb)]
    for i in range(nb):
        dyv[i].copy_(dys[i])
        xv[i].copy_(xs[i])
        dwv[i].fill_(0.5)
        dbv[i].fill_(0.25)
    Fx.gemm_tn_batch(dyv, xv, dwv, dbv)
    U.assert_outside_untouched(dwp, dwv, U.SENTINEL, "tn batch dW")
    U.assert_outside_untouched(dbp, dbv, U.SENTINEL, "tn batch dbias")
    for i in range(nb):
        ref_w, bw, ref_b, bb = U.tn_bound(dys[i], xs[i], 0.5, 0.25)
        _report(f"tn batch {i} dW", U.check_f32(dwv[i], ref_w, bw, f"tn batch {i} dW"))
        _report(f"tn batch {i} dbias", U.check_f32(dbv[i], ref_b, bb, f"tn batch {i} dbias"))
        dwc, dbc = _full((N, K), 0.5, F32), _full((N,), 0.25, F32)   # the single call on contiguous copies meets the same bound
        Fx.gemm_tn(dys[i], xs[i], dwc, dbias=dbc)
        U.check_f32(dwc, ref_w, bw, f"tn single {i} dW")
        U.check_f32(dbc, ref_b, bb, f"tn single {i} dbias")


@pytest.mark.parametrize("integers", [False, True])
def test_gemm_tn_group_strided(integers):
    """Two 256-tileable items (cut stream-K style over a ragged M) and one that falls back to xfm_gemm_tn, dY and X the middle column
    blocks of wider parents, dW strided, dbias on every other item."""
    Fx = _fx()
    M = 1024 + 63
    shapes = [(512, 256), (256, 512), (320, 256)]
    ops, refs = [], []
    for i, (N, K) in enumerate(shapes):
        dy = U.int_operands((M, N), 7, 13, DEV) if integers else _rand((M, N), 1.0, BF16, 50 + i)
        x = U.int_operands((M, K), 5, 11, DEV) if integers else _rand((M, K), 1.0, BF16, 60 + i)
        ops.append((_in(dy, "block", 0)[0], _in(x, "block", 0)[0]))
        refs.append(U.tn_bound(dy, x, 0.5, 0.25))

    def run():
        outs = [_tn_outputs(N, K, "tight") for N, K in shapes]
        Fx.gemm_tn_group([(dyv, xv, o[0], o[2] if i % 2 == 0 else None) for i, ((dyv, xv), o) in enumerate(zip(ops, outs))])
        return outs

    outs = run()
    for i, ((dwv, dwp, dbv, dbp), (ref_w, bw, ref_b, bb)) in enumerate(zip(outs, refs)):
        tag = f"tn group item {i} {'integers' if integers else 'random'}"
        U.assert_outside_untouched(dwp, dwv, U.SENTINEL, f"{tag} dW")
        if i % 2 == 0:
            U.assert_outside_untouched(dbp, dbv, U.SENTINEL, f"{tag} dbias")
        else:   # no dbias passed: nothing of the vector is written
            assert bool((dbv == 0.25).all())
            U.assert_outside_untouched(dbp, dbv, U.SENTINEL, f"{tag} dbias (absent)")
        if integers:
            U.check_exact(dwv, ref_w, f"{tag} dW")
            if i % 2 == 0:
                U.check_exact(dbv, ref_b, f"{tag} dbias")
        else:
            _report(f"{tag} dW", U.check_f32(dwv, ref_w, bw, f"{tag} dW"))
            if i % 2 == 0:
                _report(f"{tag} dbias", U.check_f32(dbv, ref_b, bb, f"{tag} dbias"))
    again = run()
    for i in (0, 1):   # the grouped kernel's pieces are added in workgroup order: the same bits on every run
        assert torch.equal(outs[i][0], again[i][0]), f"tn group item {i}: dW differs between two runs"
    assert torch.equal(outs[0][2], again[0][2]), "tn group item 0: dbias differs between two runs"
