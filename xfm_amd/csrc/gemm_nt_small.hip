// gemm_nt, small tiles: BM x BN in {128 x 128, 64 x 128, 64 x 64} on 2 - 4 LDS stages, and the 256 x 128 three-slot ring (gemm_common.h).

// NS = LDS stages: 2 = load K-tile kt+1 while computing kt (enough when several workgroups share a CU); 3 / 4 keep one / two
// more K-tiles in flight behind a counted s_waitcnt -- for the small-M problems (text tower) where a CU holds one or two
// workgroups and each K-step would otherwise expose the full L2 latency.
template <int BM, int BN, int EPI, int NS>
__global__ __launch_bounds__(256) void gemm_nt_kernel(GemmNT g) {
  constexpr int MT = BM / 32, NT = BN / 32;
  constexpr int LOADS = (BM + BN) / 32;  // direct-to-LDS loads per thread per stage
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int lr = lane & 15, lg = lane >> 4;
  const int tiles_n = (g.N + BN - 1) / BN, tiles_m = (g.M + BM - 1) / BM;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  int tm, tn;
  grouped_tile(wg, tiles_m, tiles_n, g.group_m, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  // K-slice of this workgroup (k_splits > 1: the LM-head dgrad, K = 50304 against 90 output tiles)
  const int nk_all = g.K / 64;
  const int nk_per = (nk_all + g.k_splits - 1) / g.k_splits;
  const int kt0 = blockIdx.y * nk_per;
  const int nk = nk_all - kt0 < nk_per ? nk_all - kt0 : nk_per;
  if (nk <= 0) return;  // workgroup-uniform, before any barrier
  auto stage = [&](int buf, int kt) {
    char* sA = smem + buf * STAGE;
    char* sB = sA + A_BYTES;
    const int k0 = (kt0 + kt) * 64;
#pragma unroll
    for (int i = 0; i < BM / 32; ++i) {
      const int blk = i * 4 + w;  // one wave-instruction fills 1 KiB = 8 rows x 128 B, lane-linear
      const int r = blk * 8 + (lane >> 3);
      const int c = (lane & 7) ^ swz_x(r);
      int gr = m0 + r;
      gr = gr < g.M ? gr : g.M - 1;
      const bf16* src = g.A + (long)gr * g.lda + k0 + c * 8;
      __builtin_amdgcn_global_load_lds(GLB_PTR(void, src), LDS_PTR(void, sA + blk * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < BN / 32; ++i) {
      const int blk = i * 4 + w;
      const int r = blk * 8 + (lane >> 3);
      const int c = (lane & 7) ^ swz_w(r);
      int gr = n0 + r;
      gr = gr < g.N ? gr : g.N - 1;
      const bf16* src = g.B + (long)gr * g.ldb + k0 + c * 8;
      __builtin_amdgcn_global_load_lds(GLB_PTR(void, src), LDS_PTR(void, sB + blk * 1024), 16, 0, 0);
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-lane LDS row of each fragment (constant over the K loop)
  int xrow[MT], wrow[NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) xrow[mt] = wm * (BM / 2) + mt * 16 + lr;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) wrow[nt] = wn * (BN / 2) + (nt >> 1) * 32 + 8 * (lr >> 2) + 4 * (nt & 1) + (lr & 3);

  if (NS == 2) {
    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  } else {
#pragma unroll
    for (int s0 = 0; s0 < NS - 1; ++s0)
      if (s0 < nk) stage(s0, s0);
  }
  int slot = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (NS == 2) {
      if (kt + 1 < nk) stage((kt & 1) ^ 1, kt + 1);
    } else {
      // stage kt must have landed; the younger stages kt+1 .. kt+NS-2 (where they exist) stay in flight across the barrier
      const int younger = nk - 1 - kt < NS - 2 ? nk - 1 - kt : NS - 2;
      if (younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LOADS) : "memory");
      else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LOADS) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      XFM_BAR();  // everyone's share of stage kt has landed; everyone is done reading the slot of stage kt-1
      if (kt + NS - 1 < nk) stage(slot == 0 ? NS - 1 : slot - 1, kt + NS - 1);
    }
    const int cur = NS == 2 ? (kt & 1) : slot;
    const char* sA = smem + cur * STAGE;
    const char* sB = sA + A_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = ks * 4 + lg;
      bf16x8 xf[MT], wf[NT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        xf[mt] = *reinterpret_cast<const bf16x8*>(sA + xrow[mt] * 128 + ((c ^ swz_x(xrow[mt])) << 4));
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        wf[nt] = *reinterpret_cast<const bf16x8*>(sB + wrow[nt] * 128 + ((c ^ swz_w(wrow[nt])) << 4));
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], xf[mt], acc[mt][nt], 0, 0, 0);
    }
    if (NS == 2) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    } else {
      slot = slot == NS - 1 ? 0 : slot + 1;
    }
  }

  gemm_epilogue<MT, NT, EPI>(g, acc, m0 + wm * (BM / 2), n0 + wn * (BN / 2), lr, lg);
}

// ---------------------------------------------------------------------------------------------
// Large-M variant: 256 x 128 tile, 8 waves (4 x 2, the same 64 x 64 micro-kernel per wave), one workgroup per CU, and a
// 3-slot LDS ring (3 x 48 KiB) filled by direct-to-LDS loads that stay in flight ACROSS the per-step barrier: a counted
// s_waitcnt vmcnt(6) retires only the slot about to be read while the next slot's 6 loads per wave keep flying, and
// the slot after that is issued right behind the barrier.  The projections of this model sit at the MI355X ridge
// (N = 768, K = 768: ~370 FLOP/B), so bytes in flight per CU, not MFMA issue, decide their speed.
// ---------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(512) void gemm_nt_ring_kernel(GemmNT g) {
  constexpr int BM = 256, BN = 128, MT = 4, NT = 4;
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;  // 48 KiB
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w >> 1, wn = w & 1;
  const int lr = lane & 15, lg = lane >> 4;
  const int tiles_n = (g.N + BN - 1) / BN, tiles_m = (g.M + BM - 1) / BM;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  int tm, tn;
  grouped_tile(wg, tiles_m, tiles_n, g.group_m, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  auto stage = [&](int slot, int kt) {  // 48 wave-instructions of 1 KiB: 6 per wave (4 of A, 2 of B)
    char* sA = smem + slot * STAGE;
    char* sB = sA + A_BYTES;
    const int k0 = kt * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int blk = i * 8 + w;
      const int r = blk * 8 + (lane >> 3);
      const int c = (lane & 7) ^ swz_x(r);
      int gr = m0 + r;
      gr = gr < g.M ? gr : g.M - 1;
      __builtin_amdgcn_global_load_lds(GLB_PTR(void, g.A + (long)gr * g.lda + k0 + c * 8), LDS_PTR(void, sA + blk * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int blk = i * 8 + w;
      const int r = blk * 8 + (lane >> 3);
      const int c = (lane & 7) ^ swz_w(r);
      int gr = n0 + r;
      gr = gr < g.N ? gr : g.N - 1;
      __builtin_amdgcn_global_load_lds(GLB_PTR(void, g.B + (long)gr * g.ldb + k0 + c * 8), LDS_PTR(void, sB + blk * 1024), 16, 0, 0);
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  int xrow[MT], wrow[NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) xrow[mt] = wm * 64 + mt * 16 + lr;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) wrow[nt] = wn * 64 + (nt >> 1) * 32 + 8 * (lr >> 2) + 4 * (nt & 1) + (lr & 3);

  const int nk = g.K / 64;
  stage(0, 0);
  if (nk > 1) stage(1, 1);
  int slot = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // retire slot `kt` (this wave's share), keep the 6 loads of slot kt+1 in flight across the barrier
    if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave's share of slot kt has landed; everyone is done reading slot kt-1
    if (kt + 2 < nk) stage(slot == 0 ? 2 : slot - 1, kt + 2);  // (kt+2) % 3 == (kt-1) % 3: the slot just released
    const char* sA = smem + slot * STAGE;
    const char* sB = sA + A_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = ks * 4 + lg;
      bf16x8 xf[MT], wf[NT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        xf[mt] = *reinterpret_cast<const bf16x8*>(sA + xrow[mt] * 128 + ((c ^ swz_x(xrow[mt])) << 4));
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        wf[nt] = *reinterpret_cast<const bf16x8*>(sB + wrow[nt] * 128 + ((c ^ swz_w(wrow[nt])) << 4));
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt], xf[mt], acc[mt][nt], 0, 0, 0);
    }
    slot = slot == 2 ? 0 : slot + 1;
  }
  gemm_epilogue<MT, NT, EPI>(g, acc, m0 + wm * 64, n0 + wn * 64, lr, lg);
}

// ---- host side ----
static int launch_nt_ring(const GemmNT& g, int epi, hipStream_t st) {
  constexpr int lds = 3 * (256 + 128) * 128;
  const int tiles = cdiv(g.M, 256) * cdiv(g.N, 128);
  const int rc = nt_with_epilogue(epi, [&](auto e) { lds_launch<gemm_nt_ring_kernel<decltype(e)::value>, lds>(dim3(tiles), dim3(512), lds, st, g); });
  return rc != XFM_OK ? rc : xfm_check_launch("gemm_nt_ring");
}

template <int BM, int BN, int NS>
static int launch_nt(const GemmNT& g, int epi, hipStream_t st) {
  constexpr int lds = NS * (BM + BN) * 128;
  const dim3 grid(cdiv(g.M, BM) * cdiv(g.N, BN), g.k_splits);
  const int rc = nt_with_epilogue(epi, [&](auto e) { lds_launch<gemm_nt_kernel<BM, BN, decltype(e)::value, NS>, lds>(grid, dim3(256), lds, st, g); });
  return rc != XFM_OK ? rc : xfm_check_launch("gemm_nt");
}
