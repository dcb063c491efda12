// gemm_tn, 128 x 128 tiles (gemm_common.h): the register-staged kernel, the 4-slot ring kernel and the reduce of their split partials.
// ---------------------------------------------------------------------------------------------
// wgrad: dW[N,K] += dY[M,N]^T . X[M,K]   (contraction over the row index of both operands)
// Both tiles are staged row-major ([m][n], [m][k], 256-B rows) and consumed with the gfx950 transposed LDS
// read ds_read_b64_tr_b16, which hands each lane 4 consecutive m for its own column.
// ---------------------------------------------------------------------------------------------
// Several weight gradients of ONE shape in one launch (the three 768 x 768 projections of a fusion layer: 36 tiles each would
// need 9 splits apiece to fill the chip; together they are 108 tiles x 4 splits, one launch and one reduce instead of three).
#define TN_BATCH_MAX 4
struct TnBatch {
  int nb;           // 1 = plain call (the arrays are unused)
  int wg_per;       // workgroups per problem
  long ws_stride;   // floats of workspace per problem
  const bf16* dY[TN_BATCH_MAX];
  const bf16* X[TN_BATCH_MAX];
  float* dW[TN_BATCH_MAX];
  float* dbias[TN_BATCH_MAX];
};

__device__ __forceinline__ bf16x8 tr_read_pair(const char* tile, int row0, int col0, int lr) {
  // rows row0..row0+3 then row0+4..row0+7, columns col0..col0+15; lane lr (0..15 in its 16-lane group) gets column lr
  const int r = row0 + (lr >> 2);
  const int col = col0 + 4 * (lr & 3);
  const int off0 = r * 256 + ((((col >> 3)) ^ swz_t(r)) << 4) + (col & 7) * 2;
  const int r2 = r + 4;
  const int off1 = r2 * 256 + ((((col >> 3)) ^ swz_t(r2)) << 4) + (col & 7) * 2;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, tile + off0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, tile + off1));
  union { struct { s16x4 a, b; } s; bf16x8 v; } u;
  u.s.a = lo;
  u.s.b = hi;
  return u.v;
}

__global__ __launch_bounds__(256) void gemm_tn_kernel(GemmTN g) {
  constexpr int TILE = 64 * 256;  // 64 m-rows x 128 columns bf16
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wn = w >> 1, wk = w & 1;
  const int lr = lane & 15, lg = lane >> 4;
  const int tiles_k = (g.K + 127) / 128, tiles_n = (g.N + 127) / 128;
  const int per_split = tiles_k * tiles_n;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int split = wg / per_split, t = wg % per_split;
  const int n0 = (t / tiles_k) * 128, k0 = (t % tiles_k) * 128;
  const int mbeg = split * g.m_per_split;
  int mend = mbeg + g.m_per_split;
  mend = mend < g.M ? mend : g.M;
  const int nsteps = (mend - mbeg + 63) / 64;

  const bool do_bias = g.dbias != nullptr && k0 == 0;
  float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // this thread's 8 dY columns (chunk tid & 15), over its rows
  u32x4 ry[4], rx[4];
  auto gload = [&](int step) {
    const int mb = mbeg + step * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = i * 256 + tid, r = q >> 4, c = q & 15;
      const int m = mb + r;
      const bool okm = m < mend;
      const int nn = n0 + c * 8, kk = k0 + c * 8;
      ry[i] = u32x4{0, 0, 0, 0};
      rx[i] = u32x4{0, 0, 0, 0};
      if (okm && nn < g.N) {
        if (nn + 8 <= g.N) ry[i] = *reinterpret_cast<const u32x4*>(g.dY + (long)m * g.ldy + nn);
        else {
          union { bf16 h[8]; u32x4 v; } u; u.v = u32x4{0, 0, 0, 0};
          for (int e = 0; e < 8; ++e) if (nn + e < g.N) u.h[e] = g.dY[(long)m * g.ldy + nn + e];
          ry[i] = u.v;
        }
      }
      if (okm && kk < g.K) rx[i] = *reinterpret_cast<const u32x4*>(g.X + (long)m * g.ldx + kk);  // K % 8 == 0
    }
  };
  auto lstore = [&](int buf) {
    char* sY = smem + buf * 2 * TILE;
    char* sX = sY + TILE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = i * 256 + tid, r = q >> 4, c = q & 15;
      const int off = r * 256 + ((c ^ swz_t(r)) << 4);
      *reinterpret_cast<u32x4*>(sY + off) = ry[i];
      *reinterpret_cast<u32x4*>(sX + off) = rx[i];
      if (do_bias) {  // consumed here (after the MFMAs), never at the load site: the loads must stay in flight
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          bsum[2 * e] += __uint_as_float(ry[i][e] << 16);
          bsum[2 * e + 1] += __uint_as_float(ry[i][e] & 0xFFFF0000u);
        }
      }
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (nsteps > 0) {
    gload(0);
    lstore(0);
  }
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int cur = s & 1;
    if (s + 1 < nsteps) gload(s + 1);
    const char* sY = smem + cur * 2 * TILE;
    const char* sX = sY + TILE;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) af[nt] = tr_read_pair(sY, ks * 32 + 8 * lg, wn * 64 + nt * 16, lr);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) bfr[kt] = tr_read_pair(sX, ks * 32 + 8 * lg, wk * 64 + kt * 16, lr);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
          acc[nt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[nt], bfr[kt], acc[nt][kt], 0, 0, 0);
    }
    if (s + 1 < nsteps) lstore(cur ^ 1);
    __syncthreads();
  }

  if (do_bias) {  // fold the 16 row-slices of each column chunk through LDS (the tiles are no longer needed)
    float* red = reinterpret_cast<float*>(smem);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) red[(tid >> 4) * 128 + (tid & 15) * 8 + e] = bsum[e];
    __syncthreads();
    if (tid < 128 && n0 + tid < g.N) {
      float t2 = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) t2 += red[r * 128 + tid];
      atomicAdd(g.dbias + n0 + tid, t2);
    }
  }
  if (g.ws != nullptr) {  // split partial in accumulator-register order (coalesced 16-B stores); tn_reduce128_kernel sums them
    f32x4* wsp = reinterpret_cast<f32x4*>(g.ws) + ((((long)split * per_split + t) * 4 + w) * 16) * 64 + lane;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) wsp[(nt * 4 + kt) * 64] = acc[nt][kt];
    return;
  }
  // D[i = n slot][j = k col]: lane (lg, lr) holds k = ..+lr and n = ..+4*lg+reg
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const int k = k0 + wk * 64 + kt * 16 + lr;
#pragma unroll
      for (int rgi = 0; rgi < 4; ++rgi) {
        const int n = n0 + wn * 64 + nt * 16 + 4 * lg + rgi;
        if (n < g.N && k < g.K) {
          float* dst = g.dW + (long)n * g.ldw + k;
          if (g.direct) *dst += acc[nt][kt][rgi];  // single split: this workgroup is the element's only writer
          else atomicAdd(dst, acc[nt][kt][rgi]);
        }
      }
    }
}

// ---------------------------------------------------------------------------------------------
// wgrad, 128 x 128 tile on a 4-slot LDS ring (the mid-size problems: M of a few thousand token rows, the text / fusion towers).
// The register-staged kernel above keeps ONE K-step in flight, and at two workgroups per CU every 64-row step exposes the
// load latency (measured 1.7 us per step against 0.22 us of MFMA).  Here a step is 32 rows of M (one MFMA k-slice): two
// [32 m][128 col] images (256-B rows, swz_t on the SOURCE address) = 16 KB, filled by direct-to-LDS loads issued as inline
// asm (see gemm_tn_256_kernel: the compiler would drain them in front of every transposed LDS read); THREE steps stay in
// flight behind a counted s_waitcnt vmcnt(8) and one raw barrier per step.  4 waves as 2 (n) x 2 (k), 64 x 64 each -- the
// register layout of gemm_tn_kernel, so the split partials go through the same tn_reduce128_kernel.  Rows past the end of a
// split read a zero row (a wgrad must not see clamped rows).  Needs N % 128 == 0 and K % 128 == 0; the bias gradient rides on
// the matrix cores (dY fragment x ones) in the k-tile-0 workgroups.
// ---------------------------------------------------------------------------------------------
__device__ __attribute__((aligned(256))) static const uint32_t g_zero_row[64] = {0};

__global__ __launch_bounds__(256) void gemm_tn_ring_kernel(GemmTN g, TnBatch bt) {
  constexpr int IMG = 32 * 256, STG = 2 * IMG, NS = 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wn = w >> 1, wk = w & 1;
  const int lr = lane & 15, lg = lane >> 4;
  const int tiles_k = g.K / 128, tiles_n = g.N / 128;
  const int per_split = tiles_k * tiles_n;
  int wg = xcd_remap(blockIdx.x, gridDim.x);
  if (bt.nb > 1) {  // which problem of the batch (wave-uniform: scalar loads from the argument arrays)
    const int bi = wg / bt.wg_per;
    wg -= bi * bt.wg_per;
    g.dY = bt.dY[bi];
    g.X = bt.X[bi];
    g.dW = bt.dW[bi];
    g.dbias = bt.dbias[bi];
    g.ws += (long)bi * bt.ws_stride;
  }
  const int split = wg / per_split, t = wg % per_split;
  const int n0 = (t / tiles_k) * 128, k0 = (t % tiles_k) * 128;
  const int mbeg = split * g.m_per_split;
  int mend = mbeg + g.m_per_split;
  mend = mend < g.M ? mend : g.M;
  const int nsteps = (mend - mbeg + 31) / 32;
  const bool do_bias = g.dbias != nullptr && k0 == 0 && wk == 0;

  // this wave's 4 loads of a step: blocks {w, w + 4} of the dY image and of the X image (a block = 4 rows x 256 B = 1 KiB)
  const bf16* zrow = reinterpret_cast<const bf16*>(g_zero_row);
  int lrow[2], lcol[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    lrow[i] = 4 * (i * 4 + w) + (lane >> 4);
    lcol[i] = ((lane & 15) ^ swz_t(lrow[i])) * 8;  // logical column stored at this lane's 16-B slot
  }
  auto issue = [&](int s) {
    if (s >= nsteps) return;
    char* base = smem + (s & (NS - 1)) * STG;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = mbeg + s * 32 + lrow[i];
      const bool ok = m < mend;
      const bf16* sy = ok ? g.dY + (long)m * g.ldy + n0 + lcol[i] : zrow + lcol[i];
      const bf16* sx = ok ? g.X + (long)m * g.ldx + k0 + lcol[i] : zrow + lcol[i];
      const unsigned dy_lds = (unsigned)(uintptr_t)LDS_PTR(void, base) + (unsigned)__builtin_amdgcn_readfirstlane((i * 4 + w) * 1024);
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(sy), "s"(dy_lds) : "memory", "m0");
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(sx), "s"(dy_lds + (unsigned)IMG) : "memory", "m0");
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 bacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) bacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = f2bf(1.0f);

  issue(0);
  issue(1);
  issue(2);
  for (int s = 0; s < nsteps; ++s) {
    // step s has landed (this wave's share); the younger steps s+1, s+2 (4 loads each, where they exist) stay in flight
    const int younger = nsteps - 1 - s < 2 ? nsteps - 1 - s : 2;
    if (younger == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    XFM_BAR();      // every wave's share of step s is in LDS; everyone is done reading step s-1, whose slot step s+3 reuses
    issue(s + 3);
    const char* sY = smem + (s & (NS - 1)) * STG;
    const char* sX = sY + IMG;
    bf16x8 af[4], bfr[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) af[nt] = tr_read_pair(sY, 8 * lg, wn * 64 + nt * 16, lr);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) bfr[kt] = tr_read_pair(sX, 8 * lg, wk * 64 + kt * 16, lr);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
        acc[nt][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[nt], bfr[kt], acc[nt][kt], 0, 0, 0);
    if (do_bias) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) bacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[nt], ones, bacc[nt], 0, 0, 0);
    }
  }

  if (do_bias && lr == 0) {  // D[i = n][j]: every column j holds the same sum; lane (lg, lr = 0) owns rows 4*lg .. 4*lg+3
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int i = 0; i < 4; ++i) atomicAdd(g.dbias + n0 + wn * 64 + nt * 16 + 4 * lg + i, bacc[nt][i]);
  }
  if (g.ws != nullptr) {  // split partial in accumulator-register order (coalesced 16-B stores); tn_reduce128_kernel sums them
    f32x4* wsp = reinterpret_cast<f32x4*>(g.ws) + ((((long)split * per_split + t) * 4 + w) * 16) * 64 + lane;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) wsp[(nt * 4 + kt) * 64] = acc[nt][kt];
    return;
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const int k = k0 + wk * 64 + kt * 16 + lr;
#pragma unroll
      for (int rgi = 0; rgi < 4; ++rgi) {
        const int n = n0 + wn * 64 + nt * 16 + 4 * lg + rgi;
        float* dst = g.dW + (long)n * g.ldw + k;
        if (g.direct) *dst += acc[nt][kt][rgi];  // single split: this workgroup is the element's only writer
        else atomicAdd(dst, acc[nt][kt][rgi]);
      }
    }
}

// dW += sum over splits of the 128 x 128 partial tiles (register order of gemm_tn_kernel), fixed summation order.
__global__ __launch_bounds__(256) void tn_reduce128_kernel(const float* __restrict__ ws, float* __restrict__ dW, long ldw, int N, int K,
                                                           int tiles_k, int per_split, int splits, TnBatch bt) {
  if (bt.nb > 1) {  // grid.y = problem
    ws += (long)blockIdx.y * bt.ws_stride;
    dW = bt.dW[blockIdx.y];
  }
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // (tile t, wave w, quad q = nt*4+kt, lane)
  const int lane = (int)(idx & 63), q = (int)((idx >> 6) & 15), w = (int)((idx >> 10) & 3);
  const int t = (int)(idx >> 12);
  if (t >= per_split) return;
  const f32x4* p = reinterpret_cast<const f32x4*>(ws) + idx;
  const long stride = (long)per_split * 4 * 16 * 64;
  f32x4 sum = p[0];
  for (int sp = 1; sp < splits; ++sp) sum += p[sp * stride];
  const int n0 = (t / tiles_k) * 128, k0 = (t % tiles_k) * 128;
  const int wn = w >> 1, wk = w & 1, lr = lane & 15, lg = lane >> 4, nt = q >> 2, kt = q & 3;
  const int k = k0 + wk * 64 + kt * 16 + lr;
  const int n = n0 + wn * 64 + nt * 16 + 4 * lg;
  if (k >= K) return;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (n + i < N) dW[(long)(n + i) * ldw + k] += sum[i];
}
