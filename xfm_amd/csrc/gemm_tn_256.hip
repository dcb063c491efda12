// gemm_tn, 256 x 256 tiles (gemm_common.h): one pipeline body, the split-M kernel with its reduce, the grouped persistent kernel with its fix-up.
// ---------------------------------------------------------------------------------------------
// wgrad on the 256 x 256 phase pipeline (see gemm_nt_256_kernel): dW tile 256 (n) x 256 (k), 8 waves as 2 (n) x 4 (k),
// a K-tile = 64 rows of M.  Staging units are [64 m][128 col] images (256-B rows, swz_t on the source address) of the
// column subsets each phase consumes: U0 = dY cols {wr*128 + 0..63}, U1 = X cols {wc*64 + 0..31}, U2 = X cols
// {wc*64 + 32..63}, U3 = dY cols {wr*128 + 64..127}; fragments come out with ds_read_b64_tr_b16.  No bounds checks:
// the launcher only picks this kernel for M % 64 == 0 and N, K % 256 == 0.  The bias gradient (column sums of dY) rides
// on the matrix cores: in the k-tile-0 workgroups wave wc multiplies its wc-th dY fragment of each half with a ones
// fragment (4 extra MFMA per K-tile per wave).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void wait_younger(int y) {  // leave the y youngest units (2 loads each) in flight
  if (y >= 3) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if (y == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if (y == 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One (tile, M-range) of the pipeline: rows [mbeg, mbeg + 64 nk) of dY columns [n0, n0 + 256) against X columns [k0, k0 + 256).
struct Tn256Seg {
  const bf16* dY; const bf16* X;
  unsigned ldy, ldx;
  int n0, k0, mbeg, nk;
  bool do_bias;
  int rows;   // RAGGED: rows of this piece that exist (the last K-step of a problem whose M is no multiple of 64 is short)
};
__device__ __attribute__((aligned(16))) const unsigned tn_zero16[4] = {0u, 0u, 0u, 0u};

// RAGGED: rows at or past sg.rows are staged as zeros (their lanes point the direct-to-LDS load at a 16-byte zero constant).
template <bool RAGGED>
__device__ __forceinline__ void tn256_mainloop(const Tn256Seg& sg, char* smem, f32x4 (&acc)[8][4], f32x4 (&bacc)[2]) {
  constexpr int UNIT = 64 * 256, BUF = 4 * UNIT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 2, wc = w & 3;
  const int lr = lane & 15, lg = lane >> 4;
  const int n0 = sg.n0, k0 = sg.k0, mbeg = sg.mbeg, nk = sg.nk;
  const int total = 4 * nk;
  const bool do_bias = sg.do_bias;

  // per-lane source element offsets (K-tile 0) and wave-uniform LDS destinations of the 8 (unit, instruction) loads
  unsigned soff[4][2];
  int doff[4][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int b = i * 8 + w;                 // 1-KiB block of the unit: rows 4b .. 4b+3
    const int r = 4 * b + (lane >> 4);
    const int c = ((lane & 15) ^ swz_t(r)) * 8;  // logical column (0..127) stored at this lane's 16-B slot
    const unsigned rowy = (unsigned)(mbeg + r) * (unsigned)sg.ldy, rowx = (unsigned)(mbeg + r) * (unsigned)sg.ldx;
    soff[0][i] = rowy + n0 + (c >> 6) * 128 + (c & 63);
    soff[3][i] = rowy + n0 + (c >> 6) * 128 + 64 + (c & 63);
    soff[1][i] = rowx + k0 + (c >> 5) * 64 + (c & 31);
    soff[2][i] = rowx + k0 + (c >> 5) * 64 + 32 + (c & 31);
    doff[0][i] = 0 * UNIT + b * 1024;
    doff[1][i] = 1 * UNIT + b * 1024;
    doff[2][i] = 2 * UNIT + b * 1024;
    doff[3][i] = 3 * UNIT + b * 1024;
  }
  auto issue = [&](int s) {
    if (s >= total) return;
    const int kt = s >> 2, j = s & 3;
    char* base = smem + (kt & 1) * BUF;
    const bool isy = (j == 0 || j == 3);
    const bf16* src = (isy ? sg.dY : sg.X) + (size_t)kt * 64 * (size_t)(isy ? sg.ldy : sg.ldx);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned so = j == 0 ? soff[0][i] : j == 1 ? soff[1][i] : j == 2 ? soff[2][i] : soff[3][i];
      const int dofs = j == 0 ? doff[0][i] : j == 1 ? doff[1][i] : j == 2 ? doff[2][i] : doff[3][i];
      // Issued as inline asm on purpose: when the compiler sees a direct-to-LDS load it drains it (s_waitcnt vmcnt(0)) in
      // front of every ds_read_b64_tr_b16, whose intrinsic carries no alias information -- that serialises the pipeline.
      const unsigned lds_addr = (unsigned)(uintptr_t)LDS_PTR(void, base) + (unsigned)__builtin_amdgcn_readfirstlane(dofs);
      const bf16* ptr = src + (size_t)so;
      if (RAGGED && kt * 64 + 4 * (i * 8 + w) + (lane >> 4) >= sg.rows) ptr = reinterpret_cast<const bf16*>(tn_zero16);
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(ptr), "s"(lds_addr) : "memory", "m0");
    }
  };

#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bacc[0] = bacc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = f2bf(1.0f);

  // per-lane byte offsets of the transposed fragment reads inside a unit image (+ ks * 8192, + 1024 for rows +4)
  const int lrow = 8 * lg + (lr >> 2);
  const int tsw = swz_t(lrow);
  int offa[4], offb[2];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int col = wr * 64 + f * 16 + 4 * (lr & 3);
    offa[f] = lrow * 256 + (((col >> 3) ^ tsw) << 4) + (col & 7) * 2;
  }
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int col = wc * 32 + f * 16 + 4 * (lr & 3);
    offb[f] = lrow * 256 + (((col >> 3) ^ tsw) << 4) + (col & 7) * 2;
  }
  auto tr_pair = [&](const char* p) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, p));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, p + 1024));
    union { struct { s16x4 a, b; } s; bf16x8 v; } u;
    u.s.a = lo;
    u.s.b = hi;
    return u.v;
  };
  bf16x8 xa[4][2], wb0[2][2], wb1[2][2];
  auto read_a = [&](const char* unit) {
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      xa[f][0] = tr_pair(unit + offa[f]);
      xa[f][1] = tr_pair(unit + offa[f] + 8192);
    }
  };
  auto read_b = [&](const char* unit, bf16x8 (&wb)[2][2]) {
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      wb[f][0] = tr_pair(unit + offb[f]);
      wb[f][1] = tr_pair(unit + offb[f] + 8192);
    }
  };
#define XFM_TQUAD(MH, NH, WB)                                                                                    \
  do {                                                                                                           \
    __builtin_amdgcn_s_setprio(1);                                                                               \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                             \
    _Pragma("unroll") for (int m = 0; m < 4; ++m)                                                                \
    _Pragma("unroll") for (int n = 0; n < 2; ++n)                                                                \
      acc[MH * 4 + m][NH * 2 + n] =                                                                              \
          __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[m][ks], WB[n][ks], acc[MH * 4 + m][NH * 2 + n], 0, 0, 0);  \
    __builtin_amdgcn_s_setprio(0);                                                                               \
  } while (0)
#define XFM_TBIAS(H)                                                                                             \
  do {                                                                                                           \
    if (do_bias) {                                                                                               \
      _Pragma("unroll") for (int f = 0; f < 4; ++f)                                                              \
        if (f == wc) {                                                                                           \
          bacc[H] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[f][0], ones, bacc[H], 0, 0, 0);                  \
          bacc[H] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[f][1], ones, bacc[H], 0, 0, 0);                  \
        }                                                                                                        \
    }                                                                                                            \
  } while (0)

#pragma unroll
  for (int s = 0; s < 5; ++s) issue(s);
  wait_younger((total - 1 < 4 ? total - 1 : 4) - 1);
  XFM_BAR();
  if (wr == 1) XFM_BAR();

  for (int kt = 0; kt < nk; ++kt) {
    const char* buf = smem + (kt & 1) * BUF;
    const int ph = 4 * kt;
    int last;
    // ---- P0: (a0, b0)
    issue(ph + 5);
    read_a(buf + 0 * UNIT);
    read_b(buf + 1 * UNIT, wb0);
    last = ph + 5 < total ? ph + 5 : total - 1;
    wait_younger(last - (ph + 2));
    XFM_BAR();
    XFM_TQUAD(0, 0, wb0);
    XFM_TBIAS(0);
    XFM_BAR();
    // ---- P1: (a0, b1)
    issue(ph + 6);
    read_b(buf + 2 * UNIT, wb1);
    last = ph + 6 < total ? ph + 6 : total - 1;
    wait_younger(last - (ph + 3));
    XFM_BAR();
    XFM_TQUAD(0, 1, wb1);
    XFM_BAR();
    // ---- P2: (a1, b1)
    issue(ph + 7);
    read_a(buf + 3 * UNIT);
    XFM_BAR();
    XFM_TQUAD(1, 1, wb1);
    XFM_TBIAS(1);
    XFM_BAR();
    // ---- P3: (a1, b0)
    issue(ph + 8);
    last = ph + 8 < total ? ph + 8 : total - 1;
    wait_younger(last - (ph + 5) < 0 ? 0 : last - (ph + 5));
    XFM_BAR();
    XFM_TQUAD(1, 0, wb0);
    XFM_BAR();
  }
  if (wr == 0) XFM_BAR();
#undef XFM_TQUAD
#undef XFM_TBIAS

}

// the bias gradient of the tile's 256 dY columns: D[i = n][j], every column j holds the same sum; lane (lg, lr = 0) owns rows 4 lg .. 4 lg + 3
template <bool ATOMIC>
__device__ __forceinline__ void tn256_bias_out(float* dbias, int n0, const f32x4 (&bacc)[2]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 2, wc = w & 3, lr = lane & 15, lg = lane >> 4;
  if (lr != 0) return;
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float* d = dbias + n0 + wr * 128 + h * 64 + wc * 16 + 4 * lg + i;
      if (ATOMIC) atomicAdd(d, bacc[h][i]);
      else *d += bacc[h][i];
    }
}
// a cut tile's piece: its share of the 256 column sums parked in the piece's slot (tn_group_fixup_kernel adds the pieces in
// workgroup order: a float atomic per piece moved the last bits of the bias gradient of whichever problem the cut tiles belong to)
__device__ __forceinline__ void tn256_bias_part(float* part, const f32x4 (&bacc)[2]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 2, wc = w & 3, lr = lane & 15, lg = lane >> 4;
  if (lr != 0) return;
#pragma unroll
  for (int h = 0; h < 2; ++h) *reinterpret_cast<f32x4*>(part + wr * 128 + h * 64 + wc * 16 + 4 * lg) = bacc[h];
}
// partial tile -> workspace slot, one coalesced 16-B store per accumulator register quad (the reduce kernels read the same order)
__device__ __forceinline__ void tn256_store_partial(float* ws, long slot, const f32x4 (&acc)[8][4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  f32x4* wsp = reinterpret_cast<f32x4*>(ws) + ((slot * 8 + w) * 32) * 64 + lane;
#pragma unroll
  for (int nt = 0; nt < 8; ++nt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) wsp[(nt * 4 + kt) * 64] = acc[nt][kt];
}
template <bool ATOMIC>
__device__ __forceinline__ void tn256_add_out(float* dW, long ldw, int n0, int k0, const f32x4 (&acc)[8][4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 2, wc = w & 3, lr = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int nt = 0; nt < 8; ++nt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const int k = k0 + wc * 64 + kt * 16 + lr;
#pragma unroll
      for (int rgi = 0; rgi < 4; ++rgi) {
        const int n = n0 + wr * 128 + nt * 16 + 4 * lg + rgi;
        if (ATOMIC) atomicAdd(dW + (long)n * ldw + k, acc[nt][kt][rgi]);
        else dW[(long)n * ldw + k] += acc[nt][kt][rgi];
      }
    }
}

__global__ __launch_bounds__(512) void gemm_tn_256_kernel(GemmTN g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tiles_k = g.K / 256, tiles_n = g.N / 256;
  const int per_split = tiles_k * tiles_n;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int split = wg / per_split, t = wg % per_split;
  const int n0 = (t / tiles_k) * 256, k0 = (t % tiles_k) * 256;
  const int mbeg = split * g.m_per_split;
  int mend = mbeg + g.m_per_split;
  mend = mend < g.M ? mend : g.M;
  const Tn256Seg sg{g.dY, g.X, (unsigned)g.ldy, (unsigned)g.ldx, n0, k0, mbeg, (mend - mbeg) / 64, g.dbias != nullptr && k0 == 0, 0};
  f32x4 acc[8][4], bacc[2];
  tn256_mainloop<false>(sg, smem, acc, bacc);
  if (sg.do_bias) tn256_bias_out<true>(g.dbias, n0, bacc);
  if (g.ws != nullptr) {  // tn_reduce_kernel sums the splits
    tn256_store_partial(g.ws, (long)split * per_split + t, acc);
    return;
  }
  tn256_add_out<true>(g.dW, g.ldw, n0, k0, acc);
}

// ---------------------------------------------------------------------------------------------
// GROUPED weight gradients (round 4): many problems of one M (every projection of several layers) in ONE persistent launch.
// A single wgrad has 9-36 output tiles of 256 x 256 and needs 7+ M-splits to fill 256 CUs: each split writes a 256-KB fp32 partial
// per tile (64 MB per GEMM whatever its shape -- one accumulator tile per CU) that a reduce kernel reads back, ~20 % on top of the MFMA
// loop.  With the tiles of ALL queued problems in one list, workgroup i walks WHOLE tiles i, i + G, ... over the full M (one owner per
// dW element: plain += into the fp32 gradient, bias gradient included) and only the last total % G tiles are cut stream-K style:
// their R = r * nk K-steps are dealt out evenly over the G workgroups (boundaries snapped so that no piece is shorter than 4 steps),
// at most two partial pieces per workgroup go to workspace slots 2 i / 2 i + 1, and a fix-up kernel adds each cut tile's pieces in
// workgroup order -- the same bits on every run.
// ---------------------------------------------------------------------------------------------
#define TN_GROUP_MAX 48
struct TnGroupProb {
  const bf16* dY; const bf16* X;
  float* dW; float* dbias;
  unsigned ldy, ldx;
  long ldw;
  int tiles_k;
  int tile_end;   // prefix: this problem owns tiles [previous tile_end, tile_end)
};
struct TnGroup {
  int nprob, nk;             // problems; K-steps (64 rows of M, the last one possibly short) per tile
  int M;                     // rows
  int total_tiles, full_tiles;
  int sk_wgs;                // workgroups that share the cut tiles (0: none)
  long sk_iters;             // (total_tiles - full_tiles) * nk
  float* ws;
  float* ws_bias;            // 256 floats per partial-piece slot, behind the slots' tiles
  TnGroupProb p[TN_GROUP_MAX];
};
__host__ __device__ __forceinline__ long tn_sk_bound(long R, int nk, int sk_wgs, int i) {
  long raw = (long)i * R / sk_wgs;
  const int rem = (int)(raw % nk);
  if (rem < 4) raw -= rem;
  else if (nk - rem < 4) raw += nk - rem;
  return raw;
}

__global__ __launch_bounds__(512) void gemm_tn_group_kernel(TnGroup G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wg = xcd_remap(blockIdx.x, gridDim.x), nwg = gridDim.x;
  int dp_t = wg;
  long sk_pos = 0, sk_end = 0;
  if (wg < G.sk_wgs) {
    sk_pos = tn_sk_bound(G.sk_iters, G.nk, G.sk_wgs, wg);
    sk_end = tn_sk_bound(G.sk_iters, G.nk, G.sk_wgs, wg + 1);
  }
  const long sk_a = sk_pos;
  bool first = true;
  for (;;) {   // (everything that steers this loop is a function of blockIdx: uniform over the workgroup)
    int tile, it0, it1;
    long slot = -1;   // >= 0: partial piece
    if (dp_t < G.full_tiles) {
      tile = dp_t;
      dp_t += nwg;
      it0 = 0;
      it1 = G.nk;
    } else if (sk_pos < sk_end) {
      const int rt = (int)(sk_pos / G.nk);
      const long t_end = (long)(rt + 1) * G.nk;
      it0 = (int)(sk_pos - (long)rt * G.nk);
      it1 = (int)((sk_end < t_end ? sk_end : t_end) - (long)rt * G.nk);
      tile = G.full_tiles + rt;
      if (it0 != 0 || it1 != G.nk) slot = 2l * wg + (sk_pos == sk_a ? 0 : 1);
      sk_pos = (long)rt * G.nk + it1;
    } else {
      break;
    }
    if (!first) __syncthreads();   // the previous piece's LDS reads are over before this one's staging lands
    first = false;
    int pi = 0;
    while (pi + 1 < G.nprob && tile >= G.p[pi].tile_end) ++pi;
    const TnGroupProb& P = G.p[pi];
    const int tl = tile - (pi > 0 ? G.p[pi - 1].tile_end : 0);
    const int n0 = (tl / P.tiles_k) * 256, k0 = (tl % P.tiles_k) * 256;
    const Tn256Seg sg{P.dY, P.X, P.ldy, P.ldx, n0, k0, it0 * 64, it1 - it0, P.dbias != nullptr && k0 == 0, G.M - it0 * 64};
    f32x4 acc[8][4], bacc[2];
    tn256_mainloop<true>(sg, smem, acc, bacc);
    if (slot >= 0) {
      if (sg.do_bias) tn256_bias_part(G.ws_bias + slot * 256, bacc);
      tn256_store_partial(G.ws, slot, acc);
    } else {
      if (sg.do_bias) tn256_bias_out<false>(P.dbias, n0, bacc);
      tn256_add_out<false>(P.dW, P.ldw, n0, k0, acc);
    }
  }
}

// the cut tiles: dW += the pieces in workgroup order.  grid (64, cut tiles): one thread per accumulator quad, as tn_reduce_kernel.
__global__ __launch_bounds__(256) void tn_group_fixup_kernel(TnGroup G) {
  const int rt = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;   // < 8 * 32 * 64
  const long R = G.sk_iters;
  const long a = (long)rt * G.nk, b = a + G.nk;
  int i0 = (int)(a * G.sk_wgs / R);
  i0 = i0 < G.sk_wgs - 1 ? i0 : G.sk_wgs - 1;
  while (i0 > 0 && tn_sk_bound(R, G.nk, G.sk_wgs, i0) > a) --i0;
  while (i0 + 1 < G.sk_wgs && tn_sk_bound(R, G.nk, G.sk_wgs, i0 + 1) <= a) ++i0;
  int i1 = i0;
  while (i1 + 1 < G.sk_wgs && tn_sk_bound(R, G.nk, G.sk_wgs, i1 + 1) < b) ++i1;
  if (i0 == i1) return;   // one workgroup walked the whole tile and added it to dW itself
  const f32x4* ws = reinterpret_cast<const f32x4*>(G.ws);
  f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = i0; i <= i1; ++i) {
    const long slot = 2l * i + (tn_sk_bound(R, G.nk, G.sk_wgs, i) >= a ? 0 : 1);
    sum += ws[slot * (8 * 32 * 64) + idx];
  }
  const int tile = G.full_tiles + rt;
  int pi = 0;
  while (pi + 1 < G.nprob && tile >= G.p[pi].tile_end) ++pi;
  const TnGroupProb& P = G.p[pi];
  const int tl = tile - (pi > 0 ? G.p[pi - 1].tile_end : 0);
  const int n0 = (tl / P.tiles_k) * 256, k0 = (tl % P.tiles_k) * 256;
  const int lane = idx & 63, q = (idx >> 6) & 31, w = idx >> 11;
  const int wr = w >> 2, wc = w & 3, lr = lane & 15, lg = lane >> 4, nt = q >> 2, kt = q & 3;
  const int k = k0 + wc * 64 + kt * 16 + lr;
  const int n = n0 + wr * 128 + nt * 16 + 4 * lg;
#pragma unroll
  for (int i = 0; i < 4; ++i) P.dW[(long)(n + i) * P.ldw + k] += sum[i];
  if (blockIdx.x == 0 && P.dbias != nullptr && k0 == 0) {   // the pieces' column sums, same order (256 threads, one column each)
    float b = 0.f;
    for (int i = i0; i <= i1; ++i) {
      const long slot = 2l * i + (tn_sk_bound(R, G.nk, G.sk_wgs, i) >= a ? 0 : 1);
      b += G.ws_bias[slot * 256 + threadIdx.x];
    }
    P.dbias[n0 + threadIdx.x] += b;
  }
}

// dW += sum over splits of the partial tiles written by gemm_tn_256_kernel (deterministic: fixed summation order).
// One thread per accumulator quad: (tile t, wave w, quad q = nt*4+kt, lane) -> rows n..n+3 at column k.
__global__ __launch_bounds__(256) void tn_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dW, long ldw, int tiles_k,
                                                        int per_split, int splits) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // < per_split * 8 * 32 * 64
  const int lane = (int)(idx & 63), q = (int)((idx >> 6) & 31), w = (int)((idx >> 11) & 7);
  const int t = (int)(idx >> 14);
  if (t >= per_split) return;
  const f32x4* p = reinterpret_cast<const f32x4*>(ws) + idx;
  const long stride = (long)per_split * 8 * 32 * 64;
  f32x4 sum = p[0];
  for (int sp = 1; sp < splits; ++sp) {
    const f32x4 v = p[sp * stride];
    sum += v;
  }
  const int n0 = (t / tiles_k) * 256, k0 = (t % tiles_k) * 256;
  const int wr = w >> 2, wc = w & 3, lr = lane & 15, lg = lane >> 4, nt = q >> 2, kt = q & 3;
  const int k = k0 + wc * 64 + kt * 16 + lr;
  const int n = n0 + wr * 128 + nt * 16 + 4 * lg;
#pragma unroll
  for (int i = 0; i < 4; ++i) dW[(long)(n + i) * ldw + k] += sum[i];
}
