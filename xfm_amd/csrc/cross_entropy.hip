// Cross-entropy on fp32 logits, one workgroup per row: one-hot labels, soft / label-smoothed targets, the one-pass evaluation.
#include "common.h"

// Vocabulary cross-entropy on fp32 logits [R, ld] (xroberta.py:1296-1297, CrossEntropyLoss(ignore_index=-100)).
// forward: per-row logsumexp and loss (0 for ignored rows).  backward: dlogits (bf16) = (softmax - onehot) * scale[0],
// zero in ignored rows and in the padding columns [V, ldd).
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ logits, long ld, int V, const int64_t* __restrict__ labels,
                                                     float* __restrict__ lse, float* __restrict__ loss) {
  __shared__ float red[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)row * ld;
  float mx = -3.0e38f;
  for (int c = tid * 4; c < V; c += 1024) {
    if (c + 4 <= V) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(x + c);
      mx = fmaxf(fmaxf(mx, fmaxf(a[0], a[1])), fmaxf(a[2], a[3]));
    } else {
      for (int i = c; i < V; ++i) mx = fmaxf(mx, x[i]);
    }
  }
  mx = block_max256(mx, red);
  float s = 0.f;
  for (int c = tid * 4; c < V; c += 1024) {
    if (c + 4 <= V) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(x + c);
      s += __expf(a[0] - mx) + __expf(a[1] - mx) + __expf(a[2] - mx) + __expf(a[3] - mx);
    } else {
      for (int i = c; i < V; ++i) s += __expf(x[i] - mx);
    }
  }
  s = block_sum256_serial(s, red);
  if (tid == 0) {
    const float l = mx + __logf(s);
    lse[row] = l;
    const int64_t lab = labels[row];
    loss[row] = (lab >= 0 && lab < V) ? l - x[lab] : 0.f;
  }
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, long ld, int V, const int64_t* __restrict__ labels,
                                                     const float* __restrict__ lse, const float* __restrict__ scale,
                                                     int per_row_scale, bf16* __restrict__ dlogits, long ldd) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)row * ld;
  bf16* d = dlogits + (long)row * ldd;
  const int64_t lab = labels[row];
  const bool valid = lab >= 0 && lab < V;
  const float l = lse[row], sc = per_row_scale ? scale[row] : scale[0];
  for (int c = tid * 8; c < ldd; c += 2048) {
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int col = c + i;
      float g = 0.f;
      if (valid && col < V) g = (__expf(x[col] - l) - (col == lab ? 1.f : 0.f)) * sc;
      o[i] = f2bf(g);
    }
    if (c + 8 <= ldd) *reinterpret_cast<bf16x8*>(d + c) = o;
    else
      for (int i = 0; c + i < ldd; ++i) d[c + i] = o[i];
  }
}

// Cross-entropy against a target row that is not one-hot (the device batch mix of mixup.hip produces such rows): the ImageNet fine-tune
// step (Imagenet.py:468-469 mixup_fn(samples, targets); :592-609 Mixup / SoftTargetCrossEntropy / LabelSmoothingCrossEntropy) and label
// smoothing in the causal LM heads (xbert.py:1190-1229 LabelSmoothSoftmaxCEV1, :1346-1347).  One family of loss,
//   loss_r = -sum_c t_c * log_softmax(x)_c = lse_r * sum_c t_c - sum_c t_c x_c,     dlogits = (softmax * sum_c t_c - t) * scale,
// in two forms: the LABEL form describes the row (two labels, a mixing weight, an on and an off value) and never materialises it; the
// DENSE form reads an fp32 target.  fp32 logits [R, ld] with V live columns as in xfm_ce_fwd; the forward reads every row ONCE (online
// max / sum-exp next to the running sums), one workgroup per row, 16-byte loads with a scalar tail.  Plain vector loads and stores, no
// atomics.

// running (max, sum exp(x - max)) of one lane, merged across the workgroup at the end
struct OnlineLse {
  float m = -3.0e38f, s = 0.f;
  __device__ __forceinline__ void add4(const f32x4 a) {
    const float cm = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3]));
    if (cm > m) { s *= __expf(m - cm); m = cm; }
    s += (__expf(a[0] - m) + __expf(a[1] - m)) + (__expf(a[2] - m) + __expf(a[3] - m));
  }
  __device__ __forceinline__ void add1(const float a) {
    if (a > m) { s *= __expf(m - a); m = a; }
    s += __expf(a - m);
  }
  // The row's log-sum-exp from the 256 lanes' pairs, in every lane, through red: LDS, one row of STRIDE floats per wave.  STRIDE = 4: two
  // more per-lane sums ride along, x2 and x3; the four waves' sums of them are left in red[.][2] and red[.][3] for the caller to add
  // up -- four values, one barrier.  Earlier readers of red must be done.
  template <int STRIDE>
  __device__ __forceinline__ float block_lse(float (*red)[STRIDE], float x2 = 0.f, float x3 = 0.f) const {
    const int w = threadIdx.x >> 6;
    const float wm = wave_max(m);
    const float ws = wave_sum(s * __expf(m - wm));
    if constexpr (STRIDE == 4) { x2 = wave_sum(x2); x3 = wave_sum(x3); }
    if ((threadIdx.x & 63) == 0) {
      red[w][0] = wm; red[w][1] = ws;
      if constexpr (STRIDE == 4) { red[w][2] = x2; red[w][3] = x3; }
    }
    __syncthreads();
    const float bm = fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0]));
    float bs = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)   // each product is rounded before it is added, in every kernel that merges (left to itself the compiler fuses in some)
      bs += red[i][1] * __expf(red[i][0] - bm);
    }
    return bm + __logf(bs);
  }
};

// the row described by the label form: t_c = off + (on - off) * (lam [c == a] + (1 - lam) [c == b]); ignored (a outside [0, V), e.g.
// -100; or b outside it) = no loss and no gradient
struct SmoothRow {
  int a, b;
  float wa, wb, off, tsum;
  bool valid;
  __device__ __forceinline__ float t(int c) const { return off + (c == a ? wa : 0.f) + (c == b ? wb : 0.f); }
};
__device__ __forceinline__ SmoothRow smooth_row(const int64_t* __restrict__ labels_a, const int64_t* __restrict__ labels_b,
                                                const float* __restrict__ lam, float on, float off, int row, int V) {
  SmoothRow r;
  const int64_t a = labels_a[row], b = labels_b != nullptr ? labels_b[row] : a;
  r.valid = a >= 0 && a < V && b >= 0 && b < V;
  r.a = (int)a;
  r.b = (int)b;
  const float l = lam != nullptr ? lam[row] : 1.f;
  r.wa = (on - off) * l;
  r.wb = (on - off) * (1.f - l);
  r.off = off;
  r.tsum = (float)V * off + (on - off);
  return r;
}

// DENSE = false: acc0 = sum x                (label form; `target` unused)
// DENSE = true:  acc0 = sum t, acc1 = sum t x (`row` unused)
template <bool DENSE>
__global__ __launch_bounds__(256) void ce_soft_fwd_kernel(const float* __restrict__ logits, long ld, int V, const float* __restrict__ target,
                                                          long ldt, const int64_t* __restrict__ labels_a, const int64_t* __restrict__ labels_b,
                                                          const float* __restrict__ lam, float on, float off, float* __restrict__ lse,
                                                          float* __restrict__ tsum, float* __restrict__ loss) {
  __shared__ float red[4][4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)row * ld;
  const float* t = DENSE ? target + (long)row * ldt : nullptr;
  OnlineLse o;
  float acc0 = 0.f, acc1 = 0.f;
  auto take = [&](const f32x4 a, int c) {
    o.add4(a);
    if (DENSE) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(t + c);
      acc0 += (b[0] + b[1]) + (b[2] + b[3]);
      acc1 += (b[0] * a[0] + b[1] * a[1]) + (b[2] * a[2] + b[3] * a[3]);
    } else {
      acc0 += (a[0] + a[1]) + (a[2] + a[3]);
    }
  };
  const int Vv = V & ~3;   // columns covered by whole 16-byte granules
  int c = tid * 4;
  for (; c + 3 * 1024 < Vv; c += 4096) {   // four independent loads in flight per lane
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(x + c), a1 = *reinterpret_cast<const f32x4*>(x + c + 1024);
    const f32x4 a2 = *reinterpret_cast<const f32x4*>(x + c + 2048), a3 = *reinterpret_cast<const f32x4*>(x + c + 3072);
    take(a0, c);
    take(a1, c + 1024);
    take(a2, c + 2048);
    take(a3, c + 3072);
  }
  for (; c < Vv; c += 1024) take(*reinterpret_cast<const f32x4*>(x + c), c);
  if (tid < V - Vv) {   // the scalar tail: at most 3 columns
    const float a = x[Vv + tid];
    o.add1(a);
    if (DENSE) { const float b = t[Vv + tid]; acc0 += b; acc1 += b * a; }
    else acc0 += a;
  }
  const float l = o.block_lse(red, acc0, acc1);   // also fills red[i][2], red[i][3] with the four waves' sums of acc0, acc1
  if (tid != 0) return;
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) { s0 += red[i][2]; s1 += red[i][3]; }
  lse[row] = l;
  if (DENSE) {
    tsum[row] = s0;
    loss[row] = l * s0 - s1;
  } else {
    const SmoothRow r = smooth_row(labels_a, labels_b, lam, on, off, row, V);
    // (the two label terms are added only where their weight is non-zero: lam = 1 must not read x_b into the result at all)
    float lab = 0.f;
    if (r.valid) lab = (r.wa != 0.f ? r.wa * x[r.a] : 0.f) + (r.wb != 0.f ? r.wb * x[r.b] : 0.f);
    loss[row] = r.valid ? r.tsum * l - off * s0 - lab : 0.f;
  }
}

template <bool DENSE>
__global__ __launch_bounds__(256) void ce_soft_bwd_kernel(const float* __restrict__ logits, long ld, int V, const float* __restrict__ target,
                                                          long ldt, const int64_t* __restrict__ labels_a, const int64_t* __restrict__ labels_b,
                                                          const float* __restrict__ lam, float on, float off, const float* __restrict__ lse,
                                                          const float* __restrict__ tsum, const float* __restrict__ scale, int per_row_scale,
                                                          bf16* __restrict__ dlogits, long ldd) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long)row * ld;
  const float* t = DENSE ? target + (long)row * ldt : nullptr;
  bf16* d = dlogits + (long)row * ldd;
  SmoothRow r;
  if (!DENSE) r = smooth_row(labels_a, labels_b, lam, on, off, row, V);
  const bool valid = DENSE || r.valid;
  const float l = lse[row], sc = per_row_scale ? scale[row] : scale[0], ts = DENSE ? tsum[row] : r.tsum;
  const bool vec = (ld & 3) == 0 && (!DENSE || (ldt & 3) == 0);   // rows start on 16 bytes
  for (int c = tid * 8; c < ldd; c += 2048) {   // ldd % 8 == 0: whole 16-byte stores
    bf16x8 o;
    if (!valid || c >= V) {
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = f2bf(0.f);
    } else if (vec && c + 8 <= V) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(x + c), a1 = *reinterpret_cast<const f32x4*>(x + c + 4);
      f32x4 b0, b1;
      if (DENSE) { b0 = *reinterpret_cast<const f32x4*>(t + c); b1 = *reinterpret_cast<const f32x4*>(t + c + 4); }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float xv = i < 4 ? a0[i] : a1[i - 4];
        const float tv = DENSE ? (i < 4 ? b0[i] : b1[i - 4]) : r.t(c + i);
        o[i] = f2bf((ts * __expf(xv - l) - tv) * sc);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int col = c + i;
        float g = 0.f;
        if (col < V) g = (ts * __expf(x[col] - l) - (DENSE ? t[col] : r.t(col))) * sc;
        o[i] = f2bf(g);
      }
    }
    *reinterpret_cast<bf16x8*>(d + c) = o;
  }
}

// The evaluation step of the ImageNet loop in one pass (Imagenet.py:495-536 evaluate: CrossEntropyLoss, accuracy(topk=(1, 2)) and two
// .item() per validation batch): per row the log-sum-exp, the loss lse - x[label] and the label's RANK = its position in a stable
// descending sort = #{j: x[j] > x[label]} + #{j < label: x[j] == x[label]}; the label is in the top k iff rank < k.  One workgroup per row,
// online max / sum-exp as above next to the integer count; 16-byte loads when every row starts on 16 bytes (VEC), scalar loads
// otherwise (ld is free here: num_labels of the shipped configs is 2 ... 1000, most of them no multiple of 4).

struct TopkRow {
  float loss;
  int rank;
};
// whole workgroup (256 threads) on one row; the result is valid in thread 0.  A label outside [0, V): loss 0, rank V.
template <bool VEC>
__device__ __forceinline__ TopkRow ce_topk_row(const float* __restrict__ x, int V, int64_t label, float (*red)[2], int* redc) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bool valid = label >= 0 && label < V;
  const int lab = valid ? (int)label : 0;
  const float xl = valid ? x[lab] : 0.f;
  OnlineLse o;
  int ahead = 0;
  auto take1 = [&](const float a, int c) {
    o.add1(a);
    ahead += (a > xl || (a == xl && c < lab)) ? 1 : 0;
  };
  if (VEC) {
    const int Vv = V & ~3;
    for (int c = tid * 4; c < Vv; c += 1024) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(x + c);
      o.add4(a);
#pragma unroll
      for (int i = 0; i < 4; ++i) ahead += (a[i] > xl || (a[i] == xl && c + i < lab)) ? 1 : 0;
    }
    if (tid < V - Vv) take1(x[Vv + tid], Vv + tid);   // the scalar tail: at most 3 columns
  } else {
    for (int c = tid; c < V; c += 256) take1(x[c], c);
  }
  ahead = wave_sum_int(ahead);
  __syncthreads();   // (the previous row's readers of red / redc are done: the serial form calls this in a loop)
  if (lane == 0) redc[w] = ahead;   // (parked behind the barrier of block_lse)
  const float l = o.block_lse(red);
  TopkRow r{0.f, V};
  if (tid == 0 && valid) {
    r.loss = l - xl;
    r.rank = (redc[0] + redc[1]) + (redc[2] + redc[3]);
  }
  return r;
}

template <bool VEC>
__global__ __launch_bounds__(256) void ce_topk_rows_kernel(const float* __restrict__ logits, long ld, int V, const int64_t* __restrict__ labels,
                                                           float* __restrict__ row_loss, int* __restrict__ row_rank) {
  __shared__ float red[4][2];
  __shared__ int redc[4];
  const long row = blockIdx.x;
  const TopkRow r = ce_topk_row<VEC>(logits + row * ld, V, labels[row], red, redc);
  if (threadIdx.x == 0) { row_loss[row] = r.loss; row_rank[row] = r.rank; }
}

// the trailing workgroup: acc[0] += sum_r loss_r, acc[1] += #{rank_r < k1}, acc[2] += #{rank_r < k2}, the rows added one after the other in
// ascending order by ONE thread (256 rows at a time through LDS): no atomics, no tree whose shape depends on R
__global__ __launch_bounds__(256) void ce_topk_acc_kernel(const float* __restrict__ row_loss, const int* __restrict__ row_rank, int R, int k1,
                                                          int k2, float* __restrict__ acc) {
  __shared__ float sl[256];
  __shared__ int sr[256];
  float s = 0.f;
  int c1 = 0, c2 = 0;
  for (int base = 0; base < R; base += 256) {
    const int r = base + threadIdx.x;
    if (r < R) { sl[threadIdx.x] = row_loss[r]; sr[threadIdx.x] = row_rank[r]; }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = R - base < 256 ? R - base : 256;
      for (int i = 0; i < n; ++i) { s += sl[i]; c1 += sr[i] < k1 ? 1 : 0; c2 += sr[i] < k2 ? 1 : 0; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { acc[0] += s; acc[1] += (float)c1; acc[2] += (float)c2; }
}

// row_loss or row_rank NULL: the library owns no scratch memory to park the rows in, so ONE workgroup walks the rows itself, in the same
// order with the same per-row arithmetic (the sums are bit-identical to the two-kernel form); slower, meant for small R
template <bool VEC>
__global__ __launch_bounds__(256) void ce_topk_serial_kernel(const float* __restrict__ logits, long ld, int R, int V,
                                                             const int64_t* __restrict__ labels, int k1, int k2, float* __restrict__ row_loss,
                                                             int* __restrict__ row_rank, float* __restrict__ acc) {
  __shared__ float red[4][2];
  __shared__ int redc[4];
  float s = 0.f;
  int c1 = 0, c2 = 0;
  for (long row = 0; row < R; ++row) {
    const TopkRow r = ce_topk_row<VEC>(logits + row * ld, V, labels[row], red, redc);
    if (threadIdx.x == 0) {
      s += r.loss; c1 += r.rank < k1 ? 1 : 0; c2 += r.rank < k2 ? 1 : 0;
      if (row_loss != nullptr) row_loss[row] = r.loss;
      if (row_rank != nullptr) row_rank[row] = r.rank;
    }
  }
  if (threadIdx.x == 0) { acc[0] += s; acc[1] += (float)c1; acc[2] += (float)c2; }
}

// ---- host side ----
int xfm_ce_fwd_impl(const float* logits, long ld, int R, int V, const int64_t* labels, float* lse, float* loss, hipStream_t st) {
  XFM_REQUIRE(R > 0 && V > 0 && ld >= V && (ld % 4 == 0 || V < 4), "ce_fwd: bad shape R=%d V=%d ld=%ld", R, V, ld);
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(R), dim3(256), 0, st, logits, ld, V, labels, lse, loss);
  return xfm_check_launch("ce_fwd");
}
int xfm_ce_bwd_impl(const float* logits, long ld, int R, int V, const int64_t* labels, const float* lse, const float* scale,
                    int per_row_scale, void* dlogits, long ldd, hipStream_t st) {
  XFM_REQUIRE(R > 0 && V > 0 && ld >= V && ldd >= V && ldd % 8 == 0, "ce_bwd: bad shape R=%d V=%d ld=%ld ldd=%ld", R, V, ld, ldd);
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(R), dim3(256), 0, st, logits, ld, V, labels, lse, scale, per_row_scale, (bf16*)dlogits, ldd);
  return xfm_check_launch("ce_bwd");
}

// what the soft-target kernels ask of a [R, ld] fp32 operand with V live columns: their 16-byte loads (none when V < 4) need rows_aligned16
static inline bool soft_rows_ok(const void* p, long ld, int V) { return ld >= V && (V < 4 || rows_aligned16(p, ld)); }

int xfm_ce_smooth_fwd_impl(const float* logits, long ld, int R, int V, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                           float on, float off, float* lse, float* loss, hipStream_t st) {
  XFM_REQUIRE(R > 0 && V > 0 && soft_rows_ok(logits, ld, V), "ce_smooth_fwd: bad shape R=%d V=%d ld=%ld (ld %% 4 == 0 and 16-byte aligned logits unless V < 4)", R, V, ld);
  hipLaunchKernelGGL(ce_soft_fwd_kernel<false>, dim3(R), dim3(256), 0, st, logits, ld, V, (const float*)nullptr, 0L, labels_a, labels_b, lam, on,
                     off, lse, (float*)nullptr, loss);
  return xfm_check_launch("ce_smooth_fwd");
}
int xfm_ce_smooth_bwd_impl(const float* logits, long ld, int R, int V, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                           float on, float off, const float* lse, const float* scale, int per_row_scale, void* dlogits, long ldd,
                           hipStream_t st) {
  XFM_REQUIRE(R > 0 && V > 0 && soft_rows_ok(logits, ld, V) && ldd >= V && ldd % 8 == 0 && aligned16(dlogits),
              "ce_smooth_bwd: bad shape R=%d V=%d ld=%ld ldd=%ld (ldd %% 8 == 0, 16-byte aligned dlogits)", R, V, ld, ldd);
  hipLaunchKernelGGL(ce_soft_bwd_kernel<false>, dim3(R), dim3(256), 0, st, logits, ld, V, (const float*)nullptr, 0L, labels_a, labels_b, lam, on,
                     off, lse, (const float*)nullptr, scale, per_row_scale, (bf16*)dlogits, ldd);
  return xfm_check_launch("ce_smooth_bwd");
}
int xfm_ce_soft_fwd_impl(const float* logits, long ld, const float* target, long ldt, int R, int V, float* lse, float* tsum, float* loss,
                         hipStream_t st) {
  XFM_REQUIRE(R > 0 && V > 0 && soft_rows_ok(logits, ld, V) && soft_rows_ok(target, ldt, V),
              "ce_soft_fwd: bad shape R=%d V=%d ld=%ld ldt=%ld (strides %% 4 == 0 and 16-byte aligned operands unless V < 4)", R, V, ld, ldt);
  hipLaunchKernelGGL(ce_soft_fwd_kernel<true>, dim3(R), dim3(256), 0, st, logits, ld, V, target, ldt, (const int64_t*)nullptr,
                     (const int64_t*)nullptr, (const float*)nullptr, 0.f, 0.f, lse, tsum, loss);
  return xfm_check_launch("ce_soft_fwd");
}
int xfm_ce_soft_bwd_impl(const float* logits, long ld, const float* target, long ldt, int R, int V, const float* lse, const float* tsum,
                         const float* scale, int per_row_scale, void* dlogits, long ldd, hipStream_t st) {
  XFM_REQUIRE(R > 0 && V > 0 && soft_rows_ok(logits, ld, V) && soft_rows_ok(target, ldt, V) && ldd >= V && ldd % 8 == 0 && aligned16(dlogits),
              "ce_soft_bwd: bad shape R=%d V=%d ld=%ld ldt=%ld ldd=%ld (ldd %% 8 == 0, 16-byte aligned dlogits)", R, V, ld, ldt, ldd);
  hipLaunchKernelGGL(ce_soft_bwd_kernel<true>, dim3(R), dim3(256), 0, st, logits, ld, V, target, ldt, (const int64_t*)nullptr,
                     (const int64_t*)nullptr, (const float*)nullptr, 0.f, 0.f, lse, tsum, scale, per_row_scale, (bf16*)dlogits, ldd);
  return xfm_check_launch("ce_soft_bwd");
}

int xfm_ce_topk_eval_impl(const float* logits, long ld, int R, int V, const int64_t* labels, int k1, int k2, float* row_loss, int* row_rank,
                          float* acc, hipStream_t st) {
  XFM_REQUIRE(R >= 1 && k1 >= 1 && k2 >= k1 && k2 <= V && ld >= V, "ce_topk_eval: bad arguments R=%d V=%d ld=%ld k1=%d k2=%d (need R >= 1, 1 <= k1 <= k2 <= V <= ld)",
              R, V, ld, k1, k2);
  const bool vec = rows_aligned16(logits, ld);
  if (row_loss == nullptr || row_rank == nullptr) {
    if (vec) hipLaunchKernelGGL(ce_topk_serial_kernel<true>, dim3(1), dim3(256), 0, st, logits, ld, R, V, labels, k1, k2, row_loss, row_rank, acc);
    else hipLaunchKernelGGL(ce_topk_serial_kernel<false>, dim3(1), dim3(256), 0, st, logits, ld, R, V, labels, k1, k2, row_loss, row_rank, acc);
    return xfm_check_launch("ce_topk_eval");
  }
  if (vec) hipLaunchKernelGGL(ce_topk_rows_kernel<true>, dim3(R), dim3(256), 0, st, logits, ld, V, labels, row_loss, row_rank);
  else hipLaunchKernelGGL(ce_topk_rows_kernel<false>, dim3(R), dim3(256), 0, st, logits, ld, V, labels, row_loss, row_rank);
  int rc = xfm_check_launch("ce_topk_eval");
  if (rc != XFM_OK) return rc;
  hipLaunchKernelGGL(ce_topk_acc_kernel, dim3(1), dim3(256), 0, st, row_loss, row_rank, R, k1, k2, acc);
  return xfm_check_launch("ce_topk_eval_acc");
}
