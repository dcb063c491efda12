// Cross-entropy against a target row that is not one-hot, and the device batch mix that produces such rows: the ImageNet fine-tune step
// (Imagenet.py:468-469 mixup_fn(samples, targets); :592-609 Mixup / SoftTargetCrossEntropy / LabelSmoothingCrossEntropy) and label
// smoothing in the causal LM heads (xbert.py:1190-1229 LabelSmoothSoftmaxCEV1, :1346-1347).  One family of loss,
//   loss_r = -sum_c t_c * log_softmax(x)_c = lse_r * sum_c t_c - sum_c t_c x_c,     dlogits = (softmax * sum_c t_c - t) * scale,
// in two forms: the LABEL form describes the row (two labels, a mixing weight, an on and an off value) and never materialises it; the
// DENSE form reads an fp32 target.  fp32 logits [R, ld] with V live columns as in xfm_ce_fwd; the forward reads every row ONCE (online
// max / sum-exp next to the running sums), one workgroup per row, 16-byte loads with a scalar tail.  Plain vector loads and stores, no
// atomics.
#include "common.h"

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
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
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
  const float wm = wave_max(o.m);
  const float ws = wave_sum(o.s * __expf(o.m - wm));
  acc0 = wave_sum(acc0);
  acc1 = wave_sum(acc1);
  if (lane == 0) { red[w][0] = wm; red[w][1] = ws; red[w][2] = acc0; red[w][3] = acc1; }
  __syncthreads();
  if (tid != 0) return;
  const float m = fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0]));
  float s = 0.f, s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) { s += red[i][1] * __expf(red[i][0] - m); s0 += red[i][2]; s1 += red[i][3]; }
  const float l = m + __logf(s);
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

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// what the row kernels ask of a [R, ld] fp32 operand with V live columns: 16-byte loads need rows that start on 16 bytes
#define XFM_SOFT_ROWS_OK(p, ld, V) ((ld) >= (V) && ((V) < 4 || (((ld) & 3) == 0 && aligned16(p))))

int xfm_ce_smooth_fwd_impl(const float* logits, long ld, int R, int V, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                           float on, float off, float* lse, float* loss, hipStream_t st) {
  XFM_REQUIRE(R > 0 && V > 0 && XFM_SOFT_ROWS_OK(logits, ld, V), "ce_smooth_fwd: bad shape R=%d V=%d ld=%ld (ld %% 4 == 0 and 16-byte aligned logits unless V < 4)", R, V, ld);
  hipLaunchKernelGGL(ce_soft_fwd_kernel<false>, dim3(R), dim3(256), 0, st, logits, ld, V, (const float*)nullptr, 0L, labels_a, labels_b, lam, on,
                     off, lse, (float*)nullptr, loss);
  return xfm_check_launch("ce_smooth_fwd");
}
int xfm_ce_smooth_bwd_impl(const float* logits, long ld, int R, int V, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                           float on, float off, const float* lse, const float* scale, int per_row_scale, void* dlogits, long ldd,
                           hipStream_t st) {
  XFM_REQUIRE(R > 0 && V > 0 && XFM_SOFT_ROWS_OK(logits, ld, V) && ldd >= V && ldd % 8 == 0 && aligned16(dlogits),
              "ce_smooth_bwd: bad shape R=%d V=%d ld=%ld ldd=%ld (ldd %% 8 == 0, 16-byte aligned dlogits)", R, V, ld, ldd);
  hipLaunchKernelGGL(ce_soft_bwd_kernel<false>, dim3(R), dim3(256), 0, st, logits, ld, V, (const float*)nullptr, 0L, labels_a, labels_b, lam, on,
                     off, lse, (const float*)nullptr, scale, per_row_scale, (bf16*)dlogits, ldd);
  return xfm_check_launch("ce_smooth_bwd");
}
int xfm_ce_soft_fwd_impl(const float* logits, long ld, const float* target, long ldt, int R, int V, float* lse, float* tsum, float* loss,
                         hipStream_t st) {
  XFM_REQUIRE(R > 0 && V > 0 && XFM_SOFT_ROWS_OK(logits, ld, V) && XFM_SOFT_ROWS_OK(target, ldt, V),
              "ce_soft_fwd: bad shape R=%d V=%d ld=%ld ldt=%ld (strides %% 4 == 0 and 16-byte aligned operands unless V < 4)", R, V, ld, ldt);
  hipLaunchKernelGGL(ce_soft_fwd_kernel<true>, dim3(R), dim3(256), 0, st, logits, ld, V, target, ldt, (const int64_t*)nullptr,
                     (const int64_t*)nullptr, (const float*)nullptr, 0.f, 0.f, lse, tsum, loss);
  return xfm_check_launch("ce_soft_fwd");
}
int xfm_ce_soft_bwd_impl(const float* logits, long ld, const float* target, long ldt, int R, int V, const float* lse, const float* tsum,
                         const float* scale, int per_row_scale, void* dlogits, long ldd, hipStream_t st) {
  XFM_REQUIRE(R > 0 && V > 0 && XFM_SOFT_ROWS_OK(logits, ld, V) && XFM_SOFT_ROWS_OK(target, ldt, V) && ldd >= V && ldd % 8 == 0 && aligned16(dlogits),
              "ce_soft_bwd: bad shape R=%d V=%d ld=%ld ldt=%ld ldd=%ld (ldd %% 8 == 0, 16-byte aligned dlogits)", R, V, ld, ldt, ldd);
  hipLaunchKernelGGL(ce_soft_bwd_kernel<true>, dim3(R), dim3(256), 0, st, logits, ld, V, target, ldt, (const int64_t*)nullptr,
                     (const int64_t*)nullptr, (const float*)nullptr, 0.f, 0.f, lse, tsum, scale, per_row_scale, (bf16*)dlogits, ldd);
  return xfm_check_launch("ce_soft_bwd");
}

// ---------------------------------------------------------------------------------------------
// The evaluation step of the ImageNet loop in one pass (Imagenet.py:495-536 evaluate: CrossEntropyLoss, accuracy(topk=(1, 2)) and two
// .item() per validation batch): per row the log-sum-exp, the loss lse - x[label] and the label's RANK = its position in a stable
// descending sort = #{j: x[j] > x[label]} + #{j < label: x[j] == x[label]}; the label is in the top k iff rank < k.  One workgroup per row,
// online max / sum-exp as above next to the integer count; 16-byte loads when every row starts on 16 bytes (VEC), scalar loads
// otherwise (ld is free here: num_labels of the shipped configs is 2 ... 1000, most of them no multiple of 4).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

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
  const float wm = wave_max(o.m);
  const float ws = wave_sum(o.s * __expf(o.m - wm));
  ahead = wave_sum_int(ahead);
  __syncthreads();   // (the previous row's readers of red / redc are done: the serial form calls this in a loop)
  if (lane == 0) { red[w][0] = wm; red[w][1] = ws; redc[w] = ahead; }
  __syncthreads();
  TopkRow r{0.f, V};
  if (tid == 0 && valid) {
    const float m = fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0]));
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += red[i][1] * __expf(red[i][0] - m);
    r.loss = (m + __logf(s)) - xl;
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

int xfm_ce_topk_eval_impl(const float* logits, long ld, int R, int V, const int64_t* labels, int k1, int k2, float* row_loss, int* row_rank,
                          float* acc, hipStream_t st) {
  XFM_REQUIRE(R >= 1 && k1 >= 1 && k2 >= k1 && k2 <= V && ld >= V, "ce_topk_eval: bad arguments R=%d V=%d ld=%ld k1=%d k2=%d (need R >= 1, 1 <= k1 <= k2 <= V <= ld)",
              R, V, ld, k1, k2);
  const bool vec = (ld & 3) == 0 && aligned16(logits);   // every row starts on 16 bytes
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

// ---------------------------------------------------------------------------------------------
// timm Mixup._mix_batch / _mix_elem in place (Imagenet.py:468-469): row i against the ORIGINAL row j = B - 1 - i.  blockIdx.y = the pair
// (i, j), i < B / 2; one lane owns VEC consecutive elements of both rows, loads both originals and writes both results, so no second
// buffer is needed.  Per row: lam == 1 leaves it alone (timm skips it too); an empty box mixes, x_i <- lam_i x_i + (1 - lam_i) x_j; a
// non-empty box copies its pixels from x_j bit for bit and leaves the rest.
// ---------------------------------------------------------------------------------------------
struct MixRow {
  float lam;
  int yl, yh, xl, xh;
  bool active, cut;
  __device__ __forceinline__ bool inside(int y, int x) const { return y >= yl && y < yh && x >= xl && x < xh; }
};
__device__ __forceinline__ MixRow mix_row(const float* __restrict__ lam, const int* __restrict__ box, int i) {
  MixRow r;
  r.lam = lam[i];
  r.yl = box[4 * i]; r.yh = box[4 * i + 1]; r.xl = box[4 * i + 2]; r.xh = box[4 * i + 3];
  r.cut = r.yh > r.yl && r.xh > r.xl;
  r.active = r.lam != 1.f;
  return r;
}

template <int VEC>   // 4: 16-byte loads and stores (N % 4 == 0, aligned base); 1: any shape
__global__ __launch_bounds__(256) void mixup_kernel(float* __restrict__ x, int B, long N, int H, int W, const float* __restrict__ lam,
                                                    const int* __restrict__ box) {
  const int i = blockIdx.y, j = B - 1 - i;
  const MixRow ri = mix_row(lam, box, i), rj = mix_row(lam, box, j);
  if (!ri.active && !rj.active) return;
  const long e = ((long)blockIdx.x * 256 + threadIdx.x) * VEC;
  if (e >= N) return;   // (N % VEC == 0)
  float* pi = x + (long)i * N + e;
  float* pj = x + (long)j * N + e;
  float a[VEC], b[VEC];
  if constexpr (VEC == 4) {
    const f32x4 va = *reinterpret_cast<const f32x4*>(pi), vb = *reinterpret_cast<const f32x4*>(pj);
#pragma unroll
    for (int k = 0; k < 4; ++k) { a[k] = va[k]; b[k] = vb[k]; }
  } else {
    a[0] = pi[0];
    b[0] = pj[0];
  }
  const long line = e / W;
  int px = (int)(e - line * W), py = (int)(line % H);
  bool ta = ri.active && !ri.cut, tb = rj.active && !rj.cut;   // does the lane's store change anything?
  float oa[VEC], ob[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    oa[k] = a[k];
    ob[k] = b[k];
    if (ri.active) {
      if (!ri.cut) oa[k] = ri.lam * a[k] + (1.f - ri.lam) * b[k];
      else if (ri.inside(py, px)) { oa[k] = b[k]; ta = true; }
    }
    if (rj.active) {
      if (!rj.cut) ob[k] = rj.lam * b[k] + (1.f - rj.lam) * a[k];
      else if (rj.inside(py, px)) { ob[k] = a[k]; tb = true; }
    }
    if (++px == W) { px = 0; if (++py == H) py = 0; }
  }
  if constexpr (VEC == 4) {
    if (ta) *reinterpret_cast<f32x4*>(pi) = f32x4{oa[0], oa[1], oa[2], oa[3]};
    if (tb) *reinterpret_cast<f32x4*>(pj) = f32x4{ob[0], ob[1], ob[2], ob[3]};
  } else {
    if (ta) pi[0] = oa[0];
    if (tb) pj[0] = ob[0];
  }
}

int xfm_mixup_impl(float* x, int B, int C, int H, int W, const float* lam, const int* box, hipStream_t st) {
  XFM_REQUIRE(B > 0 && B % 2 == 0 && C > 0 && H > 0 && W > 0, "mixup: need an even batch and a positive image shape (got B=%d C=%d H=%d W=%d)", B, C, H, W);
  XFM_REQUIRE(B / 2 <= 65535, "mixup: batch %d too large", B);
  const long N = (long)C * H * W;
  if (N % 4 == 0 && aligned16(x)) hipLaunchKernelGGL(mixup_kernel<4>, dim3(cdiv(N / 4, 256), B / 2), dim3(256), 0, st, x, B, N, H, W, lam, box);
  else hipLaunchKernelGGL(mixup_kernel<1>, dim3(cdiv(N, 256), B / 2), dim3(256), 0, st, x, B, N, H, W, lam, box);
  return xfm_check_launch("mixup");
}

// timm mixup_target (Imagenet.py:468-469 through Mixup.__call__): out[i, c] = lam_i onehot_s(y_i)_c + (1 - lam_i) onehot_s(y_{B-1-i})_c with
// off = s / num_classes, on = 1 - s + off; columns [num_classes, ldo) are zeroed (the dense CE never reads them)
__global__ __launch_bounds__(256) void mixup_target_kernel(const int64_t* __restrict__ labels, const float* __restrict__ lam, int B, int nc,
                                                           float on, float off, float* __restrict__ out, long ldo) {
  const int i = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ldo) return;
  const int64_t ya = labels[i], yb = labels[B - 1 - i];
  const float l = lam[i];
  out[(long)i * ldo + c] = c < nc ? l * (c == ya ? on : off) + (1.f - l) * (c == yb ? on : off) : 0.f;
}

int xfm_mixup_target_impl(const int64_t* labels, const float* lam, int B, int num_classes, float smoothing, float* out, long ldo,
                          hipStream_t st) {
  XFM_REQUIRE(B > 0 && B <= 65535 && num_classes > 0 && ldo >= num_classes, "mixup_target: bad shape B=%d num_classes=%d ldo=%ld", B, num_classes, ldo);
  XFM_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "mixup_target: smoothing %f outside [0, 1)", (double)smoothing);
  const float off = smoothing / (float)num_classes, on = 1.f - smoothing + off;
  hipLaunchKernelGGL(mixup_target_kernel, dim3(cdiv(ldo, 256), B), dim3(256), 0, st, labels, lam, B, num_classes, on, off, out, ldo);
  return xfm_check_launch("mixup_target");
}
