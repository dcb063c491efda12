// The evaluation side of the GLUE task (run_glue.py:370-386) and the regression loss of XFMForClassification (model_classification.py:89-93).
// Plain vector loads and stores, no float atomics, no global atomics; every result has the same bits with and without XFM_DETERMINISTIC.
//   cls_eval    outputs.argmax(dim=-1) + metric.add_batch (run_glue.py:380-384): the predictions of a batch behind the previous batch's in
//               one device buffer, and the batch's confusion counts added into one int64 [L, L] buffer -- ONE workgroup owns it
//   corr_rank   pearsonr / spearmanr of the glue metric for stsb: fp64 two-pass Pearson with ordered sums, and the same formula on AVERAGE
//               ranks (scipy.stats.rankdata(method='average')) -- the values are sorted in LDS by answer_rank.hip's bitonic network on
//               64-bit unique keys, built from an image that orders ALL floats: one workgroup
//   mse_fwd/bwd mean((p - t)^2) over a strided fp32 / bf16 prediction column, and its gradient from a device scalar
#include "common.h"

constexpr int METRIC_THREADS = 256;
static_assert(METRIC_THREADS == ANSWER_THREADS, "corr_rank sorts with answer_sort_desc");

// ---------------------------------------------------------------------------------------------------------------- classification
// torch.argmax's rule over one row: the first index of the maximum; a NaN counts as the maximum and the first NaN wins; -0.0 == +0.0
// (the comparison is the float `>`, so a later +0.0 does not displace an earlier -0.0).
__device__ __forceinline__ int metric_argmax(const float* __restrict__ x, int L) {
  float best = x[0];
  int bi = 0;
  for (int j = 1; j < L; ++j) {
    const float v = x[j];
    if (best == best && (v != v || v > best)) {   // (once best is a NaN nothing displaces it)
      best = v;
      bi = j;
    }
  }
  return bi;
}

// One workgroup.  The counts of the call are collected in LDS as int32 (integer adds: their order cannot change the result) and added
// into conf by the lanes that own the cells, with plain 64-bit loads and stores.
__global__ __launch_bounds__(METRIC_THREADS) void cls_eval_kernel(const float* __restrict__ logits, long ld, int B, int L,
                                                                  const int64_t* __restrict__ labels, int64_t* __restrict__ conf,
                                                                  int64_t* __restrict__ pred, long pred_offset) {
  __shared__ int cnt[XFM_METRIC_MAX_L * XFM_METRIC_MAX_L];
  const int tid = threadIdx.x;
  for (int c = tid; c < L * L; c += METRIC_THREADS) cnt[c] = 0;
  __syncthreads();
  for (int r = tid; r < B; r += METRIC_THREADS) {
    const int p = metric_argmax(logits + (long)r * ld, L);
    if (pred != nullptr) pred[pred_offset + r] = (int64_t)p;
    const int64_t t = labels[r];
    if (t >= 0 && t < (int64_t)L) atomicAdd(&cnt[(int)t * L + p], 1);   // LDS integer add
  }
  __syncthreads();
  for (int c = tid; c < L * L; c += METRIC_THREADS) {
    const int n = cnt[c];
    if (n != 0) conf[c] += (int64_t)n;
  }
}

int xfm_cls_eval_impl(const float* logits, long ld, int B, int L, const int64_t* labels, int64_t* conf, int64_t* pred, long pred_offset,
                      hipStream_t st) {
  XFM_REQUIRE(logits != nullptr && labels != nullptr && conf != nullptr, "cls_eval: null operand");
  XFM_REQUIRE(B >= 1, "cls_eval: B=%d (need B >= 1)", B);
  XFM_REQUIRE(L >= 2 && L <= XFM_METRIC_MAX_L, "cls_eval: L=%d outside [2, %d]", L, XFM_METRIC_MAX_L);
  XFM_REQUIRE(ld >= L, "cls_eval: ld=%ld < L=%d", ld, L);
  XFM_REQUIRE(pred_offset >= 0, "cls_eval: negative pred offset %ld", pred_offset);
  hipLaunchKernelGGL(cls_eval_kernel, dim3(1), dim3(METRIC_THREADS), 0, st, logits, ld, B, L, labels, conf, pred, pred_offset);
  return xfm_check_launch("cls_eval");
}

// ---------------------------------------------------------------------------------------------------------------- correlations
// An order-preserving 32-bit image of a float: negative floats with all bits flipped, non-negative ones with the sign bit set; -0.0 is
// +0.0 first, so the two zeros share an image (and a rank).  (answer_key of answer_rank.hip takes the bits as they are: probabilities.)
__device__ __forceinline__ uint32_t corr_image(float v) {
  uint32_t u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Sum over the workgroup in a FIXED order: each lane has added its elements i = tid, tid + 256, ... in ascending i; the 64 lanes of a
// wave through the xor tree; the four wave sums left to right.  red: four doubles of LDS.  Every lane gets the result.
__device__ __forceinline__ double corr_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// Pearson's r of (a_i, b_i), i < N, in fp64, two passes (means, then centred sums); 0 / 0 = NaN for a constant vector, as scipy.
template <typename GetA, typename GetB>
__device__ __forceinline__ double corr_pearson(GetA a, GetB b, int N, double* red) {
  const int tid = threadIdx.x;
  double sa = 0.0, sb = 0.0;
  for (int i = tid; i < N; i += METRIC_THREADS) {
    sa += a(i);
    sb += b(i);
  }
  const double ma = corr_block_sum(sa, red) / (double)N;
  const double mb = corr_block_sum(sb, red) / (double)N;
  double saa = 0.0, sbb = 0.0, sab = 0.0;
  for (int i = tid; i < N; i += METRIC_THREADS) {
    const double da = a(i) - ma, db = b(i) - mb;
    saa += da * da;
    sbb += db * db;
    sab += da * db;
  }
  saa = corr_block_sum(saa, red);
  sbb = corr_block_sum(sbb, red);
  sab = corr_block_sum(sab, red);
  return sab / sqrt(saa * sbb);
}

// Doubled average ranks of v[0 .. N) into r2 (int32 LDS).  The key is (image, position), unique; its COMPLEMENT is sorted descending by
// answer_sort_desc (answer_rank.hip), so sorted position j holds the j-th smallest key, and the padding keys, 0, lie below every
// complemented real key: they sort after all N of them for any N.  A tie is a run of equal high words; the run [s, e) of 0-based sorted
// positions holds the 1-based positions s + 1 .. e, whose mean is (s + 1 + e) / 2.  Both ends by binary search.
__device__ __forceinline__ void corr_ranks2(const float* __restrict__ v, int N, int n_pad, unsigned long long* keys, int* r2) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n_pad; i += METRIC_THREADS)
    keys[i] = i < N ? ~(((unsigned long long)corr_image(v[i]) << 32) | (unsigned long long)(uint32_t)i) : 0ull;
  __syncthreads();
  answer_sort_desc(keys, n_pad);
  for (int j = tid; j < N; j += METRIC_THREADS) {
    const unsigned long long key = ~keys[j];
    // (a real key's high word is at most the image of +inf, 0xFF800000: hi_key does not wrap)
    const unsigned long long lo_key = key & 0xFFFFFFFF00000000ull, hi_key = lo_key + 0x100000000ull;
    int a = 0, b = j;   // s = first position in [0, j] whose key >= lo_key
    while (a < b) {
      const int m = (a + b) >> 1;
      if (~keys[m] >= lo_key) b = m; else a = m + 1;
    }
    const int s = a;
    a = j + 1, b = N;   // e = first position in (j, N] whose key >= hi_key
    while (a < b) {
      const int m = (a + b) >> 1;
      if (~keys[m] >= hi_key) b = m; else a = m + 1;
    }
    r2[(int)(uint32_t)key] = s + 1 + a;
  }
  __syncthreads();
}

// Dynamic LDS: n_pad keys (8 bytes each), two int32 [N_pad4] arrays of doubled ranks, 4 doubles + 1 int of scratch.
__global__ __launch_bounds__(METRIC_THREADS) void corr_rank_kernel(const float* __restrict__ x, const float* __restrict__ y, int N, int n_pad,
                                                                   double* __restrict__ out, float* __restrict__ rank_x,
                                                                   float* __restrict__ rank_y) {
  extern __shared__ __attribute__((aligned(16))) unsigned char corr_lds[];
  const int n4 = (N + 3) & ~3;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(corr_lds);
  int* r2x = reinterpret_cast<int*>(keys + n_pad);
  int* r2y = r2x + n4;
  double* red = reinterpret_cast<double*>(r2y + n4);
  int* flag = reinterpret_cast<int*>(red + 4);
  const int tid = threadIdx.x;
  if (tid == 0) *flag = 0;
  __syncthreads();
  bool nan = false;
  for (int i = tid; i < N; i += METRIC_THREADS) {
    const float a = x[i], b = y[i];
    nan = nan || a != a || b != b;
  }
  if (nan) *flag = 1;   // (every writer stores the same value)
  __syncthreads();
  if (*flag != 0) {     // any NaN: both correlations are NaN, and so are the ranks
    const float qnan = __uint_as_float(0x7FC00000u);
    if (tid == 0) out[0] = out[1] = (double)qnan;
    for (int i = tid; i < N; i += METRIC_THREADS) {
      if (rank_x != nullptr) rank_x[i] = qnan;
      if (rank_y != nullptr) rank_y[i] = qnan;
    }
    return;
  }
  const double pearson = corr_pearson([=](int i) { return (double)x[i]; }, [=](int i) { return (double)y[i]; }, N, red);
  corr_ranks2(x, N, n_pad, keys, r2x);
  corr_ranks2(y, N, n_pad, keys, r2y);
  const double spearman = corr_pearson([=](int i) { return 0.5 * (double)r2x[i]; }, [=](int i) { return 0.5 * (double)r2y[i]; }, N, red);
  if (tid == 0) {
    out[0] = pearson;
    out[1] = spearman;
  }
  for (int i = tid; i < N; i += METRIC_THREADS) {
    if (rank_x != nullptr) rank_x[i] = 0.5f * (float)r2x[i];
    if (rank_y != nullptr) rank_y[i] = 0.5f * (float)r2y[i];
  }
}

static inline int corr_pow2(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

int xfm_corr_rank_impl(const float* x, const float* y, int N, double* out, float* rank_x, float* rank_y, hipStream_t st) {
  XFM_REQUIRE(x != nullptr && y != nullptr && out != nullptr, "corr_rank: null operand");
  XFM_REQUIRE(N >= 2 && N <= XFM_CORR_MAX_N, "corr_rank: N=%d outside [2, %d]", N, XFM_CORR_MAX_N);
  XFM_REQUIRE(((uintptr_t)out & 7) == 0, "corr_rank: out must lie on 8 bytes");
  const int n_pad = corr_pow2(N), n4 = (N + 3) & ~3;
  constexpr int MAX_LDS = XFM_CORR_MAX_N * 16 + 48;   // 64 KiB of keys, 2 x 32 KiB of doubled ranks, the reduction scratch
  lds_launch<corr_rank_kernel, MAX_LDS>(dim3(1), dim3(METRIC_THREADS), (size_t)n_pad * 8 + (size_t)n4 * 8 + 48, st, x, y, N, n_pad, out,
                                        rank_x, rank_y);
  return xfm_check_launch("corr_rank");
}

// ---------------------------------------------------------------------------------------------------------------- regression loss
__device__ __forceinline__ float mse_pred(const void* __restrict__ pred, long stride, int pred_bf16, long i) {
  return pred_bf16 ? bf2f(reinterpret_cast<const bf16*>(pred)[i * stride]) : reinterpret_cast<const float*>(pred)[i * stride];
}

// One workgroup, fp32: lane sums over i = tid, tid + 256, ... in ascending i, the wave xor tree, the four wave sums pairwise; / B.
__global__ __launch_bounds__(METRIC_THREADS) void mse_fwd_kernel(const void* __restrict__ pred, long stride, int pred_bf16,
                                                                 const float* __restrict__ target, int B, float* __restrict__ loss) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < B; i += METRIC_THREADS) {
    const float d = mse_pred(pred, stride, pred_bf16, i) - target[i];
    s = fmaf(d, d, s);
  }
  s = block_sum256(s, red);
  if (threadIdx.x == 0) loss[0] = s / (float)B;
}

__global__ __launch_bounds__(METRIC_THREADS) void mse_bwd_kernel(const void* __restrict__ pred, long stride, int pred_bf16,
                                                                 const float* __restrict__ target, const float* __restrict__ dloss, int B,
                                                                 float* __restrict__ dpred) {
  const int i = blockIdx.x * METRIC_THREADS + threadIdx.x;
  if (i >= B) return;
  const float g = 2.0f * dloss[0];
  dpred[i] = g * (mse_pred(pred, stride, pred_bf16, i) - target[i]) / (float)B;
}

int xfm_mse_fwd_impl(const void* pred, long stride, int pred_bf16, const float* target, int B, float* loss, hipStream_t st) {
  XFM_REQUIRE(pred != nullptr && target != nullptr && loss != nullptr, "mse_fwd: null operand");
  XFM_REQUIRE(B >= 1 && stride >= 1, "mse_fwd: bad shape B=%d stride=%ld (need B >= 1, stride >= 1)", B, stride);
  hipLaunchKernelGGL(mse_fwd_kernel, dim3(1), dim3(METRIC_THREADS), 0, st, pred, stride, pred_bf16, target, B, loss);
  return xfm_check_launch("mse_fwd");
}

int xfm_mse_bwd_impl(const void* pred, long stride, int pred_bf16, const float* target, const float* dloss, int B, float* dpred,
                     hipStream_t st) {
  XFM_REQUIRE(pred != nullptr && target != nullptr && dloss != nullptr && dpred != nullptr, "mse_bwd: null operand");
  XFM_REQUIRE(B >= 1 && stride >= 1, "mse_bwd: bad shape B=%d stride=%ld (need B >= 1, stride >= 1)", B, stride);
  hipLaunchKernelGGL(mse_bwd_kernel, dim3(cdiv(B, METRIC_THREADS)), dim3(METRIC_THREADS), 0, st, pred, stride, pred_bf16, target, dloss, B,
                     dpred);
  return xfm_check_launch("mse_bwd");
}
