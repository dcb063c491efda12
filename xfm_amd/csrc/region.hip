// Device glue of the region pre-training step (Pretrain.py:94-121 run_region_iter): the vision tower's per-sample region output
// (beit2.py:467-475) and the paired L1 + GIoU box loss (xfm.py:815-840).  Plain vector loads and stores, no atomics: every sum below
// runs in one fixed order, so the results are bit-reproducible with or without XFM_DETERMINISTIC.
#include "common.h"

// ---------------------------------------------------------------------------------------------
// Region pooling.  full bf16 [n_img, 1 + P, D] (the tower's normalised output), idx int32 [bs], atts bytes [bs, P] (the patch columns
// of image_atts).  out[s, 1 + p, :] = full[idx[s], 1 + p, :] bit for bit; out[s, 0, :] = sum_p atts[s, p] full[idx[s], 1 + p, :] /
// sum_p atts[s, p] (fp32 sums, one rounding).  One workgroup per (sample, 512 columns): lane = 8 columns, wave w takes the patch rows
// w, w + 4, ...; every gathered row is read once and no fp32 copy of it is made.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void region_pool_fwd_kernel(const bf16* __restrict__ full, const int* __restrict__ idx,
                                                              const uint8_t* __restrict__ atts, int P, int D, bf16* __restrict__ out,
                                                              float* __restrict__ wsum) {
  __shared__ float part[4][64][8];
  __shared__ float cnt[4];
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = (blockIdx.x * 64 + lane) * 8;
  const bool live = c < D;
  const long row = (long)(1 + P) * D;
  const bf16* src = full + (long)idx[s] * row + D + c;
  bf16* dst = out + (long)s * row + D + c;
  const uint8_t* a = atts + (long)s * P;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float n = 0.f;
  for (int p = w; p < P; p += 4) {
    const float wt = (float)a[p];   // wave-uniform
    n += wt;
    if (!live) continue;
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + (long)p * D);
    *reinterpret_cast<bf16x8*>(dst + (long)p * D) = v;
    if (wt != 0.f) {
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(wt, bf2f(v[i]), acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) part[w][lane][i] = acc[i];
  if (lane == 0) cnt[w] = n;
  __syncthreads();
  if (w != 0) return;
  const float total = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
  if (blockIdx.x == 0 && lane == 0) wsum[s] = total;
  if (!live) return;
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = f2bf(((part[0][lane][i] + part[1][lane][i]) + (part[2][lane][i] + part[3][lane][i])) / total);
  *reinterpret_cast<bf16x8*>(out + (long)s * row + c) = o;
}

// dfull[i, 1 + p, :] = sum over the samples s with idx[s] == i, in ascending s, of dout[s, 1 + p, :] + atts[s, p] / wsum[s] * dout[s, 0, :]
// (fp32 sums, one rounding); dfull[i, 0, :] = 0; an image that no sample reads gets zeros.  One thread per (image, row, 8 columns) walks
// the sample list in order: the image test is block-uniform.
__global__ __launch_bounds__(256) void region_pool_bwd_kernel(const bf16* __restrict__ dout, const int* __restrict__ idx,
                                                              const uint8_t* __restrict__ atts, const float* __restrict__ wsum, int bs,
                                                              int P, int D, bf16* __restrict__ dfull) {
  const int img = blockIdx.y, cv = D >> 3;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int r = t / cv, c = (t - r * cv) * 8;
  if (r > P) return;
  const long row = (long)(1 + P) * D;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (r > 0) {
    for (int s = 0; s < bs; ++s) {
      if (idx[s] != img) continue;
      const bf16* d = dout + (long)s * row;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(d + (long)r * D + c);
      const float wt = (float)atts[(long)s * P + (r - 1)];
      if (wt != 0.f) {
        const float k = wt / wsum[s];
        const bf16x8 v0 = *reinterpret_cast<const bf16x8*>(d + c);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += fmaf(k, bf2f(v0[i]), bf2f(v[i]));
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += bf2f(v[i]);
      }
    }
  }
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = f2bf(acc[i]);
  *reinterpret_cast<bf16x8*>(dfull + (long)img * row + (long)r * D + c) = o;
}

int xfm_region_pool_fwd_impl(const void* full, const int* idx, const uint8_t* atts, int n_img, int bs, int P, int D, void* out, float* wsum,
                             hipStream_t st) {
  XFM_REQUIRE(n_img > 0 && bs > 0 && bs <= 65535 && P > 0 && D > 0 && D % 8 == 0, "region_pool_fwd: bad shape n_img=%d bs=%d P=%d D=%d",
              n_img, bs, P, D);
  hipLaunchKernelGGL(region_pool_fwd_kernel, dim3(cdiv(D, 512), bs), dim3(256), 0, st, (const bf16*)full, idx, atts, P, D, (bf16*)out, wsum);
  return xfm_check_launch("region_pool_fwd");
}

int xfm_region_pool_bwd_impl(const void* dout, const int* idx, const uint8_t* atts, const float* wsum, int n_img, int bs, int P, int D,
                             void* dfull, hipStream_t st) {
  XFM_REQUIRE(n_img > 0 && n_img <= 65535 && bs > 0 && P > 0 && D > 0 && D % 8 == 0, "region_pool_bwd: bad shape n_img=%d bs=%d P=%d D=%d",
              n_img, bs, P, D);
  hipLaunchKernelGGL(region_pool_bwd_kernel, dim3(cdiv((long)(1 + P) * (D / 8), 256), n_img), dim3(256), 0, st, (const bf16*)dout, idx, atts,
                     wsum, bs, P, D, (bf16*)dfull);
  return xfm_check_launch("region_pool_bwd");
}

// ---------------------------------------------------------------------------------------------
// Box loss.  coord / target fp32 [bs, 4] as (cx, cy, w, h); is_image fp32 [bs] or NULL (row weight 1 - is_image).
//   out[0] = sum_r w_r sum_j |coord - target| / num,   out[1] = sum_r w_r (1 - giou(xyxy coord_r, xyxy target_r)) / num,
//   num = sum_r w_r (bs without is_image).  If ANY box of either set has x2 < x1 or y2 < y1 the GIoU term of the whole batch is 0 and
//   carries no gradient (xfm.py:824-827).
// One workgroup; thread t takes rows t, t + 256, ...; the block sums are a fixed tree.  The row arithmetic and the sums run in fp64
// (a few hundred rows: nothing to pay on the latency-bound tail of the step) and are rounded to fp32 once, so the result does not
// depend on a summation order at fp32 precision.  state fp64 [bs, 8]: d out[0] / d coord[r, :] and d out[1] / d coord[r, :].
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double d_max_first(double a, double b) { return a > b ? 1.0 : (a == b ? 0.5 : 0.0); }   // d max(a, b) / d a
__device__ __forceinline__ double d_min_first(double a, double b) { return a < b ? 1.0 : (a == b ? 0.5 : 0.0); }

__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void box_loss_fwd_kernel(const float* __restrict__ coord, const float* __restrict__ target,
                                                           const float* __restrict__ is_image, int bs, float* __restrict__ out,
                                                           double* __restrict__ state) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double l1 = 0.0, gl = 0.0, num = 0.0, bad = 0.0;
  for (int r = tid; r < bs; r += 256) {
    const f32x4 cf = *reinterpret_cast<const f32x4*>(coord + 4L * r), tf = *reinterpret_cast<const f32x4*>(target + 4L * r);
    const double wr = is_image != nullptr ? 1.0 - (double)is_image[r] : 1.0;
    double* sr = state + 8L * r;
    double row_l1 = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double d = (double)cf[j] - (double)tf[j];
      row_l1 += fabs(d);
      sr[j] = wr * (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0));
    }
    // xyxy (box_ops.py:9-13)
    const double a[4] = {cf[0] - 0.5 * cf[2], cf[1] - 0.5 * cf[3], cf[0] + 0.5 * cf[2], cf[1] + 0.5 * cf[3]};
    const double b[4] = {tf[0] - 0.5 * tf[2], tf[1] - 0.5 * tf[3], tf[0] + 0.5 * tf[2], tf[1] + 0.5 * tf[3]};
    if (a[2] < a[0] || a[3] < a[1] || b[2] < b[0] || b[3] < b[1]) bad = 1.0;
    // paired IoU / GIoU (box_ops.py:24-59) and d giou / d a
    double lt[2], rb[2], e0[2], e1[2], iw[2], ew[2], sa[2], sb[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      lt[k] = fmax(a[k], b[k]);
      rb[k] = fmin(a[2 + k], b[2 + k]);
      e0[k] = fmin(a[k], b[k]);
      e1[k] = fmax(a[2 + k], b[2 + k]);
      iw[k] = rb[k] - lt[k];
      ew[k] = e1[k] - e0[k];
      sa[k] = a[2 + k] - a[k];
      sb[k] = b[2 + k] - b[k];
    }
    const double ci[2] = {iw[0] >= 0.0 ? 1.0 : 0.0, iw[1] >= 0.0 ? 1.0 : 0.0}, ce[2] = {ew[0] >= 0.0 ? 1.0 : 0.0, ew[1] >= 0.0 ? 1.0 : 0.0};
    const double iwc[2] = {fmax(iw[0], 0.0), fmax(iw[1], 0.0)}, ewc[2] = {fmax(ew[0], 0.0), fmax(ew[1], 0.0)};
    const double inter = iwc[0] * iwc[1], uni = sa[0] * sa[1] + sb[0] * sb[1] - inter, earea = ewc[0] * ewc[1];
    const double giou = inter / uni - (earea - uni) / earea;
    double dg[4];   // d giou / d (x1, y1, x2, y2) of box a
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int o = 1 - k;
      const double dinter1 = -iwc[o] * ci[k] * d_max_first(a[k], b[k]), dinter2 = iwc[o] * ci[k] * d_min_first(a[2 + k], b[2 + k]);
      const double dun1 = -sa[o] - dinter1, dun2 = sa[o] - dinter2;
      const double de1 = -ewc[o] * ce[k] * d_min_first(a[k], b[k]), de2 = ewc[o] * ce[k] * d_max_first(a[2 + k], b[2 + k]);
      dg[k] = dinter1 / uni - inter * dun1 / (uni * uni) + dun1 / earea - uni * de1 / (earea * earea);
      dg[2 + k] = dinter2 / uni - inter * dun2 / (uni * uni) + dun2 / earea - uni * de2 / (earea * earea);
    }
    // loss = 1 - giou; back to (cx, cy, w, h)
    sr[4] = -wr * (dg[0] + dg[2]);
    sr[5] = -wr * (dg[1] + dg[3]);
    sr[6] = -wr * 0.5 * (dg[2] - dg[0]);
    sr[7] = -wr * 0.5 * (dg[3] - dg[1]);
    l1 += wr * row_l1;
    gl += wr * (1.0 - giou);
    num += wr;
  }
  l1 = block_sum(l1, red);
  num = block_sum(num, red);
  bad = block_sum(bad, red);
  gl = block_sum(gl, red);   // (not finite where a degenerate box made a row 0 / 0: selected away below, never multiplied)
  const bool degenerate = bad != 0.0;
  if (tid == 0) {
    out[0] = (float)(l1 / num);
    out[1] = degenerate ? 0.f : (float)(gl / num);
  }
  for (int r = tid; r < bs; r += 256) {   // the rows this thread wrote above
    double* sr = state + 8L * r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sr[j] = sr[j] / num;
      sr[4 + j] = degenerate ? 0.0 : sr[4 + j] / num;
    }
  }
}

// dcoord[r, :] = g[0] d out[0] / d coord[r, :] + g[1] d out[1] / d coord[r, :]   (g: the two upstream scalars, on the device)
__global__ __launch_bounds__(256) void box_loss_bwd_kernel(const double* __restrict__ state, const float* __restrict__ g, int bs,
                                                           float* __restrict__ dcoord) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= bs * 4) return;
  const int r = t >> 2, j = t & 3;
  dcoord[t] = (float)((double)g[0] * state[8L * r + j] + (double)g[1] * state[8L * r + 4 + j]);
}

int xfm_box_loss_fwd_impl(const float* coord, const float* target, const float* is_image, int bs, float* out, double* state, hipStream_t st) {
  XFM_REQUIRE(bs > 0 && bs <= (1 << 20), "box_loss_fwd: bad batch size %d", bs);
  XFM_REQUIRE(((uintptr_t)coord % 16) == 0 && ((uintptr_t)target % 16) == 0 && ((uintptr_t)state % 8) == 0,
              "box_loss_fwd: coord / target must be 16-byte aligned, state 8-byte aligned");
  hipLaunchKernelGGL(box_loss_fwd_kernel, dim3(1), dim3(256), 0, st, coord, target, is_image, bs, out, state);
  return xfm_check_launch("box_loss_fwd");
}

int xfm_box_loss_bwd_impl(const double* state, const float* g, int bs, float* dcoord, hipStream_t st) {
  XFM_REQUIRE(bs > 0 && bs <= (1 << 20), "box_loss_bwd: bad batch size %d", bs);
  hipLaunchKernelGGL(box_loss_bwd_kernel, dim3(cdiv(4L * bs, 256)), dim3(256), 0, st, state, g, bs, dcoord);
  return xfm_check_launch("box_loss_bwd");
}
