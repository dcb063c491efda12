// The evaluation side of the grounding task (Grounding_bbox.py:73-93 val + dataset/utils.py:271-345 grounding_eval_bbox /
// grounding_eval_bbox_vlue + :349-361 computeIoU): one launch per batch in place of one device round trip and one Python IoU per sample.
// Plain vector loads and stores, no float atomics, no global atomics; the same bits with and without XFM_DETERMINISTIC.
//   box_eval    (cx, cy, w, h) in [0, 1] -> the pixel box and its IoU with the reference box of the sample's row of the ref tables, and
//               the (#IoU >= 0.5, #samples) counts of the three splits added into one int64 [3, 2] buffer -- ONE workgroup owns it
//   cam_box_rank  (Grounding.py's mask evaluation, dataset/utils.py:178-223) a [p, p] map per ref -> the detector box with the largest
//               bicubic-upsampled sum / area^alpha, its IoU with the reference box, and the same per-split counts
#include "common.h"

constexpr int GROUNDING_THREADS = 256;

// computeIoU's arithmetic in fp64, step for step (no contraction: every product and sum is rounded on its own, as numpy's are).
// box: (x, y, w, h) in pixels, px..ph the prediction in pixels.  union <= 0 (the reference would divide by zero): 0.
__device__ __forceinline__ double box_eval_iou(double rx, double ry, double rw, double rh, double px, double py, double pw, double ph) {
#pragma clang fp contract(off)
  const double x1 = fmax(rx, px), y1 = fmax(ry, py);
  const double x2 = fmin(rx + rw - 1.0, px + pw - 1.0), y2 = fmin(ry + rh - 1.0, py + ph - 1.0);
  const double inter = (x1 < x2 && y1 < y2) ? (x2 - x1 + 1.0) * (y2 - y1 + 1.0) : 0.0;
  const double uni = rw * rh + pw * ph - inter;
  return uni <= 0.0 ? 0.0 : inter / uni;
}

// One workgroup strides over the samples.  The counts of the call are collected in LDS as int32 (integer adds: their order cannot change
// the result) and added into counts by the six lanes that own the cells, with plain 64-bit loads and stores.
__global__ __launch_bounds__(GROUNDING_THREADS) void box_eval_kernel(const float* __restrict__ coord, const int* __restrict__ ref_row,
                                                                     const float* __restrict__ ref_box, const float* __restrict__ ref_size,
                                                                     const int* __restrict__ ref_split, int n, int R, float* __restrict__ out,
                                                                     long out_offset, int64_t* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ int cnt[6];
  const int tid = threadIdx.x;
  if (tid < 6) cnt[tid] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += GROUNDING_THREADS) {
    const int r = ref_row != nullptr ? ref_row[i] : i;
    float* o = out != nullptr ? out + (out_offset + i) * 5 : nullptr;
    if (r < 0 || r >= R) {   // no such ref: nothing of the tables is read, the sample is counted nowhere
      if (o != nullptr) {
        const float qnan = __uint_as_float(0x7FC00000u);
        o[0] = o[1] = o[2] = o[3] = o[4] = qnan;
      }
      continue;
    }
    const double W = (double)ref_size[(long)r * 2], H = (double)ref_size[(long)r * 2 + 1];
    const double pw = (double)coord[(long)i * 4 + 2] * W, ph = (double)coord[(long)i * 4 + 3] * H;
    const double px = (double)coord[(long)i * 4] * W - pw / 2.0, py = (double)coord[(long)i * 4 + 1] * H - ph / 2.0;
    const float* b = ref_box + (long)r * 4;
    const double iou = box_eval_iou((double)b[0], (double)b[1], (double)b[2], (double)b[3], px, py, pw, ph);
    if (o != nullptr) {
      o[0] = (float)px;
      o[1] = (float)py;
      o[2] = (float)pw;
      o[3] = (float)ph;
      o[4] = (float)iou;
    }
    const int s = ref_split[r];
    if (s >= 0 && s < 3) {
      atomicAdd(&cnt[s * 2 + 1], 1);   // LDS integer add
      if (iou >= 0.5) atomicAdd(&cnt[s * 2], 1);
    }
  }
  __syncthreads();
  if (tid < 6) {
    const int c = cnt[tid];
    if (c != 0) counts[tid] += (int64_t)c;
  }
}

// ---------------------------------------------------------------------------------------------
// cam_box_rank: the loop body of grounding_eval (dataset/utils.py:183-216) for a batch of refs, one workgroup per ref.
// ---------------------------------------------------------------------------------------------
// The reference upsamples the [p, p] map to the image with F.interpolate(mode='bicubic') and sums it over each detector box.  The bicubic
// filter is separable and the box is a product of two index ranges, so the sum over the box is a^T cam b with a_i = the sum over the box's
// rows y of the weight that output row y gives input row i, b_j the same over its columns: the [height, width] map is never built.
// The tap weights are ATen's (UpSample.h: area_pixel_compute_source_index, guard_index_and_lambda, get_cubic_upsample_coefficients,
// A = -0.75), in fp32, every operation rounded on its own, in its order; a, b and the product are fp64.
constexpr int CAM_RANK_THREADS = 128;
constexpr int CAM_RANK_PASS = CAM_RANK_THREADS / 2;   // detector boxes per pass: one thread per (box, axis)
constexpr int CAM_RANK_ROW = XFM_CAM_MAX_P + 1;        // padded row of the weight sums (fp64)

__device__ __forceinline__ void cubic_taps(int dst, float scale, int in, int (&idx)[4], float (&wt)[4]) {
#pragma clang fp contract(off)
  const float A = -0.75f;
  const float real = scale * ((float)dst + 0.5f) - 0.5f;
  int i0 = (int)floorf(real);
  i0 = i0 < in - 1 ? i0 : in - 1;
  const float t = fminf(fmaxf(real - (float)i0, 0.f), 1.f);
  const float x0 = t + 1.0f, x2 = 1.0f - t, x3 = x2 + 1.0f;
  wt[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
  wt[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  wt[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  wt[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = i0 + j - 1;
    idx[j] = i < 0 ? 0 : (i > in - 1 ? in - 1 : i);
  }
}
// Python's int() of a non-negative coordinate, then the slice's clamp at the border `hi` (anything else -- negative, NaN -- is 0: the host
// rejects such boxes, this only keeps the loops bounded)
__device__ __forceinline__ int slice_bound(double v, int hi) { return v >= (double)hi ? hi : (v > 0.0 ? (int)v : 0); }

__global__ __launch_bounds__(CAM_RANK_THREADS) void cam_box_rank_kernel(const float* __restrict__ cam, int p, const int* __restrict__ img_hw,
                                                                        const double* __restrict__ det, const int* __restrict__ det_start,
                                                                        const double* __restrict__ ref_box, double alpha,
                                                                        double* __restrict__ out, long out_offset) {
#pragma clang fp contract(off)
  __shared__ double wsum[CAM_RANK_THREADS][CAM_RANK_ROW];   // pass-local: row 2 d = a of box d, row 2 d + 1 = b
  __shared__ float scam[XFM_CAM_MAX_P * XFM_CAM_MAX_P];
  __shared__ double score[XFM_CAM_MAX_DETS];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int H = img_hw[i * 2], W = img_hw[i * 2 + 1];
  const int d0 = det_start[i];
  int nd = det_start[i + 1] - d0;
  nd = nd < 0 ? 0 : (nd > XFM_CAM_MAX_DETS ? XFM_CAM_MAX_DETS : nd);   // (the host refuses more; never index past the LDS arrays)
  for (int e = tid; e < p * p; e += CAM_RANK_THREADS) scam[e] = cam[(long)i * p * p + e];
  for (int base = 0; base < nd; base += CAM_RANK_PASS) {
    __syncthreads();   // the previous pass's sums are read (first pass: scam is written)
    const int d = base + (tid >> 1), axis = tid & 1;   // axis 0: rows (y, h, image height), 1: columns
    if (d < nd) {
      const double* bx = det + (long)(d0 + d) * 4;
      const int size = axis == 0 ? H : W;
      const double lo = axis == 0 ? bx[1] : bx[0], ext = axis == 0 ? bx[3] : bx[2];
      const int s0 = slice_bound(lo, size), s1 = slice_bound(lo + ext, size);
      double* row = wsum[tid];
      for (int e = 0; e < p; ++e) row[e] = 0.0;
      const float scale = (float)p / (float)size;
      for (int y = s0; y < s1; ++y) {
        int idx[4];
        float wt[4];
        cubic_taps(y, scale, p, idx, wt);
#pragma unroll
        for (int j = 0; j < 4; ++j) row[idx[j]] += (double)wt[j];
      }
    }
    __syncthreads();
    if (tid < CAM_RANK_PASS && base + tid < nd) {
      const double* a = wsum[2 * tid];
      const double* bv = wsum[2 * tid + 1];
      double sum = 0.0;
      for (int r = 0; r < p; ++r) {
        double u = 0.0;
        for (int c = 0; c < p; ++c) u += (double)scam[r * p + c] * bv[c];
        sum += a[r] * u;
      }
      const double* bx = det + (long)(d0 + base + tid) * 4;
      score[base + tid] = sum / pow(bx[2] * bx[3], alpha);
    }
  }
  __syncthreads();
  if (tid == 0) {   // first strict maximum from 0 (utils.py:194-201), in box order
    double best = 0.0, iou = 0.0;
    int pick = -1;
    for (int d = 0; d < nd; ++d)
      if (score[d] > best) {
        best = score[d];
        pick = d;
      }
    if (pick >= 0) {
      const double* bx = det + (long)(d0 + pick) * 4;
      const double* rb = ref_box + (long)i * 4;
      iou = box_eval_iou(rb[0], rb[1], rb[2], rb[3], bx[0], bx[1], bx[2], bx[3]);
    }
    double* o = out + (out_offset + i) * 3;
    o[0] = (double)pick;
    o[1] = best;
    o[2] = iou;
  }
}

// The counts of the call, by ONE workgroup (as box_eval's): a ref without a chosen box is counted as wrong.
__global__ __launch_bounds__(GROUNDING_THREADS) void cam_box_count_kernel(const double* __restrict__ out, long out_offset,
                                                                          const int* __restrict__ ref_split, int n, int64_t* __restrict__ counts) {
  __shared__ int cnt[6];
  const int tid = threadIdx.x;
  if (tid < 6) cnt[tid] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += GROUNDING_THREADS) {
    const int s = ref_split[i];
    if (s < 0 || s >= 3) continue;
    const double* o = out + (out_offset + i) * 3;
    atomicAdd(&cnt[s * 2 + 1], 1);   // LDS integer add
    if (o[0] >= 0.0 && o[2] >= 0.5) atomicAdd(&cnt[s * 2], 1);
  }
  __syncthreads();
  if (tid < 6) {
    const int c = cnt[tid];
    if (c != 0) counts[tid] += (int64_t)c;
  }
}

int xfm_cam_box_rank_impl(const float* cam, int p, const int* img_hw, const double* det, const int* det_start, int max_dets, const double* ref_box,
                          const int* ref_split, int n, double alpha, double* out, long out_offset, int64_t* counts, hipStream_t st) {
  XFM_REQUIRE(cam != nullptr && img_hw != nullptr && det != nullptr && det_start != nullptr && ref_box != nullptr && ref_split != nullptr &&
                  out != nullptr && counts != nullptr,
              "cam_box_rank: null operand");
  XFM_REQUIRE(n >= 1 && p >= 1 && out_offset >= 0, "cam_box_rank: n=%d p=%d out_offset=%ld (need n, p >= 1, out_offset >= 0)", n, p, out_offset);
  XFM_REQUIRE(alpha == alpha && alpha > -1.0e300 && alpha < 1.0e300, "cam_box_rank: alpha is not finite");
  XFM_REQUIRE(max_dets >= 0, "cam_box_rank: max_dets=%d", max_dets);
  if (p > XFM_CAM_MAX_P || max_dets > XFM_CAM_MAX_DETS) {
    xfm_set_error("cam_box_rank: p=%d max_dets=%d (the LDS layout holds p <= %d, %d boxes per ref)", p, max_dets, XFM_CAM_MAX_P, XFM_CAM_MAX_DETS);
    return XFM_E_UNSUPPORTED;
  }
  hipLaunchKernelGGL(cam_box_rank_kernel, dim3(n), dim3(CAM_RANK_THREADS), 0, st, cam, p, img_hw, det, det_start, ref_box, alpha, out, out_offset);
  hipLaunchKernelGGL(cam_box_count_kernel, dim3(1), dim3(GROUNDING_THREADS), 0, st, out, out_offset, ref_split, n, counts);
  return xfm_check_launch("cam_box_rank");
}

int xfm_box_eval_impl(const float* coord, const int* ref_row, const float* ref_box, const float* ref_size, const int* ref_split, int n, int R,
                      float* out, long out_offset, int64_t* counts, hipStream_t st) {
  XFM_REQUIRE(coord != nullptr && ref_box != nullptr && ref_size != nullptr && ref_split != nullptr && counts != nullptr,
              "box_eval: null operand");
  XFM_REQUIRE(n >= 1 && R >= 1, "box_eval: n=%d R=%d (need n >= 1, R >= 1)", n, R);
  XFM_REQUIRE(out_offset >= 0, "box_eval: negative out offset %ld", out_offset);
  hipLaunchKernelGGL(box_eval_kernel, dim3(1), dim3(GROUNDING_THREADS), 0, st, coord, ref_row, ref_box, ref_size, ref_split, n, R, out,
                     out_offset, counts);
  return xfm_check_launch("box_eval");
}
