// The evaluation side of the grounding task (Grounding_bbox.py:73-93 val + dataset/utils.py:271-345 grounding_eval_bbox /
// grounding_eval_bbox_vlue + :349-361 computeIoU): one launch per batch in place of one device round trip and one Python IoU per sample.
// Plain vector loads and stores, no float atomics, no global atomics; the same bits with and without XFM_DETERMINISTIC.
//   box_eval    (cx, cy, w, h) in [0, 1] -> the pixel box and its IoU with the reference box of the sample's row of the ref tables, and
//               the (#IoU >= 0.5, #samples) counts of the three splits added into one int64 [3, 2] buffer -- ONE workgroup owns it
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
