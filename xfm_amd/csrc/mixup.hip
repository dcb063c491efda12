// timm Mixup._mix_batch / _mix_elem in place (Imagenet.py:468-469): row i against the ORIGINAL row j = B - 1 - i.  blockIdx.y = the pair
// (i, j), i < B / 2; one lane owns VEC consecutive elements of both rows, loads both originals and writes both results, so no second
// buffer is needed.  Per row: lam == 1 leaves it alone (timm skips it too); an empty box mixes, x_i <- lam_i x_i + (1 - lam_i) x_j; a
// non-empty box copies its pixels from x_j bit for bit and leaves the rest.
#include "common.h"

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

// ---- host side ----
int xfm_mixup_impl(float* x, int B, int C, int H, int W, const float* lam, const int* box, hipStream_t st) {
  XFM_REQUIRE(B > 0 && B % 2 == 0 && C > 0 && H > 0 && W > 0, "mixup: need an even batch and a positive image shape (got B=%d C=%d H=%d W=%d)", B, C, H, W);
  XFM_REQUIRE(B / 2 <= 65535, "mixup: batch %d too large", B);
  const long N = (long)C * H * W;
  if (N % 4 == 0 && aligned16(x)) hipLaunchKernelGGL(mixup_kernel<4>, dim3(cdiv(N / 4, 256), B / 2), dim3(256), 0, st, x, B, N, H, W, lam, box);
  else hipLaunchKernelGGL(mixup_kernel<1>, dim3(cdiv(N, 256), B / 2), dim3(256), 0, st, x, B, N, H, W, lam, box);
  return xfm_check_launch("mixup");
}

int xfm_mixup_target_impl(const int64_t* labels, const float* lam, int B, int num_classes, float smoothing, float* out, long ldo,
                          hipStream_t st) {
  XFM_REQUIRE(B > 0 && B <= 65535 && num_classes > 0 && ldo >= num_classes, "mixup_target: bad shape B=%d num_classes=%d ldo=%ld", B, num_classes, ldo);
  XFM_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "mixup_target: smoothing %f outside [0, 1)", (double)smoothing);
  const float off = smoothing / (float)num_classes, on = 1.f - smoothing + off;
  hipLaunchKernelGGL(mixup_target_kernel, dim3(cdiv(ldo, 256), B), dim3(256), 0, st, labels, lam, B, num_classes, on, off, out, ldo);
  return xfm_check_launch("mixup_target");
}
