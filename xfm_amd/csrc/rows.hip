// Row gather / scatter-add on bf16 rows (packed token rows: [CLS] and masked-position gathers, fusion batch assembly).
// One 16-B chunk per thread; index < 0 -> zero row (gather) / skipped (scatter).
#include "common.h"

__global__ __launch_bounds__(256) void rows_gather_kernel(const bf16* __restrict__ src, const int* __restrict__ index, int R, int D,
                                                          bf16* __restrict__ dst) {
  const int cpr = D >> 3;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)R * cpr) return;
  const int r = (int)(t / cpr), c = (int)(t % cpr);
  const int s = index[r];
  u32x4 v = u32x4{0, 0, 0, 0};
  if (s >= 0) v = *reinterpret_cast<const u32x4*>(src + (long)s * D + c * 8);
  *reinterpret_cast<u32x4*>(dst + (long)r * D + c * 8) = v;
}
__global__ __launch_bounds__(256) void rows_scatter_add_kernel(const bf16* __restrict__ src, const int* __restrict__ index, int R, int D,
                                                               float* __restrict__ dst) {
  const int cpr = D >> 3;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)R * cpr) return;
  const int r = (int)(t / cpr), c = (int)(t % cpr);
  const int s = index[r];
  if (s < 0) return;
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + (long)r * D + c * 8);
  float* d = dst + (long)s * D + c * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) atomicAdd(d + i, bf2f(v[i]));
}

// out[key] += the rows of one run of equal sorted keys, in position order: block i owns the run that STARTS at position i (others exit)
__global__ __launch_bounds__(256) void rows_segment_sum_kernel(const float* __restrict__ src, const int64_t* __restrict__ perm,
                                                               const int64_t* __restrict__ key, long R, int D, long skip_key,
                                                               float* __restrict__ out) {
  const long i = blockIdx.x;
  const int64_t k = key[i];
  if (k < 0 || k == skip_key || (i > 0 && key[i - 1] == k)) return;
  for (int c = threadIdx.x * 4; c < D; c += 1024) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (long j = i; j < R && key[j] == k; ++j) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + perm[j] * D + c);
      acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
    }
    f32x4* dst = reinterpret_cast<f32x4*>(out + k * D + c);
    *dst = *dst + acc;
  }
}

// ---- host side ----
int xfm_rows_gather_impl(const bf16* src, const int* index, int R, int D, bf16* dst, hipStream_t st) {
  XFM_REQUIRE(R > 0 && D > 0 && D % 8 == 0, "rows_gather: bad shape R=%d D=%d", R, D);
  hipLaunchKernelGGL(rows_gather_kernel, dim3(cdiv((long)R * (D >> 3), 256)), dim3(256), 0, st, src, index, R, D, dst);
  return xfm_check_launch("rows_gather");
}
int xfm_rows_scatter_add_impl(const bf16* src, const int* index, int R, int D, float* dst, hipStream_t st) {
  XFM_REQUIRE(R > 0 && D > 0 && D % 8 == 0, "rows_scatter_add: bad shape R=%d D=%d", R, D);
  hipLaunchKernelGGL(rows_scatter_add_kernel, dim3(cdiv((long)R * (D >> 3), 256)), dim3(256), 0, st, src, index, R, D, dst);
  return xfm_check_launch("rows_scatter_add");
}

int xfm_rows_segment_sum_impl(const float* src, const int64_t* perm, const int64_t* key, long R, int D, long skip_key, float* out,
                              hipStream_t st) {
  XFM_REQUIRE(R >= 0 && D > 0 && D % 4 == 0, "rows_segment_sum: bad shape R=%ld D=%d", R, D);
  if (R == 0) return XFM_OK;
  hipLaunchKernelGGL(rows_segment_sum_kernel, dim3((unsigned)R), dim3(256), 0, st, src, perm, key, R, D, skip_key, out);
  return xfm_check_launch("rows_segment_sum");
}
