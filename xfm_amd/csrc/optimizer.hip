// The optimizer step on the flat arena: AdamW (two update rules) and the deterministic sum of squares behind the gradient-norm clip.
#include "common.h"

// Flat-arena AdamW (optim.py:4-50 parameter groups; transformers AdamW: correct_bias=True, decoupled decay) with the
// global-norm clip factor folded in (apex_ddp_accelerator.py:100-110).  Per-element group id selects lr / decay.
typedef xfm_adamw_args AdamArgs;
// TORCH = false: the transformers rule above (eps before the bias correction, decay after the update).
// TORCH = true: torch.optim.AdamW's single-tensor rule (Imagenet.py:569-570 builds that optimizer): decay first, eps after sqrt(v) is
// divided by sqrt(bc2).  Same traffic, same launch shape; only the arithmetic of the element differs.
template <bool TORCH>
__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a) {
  const float cc = a.clip_coef ? a.clip_coef[0] : 1.f;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < a.n; i += (long)gridDim.x * 1024) {
    const int gid = a.group[i >> 8];
    const float lr = a.lr[gid], wd = a.wd[gid];
    f32x4 p = *reinterpret_cast<f32x4*>(a.p + i);
    const f32x4 g = *reinterpret_cast<const f32x4*>(a.g + i);
    f32x4 m = *reinterpret_cast<f32x4*>(a.m + i), v = *reinterpret_cast<f32x4*>(a.v + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gj = g[j] * cc;
      if constexpr (TORCH) {
        p[j] *= 1.f - lr * wd;
        m[j] = a.beta1 * m[j] + (1.f - a.beta1) * gj;
        v[j] = a.beta2 * v[j] + (1.f - a.beta2) * gj * gj;
        p[j] -= (lr / a.bc1) * m[j] / (sqrtf(v[j]) / sqrtf(a.bc2) + a.eps);
      } else {
        m[j] = a.beta1 * m[j] + (1.f - a.beta1) * gj;
        v[j] = a.beta2 * v[j] + (1.f - a.beta2) * gj * gj;
        const float step = lr * sqrtf(a.bc2) / a.bc1;
        p[j] -= step * m[j] / (sqrtf(v[j]) + a.eps);
        p[j] -= lr * wd * p[j];
      }
    }
    *reinterpret_cast<f32x4*>(a.p + i) = p;
    *reinterpret_cast<f32x4*>(a.m + i) = m;
    *reinterpret_cast<f32x4*>(a.v + i) = v;
    if (a.zero_grad) *reinterpret_cast<f32x4*>(a.g + i) = f32x4{0.f, 0.f, 0.f, 0.f};  // zero_grad() in the same sweep (Pretrain.py:76)
  }
}

// out[0] += sum of squares of an fp32 vector, DETERMINISTIC: block partials in a fixed grid, then one workgroup adds them in a
// fixed order.  The gradient norm feeds the clip coefficient of the optimizer, i.e. it is evaluated after the all-reduce on
// every data-parallel rank: an atomic accumulation (rank-dependent rounding) makes the replicas' weights drift apart by an ulp
// per step, which nothing ever re-synchronises.
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ x, long n, float* __restrict__ partial) {
  __shared__ float red[4];
  float s = 0.f;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long)gridDim.x * 1024) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + i);
    s += a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3];
  }
  s = block_sum256(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* __restrict__ partial, int nparts, float* __restrict__ out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) s += partial[i];
  s = block_sum256(s, red);
  if (threadIdx.x == 0) out[0] += s;
}

// ---- host side ----
int xfm_adamw_impl(const AdamArgs& a, bool torch_rule, hipStream_t st) {
  XFM_REQUIRE(a.n > 0 && a.n % 256 == 0, "adamw: arena length %ld must be a positive multiple of 256", a.n);
  int grid = cdiv(a.n, 1024);
  if (grid > 4096) grid = 4096;
  if (torch_rule) hipLaunchKernelGGL(adamw_kernel<true>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(adamw_kernel<false>, dim3(grid), dim3(256), 0, st, a);
  return xfm_check_launch(torch_rule ? "adamw_torch" : "adamw");
}

int xfm_sumsq_impl(const float* x, long n, float* out, float* workspace, hipStream_t st) {
  XFM_REQUIRE(n > 0 && n % 4 == 0, "sumsq: length %ld must be a positive multiple of 4", n);
  int grid = cdiv(n, 1024);
  if (grid > XFM_SUMSQ_WORKSPACE_FLOATS) grid = XFM_SUMSQ_WORKSPACE_FLOATS;
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(grid), dim3(256), 0, st, x, n, workspace);
  int rc = xfm_check_launch("sumsq");
  if (rc != XFM_OK) return rc;
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, st, workspace, grid, out);
  return xfm_check_launch("sumsq_final");
}
