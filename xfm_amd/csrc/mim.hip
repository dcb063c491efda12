// Masked image modelling: the MSE loss between the masked and the clean view's embeddings, and the block-wise mask sampler.
#include "common.h"

// MIM loss (xfm.py:624-635): MSE over the masked patch rows + MSE over the pooled cls row, between the masked view's embeddings x and
// the (detached) clean view's t, both bf16 [B, N, D].  Forward: sums = {sum (x-t)^2 over masked patch rows, the same over cls rows,
// number of masked patches}; backward: dx = g * 2 (x - t) / (count * D) on masked rows, g * 2 (x - t) / (B * D) on cls rows, 0 elsewhere.
// One read of x and t each way instead of eight fp32 elementwise passes.
__global__ __launch_bounds__(256) void mim_loss_fwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ t,
                                                           const uint8_t* __restrict__ mask, int B, int N, int D, float* __restrict__ partial) {
  // block partials (fixed grid, fixed order inside a block) -> mim_loss_final_kernel: bit-reproducible, and no 8192 waves queueing on
  // three atomic addresses (round 3: 110 us for a 38 MB read)
  __shared__ float red[4][3];
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = ((long)gridDim.x * 256) >> 6;
  float sp = 0.f, sc = 0.f, cnt = 0.f;
  for (long r = wave; r < (long)B * N; r += nwaves) {
    const int n = (int)(r % N), b = (int)(r / N);
    const bool cls = n == 0;
    if (!cls && !mask[(long)b * (N - 1) + n - 1]) continue;  // wave-uniform
    float s = 0.f;
    for (int c = lane * 8; c < D; c += 512) {
      const bf16x8 xv = *reinterpret_cast<const bf16x8*>(x + r * D + c);
      const bf16x8 tv = *reinterpret_cast<const bf16x8*>(t + r * D + c);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = bf2f(xv[i]) - bf2f(tv[i]);
        s = fmaf(d, d, s);
      }
    }
    s = wave_sum(s);
    if (cls) sc += s; else { sp += s; cnt += 1.f; }
  }
  if (lane == 0) { red[threadIdx.x >> 6][0] = sp; red[threadIdx.x >> 6][1] = sc; red[threadIdx.x >> 6][2] = cnt; }
  __syncthreads();
  if (threadIdx.x < 3) partial[blockIdx.x * 3 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
__global__ __launch_bounds__(64) void mim_loss_final_kernel(const float* __restrict__ partial, int nparts, float* __restrict__ sums) {
  for (int q = 0; q < 3; ++q) {
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 64) s += partial[i * 3 + q];
    s = wave_sum(s);
    if (threadIdx.x == 0) sums[q] += s;
  }
}

__global__ __launch_bounds__(256) void mim_loss_bwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ t,
                                                           const uint8_t* __restrict__ mask, const float* __restrict__ sums,
                                                           const float* __restrict__ gout, int cls_term, int B, int N, int D,
                                                           bf16* __restrict__ dx) {
  const int d8 = D / 8;
  const long total = (long)B * N * d8;
  const float g = gout[0];
  const float patch_den = fmaxf(sums[2] * (float)D, 1.0f);
  const float kp = 2.0f * g / patch_den, kc = cls_term ? 2.0f * g / ((float)B * (float)D) : 0.f;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long r = e / d8;
    const int c = (int)(e % d8) * 8;
    const int n = (int)(r % N), b = (int)(r / N);
    const float k = n == 0 ? kc : (mask[(long)b * (N - 1) + n - 1] ? kp : 0.f);
    bf16x8 o;
    if (k != 0.f) {
      const bf16x8 xv = *reinterpret_cast<const bf16x8*>(x + r * D + c);
      const bf16x8 tv = *reinterpret_cast<const bf16x8*>(t + r * D + c);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = f2bf(k * (bf2f(xv[i]) - bf2f(tv[i])));
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = f2bf(0.f);
    }
    *reinterpret_cast<bf16x8*>(dx + r * D + c) = o;
  }
}

// Block-wise MIM mask sampler on the device (masking_generator.py:27-105 of the reference: MaskingGenerator.__call__ / _mask).
// The reference draws every image's mask with Python `random` on the host, B times per step (beit2.py:432-439); here one wavefront
// owns one image and runs the same rejection loop with a counter-based generator (every draw is a pure function of (seed, image,
// draw index), so a launch is reproducible): rectangles of area U[min, remaining] and log-uniform aspect in [lo, hi], at most ten
// attempts per block, accepted when they add between 1 and `remaining` new patches; then the uniform top-up to exactly `num`.
// The patch grid lives in registers, lane l holding patches l, l + 64, ... ; counting a rectangle's overlap is a ballot + popcount.
// delta_hist (optional, int32 [H*W + 1]): histogram of the new patches each accepted block added (the distribution pin of the tests).
__device__ __forceinline__ float mim_u01(uint32_t seed_lo, uint32_t seed_hi, uint32_t img, uint32_t& ctr) {
  const uint32_t key = rng_row_key(seed_lo, seed_hi, img);
  const uint32_t r = rng_u32(key, ctr++);
  return (float)(r >> 8) * (1.0f / 16777216.0f);
}

__global__ __launch_bounds__(256) void mim_masks_kernel(int B, int GH, int GW, int num, int min_num, float log_lo, float log_hi,
                                                         uint32_t seed_lo, uint32_t seed_hi, uint8_t* __restrict__ out,
                                                         int* __restrict__ delta_hist) {
  const int lane = threadIdx.x & 63;
  const int img = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (img >= B) return;  // whole waves leave together
  const int P = GH * GW;
  constexpr int MAXW = 16;  // up to 1024 patches (32 x 32 grid)
  bool m[MAXW];
#pragma unroll
  for (int i = 0; i < MAXW; ++i) m[i] = false;
  uint32_t ctr = 0;
  int count = 0;
  while (count < num) {
    const int maxp = num - count;
    int delta = 0;
    for (int attempt = 0; attempt < 10 && delta == 0; ++attempt) {
      const float area = (float)min_num + ((float)maxp - (float)min_num) * mim_u01(seed_lo, seed_hi, img, ctr);
      const float ar = __expf(log_lo + (log_hi - log_lo) * mim_u01(seed_lo, seed_hi, img, ctr));
      const int h = (int)rintf(sqrtf(area * ar)), w = (int)rintf(sqrtf(area / ar));
      // (the two position draws are consumed whether or not the rectangle fits, so the stream stays aligned per attempt)
      const float ut = mim_u01(seed_lo, seed_hi, img, ctr), ul = mim_u01(seed_lo, seed_hi, img, ctr);
      if (!(w < GW && h < GH)) continue;
      int top = (int)(ut * (float)(GH - h + 1)), left = (int)(ul * (float)(GW - w + 1));
      top = top > GH - h ? GH - h : top;
      left = left > GW - w ? GW - w : left;
      int masked = 0;
      bool in[MAXW];
#pragma unroll
      for (int i = 0; i < MAXW; ++i) {
        const int p = i * 64 + lane, y = p / GW, x = p - y * GW;
        in[i] = p < P && y >= top && y < top + h && x >= left && x < left + w;
        masked += __popcll(__ballot(in[i] && m[i]));
      }
      const int fresh = h * w - masked;
      if (fresh > 0 && fresh <= maxp) {
#pragma unroll
        for (int i = 0; i < MAXW; ++i) m[i] = m[i] || in[i];
        delta = fresh;
      }
    }
    if (delta == 0) break;
    count += delta;
    if (delta_hist != nullptr && lane == 0) atomicAdd(delta_hist + delta, 1);
  }
  // top-up: `num - count` of the free patches, uniformly without replacement (np.random.choice(..., replace=False))
  int nfree = P - count;
  while (count < num) {
    int r = (int)(mim_u01(seed_lo, seed_hi, img, ctr) * (float)nfree);
    r = r >= nfree ? nfree - 1 : r;
#pragma unroll
    for (int i = 0; i < MAXW; ++i) {
      const int p = i * 64 + lane;
      const bool fr = p < P && !m[i];
      const unsigned long long bal = __ballot(fr);
      const int before = __popcll(bal & ((1ull << lane) - 1ull));
      const int tot = __popcll(bal);
      if (r >= 0 && r < tot && fr && before == r) m[i] = true;
      r -= tot;  // (negative once the patch was found in an earlier word: no later word matches)
    }
    ++count;
    --nfree;
  }
#pragma unroll
  for (int i = 0; i < MAXW; ++i) {
    const int p = i * 64 + lane;
    if (p < P) out[(long)img * P + p] = m[i] ? 1 : 0;
  }
}

// ---- host side ----
int xfm_mim_loss_fwd_impl(const void* x, const void* t, const uint8_t* mask, int B, int N, int D, float* sums, hipStream_t st) {
  XFM_REQUIRE(B > 0 && N > 1 && D > 0 && D % 8 == 0, "mim_loss: bad shape B=%d N=%d D=%d", B, N, D);
  int grid = cdiv((long)B * N, 4);
  if (grid > XFM_MIM_PARTIALS) grid = XFM_MIM_PARTIALS;
  hipLaunchKernelGGL(mim_loss_fwd_kernel, dim3(grid), dim3(256), 0, st, (const bf16*)x, (const bf16*)t, mask, B, N, D, sums + 3);
  int rc = xfm_check_launch("mim_loss_fwd");
  if (rc != XFM_OK) return rc;
  hipLaunchKernelGGL(mim_loss_final_kernel, dim3(1), dim3(64), 0, st, sums + 3, grid, sums);
  return xfm_check_launch("mim_loss_final");
}

int xfm_mim_loss_bwd_impl(const void* x, const void* t, const uint8_t* mask, const float* sums, const float* gout, int cls_term, int B,
                          int N, int D, void* dx, hipStream_t st) {
  XFM_REQUIRE(B > 0 && N > 1 && D > 0 && D % 8 == 0, "mim_loss: bad shape B=%d N=%d D=%d", B, N, D);
  int grid = cdiv((long)B * N * (D / 8), 256);
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(mim_loss_bwd_kernel, dim3(grid), dim3(256), 0, st, (const bf16*)x, (const bf16*)t, mask, sums, gout, cls_term, B, N, D,
                     (bf16*)dx);
  return xfm_check_launch("mim_loss_bwd");
}

int xfm_mim_masks_impl(int B, int GH, int GW, int num, int min_num, float min_aspect, float max_aspect, uint64_t seed, uint8_t* out,
                       int* delta_hist, hipStream_t st) {
  XFM_REQUIRE(B > 0 && GH > 0 && GW > 0 && GH * GW <= 1024 && num >= 0 && num <= GH * GW && min_num >= 0, "mim_masks: bad geometry");
  XFM_REQUIRE(min_aspect > 0.f && max_aspect >= min_aspect, "mim_masks: bad aspect range");
  hipLaunchKernelGGL(mim_masks_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, B, GH, GW, num, min_num, logf(min_aspect), logf(max_aspect),
                     (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), out, delta_hist);
  return xfm_check_launch("mim_masks");
}
