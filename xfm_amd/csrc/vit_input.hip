// The ViT's way in and out of its token rows (gfx950): patch gather, token assembly with the MIM mask, and the pooled-cls tail.  HBM-bound,
// 8-16 bytes per lane.
#include "common.h"

// Patch gather: NCHW fp32 image -> bf16 patch matrix [B*gh*gw, C*P*P] with column order (c, ky, kx), i.e. the A
// operand of the patch-embed GEMM against Conv2d.weight.view(D, C*P*P)  (beit2.py:224-230).
// Each thread converts 8 consecutive kx of one (patch, c, ky): a 32-B coalesced read, a 16-B store.
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ img, int B, int C, int Himg, int Wimg, int P,
                                                       bf16* __restrict__ out) {
  const int gh = Himg / P, gw = Wimg / P;
  const int kcols = C * P * P;
  const int per_row = kcols / 8;
  const long total = (long)B * gh * gw * per_row;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int c8 = (int)(t % per_row);
    const long prow = t / per_row;
    const int col = c8 * 8;
    const int c = col / (P * P), ky = (col / P) % P, kx = col % P;
    const int px = (int)(prow % gw), py = (int)((prow / gw) % gh), b = (int)(prow / ((long)gw * gh));
    const float* src = img + (((long)b * C + c) * Himg + py * P + ky) * Wimg + px * P + kx;
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(src), a1 = *reinterpret_cast<const f32x4*>(src + 4);
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[i] = f2bf(a0[i]); o[4 + i] = f2bf(a1[i]); }
    *reinterpret_cast<bf16x8*>(out + prow * kcols + col) = o;
  }
}

// ViT token assembly (beit2.py:432-446): x0[b] = [cls | tok[b mod Bt] with masked patches replaced by mask_token], fp32.
// Bx = reps * Bt output rows read the SAME Bt patch-embedded images (the pre-training step runs the clean and the MIM-masked
// view of an image in one 2B pass: the patch-embed GEMM, its weight gradient and the image gather are done once per image).
// Replaces tok * (1 - w) + mask_token * w, the cls concat and their five autograd kernels.
__global__ __launch_bounds__(256) void vit_tokens_fwd_kernel(const float* __restrict__ tok, const float* __restrict__ cls,
                                                             const float* __restrict__ mask_token, const uint8_t* __restrict__ mask,
                                                             int Bt, int Bx, int P, int D, float* __restrict__ x0) {
  const int d4 = D / 4;
  const long total = (long)Bx * (P + 1) * d4;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int c = (int)(t % d4) * 4;
    const long row = t / d4;
    const int i = (int)(row % (P + 1)), b = (int)(row / (P + 1));
    const float* src;
    if (i == 0) src = cls + c;
    else if (mask != nullptr && mask[(long)b * P + i - 1]) src = mask_token + c;
    else src = tok + ((long)(b % Bt) * P + i - 1) * D + c;
    *reinterpret_cast<f32x4*>(x0 + row * D + c) = *reinterpret_cast<const f32x4*>(src);
  }
}

// dtok[s, i] = sum over the rows b = s (mod Bt) that kept patch i of dx0[b, 1 + i]   (written, not accumulated)
__global__ __launch_bounds__(256) void vit_tokens_bwd_tok_kernel(const float* __restrict__ dx0, const uint8_t* __restrict__ mask, int Bt,
                                                                 int Bx, int P, int D, float* __restrict__ dtok) {
  const int d4 = D / 4;
  const long total = (long)Bt * P * d4;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int c = (int)(t % d4) * 4;
    const long row = t / d4;
    const int i = (int)(row % P), s0 = (int)(row / P);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int b = s0; b < Bx; b += Bt) {
      if (mask != nullptr && mask[(long)b * P + i]) continue;
      const f32x4 v = *reinterpret_cast<const f32x4*>(dx0 + ((long)b * (P + 1) + 1 + i) * D + c);
      acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
    }
    *reinterpret_cast<f32x4*>(dtok + row * D + c) = acc;
  }
}

// dcls += sum_b dx0[b, 0];  dmask_token += sum over masked (b, i) of dx0[b, 1 + i].  One workgroup per (batch row, chunk of the patches),
// thread = 4 columns (D <= 1024), row skips are workgroup-uniform.  The workgroups' sums are PARKED -- part[set][wg][D], the layout of
// the LayerNorm column-sum partials, in the head of dtok, which the token kernel overwrites afterwards -- and folded by reduce_sets in
// workgroup order: the 128 float atomics per element this used to end in moved the last bits of both gradients from run to run (and
// 128 workgroups walking 196 patches each took 103 us at the end of the ViT's backward chain; 4 chunks per row: a quarter of that).
__global__ __launch_bounds__(256) void vit_tokens_bwd_vec_kernel(const float* __restrict__ dx0, const uint8_t* __restrict__ mask, int Bx,
                                                                 int P, int D, int chunks, float* __restrict__ part) {
  const int c = threadIdx.x * 4;
  if (c >= D) return;
  const int np = Bx * chunks, b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const int per = (P + chunks - 1) / chunks, i0 = ch * per, i1 = i0 + per < P ? i0 + per : P;
  const float* base = dx0 + (long)b * (P + 1) * D + c;
  f32x4 ac = {0.f, 0.f, 0.f, 0.f}, am = {0.f, 0.f, 0.f, 0.f};
  if (ch == 0) ac = *reinterpret_cast<const f32x4*>(base);
  if (mask != nullptr) {
    for (int i = i0; i < i1; ++i) {
      if (!mask[(long)b * P + i]) continue;
      const f32x4 u = *reinterpret_cast<const f32x4*>(base + (long)(1 + i) * D);
      am[0] += u[0]; am[1] += u[1]; am[2] += u[2]; am[3] += u[3];
    }
  }
  *reinterpret_cast<f32x4*>(part + ((long)0 * np + blockIdx.x) * D + c) = ac;
  *reinterpret_cast<f32x4*>(part + ((long)1 * np + blockIdx.x) * D + c) = am;
}

// BEiT pooled-cls tail (beit2.py:455-466): y[b, 0, :] <- mean_i y[b, 1 + i, :] in place (bf16 rows, fp32 mean), and its backward
// dy'[b, 0] = 0, dy'[b, 1 + i] = dy[b, 1 + i] + dy[b, 0] / P.  Replaces float() / mean / cast / cat and their autograd kernels.
__global__ __launch_bounds__(256) void pool_rows_fwd_kernel(bf16* __restrict__ y, int N, int D) {
  __shared__ float red[2][1024];
  const int b = blockIdx.x, d8 = D / 8;
  const int cg = threadIdx.x % d8, ph = threadIdx.x / d8;  // column group (8 columns), row phase; blockDim = 2 * d8
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bf16* base = y + (long)b * N * D + cg * 8;
  for (int i = 1 + ph; i < N; i += 2) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(base + (long)i * D);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += bf2f(v[j]);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[ph][cg * 8 + j] = acc[j];
  __syncthreads();
  if (ph == 0) {
    const float inv = 1.0f / (float)(N - 1);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf((red[0][cg * 8 + j] + red[1][cg * 8 + j]) * inv);
    *reinterpret_cast<bf16x8*>(base) = o;
  }
}

__global__ __launch_bounds__(256) void pool_rows_bwd_kernel(const bf16* __restrict__ dy, int B, int N, int D, bf16* __restrict__ out) {
  const int d8 = D / 8;
  const long total = (long)B * N * d8;
  const float inv = 1.0f / (float)(N - 1);
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long r = e / d8;
    const int c = (int)(e % d8) * 8;
    const int n = (int)(r % N);
    bf16x8 o;
    if (n == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2bf(0.f);
    } else {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(dy + r * D + c);
      const bf16x8 g0 = *reinterpret_cast<const bf16x8*>(dy + (r - n) * D + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2bf(fmaf(bf2f(g0[j]), inv, bf2f(v[j])));
    }
    *reinterpret_cast<bf16x8*>(out + r * D + c) = o;
  }
}

// ---- host side ----
int xfm_patchify_impl(const float* img, int B, int C, int H, int W, int P, void* out, hipStream_t st) {
  XFM_REQUIRE(B > 0 && C > 0 && P % 8 == 0 && H % P == 0 && W % P == 0 && W % 4 == 0, "patchify: bad geometry B=%d C=%d H=%d W=%d P=%d", B, C, H, W, P);
  const long total = (long)B * (H / P) * (W / P) * (C * P * P / 8);
  int grid = cdiv(total, 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(patchify_kernel, dim3(grid), dim3(256), 0, st, img, B, C, H, W, P, (bf16*)out);
  return xfm_check_launch("patchify");
}

static int vit_tokens_check(int Bt, int Bx, int P, int D) {
  XFM_REQUIRE(Bt > 0 && Bx >= Bt && Bx % Bt == 0 && P > 0 && D > 0 && D % 4 == 0 && D <= 1024,
              "vit_tokens: bad shape Bt=%d Bx=%d P=%d D=%d (Bx must be a multiple of Bt, D a multiple of 4 and <= 1024)", Bt, Bx, P, D);
  return XFM_OK;
}

int xfm_vit_tokens_fwd_impl(const float* tok, const float* cls, const float* mask_token, const uint8_t* mask, int Bt, int Bx, int P,
                            int D, float* x0, hipStream_t st) {
  int rc = vit_tokens_check(Bt, Bx, P, D);
  if (rc != XFM_OK) return rc;
  const long total = (long)Bx * (P + 1) * (D / 4);
  int grid = cdiv(total, 256);
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(vit_tokens_fwd_kernel, dim3(grid), dim3(256), 0, st, tok, cls, mask_token, mask, Bt, Bx, P, D, x0);
  return xfm_check_launch("vit_tokens_fwd");
}

int xfm_vit_tokens_bwd_impl(const float* dx0, const uint8_t* mask, int Bt, int Bx, int P, int D, float* dtok, float* dcls,
                            float* dmask_token, hipStream_t st) {
  int rc = vit_tokens_check(Bt, Bx, P, D);
  if (rc != XFM_OK) return rc;
  const long total = (long)Bt * P * (D / 4);
  int grid = cdiv(total, 256);
  if (grid > 8192) grid = 8192;
  // the cls / mask-token sums first: their per-workgroup parts borrow the head of dtok (Bt * P * D floats), which the token kernel then
  // writes in full
  int chunks = 4;
  while (chunks > 1 && (long)Bx * chunks * 2 > (long)Bt * P) chunks >>= 1;
  XFM_REQUIRE((long)Bx * chunks * 2 <= (long)Bt * P, "vit_tokens_bwd: dtok too small to lend the scratch");
  hipLaunchKernelGGL(vit_tokens_bwd_vec_kernel, dim3(Bx * chunks), dim3(256), 0, st, dx0, mask, Bx, P, D, chunks, dtok);
  rc = xfm_check_launch("vit_tokens_bwd_vec");
  if (rc != XFM_OK) return rc;
  ReduceSets rs{dtok, {dcls, mask != nullptr ? dmask_token : nullptr, nullptr, nullptr}, Bx * chunks, D};
  rc = launch_reduce_sets(rs, 2, st, "vit_tokens_bwd_fold");
  if (rc != XFM_OK) return rc;
  hipLaunchKernelGGL(vit_tokens_bwd_tok_kernel, dim3(grid), dim3(256), 0, st, dx0, mask, Bt, Bx, P, D, dtok);
  return xfm_check_launch("vit_tokens_bwd");
}

int xfm_pool_rows_fwd_impl(void* y, int B, int N, int D, hipStream_t st) {
  XFM_REQUIRE(B > 0 && N > 1 && D % 8 == 0 && D <= 1024 && D >= 8, "pool_rows: bad shape B=%d N=%d D=%d (D a multiple of 8, <= 1024)", B, N, D);
  hipLaunchKernelGGL(pool_rows_fwd_kernel, dim3(B), dim3(2 * (D / 8)), 0, st, (bf16*)y, N, D);
  return xfm_check_launch("pool_rows_fwd");
}

int xfm_pool_rows_bwd_impl(const void* dy, int B, int N, int D, void* out, hipStream_t st) {
  XFM_REQUIRE(B > 0 && N > 1 && D % 8 == 0, "pool_rows: bad shape B=%d N=%d D=%d", B, N, D);
  int grid = cdiv((long)B * N * (D / 8), 256);
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(pool_rows_bwd_kernel, dim3(grid), dim3(256), 0, st, (const bf16*)dy, B, N, D, (bf16*)out);
  return xfm_check_launch("pool_rows_bwd");
}
