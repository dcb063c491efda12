// RoBERTa embeddings: y = dropout(LN(word[id] + type[0] + pos[p])), p = cumsum(id != pad) * (id != pad) + pad
// (xroberta.py:104-137, :1747-1757); pos_mode 1 = BERT: p = t, no padding row in the position table (xbert.py:188-215).
// One wave per token.
#include "common.h"

typedef xfm_embed_args EmbArgs;

__device__ __forceinline__ int roberta_pos(const int64_t* ids_row, int t, int pad, int lane) {
  int cnt = 0;
  for (int j0 = 0; j0 <= t; j0 += 64) {
    const int j = j0 + lane;
    const bool nz = (j <= t) && (ids_row[j] != pad);
    cnt += __popcll(__ballot(nz));
  }
  return (ids_row[t] != pad) ? cnt + pad : pad;
}

template <int NCH>
__global__ __launch_bounds__(256) void emb_fwd_kernel(EmbArgs p) {
  constexpr int D = NCH * 256;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  const int rows = p.B * p.T;
  for (int row = wave; row < rows; row += nwaves) {
    const int b = row / p.T, t = row % p.T;
    const int orow = p.row_map != nullptr ? p.row_map[row] : row;  // packed output row (wave-uniform)
    if (orow < 0) continue;
    const uint32_t rkey = rng_row_key(p.seed_lo, p.seed_hi, (uint32_t)row);
    const int64_t* ids_row = p.ids + (long)b * p.T;
    const int pid = p.pos_mode ? t : roberta_pos(ids_row, t, p.pad_id, lane);
    const long wid = ids_row[t];
    if (lane == 0) p.pos_ids[row] = pid;
    float v[NCH][4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int e = (i * 64 + lane) * 4;
      const f32x4 a = *reinterpret_cast<const f32x4*>(p.word + wid * D + e);
      const f32x4 c = *reinterpret_cast<const f32x4*>(p.pos + (long)pid * D + e);
      const f32x4 d = *reinterpret_cast<const f32x4*>(p.type + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[i][j] = a[j] + d[j] + c[j]; s += v[i][j]; }
    }
    const float mu = wave_sum(s) * (1.0f / D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float d = v[i][j] - mu; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) * (1.0f / D) + p.eps);
    if (lane == 0) { p.mean[row] = mu; p.rstd[row] = rstd; }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int e = (i * 64 + lane) * 4;
      const f32x4 wv = *reinterpret_cast<const f32x4*>(p.w + e), bv = *reinterpret_cast<const f32x4*>(p.b + e);
      bf16x4 o;
      f32x4 o32;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float yv = (v[i][j] - mu) * rstd * wv[j] + bv[j];
        if (p.drop_thresh != 0u) {
          yv = rng_keep(rng_u32(rkey, (uint32_t)(e + j)), p.drop_thresh) ? yv * p.drop_scale : 0.f;
        }
        o[j] = f2bf(yv);
        o32[j] = yv;
      }
      *reinterpret_cast<bf16x4*>(p.y + (long)orow * D + e) = o;
      if (p.y32 != nullptr) *reinterpret_cast<f32x4*>(p.y32 + (long)orow * D + e) = o32;
    }
  }
}

template <int NCH>
__global__ __launch_bounds__(256) void emb_bwd_kernel(EmbArgs p) {
  constexpr int D = NCH * 256;
  __shared__ float red[4][D];
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  const int rows = p.B * p.T;
  float acc[3][NCH][4];
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[s][i][j] = 0.f;
  for (int row = wave; row < rows; row += nwaves) {
    const int orow = p.row_map != nullptr ? p.row_map[row] : row;
    if (orow < 0) continue;
    const uint32_t rkey = rng_row_key(p.seed_lo, p.seed_hi, (uint32_t)row);
    const long wid = p.ids[row];
    const int pid = p.pos_ids[row];
    const float mu = p.mean[row], rstd = p.rstd[row];
    float dy[NCH][4], xh[NCH][4], wv[NCH][4];
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int e = (i * 64 + lane) * 4;
      const f32x4 a = *reinterpret_cast<const f32x4*>(p.word + wid * D + e);
      const f32x4 c = *reinterpret_cast<const f32x4*>(p.pos + (long)pid * D + e);
      const f32x4 d = *reinterpret_cast<const f32x4*>(p.type + e);
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(p.w + e);
      const bf16x4 g = *reinterpret_cast<const bf16x4*>(p.dy + (long)orow * D + e);
      f32x4 g32 = {0.f, 0.f, 0.f, 0.f};
      if (p.dy32 != nullptr) g32 = *reinterpret_cast<const f32x4*>(p.dy32 + (long)orow * D + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float gv = bf2f(g[j]) + g32[j];
        if (p.drop_thresh != 0u) {
          gv = rng_keep(rng_u32(rkey, (uint32_t)(e + j)), p.drop_thresh) ? gv * p.drop_scale : 0.f;
        }
        dy[i][j] = gv;
        wv[i][j] = w4[j];
        xh[i][j] = (a[j] + d[j] + c[j] - mu) * rstd;
        const float gw = gv * w4[j];
        c1 += gw;
        c2 += gw * xh[i][j];
        acc[0][i][j] += gv * xh[i][j];
        acc[1][i][j] += gv;
      }
    }
    c1 = wave_sum(c1) * (1.0f / D);
    c2 = wave_sum(c2) * (1.0f / D);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int e = (i * 64 + lane) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dz = rstd * (dy[i][j] * wv[i][j] - c1 - xh[i][j] * c2);
        acc[2][i][j] += dz;
        if (p.dz_out != nullptr) {   // ordered scatter by the caller (xfm_rows_segment_sum)
          p.dz_out[(long)row * D + e + j] = dz;
          continue;
        }
        // nn.Embedding(padding_idx): the pad row receives no gradient (xroberta.py:80,100-102)
        if (wid != p.pad_id) atomicAdd(p.dword + wid * D + e + j, dz);
        if (p.pos_mode || pid != p.pad_id) atomicAdd(p.dpos + (long)pid * D + e + j, dz);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[wib][(i * 64 + lane) * 4 + j] = acc[s][i][j];
    __syncthreads();
    float* dst = p.partial + ((long)s * gridDim.x + blockIdx.x) * D;
    for (int c = threadIdx.x; c < D; c += 256) dst[c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
  }
}

// ---- host side ----
static int emb_grid(int rows) {
  int g = cdiv(rows, 16);
  if (g > 256) g = 256;
  return g < 1 ? 1 : g;
}

int xfm_emb_fwd_impl(const EmbArgs& p, int D, hipStream_t st) {
  XFM_REQUIRE(D == 768 || D == 1024, "embedding: unsupported width %d", D);
  XFM_REQUIRE(p.B > 0 && p.T > 0, "embedding: empty batch");
  int grid = cdiv(p.B * p.T, 4);
  if (grid > 2048) grid = 2048;
  if (D == 768) hipLaunchKernelGGL(emb_fwd_kernel<3>, dim3(grid), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(emb_fwd_kernel<4>, dim3(grid), dim3(256), 0, st, p);
  return xfm_check_launch("emb_fwd");
}

int xfm_emb_bwd_impl(EmbArgs p, int D, float* dgamma, float* dbeta, float* dtype, float* workspace, long workspace_bytes,
                     hipStream_t st) {
  XFM_REQUIRE(D == 768 || D == 1024, "embedding: unsupported width %d", D);
  const int grid = emb_grid(p.B * p.T);
  XFM_REQUIRE(workspace != nullptr && workspace_bytes >= (long)3 * grid * D * 4, "embedding bwd: workspace too small");
  p.partial = workspace;
  if (D == 768) hipLaunchKernelGGL(emb_bwd_kernel<3>, dim3(grid), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(emb_bwd_kernel<4>, dim3(grid), dim3(256), 0, st, p);
  int rc = xfm_check_launch("emb_bwd");
  if (rc != XFM_OK) return rc;
  ReduceSets r{workspace, {dgamma, dbeta, dtype, nullptr}, grid, D};
  hipLaunchKernelGGL(reduce_sets_kernel, dim3(cdiv(D, 64), 3), dim3(256), 0, st, r);
  return xfm_check_launch("emb_bwd_reduce");
}
