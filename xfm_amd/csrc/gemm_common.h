// bf16 MFMA GEMMs for the XFM hot path (gfx950).
//
//   gemm_nt : C[M,N] = A[M,K] . B[N,K]^T (+bias, +GELU ...)   forward Linear (B = W) and dgrad (B = W^T copy)
//   gemm_tn : dW[N,K] += dY[M,N]^T . X[M,K]                     wgrad, split over M, fp32 atomics into the grad arena
//
// Covers every Linear on the path: beit2.py:131 (qkv), :162 (proj), :64-68 (fc1/fc2), :229 (patch-embed conv as
// GEMM); xroberta.py:211,224-234 (query/key/value), :301 (attention output), :368 (intermediate), :382 (output),
// :1326,1331 (LM head); xfm.py:117-120 (itm_head), :617-620 (vision_proj/text_proj).
//
// Tiling is for 64-wide wavefronts: 256 threads = 2x2 waves, v_mfma_f32_16x16x32_bf16.  The NT kernel computes
// C^T tiles (A-operand = weight rows, B-operand = activation rows) so that after the K loop every lane owns 8
// CONSECUTIVE output columns of one output row: bias/GELU are applied in registers and the row is stored 16 B per lane.
//
// This header: what more than one kernel family uses.  The families: gemm_nt_small.hip (small tiles, the 256 x 128 ring),
// gemm_nt_256.hip (256 x 256 phase pipeline), gemm_tn_small.hip (128 x 128 wgrad), gemm_tn_256.hip (256 x 256 wgrad, single and grouped),
// gemm_cast.hip (operand copies); gemm.hip is the host side and includes them all.
#pragma once
#include "common.h"

enum { EPI_BF16 = 0, EPI_F32 = 1, EPI_GELU = 2, EPI_DGELU = 3, EPI_F32_ACC = 4 };

// raw workgroup barrier fenced for the compiler only: direct-to-LDS loads stay in flight across it (no vmcnt(0) drain)
#define XFM_FENCE() asm volatile("" ::: "memory")
#define XFM_BAR()                    \
  do {                               \
    XFM_FENCE();                     \
    __builtin_amdgcn_s_barrier();    \
    XFM_FENCE();                     \
  } while (0)

struct GemmNT {
  const bf16* A; long lda;
  const bf16* B; long ldb;
  void* C; long ldc;
  const float* bias;
  bf16* aux; long ldaux;
  int M, N, K;
  int group_m;  // row-panels per tile group (L2 locality of the block order)
  int k_splits; // small-tile kernels, EPI_F32_ACC only: gridDim.y K-slices, fp32 atomics into C (1 = off)
  long split_stride;  // EPI_F32 with k_splits > 1: K-slice y stores its partial tile to C + y * split_stride (elements), plain stores
#ifdef XFM_DIAG
  long long* dbg;  // 256 x 256 kernel (tools/tile_timeline.py): wave 0 of every workgroup writes 10-ns timestamps
                   // [tile index, start, K loop done, epilogue done] per tile it walks; NULL = no stamps
#endif
};

// LDS swizzles (16-B chunk index XOR) for 128-B tile rows read with ds_read_b128.
// X tile: a 16-lane group reads 16 consecutive rows; W tile: rows {0-3,8-11,16-19,24-27}(+4) (see header comment).
__device__ __forceinline__ int swz_x(int r) { return (r >> 1) & 7; }
__device__ __forceinline__ int swz_w(int r) { return ((r >> 1) & 1) | (((r >> 3) & 3) << 1); }

// Epilogue of one wave's (MT*16) x (NT*16) sub-tile: lane (lg, lr) owns row m_base + mt*16 + lr and the 8 consecutive
// columns n_base + np*32 + 8*lg .. +7 of every (mt, np): bias / GELU in registers, one 16-B store per (mt, np).
// lds_bias (optional): the wave's NT*16 bias values already in LDS (fp32, index = column - n_base), zeros when there is no bias -- for
// the persistent 256 x 256 kernel, whose epilogue runs with the next tile's staging loads in flight: a load issued here has to wait
// for all of them (loads return in order).
template <int MT, int NT, int EPI>
__device__ __forceinline__ void gemm_epilogue(const GemmNT& g, f32x4 (&acc)[MT][NT], int m_base, int n_base, int lr, int lg,
                                              const float* lds_bias = nullptr) {
  const bool vec_c = (g.ldc % 8) == 0;
  // DGELU: all gelu'(x) loads of the sub-tile go out first, so their latency is paid once, not once per (mt, np)
  bf16x8 pre_all[EPI == EPI_DGELU ? NT / 2 : 1][EPI == EPI_DGELU ? MT : 1];
  const bool vec_aux = (g.ldaux % 8) == 0;
  if (EPI == EPI_DGELU && vec_aux) {
#pragma unroll
    for (int np = 0; np < NT / 2; ++np)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int nb = n_base + np * 32 + 8 * lg, m = m_base + mt * 16 + lr;
        const int mc = m < g.M ? m : g.M - 1, nc = nb + 8 <= g.N ? nb : 0;  // clamped: out-of-range lanes are never stored
        pre_all[np][mt] = *reinterpret_cast<const bf16x8*>(g.aux + (long)mc * g.ldaux + nc);
      }
    // every chunk counts as read here: a chunk left pending on the paths that skip its rows would make the compiler drain all
    // memory operations before the persistent kernel's next tile may reuse the register
#pragma unroll
    for (int np = 0; np < NT / 2; ++np)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) asm volatile("" ::"v"(pre_all[np][mt]));
  }
#pragma unroll
  for (int np = 0; np < NT / 2; ++np) {
    const int nb = n_base + np * 32 + 8 * lg;
    float bv[8];
    if (lds_bias != nullptr) {
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(lds_bias + np * 32 + 8 * lg), b1 = *reinterpret_cast<const f32x4*>(lds_bias + np * 32 + 8 * lg + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) { bv[i] = b0[i]; bv[4 + i] = b1[i]; }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) bv[i] = (g.bias != nullptr && nb + i < g.N) ? g.bias[nb + i] : 0.f;
    }
    if (EPI == EPI_F32 && g.k_splits > 1 && blockIdx.y != 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) bv[i] = 0.f;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = m_base + mt * 16 + lr;
      if (m >= g.M || nb >= g.N) continue;
      float v[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] = acc[mt][2 * np][i] + bv[i];
        v[4 + i] = acc[mt][2 * np + 1][i] + bv[4 + i];
      }
      const bool full = (nb + 8 <= g.N) && vec_c;
      if (EPI == EPI_F32 || EPI == EPI_F32_ACC) {
        float* cp = reinterpret_cast<float*>(g.C) + (long)m * g.ldc + nb;
        if (EPI == EPI_F32 && g.k_splits > 1) {  // K-slices leave as separate planes, summed in a fixed order by ksplit_reduce_kernel
          cp += (long)blockIdx.y * g.split_stride;  // (slice 0 carries the bias: bv is zero on the others)
        }
        if (EPI == EPI_F32_ACC && g.k_splits > 1) {  // K-slices meet in C through fp32 atomics; slice 0 carried the bias
          for (int i = 0; i < 8; ++i)
            if (nb + i < g.N) atomicAdd(cp + i, v[i] - (blockIdx.y == 0 ? 0.f : bv[i]));
          continue;
        }
        if (EPI == EPI_F32_ACC) {
          for (int i = 0; i < 8; ++i)
            if (nb + i < g.N) v[i] += cp[i];
        }
        if (full) {
          *reinterpret_cast<f32x4*>(cp) = f32x4{v[0], v[1], v[2], v[3]};
          *reinterpret_cast<f32x4*>(cp + 4) = f32x4{v[4], v[5], v[6], v[7]};
        } else {
          for (int i = 0; i < 8; ++i)
            if (nb + i < g.N) cp[i] = v[i];
        }
      } else {
        bf16* cp = reinterpret_cast<bf16*>(g.C) + (long)m * g.ldc + nb;
        bf16x8 o;
        if (EPI == EPI_GELU) {
          // GELU and its derivative share one erf / exp evaluation, so the forward stores gelu'(x) for the backward (x = the
          // bf16-rounded pre-activation, the value the reference's autocast GELU sees): the dgrad epilogue is then one
          // multiply per element instead of a second erf evaluation that costs as much as a whole K = 768 MFMA loop.
          bf16* ap = g.aux + (long)m * g.ldaux + nb;
          bf16x8 dact;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float x = bf2f(f2bf(v[i]));
            float cdf, pdf;
            gelu_parts(x, cdf, pdf);
            o[i] = f2bf(x * cdf);
            dact[i] = f2bf(fmaf(x, pdf, cdf));
          }
          if (full) *reinterpret_cast<bf16x8*>(ap) = dact;
          else
            for (int i = 0; i < 8; ++i)
              if (nb + i < g.N) ap[i] = dact[i];
        } else if (EPI == EPI_DGELU) {
          const bf16* ap = g.aux + (long)m * g.ldaux + nb;
          if (full && vec_aux) {
            const bf16x8 dact = pre_all[np][mt];
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = f2bf(v[i] * bf2f(dact[i]));
          } else {
            for (int i = 0; i < 8; ++i) o[i] = (nb + i < g.N) ? f2bf(v[i] * bf2f(ap[i])) : f2bf(0.f);
          }
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) o[i] = f2bf(v[i]);
        }
        if (full) *reinterpret_cast<bf16x8*>(cp) = o;
        else
          for (int i = 0; i < 8; ++i)
            if (nb + i < g.N) cp[i] = o[i];
      }
    }
  }
}

// wgrad: dW[N,K] += dY[M,N]^T . X[M,K] (gemm_tn_small.hip, gemm_tn_256.hip)
struct GemmTN {
  const bf16* dY; long ldy;
  const bf16* X; long ldx;
  float* dW; long ldw;
  float* dbias;  // optional: dbias[n] += sum_m dY[m,n] (bias gradient), folded into the k-tile-0 workgroups
  int M, N, K;
  int m_per_split;
  float* ws;  // per-(split, tile) partial tiles in accumulator-register order, summed by the reduce kernels (null: see direct)
  int direct; // no workspace: 1 = single split, every dW element has one owner -> plain read-modify-write; 0 = fp32 atomics
};

__device__ __forceinline__ int swz_t(int r) { return ((r & 3) | (((r >> 3) & 1) << 2)) << 1; }  // XOR on the 16-B chunk idx

// ---- host side ----
// The run-time epilogue of an NT launch as a compile-time constant: f(Epi<E>{}) for the E that epi names.
template <int E>
struct Epi { static constexpr int value = E; };
template <typename F>
static int nt_with_epilogue(int epi, F&& f) {
  switch (epi) {
    case EPI_BF16: f(Epi<EPI_BF16>{}); return XFM_OK;
    case EPI_F32: f(Epi<EPI_F32>{}); return XFM_OK;
    case EPI_GELU: f(Epi<EPI_GELU>{}); return XFM_OK;
    case EPI_DGELU: f(Epi<EPI_DGELU>{}); return XFM_OK;
    case EPI_F32_ACC: f(Epi<EPI_F32_ACC>{}); return XFM_OK;
  }
  xfm_set_error("gemm_nt: bad epilogue %d", epi);
  return XFM_E_ARG;
}
