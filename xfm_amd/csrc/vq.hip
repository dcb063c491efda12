// Nearest-code assignment of the VQ-KD tokenizer (models/norm_ema_quantizer.py:149-162): l2-normalise each patch feature, score it
// against the WHOLE codebook, take the argmin --
//   zn = z[r] / max(||z[r]||, 1e-12),   index[r] = argmin_c (|code[c]|^2 - 2 zn . code[c])      (|zn|^2 is the same for every c: dropped)
// -- in ONE launch.  The [M, n_code] score matrix of the reference lives only in accumulator registers.
//
// One workgroup of four waves owns 64 rows.  Their normalised features stay in LDS for the whole kernel, transposed ([k][row]) so that
// the A operand of v_mfma_f32_32x32x2_f32 (lane l: row l & 31, k = l >> 5) is one conflict-free ds_read_b32; the codebook streams through
// LDS in chunks of 128 codes, transposed the same way ([k][code], the B operand: k = l >> 5, code l & 31), the next chunk's rows already
// on their way from global memory into registers while the MFMAs of this one run.  Wave w owns codes 32 w .. + 31 of a chunk against both
// 32-row halves: its lane holds one code column, 2 x 16 rows of it in the accumulators, and a running (best, argbest) for each of those 32
// rows.  A lane meets its codes in ascending order and replaces on strict <, so it keeps the lowest index among equal scores; the
// lanes of a row are then merged by (score, index) lexicographically, which keeps that rule across lanes and waves.
//
// Every score is the same arithmetic wherever its code sits: the dot product is the MFMA's k-ordered fmaf chain from 0 (exact fp32), |e|^2
// a k-ordered fmaf chain from 0, the score fmaf(-2, dot, |e|^2).  Two equal codebook rows therefore score bit-equal against every row, and
// the lower index wins.  No floating-point atomics, no workspace; the histogram is integer atomics, whose sum has no order.
#include "common.h"

constexpr int VQ_THREADS = 256;
constexpr int VQ_ROWS = 64;            // rows of z per workgroup
constexpr int VQ_CHUNK = 128;          // codes per staging chunk (32 per wave)
constexpr int VQ_ZLD = VQ_ROWS + 32;   // floats per k-row of the feature image: lane halves (k, k + 1) fall on disjoint banks
constexpr int VQ_CLD = VQ_CHUNK + 32;  // the same for the code image
constexpr int VQ_MAX_K = 64;
constexpr int VQ_PRE = VQ_CHUNK * (VQ_MAX_K / 4) / VQ_THREADS;   // 16-byte pieces of a chunk per lane, at most (8)
constexpr int VQ_RED = 4 * VQ_ROWS * 8;                          // the four waves' (score, index) per row
constexpr int VQ_MAX_LDS = VQ_MAX_K * (VQ_ZLD + VQ_CLD) * 4 + VQ_RED;

typedef __attribute__((ext_vector_type(16))) float f32x16;

// piece u of a lane: code tid & 127 of the chunk, components 4 kg .. + 3 with kg = (tid >> 7) + 2 u
__device__ __forceinline__ void vq_fetch(f32x4 (&pre)[VQ_PRE], const float* code, long code_ld, int n_code, int c0, int K4, int tid) {
  const int c = c0 + (tid & (VQ_CHUNK - 1));
#pragma unroll
  for (int u = 0; u < VQ_PRE; ++u) {
    const int kg = (tid >> 7) + 2 * u;
    pre[u] = f32x4{0.f, 0.f, 0.f, 0.f};   // (past the last code: zeros; its |e|^2 is set to +inf, it never wins)
    if (kg < K4 && c < n_code) pre[u] = *reinterpret_cast<const f32x4*>(code + (long)c * code_ld + 4 * kg);
  }
}
__device__ __forceinline__ void vq_park(const f32x4 (&pre)[VQ_PRE], float* sC, int K4, int tid) {
  const int c = tid & (VQ_CHUNK - 1);
#pragma unroll
  for (int u = 0; u < VQ_PRE; ++u) {
    const int kg = (tid >> 7) + 2 * u;
    if (kg < K4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) sC[(4 * kg + e) * VQ_CLD + c] = pre[u][e];
    }
  }
}

__global__ __launch_bounds__(VQ_THREADS) void vq_assign_kernel(const float* __restrict__ z, long z_ld, int M, int K, const float* __restrict__ code,
                                                               long code_ld, int n_code, int64_t* __restrict__ index, int* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) char vq_lds[];
  float* sZ = reinterpret_cast<float*>(vq_lds);          // [K][VQ_ZLD]
  float* sC = sZ + K * VQ_ZLD;                            // [K][VQ_CLD]
  float* red_v = sC + K * VQ_CLD;                         // [4][64]
  int* red_i = reinterpret_cast<int*>(red_v + 4 * VQ_ROWS);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
  const long row0 = (long)blockIdx.x * VQ_ROWS;
  const int K4 = K >> 2;

  f32x4 pre[VQ_PRE];
  vq_fetch(pre, code, code_ld, n_code, 0, K4, tid);

  {   // the 64 rows, normalised: four lanes per row, lane q of them holds the 16-byte pieces q, q + 4, q + 8, q + 12
    const int r = tid >> 2, q = tid & 3;
    const bool live = row0 + r < M;
    const float* zp = z + (row0 + (live ? r : 0)) * z_ld;
    f32x4 v[4];
    float ss = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int kg = q + 4 * g;
      v[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (live && kg < K4) v[g] = *reinterpret_cast<const f32x4*>(zp + 4 * kg);
#pragma unroll
      for (int e = 0; e < 4; ++e) ss = fmaf(v[g][e], v[g][e], ss);
    }
    ss += __shfl_xor(ss, 1, 64);
    ss += __shfl_xor(ss, 2, 64);
    const float den = fmaxf(sqrtf(ss), 1e-12f);   // F.normalize: x / norm.clamp_min(eps)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int kg = q + 4 * g;
      if (kg < K4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sZ[(4 * kg + e) * VQ_ZLD + r] = v[g][e] / den;
      }
    }
  }
  vq_park(pre, sC, K4, tid);
  __syncthreads();

  float best[32];
  int arg[32];
#pragma unroll
  for (int r = 0; r < 32; ++r) {
    best[r] = __builtin_inff();   // a row whose every score is NaN or +inf keeps code 0: in range
    arg[r] = 0;
  }

  const int n_chunks = (n_code + VQ_CHUNK - 1) / VQ_CHUNK;
  for (int ch = 0; ch < n_chunks; ++ch) {
    const bool more = ch + 1 < n_chunks;
    if (more) vq_fetch(pre, code, code_ld, n_code, (ch + 1) * VQ_CHUNK, K4, tid);
    const int cl = 32 * w + j, c = ch * VQ_CHUNK + cl;
    float e2 = 0.f;
    for (int k = 0; k < K; ++k) {
      const float e = sC[k * VQ_CLD + cl];
      e2 = fmaf(e, e, e2);
    }
    if (c >= n_code) e2 = __builtin_inff();
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
    // (reading step s + 2's operands by hand ahead of step s's MFMAs measured SLOWER, 0.205 against 0.173 ms at 12544 x 8192 x 32: the
    // plain loop is what the compiler schedules best)
    for (int s = 0; s < K; s += 2) {
      const float b = sC[(s + h) * VQ_CLD + cl];
      const float a0 = sZ[(s + h) * VQ_ZLD + j], a1 = sZ[(s + h) * VQ_ZLD + 32 + j];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float s0 = fmaf(-2.f, acc0[r], e2), s1 = fmaf(-2.f, acc1[r], e2);
      if (s0 < best[r]) {
        best[r] = s0;
        arg[r] = c;
      }
      if (s1 < best[16 + r]) {
        best[16 + r] = s1;
        arg[16 + r] = c;
      }
    }
    if (more) {
      __syncthreads();   // every wave has read this chunk
      vq_park(pre, sC, K4, tid);
      __syncthreads();
    }
  }

  // accumulator register r of half a: row 32 a + (r & 3) + 8 (r >> 2) + 4 h, this lane's code column; the 32 lanes of a half merge
#pragma unroll
  for (int r = 0; r < 32; ++r) {
    float v = best[r];
    int i = arg[r];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) argmin_merge(v, i, __shfl_xor(v, o, 64), __shfl_xor(i, o, 64));
    if (j == 0) {
      const int row = 32 * (r >> 4) + (r & 3) + 8 * ((r & 15) >> 2) + 4 * h;
      red_v[w * VQ_ROWS + row] = v;
      red_i[w * VQ_ROWS + row] = i;
    }
  }
  __syncthreads();
  if (tid < VQ_ROWS && row0 + tid < M) {
    float v = red_v[tid];
    int i = red_i[tid];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) argmin_merge(v, i, red_v[ww * VQ_ROWS + tid], red_i[ww * VQ_ROWS + tid]);
    index[row0 + tid] = (int64_t)i;
    if (counts != nullptr) atomicAdd(counts + i, 1);
  }
}

int xfm_vq_assign_impl(const float* z, long z_ld, int M, int K, const float* code, long code_ld, int n_code, int64_t* index, int* counts,
                       hipStream_t st) {
  XFM_REQUIRE(z != nullptr && code != nullptr && index != nullptr, "vq_assign: null operand");
  XFM_REQUIRE(M >= 1 && n_code >= 1, "vq_assign: M=%d n_code=%d (need >= 1)", M, n_code);
  if (K < 4 || K > VQ_MAX_K || K % 4 != 0) {
    xfm_set_error("vq_assign: K=%d (the kernel takes a multiple of 4 in [4, %d])", K, VQ_MAX_K);
    return XFM_E_UNSUPPORTED;
  }
  XFM_REQUIRE(z_ld >= K && code_ld >= K, "vq_assign: z_ld=%ld code_ld=%ld below K=%d", z_ld, code_ld, K);
  XFM_REQUIRE(rows_aligned16(z, z_ld) && rows_aligned16(code, code_ld),
              "vq_assign: z and code must be 16-byte aligned, their leading dimensions multiples of 4");
  const size_t lds = (size_t)K * (VQ_ZLD + VQ_CLD) * 4 + VQ_RED;
  lds_launch<vq_assign_kernel, VQ_MAX_LDS>(dim3(cdiv(M, VQ_ROWS)), dim3(VQ_THREADS), lds, st, z, z_ld, M, K, code, code_ld, n_code, index, counts);
  return xfm_check_launch("vq_assign");
}
