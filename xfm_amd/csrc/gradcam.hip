// Grad-CAM of one cross-attention layer (Grounding.py:101-115 on the attention-map contract of xroberta.py:182-194, 268-270): the
// probabilities P = softmax(q k^T scale), the gradient dP = dO v^T that reaches them (no attention dropout, no head mask), and
//   cam[b, j-1] = 1/(H t_div) sum_h sum_{t < q_len[b]} P[b,h,t,j] max(dP[b,h,t,j], 0),  j = 1 .. Sk-1
// in ONE launch, from what the backward of the layer already holds (q, dO, the K | V projection and the forward's log-sum-exp).
//
// One workgroup of four waves owns (batch entry, 64 keys) and walks the heads; wave w owns keys 16 w .. + 15 of the tile.  A key's K and
// V rows are the B operands of that one wave alone, so they go from global memory straight into its fragment registers (an LDS image would
// be written once and read once); Q_h and dO_h, which all four waves read as A operands, are staged in LDS (16 KB).  With the query rows on
// the accumulator registers and the key on the lane (S = Q K^T: row 4 lg + r, column lr), the sum over the query rows is a walk over a
// lane's own registers in a fixed order, carried across the heads in one register, and finished by two lane exchanges: no atomics, no
// workspace, the same bits on every launch.  The two maps are stored from the same registers when asked for.
#include "attention_common.h"

typedef xfm_gradcam_args GradcamArgs;
constexpr int GRADCAM_THREADS = 256;

__global__ __launch_bounds__(GRADCAM_THREADS) void xattn_gradcam_kernel(const GradcamArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[ATTN_SLOT];   // Q_h | dO_h, 64 rows each (rows past the entry's length: zeros)
  const int b = blockIdx.y, kt = blockIdx.x;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4;
  const long qbase = a.q_start != nullptr ? (long)a.q_start[b] : (long)b * a.Sq;
  int sq = a.q_len != nullptr ? a.q_len[b] : a.Sq;
  sq = sq < 0 ? 0 : (sq > a.Sq ? a.Sq : sq);
  int src = a.kv_src != nullptr ? a.kv_src[b] : b;
  if (src < 0 || src >= a.n_src) {   // no such source: nothing of it is read, the entry's maps and cam row are zeros
    src = 0;
    sq = 0;
  }
  const int kj = kt * 64 + w * 16 + lr;                 // this lane's key
  const int kjc = kj < a.Sk ? kj : a.Sk - 1;            // (past the last key: a finite row, nothing of it is stored)
  const bf16* kp = a.k + ((long)src * a.Sk + kjc) * a.k_rs + 8 * lg;
  const bf16* vp = a.v + ((long)src * a.Sk + kjc) * a.v_rs + 8 * lg;
  char* sQ = lds;
  char* sD = lds + ATTN_TILE;
  float acc = 0.f;
  for (int h = 0; h < a.H; ++h) {
    __syncthreads();   // the previous head's fragments are read
    stage_pair<64, 2>(sQ, a.q + qbase * a.q_rs + h * 64, a.q_rs, sD, a.dout + qbase * a.do_rs + h * 64, a.do_rs, 0, sq, tid, GRADCAM_THREADS);
    const bf16x8 kf0 = *reinterpret_cast<const bf16x8*>(kp + h * 64), kf1 = *reinterpret_cast<const bf16x8*>(kp + h * 64 + 32);
    const bf16x8 vf0 = *reinterpret_cast<const bf16x8*>(vp + h * 64), vf1 = *reinterpret_cast<const bf16x8*>(vp + h * 64 + 32);
    __syncthreads();
    const float* lse = a.lse + ((long)b * a.H + h) * a.stat_ld;
    const long map_row0 = ((long)b * a.H + h) * a.Sq;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int q0 = t * 16 + 4 * lg;
      f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, g = f32x4{0.f, 0.f, 0.f, 0.f}, l = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t * 16 < sq) {   // (workgroup-uniform: a tile of padding rows has nothing to multiply)
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sQ, t * 16, 0, lr, lg), kf0, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sQ, t * 16, 1, lr, lg), kf1, s, 0, 0, 0);
        g = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sD, t * 16, 0, lr, lg), vf0, g, 0, 0, 0);
        g = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sD, t * 16, 1, lr, lg), vf1, g, 0, 0, 0);
        if (q0 < sq) l = *reinterpret_cast<const f32x4*>(lse + q0);   // q0 + 3 < stat_ld: stat_ld is a multiple of 4 and >= Sq
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = q0 + r;
        const bool valid = qi < sq;   // columns [q_len, stat_ld) of lse hold nothing: selected away, never multiplied
        const float p = valid ? expf(fmaf(s[r], a.scale, -l[r])) : 0.f;
        const float dp = valid ? g[r] : 0.f;
        acc = fmaf(p, fmaxf(dp, 0.f), acc);
        if (qi < a.Sq && kj < a.Sk) {
          const long at = (map_row0 + qi) * a.Sk + kj;
          if (a.p_out != nullptr) a.p_out[at] = p;
          if (a.dp_out != nullptr) a.dp_out[at] = dp;
        }
      }
    }
  }
  acc = group4_sum(acc);   // the four lanes of a key hold disjoint query rows
  if (a.cam != nullptr && lg == 0 && kj >= 1 && kj < a.Sk) a.cam[(long)b * (a.Sk - 1) + (kj - 1)] = acc / ((float)a.H * (float)a.t_div);
}

static bool gradcam_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int xfm_xattn_gradcam_impl(const GradcamArgs* ap, hipStream_t st) {
  const GradcamArgs& a = *ap;
  XFM_REQUIRE(a.q != nullptr && a.dout != nullptr && a.k != nullptr && a.v != nullptr && a.lse != nullptr, "xattn_gradcam: null operand");
  XFM_REQUIRE(a.cam != nullptr || a.p_out != nullptr || a.dp_out != nullptr, "xattn_gradcam: no output asked for (cam, p_out, dp_out all NULL)");
  XFM_REQUIRE(a.B >= 1 && a.B <= 65535 && a.H >= 1 && a.Sq >= 1 && a.Sk >= 2, "xattn_gradcam: B=%d H=%d Sq=%d Sk=%d (need 1 <= B <= 65535, H, Sq >= 1, Sk >= 2)",
              a.B, a.H, a.Sq, a.Sk);
  const long cols = (long)a.H * 64;
  XFM_REQUIRE(a.q_rs >= cols && a.do_rs >= cols && a.k_rs >= cols && a.v_rs >= cols, "xattn_gradcam: a row stride below H * 64 = %ld", cols);
  XFM_REQUIRE(a.q_rs % 8 == 0 && a.do_rs % 8 == 0 && a.k_rs % 8 == 0 && a.v_rs % 8 == 0 && gradcam_aligned(a.q) && gradcam_aligned(a.dout) &&
                  gradcam_aligned(a.k) && gradcam_aligned(a.v) && gradcam_aligned(a.lse),
              "xattn_gradcam: operands must be 16-byte aligned, row strides multiples of 8");
  XFM_REQUIRE(a.stat_ld >= a.Sq && a.stat_ld % 4 == 0, "xattn_gradcam: stat_ld=%ld (need a multiple of 4, >= Sq=%d)", a.stat_ld, a.Sq);
  XFM_REQUIRE(a.q_start == nullptr || a.q_len != nullptr, "xattn_gradcam: q_start without q_len");
  XFM_REQUIRE(a.n_src >= 1 && a.t_div >= 1, "xattn_gradcam: n_src=%d t_div=%d (need >= 1)", a.n_src, a.t_div);
  XFM_REQUIRE(a.scale > 0.f && a.scale < 3.0e38f, "xattn_gradcam: scale must be positive and finite");
  if (a.Sq > 64) {
    xfm_set_error("xattn_gradcam: Sq=%d (the kernel keeps one entry's query rows in one 64-row tile)", a.Sq);
    return XFM_E_UNSUPPORTED;
  }
  hipLaunchKernelGGL(xattn_gradcam_kernel, dim3(cdiv(a.Sk, 64), a.B), dim3(GRADCAM_THREADS), 0, st, a);
  return xfm_check_launch("xattn_gradcam");
}
