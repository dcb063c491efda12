// Incremental decoding (models/xbert.py:1368-1484, models/xroberta.py:1130-1153; the cached branches of the self- and cross-attention
// at models/xroberta.py:224-262): attention of ONE new query token per batch row against a key/value cache, and the token choice of one
// decoding step.
//   decode_attn   one workgroup per (batch row, head), one wave per 64-key chunk (up to 8 waves), head_dim 64.  With a single query row
//                 an MFMA tile would be 1/16 used and the kernel is bound by reading 2 * Sk * 128 bytes per (b, h), so this is a plain
//                 vector kernel: 8 lanes x 16 bytes cover one key row, 8 rows per load instruction; q.k, the online softmax (64-key chunks)
//                 and P.V all in fp32; the probabilities are never rounded to bf16.  In self mode the workgroup that owns (b, h) appends k_new / v_new to cache row pos itself and reads the new
//                 key from k_new / v_new, never back from the cache: no second launch, no ordering between workgroups.
//   next_token    one workgroup per row of fp32 logits: repetition penalty (once per distinct id, through an LDS bitmap), argmax with the
//                 lowest index among equal maxima (or a pre-drawn token), log_softmax at the token in ce_fwd_kernel's arithmetic, the
//                 unfinished bookkeeping of xbert.py:1446-1462.  No float atomics: every result is a plain store of one lane, and the count
//                 of unfinished rows is one integer add per row -- the same bits with and without XFM_DETERMINISTIC.
#include "common.h"

constexpr int DECODE_PEN_WORDS = XFM_NEXT_TOKEN_MAX_V / 32;   // LDS bitmap of the ids seen so far

// 8 bf16 of a row as fp32
__device__ __forceinline__ void decode_load8(const bf16* p, float (&f)[8]) {
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = bf2f(v[e]);
}

// One workgroup of 1 .. 8 waves per (b, h); wave w walks the 64-key chunks w, w + nw, ...  Lane l = (r = l >> 3, g = l & 7): in step i
// of a chunk it holds the 16 bytes [g * 8, g * 8 + 8) of key chunk * 64 + i * 8 + r -- the K and the V rows of a chunk are all requested
// before the first is used (16 loads of 16 bytes in flight per lane).  Every wave keeps its own running (max, sum, accumulator); they meet
// through LDS at the end: o = sum_w o_w exp(m_w - M) / sum_w l_w exp(m_w - M).
constexpr int DECODE_MAX_WAVES = 8;

__global__ __launch_bounds__(64 * DECODE_MAX_WAVES) void decode_attn_kernel(const xfm_decode_attn_args a) {
  __shared__ float part[DECODE_MAX_WAVES][8][64];
  __shared__ float o_w[DECODE_MAX_WAVES][64];
  __shared__ float ml_w[DECODE_MAX_WAVES][2];
  const int b = blockIdx.x / a.H, h = blockIdx.x - b * a.H;
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int lane = threadIdx.x & 63, r = lane >> 3, g = lane & 7, n_keys = a.Sk;
  const bool self = a.k_new != nullptr;
  bf16* out = a.o + (long)b * a.o_rs + h * 64;
  const int src = a.kv_index != nullptr ? a.kv_index[b] : b;
  if (src < 0 || src >= a.n_src) {   // no such source (uniform over the workgroup): nothing is read, the row is zero
    if (wave == 0) out[lane] = f2bf(0.f);
    return;
  }
  const long col = (long)h * 64 + g * 8;
  const bf16* kc = a.k_cache + (long)src * a.cap * a.rs + col;
  const bf16* vc = a.v_cache + (long)src * a.cap * a.rs + col;
  const bf16* kn = self ? a.k_new + (long)b * a.k_new_rs + col : nullptr;
  const bf16* vn = self ? a.v_new + (long)b * a.v_new_rs + col : nullptr;
  const int last = self ? a.pos : -1;   // the key that lives in k_new / v_new (read from there, never back from the cache)
  if (self && wave == 0 && r < 2) {     // the append: 8 lanes copy the key row, 8 the value row
    const bf16* from = r == 0 ? kn : vn;
    bf16* to = (r == 0 ? a.k_cache : a.v_cache) + ((long)src * a.cap + a.pos) * a.rs + col;
    *reinterpret_cast<bf16x8*>(to) = *reinterpret_cast<const bf16x8*>(from);
  }
  float q[8];
  decode_load8(a.q + (long)b * a.q_rs + col, q);
  const int* keep = a.key_keep != nullptr ? a.key_keep + (long)src * a.keep_ld : nullptr;

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int base = wave * 64; base < n_keys; base += nw * 64) {
    bf16x8 kraw[8], vraw[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = base + i * 8 + r;
      if (j < n_keys) {
        kraw[i] = *reinterpret_cast<const bf16x8*>(j == last ? kn : kc + (long)j * a.rs);
        vraw[i] = *reinterpret_cast<const bf16x8*>(j == last ? vn : vc + (long)j * a.rs);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) kraw[i][e] = vraw[i][e] = f2bf(0.f);
      }
    }
    float s[8];
    float cmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = base + i * 8 + r;
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) d = fmaf(q[e], bf2f(kraw[i][e]), d);
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      d += __shfl_xor(d, 4, 64);
      float sc = -INFINITY;
      if (j < n_keys) {
        sc = d * a.scale;
        if (keep != nullptr && keep[j] == 0) sc += -10000.f;
      }
      s[i] = sc;
      cmax = fmaxf(cmax, sc);
    }
    const float mn = fmaxf(m, wave_max(cmax));   // finite: key `base` exists
    const float alpha = __expf(m - mn);
    m = mn;
    float psum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= alpha;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float p = __expf(s[i] - mn);           // 0 past the end (where the V registers hold zeros)
      psum += p;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(p, bf2f(vraw[i][e]), acc[e]);
    }
    l = fmaf(l, alpha, wave_sum(g == 0 ? psum : 0.f));   // each key counted once
  }
  // the wave's 8 partial rows (one per r) -> its output row, then the waves meet
#pragma unroll
  for (int e = 0; e < 8; ++e) part[wave][r][g * 8 + e] = acc[e];
  __syncthreads();
  float o = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) o += part[wave][i][lane];
  o_w[wave][lane] = o;
  if (lane == 0) {
    ml_w[wave][0] = m;
    ml_w[wave][1] = l;
  }
  __syncthreads();
  if (wave == 0) {
    float M = ml_w[0][0];   // finite: wave 0 always has chunk 0
    for (int w = 1; w < nw; ++w) M = fmaxf(M, ml_w[w][0]);
    float osum = 0.f, lsum = 0.f;
    for (int w = 0; w < nw; ++w) {
      const float f = __expf(ml_w[w][0] - M);   // a wave without a chunk: exp(-inf) = 0 times its zeros
      osum = fmaf(o_w[w][lane], f, osum);
      lsum = fmaf(ml_w[w][1], f, lsum);
    }
    out[lane] = f2bf(osum / lsum);
  }
}

int xfm_decode_attn_impl(const xfm_decode_attn_args& a, hipStream_t st) {
  XFM_REQUIRE(a.q && a.k_cache && a.v_cache && a.o, "decode_attn: null operand");
  XFM_REQUIRE(a.B >= 1 && a.H >= 1 && a.cap >= 1 && a.n_src >= 1, "decode_attn: B=%d H=%d cap=%d n_src=%d (need all >= 1)", a.B, a.H, a.cap,
              a.n_src);
  XFM_REQUIRE((long)a.H * 64 <= a.rs, "decode_attn: H * 64 = %ld exceeds the cache row stride %ld", (long)a.H * 64, a.rs);
  XFM_REQUIRE((long)a.H * 64 <= a.q_rs && (long)a.H * 64 <= a.o_rs, "decode_attn: q / o row strides %ld / %ld below H * 64", a.q_rs, a.o_rs);
  XFM_REQUIRE(a.Sk >= 1, "decode_attn: Sk = %d (need >= 1)", a.Sk);
  const bool self = a.k_new != nullptr;
  if (self) {
    XFM_REQUIRE(a.v_new != nullptr && a.kv_index == nullptr, "decode_attn: self mode needs v_new and takes no kv_index");
    XFM_REQUIRE(a.pos >= 0 && (long)a.pos + 1 <= a.cap, "decode_attn: pos + 1 = %ld exceeds the cache capacity %d", (long)a.pos + 1, a.cap);
    XFM_REQUIRE(a.Sk == a.pos + 1, "decode_attn: self mode attends over pos + 1 = %d keys, Sk = %d", a.pos + 1, a.Sk);
    XFM_REQUIRE(a.n_src == a.B, "decode_attn: self mode has one cache entry per batch row");
    XFM_REQUIRE((long)a.H * 64 <= a.k_new_rs && (long)a.H * 64 <= a.v_new_rs, "decode_attn: k_new / v_new row strides below H * 64");
    XFM_REQUIRE(aligned16(a.k_new) && aligned16(a.v_new) && a.k_new_rs % 8 == 0 && a.v_new_rs % 8 == 0,
                "decode_attn: k_new / v_new rows must start on 16 bytes");
  } else {
    XFM_REQUIRE(a.v_new == nullptr, "decode_attn: v_new without k_new");
    XFM_REQUIRE(a.Sk <= a.cap, "decode_attn: Sk = %d exceeds the cache capacity %d", a.Sk, a.cap);
  }
  XFM_REQUIRE(a.key_keep == nullptr || a.keep_ld >= a.Sk, "decode_attn: key_keep row stride %ld below Sk = %d", a.keep_ld, a.Sk);
  XFM_REQUIRE(aligned16(a.q) && aligned16(a.k_cache) && aligned16(a.v_cache) && a.q_rs % 8 == 0 && a.rs % 8 == 0,
              "decode_attn: q and cache rows must start on 16 bytes");
  XFM_REQUIRE((long)a.B * a.H < (1L << 31), "decode_attn: B * H too large");
  const int chunks = (a.Sk + 63) / 64;   // one wave per 64-key chunk, up to 8: the kernel waits on memory, more waves keep more of it in flight
  const int waves = chunks < DECODE_MAX_WAVES ? chunks : DECODE_MAX_WAVES;
  hipLaunchKernelGGL(decode_attn_kernel, dim3(a.B * a.H), dim3(64 * waves), 0, st, a);
  return xfm_check_launch("decode_attn");
}

// ---------------------------------------------------------------------------------------------------------------------- next_token
// The (penalised) logit of column j: xbert.py:1425-1432 in fp32 -- negative logits times the penalty, the others divided by it, for the
// columns whose bit is set in `seen`.
__device__ __forceinline__ float next_token_value(float x, int j, const uint32_t* seen, float penalty) {
  if (seen != nullptr && ((seen[j >> 5] >> (j & 31)) & 1u)) return x < 0.f ? x * penalty : x / penalty;
  return x;
}

__global__ __launch_bounds__(256) void next_token_kernel(const xfm_next_token_args a) {
  __shared__ uint32_t seen_bits[DECODE_PEN_WORDS];
  __shared__ float red[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* x = a.logits + (long)row * a.ld;
  int64_t* ids = a.ids + (long)row * a.ids_ld;
  const int V = a.V;
  const uint32_t* seen = nullptr;
  if (a.penalty != 1.0f) {
    const int words = (V + 31) >> 5;
    for (int w = tid; w < words; w += 256) seen_bits[w] = 0u;
    __syncthreads();
    for (int t = tid; t < a.cur_len; t += 256) {
      const int64_t id = ids[t];
      if (id >= 0 && id < V) atomicOr(&seen_bits[id >> 5], 1u << (id & 31));   // LDS integer or: a repeated id sets its bit once
    }
    __syncthreads();
    seen = seen_bits;
  }
  // maximum and the lowest column that holds it (a thread walks its columns in rising order, so `>` keeps its first)
  float mx = -INFINITY;
  int at = V;
  for (int c = tid; c < V; c += 256) {
    const float v = next_token_value(x[c], c, seen, a.penalty);
    if (v > mx) { mx = v; at = c; }
  }
  const float bmx = block_max256(mx, red);
  // columns are below 2^24, exact in fp32: the lowest column among the threads that hold the maximum is a max of the negated column
  const float cand = (mx == bmx && at < V) ? -(float)at : -(float)V;
  int tok = (int)(-block_max256(cand, red));
  if (tok >= V) tok = 0;   // a row without a finite maximum (all -inf / NaN): torch.argmax's column 0
  float s = 0.f;
  for (int c = tid; c < V; c += 256) s += __expf(next_token_value(x[c], c, seen, a.penalty) - bmx);
  s = block_sum256_serial(s, red);
  if (tid == 0) {
    const float lse = bmx + __logf(s);
    long chosen = tok;
    if (a.next_token != nullptr) chosen = a.next_token[row];
    float lp = __uint_as_float(0x7FC00000u);   // a pre-drawn token outside [0, V): nothing is read
    if (chosen >= 0 && chosen < V) lp = next_token_value(x[chosen], (int)chosen, seen, a.penalty) - lse;
    const int unf = a.unfinished[row] != 0 ? 1 : 0;
    const int64_t add = unf ? (int64_t)chosen : (int64_t)a.pad_id;
    ids[a.cur_len] = add;
    a.hist_unfinished[(long)row * a.hist_ld + a.step] = unf;
    a.hist_logprob[(long)row * a.hist_ld + a.step] = lp;
    int still = unf;
    for (int e = 0; e < a.n_eos; ++e) still = (add == (int64_t)a.eos_ids[e]) ? 0 : still;
    a.unfinished[row] = still;
    if (still && a.n_unfinished != nullptr) atomicAdd(a.n_unfinished, 1);   // integer: the order of the rows cannot change the sum
  }
}

int xfm_next_token_impl(const xfm_next_token_args& a, hipStream_t st) {
  XFM_REQUIRE(a.logits && a.ids && a.unfinished && a.hist_unfinished && a.hist_logprob, "next_token: null operand");
  XFM_REQUIRE(a.B >= 1 && a.V >= 1 && (long)a.V <= a.ld, "next_token: B=%d V=%d ld=%ld (need B >= 1, 1 <= V <= ld)", a.B, a.V, a.ld);
  XFM_REQUIRE(a.V <= XFM_NEXT_TOKEN_MAX_V, "next_token: V = %d exceeds %d", a.V, XFM_NEXT_TOKEN_MAX_V);
  XFM_REQUIRE(a.cur_len >= 0 && (long)a.cur_len < a.ids_ld, "next_token: column cur_len = %d is outside the id rows of %ld", a.cur_len, a.ids_ld);
  XFM_REQUIRE(a.step >= 0 && (long)a.step < a.hist_ld, "next_token: step %d is outside the history rows of %ld", a.step, a.hist_ld);
  XFM_REQUIRE(a.n_eos >= 0 && a.n_eos <= XFM_NEXT_TOKEN_MAX_EOS, "next_token: %d eos ids (at most %d)", a.n_eos, XFM_NEXT_TOKEN_MAX_EOS);
  XFM_REQUIRE(a.penalty > 0.f, "next_token: repetition penalty %g (need > 0)", (double)a.penalty);
  hipLaunchKernelGGL(next_token_kernel, dim3(a.B), dim3(256), 0, st, a);
  return xfm_check_launch("next_token");
}
