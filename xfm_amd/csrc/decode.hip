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
//   sample_token  the sampled step (xbert.py:1434-1441 with top_k_top_p_filtering :1487-1519) in one launch: one workgroup of 1024 lanes
//                 per row; penalty and temperature, top-k and top-p by radix selects, the draw, the score, next_token's bookkeeping.
//                 All sums are 64-bit integer sums of fixed-point weights (see above the kernel).
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

// The bookkeeping of one row's step (xbert.py:1449-1462), by one lane; A = xfm_next_token_args or xfm_sample_token_args (the same fields).
template <class A>
__device__ __forceinline__ void decode_book_step(const A& a, int64_t* ids, int row, long chosen, float lp) {
  const int unf = a.unfinished[row] != 0 ? 1 : 0;
  const int64_t add = unf ? (int64_t)chosen : (int64_t)a.pad_id;
  ids[a.cur_len] = add;
  a.hist_unfinished[(long)row * a.hist_ld + a.step] = unf;
  a.hist_logprob[(long)row * a.hist_ld + a.step] = lp;
  int still = unf;
  for (int e = 0; e < a.n_eos; ++e) still = (add == (int64_t)a.eos_ids[e]) ? 0 : still;
  a.unfinished[row] = still;
  int* const counter = a.n_unfinished;
  if (still && counter != nullptr) atomicAdd(counter, 1);   // integer: the order of the rows cannot change the sum
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
    decode_book_step(a, ids, row, chosen, lp);
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

// -------------------------------------------------------------------------------------------------------------------- sample_token
// One workgroup of 1024 lanes per row; the row (196 KiB at V = 50 265, more than the LDS) stays in global memory / L2 and every pass
// recomputes z_j = penalised logit / temperature from it (one load, one divide).  Passes over the row:
//   always      1 maximum (+ the NaN / inf check), 2 the kept weights: Z, the first level of the draw, `filtered`;
//   top_k > 0   4 more: a radix select (8-bit digits, per-bin COUNTS in LDS) of the k'-th largest 32-bit image of z;
//   top_p < 1   4 more: a radix select over per-bin MASS of the image where the running softmax mass passes top_p; a cut that falls
//               inside a run of equal values takes 4 count passes over the columns of that run (lowest columns stay).
// Weights are integers, w_j = floor(2^44 exp(z_j - m)), and every sum of them a 64-bit integer sum (at most 2^17 * 2^44 = 2^61): LDS
// integer atomics and wave shuffles in any order give the same bits, and the longest chain of fp32 additions in the kernel is ZERO long
// -- the error of a running sum is the V floors, below 2^17 * 2^-44 = 2^-27 of Z (Z >= w_max = 1), against the 1e-4 the tests allow.
// The draw walks the columns in rising order through three levels (64 bins of 2048 columns from pass 2, then 64 bins of 32 and 32
// single columns read by wave 0 alone).
constexpr int SAMPLE_LANES = 1024;
constexpr float SAMPLE_FIX = 17592186044416.f;   // 2^44
typedef unsigned long long sample_u64;

struct SampleRow {
  const float* x;
  const uint32_t* seen;
  float penalty, temperature;
  __device__ __forceinline__ float z(int c) const {
    const float v = next_token_value(x[c], c, seen, penalty) / temperature;
    return v == 0.f ? 0.f : v;   // -0 -> +0: equal values get equal images
  }
};
// order-preserving 32-bit image of a float (no NaN reaches it) and back
__device__ __forceinline__ uint32_t sample_key(float z) {
  const uint32_t u = __float_as_uint(z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sample_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
__device__ __forceinline__ sample_u64 sample_mass(float z, float m) { return (sample_u64)(__expf(z - m) * SAMPLE_FIX); }

__device__ __forceinline__ sample_u64 wave_sum_u64(sample_u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <class T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// The k-th largest key (1 <= k <= the number of members) among the members of the row.  MODE 0: every column, keyed by the image of
// z.  MODE 1: the columns whose image is `tie`, keyed by V - 1 - column (the k-th LOWEST column of a run of equal values).
template <int MODE>
__device__ uint32_t sample_select_count(const SampleRow& r, int V, uint32_t k, uint32_t tie, uint32_t* hist, uint32_t* pick) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    for (int c = tid; c < V; c += SAMPLE_LANES) {
      const uint32_t zk = sample_key(r.z(c));
      if (MODE == 1 && zk != tie) continue;
      const uint32_t key = MODE == 0 ? zk : (uint32_t)(V - 1 - c);
      if (shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {   // lane l owns bins 255 - 4 l .. 252 - 4 l: the scan runs from the largest digit down
      uint32_t h[4], s = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) { h[e] = hist[255 - 4 * tid - e]; s += h[e]; }
      uint32_t run = wave_scan_incl(s, tid) - s;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (run < k && run + h[e] >= k) { pick[0] = (uint32_t)(255 - 4 * tid - e); pick[1] = k - run; }
        run += h[e];
      }
    }
    __syncthreads();
    prefix |= pick[0] << shift;
    k = pick[1];
  }
  return prefix;
}

// Top-p cut over the columns whose image is >= kmin: walking the images downwards, the lowest image whose columns still start at a
// running mass <= floor(top_p * total).  -> key; pick[1] = the mass above that image, pick[2] = the mass of its columns, pick[3] = the limit.
__device__ uint32_t sample_select_mass(const SampleRow& r, int V, float m, uint32_t kmin, float top_p, sample_u64* mh, sample_u64* pick) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0;
  sample_u64 above = 0, limit = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) mh[tid] = 0ull;
    __syncthreads();
    for (int c = tid; c < V; c += SAMPLE_LANES) {
      const float z = r.z(c);
      const uint32_t zk = sample_key(z);
      if (zk < kmin) continue;
      if (shift == 24 || (zk >> (shift + 8)) == (prefix >> (shift + 8))) {
        const sample_u64 w = sample_mass(z, m);
        if (w != 0ull) atomicAdd(&mh[(zk >> shift) & 255u], w);
      }
    }
    __syncthreads();
    if (tid < 64) {
      sample_u64 h[4], s = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) { h[e] = mh[255 - 4 * tid - e]; s += h[e]; }
      const sample_u64 inc = wave_scan_incl(s, tid);
      if (shift == 24) {   // the total of the first level is the softmax denominator of the top-p stage
        const sample_u64 total = __shfl(inc, 63, 64);
        limit = (sample_u64)((double)top_p * (double)total);   // top_p < 1: below the total
        if (tid == 0) pick[3] = limit;
      }
      sample_u64 run = above + inc - s;
#pragma unroll
      for (int e = 0; e < 4; ++e) {   // exactly one bin: the bins of a level split a mass that straddles the limit
        if (h[e] != 0ull && run <= limit && run + h[e] > limit) { pick[0] = (sample_u64)(255 - 4 * tid - e); pick[1] = run; pick[2] = h[e]; }
        run += h[e];
      }
    }
    __syncthreads();
    prefix |= (uint32_t)pick[0] << shift;
    above = pick[1];
    limit = pick[3];
  }
  return prefix;
}

__global__ __launch_bounds__(SAMPLE_LANES) void sample_token_kernel(const xfm_sample_token_args a) {
  __shared__ uint32_t seen_bits[DECODE_PEN_WORDS];
  __shared__ sample_u64 mh[256];
  __shared__ sample_u64 pick64[4];
  __shared__ sample_u64 draw_bins[64];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t pick32[2];
  __shared__ float red[SAMPLE_LANES / 64];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  int64_t* ids = a.ids + (long)row * a.ids_ld;
  const int V = a.V;
  const uint32_t* seen = nullptr;
  if (a.penalty != 1.0f) {
    const int words = (V + 31) >> 5;
    for (int w = tid; w < words; w += SAMPLE_LANES) seen_bits[w] = 0u;
    __syncthreads();
    for (int t = tid; t < a.cur_len; t += SAMPLE_LANES) {
      const int64_t id = ids[t];
      if (id >= 0 && id < V) atomicOr(&seen_bits[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
    seen = seen_bits;
  }
  const SampleRow r{a.logits + (long)row * a.ld, seen, a.penalty, a.temperature};
  float* filtered = a.filtered != nullptr ? a.filtered + (long)row * a.filtered_ld : nullptr;

  // pass 1: the maximum; a NaN or +inf anywhere, or no finite value, ends the row
  float mx = -INFINITY;
  int bad = 0;
  for (int c = tid; c < V; c += SAMPLE_LANES) {
    const float z = r.z(c);
    bad |= (z != z) || z == INFINITY;
    mx = fmaxf(mx, z);
  }
  mx = wave_max(mx);
  if (lane == 0) red[tid >> 6] = mx;
  bad = __syncthreads_or(bad);
  float m = red[0];
#pragma unroll
  for (int w = 1; w < SAMPLE_LANES / 64; ++w) m = fmaxf(m, red[w]);
  if (bad || m == -INFINITY) {
    if (filtered != nullptr)
      for (int c = tid; c < V; c += SAMPLE_LANES) filtered[c] = r.z(c);
    if (tid == 0) decode_book_step(a, ids, row, 0L, __uint_as_float(0x7FC00000u));
    return;
  }

  // top-k: the image of the k'-th largest value; everything at or above it stays
  uint32_t kmin = 0u;
  if (a.top_k > 0 && a.top_k < V) kmin = sample_select_count<0>(r, V, (uint32_t)a.top_k, 0u, hist, pick32);
  // top-p: images above pkey stay; of the columns AT pkey the lowest ones up to column pcol
  const bool nucleus = a.top_p < 1.0f;
  uint32_t pkey = 0u;
  int pcol = V;
  if (nucleus) {
    pkey = sample_select_mass(r, V, m, kmin, a.top_p, mh, pick64);
    const sample_u64 above = pick64[1], ties = pick64[2], limit = pick64[3];
    const sample_u64 w = sample_mass(sample_unkey(pkey), m);   // > 0: its bin had mass
    const sample_u64 n_ties = ties / w, stay = (limit - above) / w + 1ull;   // tie j (from 0) stays iff above + j w <= limit
    if (stay < n_ties) pcol = V - 1 - (int)sample_select_count<1>(r, V, (uint32_t)stay, pkey, hist, pick32);
  }

  // pass 2: the kept weights -- their sum per 2048 columns (the first level of the draw) and `filtered`
  if (tid < 64) draw_bins[tid] = 0ull;
  __syncthreads();
  for (int c0 = tid - lane; c0 < V; c0 += SAMPLE_LANES) {   // a wave walks 64 columns of one bin together
    const int c = c0 + lane;
    sample_u64 w = 0ull;
    if (c < V) {
      const float z = r.z(c);
      const uint32_t zk = sample_key(z);
      const bool kept = zk >= kmin && (!nucleus || zk > pkey || (zk == pkey && c <= pcol));
      if (kept) w = sample_mass(z, m);
      if (filtered != nullptr) filtered[c] = kept ? z : -INFINITY;
    }
    w = wave_sum_u64(w);
    if (lane == 0 && w != 0ull) atomicAdd(&draw_bins[c0 >> 11], w);
  }
  __syncthreads();
  if (tid >= 64) return;

  // the draw, by wave 0: the lowest kept column whose inclusive running weight exceeds floor(u Z)
  float u;
  if (a.uniforms != nullptr) u = a.uniforms[row];
  else u = (float)(rng_u32(rng_row_key(a.seed_lo, a.seed_hi, (uint32_t)row), (uint32_t)a.step) >> 8) * 5.9604644775390625e-8f;
  sample_u64 h = draw_bins[lane];
  sample_u64 inc = wave_scan_incl(h, lane);
  const sample_u64 Z = __shfl(inc, 63, 64);   // >= 2^44: the maximum is always kept
  sample_u64 target = (sample_u64)((double)u * (double)Z);
  if (!(target < Z)) target = Z - 1ull;       // u >= 1 or rounding: the highest kept column with weight
  int first = __ffsll((unsigned long long)__ballot(inc > target)) - 1;
  sample_u64 base = __shfl(inc - h, first, 64);
  // level 2: lane l sums columns [first * 2048 + 32 l, + 32)
  auto weight = [&](int c) -> sample_u64 {
    if (c >= V) return 0ull;
    const float z = r.z(c);
    const uint32_t zk = sample_key(z);
    const bool kept = zk >= kmin && (!nucleus || zk > pkey || (zk == pkey && c <= pcol));
    return kept ? sample_mass(z, m) : 0ull;
  };
  h = 0ull;
  for (int i = 0; i < 32; ++i) h += weight(first * 2048 + lane * 32 + i);
  inc = base + wave_scan_incl(h, lane);
  const int second = __ffsll((unsigned long long)__ballot(inc > target)) - 1;
  base = __shfl(inc - h, second, 64);
  // level 3: one column per lane
  const int c3 = first * 2048 + second * 32 + (lane & 31);
  h = lane < 32 ? weight(c3) : 0ull;
  inc = base + wave_scan_incl(h, lane);
  const int third = __ffsll((unsigned long long)__ballot(h != 0ull && inc > target)) - 1;
  if (tid == 0) {
    int tok = first * 2048 + second * 32 + third;
    tok = tok < 0 ? 0 : (tok < V ? tok : V - 1);   // (always inside already: the three ballots cannot come up empty)
    const float lp = r.z(tok) - m - __logf((float)Z * (1.0f / SAMPLE_FIX));
    decode_book_step(a, ids, row, (long)tok, lp);
  }
}

int xfm_sample_token_impl(const xfm_sample_token_args& a, hipStream_t st) {
  XFM_REQUIRE(a.logits && a.ids && a.unfinished && a.hist_unfinished && a.hist_logprob, "sample_token: null operand");
  XFM_REQUIRE(a.B >= 1 && a.V >= 1 && (long)a.V <= a.ld, "sample_token: B=%d V=%d ld=%ld (need B >= 1, 1 <= V <= ld)", a.B, a.V, a.ld);
  XFM_REQUIRE(a.V <= XFM_NEXT_TOKEN_MAX_V, "sample_token: V = %d exceeds %d", a.V, XFM_NEXT_TOKEN_MAX_V);
  XFM_REQUIRE(a.cur_len >= 0 && (long)a.cur_len < a.ids_ld, "sample_token: column cur_len = %d is outside the id rows of %ld", a.cur_len, a.ids_ld);
  XFM_REQUIRE(a.step >= 0 && (long)a.step < a.hist_ld, "sample_token: step %d is outside the history rows of %ld", a.step, a.hist_ld);
  XFM_REQUIRE(a.n_eos >= 0 && a.n_eos <= XFM_NEXT_TOKEN_MAX_EOS, "sample_token: %d eos ids (at most %d)", a.n_eos, XFM_NEXT_TOKEN_MAX_EOS);
  XFM_REQUIRE(a.penalty > 0.f, "sample_token: repetition penalty %g (need > 0)", (double)a.penalty);
  XFM_REQUIRE(a.temperature > 0.f && a.temperature <= 3.402823466e38f, "sample_token: temperature %g (need finite and > 0)", (double)a.temperature);
  XFM_REQUIRE(a.top_p > 0.f && a.top_p <= 1.f, "sample_token: top_p %g (need 0 < top_p <= 1)", (double)a.top_p);
  XFM_REQUIRE(a.top_k >= 0, "sample_token: top_k %d (need >= 0)", a.top_k);
  XFM_REQUIRE(a.filtered == nullptr || a.filtered_ld >= (long)a.V, "sample_token: filtered row stride %ld below V = %d", a.filtered_ld, a.V);
  hipLaunchKernelGGL(sample_token_kernel, dim3(a.B), dim3(SAMPLE_LANES), 0, st, a);
  return xfm_check_launch("sample_token");
}
