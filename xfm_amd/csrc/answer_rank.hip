// The inference side of the VQA task (VQA.py:75-100 evaluation -> model_generation.py:146-202 rank_answer): answers are RANKED, not
// generated.  Two kernels, one workgroup (256 lanes) per question, plain vector loads and stores, no atomics:
//   answer_shortlist  first-token logits -> the k most probable candidates            (model_generation.py:157-160: softmax over the
//                     vocabulary, index_select of the candidates' first tokens, topk)
//   answer_rerank     chain-rule score log p(first) - NLL(rest), softmax over the k, sort, and the winner's candidate id into a device
//                     result buffer                                                    (model_generation.py:194-200, VQA.py:95-98)
// Both ORDER by the key (probability descending, position ascending).  The key is unique, so the result does not depend on the launch
// geometry or on the order the lanes meet the elements: it is packed into 64 bits -- the probability's fp32 bits (non-negative floats
// order like unsigned integers) above the complemented position -- and a bitonic network in LDS sorts the keys descending.  Padding keys
// are 0, below every real key (a real key's low word is ~position != 0).
#include "common.h"

constexpr int ANSWER_THREADS = 256;
static_assert(XFM_ANSWER_MAX_K <= XFM_ANSWER_MAX_A, "the shortlist is a prefix of the sorted candidates");

__device__ __forceinline__ unsigned long long answer_key(float p, int pos) {
  return ((unsigned long long)__float_as_uint(p) << 32) | (unsigned long long)(~(uint32_t)pos);
}
__device__ __forceinline__ float answer_key_prob(unsigned long long key) { return __uint_as_float((uint32_t)(key >> 32)); }
__device__ __forceinline__ int answer_key_pos(unsigned long long key) { return (int)(~(uint32_t)key); }

// keys[0 .. n) descending, n a power of two >= 2, all 256 lanes; ends with a barrier
__device__ __forceinline__ void answer_sort_desc(unsigned long long* keys, int n) {
  const int tid = threadIdx.x;
  for (int span = 2; span <= n; span <<= 1) {
    for (int j = span >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (n >> 1); t += ANSWER_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;   // l < n: i has bit j clear and i < n
        const unsigned long long a = keys[i], b = keys[l];
        const bool desc = (i & span) == 0;
        if ((a < b) == desc && a != b) { keys[i] = b; keys[l] = a; }
      }
      __syncthreads();
    }
  }
}

// Dynamic LDS: n_pad keys (8 bytes each), then 4 floats.  vec: every row starts on 16 bytes (ld % 4 == 0, aligned base).
// Two passes over the row (max, then sum of expf(x - max) with the accurate expf: the probabilities are compared against fp64 softmax
// at the resolution of fp32 arithmetic, which __expf's argument scaling does not keep for |x - max| ~ 100); the row is 200 KB at the
// RoBERTa vocabulary and the second pass reads it from L2.
__global__ __launch_bounds__(ANSWER_THREADS) void answer_shortlist_kernel(const float* __restrict__ logits, long ld, int V,
                                                                          const int64_t* __restrict__ first_tok, int A, int k, int n_pad,
                                                                          int vec, float* __restrict__ prob, int64_t* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) unsigned char answer_lds[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(answer_lds);
  float* red = reinterpret_cast<float*>(keys + n_pad);
  const int tid = threadIdx.x;
  const long q = blockIdx.x;
  const float* x = logits + q * ld;
  const int Vv = vec ? (V & ~3) : 0;   // columns covered by whole 16-byte granules
  float m = -3.0e38f;
  for (int c = tid * 4; c < Vv; c += ANSWER_THREADS * 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + c);
    m = fmaxf(m, fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])));
  }
  for (int c = Vv + tid; c < V; c += ANSWER_THREADS) m = fmaxf(m, x[c]);
  m = block_max256(m, red);
  float s = 0.f;
  for (int c = tid * 4; c < Vv; c += ANSWER_THREADS * 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + c);
    s += (expf(a[0] - m) + expf(a[1] - m)) + (expf(a[2] - m) + expf(a[3] - m));
  }
  for (int c = Vv + tid; c < V; c += ANSWER_THREADS) s += expf(x[c] - m);
  s = block_sum256(s, red);
  for (int a = tid; a < n_pad; a += ANSWER_THREADS) {
    unsigned long long key = 0ull;
    if (a < A) {
      const int64_t t = first_tok[a];
      // a first token outside the vocabulary is the caller's error: such a candidate gets probability 0 and is never read out of bounds
      const float p = (t >= 0 && t < V) ? expf(x[t] - m) / s : 0.f;
      key = answer_key(p, a);
    }
    keys[a] = key;
  }
  __syncthreads();
  answer_sort_desc(keys, n_pad);
  for (int j = tid; j < k; j += ANSWER_THREADS) {
    const unsigned long long key = keys[j];
    prob[q * k + j] = answer_key_prob(key);
    cand[q * k + j] = (int64_t)answer_key_pos(key);
  }
}

// k <= XFM_ANSWER_MAX_K keys in static LDS.  score_j = log(prob_j) - seq_loss_j (prob 0 -> -inf, as torch), softmax over the k (accurate
// logf / expf), sort on (probability descending, position ascending).
__global__ __launch_bounds__(ANSWER_THREADS) void answer_rerank_kernel(const float* __restrict__ prob, const float* __restrict__ seq_loss,
                                                                       const int64_t* __restrict__ cand, int k, int n_pad,
                                                                       int64_t* __restrict__ topk_ids, float* __restrict__ topk_probs,
                                                                       int64_t* __restrict__ result, long result_offset) {
  __shared__ unsigned long long keys[XFM_ANSWER_MAX_K];
  __shared__ float score[XFM_ANSWER_MAX_K];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const long q = blockIdx.x;
  float m = -3.0e38f;
  for (int j = tid; j < k; j += ANSWER_THREADS) {
    const float sc = logf(prob[q * k + j]) - seq_loss[q * k + j];
    score[j] = sc;
    m = fmaxf(m, sc);
  }
  m = block_max256(m, red);
  float s = 0.f;
  for (int j = tid; j < k; j += ANSWER_THREADS) s += expf(score[j] - m);   // (each lane reads back its own entries)
  s = block_sum256(s, red);
  for (int j = tid; j < n_pad; j += ANSWER_THREADS) keys[j] = j < k ? answer_key(expf(score[j] - m) / s, j) : 0ull;
  __syncthreads();
  answer_sort_desc(keys, n_pad);
  for (int j = tid; j < k; j += ANSWER_THREADS) {
    const unsigned long long key = keys[j];
    const int64_t id = cand[q * k + answer_key_pos(key)];
    topk_probs[q * k + j] = answer_key_prob(key);
    topk_ids[q * k + j] = id;
    if (j == 0 && result != nullptr) result[result_offset + q] = id;
  }
}

static inline int answer_pow2(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

int xfm_answer_shortlist_impl(const float* logits, long ld, int Q, int V, const int64_t* first_tok, int A, int k, float* prob, int64_t* cand,
                              hipStream_t st) {
  XFM_REQUIRE(Q >= 1 && V >= 1 && ld >= V, "answer_shortlist: bad shape Q=%d V=%d ld=%ld (need Q >= 1, 1 <= V <= ld)", Q, V, ld);
  XFM_REQUIRE(A >= 1 && A <= XFM_ANSWER_MAX_A, "answer_shortlist: A=%d outside [1, %d]", A, XFM_ANSWER_MAX_A);
  XFM_REQUIRE(k >= 1 && k <= A && k <= XFM_ANSWER_MAX_K, "answer_shortlist: k=%d outside [1, min(A=%d, %d)]", k, A, XFM_ANSWER_MAX_K);
  const int n_pad = answer_pow2(A);
  const int vec = rows_aligned16(logits, ld) ? 1 : 0;
  constexpr int MAX_LDS = XFM_ANSWER_MAX_A * 8 + 16;
  lds_launch<answer_shortlist_kernel, MAX_LDS>(dim3(Q), dim3(ANSWER_THREADS), (size_t)n_pad * 8 + 16, st, logits, ld, V, first_tok, A, k, n_pad,
                                               vec, prob, cand);
  return xfm_check_launch("answer_shortlist");
}

int xfm_answer_rerank_impl(const float* prob, const float* seq_loss, const int64_t* cand, int Q, int k, int64_t* topk_ids, float* topk_probs,
                           int64_t* result, long result_offset, hipStream_t st) {
  XFM_REQUIRE(Q >= 1 && k >= 1 && k <= XFM_ANSWER_MAX_K, "answer_rerank: bad shape Q=%d k=%d (need Q >= 1, 1 <= k <= %d)", Q, k, XFM_ANSWER_MAX_K);
  XFM_REQUIRE(result == nullptr || result_offset >= 0, "answer_rerank: negative result offset %ld", result_offset);
  hipLaunchKernelGGL(answer_rerank_kernel, dim3(Q), dim3(ANSWER_THREADS), 0, st, prob, seq_loss, cand, k, answer_pow2(k), topk_ids, topk_probs,
                     result, result_offset);
  return xfm_check_launch("answer_rerank");
}
