// Host side of the bf16 MFMA GEMMs (gemm_common.h says what they compute and where the kernel families live): argument checks, the
// launch plans and the _impl entry points behind capi.hip.  Every plan is ONE function that both the workspace query and the call that
// launches read, so the bytes a caller is told to bring and the launches that write through them cannot disagree.
#include "gemm_common.h"
#include <limits.h>
#include "gemm_nt_small.hip"
#include "gemm_nt_256.hip"
#include "nt320_gemm.hip"
#include "gemm_tn_small.hip"
#include "gemm_tn_256.hip"
#include "gemm_cast.hip"

// K-slices of an NT product with a VERY long K loop against very few tiles (LM-head dgrad: K = 50304, 90 tiles of 64x128); 1 = unsliced
static int nt_k_slices(int M, int N, int K) {
  const long t = (long)cdiv(M, 64) * cdiv(N, 128);
  if (K < 8192 || t >= 192) return 1;
  int sp = (int)(512 / t);
  if (sp > K / 1024) sp = K / 1024;
  return sp < 1 ? 1 : sp;
}

// Launch plan of xfm_gemm_nt for a shape: the tile configuration (1 = 128x128, 2 = 64x128, 3 = 64x64, 4 = 256x128 ring, 5 = 256x256
// phase pipeline, 6 = 320x256 one-round tile, 7 = 64x128 on 3 LDS stages, 8 = 64x64 on 4) and, for the tail split, the leading rows
// that run as whole rounds of 256x256 tiles (rows_a > 0: those rows go to configuration 5, the rest is planned again with hint -1).
// Exported as xfm_gemm_nt_plan so that a profiler / benchmark can attribute a call to the kernels it launches.
// The leading dimensions take part: the 256x256 kernel addresses its operands with 32-bit element offsets (nt256_eligible,
// gemm_nt_256.hip), so where the automatic plan or the tail split would pick it for operands past that range it steps down to
// configuration 1, whose row offsets are 64-bit -- as tn_plan does with tn256_eligible.  An explicit hint 5 is left to fail in the launcher.
// Configuration 6 (nt320_gemm.hip) is never chosen automatically: a caller whose M makes 256x256 tiles spill into a nearly empty second
// round asks for it with hint 6, and a call that is not eligible for it (nt320_eligible: N % 256, K % 64, one round of tiles, 32-bit
// offsets) or XFM_GEMM_NT320=0 (A/B knob) is planned as hint 0.
static int nt_plan(int M, int N, int K, long lda, long ldb, int epi, int tile_hint, int* rows_a_out, int* k_splits_out) {
  *rows_a_out = 0;
  *k_splits_out = 1;
  if (tile_hint == 6) {
    static const int nt320_env = xfm_env_int("XFM_GEMM_NT320", 1);
    if (nt320_env && nt320_eligible(M, lda, N, ldb, K)) return 6;
    tile_hint = 0;
  }
  int cfg = tile_hint;
  if (cfg <= 0) {  // measured on MI355X (tools/tune_gemm.py): 128x128 pays from ~3 workgroups per CU, else go smaller
    // Tail split: one workgroup per CU, so T tiles of 256x256 cost ceil(T / 256) rounds.  When the last round would be
    // nearly empty (N = 768: 99 x 3 = 297 tiles = 1.16 rounds), the whole rounds run as 256x256 tiles and the remaining
    // rows go to the small-tile kernels, which fill every CU for a fraction of a big-tile time.
    static const int split_env = xfm_env_int("XFM_GEMM_TAIL_SPLIT", 35);  // tuning knob: max tail % (35 measured best, tools/split_sweep.sh)
    const long tn256 = cdiv(N, 256), t256 = (long)cdiv(M, 256) * tn256;
    if (split_env && tile_hint == 0 && M >= 2048 && t256 > 256 && t256 % 256 != 0 && (t256 % 256) * 100 < split_env * 256) {
      const int rows_a = (int)((t256 / 256) * 256 / tn256) * 256;  // row tiles that exactly fill the whole rounds
      if (rows_a > 0 && rows_a < M) {
        if (!nt256_eligible(rows_a, lda, N, ldb)) return 1;
        *rows_a_out = rows_a;
        return 5;
      }
    }
    // ~half a round of 256x256 tiles already beats the rest on the tall problems (M = 12608 / 25216); on the packed token rows of
    // the text / fusion towers (M ~ 2600 .. 5300, tools/tune_small.py) it needs ~0.7 of a round, below that 128x128 tiles win
    // (5248x1536x768: 25.2 -> 17.4 us, 2624x3072x768: 24.0 -> 17.1 us)
    if (M >= 2048 && (t256 >= 180 || (t256 >= 120 && M >= 8192))) cfg = nt256_eligible(M, lda, N, ldb) ? 5 : 1;
    else if (M >= 2048 && t256 >= 120) cfg = 1;
    else if ((long)cdiv(M, 256) * cdiv(N, 128) >= 768) cfg = 4;  // >= 3 rounds of 256x128 tiles: the 3-slot ring wins on cold operands
    else if ((long)cdiv(M, 128) * cdiv(N, 128) >= 800) cfg = 1;
    else if ((long)cdiv(M, 64) * cdiv(N, 128) >= 512) cfg = 2;
    else if (K >= 1536 && epi != EPI_F32_ACC && (long)cdiv(M, 64) * cdiv(N, 128) < 300) {
      // a long K loop against about one 64x128 tile per CU or fewer (the FFN / QKV dgrads of the text tower and of a 2B-sequence
      // fusion pass): 64x64 tiles double the workgroups and four LDS stages keep three K-tiles in flight
      // (2624x768x3072: 24.4 -> 21.9 us, 1344x768x3072: 24.2 -> 18.5 us, 1344x768x2304: 19.3 -> 14.5 us)
      cfg = 8;
    }
    else if ((long)cdiv(M, 64) * cdiv(N, 128) >= 128 || K >= 1536) {  // under two workgroups per CU (tail-split row blocks, text
      // tower) the 2-stage loop exposes the load latency of every K-step: keep two K-tiles in flight (3-stage 64x128; measured
      // 45.9 -> 31.7 us on 3456x768x3072, 18.9 -> 20.6 us on the 720-tile 7680x768x768 which therefore stays 2-stage)
      cfg = 7;
      // ... and when the loop is VERY long against very few tiles slice K over gridDim.y (nt_k_slices); only the fp32-accumulate
      // epilogue can merge slices (atomics), so callers ask for it with a zeroed fp32 C
      if (epi == EPI_F32_ACC) *k_splits_out = nt_k_slices(M, N, K);
    }
    else cfg = 3;
  }
  return cfg;
}

int xfm_gemm_nt_plan_impl(int M, int N, int K, int epi, int tile_hint, int* cfg, int* rows_a) {
  XFM_REQUIRE(M > 0 && N > 0 && K > 0 && cfg != nullptr && rows_a != nullptr, "gemm_nt_plan: bad arguments");
  int ks = 1;
  *cfg = nt_plan(M, N, K, K, K, epi, tile_hint, rows_a, &ks);   // the plan of tight operands (lda = ldb = K)
  return XFM_OK;
}

// the fields every NT launch sets; the rest (aux, K-slices) stays off
static GemmNT gemm_nt_args(const void* A, long lda, const void* B, long ldb, void* C, long ldc, const float* bias, int M, int N, int K) {
  static const int gm_env = xfm_env_int("XFM_GEMM_GROUP_M", 0);  // tuning knob
  GemmNT g{};
  g.A = (const bf16*)A; g.lda = lda;
  g.B = (const bf16*)B; g.ldb = ldb;
  g.C = C; g.ldc = ldc;
  g.bias = bias;
  g.M = M; g.N = N; g.K = K;
  g.group_m = gm_env > 0 ? gm_env : 8;
  g.k_splits = 1;
  return g;
}

int xfm_gemm_nt_impl(const void* A, long lda, const void* B, long ldb, void* C, long ldc, const float* bias,
                     void* aux, long ldaux, int M, int N, int K, int epi, int tile_hint, hipStream_t st) {
  XFM_REQUIRE(M > 0 && N > 0 && K > 0, "gemm_nt: empty problem M=%d N=%d K=%d", M, N, K);
  XFM_REQUIRE(K % 64 == 0, "gemm_nt: K=%d must be a multiple of 64", K);
  XFM_REQUIRE(lda % 8 == 0 && ldb % 8 == 0, "gemm_nt: lda=%ld ldb=%ld must be multiples of 8", lda, ldb);
  XFM_REQUIRE(((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0 && ((uintptr_t)C % 16) == 0,
              "gemm_nt: operands must be 16-byte aligned");
  XFM_REQUIRE((epi != EPI_GELU && epi != EPI_DGELU) || aux != nullptr, "gemm_nt: epilogue %d needs aux", epi);
  GemmNT g = gemm_nt_args(A, lda, B, ldb, C, ldc, bias, M, N, K);
  g.aux = (bf16*)aux; g.ldaux = ldaux;
  int rows_a = 0, k_splits = 1;
  const int cfg = nt_plan(M, N, K, lda, ldb, epi, tile_hint, &rows_a, &k_splits);
  if (rows_a > 0) {  // tail split: whole rounds of 256x256 tiles first, the remaining rows on the small-tile kernels
    int rc = xfm_gemm_nt_impl(A, lda, B, ldb, C, ldc, bias, aux, ldaux, rows_a, N, K, epi, 5, st);
    if (rc != XFM_OK) return rc;
    const long esz = (epi == EPI_F32 || epi == EPI_F32_ACC) ? 4 : 2;
    return xfm_gemm_nt_impl((const bf16*)A + (long)rows_a * lda, lda, B, ldb, (char*)C + (long)rows_a * ldc * esz, ldc, bias,
                            aux ? (void*)((bf16*)aux + (long)rows_a * ldaux) : nullptr, ldaux, M - rows_a, N, K, epi, -1, st);
  }
  g.k_splits = k_splits;
  switch (cfg) {
    case 1: return launch_nt<128, 128, 2>(g, epi, st);
    case 2: return launch_nt<64, 128, 2>(g, epi, st);
    case 7: return launch_nt<64, 128, 3>(g, epi, st);
    case 8: return launch_nt<64, 64, 4>(g, epi, st);
    case 4: return launch_nt_ring(g, epi, st);
    case 5: return launch_nt_256(g, epi, st);
    case 6: return launch_nt_320(g, epi, st);
    default: return launch_nt<64, 64, 2>(g, epi, st);
  }
}

// ---------------------------------------------------------------------------------------------
// Deterministic K-sliced C = A . B^T for a very long K against few output tiles (the LM-head dgrad of xroberta.py:1325-1333 /
// xbert.py:680-697: K = the padded vocabulary, 50304, against a [rows, 768] output).  The slices of gridDim.y write fp32 partial
// planes to a workspace with plain stores and ksplit_reduce_kernel sums them IN SLICE ORDER, rounding once to the output type.
// Why not the fp32-atomic merge of EPI_F32_ACC (round 1-3): the order of the atomic adds changes the last bits of the sum from run
// to run, the sum is an ACTIVATION gradient that is rounded to bf16 next, and an element that sits on a rounding boundary then comes
// out one bf16 ulp apart -- a 2e-5 perturbation that the remaining backward (bf16 roundings at every layer) amplifies to 1e-3 of the
// gradient norm (tools/cold_probe.py: 2 of 28 cold runs, both landing on the same second value).  Atomics stay where their sum is a
// final fp32 parameter gradient.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ksplit_reduce_kernel(const float* __restrict__ ws, int slices, long plane, int M, int N, void* __restrict__ out,
                                                            long ldo, int out_bf16) {
  const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 8;  // 8 consecutive columns of one row (N % 8 == 0)
  if (e >= (long)M * N) return;
  const int m = (int)(e / N), n = (int)(e - (long)m * N);
  f32x4 a0 = *reinterpret_cast<const f32x4*>(ws + e), a1 = *reinterpret_cast<const f32x4*>(ws + e + 4);
  for (int s = 1; s < slices; ++s) {
    a0 += *reinterpret_cast<const f32x4*>(ws + (long)s * plane + e);
    a1 += *reinterpret_cast<const f32x4*>(ws + (long)s * plane + e + 4);
  }
  if (out_bf16) {
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[i] = f2bf(a0[i]); o[4 + i] = f2bf(a1[i]); }
    *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16*>(out) + (long)m * ldo + n) = o;
  } else {
    float* op = reinterpret_cast<float*>(out) + (long)m * ldo + n;
    *reinterpret_cast<f32x4*>(op) = a0;
    *reinterpret_cast<f32x4*>(op + 4) = a1;
  }
}

// K-slices for a shape (1 = the plain kernels are the better plan) and the K-tiles per slice
static int ksplit_plan(int M, int N, int K, int* nk_per_out) {
  const int nk_all = K / 64, nk_per = cdiv(nk_all, nt_k_slices(M, N, K));
  *nk_per_out = nk_per;
  return cdiv(nk_all, nk_per);  // slices that own at least one K-tile
}

long xfm_gemm_nt_ksplit_workspace_impl(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  int nk_per;
  const int slices = ksplit_plan(M, N, K, &nk_per);
  return slices > 1 ? (long)slices * M * N * 4 : 0;
}

int xfm_gemm_nt_ksplit_impl(const void* A, long lda, const void* B, long ldb, void* out, long ldo, int out_bf16, const float* bias, int M, int N,
                            int K, float* ws, long ws_bytes, hipStream_t st) {
  XFM_REQUIRE(M > 0 && N > 0 && K > 0 && K % 64 == 0, "gemm_nt_ksplit: bad shape M=%d N=%d K=%d", M, N, K);
  int nk_per;
  const int slices = ksplit_plan(M, N, K, &nk_per);
  if (slices <= 1) return xfm_gemm_nt_impl(A, lda, B, ldb, out, ldo, bias, nullptr, 0, M, N, K, out_bf16 ? EPI_BF16 : EPI_F32, 0, st);
  XFM_REQUIRE(N % 8 == 0 && ldo % 8 == 0 && ((uintptr_t)out % 16) == 0, "gemm_nt_ksplit: N=%d, ldo=%ld must be multiples of 8 and out 16-byte aligned", N, ldo);
  XFM_REQUIRE(lda % 8 == 0 && ldb % 8 == 0 && ((uintptr_t)A % 16) == 0 && ((uintptr_t)B % 16) == 0, "gemm_nt_ksplit: operands must be 16-byte aligned rows");
  XFM_REQUIRE(ws != nullptr && ((uintptr_t)ws % 16) == 0 && ws_bytes >= (long)slices * M * N * 4,
              "gemm_nt_ksplit: workspace of %ld bytes needed (xfm_gemm_nt_ksplit_workspace)", (long)slices * M * N * 4);
  GemmNT g = gemm_nt_args(A, lda, B, ldb, ws, (long)N, bias, M, N, K);
  g.k_splits = slices;
  g.split_stride = (long)M * N;
  // k_splits = the slices that own K-tiles; the kernel re-derives nk_per = ceil(nk_all / k_splits) <= the planned one, under which
  // exactly those slices stay non-empty, so every plane of the workspace is written in full
  XFM_REQUIRE(cdiv(K / 64, cdiv(K / 64, slices)) == slices, "gemm_nt_ksplit: slice plan mismatch");
  int rc = launch_nt<64, 128, 3>(g, EPI_F32, st);
  if (rc != XFM_OK) return rc;
  hipLaunchKernelGGL(ksplit_reduce_kernel, dim3(cdiv((long)M * N / 8, 256)), dim3(256), 0, st, ws, slices, (long)M * N, M, N, out, ldo, out_bf16);
  return xfm_check_launch("ksplit_reduce");
}

// ---------------------------------------------------------------------------------------------
// wgrad: dW[N,K] += dY[M,N]^T . X[M,K]
// Split partials go to the caller's workspace with plain coalesced stores and are summed by a reduce kernel: fp32 atomics
// into dW run at ~0.8 TB/s on this part (28 MB of them cost more than the MFMA loop of a mid-size wgrad).  A single
// split updates dW with plain read-modify-writes.  Atomics remain only when splits > 1 and no workspace was passed.
// ---------------------------------------------------------------------------------------------
static int tn256_plan(int M, int N, int K, int& splits, int& mps) {  // -> number of 256x256 tiles
  const int t256 = (N / 256) * (K / 256);
  splits = 256 / t256;
  const int steps = M / 64;
  if (splits > steps / 8) splits = steps / 8;
  if (splits < 1) splits = 1;
  mps = cdiv(steps, splits) * 64;
  splits = cdiv(M, mps);
  return t256;
}

static bool tn256_eligible(long ldy, long ldx, int M, int N, int K) {
  return M % 64 == 0 && N % 256 == 0 && K % 256 == 0 && N >= 256 && K >= 256 &&
         (unsigned long)M * (unsigned long)(ldy > ldx ? ldy : ldx) < (1ul << 32);
}

// Below this many bytes of split partials the atomics' ~12 us/10 MB beat the extra reduce launch (measured, tools/tune_gemm.py).
#define TN_WS_MIN_BYTES (16l << 20)

static int tn128_plan(int M, int N, int K, int splits_hint, int& splits, int& mps) {  // -> number of 128x128 tiles
  const int tiles = cdiv(N, 128) * cdiv(K, 128);
  splits = splits_hint < 0 ? 0 : splits_hint;
  if (splits <= 0) {
    splits = (432 + tiles / 2) / tiles;        // measured optimum: ~432 workgroups in total (tools/tune_gemm.py)
    int max_splits = M / 480;                  // ... while every split still walks >= ~8 K-steps
    if (max_splits < 2 && M >= 640) max_splits = 2;  // (M = 928, the VQA / retrieval text rows: two splits 15-24 us, one 25-33 us)
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
  }
  mps = cdiv(cdiv(M, splits), 64) * 64;
  splits = cdiv(M, mps);
  return tiles;
}

// Ragged M on an otherwise 256-tileable problem (the 577 / 901-token ViT of the 384 / 480 px configurations: M = B * tokens is no
// multiple of 64): the leading rows run on the 256 x 256 kernel and the last M % 64 rows as a second, single-split call that adds
// into dW -- the 128 x 128 ring kernel on all of M costs 30-40 % more (591 vs 900+ TFLOP/s at M = 21624).
static int tn256_body_rows(int M, int N, int K) {
  const int M0 = M - M % 64;
  // (from 8192 rows: at the fusion tower's packed M ~ 5200 the 7 x 36 workgroups of the 256 x 256 plan walk 12 K-steps each and lose to
  // the ring kernel -- 73 vs 56 us at 5252 x 3072 x 768; round 3 had put those calls here too)
  static const int min_rows = xfm_env_int("XFM_TN256_RAGGED_MIN", 8192);  // A/B knob
  if (M % 64 == 0 || M0 < min_rows || N % 256 != 0 || K % 256 != 0) return 0;
  int splits, mps;
  return tn256_plan(M0, N, K, splits, mps) >= 18 ? M0 : 0;
}

// What one xfm_gemm_tn call launches.  Filled by tn_plan alone; xfm_gemm_tn_workspace, xfm_gemm_tn_plan and xfm_gemm_tn read it.
enum { TN_K256 = 0, TN_KRING = 1, TN_KREG = 2 };         // kernel: gemm_tn_256_kernel, gemm_tn_ring_kernel, gemm_tn_kernel
enum { TN_REDUCE = 0, TN_ATOMIC = 1, TN_DIRECT = 2 };    // merge of the M-splits: workspace planes + reduce kernel | fp32 atomics into dW |
                                                         // one split, plain read-modify-write
struct TnPlan {
  int kernel, merge;
  int tiles, splits, mps;   // output tiles (256x256 or 128x128), M-splits, rows per split
  long ws_bytes;            // workspace the route writes through (0 unless merge == TN_REDUCE)
  int body_rows;            // > 0: ragged M -- the plan is that of the leading body_rows rows; the rest follows as a single-split call
};
constexpr long TN_WS_UNLIMITED = LONG_MAX;
constexpr int TN128_LDS = 4 * 64 * 256, TN256_LDS = 2 * 4 * 64 * 256;   // dynamic LDS of the 128x128 kernels / of the 256x256 pipeline

// splits_hint: 0 = auto, > 0 = that many splits of the 128x128 kernels, -3 forces / -4 forbids the 256x256 kernel, -5 = the
// register-staged 128x128 kernel.  ws_avail: the bytes the caller brought (0: no workspace); a route whose planes do not fit steps
// down -- the ragged split to one call, the 256x256 route to the 128x128 plan, that one to atomics.
static TnPlan tn_plan(int M, int N, int K, long ldy, long ldx, int splits_hint, long ws_avail) {
  if (splits_hint == 0) {
    const int M0 = tn256_body_rows(M, N, K);
    if (M0 > 0 && tn256_eligible(ldy, ldx, M0, N, K) && ws_avail > 0 && ws_avail >= tn_plan(M0, N, K, N, K, 0, TN_WS_UNLIMITED).ws_bytes) {
      TnPlan p = tn_plan(M0, N, K, ldy, ldx, 0, ws_avail);
      p.body_rows = M0;
      return p;
    }
  }
  TnPlan p{};
  // 256 x 256 phase-pipelined kernel: shapes without edges and with enough output tiles
  if (tn256_eligible(ldy, ldx, M, N, K) && splits_hint != -4) {
    p.tiles = tn256_plan(M, N, K, p.splits, p.mps);
    const long need = (long)p.splits * N * K * 4;
    const bool have_ws = ws_avail >= need;
    if (splits_hint == -3 || (splits_hint == 0 && p.tiles >= 18 && M >= 4096 && have_ws)) {
      p.kernel = TN_K256;
      p.merge = have_ws ? TN_REDUCE : TN_ATOMIC;
      p.ws_bytes = have_ws ? need : 0;
      return p;
    }
  }
  static const int ring_env = xfm_env_int("XFM_TN_RING", 1);  // A/B knob
  p.kernel = ring_env && N % 128 == 0 && K % 128 == 0 && splits_hint != -5 ? TN_KRING : TN_KREG;
  p.tiles = tn128_plan(M, N, K, splits_hint, p.splits, p.mps);
  const long need = (long)p.splits * p.tiles * 128 * 128 * 4;
  const bool use_ws = p.splits > 1 && ws_avail >= need && (need >= TN_WS_MIN_BYTES || splits_hint > 0);
  p.merge = use_ws ? TN_REDUCE : p.splits == 1 ? TN_DIRECT : TN_ATOMIC;
  p.ws_bytes = use_ws ? need : 0;
  return p;
}

// Workspace (bytes) xfm_gemm_tn wants for this shape with splits_hint = 0: the split partials of whichever kernel the
// heuristic picks (0 when a single split writes dW directly).
long xfm_gemm_tn_workspace_impl(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return tn_plan(M, N, K, N, K, 0, TN_WS_UNLIMITED).ws_bytes;
}

int xfm_gemm_tn_plan_impl(int M, int N, int K, long ldy, long ldx, int splits_hint, long workspace_bytes, int* kernel, int* splits,
                          long* workspace_used) {
  XFM_REQUIRE(M > 0 && N > 0 && K > 0 && kernel != nullptr && splits != nullptr && workspace_used != nullptr, "gemm_tn_plan: bad arguments");
  const TnPlan p = tn_plan(M, N, K, ldy, ldx, splits_hint, workspace_bytes);
  *kernel = p.kernel;
  *splits = p.splits;
  *workspace_used = p.ws_bytes;
  return XFM_OK;
}

// the launches of a plan over rows [0, M) (M = the plan's body_rows for a ragged split)
static int tn_run(const TnPlan& p, const void* dY, long ldy, const void* X, long ldx, float* dW, long ldw, float* dbias, int M, int N, int K,
                  float* workspace, hipStream_t st) {
  float* ws = p.merge == TN_REDUCE ? workspace : nullptr;
  const GemmTN g{(const bf16*)dY, ldy, (const bf16*)X, ldx, dW, ldw, dbias, M, N, K, p.mps, ws, p.merge == TN_DIRECT ? 1 : 0};
  if (p.kernel == TN_K256) {
    lds_launch<gemm_tn_256_kernel, TN256_LDS>(dim3(p.tiles * p.splits), dim3(512), TN256_LDS, st, g);
    int rc = xfm_check_launch("gemm_tn_256");
    if (rc != XFM_OK || ws == nullptr) return rc;
    const long quads = (long)p.tiles * 8 * 32 * 64;
    hipLaunchKernelGGL(tn_reduce_kernel, dim3((unsigned)cdiv(quads, 256)), dim3(256), 0, st, ws, dW, ldw, K / 256, p.tiles, p.splits);
    return xfm_check_launch("gemm_tn_reduce");
  }
  TnBatch one{};
  one.nb = 1;
  if (p.kernel == TN_KRING) lds_launch<gemm_tn_ring_kernel, TN128_LDS>(dim3(p.tiles * p.splits), dim3(256), TN128_LDS, st, g, one);
  else lds_launch<gemm_tn_kernel, TN128_LDS>(dim3(p.tiles * p.splits), dim3(256), TN128_LDS, st, g);
  int rc = xfm_check_launch("gemm_tn");
  if (rc != XFM_OK || ws == nullptr) return rc;
  const long quads = (long)p.tiles * 4 * 16 * 64;
  hipLaunchKernelGGL(tn_reduce128_kernel, dim3((unsigned)cdiv(quads, 256)), dim3(256), 0, st, ws, dW, ldw, N, K, cdiv(K, 128), p.tiles, p.splits,
                     one);
  return xfm_check_launch("gemm_tn_reduce128");
}

int xfm_gemm_tn_impl(const void* dY, long ldy, const void* X, long ldx, float* dW, long ldw, float* dbias, int M, int N, int K,
                     int splits_hint, float* workspace, long workspace_bytes, hipStream_t st) {
  XFM_REQUIRE(M > 0 && N > 0 && K > 0, "gemm_tn: empty problem M=%d N=%d K=%d", M, N, K);
  XFM_REQUIRE(K % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0, "gemm_tn: K=%d ldx=%ld ldy=%ld must be multiples of 8", K, ldx, ldy);
  XFM_REQUIRE(((uintptr_t)dY % 16) == 0 && ((uintptr_t)X % 16) == 0, "gemm_tn: operands must be 16-byte aligned");
  const TnPlan p = tn_plan(M, N, K, ldy, ldx, splits_hint, workspace != nullptr ? workspace_bytes : 0);
  if (p.body_rows == 0) return tn_run(p, dY, ldy, X, ldx, dW, ldw, dbias, M, N, K, workspace, st);
  const int M0 = p.body_rows;
  int rc = tn_run(p, dY, ldy, X, ldx, dW, ldw, dbias, M0, N, K, workspace, st);
  if (rc != XFM_OK) return rc;
  return xfm_gemm_tn_impl((const bf16*)dY + (long)M0 * ldy, ldy, (const bf16*)X + (long)M0 * ldx, ldx, dW, ldw, dbias, M - M0, N, K, 1, workspace,
                          workspace_bytes, st);
}

// nb (<= TN_BATCH_MAX) weight gradients of one shape and one set of leading dimensions in ONE launch of the ring kernel + ONE reduce.
// Falls back to nb plain calls when the shape is not the ring kernel's (N, K multiples of 128) or the workspace is too small.
struct TnBatchPlan {
  int tiles, splits, mps;   // splits == 0: not a shape of the batched launch
  long ws_bytes;            // nb problems' split planes
};
static TnBatchPlan tn_batch_plan(int nb, int M, int N, int K) {
  TnBatchPlan p{cdiv(N, 128) * cdiv(K, 128), 0, M, 0};
  if (nb < 2 || nb > TN_BATCH_MAX || M <= 0 || N <= 0 || K <= 0 || N % 128 != 0 || K % 128 != 0) return p;
  int hint = (432 + nb * p.tiles / 2) / (nb * p.tiles);  // ~432 workgroups in total, as for a single problem
  hint = hint < 1 ? 1 : hint;
  tn128_plan(M, N, K, hint, p.splits, p.mps);
  p.ws_bytes = (long)nb * p.splits * p.tiles * 128 * 128 * 4;
  return p;
}
long xfm_gemm_tn_batch_workspace_impl(int nb, int M, int N, int K) {
  if (nb <= 0 || M <= 0 || N <= 0 || K <= 0) return 0;
  const long single = xfm_gemm_tn_workspace_impl(M, N, K), need = tn_batch_plan(nb, M, N, K).ws_bytes;
  return need > single ? need : single;
}
int xfm_gemm_tn_batch_impl(int nb, const void* const* dY, long ldy, const void* const* X, long ldx, float* const* dW, long ldw,
                           float* const* dbias, int M, int N, int K, float* workspace, long workspace_bytes, hipStream_t st) {
  XFM_REQUIRE(nb >= 1 && dY != nullptr && X != nullptr && dW != nullptr, "gemm_tn_batch: bad arguments");
  const TnBatchPlan p = tn_batch_plan(nb, M, N, K);
  bool batched = p.splits > 1 && ldx % 8 == 0 && ldy % 8 == 0 && workspace != nullptr && workspace_bytes >= p.ws_bytes;
  for (int i = 0; i < nb && batched; ++i) batched = ((uintptr_t)dY[i] % 16) == 0 && ((uintptr_t)X[i] % 16) == 0;
  if (!batched) {
    for (int i = 0; i < nb; ++i) {
      int rc = xfm_gemm_tn_impl(dY[i], ldy, X[i], ldx, dW[i], ldw, dbias ? dbias[i] : nullptr, M, N, K, 0, workspace, workspace_bytes, st);
      if (rc != XFM_OK) return rc;
    }
    return XFM_OK;
  }
  TnBatch bt{};
  bt.nb = nb;
  bt.wg_per = p.tiles * p.splits;
  bt.ws_stride = (long)p.splits * p.tiles * 128 * 128;
  for (int i = 0; i < nb; ++i) {
    bt.dY[i] = (const bf16*)dY[i];
    bt.X[i] = (const bf16*)X[i];
    bt.dW[i] = dW[i];
    bt.dbias[i] = dbias ? dbias[i] : nullptr;
  }
  const GemmTN g{bt.dY[0], ldy, bt.X[0], ldx, bt.dW[0], ldw, bt.dbias[0], M, N, K, p.mps, workspace, 0};
  lds_launch<gemm_tn_ring_kernel, TN128_LDS>(dim3(nb * p.tiles * p.splits), dim3(256), TN128_LDS, st, g, bt);
  int rc = xfm_check_launch("gemm_tn_batch");
  if (rc != XFM_OK) return rc;
  const long quads = (long)p.tiles * 4 * 16 * 64;
  hipLaunchKernelGGL(tn_reduce128_kernel, dim3((unsigned)cdiv(quads, 256), nb), dim3(256), 0, st, workspace, bt.dW[0], ldw, N, K, cdiv(K, 128),
                     p.tiles, p.splits, bt);
  return xfm_check_launch("gemm_tn_batch_reduce");
}

// Any number of weight gradients over the SAME M rows (all the projections of the layers whose dY are still alive) -> persistent
// grouped launches of gemm_tn_group_kernel, TN_GROUP_MAX problems each.  Problems the 256 x 256 pipeline does not take (N or K not a
// multiple of 256, fewer than 1024 rows) go through xfm_gemm_tn one by one.
static int tn_group_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    n = n / 8 * 8 > 0 ? n / 8 * 8 : 8;
  }
  return n;
}
static bool tn_group_item_ok(const xfm_tn_item& it, int M) {   // (any M from 1024 rows: the kernel zero-fills a short last K-step)
  return M >= 1024 && it.N % 256 == 0 && it.K % 256 == 0 && it.N >= 256 && it.K >= 256 && it.ldy % 8 == 0 && it.ldx % 8 == 0 &&
         (unsigned long)(M + 64) * (unsigned long)(it.ldy > it.ldx ? it.ldy : it.ldx) < (1ul << 32) && ((uintptr_t)it.dY % 16) == 0 &&
         ((uintptr_t)it.X % 16) == 0;
}
static void tn_group_plan(int tiles, int nk, int G, int& full, int& sk_wgs, long& R) {
  full = tiles / G * G;
  // a last round that is at least 90 % full runs as whole tiles too: cutting it would even out the last 10 % of one round at the price
  // of two partial planes + a fix-up pass for every tile of it (the fusion tower: 1512 tiles = 5 rounds + 232)
  if ((tiles - full) * 10 >= G * 9) full = tiles;
  R = (long)(tiles - full) * nk;
  sk_wgs = 0;
  if (R > 0) {
    const long m = R / 16;   // >= 16 K-steps per workgroup: pieces stay >= 4 steps after the boundaries snap to tile edges
    sk_wgs = (int)(m < G ? m : G);
    if (sk_wgs < 1) sk_wgs = 1;
  }
}
long xfm_gemm_tn_group_workspace_impl(int n, const xfm_tn_item* items, int M) {
  if (n <= 0 || items == nullptr || M <= 0) return 0;
  const int G = tn_group_cus();
  long need = 0;
  int tiles = 0, np = 0;
  auto close = [&]() {
    if (np == 0) return;
    int full, sk;
    long R;
    tn_group_plan(tiles, cdiv(M, 64), G, full, sk, R);
    const long b = sk > 1 ? 2l * sk * (256 * 256 + 256) * 4 : 0;   // two partial-piece slots per sharing workgroup (tile + column sums)
    need = b > need ? b : need;
    tiles = np = 0;
  };
  for (int i = 0; i < n; ++i) {
    const xfm_tn_item& it = items[i];
    if (tn_group_item_ok(it, M)) {
      tiles += (it.N / 256) * (it.K / 256);
      if (++np == TN_GROUP_MAX) close();
    } else {
      const long b = xfm_gemm_tn_workspace_impl(M, it.N, it.K);
      need = b > need ? b : need;
    }
  }
  close();
  return need;
}
int xfm_gemm_tn_group_impl(int n, const xfm_tn_item* items, int M, float* workspace, long workspace_bytes, hipStream_t st) {
  XFM_REQUIRE(n >= 0 && (n == 0 || items != nullptr) && M > 0, "gemm_tn_group: bad arguments");
  XFM_REQUIRE(workspace_bytes >= xfm_gemm_tn_group_workspace_impl(n, items, M) && (workspace != nullptr || workspace_bytes == 0),
              "gemm_tn_group: workspace smaller than xfm_gemm_tn_group_workspace()");
  const int G = tn_group_cus();
  TnGroup g{};
  g.nk = cdiv(M, 64);
  g.M = M;
  g.ws = workspace;
  auto flush = [&]() -> int {
    if (g.nprob == 0) return XFM_OK;
    tn_group_plan(g.total_tiles, g.nk, G, g.full_tiles, g.sk_wgs, g.sk_iters);
    g.ws_bias = g.ws != nullptr ? g.ws + 2l * g.sk_wgs * 256 * 256 : nullptr;
    const int grid = g.full_tiles > 0 ? G : g.sk_wgs;
    lds_launch<gemm_tn_group_kernel, TN256_LDS>(dim3(grid), dim3(512), TN256_LDS, st, g);
    int rc = xfm_check_launch("gemm_tn_group");
    if (rc == XFM_OK && g.sk_wgs > 1) {
      hipLaunchKernelGGL(tn_group_fixup_kernel, dim3(64, g.total_tiles - g.full_tiles), dim3(256), 0, st, g);
      rc = xfm_check_launch("gemm_tn_group_fixup");
    }
    g.nprob = g.total_tiles = 0;
    return rc;
  };
  for (int i = 0; i < n; ++i) {
    const xfm_tn_item& it = items[i];
    XFM_REQUIRE(it.dY && it.X && it.dW && it.N > 0 && it.K > 0, "gemm_tn_group: bad problem %d", i);
    if (!tn_group_item_ok(it, M)) continue;
    TnGroupProb& P = g.p[g.nprob++];
    P.dY = (const bf16*)it.dY; P.X = (const bf16*)it.X; P.dW = it.dW; P.dbias = it.dbias;
    P.ldy = (unsigned)it.ldy; P.ldx = (unsigned)it.ldx; P.ldw = it.ldw;
    P.tiles_k = it.K / 256;
    g.total_tiles += (it.N / 256) * (it.K / 256);
    P.tile_end = g.total_tiles;
    if (g.nprob == TN_GROUP_MAX) {
      const int rc = flush();
      if (rc != XFM_OK) return rc;
    }
  }
  int rc = flush();
  if (rc != XFM_OK) return rc;
  for (int i = 0; i < n; ++i) {   // what the grouped kernel did not take
    const xfm_tn_item& it = items[i];
    if (!tn_group_item_ok(it, M))
      rc = xfm_gemm_tn_impl(it.dY, it.ldy, it.X, it.ldx, it.dW, it.ldw, it.dbias, M, it.N, it.K, 0, workspace, workspace_bytes, st);
    if (rc != XFM_OK) return rc;
  }
  return XFM_OK;
}
