/* libxfm_hip.so -- C ABI of the MI355X-native XFM transformer forward/backward hot path.
 *
 * Every entry point returns 0 on success or a negative XFM_E_* code; the message is available from
 * xfm_last_error() (thread local).  No entry point allocates, synchronises the device or throws: the caller owns
 * all device memory (PyTorch's caching allocator in the shipped binding), passes plain device pointers, element
 * strides and a hipStream_t (as void*), and every kernel is enqueued on that stream only, so calls are re-entrant
 * per stream and hipGraph-capturable.  There is no global mutable state.
 *
 * The reference has no FFI for this path (it bottoms out in stock ATen ops); each symbol below
 * cites the Python code whose arithmetic it replaces.  bf16 tensors are row-major uint16 payloads.
 */
#ifndef XFM_HIP_H
#define XFM_HIP_H
#include <stdint.h>

#ifdef XFM_INTERNAL_BF16
typedef __bf16 xfm_bf16;
#else
typedef uint16_t xfm_bf16;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define XFM_OK 0
#define XFM_E_ARG (-1)
#define XFM_E_LAUNCH (-2)
#define XFM_E_UNSUPPORTED (-3)

#define XFM_ABI_VERSION 20

const char* xfm_last_error(void);
int xfm_abi_version(void);

/* ---- Linear layers (torch.nn.Linear / F.linear call sites: beit2.py:131,162,64-68,229; xroberta.py:211,224-234,
 * 301,368,382,1326,1331; xfm.py:117-120,617-620) ------------------------------------------------------------------ */
enum { XFM_EPI_BF16 = 0, XFM_EPI_F32 = 1, XFM_EPI_GELU = 2, XFM_EPI_DGELU = 3, XFM_EPI_F32_ACC = 4 };

/* C[M,N] = A[M,K] . B[N,K]^T + bias.  A, B bf16 (K contiguous).  Epilogues: bf16 out | fp32 out |
 * C = gelu(x), aux = gelu'(x) (bf16; x = the bf16-rounded pre-activation)  | C = acc * aux (the GELU dgrad, aux from the
 * forward) | fp32 C += acc.  K % 64 == 0; lda, ldb % 8 == 0.
 * tile_hint: 0 = auto, 1 = 128x128, 2 = 64x128, 3 = 64x64, 4 = 256x128 with a 3-slot LDS ring, 5 = 256x256 phase pipeline
 * (large M), 6 = 320x256 one-round tile, 7 = 64x128 with 3 LDS stages, 8 = 64x64 with 4 (few workgroups, long K).
 * 6 is never picked automatically: it is for a tall M whose 256x256 tiles spill into a nearly empty second round (25216 x 768: 297 tiles
 * on 256 CUs, 237 of 320x256), one workgroup per tile, results bit-identical to 5.  It needs N % 256 == 0, at most one tile per CU and
 * operands inside 32-bit element offsets; a call that is not such a shape (or any call under XFM_GEMM_NT320=0) runs as tile_hint 0. */
int xfm_gemm_nt(const xfm_bf16* A, long lda, const xfm_bf16* B, long ldb, void* C, long ldc, const float* bias,
                xfm_bf16* aux, long ldaux, int M, int N, int K, int epilogue, int tile_hint, void* stream);

/* The launch plan xfm_gemm_nt follows for a shape (profilers / benchmarks attribute a call to its kernels with it): *cfg = tile
 * configuration (the tile_hint numbering), *rows_a > 0 = tail split: the leading rows_a rows run as whole rounds of 256x256 tiles
 * (configuration 5), the remaining rows are planned again with tile_hint -1.  This is the plan of tight operands (lda = ldb = K):
 * configuration 5 addresses its operands with 32-bit element offsets, so a call whose M * lda or N * ldb reaches 2^32 runs
 * configuration 1 wherever this plan says 5 for tile_hint 0 or for the tail split; an explicit tile_hint 5 is then an error. */
int xfm_gemm_nt_plan(int M, int N, int K, int epilogue, int tile_hint, int* cfg, int* rows_a);

/* out[M,N] = A[M,K] . B[N,K]^T (+ bias) for a very long K against few output tiles -- the activation gradient of the vocabulary
 * projection (RobertaLMHead.decoder, xroberta.py:1325-1333; BertLMPredictionHead.decoder, xbert.py:680-697: K = the padded vocabulary).
 * K is sliced over the grid; the slices' fp32 partial planes go to `workspace` (xfm_gemm_nt_ksplit_workspace bytes; 0 = the shape
 * runs unsliced and needs none) and are summed in slice order by a second kernel that rounds once to the output type
 * (out_bf16 != 0: bf16, else fp32): bit-reproducible, unlike the fp32-atomic merge of XFM_EPI_F32_ACC.  Sliced shapes need
 * N % 8 == 0 and ldo % 8 == 0. */
long xfm_gemm_nt_ksplit_workspace(int M, int N, int K);
int xfm_gemm_nt_ksplit(const xfm_bf16* A, long lda, const xfm_bf16* B, long ldb, void* out, long ldo, int out_bf16, const float* bias,
                       int M, int N, int K, float* workspace, long workspace_bytes, void* stream);

/* dW[N,K] (fp32) += dY[M,N]^T . X[M,K]   (weight gradient, split over M).
 * dbias (optional, fp32 [N]) += column sums of dY: the bias gradient rides along in the same pass over dY.
 * The split partials are written to `workspace` (xfm_gemm_tn_workspace bytes for splits_hint 0; may be 0) and summed
 * in a fixed order by a reduce kernel; a single split updates dW in place; only splits without a workspace fall back to
 * fp32 atomics.  Large edge-free shapes (M % 64 == 0; N, K % 256 == 0) run on a 256x256 pipelined kernel.
 * splits_hint: 0 = auto, > 0 = that many splits of the 128x128 kernel; the kernel A/B switches -3 = the 256x256 kernel wherever the
 * shape allows it, -4 = never the 256x256 kernel, -5 = the register-staged 128x128 kernel instead of the ring kernel.
 * A workspace smaller than the route needs is not an error: the 256x256 route steps down to the 128x128 plan, and that one to atomics.
 * xfm_gemm_tn_workspace and xfm_gemm_tn read ONE plan (xfm_gemm_tn_plan): the query is the plan of (M, N, K, ldy = N, ldx = K,
 * splits_hint 0) with no limit on the workspace. */
long xfm_gemm_tn_workspace(int M, int N, int K);
int xfm_gemm_tn(const xfm_bf16* dY, long ldy, const xfm_bf16* X, long ldx, float* dW, long ldw, float* dbias, int M, int N,
                int K, int splits_hint, float* workspace, long workspace_bytes, void* stream);
/* The plan xfm_gemm_tn follows for these arguments and a workspace of workspace_bytes (LONG_MAX: whatever it wants; 0: none) -- for
 * sizing the workspace of a call with a splits_hint, and for attributing a call to its kernels as with xfm_gemm_nt_plan (ABI 12).
 * *kernel: 0 = 256x256 pipeline, 1 = 128x128 ring, 2 = 128x128 register-staged; *splits = M-splits; *workspace_used = the bytes the
 * route writes through (0: one split in place, or atomics).  For a ragged M that runs as 256x256 body + last M % 64 rows the plan is
 * the body's; the rest is one more single-split 128x128 launch and needs no workspace. */
int xfm_gemm_tn_plan(int M, int N, int K, long ldy, long ldx, int splits_hint, long workspace_bytes, int* kernel, int* splits,
                     long* workspace_used);
/* nb (1..4) weight gradients of ONE shape (same M, N, K and leading dimensions; host arrays of device pointers; dbias / its entries may be
 * NULL) as one launch + one reduce -- the three 768 x 768 projections of a RobertaLayer with cross-attention (xroberta.py:201-304).  Falls
 * back to nb xfm_gemm_tn calls when N or K is not a multiple of 128 or the workspace is smaller than xfm_gemm_tn_batch_workspace(). */
long xfm_gemm_tn_batch_workspace(int nb, int M, int N, int K);
int xfm_gemm_tn_batch(int nb, const void* const* dY, long ldy, const void* const* X, long ldx, float* const* dW, long ldw,
                      float* const* dbias, int M, int N, int K, float* workspace, long workspace_bytes, void* stream);

/* Any number of weight gradients over the SAME M rows in persistent grouped launches (the deferred weight gradients of a whole tower:
 * every wgrad of one ViT block has 9-36 output tiles of 256 x 256 and needs 7 M-splits, partial planes and a reduce to fill the chip; the
 * tiles of all blocks together are walked whole, one owner per dW element, and only the last total % CUs tiles are cut stream-K
 * style and fixed up in workgroup order -- deterministic).  `items` is HOST memory.  Any M from 1024 rows (a short last K-step is
 * staged as zeros); problems with N or K not a multiple of 256 (or fewer rows) run through xfm_gemm_tn. */
typedef struct {
  const xfm_bf16* dY; long ldy;   /* [M, N] */
  const xfm_bf16* X; long ldx;    /* [M, K] */
  float* dW; long ldw;            /* [N, K] += */
  float* dbias;                   /* optional [N] += column sums of dY */
  int N, K;
} xfm_tn_item;
long xfm_gemm_tn_group_workspace(int n, const xfm_tn_item* items, int M);
int xfm_gemm_tn_group(int n, const xfm_tn_item* items, int M, float* workspace, long workspace_bytes, void* stream);

/* fp32 master weight [N,K] -> bf16 copy wb[N,ldb] and/or transposed bf16 copy wt[K,ldt] (zero padded). */
int xfm_cast_transpose(const float* w, int N, int K, xfm_bf16* wb, long ldb, xfm_bf16* wt, long ldt, void* stream);

/* The same for a table of weights in one launch.  `items` is DEVICE memory, sorted by tile_start; item i covers the 64x64
 * tiles [tile_start, tile_start + tiles_x * tiles_y) with tiles_x = ceil(max(K, ldb if wb) / 64), tiles_y = ceil(max(N, ldt
 * if wt) / 64) (the padded extents, so the zero padding is rewritten too); total_tiles = the sum. */
typedef struct {
  const float* w;
  xfm_bf16* wb;
  xfm_bf16* wt;
  long ldb, ldt;
  int N, K;
  int tiles_x, reserved;
  long tile_start;
} xfm_cast_item;
int xfm_cast_transpose_batch(const xfm_cast_item* items, int n_items, long total_tiles, void* stream);

/* out[n] += sum_m Y[m,n]  (bias gradients).  workspace >= xfm_colsum_workspace(M,N) bytes. */
long xfm_colsum_workspace(int M, int N);
int xfm_colsum(const xfm_bf16* Y, long ldy, int M, int N, float* out, float* workspace, long workspace_bytes,
               void* stream);

/* ---- LayerNorm family (nn.LayerNorm call sites: beit2.py:191-206,460; xroberta.py:300-304,381-385,1329;
 * xfm.py:118).  Width D in {256,512,768,1024,1536}. ---------------------------------------------------------------- */
enum { XFM_LN_PLAIN = 0, XFM_LN_POST = 1, XFM_LN_LS = 2 };

typedef struct {
  const float* x32;        /* PLAIN: fp32 input | LS: residual stream in */
  const xfm_bf16* x16;     /* PLAIN: bf16 input */
  const xfm_bf16* h;       /* POST / LS: output of the producing GEMM (bias included) */
  const xfm_bf16* res;     /* POST: residual */
  const float* ls_gamma;   /* LS: layer-scale gamma_1 / gamma_2 */
  const float* row_scale;  /* LS: per-sample drop-path scale [rows / rows_per_sample] or NULL */
  const float* w; const float* b;
  float* x_out;            /* LS: residual stream out (may alias x32) */
  xfm_bf16* z_out;         /* POST: pre-norm sum saved for backward */
  xfm_bf16* y;             /* normalised output */
  float* y32;              /* optional fp32 copy of y */
  float* mean; float* rstd;
  int rows, rows_per_sample;
  float eps;
  uint32_t drop_thresh; float drop_scale; uint32_t seed_lo, seed_hi;  /* POST: dropout on h (thresh = p * 2^32) */
  int gelu;                /* y = GELU(LN(..)): the Linear -> LayerNorm -> GELU heads (xfm.py:115-121, model_classification.py:33-48) */
  const float* res32;      /* POST: the residual in fp32 (replaces `res`): the un-rounded output of the previous LayerNorm -- the reference's
                              autocast keeps LayerNorm outputs and the residual sum in fp32 (xroberta.py:300-304, 381-385) */
  float* z32_out;          /* POST: the pre-norm sum in fp32 for the backward (z_out may then be NULL) */
} xfm_ln_fwd_args;

typedef struct {
  const xfm_bf16* dy1; const xfm_bf16* dy2; const float* dy32;  /* gradients w.r.t. y, summed on load (NULL ok) */
  const float* x32; const xfm_bf16* x16;                        /* the tensor that was normalised */
  const float* mean; const float* rstd; const float* w;
  float* dx32; xfm_bf16* dx16; int dx_accum;                     /* PLAIN: gradient w.r.t. the input */
  xfm_bf16* dh; xfm_bf16* dres;                                  /* POST / LS: to the producing GEMM / residual */
  float* dstream;                                                /* LS: in/out fp32 residual-stream gradient */
  const xfm_bf16* h; const float* ls_gamma; const float* row_scale;
  float* partial;                                                /* set by the library (workspace) */
  int rows, rows_per_sample;
  uint32_t drop_thresh; float drop_scale; uint32_t seed_lo, seed_hi;
  const float* gelu_b;     /* non-NULL: the forward applied GELU after the affine; this is the LayerNorm bias (the pre-activation
                              xhat * w + b is rebuilt and dy is multiplied by gelu'(.) first) */
  struct xfm_reduce_item_s* defer;  /* non-NULL: do NOT launch the column-sum reduce; describe it here instead.  The caller keeps `workspace`
                              untouched until it has run the item through xfm_reduce_sets_batch (one launch for a whole tower's LayerNorms
                              instead of one 7-us kernel behind each of them on the activation-gradient chain) */
  float* dres32;           /* POST: the gradient of the residual branch in fp32 (the next LayerNorm backward up the stream takes it as
                              dy32); `dres` may then be NULL */
} xfm_ln_bwd_args;

/* out[s][c] += sum over the nblocks rows of partial[s][.][c], s < nset: the deferred second half of xfm_layernorm_bwd. */
typedef struct xfm_reduce_item_s {
  const float* partial;    /* [nset][nblocks][D]; scratch the reduce may overwrite (an item split over row groups parks the groups' sums in
                              it and adds them in group order: no float atomics between the groups, bit-reproducible sums) */
  float* out[4];           /* NULL = skip the set */
  int nblocks, D, nset, reserved;
} xfm_reduce_item;
/* n items (HOST array) in launches of up to 56; the same sums, in the same order, as the per-call reduce. */
int xfm_reduce_sets_batch(int n, const xfm_reduce_item* items, void* stream);

int xfm_layernorm_fwd(const xfm_ln_fwd_args* a, int D, int mode, void* stream);
long xfm_layernorm_bwd_workspace(int rows, int D, int mode);
/* dgamma/dbeta (LN affine), dbias (column sums of dh: bias grad of the producing Linear), dls (layer-scale grad):
 * fp32 [D], accumulated (+=); NULL skips. */
int xfm_layernorm_bwd(const xfm_ln_bwd_args* a, int D, int mode, float* dgamma, float* dbeta, float* dbias, float* dls,
                      float* workspace, long workspace_bytes, void* stream);

/* ---- Attention, head_dim 64 (beit2.py:126-166; xroberta.py:201-289; causal mask xroberta.py:772-792) ------------- */
typedef struct {
  const xfm_bf16* q; long q_rs;   /* element (b,s,h,d) at ptr[(b*S + s)*rs + h*64 + d] */
  const xfm_bf16* k; long k_rs;
  const xfm_bf16* v; long v_rs;
  xfm_bf16* o; long o_rs;
  float* lse;                     /* [B,H,stat_ld] log-sum-exp of the final scores */
  const float* bias; long bias_ld;/* dense additive bias [H,Sq,bias_ld] or NULL */
  const int* key_keep;            /* [B,Sk] 1 attend / 0 padded (adds -10000) or NULL */
  int B, H, Sq, Sk;
  float scale; int causal;
  uint32_t drop_thresh; float drop_scale; uint32_t seed_lo, seed_hi;
  const xfm_bf16* dout; long do_rs;
  xfm_bf16* dq; long dq_rs; xfm_bf16* dk; long dk_rs; xfm_bf16* dv; long dv_rs;
  float* delta;                   /* [B,H,stat_ld] scratch */
  float* dbias;                   /* [H,Sq,bias_ld] fp32, += over the batch, or NULL */
  long stat_ld;                   /* row stride of lse / delta ([B,H,stat_ld]): multiple of 4, >= Sq */
  const float* bias_t; long bias_t_ld; /* optional transposed copy of bias [H,Sk,bias_t_ld] (vector loads in dK/dV) */
  const int* kv_index;            /* optional [B]: query batch row b reads keys/values (and key_keep) of source kv_index[b];
                                     dk/dv stay per query row (fold them with xfm_rows_index_sum) */
  /* optional GROUPED mode (Sq <= 64, no bias / causal / kv_index; Sk > 256 streams the keys through LDS): group g = query batch rows
     grp_rows[grp_start[g] .. grp_start[g+1]) and reads key/value source g (k, v, key_keep have n_groups batch entries).
     One workgroup per (source, head) keeps K/V LDS-resident for all of its rows; dk/dv are summed over the group and
     written per SOURCE ([n_groups*Sk] rows). */
  const int* grp_start; const int* grp_rows; int n_groups;
  /* optional PACKED (unpadded) token rows: batch entry b's queries are rows q_start[b] .. q_start[b] + q_len[b] (q_len[b] in
     [1, Sq]) of q / o / dout / dq, its keys rows k_start[b] .. + k_len[b] of k / v / dk / dv; NULL = dense b * S rows.  Sq / Sk
     stay the padded lengths (grids, statistics [B,H,stat_ld], dropout counters).  Keys past k_len get probability exactly 0,
     what the reference's additive -10000 mask yields in fp32 for a prefix-masked batch (xroberta.py:751-807), so no key_keep
     is needed.  Rows of o / o_lo / dq / dk / dv outside every sequence are not written, and neither are columns [q_len[b], stat_ld)
     of entry b's rows of lse / delta: the forward stores no statistic there, and whatever the backward finds there (it may load
     those columns) reaches no output.  The causal mask and key_keep apply on an entry's local indices (key_keep rows keep the
     padded stride Sk).  No bias, no kv_index in this mode; in grouped mode only the query side may be packed: k_start / k_len
     with grp_start is rejected (XFM_E_ARG), the sources' keys are the dense rows g * Sk .. + Sk. */
  const int* q_start; const int* q_len; const int* k_start; const int* k_len;
  /* xfm_attn_bwd only: 0 = both kernels; 1 = the dQ kernel alone (writes dq and the row statistics `delta`); 2 = the dK/dV kernel
     alone (reads the `delta` a phase-1 call left) -- lets a caller put dK/dV, which in cross-attention only feed weight gradients,
     on another stream than the activation-gradient chain. */
  int bwd_phase;
  /* optional second half of the output, o_lo = bf16(O - bf16(O)) (same addressing as o): the forward writes it when non-NULL; the
     backward then takes the softmax-gradient row term delta_i = sum_j P_ij dP_ij = dO_i . O_i from dO . (o + o_lo) in its prologue
     (error ~2^-17 |dO||O| plus the forward's own bf16 rounding of P, below the bf16 noise of dS) instead of recomputing it in a
     first pass over the keys -- two of the dQ kernel's five matrix products.  NULL = the exact two-pass form. */
  xfm_bf16* o_lo;
  /* optional copies of `bias` in the MFMA accumulator layout (xfm_bias_tile), used by the batch-walking kernels of the 224-px ViT
     shape (Sq == Sk <= 224, no mask / dropout): bias_tiled for the forward, bias_t_tiled (tiles of the transposed bias) for the
     backward.  One bias tile is then one contiguous 1-KB wave load instead of 16 strided row segments.  NULL = read `bias` /
     `bias_t`. */
  const float* bias_tiled; const float* bias_t_tiled;
  /* xfm_attn_bwd with dbias on a problem too long for the in-register bias-gradient kernels (Sk > 256: the 577 / 901 tokens of the
     384 / 480 px ViT, beit2.py:126-166): optional fp32 workspace [B,H,Sq,bias_ld].  The dQ kernel then STORES every batch entry's dS
     there (coalesced 16-byte stores) and a second kernel adds the sum over the batch to dbias -- instead of one float atomic per
     score and batch entry (234 M atomics per layer at B = 24, 901 tokens: 3.1 ms; with the workspace 0.6 ms).  NULL = atomics. */
  float* dbias_ws;
} xfm_attn_args;

int xfm_attn_fwd(const xfm_attn_args* a, void* stream);
int xfm_attn_bwd(const xfm_attn_args* a, void* stream);
/* bytes of `dbias_ws` an xfm_attn_bwd call with these arguments wants (0: none): the planes of [H, Sq, bias_ld] floats of the route
 * that the call's backward plan picks (csrc/attention.hip, attn_bwd_plan -- the dispatcher runs the same plan, and uses a workspace
 * only where this function asks for one).  Long dense unmasked problems with a bias gradient (Sk > 256: the 577 / 901 tokens of the
 * 384 / 480 px ViT) sum dS over the batch inside a kernel that walks the batch entries of a slice with a 128 x 128 block of the
 * gradient in registers: one plane per slice when there is more than one (a few MB), folded into dbias in slice order by a second
 * kernel.  The general kernels (masked / dropped problems, Sk > 256) take the B planes described at xfm_attn_args.dbias_ws.  Short
 * problems (Sk <= 256) want none, or with XFM_DETERMINISTIC=1 one plane per batch slice of the short dQ kernel.  A workspace that
 * is NULL, or whose bias rows (bias_ld) reach past the last 64-key chunk, is not used: atomics, or one slice. */
long xfm_attn_bwd_workspace(const xfm_attn_args* a);
/* dense additive bias [H,S,ld] (fp32) -> two tiled copies, each [H][T][T][64 lanes][4] floats with T = ceil(S / 16), pre-divided by
 * `scale` (the kernels start the score accumulators from bias / scale):
 *   tiled  [h][a][b][lane][r] = bias[h][16a + (lane & 15)][16b + 4 (lane >> 4) + r] / scale        (query on the lane: forward)
 *   tiled_t[h][a][b][lane][r] = bias[h][16b + 4 (lane >> 4) + r][16a + (lane & 15)] / scale        (key on the lane:   backward)
 * Entries whose key is past S hold -1e30 (probability 0), entries whose query is past S hold 0.  tiled_t has T + 1 key-tile rows
 * ([H][T+1][T][64][4]): the last one is all -1e30, for a kernel wave whose second key tile lies past the sequence.  Either output may be
 * NULL. */
int xfm_bias_tile(const float* bias, int H, int S, long ld, float scale, float* tiled, float* tiled_t, void* stream);
/* dense[h,i,j] = table[index[i*N+j]*H + h] (beit2.py:139-145), rows padded to ld (dense_t: optional [h,j,i] copy);
 * and its scatter-add gradient. */
/* dst[u,:] = sum_{r: index[r]==u} src[r,:]  (bf16 rows of `len` elements, fp32 accumulation). */
int xfm_rows_index_sum(const xfm_bf16* src, const int* index, int R, int U, long len, xfm_bf16* dst, void* stream);
int xfm_relpos_gather(const float* table, const int* index, int H, int N, long ld, float* dense, float* dense_t,
                      void* stream);
int xfm_relpos_scatter(const float* ddense, const int* index, int H, int N, long ld, float* dtable, void* stream);
/* the same gradient for the standard index of a G x G patch grid + cls token (N = G*G + 1 tokens, (2G-1)^2 + 3 table rows,
 * beit2.py:92-116): coalesced reads along the grid's structure, one owner per table entry (no atomics, no sort).  dtable += . */
int xfm_relpos_grid_grad(const float* ddense, int H, int G, long ld, float* dtable, void* stream);
/* the same gradient without atomics: order = positions i*N+j sorted by index[i*N+j], start = [entries+1] offsets into order */
int xfm_relpos_scatter_sorted(const float* ddense, const int* order, const int* start, int entries, int H, int N, long ld,
                              float* dtable, void* stream);

/* ---- Patch gather for the patch-embed GEMM (beit2.py:224-230) --------------------------------------------------- */
int xfm_patchify(const float* image, int B, int C, int H, int W, int P, xfm_bf16* out, void* stream);

/* ---- ViT token assembly (beit2.py:432-446: mask-token mix `x * (1 - w) + mask_token * w`, then cat(cls, x)) ----------------
 * x0[b] = [cls | tok[b mod Bt], masked patches (mask[b, i] != 0) replaced by mask_token], fp32 [Bx, P + 1, D]; Bx a multiple
 * of Bt (several masked views of the same patch-embedded images), mask [Bx, P] bytes or NULL.
 * bwd: dtok [Bt, P, D] is written (sum over the views that kept the patch); dcls [D] and dmask_token [D] are accumulated. */
int xfm_vit_tokens_fwd(const float* tok, const float* cls, const float* mask_token, const uint8_t* mask, int Bt, int Bx, int P,
                       int D, float* x0, void* stream);
int xfm_vit_tokens_bwd(const float* dx0, const uint8_t* mask, int Bt, int Bx, int P, int D, float* dtok, float* dcls,
                       float* dmask_token, void* stream);

/* ---- BEiT pooled-cls tail (beit2.py:455-466: drop cls, mean over the patch tokens, cat([mean, patches])) --------------------------
 * fwd, in place: y[b, 0, :] = mean_i y[b, 1 + i, :] (bf16 [B, N, D], fp32 mean); bwd: out[b, 0] = 0, out[b, 1 + i] = dy[b, 1 + i] + dy[b, 0] / (N - 1). */
int xfm_pool_rows_fwd(xfm_bf16* y, int B, int N, int D, void* stream);
int xfm_pool_rows_bwd(const xfm_bf16* dy, int B, int N, int D, xfm_bf16* out, void* stream);

/* ---- MIM loss (xfm.py:624-635): x = embeddings of the masked view, t = of the clean view (detached), bf16 [B, N, D]; mask [B, N-1]
 * bytes.  fwd: sums[3] += {sum (x-t)^2 over masked patch rows, the same over the cls rows, number of masked patches} (caller zeroes);
 * loss = sums[0] / max(sums[2] * D, 1) + sums[1] / (B * D).  bwd: dx (bf16 [B, N, D], fully written) = gout[0] * d loss / d x;
 * cls_term = 0 drops the cls part (the reference's `mim_cls_only` flag returns the patch term alone). */
#define XFM_MIM_PARTIALS 512
#define XFM_MIM_SUMS_FLOATS (3 + 3 * XFM_MIM_PARTIALS)
int xfm_mim_loss_fwd(const xfm_bf16* x, const xfm_bf16* t, const uint8_t* mask, int B, int N, int D, float* sums, void* stream);
int xfm_mim_loss_bwd(const xfm_bf16* x, const xfm_bf16* t, const uint8_t* mask, const float* sums, const float* gout, int cls_term,
                     int B, int N, int D, xfm_bf16* dx, void* stream);

/* ---- Block-wise MIM mask sampler (masking_generator.py:27-105, called once per image and step on the host at beit2.py:432-439):
 * out[b, p] (bytes, [B, GH*GW]) = 1 on exactly `num` patches per image, drawn by the reference's rejection loop (rectangles of area
 * U[min_num, remaining], log-uniform aspect in [min_aspect, max_aspect], <= 10 attempts per block, uniform top-up), one wavefront per
 * image, counter-based generator keyed by (seed, image).  delta_hist (optional, int32 [GH*GW + 1], +=): how many new patches each
 * accepted block added. */
int xfm_mim_masks(int B, int GH, int GW, int num, int min_num, float min_aspect, float max_aspect, uint64_t seed, uint8_t* out,
                  int* delta_hist, void* stream);

/* ---- RoBERTa embeddings + LayerNorm + dropout (xroberta.py:104-137, 1747-1757) ----------------------------------- */
typedef struct {
  const int64_t* ids;
  const float* word; const float* pos; const float* type;
  const float* w; const float* b;
  xfm_bf16* y; float* mean; float* rstd; int* pos_ids;
  int B, T, pad_id; float eps;
  uint32_t drop_thresh; float drop_scale; uint32_t seed_lo, seed_hi;
  const xfm_bf16* dy; float* dword; float* dpos; float* partial;
  int pos_mode; /* 0: RoBERTa pad-aware cumsum positions; 1: BERT absolute positions 0..T-1 (xbert.py:198-199) */
  const int* row_map; /* optional [B*T]: token (b,t) is written to / its gradient read from row row_map[b*T+t] of y / dy (packed,
                         unpadded rows); -1 skips the token (padding).  mean / rstd / pos_ids stay [B*T]. */
  float* y32;         /* optional fp32 twin of y (same rows): the embedding output enters the encoder's fp32 residual stream un-rounded */
  const float* dy32;  /* optional fp32 gradient added to dy (the residual-branch gradient of the first layer) */
  float* dz_out;      /* optional fp32 [B*T, D] (bwd): the gradient w.r.t. the embedding sum of every token is STORED here (row b*T+t;
                         skipped tokens are not written) and dword / dpos are left alone -- the caller scatters it with
                         xfm_rows_segment_sum in a fixed order instead of one float atomic per element (XFM_DETERMINISTIC) */
} xfm_embed_args;
int xfm_embed_ln_fwd(const xfm_embed_args* a, int D, void* stream);
long xfm_embed_ln_bwd_workspace(int rows, int D);
int xfm_embed_ln_bwd(const xfm_embed_args* a, int D, float* dgamma, float* dbeta, float* dtype, float* workspace,
                     long workspace_bytes, void* stream);

/* ---- Row gather / scatter-add for packed token rows (the [CLS] / masked-position gathers of xroberta.py:1215-1216 and the
 * batch assembly of xfm.py:781-793 on unpadded rows): dst[r,:] = index[r] >= 0 ? src[index[r],:] : 0 (bf16 rows of D elements,
 * D % 8 == 0); and its adjoint dst32[index[r],:] += src[r,:] (fp32 accumulation, rows with index < 0 are skipped). ------------- */
int xfm_rows_gather(const xfm_bf16* src, const int* index, int R, int D, xfm_bf16* dst, void* stream);
int xfm_rows_scatter_add(const xfm_bf16* src, const int* index, int R, int D, float* dst32, void* stream);
/* out[key, :] += sum of src[perm[i], :] over the run of positions i with sorted_key[i] == key, rows added in position order, one owner per
 * run: the scatter-add of an embedding gradient without atomics (nn.Embedding backward, xroberta.py:80-102).  sorted_key int64 [R]
 * ascending (the caller sorts; perm int64 [R] = the matching row order, a STABLE sort keeps it deterministic); runs with key < 0 or
 * key == skip_key are dropped (padding_idx, skipped tokens).  src fp32 [*, D], out fp32 [*, D], D % 4 == 0. */
int xfm_rows_segment_sum(const float* src, const int64_t* perm, const int64_t* sorted_key, long R, int D, long skip_key, float* out,
                         void* stream);

/* ---- One whole RobertaLayer per call (xroberta.py:405-473: self-attention block, optional cross-attention block, FFN block, each
 * closed by dropout + residual + LayerNorm), forward and backward.  The kernels are the ones above; what this adds is the launch
 * SEQUENCE on the native side: a host language pays microseconds per launch (Python: 7-24 us per wrapper call against ~3.5 us for
 * the launch itself), and a text / fusion tower is ~50 launches per layer of 10-30 us kernels -- its time is the host's, not the
 * GPU's, unless the layer is one call.  All buffers are the caller's: `slab` holds the layer's activations (what the backward
 * needs), `bslab` the backward's gradient temporaries, both laid out by xfm_rlayer_layout.  The weight-gradient GEMMs and the
 * cross-attention dK/dV kernel are issued on `side_stream` behind events (NULL: everything on the main stream). ------------------ */
typedef struct {        /* static per layer: bf16 operand copies ([N,K] and transposed [K,ld]), fp32 biases / LayerNorm affine, and
                           where their gradients accumulate (fp32, +=) */
  const xfm_bf16 *wqkv, *wqkv_t, *wo, *wo_t, *wq2, *wq2_t, *wkv2_t, *wo2, *wo2_t, *wi, *wi_t, *wout, *wout_t;
  long ld_wqkv_t, ld_wo_t, ld_wq2_t, ld_wkv2_t, ld_wo2_t, ld_wi_t, ld_wout_t;
  const float *bqkv, *bo, *bq2, *bo2, *bi, *bout;
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *ln3_w, *ln3_b;
  float *dwqkv, *dbqkv, *dwo, *dbo, *dwq2, *dbq2, *dwkv2, *dbkv2, *dwo2, *dbo2, *dwi, *dbi, *dwout, *dbout;
  float *dln1_w, *dln1_b, *dln2_w, *dln2_b, *dln3_w, *dln3_b;
  int D, H, FF, has_cross;
  float eps;
} xfm_rlayer_params;

typedef struct {        /* geometry + per-call inputs shared by forward and backward */
  int R, B, T;                                   /* token rows, sequences, padded sequence length */
  int R_alloc, B_alloc;                          /* geometry slab / bslab were laid out for (0: R, B); a backward over the first
                                                    sequences of a forward pass (their rows are a prefix) passes the forward's */
  int Nenc, U;                                   /* cross-attention: image tokens per image, images (0 = no cross-attention input) */
  const int* seq_start; const int* seq_len;      /* packed rows (xfm_attn_args.q_start / q_len) or NULL */
  const int* key_keep;                           /* [B,T] or NULL */
  const int* enc_keep;                           /* [U,Nenc] or NULL */
  const int* grp_start; const int* grp_rows;     /* grouped cross-attention: rows of each image listed sequence by sequence, or ... */
  const int* xq_start; const int* xq_len; int xq_max;  /* ... RANGE mode: the sequences are laid out image by image, so the queries of
                                                    image u are the contiguous rows xq_start[u] .. + xq_len[u] (<= xq_max): cross-attention
                                                    runs as one ragged problem per image on full 16-row tiles (no per-sequence tiles
                                                    that are mostly padding), dK/dV come out per image */
  int causal, zero_fill;                         /* zero_fill: attention outputs / gradients of rows outside every sequence */
  float scale;
  uint32_t att_thresh; float att_scale; uint32_t hid_thresh; float hid_scale;   /* dropout p as threshold / 1/(1-p); 0 = off */
  uint32_t seed_hi, seed_ctr;                    /* dropout stream k of the layer uses (seed_hi, seed_ctr + 1 + k) */
  const xfm_bf16* x;                             /* layer input [R,D] */
  void* slab;                                    /* forward activations, xfm_rlayer_layout(...).fwd_bytes */
  const xfm_bf16* kv; long kv_ld;                /* cross: this layer's K|V projection of the image states [U*Nenc, >= 2D] */
  void* kv_event;                                /* hipEvent_t the main stream waits for before it reads kv (NULL: none) */
  int f32_stream;                                /* 1: fp32 residual stream inside the layer (layout flag XFM_RL_F32_STREAM): every post-LN sum
                                                    z_k = dropout(h_k) + y_{k-1} uses the UN-ROUNDED fp32 output of the previous LayerNorm and is
                                                    kept in fp32 for the backward, whose residual-branch gradients are fp32 too -- what the
                                                    reference's mixed precision does (LayerNorm and the residual add run in fp32) */
  const float* x32;                              /* f32_stream: fp32 twin of x (the previous layer's y3_32) or NULL (x enters the stream as is) */
} xfm_rlayer_io;

typedef struct {        /* backward-only */
  void* bslab;                                   /* gradient temporaries, xfm_rlayer_layout(...).bwd_bytes */
  const xfm_bf16* dy_a; const xfm_bf16* dy_b;    /* gradient w.r.t. the layer output = dy_a + dy_b (dy_b may be NULL) */
  const xfm_bf16* enc;                           /* image states [U*Nenc, D] (K/V weight gradient) */
  xfm_bf16* dkv; long dkv_ld;                    /* out: dK|dV of this layer [U*Nenc, 2D] (possibly a column block) */
  float* denc32;                                 /* optional fp32 [U*Nenc, D] += dkv @ Wkv (NULL: the caller folds dkv itself) */
  int need_dprev;                                /* produce the gradient w.r.t. the layer input (dprev_a + dprev_b in bslab) */
  void* side_stream;
  float* ws_main; long ws_main_bytes; float* ws_side; long ws_side_bytes;
  float* ln_ws; long ln_ws_stride;               /* non-NULL (with ln_items): the layer's three LayerNorm backward kernels write their column-sum
                                                    partials to ln_ws + k * ln_ws_stride (floats, k = 0..2; each >= xfm_layernorm_bwd_workspace bytes)
                                                    and launch no reduce; ... */
  xfm_reduce_item* ln_items; int* ln_count;      /* ... they append their items to this HOST table instead (ln_items[*ln_count], count advanced) */
  const float* dy_b32;                           /* f32_stream: the fp32 part of the gradient w.r.t. the layer output (the next layer's dres1) or
                                                    NULL; dy_b must be NULL.  The gradient w.r.t. the layer input is dprev (bf16) + dres1 (fp32) */
  int defer_wgrad;                               /* 1: launch NO weight-gradient GEMM -- the caller queues them (the dY / X operands sit at the
                                                    layout's offsets in bslab / slab, which it keeps alive) and runs the queue of the whole
                                                    tower as grouped launches (xfm_gemm_tn_group).  Bias gradients that ride on a weight
                                                    gradient (dbi, dbq2, dbkv2, dbqkv) are deferred with it */
} xfm_rlayer_bwd_args;

typedef struct {        /* byte offsets inside slab / bslab (256-byte aligned) */
  long qkv, c1, lse1, h, z1, m1, r1, y1, q2, c2, lse2, z2, m2, r2, y2, hact, u, z3, m3, r3, y3, fwd_bytes;
  long dh3, dres3, du, d1a, dh2, dres2, dc2, dq2, delta2, d2a, dh1, dres1, dc1, dqkv, delta1, dprev, bwd_bytes;
  long ws_main_bytes, ws_side_bytes;             /* workspace the backward wants on each stream */
  long c2lo;                                     /* forward slab: low half of the cross-attention output (O = c2 + c2lo to fp32-ish precision) */
  long y1_32, y2_32, y3_32;                      /* XFM_RL_F32_STREAM: fp32 twins of y1 / y2 / y3 (-1 otherwise); z1-3 and dres1-3 are fp32 then */
} xfm_rlayer_layout_t;

enum { XFM_RL_DROPOUT = 1, XFM_RL_F32_STREAM = 2 };   /* `flags` of xfm_rlayer_layout */
int xfm_rlayer_layout(int R, int B, int T, int D, int H, int FF, int has_cross, int Nenc, int U, int xq_max, int flags,
                      xfm_rlayer_layout_t* out);
int xfm_rlayer_fwd(const xfm_rlayer_params* p, const xfm_rlayer_io* io, void* stream);
int xfm_rlayer_bwd(const xfm_rlayer_params* p, const xfm_rlayer_io* io, const xfm_rlayer_bwd_args* b, void* stream);

/* ---- Contrastive / matching glue of XFMBase (xfm.py:614-621, 683-746) as a handful of small kernels instead of a few dozen ATen
 * launches (matmul through the vendor BLAS, softmax, nll_loss, fills, multinomial):
 *   rownorm      y = x / max(|x|_2, 1e-12) per row (F.normalize, xfm.py:617-620), fp32 [R, E], E % 64 == 0, E <= 1024; inv = 1 / norm
 *   itc          logits = I . T^T / temp over N gathered rows; loss = (CE(logits, arange) + CE(logits^T, arange)) / 2 (xfm.py:699-703);
 *                fwd: lse [4N] (statistics of the rows of logits, then of logits^T; behind them the 2N rows' loss terms),
 *                loss_sum [2], zeroed by the caller: [0] += the loss, summed over the row terms in a fixed order by the block that takes
 *                the last ticket of the integer counter at [1] (bit-reproducible); bwd: dI, dT (fully written) and
 *                dtemp[0] += for the upstream gradient g[0]; `lse` is the forward's [4N] buffer: the backward parks the N row shares
 *                of dtemp in its dead upper half and adds them in a fixed order (bit-reproducible)
 *                idx != NULL (int64 [N], the gathered image ids of the retrieval fine-tuning step, xfm.py:705-713): soft labels -- the
 *                positives of row r are the rows with the same id, weight 1 / cnt_r each; fwd writes cnt [N], bwd reads it
 *   hard_neg     per row of the LOCAL batch: softmax(sim / temp) + 1e-5, own entry zeroed, ONE categorical draw (xfm.py:727-744:
 *                torch.multinomial(...).item() per row on the host there); text_neg[i] for image i, image_neg[j] for text j;
 *                idx != NULL (int64 [B]): every entry with the row's image id is zeroed (xfm.py:731-734)  -------- */
int xfm_rownorm_fwd(const float* x, int R, int E, float* y, float* inv, void* stream);
int xfm_rownorm_bwd(const float* dy, const float* y, const float* inv, int R, int E, float* dx, void* stream);
int xfm_itc_fwd(const float* I, const float* T, const float* temp, int N, int E, float* lse, float* loss_sum, const int64_t* idx,
                float* cnt, void* stream);
int xfm_itc_bwd(const float* I, const float* T, const float* temp, const float* lse, const float* g, int N, int E, float* dI, float* dT,
                float* dtemp, const int64_t* idx, const float* cnt, void* stream);
int xfm_hard_negatives(const float* I, const float* T, const float* temp, int B, int E, uint64_t seed, int64_t* image_neg,
                       int64_t* text_neg, const int64_t* idx, void* stream);

/* ---- Vocabulary cross-entropy, ignore_index -100 (xroberta.py:1296-1297, 1107-1114) ------------------------------ */
int xfm_ce_fwd(const float* logits, long ld, int R, int V, const int64_t* labels, float* lse, float* loss, void* stream);
/* dlogits = (softmax - onehot) * scale[0]  (per_row_scale = 0: mean / sum reductions) or * scale[row] (reduction 'none'). */
int xfm_ce_bwd(const float* logits, long ld, int R, int V, const int64_t* labels, const float* lse, const float* scale,
               int per_row_scale, xfm_bf16* dlogits, long ldd, void* stream);

/* ---- Cross-entropy against a target row that is not one-hot: loss_r = -sum_c t_c log_softmax(x)_c (ABI 10) ---------------------------
 * Logits, lse, scale and dlogits as in xfm_ce_fwd/bwd: fp32 [R, ld] with V live columns (ld % 4 == 0 and a 16-byte aligned base unless
 * V < 4; columns [V, ld) are never read), bf16 dlogits [R, ldd] (ldd % 8 == 0), zero in columns [V, ldd) and in ignored rows,
 * scale[0] or scale[row].  The forward reads every row once (online max / sum-exp), one workgroup per row.
 *
 * LABEL form -- the row is described, not materialised: t_c = off + (on - off) (lam_r [c == a_r] + (1 - lam_r) [c == b_r]);
 * labels_a int64 [R] (outside [0, V), e.g. -100: the row is ignored -- loss 0, gradient 0), labels_b int64 [R] or NULL (b = a; a live
 * row's b must lie in [0, V), else the row is ignored too), lam fp32 [R] or NULL (1).  With St = V off + (on - off):
 *   loss_r = St lse_r - off sum_c x_c - (on - off) (lam x_a + (1 - lam) x_b),      dlogits = (St softmax - t) scale.
 * Replaces: LabelSmoothSoftmaxCEV1 (xbert.py:1190-1229, used at :1346-1347; Captioning.yaml:28): on = 1 - s, off = s / V;
 * timm LabelSmoothingCrossEntropy (Imagenet.py:608-609) = F.cross_entropy(label_smoothing = s): on = 1 - s + s / V, off = s / V;
 * SoftTargetCrossEntropy on Mixup's two-label targets (Imagenet.py:605-607) without the dense target.  on = 1, off = 0, lam = NULL is
 * xfm_ce_fwd/bwd up to the accumulation order. */
int xfm_ce_smooth_fwd(const float* logits, long ld, int R, int V, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                      float on, float off, float* lse, float* loss, void* stream);
int xfm_ce_smooth_bwd(const float* logits, long ld, int R, int V, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                      float on, float off, const float* lse, const float* scale, int per_row_scale, xfm_bf16* dlogits, long ldd,
                      void* stream);
/* DENSE form -- timm SoftTargetCrossEntropy (Imagenet.py:605-607: sum(-target * log_softmax(x), dim=-1)): target fp32 [R, ldt] (the
 * stride rules of the logits), any non-negative row, any row sum.  loss_r = lse_r sum_c t_c - sum_c t_c x_c; the forward reads logits
 * and target once each and stores lse [R] and tsum [R] (= sum_c t_c) for the backward: dlogits = (softmax tsum - t) scale. */
int xfm_ce_soft_fwd(const float* logits, long ld, const float* target, long ldt, int R, int V, float* lse, float* tsum, float* loss,
                    void* stream);
int xfm_ce_soft_bwd(const float* logits, long ld, const float* target, long ldt, int R, int V, const float* lse, const float* tsum,
                    const float* scale, int per_row_scale, xfm_bf16* dlogits, long ldd, void* stream);

/* ---- Evaluation step of the ImageNet loop (Imagenet.py:495-536 evaluate; ABI 13) --------------------------------------------------------
 * One pass over fp32 logits [R, ld >= V] (ld need NOT be a multiple of 4 and the base need not be aligned: 16-byte loads are used when
 * every row starts on 16 bytes, scalar loads otherwise), labels int64 [R].  Per row r:
 *   row_loss[r] = logsumexp(x) - x[label]                                  (CrossEntropyLoss, reduction 'none')
 *   row_rank[r] = #{j: x[j] > x[label]} + #{j < label: x[j] == x[label]}   (int32)
 * THE TIE RULE: the rank is the label's position in a STABLE descending sort of the row -- of equal logits the lower column comes
 * first.  torch.topk leaves the order of ties unspecified; this library pins it.  The label is among the top k iff row_rank < k.
 * A trailing single workgroup then ADDS into acc (fp32 [3]), the rows one after the other in ascending order, no atomics:
 *   acc[0] += sum_r row_loss[r],   acc[1] += #{r: row_rank[r] < k1},   acc[2] += #{r: row_rank[r] < k2}.
 * The counts are exact in fp32 (up to 2^24 rows per buffer) and the result is bit-reproducible with and without XFM_DETERMINISTIC.  acc
 * accumulates across calls: zero it once per evaluation, read it once at the end.
 * A label outside [0, V) is the caller's error (the Python wrapper refuses it where it can see the labels on the host); in the kernel
 * such a row contributes nothing to acc, and gets row_loss 0 and row_rank V.
 * row_loss and row_rank may each be NULL.  The library owns no scratch memory, so with either NULL one workgroup walks all rows itself
 * (same order, same arithmetic, same bits; slower -- pass both for large R).
 * XFM_E_ARG (nothing is launched): k1 < 1, k2 < k1, k2 > V, ld < V, R < 1, or a NULL logits / labels / acc. */
int xfm_ce_topk_eval(const float* logits, long ld, int R, int V, const int64_t* labels, int k1, int k2, float* row_loss, int* row_rank,
                     float* acc, void* stream);

/* ---- Answer ranking of the VQA evaluation (VQA.py:75-100 -> model_generation.py:146-202 rank_answer; ABI 14) ---------------------------
 * Answers are ranked, not generated: the first decoder pass gives first-token logits, xfm_answer_shortlist keeps the k most probable
 * candidates of every question, the second decoder pass gives each shortlisted candidate's summed NLL, xfm_answer_rerank re-ranks.
 * One workgroup per question, no atomics; both give the same bits with and without XFM_DETERMINISTIC.
 *
 * THE TIE RULE (both functions): several candidates share a first token, so equal probabilities are normal.  The order is by the key
 * (probability descending, position ascending) -- EQUAL PROBABILITIES ORDER BY ASCENDING CANDIDATE INDEX (xfm_answer_rerank: by ascending
 * position in the shortlist).  The key is unique, so the result does not depend on the launch geometry.  torch.topk leaves the order of
 * ties unspecified; torch.sort(stable=True, descending=True) is this rule.
 *
 * xfm_answer_shortlist: logits fp32 [Q, ld] with V live columns (any ld >= V, any base alignment: 16-byte loads when every row starts
 * on 16 bytes, scalar loads otherwise), first_tok int64 [A] = the first answer token of every candidate.  Per question, in fp32:
 *   max and sum of exp over all V logits;  p[a] = exp(l[first_tok[a]] - max) / sum;  the k largest p in descending order ->
 *   prob fp32 [Q, k], cand int64 [Q, k] (candidate indices).
 * A first token outside [0, V) is the caller's error; such a candidate gets probability 0 (nothing is read out of bounds).
 * The candidates are sorted in LDS, which sets the caps below.  XFM_E_ARG (nothing is launched): k < 1, k > A, k > XFM_ANSWER_MAX_K,
 * A > XFM_ANSWER_MAX_A, Q < 1, V < 1, ld < V, or a NULL operand.
 *
 * xfm_answer_rerank: prob fp32 [Q, k] and cand int64 [Q, k] as above, seq_loss fp32 [Q * k] question-major = the decoder's summed NLL of
 * every shortlisted candidate.  Per question: s = log(prob) - seq_loss (prob 0 gives -inf, as torch; a question whose scores are ALL
 * -inf is undefined), softmax over the k, sort descending with the tie rule on the position ->
 *   topk_probs fp32 [Q, k], topk_ids int64 [Q, k] (candidate ids in the new order), and, when result is not NULL,
 *   result[result_offset + q] = topk_ids[q, 0]: the answers of a whole evaluation pass collect in ONE device buffer, read once.
 * XFM_E_ARG: k < 1, k > XFM_ANSWER_MAX_K, Q < 1, result_offset < 0, or a NULL operand (result may be NULL). */
#define XFM_ANSWER_MAX_A 8192
#define XFM_ANSWER_MAX_K 1024
int xfm_answer_shortlist(const float* logits, long ld, int Q, int V, const int64_t* first_tok, int A, int k, float* prob, int64_t* cand,
                         void* stream);
int xfm_answer_rerank(const float* prob, const float* seq_loss, const int64_t* cand, int Q, int k, int64_t* topk_ids, float* topk_probs,
                      int64_t* result, long result_offset, void* stream);

/* ---- GLUE evaluation metrics and the regression loss (run_glue.py:370-386; model_classification.py:89-93; ABI 15) -----------------------
 * Plain loads and stores, no float atomics, no global atomics: the same bits with and without XFM_DETERMINISTIC.  Any ld / stride and
 * any base alignment of the fp32 / bf16 operands (int64 and double operands lie on 8 bytes).
 *
 * xfm_cls_eval (`outputs.argmax(dim=-1)` + `metric.add_batch`, :380-384): logits fp32 [B, ld] with L live columns, labels int64 [B].
 * Per row r: p = argmax under TORCH.ARGMAX'S RULE -- the first index of the maximum; a NaN counts as the maximum and the first NaN wins;
 * -0.0 == +0.0.  pred[pred_offset + r] = p (pred int64, may be NULL).  If 0 <= labels[r] < L: conf[labels[r] * L + p] += 1; a row with
 * any other label (GLUE's test splits carry -1) is written to pred and counted nowhere.  conf int64 [L * L] ACCUMULATES across calls: zero
 * it once per pass, read it once at the end.  One workgroup owns conf for the call (integer counts: the order of the adds cannot
 * change them).  XFM_E_ARG (nothing is launched): B < 1, L < 2, L > XFM_METRIC_MAX_L, ld < L, pred_offset < 0, NULL logits / labels / conf.
 *
 * xfm_corr_rank (pearsonr / spearmanr of the glue metric for stsb): x, y fp32 [N] -> out double [2] = (Pearson, Spearman); rank_x,
 * rank_y fp32 [N] (each may be NULL) receive the average ranks.  One workgroup.  Pearson: fp64, two passes (means, then centred sums),
 * every sum in a fixed order, r = Sxy / sqrt(Sxx * Syy); a zero denominator gives NaN, as scipy.  Spearman: the same formula on AVERAGE
 * RANKS as scipy.stats.rankdata(method='average') defines them -- equal values share the mean of their 1-based positions (every rank is
 * a multiple of 0.5); -0.0 and +0.0 are equal.  The values are sorted in LDS (bitonic network, 64-bit unique keys: an order-preserving
 * image of the float above the position), which sets the cap.  Any NaN in x or y makes both outputs (and the ranks) NaN.
 * XFM_E_ARG: N < 2, N > XFM_CORR_MAX_N, NULL x / y / out.
 *
 * xfm_mse_fwd / xfm_mse_bwd (`F.mse_loss(prediction.view(-1), targets.view(-1))`): pred fp32 or bf16 (pred_bf16 != 0), element i at
 * pred[i * stride]; target fp32 [B].  fwd: loss[0] = sum_i (p_i - t_i)^2 / B in fp32, one workgroup, ordered sum.
 * bwd: dpred fp32 [B] (contiguous), dpred[i] = 2 * dloss[0] * (p_i - t_i) / B with dloss a DEVICE scalar (no host read).
 * XFM_E_ARG: B < 1, stride < 1, a NULL operand. */
#define XFM_METRIC_MAX_L 32
#define XFM_CORR_MAX_N 8192
int xfm_cls_eval(const float* logits, long ld, int B, int L, const int64_t* labels, int64_t* conf, int64_t* pred, long pred_offset,
                 void* stream);
int xfm_corr_rank(const float* x, const float* y, int N, double* out, float* rank_x, float* rank_y, void* stream);
int xfm_mse_fwd(const void* pred, long stride, int pred_bf16, const float* target, int B, float* loss, void* stream);
int xfm_mse_bwd(const void* pred, long stride, int pred_bf16, const float* target, const float* dloss, int B, float* dpred, void* stream);

/* ---- Grounding evaluation (Grounding_bbox.py:73-93 val; dataset/utils.py:271-345 grounding_eval_bbox / _vlue, :349-361 computeIoU; ABI 16)
 * xfm_box_eval: the box accuracy of one batch in one launch.  coord fp32 [n, 4] = the model's (cx, cy, w, h) in [0, 1]; ref_row int32 [n]
 * names each sample's row of the three ref tables (NULL: rows 0 .. n - 1); ref_box fp32 [R, 4] = ground truth (x, y, w, h) in pixels,
 * ref_size fp32 [R, 2] = (width, height) of the image, ref_split int32 [R] = 0 val, 1 testA, 2 testB (anything else: counted nowhere).
 * Per sample, in fp64 from the fp32 inputs, every operation rounded on its own, in the reference's order:
 *   pw = w W, ph = h H, px = cx W - pw / 2, py = cy H - ph / 2                                 (utils.py:281-286)
 *   x1 = max(rx, px), y1 = max(ry, py), x2 = min(rx + rw - 1, px + pw - 1), y2 = min(ry + rh - 1, py + ph - 1)
 *   inter = (x2 - x1 + 1)(y2 - y1 + 1) if x1 < x2 and y1 < y2 (both strict), else 0
 *   union = rw rh + pw ph - inter, IoU = inter / union; union <= 0 (the reference divides by zero): IoU = 0     (utils.py:349-361)
 *   correct iff IoU >= 0.5.
 * out fp32 (may be NULL): row out_offset + i = (px, py, pw, ph, IoU), each rounded to fp32 once; the rows of a whole pass collect in ONE
 * device buffer.  counts int64 [3, 2]: counts[s] += (#correct, #samples) of split s; it ACCUMULATES across calls: zero it once per pass,
 * read it once at the end.  A ref_row outside [0, R): the out row is NaN and the sample is counted nowhere (nothing is read out of
 * bounds).  One workgroup owns counts for the call: the six counts are collected in LDS as integers and added with plain 64-bit loads
 * and stores -- no global atomics, no float atomics, the same bits with and without XFM_DETERMINISTIC.
 * XFM_E_ARG (nothing is launched): n < 1, R < 1, out_offset < 0, NULL coord / ref_box / ref_size / ref_split / counts. */
int xfm_box_eval(const float* coord, const int* ref_row, const float* ref_box, const float* ref_size, const int* ref_split, int n, int R,
                 float* out, long out_offset, int64_t* counts, void* stream);

/* ---- Grad-CAM grounding (Grounding.py:76-126 val on the attention-map contract of models/xroberta.py:182-194, 268-270;
 * dataset/utils.py:178-223 grounding_eval; ABI 19)
 * xfm_xattn_gradcam: the attention map of ONE cross-attention layer, the gradient that reaches it and their Grad-CAM, in one launch, from
 * what the layer's backward holds when the gradient dout of its context output arrives.  Eval mode: no attention dropout, no head mask, so
 *   P[b,h,t,j]  = exp(scale q[b,t,h,:] . k[src(b),j,h,:] - lse[b,h,t])           (the softmax; lse is what xfm_attn_fwd left)
 *   dP[b,h,t,j] = dout[b,t,h,:] . v[src(b),j,h,:]                                 (the hook's gradient, Grounding.py:104-105)
 *   cam[b,j-1]  = 1 / (H t_div) sum_h sum_{t < q_len[b]} P[b,h,t,j] max(dP[b,h,t,j], 0),  j = 1 .. Sk - 1     (Grounding.py:109-115)
 * Both means divide by the full extents: H, and t_div = the padded length T of the batch (not q_len[b]); the sum over t < q_len[b] is the
 * reference's multiplication by the attention mask; key 0 (the image's [CLS]) is dropped.
 * Up to three outputs, each may be NULL: cam fp32 [B, Sk - 1]; p_out and dp_out fp32 [B, H, Sq, Sk], rows t >= q_len[b] written as zero
 * (the reference holds a softmax and an exactly-zero gradient there and multiplies both by the mask).
 * Operands follow xfm_attn_args addressing: q and dout bf16 token-major, element (row, h, d) at ptr[row * rs + h * 64 + d]; k and v bf16
 * with their own row strides (the two halves of the layer's K | V projection), key j of source s at row s * Sk + j; lse fp32
 * [B, H, stat_ld].  Query rows of entry b: q_start[b] .. + q_len[b] (packed), or b * Sq .. + q_len[b] when q_start is NULL (dense); q_len
 * NULL = Sq rows.  kv_src (optional int [B]): entry b reads key/value source kv_src[b] (NULL: b) of n_src sources -- image_index,
 * encoder_batch_index and the grouped layout alike; an entry outside [0, n_src) reads nothing and yields zeros.
 * Head dimension 64; no key mask and no bias (the fusion tower's image keys are never masked on this path).  One workgroup per (entry, 64
 * keys) walks the heads and sums the query rows in a fixed order: plain vector loads and stores, no atomics, no workspace, the same bits
 * on every launch, with and without XFM_DETERMINISTIC.
 * XFM_E_ARG (nothing is launched): cam, p_out and dp_out all NULL; a NULL q / dout / k / v / lse; B < 1, B > 65535, H < 1, Sq < 1, Sk < 2;
 * a row stride below H * 64 or not a multiple of 8; an operand not 16-byte aligned; stat_ld < Sq or not a multiple of 4; q_start without
 * q_len; n_src < 1; t_div < 1; scale not positive and finite.  XFM_E_UNSUPPORTED (nothing is launched): Sq > 64, the grouped kernels'
 * limit. */
typedef struct {
  const xfm_bf16* q; long q_rs;
  const xfm_bf16* dout; long do_rs;
  const xfm_bf16* k; long k_rs;
  const xfm_bf16* v; long v_rs;
  const float* lse; long stat_ld;
  const int* q_start; const int* q_len;
  const int* kv_src; int n_src;
  int B, H, Sq, Sk;
  float scale; int t_div;
  float* cam; float* p_out; float* dp_out;
} xfm_gradcam_args;
int xfm_xattn_gradcam(const xfm_gradcam_args* a, void* stream);

/* xfm_cam_box_rank: the loop body of grounding_eval (utils.py:183-216) for n refs, one workgroup per ref.  cam fp32 [n, p, p] (row = y);
 * img_hw int [n, 2] = (height, width) of each ref's image; det fp64 [Ndet, 4] = the detector boxes (x, y, w, h) in pixels, those of ref i
 * at rows det_start[i] .. det_start[i + 1] (CSR, int [n + 1]); max_dets = the largest number of boxes of one ref (the host knows it: the
 * boxes come from there); ref_box fp64 [n, 4]; ref_split int [n] = 0 val, 1 testA, 2 testB (anything else: counted nowhere).
 * The reference upsamples the map to (height, width) with F.interpolate(mode='bicubic') -- align_corners=False, no antialias, A = -0.75 --
 * and sums it over rows int(y) : int(y + h), columns int(x) : int(x + w) (Python truncation; the slice clamps at the border, and may be
 * empty).  The upsampled map is never built: the sum is a^T cam b, a_i = the sum over the box's rows of the weight output row y gives
 * input row i, b_j the same over its columns.  The tap weights are ATen's, in fp32 and in its operation order: source coordinate
 * (dst + 0.5) * (in / out) - 0.5, tap index floor(src) - 1 .. + 2 clamped to the map, lambda clamped to [0, 1]; a, b and the product are
 * fp64, and so are area ** alpha (area = w * h) and the comparison.  The chosen box is the first whose score is strictly greater than
 * every earlier one, starting from 0; its IoU with ref_box is computeIoU (utils.py:349-361), the arithmetic of xfm_box_eval.
 * out fp64 [N, 3]: row out_offset + i = (index of the chosen box among the ref's own, its score, its IoU); the rows of a whole pass
 * collect in ONE device buffer.  counts int64 [3, 2]: counts[s] += (#IoU >= 0.5, #refs) of split s, by one workgroup with plain loads
 * and stores; it ACCUMULATES across calls.  No atomics on global memory: the same bits with and without XFM_DETERMINISTIC.
 * Defined differently from the reference ON PURPOSE: a ref none of whose boxes scores above 0 gets (-1, 0, 0) and is counted as WRONG; the
 * reference would reuse the box chosen for the previous ref, or raise on the first one.
 * Boxes with a negative coordinate are the host's to reject (Python's negative slice bounds mean something else); here they are clamped
 * to 0, so nothing is read out of bounds.
 * XFM_E_ARG (nothing is launched): n < 1, p < 1, out_offset < 0, max_dets < 0, alpha not finite, a NULL operand.  XFM_E_UNSUPPORTED
 * (nothing is launched): p > XFM_CAM_MAX_P or max_dets > XFM_CAM_MAX_DETS, the caps of the LDS layout. */
#define XFM_CAM_MAX_P 32
#define XFM_CAM_MAX_DETS 256
int xfm_cam_box_rank(const float* cam, int p, const int* img_hw, const double* det, const int* det_start, int max_dets, const double* ref_box,
                     const int* ref_split, int n, double alpha, double* out, long out_offset, int64_t* counts, void* stream);

/* ---- VQ-KD visual tokenizer: nearest-code assignment (models/norm_ema_quantizer.py:149-162 NormEMAVectorQuantizer.forward; the MIM
 * targets of models/xfm.py:624-629 through models/model_vqkd.py get_codebook_indices; ABI 20)
 * xfm_vq_assign: z fp32 [M, K] (row r at z + r * z_ld), code fp32 [n_code, K] (row c at code + c * code_ld), in one launch
 *   zn       = z[r] / max(||z[r]||_2, 1e-12)                                   (F.normalize, norm_ema_quantizer.py:153)
 *   index[r] = argmin_c (|zn|^2 + |code[c]|^2 - 2 zn . code[c])                (norm_ema_quantizer.py:158-162)
 * |code[c]|^2 is part of the score: the codebook is NOT assumed to be unit-norm.  |zn|^2, the same for every code of a row, is left out of
 * the comparison.  EQUAL SCORES GO TO THE LOWEST CODE INDEX (torch.argmin's rule); every score is the same arithmetic wherever its code
 * sits -- a k-ordered fp32 fmaf chain for the dot product (v_mfma_f32_32x32x2_f32: exact fp32 products and sums, no bf16), another for
 * |code[c]|^2, one fmaf joining them -- so two equal codebook rows score bit-equal against every row and the lower index is returned.
 * index int64 [M].  counts int32 [n_code], optional (NULL: not kept): counts[c] += the number of rows assigned to c -- the histogram
 * that the eval-mode EMA of cluster_size consumes (norm_ema_quantizer.py:168-172); it ACCUMULATES across calls.  Integer atomics on global
 * memory: an integer sum does not depend on the order.
 * The [M, n_code] score matrix never exists in global memory and there is no workspace: one workgroup keeps 64 normalised rows in LDS,
 * streams the codebook through LDS in chunks of 128 codes and carries a running (best, argbest) per row in registers.  Plain vector loads
 * and stores, no floating-point atomics: the same bits on every launch, with and without XFM_DETERMINISTIC.
 * A row with a non-finite component still gets an index in [0, n_code); which one is unspecified.  An all-zero row scores |code[c]|^2.
 * XFM_E_ARG (nothing is launched): a NULL z / code / index; M < 1 or n_code < 1; z_ld < K or code_ld < K; z or code not 16-byte aligned,
 * or a leading dimension not a multiple of 4.  XFM_E_UNSUPPORTED (nothing is launched): K not a multiple of 4 or outside [4, 64]. */
int xfm_vq_assign(const float* z, long z_ld, int M, int K, const float* code, long code_ld, int n_code, int64_t* index, int* counts,
                  void* stream);

/* ---- Incremental decoding (models/xbert.py:1368-1484 prepare_inputs_for_generation / _generate_no_beam_search; the cached branches of the
 * attention at models/xroberta.py:224-262; ABI 17)
 * xfm_decode_attn: attention of ONE new query token per batch row against a key/value cache, head_dim 64 (replaces, for a step with a past,
 * xroberta.py:224-234 -- torch.cat of the past with the new key / value, or the re-projection of the encoder states -- and :240-262).
 * Cache layout: token-major, element (b, s, h, d) at ptr[(b * cap + s) * rs + h * 64 + d], bf16, `cap` rows per entry; k_cache and v_cache
 * share rs (the K | V projection of the encoder states, [sources * Sk, 2 D] with cap = Sk and rs = 2 D, is such a cache as it stands).
 *   self mode (k_new != NULL):  row b of q / k_new / v_new ([B] rows of H * 64, row strides in elements, e.g. column slices of the QKV
 *       GEMM output) is the new token; `pos` tokens are cached already (the same for every row).  The call writes k_new / v_new to cache
 *       row pos and attends over rows 0 .. pos; Sk must be pos + 1, n_src must be B, kv_index NULL.  The workgroup that owns (b, h) is the
 *       only one that touches that slice of the cache.
 *   cross mode (k_new == NULL): the Sk keys of source kv_index[b] (NULL: b) are read, nothing is written; n_src = the number of sources.
 *       A kv_index entry outside [0, n_src) reads nothing and yields a zero output row.
 * key_keep (may be NULL): int32 rows of keep_ld >= Sk elements, one per source (self mode: per batch row); 0 adds -10000 to the score, as
 * in xfm_attn_args.  score = scale q.k (+ -10000); softmax and P.V in fp32 (the probabilities are not rounded to bf16); o = bf16 rows
 * [B, H * 64] with row stride o_rs.  q, k_new, v_new and the caches must start on 16 bytes, their row strides multiples of 8 elements.
 * XFM_E_ARG (nothing is launched): pos + 1 > cap, Sk < 1, Sk > cap (cross), H * 64 > rs, a misaligned or NULL operand. */
typedef struct {
  const xfm_bf16* q; long q_rs;
  const xfm_bf16* k_new; long k_new_rs;   /* NULL: cross mode */
  const xfm_bf16* v_new; long v_new_rs;
  xfm_bf16* k_cache; xfm_bf16* v_cache;   /* read only in cross mode */
  long rs;                                /* row stride of both caches, elements */
  xfm_bf16* o; long o_rs;
  const int* key_keep; long keep_ld;
  const int* kv_index; int n_src;
  int B, H, cap, pos, Sk;
  float scale;
} xfm_decode_attn_args;
int xfm_decode_attn(const xfm_decode_attn_args* a, void* stream);

/* xfm_next_token: one launch per decoding step for xbert.py:1422-1462.  Per row b of the fp32 logits [B, ld] (V <= ld columns count) and
 * of the id buffer ids int64 [B, ids_ld] with cur_len valid columns:
 *   penalty != 1: every DISTINCT id of ids[b, :cur_len] inside [0, V) has its logit multiplied by `penalty` if negative, divided by it
 *       otherwise (:1425-1432, where the reference walks a set); the logits themselves are not modified;
 *   tok = argmax of the penalised row, the lowest column among equal maxima (:1444) -- or next_token[b] when next_token != NULL (:1441,
 *       the draw itself stays with the caller);  lp = log_softmax(penalised row)[tok]                                     (:1447-1448)
 *   u = unfinished[b];  ids[b, cur_len] = u ? tok : pad_id  (:1453-1454);  hist_unfinished[b, step] = u, hist_logprob[b, step] = lp
 *       (:1449-1450; both [B, hist_ld]);  unfinished[b] = u && the written id is none of eos_ids[0 .. n_eos)                (:1461-1462);
 *   *n_unfinished (may be NULL) += the number of rows still unfinished after the step (:1465, the host's early-exit check).
 * No float atomics; every result is a plain store and the count an integer add per row: the same bits with and without
 * XFM_DETERMINISTIC.  A pre-drawn token outside [0, V) gives lp = NaN and reads nothing.
 * XFM_E_ARG (nothing is launched): cur_len outside [0, ids_ld), step outside [0, hist_ld), V > ld, V > XFM_NEXT_TOKEN_MAX_V,
 * n_eos > XFM_NEXT_TOKEN_MAX_EOS, penalty <= 0, a NULL operand. */
#define XFM_NEXT_TOKEN_MAX_V 131072
#define XFM_NEXT_TOKEN_MAX_EOS 8
typedef struct {
  const float* logits; long ld; int V;
  int64_t* ids; long ids_ld; int cur_len;
  float penalty;
  const int64_t* next_token;              /* NULL: greedy */
  int* unfinished;                        /* [B], 1 / 0 */
  int* hist_unfinished; float* hist_logprob; long hist_ld; int step;
  int pad_id; int n_eos; int eos_ids[XFM_NEXT_TOKEN_MAX_EOS];
  int* n_unfinished;
  int B;
} xfm_next_token_args;
int xfm_next_token(const xfm_next_token_args* a, void* stream);

/* xfm_sample_token (ABI 18): one launch per SAMPLED decoding step -- xbert.py:1422-1462 with do_sample (:1434-1441) and
 * top_k_top_p_filtering (:1487-1519, min_tokens_to_keep = 1) on the device.  Per row b of the fp32 logits [B, ld] (V <= ld columns count):
 *   z_j = the repetition-penalised logit of xfm_next_token (once per distinct id of ids[b, :cur_len]) DIVIDED by `temperature` (an IEEE
 *       fp32 divide, :1437); -inf inputs stay -inf; the logits themselves are not modified.
 *   top_k > 0: k' = min(max(top_k, 1), V), t = the k'-th largest z counted with multiplicity; every z_j >= t is kept (:1500 removes only
 *       logits < kth, so equal values at the cut are all kept).  Exact: a radix select over the order-preserving 32-bit image of z.
 *   top_p < 1, over what top-k kept: the order is descending z, EQUAL VALUES IN ASCENDING COLUMN ORDER (torch.sort leaves that open; this
 *       is the library's rule); p = softmax over the kept set, c_i its inclusive running sum; position i stays iff i == 0 or
 *       c_{i-1} <= top_p (:1508-1514).
 *   draw, over the final kept set: m = max z, w_j = exp(z_j - m), Z = sum w; u = uniforms[b] when uniforms != NULL (fp32 in [0, 1), used
 *       as given), else u = (r >> 8) 2^-24 with r = rng_u32(rng_row_key(seed_lo, seed_hi, b), step) of csrc/common.h; C_j = the inclusive
 *       running sum of w over the kept columns in ascending COLUMN order; tok = the lowest kept column with C_j > u Z (if rounding leaves
 *       none: the highest kept column with w_j > 0).
 *   lp = z_tok - m - log Z: log_softmax of the filtered row at the token (:1447-1448).
 *   Sums: every w_j is taken ONCE as the integer floor(2^44 exp(z_j - m)) (fp32 __expf, exact scaling), and every sum of w -- the top-p
 *       running sum, Z, C_j -- is a 64-bit integer sum (V <= 2^17 terms of at most 2^44).  Integer addition has no order, so no sum
 *       depends on the order of the lanes, and a running sum carries no rounding beyond the V 2^-44 of the floors (the comparisons
 *       c_{i-1} <= top_p and C_j > u Z are made on integers against floor(top_p Z) and floor(u Z), both products in fp64).
 *   The bookkeeping is xfm_next_token's: ids[b, cur_len], hist_unfinished, hist_logprob, the eos update of unfinished, *n_unfinished.
 *   filtered (may be NULL): fp32 [B, filtered_ld], columns [0, V) receive z_j where kept and -inf elsewhere: top_k_top_p_filtering of the
 *       penalised, tempered row (a -0 is stored as +0).
 * A row with no finite z, with a NaN or with +inf gives tok = 0 and lp = NaN (filtered: z unfiltered).  Nothing is read or written out of
 * range.  No float atomics; the same bits run to run and with and without XFM_DETERMINISTIC.  top_k == 0 and top_p == 1 skip both selects.
 * XFM_E_ARG (nothing is launched): every case of xfm_next_token; temperature not finite or <= 0; top_p outside (0, 1]; top_k < 0;
 * filtered != NULL with filtered_ld < V. */
typedef struct {
  const float* logits; long ld; int V;
  int64_t* ids; long ids_ld; int cur_len;
  float penalty;
  float temperature; int top_k; float top_p;
  uint32_t seed_lo, seed_hi;
  const float* uniforms;                  /* [B] or NULL: the device generator */
  float* filtered; long filtered_ld;      /* may be NULL */
  int* unfinished;                        /* [B], 1 / 0 */
  int* hist_unfinished; float* hist_logprob; long hist_ld; int step;
  int pad_id; int n_eos; int eos_ids[XFM_NEXT_TOKEN_MAX_EOS];
  int* n_unfinished;
  int B;
} xfm_sample_token_args;
int xfm_sample_token(const xfm_sample_token_args* a, void* stream);

/* ---- Device Mixup / CutMix (timm Mixup._mix_batch / _mix_elem and mixup_target as called at Imagenet.py:468-469; ABI 10) -------------
 * xfm_mixup: fp32 images [B, C, H, W], B even, mixed IN PLACE: row i against the original row j = B - 1 - i, with the per-row device
 * arrays lam fp32 [B] and box int32 [B, 4] = (yl, yh, xl, xh).  lam_i == 1: row i is left alone; an empty box (yh <= yl or xh <= xl):
 * x_i <- lam_i x_i + (1 - lam_i) x_j; otherwise the pixels inside the box are copied bit for bit from x_j and the rest is untouched.
 * One pass (each element of the batch is read once and written at most once) in place of flip, mul_, mul_, add_.
 * xfm_mixup_target: out fp32 [B, ldo] (ldo >= num_classes; columns past num_classes are zeroed),
 * out[i] = lam_i onehot_s(labels_i) + (1 - lam_i) onehot_s(labels_{B-1-i}), off = s / num_classes, on = 1 - s + off. */
int xfm_mixup(float* x, int B, int C, int H, int W, const float* lam, const int* box, void* stream);
int xfm_mixup_target(const int64_t* labels, const float* lam, int B, int num_classes, float smoothing, float* out, long ldo, void* stream);

/* ---- Region pre-training step (Pretrain.py:94-121 run_region_iter; ABI 11) -------------------------------------------------------------
 * Region pooling (the vision tower's region call form, beit2.py:467-475): full bf16 [n_img, 1 + P, D] is the tower's normalised
 * output, idx int32 [bs] names the image of every sample, atts bytes [bs, P] are the patch columns of image_atts (0 / 1).
 *   fwd: out bf16 [bs, 1 + P, D]: rows 1..P of sample s = the patch rows of image idx[s], bit for bit; row 0 = sum_p atts[s, p]
 *        full[idx[s], 1 + p, :] / sum_p atts[s, p], fp32 sums rounded once.  wsum fp32 [bs] = sum_p atts[s, p], for the backward.  One
 *        pass over the gathered rows.  (A sample whose mask is all zero gets the reference's non-finite row 0.)
 *   bwd: dfull bf16 [n_img, 1 + P, D], fully written: dfull[i, 1 + p, :] = sum over the samples s with idx[s] == i, in ascending s, of
 *        dout[s, 1 + p, :] + atts[s, p] / wsum[s] * dout[s, 0, :] (fp32 sums, one rounding); dfull[i, 0, :] = 0; an image that no sample
 *        reads gets zeros.  No atomics: bit-reproducible with and without XFM_DETERMINISTIC. */
int xfm_region_pool_fwd(const xfm_bf16* full, const int* idx, const uint8_t* atts, int n_img, int bs, int P, int D, xfm_bf16* out,
                        float* wsum, void* stream);
int xfm_region_pool_bwd(const xfm_bf16* dout, const int* idx, const uint8_t* atts, const float* wsum, int n_img, int bs, int P, int D,
                        xfm_bf16* dfull, void* stream);
/* Box loss (XFMBase.get_bbox_loss, xfm.py:815-840): coord / target fp32 [bs, 4] as (cx, cy, w, h), 16-byte aligned; is_image fp32 [bs] or
 * NULL (row weight w_r = 1 - is_image[r], else 1).  out[0] = sum_r w_r sum_j |coord - target| / num, out[1] = sum_r w_r (1 - GIoU of the
 * paired xyxy boxes) / num, num = sum_r w_r.  If any box of either set has x2 < x1 or y2 < y1, out[1] = 0 and carries no gradient (the
 * reference's whole-batch rule).  One workgroup, fixed-order sums, fp64 inside, rounded to fp32 once.
 * state fp64 [bs, 8] (written by fwd): d out[0] / d coord[r, :], d out[1] / d coord[r, :].
 *   bwd: dcoord fp32 [bs, 4] = g[0] * state[r, 0:4] + g[1] * state[r, 4:8]; g fp32 [2] on the device (the two upstream scalars). */
int xfm_box_loss_fwd(const float* coord, const float* target, const float* is_image, int bs, float* out, double* state, void* stream);
int xfm_box_loss_bwd(const double* state, const float* g, int bs, float* dcoord, void* stream);

/* ---- Flat-arena optimiser step (optim.py:4-50 + clip, apex_ddp_accelerator.py:100-110) --------------------------- */
typedef struct {
  float* p; float* g; float* m; float* v;
  const uint8_t* group;       /* group id per 256-element block */
  float lr[4]; float wd[4];
  float beta1, beta2, eps, bc1, bc2;
  const float* clip_coef;     /* device scalar or NULL */
  long n;
  int zero_grad;              /* != 0: g is zeroed in the same sweep (the step's optimizer.zero_grad(): one pass over the arena less) */
} xfm_adamw_args;
int xfm_adamw(const xfm_adamw_args* a, void* stream);
/* The same sweep with torch.optim.AdamW's single-tensor rule (non-amsgrad; Imagenet.py:569-570 builds that optimizer; ABI 13).  Same
 * struct, same meaning of bc1 / bc2 / group / lr / wd / clip_coef / zero_grad, same 256-multiple length rule.  Per element, in this order:
 *   g' = g * clip;  p *= 1 - lr * wd;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g' g';  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 * (xfm_adamw, the transformers rule: eps is added BEFORE the bias correction and the decay follows the update). */
int xfm_adamw_torch(const xfm_adamw_args* a, void* stream);
/* out[0] += sum x[i]^2 (n % 4 == 0), bit-reproducible: fixed-grid block partials through `workspace`
 * (XFM_SUMSQ_WORKSPACE_FLOATS floats, contents irrelevant) summed in a fixed order -- the clip coefficient derived from it must be
 * identical on every data-parallel rank (apex_ddp_accelerator.py:100-110 clips after the all-reduce). */
#define XFM_SUMSQ_WORKSPACE_FLOATS 1024
int xfm_sumsq(const float* x, long n, float* out, float* workspace, void* stream);

/* ---- Data-parallel exchange over RCCL / xGMI ------------------------------------------------------------------------
 * What the reference does through torch.distributed: the gradient all-reduce of DistributedDataParallel
 * (accelerators/ddp_accelerator.py:34-98, apex_ddp_accelerator.py:34-110), the feature AllGather of the contrastive loss
 * (models/xfm.py:17-50), the parameter broadcast at wrap time -- for a host without torch.distributed.  One
 * communicator per process (one process per GPU); every call is enqueued on the caller's HIP stream and returns at once; nothing is
 * allocated or synchronised.  librccl is resolved at the first call (dlopen: inside a PyTorch process that is the RCCL torch already
 * mapped); XFM_E_UNSUPPORTED when it cannot be loaded.  The Python host (accelerators/rccl_ddp_accelerator.py) keeps using
 * torch.distributed's "nccl" backend, which IS RCCL; xfm_amd/dp.py wraps these for hosts that do not.
 *   rank 0: xfm_dp_unique_id(id) -> hand the XFM_DP_ID_BYTES bytes to every rank (file, socket, environment) ->
 *   every rank, with its device current: xfm_dp_init(id, rank, world, &comm) -> ... -> xfm_dp_finalize(comm). */
#define XFM_DP_ID_BYTES 128
enum { XFM_DP_F32 = 0, XFM_DP_BF16 = 1, XFM_DP_I32 = 2 };
enum { XFM_DP_SUM = 0, XFM_DP_AVG = 1, XFM_DP_MAX = 2 };
int xfm_dp_unique_id(void* id);
int xfm_dp_init(const void* id, int rank, int world, void** comm);
/* in place over one bucket (a range of the flat gradient arena): buf[i] = op over ranks; XFM_DP_AVG is the mean DistributedDataParallel
 * takes (ReduceOp.AVG: one pass, no separate division) */
int xfm_dp_bucket_allreduce(void* comm, void* buf, long n, int dtype, int op, void* stream);
/* recv[r * n_per_rank + i] = rank r's send[i]  (models/xfm.py:17-50: the forward of AllGather; its backward is the caller's slice) */
int xfm_dp_allgather(void* comm, const void* send, void* recv, long n_per_rank, int dtype, void* stream);
int xfm_dp_broadcast(void* comm, void* buf, long n, int dtype, int root, void* stream);
int xfm_dp_finalize(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* XFM_HIP_H */
