// What more than one attention kernel family uses (attention_*.hip, all one translation unit through attention.hip): the tile
// constants, the LDS staging and fragment helpers, the softmax / mask / dropout helpers, one copy of each barrier / wait /
// direct-to-LDS primitive, and the launcher that owns the dynamic-LDS attribute.
//
// Reference arithmetic: beit2.py:126-166 (q*scale, + relative-position bias, softmax, attn_drop, @v) and
// xroberta.py:201-289 (q/sqrt(d) BEFORE q@k^T, + additive -10000 key mask, softmax, dropout, @v; causal variant
// :772-792).  Scores are never materialised in HBM: each wave owns 16 query rows, keys stream through LDS in chunks
// of 64 with an online softmax, and S is computed TRANSPOSED (S^T = K.Q^T) so that the fp32 accumulator of one MFMA
// is already laid out as the B operand of the next one (P^T for O^T = V^T.P^T), with no lane movement.  V is staged
// row-major and consumed through the transposed LDS read (ds_read_b64_tr_b16).
//
// Layouts: q/k/v/o are addressed as ptr[(b*S + s)*row_stride + h*64 + d], i.e. straight out of / into the fused
// projection GEMM buffers ([B*S, 3*768] for self-attention, [B*Sk, 2*768] for the cross-attention K/V).
#pragma once
#include <type_traits>
#include "common.h"

#define MASK_NEG (-10000.0f)
#define EXCL_NEG (-1.0e30f)
#define ATTN_TILE (64 * 128)       // one 64-row x 64-column bf16 tile
#define ATTN_SLOT (2 * ATTN_TILE)  // K tile + V tile (or Q tile + dO tile)
#define ATTN_RES_MAX 4             // up to 256 rows stay LDS-resident (64 KiB); longer sequences stream chunk by chunk

typedef xfm_attn_args AttnArgs;

__device__ __forceinline__ int swz_a(int r) { return (r >> 1) & 7; }

// Two ROWS x 64 bf16 tiles (K and V, or Q and dO), 128-B rows, rows >= nvalid zero filled.  All global loads of the
// pair are issued before the first LDS store, so one thread keeps up to 8 x 16 B in flight instead of paying the
// memory latency once per 16 B (the kernels are HBM/L2-bound: 64-row tiles of the fused projection buffers).
template <int ROWS, int MAXIT>
__device__ __forceinline__ void stage_pair(char* lds0, const bf16* g0, long rs0, char* lds1, const bf16* g1, long rs1, int row0,
                                           int nvalid, int tid, int nthreads) {
  constexpr int CH = ROWS * 8;
  for (int base = 0; base < CH; base += MAXIT * nthreads) {  // one trip unless the workgroup is a single wave
    u32x4 v0[MAXIT], v1[MAXIT];
#pragma unroll
    for (int i = 0; i < MAXIT; ++i) {
      const int q = base + tid + i * nthreads;
      v0[i] = u32x4{0, 0, 0, 0};
      v1[i] = u32x4{0, 0, 0, 0};
      if (q < CH) {
        const int r = q >> 3, c = q & 7;
        if (row0 + r < nvalid) {
          v0[i] = *reinterpret_cast<const u32x4*>(g0 + (long)(row0 + r) * rs0 + c * 8);
          v1[i] = *reinterpret_cast<const u32x4*>(g1 + (long)(row0 + r) * rs1 + c * 8);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < MAXIT; ++i) {
      const int q = base + tid + i * nthreads;
      if (q < CH) {
        const int r = q >> 3, c = q & 7;
        const int off = r * 128 + ((c ^ swz_a(r)) << 4);
        *reinterpret_cast<u32x4*>(lds0 + off) = v0[i];
        *reinterpret_cast<u32x4*>(lds1 + off) = v1[i];
      }
    }
  }
}

// One LDS slot = two 64 x 64 bf16 tiles (K|V or Q|dO), filled by direct-to-LDS loads (global_load_lds_dwordx4): no
// staging registers, every wave's loads for the whole slot are in flight together.  Wave-instruction j (0..15)
// fills rows 8*(j&7).. +7 of tile j>>3, lane-linear; the XOR swizzle is applied on the SOURCE chunk.  Rows past
// `nvalid` re-read the last valid row (finite data; their scores / probabilities are masked to exactly 0).
__device__ __forceinline__ void stage_slot(char* slot, const bf16* g0, long rs0, const bf16* g1, long rs1, int row0, int nvalid,
                                           int w, int nw, int lane) {
  for (int j = w; j < 16; j += nw) {
    const int r = (j & 7) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ swz_a(r);
    int gr = row0 + r;
    gr = gr < nvalid ? gr : nvalid - 1;
    const bf16* src = ((j >> 3) ? g1 + (long)gr * rs1 : g0 + (long)gr * rs0) + c * 8;
    __builtin_amdgcn_global_load_lds(GLB_PTR(void, src), LDS_PTR(void, slot + (j >> 3) * ATTN_TILE + (j & 7) * 1024), 16, 0, 0);
  }
}
__device__ __forceinline__ void stage_wait() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// A/B fragment of a row-major tile: lane (lg, lr) -> row (row0 + lr), elements [ks*32 + 8*lg, +8)
__device__ __forceinline__ bf16x8 row_frag(const char* tile, int row0, int ks, int lr, int lg) {
  const int r = row0 + lr, c = ks * 4 + lg;
  return *reinterpret_cast<const bf16x8*>(tile + r * 128 + ((c ^ swz_a(r)) << 4));
}

// transposed fragment: k-slots (lg, j<4) -> rows rowA + 4*lg + j ; (lg, j>=4) -> rows rowB + 4*lg + (j-4); column col0 + lr
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int rowA, int rowB, int col0, int lr, int lg) {
  const int col = col0 + 4 * (lr & 3);
  const int ra = rowA + 4 * lg + (lr >> 2), rb = rowB + 4 * lg + (lr >> 2);
  const int offa = ra * 128 + (((col >> 3) ^ swz_a(ra)) << 4) + (col & 7) * 2;
  const int offb = rb * 128 + (((col >> 3) ^ swz_a(rb)) << 4) + (col & 7) * 2;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, tile + offa));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, tile + offb));
  union { struct { s16x4 a, b; } s; bf16x8 v; } u;
  u.s.a = lo;
  u.s.b = hi;
  return u.v;
}

__device__ __forceinline__ bf16x8 pack_pair(const f32x4& a, const f32x4& b) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) { r[j] = f2bf(a[j]); r[4 + j] = f2bf(b[j]); }
  return r;
}

__device__ __forceinline__ float group4_max(float v) {  // across the 4 lanes that share lane&15
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group4_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// Packed (unpadded) token rows: batch entry b's queries are rows q_start[b] .. q_start[b] + q_len[b] of q / o / dout / dq (q_len <= Sq,
// Sq stays the padded length: statistics, dropout counters and grids are laid out for it); the same for keys / values through
// k_start / k_len.  NULL = dense [B, S] rows.  Keys past k_len are excluded exactly (probability 0), which is what the additive
// -10000 mask of a padded batch gives in fp32 (xroberta.py:751-807), so a prefix-masked batch needs no key_keep when packed.
__device__ __forceinline__ void q_seq(const AttnArgs& a, int b, long& base, int& len) {
  if (a.q_start != nullptr) { base = a.q_start[b]; len = a.q_len[b]; }
  else { base = (long)b * a.Sq; len = a.Sq; }
}
__device__ __forceinline__ void k_seq(const AttnArgs& a, int b, long& base, int& len) {
  if (a.k_start != nullptr) { base = a.k_start[b]; len = a.k_len[b]; }
  else { base = (long)b * a.Sk; len = a.Sk; }
}

// Score post-processing shared by forward and dQ: s = raw*scale + bias (+ MASK_NEG when the key is masked or causally hidden),
// EXCL_NEG past the last key.  Branch-free: the key-keep flags of a chunk are fetched up front with the bias (16 dwords in
// flight, one wait) and every condition becomes a select; chunks with nothing to mask (`plain`) are a bare FMA.
__device__ __forceinline__ void load_keep(const AttnArgs& a, int kvb, int kc, int lg, int (&kk)[4][4]) {
  const int* row = a.key_keep + (long)kvb * a.Sk;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int kj = kc * 64 + t * 16 + 4 * lg + r;
      kk[t][r] = row[kj < a.Sk ? kj : a.Sk - 1];
    }
}
__device__ __forceinline__ float score_masked(const AttnArgs& a, float raw, float biasv, bool has_mask, int keep, bool causal, int qi, int kj, int sk) {
  const bool masked = (has_mask & (keep == 0)) | (causal & (kj > qi));
  const float s = fmaf(raw, a.scale, biasv) + (masked ? MASK_NEG : 0.f);
  return kj >= sk ? EXCL_NEG : s;
}

// dropout decision of score (b, h, qi, kj): row = the query row, column = the key.  `drop_key` is loop-invariant wherever a
// lane keeps its query row (forward, dQ); dK/dV walks query rows and pays the key per element.
__device__ __forceinline__ uint32_t drop_key(const AttnArgs& a, int b, int h, int qi) {
  return rng_row_key(a.seed_lo, a.seed_hi, (uint32_t)((b * a.H + h) * a.Sq + qi));
}
__device__ __forceinline__ bool drop_keep(const AttnArgs& a, uint32_t key, int kj) { return rng_keep(rng_u32(key, (uint32_t)kj), a.drop_thresh); }

// additive bias row segment of chunk kc for this lane's query row: keys kc*64 + t*16 + 4*lg .. +3, t = 0..3 (zeros past Sk)
__device__ __forceinline__ void load_bias(const AttnArgs& a, int h, int qc, int kc, int lg, f32x4 (&bv)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int kj0 = kc * 64 + t * 16 + 4 * lg;
    bv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.bias != nullptr && kj0 < a.Sk) bv[t] = *reinterpret_cast<const f32x4*>(a.bias + ((long)h * a.Sq + qc) * a.bias_ld + kj0);
  }
}

// Output row of one lane: 4 consecutive columns per d-tile, normalised; o_lo (optional) takes the bf16 of what the bf16 of O lost.
__device__ __forceinline__ void store_out(const AttnArgs& a, long row, int h, int lg, const f32x4 (&oacc)[4], float inv) {
  bf16* op = a.o + row * a.o_rs + h * 64;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    bf16x4 ov, ol;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = oacc[dt][r] * inv;
      ov[r] = f2bf(v);
      ol[r] = f2bf(v - bf2f(ov[r]));
    }
    *reinterpret_cast<bf16x4*>(op + dt * 16 + 4 * lg) = ov;
    if (a.o_lo != nullptr) *reinterpret_cast<bf16x4*>(a.o_lo + row * a.o_rs + h * 64 + dt * 16 + 4 * lg) = ol;
  }
}
// delta_i = dO_i . (O_i + Olo_i) for the query row of lane (lg, lr): each of the 4 lanes sharing lr holds 16 of the 64 columns
// (the two 8-column fragments it already loaded of dO), so the row sum is one group4_sum.
__device__ __forceinline__ float delta_from_out(const AttnArgs& a, long row, int h, int lg, const bf16x8& df0, const bf16x8& df1) {
  const bf16* op = a.o + row * a.o_rs + h * 64;
  const bf16* lp = a.o_lo + row * a.o_rs + h * 64;
  const bf16x8 o0 = *reinterpret_cast<const bf16x8*>(op + 8 * lg), o1 = *reinterpret_cast<const bf16x8*>(op + 32 + 8 * lg);
  const bf16x8 l0 = *reinterpret_cast<const bf16x8*>(lp + 8 * lg), l1 = *reinterpret_cast<const bf16x8*>(lp + 32 + 8 * lg);
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    t = fmaf(bf2f(df0[i]), bf2f(o0[i]) + bf2f(l0[i]), t);
    t = fmaf(bf2f(df1[i]), bf2f(o1[i]) + bf2f(l1[i]), t);
  }
  return group4_sum(t);
}

// ---------------------------------------------------------------------------------------------
// barriers, counted waits and the direct-to-LDS load: one copy each
// ---------------------------------------------------------------------------------------------
// direct-to-LDS load of 16 bytes per lane (one 1-KB piece: 8 rows x 128 B): per-lane source address, wave-uniform LDS destination (M0).
// Issued as inline asm on purpose: when the compiler sees a direct-to-LDS load it drains it (s_waitcnt vmcnt(0)) in front of
// every later LDS read, which would serialise the prefetch of the next entry with the MFMAs of this one.  The caller waits
// (wait_vm) before the barrier that publishes the tiles.
__device__ __forceinline__ void lds_dma16(const void* src, unsigned dst) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(dst) : "memory", "m0");
}
// workgroup barrier that orders LDS traffic only: __syncthreads() also waits for vmcnt(0), i.e. for the prefetch DMA in flight
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// raw barrier: LDS-DMA stays in flight across it
__device__ __forceinline__ void raw_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// this wave's vector-memory operations but the youngest n have completed (wave-uniform n; more than 12: all of them)
__device__ __forceinline__ void wait_vm(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
    case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

// rows [0, nrows) of a [*, 64] bf16 operand into consecutive 64-row tiles (lds_dma16, same image as stage_slot's tiles)
__device__ __forceinline__ void stage_rows(char* tiles, const bf16* g, long rs, int nrows, int w, int nw, int lane) {
  const int n = ((nrows + 63) >> 6) * 8;
  for (int j = w; j < n; j += nw) {
    const int r = (j & 7) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ swz_a(r);
    int gr = (j >> 3) * 64 + r;
    gr = gr < nrows ? gr : nrows - 1;
    const bf16* src = g + (long)gr * rs + c * 8;
    const unsigned dst = (unsigned)(uintptr_t)LDS_PTR(void, tiles) + (unsigned)__builtin_amdgcn_readfirstlane((j >> 3) * ATTN_TILE + (j & 7) * 1024);
    lds_dma16(src, dst);
  }
}
// tr_frag with the two 16-row halves of the k dimension in (possibly) different tiles
__device__ __forceinline__ bf16x8 tr_frag2(const char* tileA, int rowA, const char* tileB, int rowB, int col0, int lr, int lg) {
  const int col = col0 + 4 * (lr & 3);
  const int ra = rowA + 4 * lg + (lr >> 2), rb = rowB + 4 * lg + (lr >> 2);
  const int offa = ra * 128 + (((col >> 3) ^ swz_a(ra)) << 4) + (col & 7) * 2;
  const int offb = rb * 128 + (((col >> 3) ^ swz_a(rb)) << 4) + (col & 7) * 2;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, tileA + offa));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, tileB + offb));
  union { struct { s16x4 a, b; } s; bf16x8 v; } u;
  u.s.a = lo;
  u.s.b = hi;
  return u.v;
}

// ---- host side ----
static bool attn_plain(const AttnArgs& a) { return a.key_keep == nullptr && a.causal == 0 && a.drop_thresh == 0u; }

static void attn_geom(int S, int& nw, int& blocks, int max_nw = 8) {
  const int tiles = cdiv(S, 16);
  nw = tiles < max_nw ? tiles : max_nw;
  // balance waves over blocks (e.g. 13 tiles -> 2 blocks of 7 waves)
  blocks = cdiv(tiles, nw);
  nw = cdiv(tiles, blocks);
}
