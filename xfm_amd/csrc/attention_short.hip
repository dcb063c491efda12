// The short dense backward pair (Sk <= 256, no mask / dropout / packing: the 224-px ViT at 197 tokens, unmasked text rows):
// attn_bwd_dq_short_kernel, attn_bwd_dkv_short_kernel, their shape predicate and launches.  Included by attention.hip.
// ---------------------------------------------------------------------------------------------
// backward 1/2 for short, dense, unmasked problems (the 224-px ViT: Sq = Sk = 197; any Sk <= 256): dQ, delta, dbias.
// The general dQ kernel (attention_general.hip) gives a wave 16 queries against ALL keys; with the bias gradient that is 253 VGPRs (one 7-wave workgroup per
// CU), a bias row segment fetched per key chunk, and two passes over the keys for delta: 202 us per ViT layer, 12 us per (batch,
// head, query block), against 1 us of MFMA time.  Here a workgroup is (query group of <= 4 tiles, head) and its 16 waves are
// (query tile, key range): a wave owns 16 queries x <= 64 keys of EVERY batch entry the workgroup walks, so
//   * its bias tile is loaded once (16 VGPRs, batch-invariant) and its bias-gradient sum is 16 VGPRs, not 64;
//   * S and dP are computed once: the four key-range waves of a query tile exchange their partial delta through LDS;
//   * dS crosses LDS once (bf16, 8 B per lane and tile) and the wave with key range w sums d-tile w of dQ over all keys;
//   * K, V (second LDS buffers) and the Q / dO fragments (registers) of the next entry are fetched while this one computes.
// LDS: K (2 x 32 KB) | V (2 x 32 KB) | dS exchange (8 KB per query tile) | delta partials.  One workgroup (12 waves) per CU.
// ---------------------------------------------------------------------------------------------
#define VB_KBUF (ATTN_RES_MAX * ATTN_TILE)
#define VB_EXCH(QT) ((QT) * 16 * 512)
#define VB_LDS(QT) (4 * VB_KBUF + VB_EXCH(QT) + (QT) * 4 * 16 * 4)
#define VB_LDS_QL(QT, NP) (4 * (2 * (NP) * 2048) + (QT) * (NP) * 1024 + (QT) * 4 * 16 * 4 + 2 * (QT) * 2 * 2048)   // Q / dO through LDS (PRE, NP <= 7)


// PRE: the row term delta_i = dO_i . (O_i + Olo_i) is taken from the forward's output (a.o, a.o_lo) at the top of an entry, from
// fragments fetched one entry ahead -- no delta exchange, no second barrier, and dS leaves in the same phase as the scores.
// !PRE (no o_lo): delta_i = sum_j P_ij dP_ij from the very P and dP that form dS, exchanged between the four key-range waves.
#ifdef XFM_DIAG
// DBG: the stamped build (tools/attn_timeline.py).  dbg = the timeline buffer, 16-byte aligned, with xfm_diag_set_timeline's flags in
// its low bits: the stamping wave (0..7) | 8 = pin mode
template <int QT, int NP, bool PRE, bool DBG = false>
__global__ __launch_bounds__(QT * 256) void attn_bwd_dq_short_kernel(AttnArgs a, int nb_per_block, int G, long long* dbg) {
#else
template <int QT, int NP, bool PRE>
__global__ __launch_bounds__(QT * 256) void attn_bwd_dq_short_kernel(AttnArgs a, int nb_per_block, int G) {
#endif
  constexpr int NW = QT * 4;
  // QL (PRE and <= 14 key tiles): the Q / dO tiles of the workgroup's queries come through LDS too -- 4 QT one-KB pieces per entry instead
  // of four fragment loads in each of the 4 QT waves (every key-range wave of a query tile fetched the same rows) -- in the room
  // that 28-KB K / V buffers leave.  The vector-memory path moves ~64 B/clk per CU and every wave-load holds its wave at issue
  // while the queue is full: the loads, not the arithmetic, set the entry period (tools/attn_timeline.py).
  constexpr bool QL = PRE && NP <= 7;
  constexpr int KBUF = QL ? 2 * NP * 2048 : VB_KBUF;           // one K or V image
  constexpr int EXQ = QL ? NP * 1024 : 16 * 512;               // dS exchange of one query tile
  constexpr int QIMG = QT * 2 * 2048;                          // Q tiles | dO tiles of one entry (QL)
  extern __shared__ __attribute__((aligned(16))) char lds[];
  // (w through readfirstlane: the tile counts below are wave-uniform and the compiler must know it -- see the entry loop)
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int qt = w >> 2, kw = w & 3;
  // 1-D grid, logical id = group + G * (head + H * batch slice), an XCD takes a contiguous range of logical ids: the G groups of one
  // (head, batch slice) read the same K / V rows at about the same time and now do so through ONE L2
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int grp = wg % G, h = (wg / G) % a.H, zslice = wg / (G * a.H);
  const int sk = a.Sk, sq = a.Sq;
  const int KT = (sk + 15) >> 4;  // key tiles of 16 (<= 2 * NP), dealt to the four key-range waves as evenly as they go
  const int kbase = KT >> 2, krem = KT & 3;
  const int nt = kbase + (kw < krem ? 1 : 0);
  const int kt0 = kw * kbase + (kw < krem ? kw : krem);
  const int QTILES = (sq + 15) >> 4;  // query tiles dealt to the G groups the same way
  const int qbase_t = QTILES / G, qrem = QTILES % G;
  const int nqt = qbase_t + (grp < qrem ? 1 : 0);
  const int q0 = (grp * qbase_t + (grp < qrem ? grp : qrem) + qt) * 16;
  const bool wave_active = qt < nqt && q0 < sq;
  const int qi = q0 + lr;
  const bool qvalid = wave_active && qi < sq;
  const int qc = qi < sq ? qi : sq - 1;

  char* const sK0 = lds;
  char* const ex = lds + 4 * KBUF;
  float* const dred = reinterpret_cast<float*>(ex + QT * EXQ);
  char* const qimg = reinterpret_cast<char*>(dred) + QT * 4 * 16 * 4;   // (QL) two Q | dO images

  // LDS addressing.  A 16-row tile t of an image starts 2048 B after tile t-1 (four to a 64-row, 8 KB staging tile) and the XOR
  // swizzle of a row depends on (row >> 1) & 7 only, i.e. not on the tile: every fragment address is ONE per-lane offset plus a
  // multiple of 2048 -- an immediate -- instead of a register per fragment.
  const int sw_r = (lr >> 1) & 7;
  const int rf0 = lr * 128 + ((lg ^ sw_r) << 4), rf1 = lr * 128 + (((4 + lg) ^ sw_r) << 4);  // row fragments, k-steps 0 / 1
  const int tr_row = 4 * lg + (lr >> 2), tr_col = kw * 16 + 4 * (lr & 3);                   // transposed fragment of d-tile kw
  const int tro = tr_row * 128 + ((((tr_col >> 3) ^ ((tr_row >> 1) & 7))) << 4) + (tr_col & 7) * 2;
  // dS exchange of a query tile: key tiles in PAIRS, 16 B per lane and pair -- a lane's values of tile 2p in the low, of tile 2p + 1 in
  // the high 8 bytes: the dQ loop reads a pair as ONE ds_read_b128 (256 B/clk; the two 8-byte reads 512 B apart it used to take
  // were fused by the compiler into ds_read2st64_b64, 128 B/clk, and made its phase LDS-bound), and the value read IS the MFMA operand.
  char* const ex_q = ex + qt * EXQ + lane * 16;
  auto ex_slot = [&](int tile) { return ex_q + ((tile >> 1) << 10) + ((tile & 1) << 3); };
  // key tiles past the last one stay zero for the whole kernel (the dQ loop runs over NP pairs)
  for (int i = tid; i < QT * EXQ / 16; i += NW * 64) reinterpret_cast<u32x4*>(ex)[i] = u32x4{0, 0, 0, 0};

  // Softmax in the exponent of 2, the bias folded into the accumulator the score MFMAs start from and the row's log-sum-exp into the
  // exponent's fma:  S' = K.q + bias / scale,  P = exp2(S' * scale * log2 e - lse * log2 e)   (no subtraction, no select: keys past Sk
  // carry bias -1e30, query rows past Sq carry lse = +1e30)
  const float inv_scale = 1.0f / a.scale, c2 = a.scale * 1.44269504088896341f;
  f32x4 bvs[4], dsacc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    dsacc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kj0 = (kt0 + t) * 16 + 4 * lg;
    f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.bias != nullptr && t < nt && kj0 < sk) bv = *reinterpret_cast<const f32x4*>(a.bias + ((long)h * sq + qc) * a.bias_ld + kj0);
#pragma unroll
    for (int r = 0; r < 4; ++r) bvs[t][r] = (kj0 + r < sk ? bv[r] : -1.0e30f) * inv_scale;
  }

  // batch-invariant per-lane byte offsets; an entry adds one scalar stride to the (scalar) base pointers
  // (unsigned 32-bit lane offsets against SCALAR per-entry base pointers: every access is `global_* v_off, s[base]`; as signed offsets
  // the loop-strength reducer turned each into a per-lane 64-bit pointer carried round the loop, 26 VGPRs of them)
  const unsigned q_off = (unsigned)(((long)qc * a.q_rs + h * 64 + 8 * lg) * 2), do_off = (unsigned)(((long)qc * a.do_rs + h * 64 + 8 * lg) * 2);
  // (PRE: wave kw takes a QUARTER of the row's 64 columns of O / O_lo -- the 4 of this lane's 16 dO columns with index
  // 32 (kw >> 1) + 8 lg + 4 (kw & 1) + 0..3 -- so the four key-range waves together read O once, not four times)
  const unsigned do_q4 = (unsigned)(((long)qc * a.do_rs + h * 64 + 32 * (kw >> 1) + 8 * lg + 4 * (kw & 1)) * 2);
  const unsigned o_off = PRE ? (unsigned)(((long)qc * a.o_rs + h * 64 + 32 * (kw >> 1) + 8 * lg + 4 * (kw & 1)) * 2) : 0u;
  const unsigned dq_off = (unsigned)(((long)(qvalid ? qi : 0) * a.dq_rs + h * 64 + kw * 16 + 4 * lg) * 2), stat_off = (unsigned)((long)h * a.stat_ld + qc);
  const long q_bs = (long)sq * a.q_rs * 2, do_bs = (long)sq * a.do_rs * 2, dq_bs = (long)sq * a.dq_rs * 2, stat_bs = (long)a.H * a.stat_ld;
  const long o_bs = (long)sq * a.o_rs * 2;
  const long k_bs = (long)sk * a.k_rs * 2, v_bs = (long)sk * a.v_rs * 2;
  // this wave's pieces of a K / V image (<= 3 of the 1-KB, 8-row direct-to-LDS instructions): source offset per lane, LDS offset per
  // wave.  The 2 NP tiles the dQ loop reads are staged (rows past Sk repeat the last key: finite, their dS is zero).
  const int b_begin = zslice * nb_per_block;
  int b_end = b_begin + nb_per_block;
  b_end = b_end < a.B ? b_end : a.B;
  // Running (scalar) base pointers instead of `base + b * stride` at every use: the staging / fetch cursors point at the entry being
  // REQUESTED (one ahead of the entry computed), pdelta at the entry computed, pdq at the one before it (whose dQ is stored late);
  // one 64-bit add each per entry (the multiplications were ~100 scalar instructions per entry in a kernel that is issue-bound).
  const char *pk = reinterpret_cast<const char*>(a.k) + (long)b_begin * k_bs, *pv = reinterpret_cast<const char*>(a.v) + (long)b_begin * v_bs;
  const char *pq = reinterpret_cast<const char*>(a.q) + (long)b_begin * q_bs, *pdo = reinterpret_cast<const char*>(a.dout) + (long)b_begin * do_bs;
  const char *po = PRE ? reinterpret_cast<const char*>(a.o) + (long)b_begin * o_bs : nullptr;
  const char *plo = PRE ? reinterpret_cast<const char*>(a.o_lo) + (long)b_begin * o_bs : nullptr;
  const float* plse = a.lse + (long)b_begin * stat_bs;
  float* pdelta = a.delta + (long)b_begin * stat_bs;
  char* pdq = reinterpret_cast<char*>(a.dq) + (long)(b_begin - 1) * dq_bs;
#ifdef XFM_DIAG
  // pin mode: every request stays on the slice's first entry -- the whole walk then runs from cache, which prices the memory side of
  // the entry period; results are garbage
  const bool pin = DBG && ((uintptr_t)dbg & 8) != 0;
#endif
  auto advance = [&]() {
#ifdef XFM_DIAG
    if (pin) return;
#endif
    pk += k_bs; pv += v_bs; pq += q_bs; pdo += do_bs; plse += stat_bs;
    if constexpr (PRE) { po += o_bs; plo += o_bs; }
  };
  unsigned pc_dst[3];
  constexpr int n_pc = 4 * NP;
  static_assert(n_pc <= 3 * NW, "three pieces per wave");
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int j = w + i * NW;
    pc_dst[i] = (unsigned)__builtin_amdgcn_readfirstlane((j >> 3) * ATTN_TILE + (j & 7) * 1024);
  }
  unsigned k_offs[3] = {0, 0, 0}, v_offs[3] = {0, 0, 0};
  if constexpr (!PRE) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int j = w + i * NW;
      const int r = (j & 7) * 8 + (lane >> 3);
      const int c = (lane & 7) ^ swz_a(r);
      int gr = (j >> 3) * 64 + r;
      gr = gr < sk ? gr : sk - 1;
      k_offs[i] = (unsigned)(((long)gr * a.k_rs + h * 64 + c * 8) * 2);
      v_offs[i] = (unsigned)(((long)gr * a.v_rs + h * 64 + c * 8) * 2);
    }
  }
  auto stage_piece = [&](int b, int buf, int i) {   // K and V piece i of this wave (inline asm: see stage_rows)
    if (w + i * NW < n_pc) {
      unsigned k_off, v_off;
      if constexpr (PRE) {
        // (the lane offsets are recomputed per piece from an opaque copy of the lane id -- a dozen integer instructions -- instead of
        // living in six VGPRs for the whole kernel: with the O quarters in flight the scores' bias tile would be spilled for them)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int j = w + i * NW;
        const int r = (j & 7) * 8 + (ln >> 3);
        const int c = (ln & 7) ^ swz_a(r);
        int gr = (j >> 3) * 64 + r;
        gr = gr < sk ? gr : sk - 1;
        k_off = (unsigned)(((long)gr * a.k_rs + h * 64 + c * 8) * 2);
        v_off = (unsigned)(((long)gr * a.v_rs + h * 64 + c * 8) * 2);
      } else {
        k_off = k_offs[i];
        v_off = v_offs[i];
      }
      const char* kb = pk;
      const char* vb = pv;
      const unsigned dk = (unsigned)(uintptr_t)LDS_PTR(void, sK0) + (unsigned)buf * KBUF, dv = dk + 2 * KBUF;
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(k_off), "s"(kb), "s"(dk + pc_dst[i]) : "memory", "m0");
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(v_off), "s"(vb), "s"(dv + pc_dst[i]) : "memory", "m0");
    }
  };
  auto stage_kv = [&](int b, int buf) {
#pragma unroll
    for (int i = 0; i < 3; ++i) stage_piece(b, buf, i);
  };

  // Q / dO (/ O, O_lo) fragments and the log-sum-exp of the NEXT entry are fetched while the current one computes (a load issued at
  // the top of an entry and waited for there costs the whole HBM latency per entry: every wave of the CU sits behind the same barrier)
  bf16x8 qf0, qf1, df0, df1;
  bf16x4 oq, lq, dq4;
  bf16x4 dq_hold = bf16x4{0, 0, 0, 0};   // this wave's dQ of the entry just finished (stored one entry later)
  float lse_n = 0.f;
  // (QL) piece w of the 4 QT: 8 query rows of Q (w < 2 QT) or dO into image `buf`, rows past Sq repeat the last one
  auto stage_q = [&](int b, int buf) {
    if (w < 4 * QT) {
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const int isd = w >= 2 * QT ? 1 : 0, jj = w - isd * 2 * QT;
      const int r = (jj & 1) * 8 + (ln >> 3);
      const int c = (ln & 7) ^ swz_a(r);
      int gr = q0 - qt * 16 + (jj >> 1) * 16 + r;
      gr = gr < sq ? gr : sq - 1;
      const unsigned off = (unsigned)(((long)gr * (isd ? a.do_rs : a.q_rs) + h * 64 + c * 8) * 2);
      const char* base = isd ? pdo : pq;
      const unsigned dst = (unsigned)(uintptr_t)LDS_PTR(void, qimg) + (unsigned)(buf * QIMG + isd * (QT * 2048) + jj * 1024);
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(off), "s"(base), "s"(dst) : "memory", "m0");
    }
  };
  auto fetch_q = [&](int b) {
    if constexpr (!QL) {
      const char* qp = pq + q_off;   // (scalar base + zero-extended lane offset)
      const char* dop = pdo + do_off;
      qf0 = *reinterpret_cast<const bf16x8*>(qp);
      qf1 = *reinterpret_cast<const bf16x8*>(qp + 64);
      df0 = *reinterpret_cast<const bf16x8*>(dop);
      df1 = *reinterpret_cast<const bf16x8*>(dop + 64);
    } else {   // the dO quarter that meets this wave's O quarter (the row's fragments themselves arrive through LDS)
      dq4 = *reinterpret_cast<const bf16x4*>(pdo + do_q4);
    }
    if constexpr (PRE) {
      const char* op = po + o_off;
      const char* lp = plo + o_off;
      oq = *reinterpret_cast<const bf16x4*>(op);
      lq = *reinterpret_cast<const bf16x4*>(lp);
    }
    lse_n = plse[stat_off];
  };
  if (b_begin < b_end) {
    stage_kv(b_begin, 0);
    if constexpr (QL) stage_q(b_begin, 0);
    fetch_q(b_begin);
    advance();
  }
#ifdef XFM_DIAG
  const int dbg_wave = (int)((uintptr_t)dbg & 7);
  dbg = reinterpret_cast<long long*>((uintptr_t)dbg & ~(uintptr_t)15);
#endif
  // The number of key tiles of a wave (nt, 0..4) is a run-time, wave-uniform value.  Written as `if (t < nt)` inside the tile loops it
  // made every tile its own exec-masked basic block -- read, wait, MFMA, read, wait, MFMA: 16 LDS round trips in series.  So the whole
  // walk is straight-line code per tile COUNT (NT; -1 = a wave without a query tile: barriers and its share of the staging only),
  // picked by ONE scalar branch per kernel.  (A switch per phase inside one loop made the register allocator merge five versions of
  // the score registers: 38 spilled VGPRs.)
  auto walk = [&](auto NTc) {
    constexpr int NT = decltype(NTc)::value;
    constexpr bool ACT = NT >= 0;
    constexpr int NTS = NT > 0 ? NT : 1;
    for (int b = b_begin; b < b_end; ++b) {
      const int cur = (b - b_begin) & 1;
      const char* sK = sK0 + cur * KBUF;
#ifdef XFM_DIAG
      // one wave stamps the phases of every entry (10-ns clock)
      long long* const dbe = DBG && dbg != nullptr && tid == dbg_wave * 64 && b - b_begin < 32 ? dbg + ((long)blockIdx.x * 32 + (b - b_begin)) * 16 : nullptr;
      if (DBG && dbe) dbe[0] = wall_clock64();
#endif
      // everything up to the fetches of this entry must have landed.  (The compiler cannot see this wait: the empty asm makes it place
      // its own wait for the fetched registers HERE, before this entry's direct-to-LDS loads are issued, rather than at their first
      // use, where a counted wait would also drain those.)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      // dQ of the PREVIOUS entry leaves here, behind the wait: vmcnt counts stores too (until L2 has them), and a store issued at the
      // end of an entry made this wait, a few instructions later, sit out its whole acknowledgement
      if constexpr (ACT) {
        if (b > b_begin && qvalid) *reinterpret_cast<bf16x4*>(pdq + dq_off) = dq_hold;
      }
      if constexpr (!QL) asm volatile("" : "+v"(qf0), "+v"(qf1), "+v"(df0), "+v"(df1));
      else asm volatile("" : "+v"(dq4));
      asm volatile("" : "+v"(lse_n));
      if constexpr (PRE) asm volatile("" : "+v"(oq), "+v"(lq));
      const float nlse = qvalid ? -lse_n * 1.44269504088896341f : -1.0e30f;  // rows past Sq: P = exp2(-huge) = 0
      float delta = 0.f;
      if constexpr (PRE && ACT) {
        // this wave's quarter of dO . (O + O_lo): packed bf16 dot products with fp32 accumulation; the four quarters meet in LDS
        bf16x2 d0, d1;
        if constexpr (QL) {
          d0 = bf16x2{dq4[0], dq4[1]};
          d1 = bf16x2{dq4[2], dq4[3]};
        } else {
          const bf16x8 dh = (kw & 2) ? df1 : df0;
          d0 = (kw & 1) ? bf16x2{dh[4], dh[5]} : bf16x2{dh[0], dh[1]};
          d1 = (kw & 1) ? bf16x2{dh[6], dh[7]} : bf16x2{dh[2], dh[3]};
        }
        float t0 = __builtin_amdgcn_fdot2_f32_bf16(d0, bf16x2{oq[0], oq[1]}, 0.f, false);
        float t1 = __builtin_amdgcn_fdot2_f32_bf16(d1, bf16x2{oq[2], oq[3]}, 0.f, false);
        t0 = __builtin_amdgcn_fdot2_f32_bf16(d0, bf16x2{lq[0], lq[1]}, t0, false);
        t1 = __builtin_amdgcn_fdot2_f32_bf16(d1, bf16x2{lq[2], lq[3]}, t1, false);
        const float part = group4_sum(t0 + t1);
        if (lg == 0) dred[(qt * 16 + lr) * 4 + kw] = part;
      }
#ifdef XFM_DIAG
      if (DBG && dbe) dbe[1] = wall_clock64();
#endif
      lds_barrier();  // K(b), V(b) have landed; every wave is done with entry b-1 (its K / V buffers, the exchange tiles)
#ifdef XFM_DIAG
      if (DBG && dbe) dbe[2] = wall_clock64();
#endif
      if constexpr (PRE && ACT) {
        const f32x4 dq4 = *reinterpret_cast<const f32x4*>(dred + (qt * 16 + lr) * 4);
        delta = (dq4[0] + dq4[1]) + (dq4[2] + dq4[3]);
        if (kw == 0 && lg == 0 && qvalid) pdelta[stat_off] = delta;
      }
      const bool more = b + 1 < b_end;
      if constexpr (QL) {
        // everything of the next entry is requested HERE, a whole entry ahead of its use: its Q / dO pieces, the small per-lane loads
        // (their registers are free: this entry's went into delta and nlse above), then K / V
        if (more) {
          stage_q(b + 1, cur ^ 1);
          fetch_q(b + 1);
        }
        if constexpr (ACT) {
          const char* qi_ = qimg + cur * QIMG + qt * 2048;
          qf0 = *reinterpret_cast<const bf16x8*>(qi_ + rf0);
          qf1 = *reinterpret_cast<const bf16x8*>(qi_ + rf1);
          df0 = *reinterpret_cast<const bf16x8*>(qi_ + QT * 2048 + rf0);
          df1 = *reinterpret_cast<const bf16x8*>(qi_ + QT * 2048 + rf1);
        }
      }
      // (placing the K / V pieces between the tiles of the score phase instead -- one K + V piece per tile -- measured the same entry period
      // with ~50 more scalar instructions per entry; all of them go out here)
      if (more) stage_kv(b + 1, cur ^ 1);
#ifdef XFM_DIAG
      if (DBG && dbe) dbe[8] = wall_clock64();
#endif

      f32x4 st[NTS], dp[NTS];
      if constexpr (ACT) {
        const char* ka = sK + kt0 * 2048;
        float dpart = 0.f;
        // fragments of tile t + 1 are requested before the MFMAs of tile t (two tiles' worth, 32 VGPRs, in flight)
        bf16x8 fr[2][4];
        auto frags = [&](int t, bf16x8 (&f)[4]) {
          f[0] = *reinterpret_cast<const bf16x8*>(ka + t * 2048 + rf0);
          f[1] = *reinterpret_cast<const bf16x8*>(ka + t * 2048 + rf1);
          f[2] = *reinterpret_cast<const bf16x8*>(ka + 2 * KBUF + t * 2048 + rf0);
          f[3] = *reinterpret_cast<const bf16x8*>(ka + 2 * KBUF + t * 2048 + rf1);
        };
        auto mfmas = [&](int t) {
          st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr[t & 1][0], qf0, bvs[t], 0, 0, 0);
          st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr[t & 1][1], qf1, st[t], 0, 0, 0);
          dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
          dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr[t & 1][2], df0, dp[t], 0, 0, 0);
          dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr[t & 1][3], df1, dp[t], 0, 0, 0);
        };
        if constexpr (PRE) {
          // Software pipeline with scheduling fences between the steps: the K (V) fragments of tile t + 1 are requested as soon as the
          // score (dP) MFMAs of tile t have read theirs (16 VGPRs of fragments), and the exponentials / dS of tile t - 1 are written
          // after the MFMAs of tile t and execute beside them (two tiles of scores live).  A free schedule hoists every read and MFMA
          // to the top and spills the bias tiles, whose reloads (vmcnt) would wait behind the K / V prefetch.
          bf16x8 fk[2], fv[2];
          if constexpr (NT > 0) {
            fk[0] = *reinterpret_cast<const bf16x8*>(ka + rf0);
            fk[1] = *reinterpret_cast<const bf16x8*>(ka + rf1);
            fv[0] = *reinterpret_cast<const bf16x8*>(ka + 2 * KBUF + rf0);
            fv[1] = *reinterpret_cast<const bf16x8*>(ka + 2 * KBUF + rf1);
          }
#pragma unroll
          for (int t = 0; t <= NT; ++t) {
            if (t < NT) {
              st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk[0], qf0, bvs[t], 0, 0, 0);
              st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk[1], qf1, st[t], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              if (t + 1 < NT) {
                fk[0] = *reinterpret_cast<const bf16x8*>(ka + (t + 1) * 2048 + rf0);
                fk[1] = *reinterpret_cast<const bf16x8*>(ka + (t + 1) * 2048 + rf1);
              }
              dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
              dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv[0], df0, dp[t], 0, 0, 0);
              dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv[1], df1, dp[t], 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              if (t + 1 < NT) {
                fv[0] = *reinterpret_cast<const bf16x8*>(ka + 2 * KBUF + (t + 1) * 2048 + rf0);
                fv[1] = *reinterpret_cast<const bf16x8*>(ka + 2 * KBUF + (t + 1) * 2048 + rf1);
              }
            }
            if (t > 0) {
              bf16x4 pk;
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float pv = __builtin_amdgcn_exp2f(fmaf(st[t - 1][r], c2, nlse));
                const float ds = pv * (dp[t - 1][r] - delta);
                dsacc[t - 1][r] += ds;
                pk[r] = f2bf(ds);
              }
              *reinterpret_cast<bf16x4*>(ex_slot(kt0 + t - 1)) = pk;
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        } else {
          if constexpr (NT > 0) frags(0, fr[0]);
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            if (t + 1 < NT) frags(t + 1, fr[(t + 1) & 1]);
            mfmas(t);
            __builtin_amdgcn_sched_barrier(0xF);   // (ALU and MFMA instructions may cross, memory instructions may not)
          }
        }
        if constexpr (!PRE) {
#pragma unroll
          for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float pv = __builtin_amdgcn_exp2f(fmaf(st[t][r], c2, nlse));
              st[t][r] = pv;
              dpart = fmaf(pv, dp[t][r], dpart);
            }
          }
          dpart = group4_sum(dpart);
          if (lg == 0) dred[(qt * 4 + kw) * 16 + lr] = dpart;
        }
      }
#ifdef XFM_DIAG
      if (DBG && dbe) dbe[3] = wall_clock64();
#endif
      if constexpr (!QL) if (more) fetch_q(b + 1);  // (here, not at the top: this entry's fragments are dead now and lend their registers)
      if constexpr (!PRE) {
        lds_barrier();  // delta partials are in
#ifdef XFM_DIAG
        if (DBG && dbe) dbe[4] = wall_clock64();
#endif
        if constexpr (ACT) {
          // delta_i = sum_j P_ij dP_ij from the SAME P and dP that form dS, so that sum_j dS_ij = 0 holds to fp32 rounding
          delta = (dred[(qt * 4 + 0) * 16 + lr] + dred[(qt * 4 + 1) * 16 + lr]) + (dred[(qt * 4 + 2) * 16 + lr] + dred[(qt * 4 + 3) * 16 + lr]);
          if (kw == 0 && lg == 0 && qvalid) pdelta[stat_off] = delta;
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            bf16x4 pk;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float ds = st[t][r] * (dp[t][r] - delta);
              dsacc[t][r] += ds;
              pk[r] = f2bf(ds);
            }
            *reinterpret_cast<bf16x4*>(ex_slot(kt0 + t)) = pk;
          }
        }
      }
#ifdef XFM_DIAG
      if (PRE && DBG && dbe) dbe[4] = wall_clock64();
      if (DBG && dbe) dbe[5] = wall_clock64();
#endif
      lds_barrier();  // the query tile's dS tiles of all keys are in
#ifdef XFM_DIAG
      if (DBG && dbe) dbe[6] = wall_clock64();
#endif
      if constexpr (ACT) {
        // dQ^T[d, q] = sum_keys K^T[d, key] dS^T[key, q] for d-tile kw, two key tiles per MFMA.  Straight-line over NP pairs (tiles past
        // the last one hold zeros) so that the LDS reads of several pairs are in flight together; two chains of dependent MFMAs.
        const char* kb = sK + tro;
        f32x4 acc2[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int s2 = 0; s2 < NP; ++s2) {
          const bf16x8 pf = *reinterpret_cast<const bf16x8*>(ex_q + s2 * 1024);
          union { struct { s16x4 a, b; } s; bf16x8 v; } kf;
          kf.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, kb + (2 * s2) * 2048));
          kf.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, kb + (2 * s2 + 1) * 2048));
          acc2[s2 & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf.v, pf, acc2[s2 & 1], 0, 0, 0);
          if ((s2 & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // four pairs' fragments in flight at a time
        }
        const f32x4 acc = acc2[0] + acc2[1];
#pragma unroll
        for (int r = 0; r < 4; ++r) dq_hold[r] = f2bf(acc[r] * a.scale);
      }
#ifdef XFM_DIAG
      if (DBG && dbe) dbe[7] = wall_clock64();
#endif
      advance();
      pdelta += stat_bs;
      pdq += dq_bs;
    }
  };
  if (!wave_active) walk(std::integral_constant<int, -1>{});
  else switch (nt) {
    case 4: walk(std::integral_constant<int, 4>{}); break;
    case 3: walk(std::integral_constant<int, 3>{}); break;
    case 2: walk(std::integral_constant<int, 2>{}); break;
    case 1: walk(std::integral_constant<int, 1>{}); break;
    default: walk(std::integral_constant<int, 0>{}); break;
  }
  if (qvalid && b_begin < b_end) *reinterpret_cast<bf16x4*>(pdq + dq_off) = dq_hold;

  if (a.dbias != nullptr) {  // flush sum_b dS: a wave-private LDS transpose makes every atomic wave-instruction one run of keys of one row
    __syncthreads();
    float* fl = reinterpret_cast<float*>(lds + w * 4096);  // [16 q][64 keys], aliases the K buffers (done with)
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(fl + lr * 64 + t * 16 + 4 * lg) = dsacc[t];
    __syncthreads();
    if (wave_active && b_begin < b_end) {
      const int kj = kt0 * 16 + lane;
      // a.dbias_ws != NULL (XFM_DETERMINISTIC=1): this batch slice's sums go to its own plane [slice][H][Sq][ld] with plain stores,
      // every column below ld written (zero past the last key), and dbias_reduce_kernel adds the planes in slice order; else one float
      // atomic per element and slice straight into dbias
      float* const plane = a.dbias_ws != nullptr ? a.dbias_ws + ((long)zslice * a.H + h) * sq * a.bias_ld : nullptr;
      for (int row = 0; row < 16; ++row) {
        const int q = q0 + row;
        if (q >= sq || lane >= nt * 16) continue;
        if (plane != nullptr) {
          if (kj < a.bias_ld) plane[(long)q * a.bias_ld + kj] = kj < sk ? fl[row * 64 + lane] : 0.f;
        } else if (kj < sk) {
          atomicAdd(a.dbias + ((long)h * sq + q) * a.bias_ld + kj, fl[row * 64 + lane]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// backward 2/2 for the same short, dense, unmasked problems: dK, dV.  Mirror image of the kernel above: a workgroup is (group of
// <= 3 key tiles, head), its 12 waves are (key tile, query range), and it walks batch entries with Q, dO and the row statistics
// (log-sum-exp, delta) of the NEXT entry landing in second LDS buffers while this one computes.  A wave holds its key tile's K / V
// fragments as the B operands (fetched one entry ahead), computes S and dP for its <= 4 query tiles once, hands P and dS to its
// three sibling waves through LDS (bf16, 8 B per lane and tile) and sums d-tile `qw` of dV^T = dO^T P and dK^T = Q^T dS over all
// queries.  Its bias tile [<= 64 queries x 16 keys] is batch-invariant: 16 VGPRs, loaded once.
// LDS: Q, dO (2 images of 2 NP tiles each) | P, dS exchange (3 x 2 NP tiles x 512 B each) | statistics (2 x 2 x 1 KB).
// NP = query-tile pairs the dK / dV loops run over (tiles past the last query hold zeros in the exchange and finite rows in the
// images): 4 for Sq <= 128, 7 for Sq <= 224 (157 KB of LDS; longer sequences take the general kernel).
// ---------------------------------------------------------------------------------------------
#define VK_KT 3
#define VK_IMG(NP) (2 * (NP) * 2048)
#define VK_EXCH(NP) (VK_KT * 2 * (NP) * 512)
#define VK_LDS(NP) (4 * VK_IMG(NP) + 2 * VK_EXCH(NP) + 4 * 1024)

template <int NP>
__global__ __launch_bounds__(VK_KT * 256) void attn_bwd_dkv_short_kernel(AttnArgs a, int nb_per_block, int G) {
  constexpr int NW = VK_KT * 4, IMG = VK_IMG(NP), EXCH = VK_EXCH(NP), PIECES = 4 * NP;  // 1-KB (8-row) pieces per image
  constexpr int NPC = (PIECES + NW - 1) / NW;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform: see the dQ kernel)
  const int lr = lane & 15, lg = lane >> 4;
  const int ktl = w >> 2, qw = w & 3;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);  // (see the dQ kernel: the groups of one (head, batch slice) share an XCD)
  const int grp = wg % G, h = (wg / G) % a.H, zslice = wg / (G * a.H);
  const int sk = a.Sk, sq = a.Sq;
  const int QTILES = (sq + 15) >> 4;  // query tiles (<= 2 NP), dealt to the four query-range waves as evenly as they go
  const int qb4 = QTILES >> 2, qr4 = QTILES & 3;
  const int nqt = qb4 + (qw < qr4 ? 1 : 0);
  const int qt0 = qw * qb4 + (qw < qr4 ? qw : qr4);
  const int KT = (sk + 15) >> 4;  // key tiles dealt to the G groups the same way
  const int kb_t = KT / G, kr_t = KT % G;
  const int nkt = kb_t + (grp < kr_t ? 1 : 0);
  const int k0 = (grp * kb_t + (grp < kr_t ? grp : kr_t) + ktl) * 16;
  const bool wave_active = ktl < nkt && k0 < sk;
  const int kj = k0 + lr;
  const bool kvalid = wave_active && kj < sk;
  const int kc = kj < sk ? kj : sk - 1;

  char* const sQ0 = lds;                // images: Q0 | Q1 | dO0 | dO1
  char* const exP = lds + 4 * IMG;      // exchange: P | dS
  char* const stat0 = exP + 2 * EXCH;   // statistics: [buffer][lse | delta][256]

  // (see the dQ kernel: one per-lane offset per fragment kind, tiles are immediates)
  const int sw_r = (lr >> 1) & 7;
  const int rf0 = lr * 128 + ((lg ^ sw_r) << 4), rf1 = lr * 128 + (((4 + lg) ^ sw_r) << 4);
  const int tr_row = 4 * lg + (lr >> 2), tr_col = qw * 16 + 4 * (lr & 3);
  const int tro = tr_row * 128 + ((((tr_col >> 3) ^ ((tr_row >> 1) & 7))) << 4) + (tr_col & 7) * 2;
  // P / dS exchange of a key tile: query tiles in PAIRS, 16 B per lane and pair (tile 2p in the low, 2p + 1 in the high 8 bytes): the
  // dK / dV loop reads a pair as ONE ds_read_b128 -- the MFMA operand as it stands -- instead of a ds_read2st64_b64 at half the LDS rate
  const int ex_r = ktl * (2 * NP * 512) + lane * 16;
  auto ex_slot = [&](int tile) { return ex_r + ((tile >> 1) << 10) + ((tile & 1) << 3); };

  for (int i = tid; i < 2 * EXCH / 16; i += NW * 64) reinterpret_cast<u32x4*>(exP)[i] = u32x4{0, 0, 0, 0};  // tiles past the last query stay zero

  const float inv_scale = 1.0f / a.scale, c2 = a.scale * 1.44269504088896341f;
  f32x4 bvs[4];  // (bias[q, key] / scale; -1e30 past the last key or query) for lane (lg, lr): queries 16 t + 4 lg + r, key lr
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qi = (qt0 + t) * 16 + 4 * lg + r;
      float bv = 0.f;
      if (a.bias != nullptr && t < nqt && qi < sq && kj < sk) bv = a.bias[((long)h * sq + qi) * a.bias_ld + kj];
      bvs[t][r] = (qi < sq && kj < sk ? bv : -1.0e30f) * inv_scale;
    }

  const int k_off = (int)(((long)kc * a.k_rs + h * 64 + 8 * lg) * 2), v_off = (int)(((long)kc * a.v_rs + h * 64 + 8 * lg) * 2);
  const int dk_off = (int)(((long)kj * a.dk_rs + h * 64 + qw * 16 + 4 * lg) * 2), dv_off = (int)(((long)kj * a.dv_rs + h * 64 + qw * 16 + 4 * lg) * 2);
  const long k_bs = (long)sk * a.k_rs * 2, v_bs = (long)sk * a.v_rs * 2, dk_bs = (long)sk * a.dk_rs * 2, dv_bs = (long)sk * a.dv_rs * 2;
  const long q_bs = (long)sq * a.q_rs * 2, do_bs = (long)sq * a.do_rs * 2, stat_bs = (long)a.H * a.stat_ld;
  int q_off[NPC], do_off[NPC];
  unsigned pc_dst[NPC];
#pragma unroll
  for (int i = 0; i < NPC; ++i) {
    const int j = w + i * NW;  // piece j: rows 8 j .. 8 j + 7 of the image
    const int r = (j & 7) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ swz_a(r);
    int gr = (j >> 3) * 64 + r;
    gr = gr < sq ? gr : sq - 1;
    q_off[i] = (int)(((long)gr * a.q_rs + h * 64 + c * 8) * 2);
    do_off[i] = (int)(((long)gr * a.do_rs + h * 64 + c * 8) * 2);
    pc_dst[i] = (unsigned)__builtin_amdgcn_readfirstlane(j * 1024);
  }
  // statistics: waves 0..3 stage 64 log-sum-exps each, waves 4..7 64 deltas each (4 B per lane); rows past Sq repeat the last one
  const int st_q = (w & 3) * 64 + lane;
  const int st_src = (int)((long)h * a.stat_ld + (st_q < sq ? st_q : sq - 1)) * 4;
  const unsigned st_dst = (unsigned)__builtin_amdgcn_readfirstlane(((w >> 2) & 1) * 1024 + (w & 3) * 256);
  auto stage_q = [&](int b, int buf) {
    const char* qb = reinterpret_cast<const char*>(a.q) + (long)b * q_bs;
    const char* db = reinterpret_cast<const char*>(a.dout) + (long)b * do_bs;
    const unsigned dq = (unsigned)(uintptr_t)LDS_PTR(void, sQ0) + (unsigned)buf * IMG, dd = dq + 2 * IMG;
#pragma unroll
    for (int i = 0; i < NPC; ++i) {
      if (w + i * NW < PIECES) {  // (inline asm: see stage_rows)
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(qb + q_off[i]), "s"(dq + pc_dst[i]) : "memory", "m0");
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(db + do_off[i]), "s"(dd + pc_dst[i]) : "memory", "m0");
      }
    }
    if (w < 8) {
      const char* sp = reinterpret_cast<const char*>(w < 4 ? a.lse : a.delta) + (long)b * stat_bs * 4 + st_src;
      const unsigned sd = (unsigned)(uintptr_t)LDS_PTR(void, stat0) + (unsigned)buf * 2048 + st_dst;
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(sp), "s"(sd) : "memory", "m0");
    }
  };

  const int b_begin = zslice * nb_per_block;
  int b_end = b_begin + nb_per_block;
  b_end = b_end < a.B ? b_end : a.B;
  bf16x8 kf0, kf1, vf0, vf1;
  auto fetch_k = [&](int b) {
    const char* kp = reinterpret_cast<const char*>(a.k) + (long)b * k_bs + k_off;
    const char* vp = reinterpret_cast<const char*>(a.v) + (long)b * v_bs + v_off;
    kf0 = *reinterpret_cast<const bf16x8*>(kp);
    kf1 = *reinterpret_cast<const bf16x8*>(kp + 64);
    vf0 = *reinterpret_cast<const bf16x8*>(vp);
    vf1 = *reinterpret_cast<const bf16x8*>(vp + 64);
  };
  if (b_begin < b_end) {
    stage_q(b_begin, 0);
    fetch_k(b_begin);
  }
  for (int b = b_begin; b < b_end; ++b) {
    const int cur = (b - b_begin) & 1;
    const char* sQ = sQ0 + cur * IMG;
    const char* sD = sQ + 2 * IMG;
    const float* sL = reinterpret_cast<const float*>(stat0 + cur * 2048);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (see the dQ kernel)
    asm volatile("" : "+v"(kf0), "+v"(kf1), "+v"(vf0), "+v"(vf1));
    lds_barrier();  // Q(b), dO(b), statistics(b) have landed; every wave is done with entry b-1
    if (b + 1 < b_end) stage_q(b + 1, cur ^ 1);

    // (straight-line code per tile count, one scalar branch: see the dQ kernel)
    auto scores = [&](auto NTc) {
      constexpr int NT = decltype(NTc)::value;
      f32x4 st[NT > 0 ? NT : 1], dp[NT > 0 ? NT : 1];
      const char* qa = sQ + qt0 * 2048;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const f32x4 lsv = *reinterpret_cast<const f32x4*>(sL + (qt0 + t) * 16 + 4 * lg);
        dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) st[t][r] = fmaf(-lsv[r], inv_scale, bvs[t][r]);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(qa + t * 2048 + rf0), kf0, st[t], 0, 0, 0);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(qa + t * 2048 + rf1), kf1, st[t], 0, 0, 0);
        dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(qa + 2 * IMG + t * 2048 + rf0), vf0, dp[t], 0, 0, 0);
        dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(qa + 2 * IMG + t * 2048 + rf1), vf1, dp[t], 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const f32x4 dlv = *reinterpret_cast<const f32x4*>(sL + 256 + (qt0 + t) * 16 + 4 * lg);
        bf16x4 pp, ps;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = __builtin_amdgcn_exp2f(st[t][r] * c2);
          pp[r] = f2bf(pv);
          ps[r] = f2bf(pv * (dp[t][r] - dlv[r]));
        }
        *reinterpret_cast<bf16x4*>(exP + ex_slot(qt0 + t)) = pp;
        *reinterpret_cast<bf16x4*>(exP + EXCH + ex_slot(qt0 + t)) = ps;
      }
    };
    if (wave_active) {
      switch (nqt) {
        case 4: scores(std::integral_constant<int, 4>{}); break;
        case 3: scores(std::integral_constant<int, 3>{}); break;
        case 2: scores(std::integral_constant<int, 2>{}); break;
        case 1: scores(std::integral_constant<int, 1>{}); break;
        default: break;
      }
    }
    if (b + 1 < b_end) fetch_k(b + 1);  // (this entry's K / V fragments are dead: the next ones take their registers)
    lds_barrier();  // P and dS of all queries against this key tile are in
    if (wave_active) {
      // dV^T[d, key] = sum_q dO^T[d, q] P[q, key],  dK^T[d, key] = sum_q Q^T[d, q] dS[q, key]  for d-tile qw, two query tiles per MFMA
      const char* qb = sQ + tro;
      f32x4 av[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, ak[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int s2 = 0; s2 < NP; ++s2) {
        union { struct { s16x4 a, b; } s; bf16x8 v; } qf, df;
        const bf16x8 pfv = *reinterpret_cast<const bf16x8*>(exP + ex_r + s2 * 1024);
        const bf16x8 sfv = *reinterpret_cast<const bf16x8*>(exP + EXCH + ex_r + s2 * 1024);
        df.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, qb + 2 * IMG + (2 * s2) * 2048));
        df.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, qb + 2 * IMG + (2 * s2 + 1) * 2048));
        qf.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, qb + (2 * s2) * 2048));
        qf.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, qb + (2 * s2 + 1) * 2048));
        av[s2 & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df.v, pfv, av[s2 & 1], 0, 0, 0);
        ak[s2 & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf.v, sfv, ak[s2 & 1], 0, 0, 0);
        if ((s2 & 1) == 1) __builtin_amdgcn_sched_barrier(0);  // two pairs' fragments in flight at a time
      }
      if (kvalid) {
        bf16x4 ok_, ov_;
#pragma unroll
        for (int r = 0; r < 4; ++r) { ok_[r] = f2bf((ak[0][r] + ak[1][r]) * a.scale); ov_[r] = f2bf(av[0][r] + av[1][r]); }
        *reinterpret_cast<bf16x4*>(reinterpret_cast<char*>(a.dk) + (long)b * dk_bs + dk_off) = ok_;
        *reinterpret_cast<bf16x4*>(reinterpret_cast<char*>(a.dv) + (long)b * dv_bs + dv_off) = ov_;
      }
    }
  }
}

// ---- host side ----
// the pair takes this problem
static bool attn_short_dq_ok(const AttnArgs& a) {
  static const bool short_env = xfm_env_flag("XFM_ATTN_SHORT_BWD", true);  // A/B knob
  return short_env && attn_plain(a) && a.Sk <= 64 * ATTN_RES_MAX && a.q_start == nullptr && a.k_start == nullptr && a.kv_index == nullptr &&
         (a.bias == nullptr || a.bias_ld >= (long)cdiv(a.Sk, 16) * 16) && (a.dbias == nullptr || a.bias_ld >= a.Sk);
}
// workgroups of `groups` (row-tile groups of KT tiles) x heads per batch slice; slices so that one round of <= 256 workgroups covers
// the batch; -> batch entries per slice
static int attn_short_nb(const AttnArgs& a, int rows, int KT, int& groups) {
  groups = cdiv(cdiv(rows, 16), KT);
  int z = 256 / (groups * a.H);
  z = z < 1 ? 1 : (z > a.B ? a.B : z);
  return cdiv(a.B, z);
}
// the dQ kernel: three query tiles (12 waves) per workgroup -- four would need 128-VGPR waves (measured: 40 spilled registers) and
// 161 KB of LDS; -> number of batch slices
static int attn_short_dq_slices(const AttnArgs& a, int& groups, int& nb) {
  nb = attn_short_nb(a, a.Sq, 3, groups);
  return cdiv(a.B, nb);
}
// NP = key-tile pairs the dQ loop runs over
static int attn_short_dq_np(const AttnArgs& a) { return a.Sk <= 128 ? 4 : a.Sk <= 224 ? 7 : 8; }
// the dQ kernel can put its bias gradient into per-slice planes (plain stores; a.dbias_ws) when they cover its rows completely
static bool attn_short_planes_ok(const AttnArgs& a) { return a.bias_ld <= (long)cdiv(a.Sk, 16) * 16; }

template <int NP, bool PRE, bool DBG = false>
static void attn_short_dq_launch(dim3 grid, hipStream_t st, const AttnArgs& a, int nb, int groups, long long* dbg = nullptr) {
  constexpr int lds = PRE && NP <= 7 ? VB_LDS_QL(3, NP) : VB_LDS(3);
#ifdef XFM_DIAG
  lds_launch<attn_bwd_dq_short_kernel<3, NP, PRE, DBG>, lds>(grid, dim3(768), lds, st, a, nb, groups, dbg);   // (DBG = false ignores dbg)
#else
  lds_launch<attn_bwd_dq_short_kernel<3, NP, PRE>, lds>(grid, dim3(768), lds, st, a, nb, groups);
#endif
}
// dQ, delta and the bias gradient: into the planes of a.dbias_ws when there is one, else by float atomics into dbias.
// pre (XFM_ATTN_SHORT_PRE=1, opt-in): the row term delta from dO . (O + O_lo) when the forward kept the low half of O -- one barrier
// and the delta exchange less per entry, Q / dO through LDS, and MEASURED SLOWER (dQ 121 us against 97.5 at B = 128, 197 tokens:
// profiles/round5_attn_short.md), so the exchange form stays the default.  dbg: the stamped instantiation (diagnostic build, NP = 7).
static int launch_attn_bwd_dq_short(const AttnArgs& a, bool pre, int groups, int nb, int slices, hipStream_t st, long long* dbg = nullptr) {
  const dim3 grid(groups * a.H * slices);
  const int np = attn_short_dq_np(a);
#ifdef XFM_DIAG
  if (dbg != nullptr) {
    if (pre) attn_short_dq_launch<7, true, true>(grid, st, a, nb, groups, dbg);
    else attn_short_dq_launch<7, false, true>(grid, st, a, nb, groups, dbg);
  } else
#endif
  if (np == 4) pre ? attn_short_dq_launch<4, true>(grid, st, a, nb, groups) : attn_short_dq_launch<4, false>(grid, st, a, nb, groups);
  else if (np == 7) pre ? attn_short_dq_launch<7, true>(grid, st, a, nb, groups) : attn_short_dq_launch<7, false>(grid, st, a, nb, groups);
  else pre ? attn_short_dq_launch<8, true>(grid, st, a, nb, groups) : attn_short_dq_launch<8, false>(grid, st, a, nb, groups);
  return xfm_check_launch("attn_bwd_dq");
}

// the dK/dV kernel: the preconditions of the dQ kernel and Sq <= 224 (bounded by the LDS images)
static int launch_attn_bwd_dkv_short(const AttnArgs& a, hipStream_t st) {
  int groups;
  const int nb = attn_short_nb(a, a.Sk, VK_KT, groups);
  const dim3 grid(groups * a.H * cdiv(a.B, nb)), blk(VK_KT * 256);
  if (a.Sq <= 128) lds_launch<attn_bwd_dkv_short_kernel<4>, VK_LDS(4)>(grid, blk, VK_LDS(4), st, a, nb, groups);
  else lds_launch<attn_bwd_dkv_short_kernel<7>, VK_LDS(7)>(grid, blk, VK_LDS(7), st, a, nb, groups);
  return xfm_check_launch("attn_bwd_dkv_short");
}
