// Grouped cross-attention (one workgroup per key/value source and head), its streamed-key pair for Sk > 256, and the packed
// small self-attention forward that shares the wave layout: the xattn_* kernels and their launches.  Included by attention.hip.
// ---------------------------------------------------------------------------------------------
// Grouped cross-attention (fusion towers: Sq = 30 text queries against Sk = 197 image tokens, xroberta.py:201-289 with
// encoder_hidden_states).  Several query batch rows read the SAME key/value source (XFM's ITM negatives and MLM pass reuse
// the batch's images, xfm.py:749-802), so a workgroup is one (source, head): K/V are staged once and stay LDS-resident
// while the 8 waves walk every (row, 16-query tile) of the group; dK/dV are accumulated over the group's rows in
// registers and written once per SOURCE (no per-row copies, no fold pass).  group g = rows grp_rows[grp_start[g] ..
// grp_start[g+1]) and reads source g.  Sq <= 64, Sk <= 256, no additive bias, no causal mask.
// ---------------------------------------------------------------------------------------------
// PACK: the same wave layout serves small self-attention (Sq, Sk <= 64, e.g. the 30-token text rows): a workgroup takes nw/tq
// CONSECUTIVE batch rows, each with its own key/value source in its own LDS slot -- 8 waves per workgroup instead of 2.
// MASK / DROP (grouped mode only; the packed mode keeps its run-time switches): key-keep flags / dropout present.  Grouped mode works in
// the exponent of 2 like its backward kernels: scores scaled by scale*log2(e), the key's additive term (mask, past-the-end) from an LDS
// vector.
template <bool PACK, bool MASK, bool DROP>
__global__ __launch_bounds__(512, 4) void xattn_fwd_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int g = blockIdx.z, h = blockIdx.y;
  const int tq = (a.Sq + 15) / 16, rpp = nw / tq;  // waves per row, rows per pass
  int rstart, nrows;
  if (PACK) {
    rstart = g * rpp;
    nrows = a.B - rstart < rpp ? a.B - rstart : rpp;
  } else {
    rstart = a.grp_start[g];
    nrows = a.grp_start[g + 1] - rstart;
  }
  if (nrows <= 0) return;  // uniform: before any barrier
  const int nchunks = PACK ? 1 : (a.Sk + 63) / 64;
  if (PACK) {
    // the (start, length) pairs of the <= ATTN_RES_MAX rows first, so their scalar loads overlap instead of one load -> stage
    // chain per row
    long kb_[ATTN_RES_MAX];
    int sk_[ATTN_RES_MAX];
#pragma unroll
    for (int jj = 0; jj < ATTN_RES_MAX; ++jj) {
      const int row = rstart + (jj < nrows ? jj : 0);
      const int src = a.kv_index ? a.kv_index[row] : row;
      k_seq(a, src, kb_[jj], sk_[jj]);
    }
#pragma unroll
    for (int jj = 0; jj < ATTN_RES_MAX; ++jj)
      if (jj < nrows)
        stage_slot(lds + jj * ATTN_SLOT, a.k + kb_[jj] * a.k_rs + h * 64, a.k_rs, a.v + kb_[jj] * a.v_rs + h * 64, a.v_rs, 0, sk_[jj], w, nw, lane);
  } else {
    const bf16* kb = a.k + (long)g * a.Sk * a.k_rs + h * 64;
    const bf16* vb = a.v + (long)g * a.Sk * a.v_rs + h * 64;
    for (int kc = 0; kc < nchunks; ++kc) stage_slot(lds + kc * ATTN_SLOT, kb, a.k_rs, vb, a.v_rs, kc * 64, a.Sk, w, nw, lane);
  }
  constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
  float* madd = reinterpret_cast<float*>(lds + nchunks * ATTN_SLOT);  // grouped + MASK: see xattn_dq_kernel
  if (!PACK && tid < nchunks * 64)
    madd[tid] = tid < a.Sk ? (MASK && a.key_keep[(long)g * a.Sk + tid] == 0 ? MASK_NEG * LOG2E : 0.f) : -3.0e38f;
  stage_wait();
  const int jr = w / tq, tile = w - jr * tq;
  const bool has_mask = a.key_keep != nullptr;
  const float c2 = a.scale * LOG2E;
  const bool causal = PACK && a.causal != 0;
  if (jr >= rpp) return;  // no barriers below
  for (int j = jr; j < nrows; j += rpp) {
    const int b = PACK ? rstart + j : a.grp_rows[rstart + j];
    const int kvb = PACK ? (a.kv_index ? a.kv_index[b] : b) : g;
    long qbase, kbase_unused;
    int sq, sk = a.Sk;
    q_seq(a, b, qbase, sq);
    if (tile * 16 >= sq) continue;  // packed rows: this 16-query tile lies past the sequence's end (wave-uniform, no barrier below)
    if (PACK) k_seq(a, kvb, kbase_unused, sk);
    const int qi = tile * 16 + lr;
    const int qc = qi < sq ? qi : sq - 1;
    const uint32_t dkey = drop_key(a, b, h, qi);
    const bf16* qp = a.q + (qbase + qc) * a.q_rs + h * 64;
    const bf16x8 qf0 = *reinterpret_cast<const bf16x8*>(qp + 8 * lg);
    const bf16x8 qf1 = *reinterpret_cast<const bf16x8*>(qp + 32 + 8 * lg);
    f32x4 oacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) oacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = EXCL_NEG, l_run = 0.f;
    for (int kc = 0; kc < nchunks; ++kc) {
      const char* sK = lds + (PACK ? j : kc) * ATTN_SLOT;
      const char* sV = sK + ATTN_TILE;
      f32x4 st[4];
      int kk[4][4];
      if (PACK && has_mask) load_keep(a, kvb, kc, lg, kk);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, t * 16, 0, lr, lg), qf0, st[t], 0, 0, 0);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, t * 16, 1, lr, lg), qf1, st[t], 0, 0, 0);
      }
      float mx = EXCL_NEG;
      if constexpr (!PACK) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const f32x4 ma = *reinterpret_cast<const f32x4*>(madd + kc * 64 + t * 16 + 4 * lg);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            st[t][r] = fmaf(st[t][r], c2, ma[r]);
            mx = fmaxf(mx, st[t][r]);
          }
        }
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            st[t][r] = score_masked(a, st[t][r], 0.f, has_mask, has_mask ? kk[t][r] : 1, causal, qi, kc * 64 + t * 16 + 4 * lg + r, sk);
            mx = fmaxf(mx, st[t][r]);
          }
      }
      mx = group4_max(mx);
      const float m_new = fmaxf(m_run, mx);
      const float alpha = PACK ? __expf(m_run - m_new) : __builtin_amdgcn_exp2f(m_run - m_new);
      float psum = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          st[t][r] = PACK ? __expf(st[t][r] - m_new) : __builtin_amdgcn_exp2f(st[t][r] - m_new);
          psum += st[t][r];
        }
      if (PACK ? a.drop_thresh != 0u : DROP) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            st[t][r] = drop_keep(a, dkey, kc * 64 + t * 16 + 4 * lg + r) ? st[t][r] * a.drop_scale : 0.f;
      }
      psum = group4_sum(psum);
      l_run = l_run * alpha + psum;
      m_run = m_new;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) oacc[dt][r] *= alpha;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pf = pack_pair(st[2 * s2], st[2 * s2 + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sV, 32 * s2, 32 * s2 + 16, dt * 16, lr, lg), pf, oacc[dt], 0, 0, 0);
      }
    }
    if (qi < sq) {
      store_out(a, qbase + qi, h, lg, oacc, 1.0f / l_run);
      if (lg == 0) a.lse[((long)b * a.H + h) * a.stat_ld + qi] = PACK ? m_run + __logf(l_run) : m_run * LN2 + __logf(l_run);
    }
  }
}

// MASK / DROP: key-keep flags / dropout present (compiled out otherwise: the packed fusion tower has dropout and no mask).  The
// probabilities are taken in the exponent of 2 (one FMA with scale*log2(e) and -lse*log2(e) + the key's additive term, then v_exp), and
// the dropout decisions of the first sweep (delta) are kept as 16 bits per chunk and
// lane for the second (dS): the counter hash -- two quarter-rate integer multiplies per score -- was half of this kernel's VALU time.
template <bool MASK, bool DROP>
__global__ __launch_bounds__(512, 4) void xattn_dq_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int g = blockIdx.z, h = blockIdx.y;
  const int rstart = a.grp_start[g], nrows = a.grp_start[g + 1] - rstart;
  if (nrows <= 0) return;
  const int kvb = g;
  const bf16* kb = a.k + (long)kvb * a.Sk * a.k_rs + h * 64;
  const bf16* vb = a.v + (long)kvb * a.Sk * a.v_rs + h * 64;
  const int nchunks = (a.Sk + 63) / 64;
  constexpr float LOG2E = 1.4426950408889634f;
  for (int kc = 0; kc < nchunks; ++kc) stage_slot(lds + kc * ATTN_SLOT, kb, a.k_rs, vb, a.v_rs, kc * 64, a.Sk, w, nw, lane);
  // what a key adds to every score of its column, in the exponent of 2 (-10000 when masked, "minus infinity" past the last key), once
  // per workgroup in LDS behind the K / V slots: one ds_read_b128 + 4 adds per 16-key tile instead of 16 mask registers and selects
  float* madd = reinterpret_cast<float*>(lds + nchunks * ATTN_SLOT);
  if (tid < nchunks * 64)
    madd[tid] = tid < a.Sk ? (MASK && a.key_keep[(long)kvb * a.Sk + tid] == 0 ? MASK_NEG * LOG2E : 0.f) : -3.0e38f;
  stage_wait();
  const int tq = (a.Sq + 15) / 16, rpp = nw / tq;
  const int jr = w / tq, tile = w - jr * tq;
  if (jr >= rpp) return;
  const float c2 = a.scale * LOG2E;
  for (int j = jr; j < nrows; j += rpp) {
    const int b = a.grp_rows[rstart + j];
    long qbase;
    int sq;
    q_seq(a, b, qbase, sq);
    if (tile * 16 >= sq) continue;  // nothing of this tile belongs to the sequence
    const int qi = tile * 16 + lr;
    const bool qvalid = qi < sq;
    const int qc = qvalid ? qi : sq - 1;
    const uint32_t dkey = DROP ? drop_key(a, b, h, qi) : 0u;
    const bf16* qp = a.q + (qbase + qc) * a.q_rs + h * 64;
    const bf16* dop = a.dout + (qbase + qc) * a.do_rs + h * 64;
    const bf16x8 qf0 = *reinterpret_cast<const bf16x8*>(qp + 8 * lg);
    const bf16x8 qf1 = *reinterpret_cast<const bf16x8*>(qp + 32 + 8 * lg);
    const bf16x8 df0 = *reinterpret_cast<const bf16x8*>(dop + 8 * lg);
    const bf16x8 df1 = *reinterpret_cast<const bf16x8*>(dop + 32 + 8 * lg);
    const long stat_idx = ((long)b * a.H + h) * a.stat_ld + qc;
    const float nlse2 = qvalid ? -a.lse[stat_idx] * LOG2E : -3.0e38f;   // rows past the sequence: every probability 0
    uint32_t keep_lo = 0u, keep_hi = 0u;  // dropout decisions of chunks 0,1 / 2,3: bit (t*4 + r) of the 16-bit field (kc & 1)
    // FIRST: the sweep that draws the dropout decisions (and stores them); later sweeps read them back
    auto probs = [&](int kc, f32x4 (&st)[4], f32x4 (&dp)[4], bool first) {
      const char* sK = lds + kc * ATTN_SLOT;
      const char* sV = sK + ATTN_TILE;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, t * 16, 0, lr, lg), qf0, st[t], 0, 0, 0);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, t * 16, 1, lr, lg), qf1, st[t], 0, 0, 0);
        dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sV, t * 16, 0, lr, lg), df0, dp[t], 0, 0, 0);
        dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sV, t * 16, 1, lr, lg), df1, dp[t], 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 ma = *reinterpret_cast<const f32x4*>(madd + kc * 64 + t * 16 + 4 * lg);
#pragma unroll
        for (int r = 0; r < 4; ++r) st[t][r] = __builtin_amdgcn_exp2f(fmaf(st[t][r], c2, nlse2 + ma[r]));
      }
      if (DROP) {
        const int sh = (kc & 1) * 16;
        uint32_t bits;
        if (first) {
          bits = 0u;
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) bits |= drop_keep(a, dkey, kc * 64 + t * 16 + 4 * lg + r) ? (1u << (t * 4 + r)) : 0u;
          if (kc < 2) keep_lo |= bits << sh;
          else keep_hi |= bits << sh;
        } else {
          bits = (kc < 2 ? keep_lo : keep_hi) >> sh;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) dp[t][r] = (bits & (1u << (t * 4 + r))) ? dp[t][r] * a.drop_scale : 0.f;
      }
    };
    float delta = 0.f;
    f32x4 st[4], dp[4];
    const bool fast_delta = a.o_lo != nullptr;
    if (fast_delta) {
      delta = delta_from_out(a, qbase + qc, h, lg, df0, df1);
    } else {
      for (int kc = 0; kc < nchunks; ++kc) {
        probs(kc, st, dp, true);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) delta += st[t][r] * dp[t][r];
      }
      delta = group4_sum(delta);
    }
    if (qvalid && lg == 0) a.delta[stat_idx] = delta;
    f32x4 dqacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) dqacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < nchunks; ++kc) {
      if (nchunks > 1 || fast_delta) probs(kc, st, dp, fast_delta);
      const char* sK = lds + kc * ATTN_SLOT;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[t][r] = st[t][r] * (dp[t][r] - delta);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pf = pack_pair(st[2 * s2], st[2 * s2 + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          dqacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sK, 32 * s2, 32 * s2 + 16, dt * 16, lr, lg), pf, dqacc[dt], 0, 0, 0);
      }
    }
    if (qvalid) {
      bf16* dqp = a.dq + (qbase + qi) * a.dq_rs + h * 64;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        bf16x4 ov;
#pragma unroll
        for (int r = 0; r < 4; ++r) ov[r] = f2bf(dqacc[dt][r] * a.scale);
        *reinterpret_cast<bf16x4*>(dqp + dt * 16 + 4 * lg) = ov;
      }
    }
  }
}

// dK/dV of one (source, head): wave w owns 16 keys; the group's rows go through LDS four at a time (one 64-slot query chunk
// per row, Sq <= 64), gradients accumulate in registers across ALL rows and are written once, at the source's rows.
// DROP: the dropout stream is keyed per query row (two hash rounds) and a lane walks query rows here, so the row keys of the staged
// sequences are computed once per workgroup into LDS (behind the query slots) instead of once per score; probabilities in the
// exponent of 2 as in the dQ kernel.
template <bool DROP>
__global__ __launch_bounds__(1024) void xattn_dkv_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int g = blockIdx.z, h = blockIdx.y;
  const int rstart = a.grp_start[g], nrows = a.grp_start[g + 1] - rstart;
  const int kvb = g;
  const int k0 = (blockIdx.x * nw + w) * 16;
  const bool wave_active = k0 < a.Sk;
  const int kj = k0 + lr;
  const bool kvalid = kj < a.Sk;
  const int kcl = kvalid ? kj : a.Sk - 1;
  const bf16* kp = a.k + ((long)kvb * a.Sk + kcl) * a.k_rs + h * 64;
  const bf16* vp = a.v + ((long)kvb * a.Sk + kcl) * a.v_rs + h * 64;
  const bf16x8 kf0 = *reinterpret_cast<const bf16x8*>(kp + 8 * lg);
  const bf16x8 kf1 = *reinterpret_cast<const bf16x8*>(kp + 32 + 8 * lg);
  const bf16x8 vf0 = *reinterpret_cast<const bf16x8*>(vp + 8 * lg);
  const bf16x8 vf1 = *reinterpret_cast<const bf16x8*>(vp + 32 + 8 * lg);
  constexpr float LOG2E = 1.4426950408889634f;
  const float c2 = a.scale * LOG2E;
  // what this lane's key adds to its scores in the exponent of 2: -10000 when masked, "minus infinity" for a lane past the last key
  const float key_add2 = !kvalid ? -3.0e38f : (a.key_keep != nullptr && a.key_keep[(long)kvb * a.Sk + kcl] == 0) ? MASK_NEG * LOG2E : 0.f;
  // per staged sequence and query row, behind the query slots: dropout row key | -lse * log2(e) | delta  ([ATTN_RES_MAX][64] each)
  uint32_t* rowkeys = reinterpret_cast<uint32_t*>(lds + ATTN_RES_MAX * ATTN_SLOT);
  float* nlse2s = reinterpret_cast<float*>(rowkeys + ATTN_RES_MAX * 64);
  float* deltas = nlse2s + ATTN_RES_MAX * 64;
  f32x4 dkacc[4], dvacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { dkacc[i] = f32x4{0.f, 0.f, 0.f, 0.f}; dvacc[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  for (int j0 = 0; j0 < nrows; j0 += ATTN_RES_MAX) {  // nrows is workgroup-uniform: every wave takes the same barriers
    const int nb = nrows - j0 < ATTN_RES_MAX ? nrows - j0 : ATTN_RES_MAX;
    __syncthreads();  // readers of the previous batch are done
    for (int jj = 0; jj < nb; ++jj) {
      const int b = a.grp_rows[rstart + j0 + jj];
      long qbase;
      int sq;
      q_seq(a, b, qbase, sq);
      stage_slot(lds + jj * ATTN_SLOT, a.q + qbase * a.q_rs + h * 64, a.q_rs, a.dout + qbase * a.do_rs + h * 64, a.do_rs, 0, sq, w, nw, lane);
    }
    if (tid < nb * 64) {
      const int jj = tid >> 6, qi = tid & 63;
      const int b = a.grp_rows[rstart + j0 + jj];
      if (DROP) rowkeys[tid] = drop_key(a, b, h, qi);
      const long si = ((long)b * a.H + h) * a.stat_ld + qi;
      nlse2s[tid] = qi < a.Sq ? a.lse[si] * -LOG2E : 0.f;
      deltas[tid] = qi < a.Sq ? a.delta[si] : 0.f;
    }
    stage_wait();
    if (!wave_active) continue;
    for (int jj = 0; jj < nb; ++jj) {
      const int b = a.grp_rows[rstart + j0 + jj];
      const char* sQ = lds + jj * ATTN_SLOT;
      const char* sD = sQ + ATTN_TILE;
      const int sq = a.q_len != nullptr ? a.q_len[b] : a.Sq;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        if (s2 * 32 >= a.Sq) continue;  // uniform: no query in this half (Sq = 30 lives in the first)
        f32x4 st[2], pd[2];
        if (s2 * 32 >= sq) continue;  // uniform per row: the whole 32-query step lies past the sequence's end
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int t = 2 * s2 + u;
          const int qi0 = t * 16 + 4 * lg;
          st[u] = f32x4{0.f, 0.f, 0.f, 0.f};
          f32x4 dpu = f32x4{0.f, 0.f, 0.f, 0.f};
          if (t * 16 < sq) {  // (an empty second tile contributes zero probabilities below: skip its four products)
            st[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sQ, t * 16, 0, lr, lg), kf0, st[u], 0, 0, 0);
            st[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sQ, t * 16, 1, lr, lg), kf1, st[u], 0, 0, 0);
            dpu = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sD, t * 16, 0, lr, lg), vf0, dpu, 0, 0, 0);
            dpu = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sD, t * 16, 1, lr, lg), vf1, dpu, 0, 0, 0);
          }
          u32x4 rk = u32x4{0u, 0u, 0u, 0u};
          if (DROP) rk = *reinterpret_cast<const u32x4*>(rowkeys + jj * 64 + qi0);
          const f32x4 nl = *reinterpret_cast<const f32x4*>(nlse2s + jj * 64 + qi0);
          const f32x4 dlv = *reinterpret_cast<const f32x4*>(deltas + jj * 64 + qi0);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool ok = qi0 + r < sq;
            float pv = __builtin_amdgcn_exp2f(fmaf(st[u][r], c2, nl[r] + key_add2));
            pv = ok ? pv : 0.f;
            const float dl = ok ? dlv[r] : 0.f;
            float keepf = 1.f;
            if (DROP) keepf = rng_keep(rng_u32(rk[r], (uint32_t)kj), a.drop_thresh) ? a.drop_scale : 0.f;
            pd[u][r] = pv * keepf;
            st[u][r] = pv * (dpu[r] * keepf - dl);
          }
        }
        const bf16x8 pf = pack_pair(pd[0], pd[1]);
        const bf16x8 sf = pack_pair(st[0], st[1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dvacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sD, 32 * s2, 32 * s2 + 16, dt * 16, lr, lg), pf, dvacc[dt], 0, 0, 0);
          dkacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sQ, 32 * s2, 32 * s2 + 16, dt * 16, lr, lg), sf, dkacc[dt], 0, 0, 0);
        }
      }
    }
  }
  if (!wave_active || !kvalid) return;
  bf16* dkp = a.dk + ((long)kvb * a.Sk + kj) * a.dk_rs + h * 64;  // per SOURCE (zeros when the group is empty)
  bf16* dvp = a.dv + ((long)kvb * a.Sk + kj) * a.dv_rs + h * 64;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    bf16x4 ok_, ov_;
#pragma unroll
    for (int r = 0; r < 4; ++r) { ok_[r] = f2bf(dkacc[dt][r] * a.scale); ov_[r] = f2bf(dvacc[dt][r]); }
    *reinterpret_cast<bf16x4*>(dkp + dt * 16 + 4 * lg) = ok_;
    *reinterpret_cast<bf16x4*>(dvp + dt * 16 + 4 * lg) = ov_;
  }
}

// ---------------------------------------------------------------------------------------------
// Grouped cross-attention with STREAMED keys (Sk > 256: the 577 image tokens of 384-px retrieval fine-tuning, the 901 of 480-px VQA,
// model_retrieval.py:25-36, model_generation.py:93-130): the image's K / V no longer fit LDS whole, so the 64-key chunks go through a
// two-slot ring and the chunk loop is the OUTER one -- every (row, 16-query tile) of the group keeps its running maximum, sum and
// output (forward) or its dQ (backward) in registers across the chunks, up to XS_SLOTS per wave; a group with more than 8 * XS_SLOTS
// tiles takes another pass over the chunks.  One workgroup per (source, head), 32 KB of LDS: several workgroups share a CU and cover
// each other's staging.  dK / dV come from xattn_dkv_kernel above, which already walks any number of keys.
// ---------------------------------------------------------------------------------------------
#define XS_SLOTS 2
#define XS_RING 3   // K | V chunks of 64 keys in a 3-slot ring filled by inline-asm direct-to-LDS loads (round 4; two slots + the
// compiler-visible builtin before: hipcc drains a visible LDS-DMA in front of every LDS read, so each chunk paid its whole fetch latency)
// this wave's two 1-KiB pieces (rows 8 w .. 8 w + 7 of the K tile and of the V tile) of chunk kc -> ring slot kc mod 3 (8 waves)
__device__ __forceinline__ void xs_stage(char* lds, const bf16* kb, long k_rs, const bf16* vb, long v_rs, int kc, int sk, int w, int lane) {
  char* slot = lds + (kc % XS_RING) * ATTN_SLOT;
  const int r = w * 8 + (lane >> 3);
  const int c = (lane & 7) ^ swz_a(r);
  int gr = kc * 64 + r;
  gr = gr < sk ? gr : sk - 1;
  const bf16* s0 = kb + (long)gr * k_rs + c * 8;
  const bf16* s1 = vb + (long)gr * v_rs + c * 8;
  const unsigned d0 = (unsigned)(uintptr_t)LDS_PTR(void, slot) + (unsigned)__builtin_amdgcn_readfirstlane(w * 1024);
  lds_dma16(s0, d0);
  lds_dma16(s1, d0 + (unsigned)ATTN_TILE);
}
__global__ __launch_bounds__(512, 2) void xattn_fwd_stream_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int g = blockIdx.z, h = blockIdx.y;
  const int rstart = a.grp_start[g], nrows = a.grp_start[g + 1] - rstart;
  if (nrows <= 0) return;
  const int tq = (a.Sq + 15) / 16, n_slots = nrows * tq, nchunks = (a.Sk + 63) / 64;
  const bf16* kb = a.k + (long)g * a.Sk * a.k_rs + h * 64;
  const bf16* vb = a.v + (long)g * a.Sk * a.v_rs + h * 64;
  const bool has_mask = a.key_keep != nullptr;
  for (int base = 0; base < n_slots; base += nw * XS_SLOTS) {   // workgroup-uniform: every wave takes the same barriers
    bf16x8 qf[XS_SLOTS][2];
    f32x4 oacc[XS_SLOTS][4];
    float m_run[XS_SLOTS], l_run[XS_SLOTS];
    int qi_[XS_SLOTS], sq_[XS_SLOTS], b_[XS_SLOTS];
    long qb_[XS_SLOTS];
    uint32_t dkey[XS_SLOTS];
    bool ok[XS_SLOTS];
#pragma unroll
    for (int i = 0; i < XS_SLOTS; ++i) {
      const int s = base + w + nw * i;
      const int j = s / tq, tile = s - j * tq;
      ok[i] = s < n_slots;
      b_[i] = a.grp_rows[rstart + (ok[i] ? j : 0)];
      q_seq(a, b_[i], qb_[i], sq_[i]);
      ok[i] = ok[i] && tile * 16 < sq_[i];
      qi_[i] = tile * 16 + lr;
      const int qc = qi_[i] < sq_[i] ? qi_[i] : sq_[i] - 1;
      const bf16* qp = a.q + (qb_[i] + qc) * a.q_rs + h * 64;
      qf[i][0] = *reinterpret_cast<const bf16x8*>(qp + 8 * lg);
      qf[i][1] = *reinterpret_cast<const bf16x8*>(qp + 32 + 8 * lg);
      dkey[i] = drop_key(a, b_[i], h, qi_[i]);
      m_run[i] = EXCL_NEG;
      l_run[i] = 0.f;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) oacc[i][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // (the compiler's wait for the fragments above lands here, not inside the chunk loop where it would drain the ring)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < XS_SLOTS; ++i) asm volatile("" : "+v"(qf[i][0]), "+v"(qf[i][1]));
    xs_stage(lds, kb, a.k_rs, vb, a.v_rs, 0, a.Sk, w, lane);
    if (nchunks > 1) xs_stage(lds, kb, a.k_rs, vb, a.v_rs, 1, a.Sk, w, lane);
    for (int kc = 0; kc < nchunks; ++kc) {
      wait_vm(kc + 1 < nchunks ? 2 : 0);  // this wave's pieces of chunk kc are in (chunk kc + 1 may still fly)
      raw_barrier();                          // ... everyone's; everyone is done with chunk kc - 1, whose slot chunk kc + 2 takes
      if (kc + 2 < nchunks) xs_stage(lds, kb, a.k_rs, vb, a.v_rs, kc + 2, a.Sk, w, lane);
      const char* sK = lds + (kc % XS_RING) * ATTN_SLOT;
      const char* sV = sK + ATTN_TILE;
      int kk[4][4];
      if (has_mask) load_keep(a, g, kc, lg, kk);
#pragma unroll
      for (int i = 0; i < XS_SLOTS; ++i) {
        if (!ok[i]) continue;   // wave-uniform
        f32x4 st[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
          st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, t * 16, 0, lr, lg), qf[i][0], st[t], 0, 0, 0);
          st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, t * 16, 1, lr, lg), qf[i][1], st[t], 0, 0, 0);
        }
        float mx = EXCL_NEG;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            st[t][r] = score_masked(a, st[t][r], 0.f, has_mask, has_mask ? kk[t][r] : 1, false, qi_[i], kc * 64 + t * 16 + 4 * lg + r, a.Sk);
            mx = fmaxf(mx, st[t][r]);
          }
        mx = group4_max(mx);
        const float m_new = fmaxf(m_run[i], mx);
        const float alpha = __expf(m_run[i] - m_new);
        float psum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            st[t][r] = __expf(st[t][r] - m_new);
            psum += st[t][r];
          }
        if (a.drop_thresh != 0u) {
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              st[t][r] = drop_keep(a, dkey[i], kc * 64 + t * 16 + 4 * lg + r) ? st[t][r] * a.drop_scale : 0.f;
        }
        psum = group4_sum(psum);
        l_run[i] = l_run[i] * alpha + psum;
        m_run[i] = m_new;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r) oacc[i][dt][r] *= alpha;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const bf16x8 pf = pack_pair(st[2 * s2], st[2 * s2 + 1]);
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
            oacc[i][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sV, 32 * s2, 32 * s2 + 16, dt * 16, lr, lg), pf, oacc[i][dt], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < XS_SLOTS; ++i) {
      if (ok[i] && qi_[i] < sq_[i]) {
        store_out(a, qb_[i] + qi_[i], h, lg, oacc[i], 1.0f / l_run[i]);
        if (lg == 0) a.lse[((long)b_[i] * a.H + h) * a.stat_ld + qi_[i]] = m_run[i] + __logf(l_run[i]);
      }
    }
    __syncthreads();  // the next pass refills the ring
  }
}

// dQ (and delta) with streamed keys: two sweeps over the chunks per pass -- delta_i = sum_j P_ij dP_ij first (the exact two-pass form
// of the kernels above), then dS and dQ -- unless the forward left o_lo (one sweep).
__global__ __launch_bounds__(512, 2) void xattn_dq_stream_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), nw = blockDim.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int g = blockIdx.z, h = blockIdx.y;
  const int rstart = a.grp_start[g], nrows = a.grp_start[g + 1] - rstart;
  if (nrows <= 0) return;
  const int tq = (a.Sq + 15) / 16, n_slots = nrows * tq, nchunks = (a.Sk + 63) / 64;
  const bf16* kb = a.k + (long)g * a.Sk * a.k_rs + h * 64;
  const bf16* vb = a.v + (long)g * a.Sk * a.v_rs + h * 64;
  const bool has_mask = a.key_keep != nullptr;
  const bool fast_delta = a.o_lo != nullptr;
  for (int base = 0; base < n_slots; base += nw * XS_SLOTS) {
    bf16x8 qf[XS_SLOTS][2], df[XS_SLOTS][2];
    f32x4 dqacc[XS_SLOTS][4];
    float lse_q[XS_SLOTS], delta[XS_SLOTS];
    int qi_[XS_SLOTS], sq_[XS_SLOTS];
    long qb_[XS_SLOTS], stat_[XS_SLOTS];
    uint32_t dkey[XS_SLOTS];
    bool ok[XS_SLOTS];
#pragma unroll
    for (int i = 0; i < XS_SLOTS; ++i) {
      const int s = base + w + nw * i;
      const int j = s / tq, tile = s - j * tq;
      ok[i] = s < n_slots;
      const int b = a.grp_rows[rstart + (ok[i] ? j : 0)];
      q_seq(a, b, qb_[i], sq_[i]);
      ok[i] = ok[i] && tile * 16 < sq_[i];
      qi_[i] = tile * 16 + lr;
      const bool qvalid = qi_[i] < sq_[i];
      const int qc = qvalid ? qi_[i] : sq_[i] - 1;
      const bf16* qp = a.q + (qb_[i] + qc) * a.q_rs + h * 64;
      const bf16* dop = a.dout + (qb_[i] + qc) * a.do_rs + h * 64;
      qf[i][0] = *reinterpret_cast<const bf16x8*>(qp + 8 * lg);
      qf[i][1] = *reinterpret_cast<const bf16x8*>(qp + 32 + 8 * lg);
      df[i][0] = *reinterpret_cast<const bf16x8*>(dop + 8 * lg);
      df[i][1] = *reinterpret_cast<const bf16x8*>(dop + 32 + 8 * lg);
      stat_[i] = ((long)b * a.H + h) * a.stat_ld + qc;
      lse_q[i] = qvalid ? a.lse[stat_[i]] : 3.0e38f;
      dkey[i] = drop_key(a, b, h, qi_[i]);
      delta[i] = 0.f;
      if (fast_delta && ok[i]) delta[i] = delta_from_out(a, qb_[i] + qc, h, lg, df[i][0], df[i][1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) dqacc[i][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (see the forward kernel)
#pragma unroll
    for (int i = 0; i < XS_SLOTS; ++i)
      asm volatile("" : "+v"(qf[i][0]), "+v"(qf[i][1]), "+v"(df[i][0]), "+v"(df[i][1]), "+v"(lse_q[i]), "+v"(delta[i]));
    for (int sweep = fast_delta ? 1 : 0; sweep < 2; ++sweep) {
      xs_stage(lds, kb, a.k_rs, vb, a.v_rs, 0, a.Sk, w, lane);
      if (nchunks > 1) xs_stage(lds, kb, a.k_rs, vb, a.v_rs, 1, a.Sk, w, lane);
      for (int kc = 0; kc < nchunks; ++kc) {
        wait_vm(kc + 1 < nchunks ? 2 : 0);
        raw_barrier();
        if (kc + 2 < nchunks) xs_stage(lds, kb, a.k_rs, vb, a.v_rs, kc + 2, a.Sk, w, lane);
        const char* sK = lds + (kc % XS_RING) * ATTN_SLOT;
        const char* sV = sK + ATTN_TILE;
        int kk[4][4];
        if (has_mask) load_keep(a, g, kc, lg, kk);
#pragma unroll
        for (int i = 0; i < XS_SLOTS; ++i) {
          if (!ok[i]) continue;
          f32x4 st[4], dp[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, t * 16, 0, lr, lg), qf[i][0], st[t], 0, 0, 0);
            st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, t * 16, 1, lr, lg), qf[i][1], st[t], 0, 0, 0);
            dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sV, t * 16, 0, lr, lg), df[i][0], dp[t], 0, 0, 0);
            dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sV, t * 16, 1, lr, lg), df[i][1], dp[t], 0, 0, 0);
          }
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              st[t][r] = __expf(score_masked(a, st[t][r], 0.f, has_mask, has_mask ? kk[t][r] : 1, false, qi_[i], kc * 64 + t * 16 + 4 * lg + r, a.Sk) - lse_q[i]);
          if (a.drop_thresh != 0u) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                dp[t][r] = drop_keep(a, dkey[i], kc * 64 + t * 16 + 4 * lg + r) ? dp[t][r] * a.drop_scale : 0.f;
          }
          if (sweep == 0) {
            float d = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
              for (int r = 0; r < 4; ++r) d += st[t][r] * dp[t][r];
            delta[i] += d;
          } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
              for (int r = 0; r < 4; ++r) st[t][r] = st[t][r] * (dp[t][r] - delta[i]);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
              const bf16x8 pf = pack_pair(st[2 * s2], st[2 * s2 + 1]);
#pragma unroll
              for (int dt = 0; dt < 4; ++dt)
                dqacc[i][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sK, 32 * s2, 32 * s2 + 16, dt * 16, lr, lg), pf, dqacc[i][dt], 0, 0, 0);
            }
          }
        }
      }
      if (sweep == 0) {
#pragma unroll
        for (int i = 0; i < XS_SLOTS; ++i) delta[i] = group4_sum(delta[i]);
      }
      __syncthreads();  // the next sweep / pass refills slot 0
    }
#pragma unroll
    for (int i = 0; i < XS_SLOTS; ++i) {
      if (ok[i] && qi_[i] < sq_[i]) {
        if (lg == 0) a.delta[stat_[i]] = delta[i];
        bf16* dqp = a.dq + (qb_[i] + qi_[i]) * a.dq_rs + h * 64;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          bf16x4 ov;
#pragma unroll
          for (int r = 0; r < 4; ++r) ov[r] = f2bf(dqacc[i][dt][r] * a.scale);
          *reinterpret_cast<bf16x4*>(dqp + dt * 16 + 4 * lg) = ov;
        }
      }
    }
  }
}

// ---- host side ----
#define XATTN_LDS (ATTN_RES_MAX * ATTN_SLOT + 3 * ATTN_RES_MAX * 64 * 4)   // resident K | V + the key / row vectors
#define XS_LDS (XS_RING * ATTN_SLOT)

// Small self-attention forward (both sequence lengths within one 64-row chunk, no additive bias): the packed kernel puts up to
// four batch rows in one 8-wave workgroup (15 us instead of 18 us at B=256, S=30).  The backward kernels measured the same
// packed or not (they are bound by each wave's dependent load -> MFMA -> exp -> MFMA chain, not by occupancy) and stay
// one row per workgroup.  XFM_ATTN_PACK=0 is the A/B knob.
static bool attn_packable(const AttnArgs& a) {
  static const bool on = xfm_env_flag("XFM_ATTN_PACK", true);
  return on && a.Sq <= 64 && a.Sk <= 64 && a.bias == nullptr && a.bias_t == nullptr && a.B >= 2;
}
static int launch_xattn_fwd_packed(const AttnArgs& a, hipStream_t st) {
  const int tq = cdiv(a.Sq, 16);
  int rpb = 8 / tq < ATTN_RES_MAX ? 8 / tq : ATTN_RES_MAX;
  if (rpb > a.B) rpb = a.B;
  lds_launch<xattn_fwd_kernel<true, false, false>, XATTN_LDS>(dim3(1, a.H, cdiv(a.B, rpb)), dim3(rpb * tq * 64), (size_t)rpb * ATTN_SLOT, st, a);
  return xfm_check_launch("xattn_fwd<pack>");
}

// keys that stay LDS-resident (Sk <= 256) or stream through the ring
static bool xattn_streamed(const AttnArgs& a) { return a.Sk > 64 * ATTN_RES_MAX; }

static int launch_xattn_fwd(const AttnArgs& a, hipStream_t st) {
  const dim3 grid(1, a.H, a.n_groups), blk(512);
  if (xattn_streamed(a)) {
    lds_launch<xattn_fwd_stream_kernel, XS_LDS>(grid, blk, XS_LDS, st, a);
    return xfm_check_launch("xattn_fwd_stream");
  }
  const bool mask = a.key_keep != nullptr, drop = a.drop_thresh != 0u;
  const size_t lds = (size_t)cdiv(a.Sk, 64) * ATTN_SLOT + 1024;
  if (mask && drop) lds_launch<xattn_fwd_kernel<false, true, true>, XATTN_LDS>(grid, blk, lds, st, a);
  else if (mask) lds_launch<xattn_fwd_kernel<false, true, false>, XATTN_LDS>(grid, blk, lds, st, a);
  else if (drop) lds_launch<xattn_fwd_kernel<false, false, true>, XATTN_LDS>(grid, blk, lds, st, a);
  else lds_launch<xattn_fwd_kernel<false, false, false>, XATTN_LDS>(grid, blk, lds, st, a);
  return xfm_check_launch("xattn_fwd");
}

static int launch_xattn_dq(const AttnArgs& a, hipStream_t st) {
  const dim3 grid(1, a.H, a.n_groups), blk(512);
  const bool mask = a.key_keep != nullptr, drop = a.drop_thresh != 0u;
  const size_t lds = (size_t)cdiv(a.Sk, 64) * ATTN_SLOT + 1024;
  if (xattn_streamed(a)) lds_launch<xattn_dq_stream_kernel, XS_LDS>(grid, blk, XS_LDS, st, a);
  else if (mask && drop) lds_launch<xattn_dq_kernel<true, true>, XATTN_LDS>(grid, blk, lds, st, a);
  else if (mask) lds_launch<xattn_dq_kernel<true, false>, XATTN_LDS>(grid, blk, lds, st, a);
  else if (drop) lds_launch<xattn_dq_kernel<false, true>, XATTN_LDS>(grid, blk, lds, st, a);
  else lds_launch<xattn_dq_kernel<false, false>, XATTN_LDS>(grid, blk, lds, st, a);
  return xfm_check_launch("xattn_dq");
}

// dK / dV of both forms: walks any number of keys
static int launch_xattn_dkv(const AttnArgs& a, hipStream_t st) {
  int nw, blocks;
  static const int dkv_nw = xfm_env_int("XFM_XATTN_DKV_NW", 16);  // tuning knob: waves (16-key tiles) per workgroup
  attn_geom(a.Sk, nw, blocks, dkv_nw);
  const dim3 grid(blocks, a.H, a.n_groups), blk(nw * 64);
  if (a.drop_thresh != 0u) lds_launch<xattn_dkv_kernel<true>, XATTN_LDS>(grid, blk, XATTN_LDS, st, a);
  else lds_launch<xattn_dkv_kernel<false>, XATTN_LDS>(grid, blk, XATTN_LDS, st, a);
  return xfm_check_launch("xattn_dkv");
}
