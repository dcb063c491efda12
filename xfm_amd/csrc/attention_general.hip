// The general attention kernels: any sequence lengths, key mask, causal mask, dropout, packed rows, additive bias and its
// gradient.  attn_fwd_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel and their launches.  Included by attention.hip.
// ---------------------------------------------------------------------------------------------
// forward: grid (q blocks, H, B); block = NW waves, wave w owns query rows [qblk*16*NW + 16*w, +16)
// ---------------------------------------------------------------------------------------------
// PLAIN: no key mask, no causal mask, no dropout (the ViT towers) -- those code paths and their registers are compiled out.
template <bool RES, bool PLAIN>
__global__ __launch_bounds__(1024) void attn_fwd_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), nthreads = blockDim.x;
  const int lr = lane & 15, lg = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y;
  long qbase, kbase;
  int sq, sk;
  q_seq(a, b, qbase, sq);
  const int q0 = (blockIdx.x * (nthreads >> 6) + w) * 16;
  const bool wave_active = q0 < sq;
  const int qi = q0 + lr;
  const int qc = qi < sq ? qi : sq - 1;
  const uint32_t dkey = drop_key(a, b, h, qi);
  const bf16* qp = a.q + (qbase + qc) * a.q_rs + h * 64;
  const bf16x8 qf0 = *reinterpret_cast<const bf16x8*>(qp + 8 * lg);
  const bf16x8 qf1 = *reinterpret_cast<const bf16x8*>(qp + 32 + 8 * lg);
  const int kvb = a.kv_index ? a.kv_index[b] : b;  // several query rows may share one key/value source (deduplicated images)
  k_seq(a, kvb, kbase, sk);
  const bf16* kb = a.k + kbase * a.k_rs + h * 64;
  const bf16* vb = a.v + kbase * a.v_rs + h * 64;

  f32x4 oacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) oacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = EXCL_NEG, l_run = 0.f;

  const int nchunks = (sk + 63) / 64;
  constexpr bool resident = RES;  // all chunks of this (b,h) staged once, one barrier (host: Sk <= 256, >= 4 waves)
  const int nw = nthreads >> 6;
  if (resident) {
    for (int kc = 0; kc < nchunks; ++kc) stage_slot(lds + kc * ATTN_SLOT, kb, a.k_rs, vb, a.v_rs, kc * 64, sk, w, nw, lane);
    stage_wait();
  } else {
    stage_slot(lds, kb, a.k_rs, vb, a.v_rs, 0, sk, w, nw, lane);
  }
  for (int kc = 0; kc < nchunks; ++kc) {
    if (!resident) {  // double buffer: chunk kc has landed, everyone is done with chunk kc-1 -> refill its slot
      stage_wait();
      if (kc + 1 < nchunks) stage_slot(lds + ((kc + 1) & 1) * ATTN_SLOT, kb, a.k_rs, vb, a.v_rs, (kc + 1) * 64, sk, w, nw, lane);
    }
    const char* sK = lds + (resident ? kc : (kc & 1)) * ATTN_SLOT;
    const char* sV = sK + ATTN_TILE;
    if (!wave_active) continue;
    f32x4 st[4], bvs[4];
    int kk[PLAIN ? 1 : 4][4];
    const bool has_mask = !PLAIN && a.key_keep != nullptr;
    const bool causal = !PLAIN && a.causal != 0;
    const bool plain = !has_mask && !causal && kc * 64 + 64 <= sk;  // wave-uniform: nothing to mask in this chunk
    load_bias(a, h, qc, kc, lg, bvs);  // bias (and key-keep) loads first: their L2 latency hides under the QK^T MFMAs
    if constexpr (!PLAIN) {
      if (has_mask) load_keep(a, kvb, kc, lg, kk);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, t * 16, 0, lr, lg), qf0, st[t], 0, 0, 0);
      st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, t * 16, 1, lr, lg), qf1, st[t], 0, 0, 0);
    }
    float mx = EXCL_NEG;
    if (plain) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          st[t][r] = fmaf(st[t][r], a.scale, bvs[t][r]);
          mx = fmaxf(mx, st[t][r]);
        }
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          st[t][r] = score_masked(a, st[t][r], bvs[t][r], has_mask, has_mask ? kk[PLAIN ? 0 : t][r] : 1, causal, qi, kc * 64 + t * 16 + 4 * lg + r, sk);
          mx = fmaxf(mx, st[t][r]);
        }
    }
    mx = group4_max(mx);
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __expf(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        st[t][r] = __expf(st[t][r] - m_new);
        psum += st[t][r];
      }
    if (!PLAIN && a.drop_thresh != 0u) {  // one wave-uniform branch per chunk; the row sum above is of the undropped probabilities
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
    for (int s = 0; s < 2; ++s) {
      const bf16x8 pf = pack_pair(st[2 * s], st[2 * s + 1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sV, 32 * s, 32 * s + 16, dt * 16, lr, lg), pf, oacc[dt], 0, 0, 0);
    }
  }
  if (!wave_active || qi >= sq) return;
  store_out(a, qbase + qi, h, lg, oacc, 1.0f / l_run);
  if (lg == 0) a.lse[((long)b * a.H + h) * a.stat_ld + qi] = m_run + __logf(l_run);
}

// ---------------------------------------------------------------------------------------------
// backward 1/2: dQ (+ delta, + dbias).  Same decomposition as the forward.
// NKC > 0 selects the bias-gradient variant (Sk <= 64*NKC): one workgroup walks `nb_per_block` batch entries and keeps
// sum_b dS in registers, then flushes it through a wave-private LDS transpose so that every atomic wave-instruction
// adds 64 consecutive keys of one bias row (256 contiguous bytes; MI355X_MICROARCH "Global float atomics").
// delta_i is recomputed exactly as sum_j P_ij dP_ij in a first pass over the keys (see below).
// ---------------------------------------------------------------------------------------------
template <int NKC, bool RES, bool PLAIN>
__global__ __launch_bounds__(512) void attn_bwd_dq_kernel(AttnArgs a, int nb_per_block) {
  constexpr bool DBIAS = NKC > 0;
  constexpr int NACC = DBIAS ? NKC : 1;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), nthreads = blockDim.x;
  const int lr = lane & 15, lg = lane >> 4;
  const int h = blockIdx.y;
  const int q0 = (blockIdx.x * (nthreads >> 6) + w) * 16;
  const int qi = q0 + lr;
  constexpr bool resident = RES;

  f32x4 dsacc[NACC][4];
#pragma unroll
  for (int i = 0; i < NACC; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) dsacc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int bi = 0; bi < nb_per_block; ++bi) {
    const int b = blockIdx.z * nb_per_block + bi;
    if (b >= a.B) break;
    long qbase, kbase;
    int sq, sk;
    q_seq(a, b, qbase, sq);
    const bool wave_active = q0 < sq;
    const bool qvalid = qi < sq;
    const int qc = qvalid ? qi : sq - 1;
    const uint32_t dkey = drop_key(a, b, h, qi);
    const bf16* qp = a.q + (qbase + qc) * a.q_rs + h * 64;
    const bf16* dop = a.dout + (qbase + qc) * a.do_rs + h * 64;
    const bf16x8 qf0 = *reinterpret_cast<const bf16x8*>(qp + 8 * lg);
    const bf16x8 qf1 = *reinterpret_cast<const bf16x8*>(qp + 32 + 8 * lg);
    const bf16x8 df0 = *reinterpret_cast<const bf16x8*>(dop + 8 * lg);
    const bf16x8 df1 = *reinterpret_cast<const bf16x8*>(dop + 32 + 8 * lg);
    const long stat_idx = ((long)b * a.H + h) * a.stat_ld + qc;
    const float lse = a.lse[stat_idx];
    const int kvb = a.kv_index ? a.kv_index[b] : b;
    k_seq(a, kvb, kbase, sk);
    const int nchunks = (sk + 63) / 64;
    const bf16* kb = a.k + kbase * a.k_rs + h * 64;
    const bf16* vb = a.v + kbase * a.v_rs + h * 64;

    const int nw = nthreads >> 6;
    if (resident) {
      __syncthreads();  // previous batch entry's readers are done
      for (int kc = 0; kc < nchunks; ++kc) stage_slot(lds + kc * ATTN_SLOT, kb, a.k_rs, vb, a.v_rs, kc * 64, sk, w, nw, lane);
      stage_wait();
    }
    // streaming mode: double-buffered slots; `first` issues chunk 0 of a pass, `next` waits for chunk kc and refills
    auto stream_first = [&]() {
      __syncthreads();
      stage_slot(lds, kb, a.k_rs, vb, a.v_rs, 0, sk, w, nw, lane);
    };
    auto stream_next = [&](int kc) {
      stage_wait();
      if (kc + 1 < nchunks) stage_slot(lds + ((kc + 1) & 1) * ATTN_SLOT, kb, a.k_rs, vb, a.v_rs, (kc + 1) * 64, sk, w, nw, lane);
    };
    // probabilities P (recomputed from the forward's log-sum-exp) and dropped dP = (dO . V^T) * keep/(1-p) of one chunk
    auto probs = [&](int kc, f32x4 (&st)[4], f32x4 (&dp)[4]) {
      const char* sK = lds + (resident ? kc : (kc & 1)) * ATTN_SLOT;
      const char* sV = sK + ATTN_TILE;
      f32x4 bvs[4];
      int kk[PLAIN ? 1 : 4][4];
      const bool has_mask = !PLAIN && a.key_keep != nullptr;
      const bool causal = !PLAIN && a.causal != 0;
      const bool plain = !has_mask && !causal && kc * 64 + 64 <= sk;
      load_bias(a, h, qc, kc, lg, bvs);
      if constexpr (!PLAIN) {
        if (has_mask) load_keep(a, kvb, kc, lg, kk);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, t * 16, 0, lr, lg), qf0, st[t], 0, 0, 0);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sK, t * 16, 1, lr, lg), qf1, st[t], 0, 0, 0);
        dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sV, t * 16, 0, lr, lg), df0, dp[t], 0, 0, 0);
        dp[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sV, t * 16, 1, lr, lg), df1, dp[t], 0, 0, 0);
      }
      const float lse_q = qvalid ? lse : 3.0e38f;  // rows past Sq: exp(s - 3e38) = 0, no per-element select
      if (plain) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) st[t][r] = __expf(fmaf(st[t][r], a.scale, bvs[t][r]) - lse_q);
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)  // excluded keys: exp(EXCL_NEG - lse) = 0
            st[t][r] = __expf(score_masked(a, st[t][r], bvs[t][r], has_mask, has_mask ? kk[PLAIN ? 0 : t][r] : 1, causal, qi, kc * 64 + t * 16 + 4 * lg + r, sk) - lse_q);
      }
      if (!PLAIN && a.drop_thresh != 0u) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            dp[t][r] = drop_keep(a, dkey, kc * 64 + t * 16 + 4 * lg + r) ? dp[t][r] * a.drop_scale : 0.f;
      }
    };

    // pass 1: delta_i = sum_j P_ij dP_ij from the SAME P and dP that form dS below, so that sum_j dS_ij = 0 holds to
    // fp32 rounding (rowsum(dO*O) with a bf16-rounded O breaks it by ~2^-9 |dO||O| and swamps small dS)
    float delta = 0.f;
    f32x4 st[4], dp[4];
    const bool fast_delta = a.o_lo != nullptr;  // delta = dO . (O + Olo): no first pass over the keys (uniform over the launch)
    if (fast_delta) {
      delta = delta_from_out(a, qbase + qc, h, lg, df0, df1);
    } else {
      if (!resident) stream_first();
      for (int kc = 0; kc < nchunks; ++kc) {
        if (!resident) stream_next(kc);
        if (wave_active) {
          probs(kc, st, dp);
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) delta += st[t][r] * dp[t][r];
        }
      }
      delta = group4_sum(delta);
    }
    if (wave_active && qvalid && lg == 0) a.delta[stat_idx] = delta;

    f32x4 dqacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) dqacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    // pass 2: dS, dbias, dQ   (a single-chunk problem keeps pass 1's registers and its staged tile)
    if (!resident && (nchunks > 1 || fast_delta)) stream_first();
    for (int kc = 0; kc < nchunks; ++kc) {
      if (nchunks > 1 || fast_delta) {
        if (!resident) stream_next(kc);
        if (wave_active) probs(kc, st, dp);
      }
      if (!wave_active) continue;
      const char* sK = lds + (resident ? kc : (kc & 1)) * ATTN_SLOT;
      // bias gradient without the in-register sums (NKC = 0): this entry's dS goes to the workspace [B,H,Sq,bias_ld] when there is
      // one (dbias_reduce_kernel adds the batch sum to dbias afterwards), else one float atomic per score
      float* wsrow = (!DBIAS && a.dbias != nullptr && a.dbias_ws != nullptr) ? a.dbias_ws + (((long)b * a.H + h) * a.Sq + qi) * a.bias_ld : nullptr;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int kj0 = kc * 64 + t * 16 + 4 * lg;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kj = kj0 + r;
          const float ds = st[t][r] * (dp[t][r] - delta);
          st[t][r] = ds;
          if (!DBIAS && a.dbias != nullptr && wsrow == nullptr && kj < sk && qvalid) atomicAdd(a.dbias + ((long)h * a.Sq + qi) * a.bias_ld + kj, ds);
        }
        if (!DBIAS && wsrow != nullptr && qvalid) {
          if (kj0 + 4 <= a.bias_ld) *reinterpret_cast<f32x4*>(wsrow + kj0) = st[t];  // (columns in [Sk, bias_ld) get exact zeros: P = 0 there)
          else
            for (int r = 0; r < 4; ++r)
              if (kj0 + r < a.bias_ld) wsrow[kj0 + r] = st[t][r];
        }
      }
      if (DBIAS) {  // static register indices only: a wave-uniform compare selects the chunk's accumulator
#pragma unroll
        for (int c = 0; c < NACC; ++c)
          if (c == kc) {
#pragma unroll
            for (int t = 0; t < 4; ++t) dsacc[c][t] += st[t];
          }
      }
      // dQ^T[d, q] += K^T[d, key] . dS^T[key, q]
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pf = pack_pair(st[2 * s2], st[2 * s2 + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          dqacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sK, 32 * s2, 32 * s2 + 16, dt * 16, lr, lg), pf, dqacc[dt], 0, 0, 0);
      }
    }
    if (wave_active && qvalid) {
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

  if (DBIAS) {  // (dense rows only: the launcher never pairs the bias-gradient variant with packed rows)
    const bool wave_active = q0 < a.Sq;
    const int nchunks = (a.Sk + 63) / 64;
    float* fl = reinterpret_cast<float*>(lds + w * 4096);  // wave-private [16 q][64 keys], aliases the K/V slots (done with)
#pragma unroll
    for (int kc = 0; kc < NACC; ++kc) {
      if (kc < nchunks) {
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(fl + lr * 64 + t * 16 + 4 * lg) = dsacc[kc][t];
        __syncthreads();
        if (wave_active && a.dbias != nullptr) {
          const int kj = kc * 64 + lane;
          for (int row = 0; row < 16; ++row) {
            const int q = q0 + row;
            if (q < a.Sq && kj < a.Sk) atomicAdd(a.dbias + ((long)h * a.Sq + q) * a.bias_ld + kj, fl[row * 64 + lane]);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// backward 2/2: dK, dV.  grid (key blocks, H, B); wave w owns keys [kblk*16*NW + 16*w, +16); queries stream in chunks
// of 64 (Q and dO staged in LDS, read by rows for S / dP and transposed for dK^T / dV^T).
// ---------------------------------------------------------------------------------------------
template <bool RES, bool PLAIN>
__global__ __launch_bounds__(512) void attn_bwd_dkv_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), nthreads = blockDim.x;
  const int lr = lane & 15, lg = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y;
  const int kvb = a.kv_index ? a.kv_index[b] : b;
  long qbase, kbase, kout;
  int sq, sk, sk_unused;
  q_seq(a, b, qbase, sq);
  k_seq(a, kvb, kbase, sk);
  k_seq(a, b, kout, sk_unused);  // dk / dv rows belong to the QUERY batch entry (kv_index folds them afterwards)
  const int k0 = (blockIdx.x * (nthreads >> 6) + w) * 16;
  const bool wave_active = k0 < sk;
  const int kj = k0 + lr;
  const bool kvalid = kj < sk;
  const int kcl = kvalid ? kj : sk - 1;
  const bf16* kp = a.k + (kbase + kcl) * a.k_rs + h * 64;
  const bf16* vp = a.v + (kbase + kcl) * a.v_rs + h * 64;
  (void)sk_unused;
  const bf16x8 kf0 = *reinterpret_cast<const bf16x8*>(kp + 8 * lg);
  const bf16x8 kf1 = *reinterpret_cast<const bf16x8*>(kp + 32 + 8 * lg);
  const bf16x8 vf0 = *reinterpret_cast<const bf16x8*>(vp + 8 * lg);
  const bf16x8 vf1 = *reinterpret_cast<const bf16x8*>(vp + 32 + 8 * lg);
  const bf16* qb = a.q + qbase * a.q_rs + h * 64;
  const bf16* db = a.dout + qbase * a.do_rs + h * 64;
  const float* lse_b = a.lse + ((long)b * a.H + h) * a.stat_ld;
  const float* del_b = a.delta + ((long)b * a.H + h) * a.stat_ld;
  bool key_masked = false;
  if (!PLAIN && a.key_keep != nullptr) key_masked = a.key_keep[(long)kvb * a.Sk + kcl] == 0;
  const bool causal = !PLAIN && a.causal != 0;

  f32x4 dkacc[4], dvacc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { dkacc[i] = f32x4{0.f, 0.f, 0.f, 0.f}; dvacc[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  const int nchunks = (sq + 63) / 64;
  constexpr bool resident = RES;
  const int nw = nthreads >> 6;
  // row statistics / transposed bias of this lane's 4 consecutive queries in 32-query step `step`: 16-B loads
  auto load_stats = [&](int step, f32x4 (&l)[2], f32x4 (&d)[2], f32x4 (&bt)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int qi0 = step * 32 + u * 16 + 4 * lg;
      l[u] = d[u] = bt[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (qi0 < a.Sq) {
        l[u] = *reinterpret_cast<const f32x4*>(lse_b + qi0);
        d[u] = *reinterpret_cast<const f32x4*>(del_b + qi0);
        if (a.bias_t != nullptr && kvalid) bt[u] = *reinterpret_cast<const f32x4*>(a.bias_t + ((long)h * a.Sk + kj) * a.bias_t_ld + qi0);
      }
    }
  };
  if (resident) {
    for (int qc = 0; qc < nchunks; ++qc) stage_slot(lds + qc * ATTN_SLOT, qb, a.q_rs, db, a.do_rs, qc * 64, sq, w, nw, lane);
    stage_wait();
  } else {
    stage_slot(lds, qb, a.q_rs, db, a.do_rs, 0, sq, w, nw, lane);
  }
  _Pragma("unroll 1") for (int qc = 0; qc < nchunks; ++qc) {
    if (!resident) {
      stage_wait();
      if (qc + 1 < nchunks) stage_slot(lds + ((qc + 1) & 1) * ATTN_SLOT, qb, a.q_rs, db, a.do_rs, (qc + 1) * 64, sq, w, nw, lane);
    }
    const char* sQ = lds + (resident ? qc : (qc & 1)) * ATTN_SLOT;
    const char* sD = sQ + ATTN_TILE;
    if (!wave_active) continue;
    // one 32-query k-step at a time (two 16-query tiles): D[i = query row][j = key col], lane (lg, lr) -> query
    // 16t + 4lg + r, key lr.  Half the live registers of a whole-chunk formulation, so two workgroups fit per CU.
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      f32x4 st[2], dp[2], pd[2], lsev[2], delv[2], bvt[2];
      load_stats(qc * 2 + s2, lsev, delv, bvt);  // issued early: their latency hides under the MFMAs below
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int t = 2 * s2 + u;
        st[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        st[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sQ, t * 16, 0, lr, lg), kf0, st[u], 0, 0, 0);
        st[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sQ, t * 16, 1, lr, lg), kf1, st[u], 0, 0, 0);
        dp[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sD, t * 16, 0, lr, lg), vf0, dp[u], 0, 0, 0);
        dp[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(sD, t * 16, 1, lr, lg), vf1, dp[u], 0, 0, 0);
      }
      if (a.bias != nullptr && a.bias_t == nullptr) {  // no transposed bias copy: strided gather (slow path, wave-uniform)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int qi = qc * 64 + (2 * s2 + u) * 16 + 4 * lg + r;
            if (qi < a.Sq && kvalid) bvt[u][r] = a.bias[((long)h * a.Sq + qi) * a.bias_ld + kj];
          }
      }
      const float key_add = key_masked ? MASK_NEG : 0.f;
      const bool tail = qc * 64 + 64 > sq;  // wave-uniform: this chunk holds rows past the last query
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int qi0 = qc * 64 + (2 * s2 + u) * 16 + 4 * lg;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qi = qi0 + r;
          float sc = fmaf(st[u][r], a.scale, bvt[u][r]);
          if (!PLAIN) sc += (causal & (kj > qi)) ? MASK_NEG : key_add;  // masked once, whichever reason (xroberta.py:772-807)
          float pv = __expf(sc - lsev[u][r]);
          float dl = delv[u][r];
          if (tail) {  // the statistics past the last query are unwritten padding: select, never multiply
            pv = qi < sq ? pv : 0.f;
            dl = qi < sq ? dl : 0.f;
          }
          pv = kvalid ? pv : 0.f;
          delv[u][r] = dl;
          pd[u][r] = pv;
          st[u][r] = pv * (dp[u][r] - dl);
        }
      }
      if (!PLAIN && a.drop_thresh != 0u) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int qi = qc * 64 + (2 * s2 + u) * 16 + 4 * lg + r;
            const float keepf = drop_keep(a, drop_key(a, b, h, qi), kj) ? a.drop_scale : 0.f;
            st[u][r] = pd[u][r] * (dp[u][r] * keepf - delv[u][r]);
            pd[u][r] *= keepf;
          }
      }
      // dV^T[d, key] += dO^T[d, q] . Pd[q, key] ;  dK^T[d, key] += Q^T[d, q] . dS[q, key]
      const bf16x8 pf = pack_pair(pd[0], pd[1]);
      const bf16x8 sf = pack_pair(st[0], st[1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        dvacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sD, 32 * s2, 32 * s2 + 16, dt * 16, lr, lg), pf, dvacc[dt], 0, 0, 0);
        dkacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(sQ, 32 * s2, 32 * s2 + 16, dt * 16, lr, lg), sf, dkacc[dt], 0, 0, 0);
      }
    }
  }
  if (!wave_active || !kvalid) return;
  bf16* dkp = a.dk + (kout + kj) * a.dk_rs + h * 64;
  bf16* dvp = a.dv + (kout + kj) * a.dv_rs + h * 64;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    bf16x4 ok_, ov_;
#pragma unroll
    for (int r = 0; r < 4; ++r) { ok_[r] = f2bf(dkacc[dt][r] * a.scale); ov_[r] = f2bf(dvacc[dt][r]); }
    *reinterpret_cast<bf16x4*>(dkp + dt * 16 + 4 * lg) = ok_;
    *reinterpret_cast<bf16x4*>(dvp + dt * 16 + 4 * lg) = ov_;
  }
}

// ---- host side ----
#define ATTN_RES_LDS (ATTN_RES_MAX * ATTN_SLOT)   // the resident instantiations' limit
#define ATTN_STREAM_LDS (2 * ATTN_SLOT)

static bool attn_resident(int S, int nw) { return cdiv(S, 64) <= ATTN_RES_MAX && nw >= 4; }

static size_t attn_lds_bytes(int S, int nw, size_t at_least) {
  size_t b = (size_t)(attn_resident(S, nw) ? cdiv(S, 64) : 2) * ATTN_SLOT;
  return b > at_least ? b : at_least;
}

static int launch_attn_fwd(const AttnArgs& a, hipStream_t st) {
  int nw, blocks;
  static const int fwd_nw = xfm_env_int("XFM_ATTN_FWD_NW", 8);  // tuning knob
  attn_geom(a.Sq, nw, blocks, fwd_nw);
  const dim3 grid(blocks, a.H, a.B), blk(nw * 64);
  const size_t lds = attn_lds_bytes(a.Sk, nw, 0);
  if (attn_resident(a.Sk, nw)) {
    if (attn_plain(a)) lds_launch<attn_fwd_kernel<true, true>, ATTN_RES_LDS>(grid, blk, lds, st, a);
    else lds_launch<attn_fwd_kernel<true, false>, ATTN_RES_LDS>(grid, blk, lds, st, a);
  } else {
    if (attn_plain(a)) lds_launch<attn_fwd_kernel<false, true>, ATTN_STREAM_LDS>(grid, blk, lds, st, a);
    else lds_launch<attn_fwd_kernel<false, false>, ATTN_STREAM_LDS>(grid, blk, lds, st, a);
  }
  return xfm_check_launch("attn_fwd");
}

// batch entries whose dS one workgroup of attn_bwd_dq_kernel<4, true, true> sums before touching HBM.  The kernel holds 230+ VGPRs
// (sum_b dS of four chunks), i.e. one workgroup per CU: of 4 and 8 entries take the one with fewer (rounds of 256 workgroups) x
// entries, ties to 8 (half the atomics) -- B = 64: 192 workgroups x 8 entries beats 384 x 4 (1.5 rounds) by 6 %.
static int attn_dbias_sums_nb(const AttnArgs& a, int blocks) {
  int nb = a.B >= 8 ? 2 : 1;
  if (a.B >= 32) {
    const long c4 = (long)cdiv(blocks * a.H * cdiv(a.B, 4), 256) * 4, c8 = (long)cdiv(blocks * a.H * cdiv(a.B, 8), 256) * 8;
    nb = c8 <= c4 ? 8 : 4;
  }
  static const int nb_env = xfm_env_int("XFM_ATTN_DBIAS_NB", 0);  // tuning knob
  return nb_env > 0 ? nb_env : nb;
}

// dQ (+ delta).  sums_nb > 0: the bias gradient of sums_nb batch entries summed in registers (a resident, plain problem); 0: one entry
// per workgroup, and a bias gradient leaves per element: into a.dbias_ws when there is one, else by float atomics.
static int launch_attn_bwd_dq(const AttnArgs& a, int nw, int blocks, int sums_nb, hipStream_t st) {
  const dim3 grid(blocks, a.H, sums_nb > 0 ? cdiv(a.B, sums_nb) : a.B), blk(nw * 64);
  const bool plain = attn_plain(a);
  if (sums_nb > 0) {
    lds_launch<attn_bwd_dq_kernel<4, true, true>, ATTN_RES_LDS>(grid, blk, attn_lds_bytes(a.Sk, nw, 8 * 4096), st, a, sums_nb);
  } else if (attn_resident(a.Sk, nw)) {
    if (plain) lds_launch<attn_bwd_dq_kernel<0, true, true>, ATTN_RES_LDS>(grid, blk, attn_lds_bytes(a.Sk, nw, 0), st, a, 1);
    else lds_launch<attn_bwd_dq_kernel<0, true, false>, ATTN_RES_LDS>(grid, blk, attn_lds_bytes(a.Sk, nw, 0), st, a, 1);
  } else {
    if (plain) lds_launch<attn_bwd_dq_kernel<0, false, true>, ATTN_STREAM_LDS>(grid, blk, attn_lds_bytes(a.Sk, nw, 0), st, a, 1);
    else lds_launch<attn_bwd_dq_kernel<0, false, false>, ATTN_STREAM_LDS>(grid, blk, attn_lds_bytes(a.Sk, nw, 0), st, a, 1);
  }
  return xfm_check_launch("attn_bwd_dq");
}

static int launch_attn_bwd_dkv(const AttnArgs& a, hipStream_t st) {
  int nw, blocks;
  attn_geom(a.Sk, nw, blocks);
  const dim3 grid(blocks, a.H, a.B), blk(nw * 64);
  const bool plain = attn_plain(a);
  static const bool dkv_res = xfm_env_flag("XFM_ATTN_DKV_RES", true);  // tuning knob
  if (dkv_res && attn_resident(a.Sq, nw)) {
    if (plain) lds_launch<attn_bwd_dkv_kernel<true, true>, ATTN_RES_LDS>(grid, blk, attn_lds_bytes(a.Sq, nw, 0), st, a);
    else lds_launch<attn_bwd_dkv_kernel<true, false>, ATTN_RES_LDS>(grid, blk, attn_lds_bytes(a.Sq, nw, 0), st, a);
  } else {
    if (plain) lds_launch<attn_bwd_dkv_kernel<false, true>, ATTN_STREAM_LDS>(grid, blk, 2 * ATTN_SLOT, st, a);
    else lds_launch<attn_bwd_dkv_kernel<false, false>, ATTN_STREAM_LDS>(grid, blk, 2 * ATTN_SLOT, st, a);
  }
  return xfm_check_launch("attn_bwd_dkv");
}
