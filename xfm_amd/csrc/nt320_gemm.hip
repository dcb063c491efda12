// gemm_nt, 320 x 256 one-round tile (configuration 6): the kernel and its launch.  Included by gemm.hip behind gemm_nt_256.hip, whose
// wait_vm / nt256_eligible it shares.

// ---------------------------------------------------------------------------------------------
// 320 x 256 tile, 8 waves as 2 (M) x 4 (N), each wave a 160 x 64 output block (10 x 4 MFMA tiles, 160 accumulator registers).  The tile
// exists for ONE shape family: M = 25216 rows against N = 768 is 99 x 3 = 297 tiles of 256 x 256 (1.16 rounds on 256 CUs, which
// nt_plan splits into a whole round and a small-tile tail) but 79 x 3 = 237 tiles of 320 x 256 -- one round, one launch, no tail.
// One workgroup per tile; there is no persistent form.
//
// Operand layout as in gemm_nt_256_kernel (C-transposed MFMA tiles, swz_x / swz_w, direct-to-LDS loads in inline asm with counted
// vmcnt, rows clamped on load and skipped on store, 32-bit element offsets), and every output element is accumulated over K in the
// same order by the same MFMA: the results are bit-identical to configuration 5.
//
// Staging UNITS are 64 rows x 128 B = 8 KiB: one direct-to-LDS instruction per wave, so one unit is one count of vmcnt in every
// wave.  A 64-wide K-tile is nine units, numbered j in the order the phases need them:
//   j = 0      X0: X rows {32u + 0-31, 160 + 32u + 0-31} for u = 0 (m-tiles 2u, 2u + 1 of both M-wave rows)
//   j = 1..4   W0..W3: W rows 64h + 0-63 (the rows of N-wave column h)
//   j = 5..8   X1..X4: as X0 with u = 1..4
// and the LDS ring holds two K-tiles: 18 slots, unit j of K-tile kt in slot 9 (kt & 1) + j (144 KiB).
// A K-tile is computed in 5 phases of 16 MFMA: phase u reads X unit u (4 ds_read_b128 per wave) and multiplies its two m-tiles
// against the wave's W fragments of the whole K-tile, which phase 0 reads once (8 reads, 32 registers): 28 fragment reads per 80 MFMA
// where the 256 x 256 kernel has 24 per 64, on 48 fragment registers instead of 64.
// Issue order: the prologue puts the first 11 units (K-tile 0 and X0, W0 of K-tile 1) in flight; the phases of K-tile kt then issue
// 2, 2, 2, 2, 1 more, always 11 ahead of the first unit of kt:
//   P0: W1, W2 of kt+1    P1: W3, X1 of kt+1    P2: X2, X3 of kt+1    P3: X4 of kt+1, X0 of kt+2    P4: W0 of kt+2
// so every unit flies >= 4 phases, and the wait at the end of a phase's issue section leaves 7, 8, 9, 10, 6 units in flight (fewer
// at the end of K): exactly the unit(s) the NEXT phase reads are retired.
// The two M-wave groups run half a phase apart with two barriers per phase, as in the 256 x 256 kernel; the hazards follow from
// the same argument.  RAW: a wave's share of a unit is retired by its own counted vmcnt before barrier #1 of the phase in front of
// the one that reads it, and the readers start behind barrier #2 of that phase, which every wave of both groups reaches after its
// wait.  WAR: a unit read in phase q is last touched before the later group's barrier #2 of q; a unit issued in phase q + 2 or
// later goes out behind that barrier in both groups.  The closest pair above is X0 of kt+2 (issued in P3) over X0 of kt (read in P0).
// ---------------------------------------------------------------------------------------------
constexpr int NT320_UNIT = 64 * 128;            // bytes of a staging unit
constexpr int NT320_LEAD = 11;                  // units in flight ahead of the K-tile being computed
constexpr int NT320_LDS = 18 * NT320_UNIT;      // two K-tiles

template <int V>
struct Nt320Phase { static constexpr int v = V; };

// leave the n youngest staging units in flight (n is wave-uniform; the schedule never asks for more than 10)
__device__ __forceinline__ void nt320_wait(int n) {
  if (n >= 10) wait_vm<10>();
  else if (n == 9) wait_vm<9>();
  else if (n == 8) wait_vm<8>();
  else if (n == 7) wait_vm<7>();
  else if (n == 6) wait_vm<6>();
  else if (n == 5) wait_vm<5>();
  else if (n == 4) wait_vm<4>();
  else if (n == 3) wait_vm<3>();
  else if (n == 2) wait_vm<2>();
  else if (n == 1) wait_vm<1>();
  else wait_vm<0>();
}

template <int EPI>
__global__ __launch_bounds__(512) void gemm_nt_320_kernel(GemmNT g) {
  constexpr int BM = 320, BN = 256, MT = 10, NT = 4, UNIT = NT320_UNIT, LEAD = NT320_LEAD;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 2, wc = w & 3;
  const int lr = lane & 15, lg = lane >> 4;
  const int tiles_n = (g.N + BN - 1) / BN, tiles_m = (g.M + BM - 1) / BM;
  const int nk = g.K / 64;
  int tm, tn;
  grouped_tile(xcd_remap(blockIdx.x, tiles_m * tiles_n), tiles_m, tiles_n, g.group_m, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  // per-lane global element offsets of the nine unit loads of a K-tile; the K offset is added per K-tile.  Wave w fills the 1-KiB
  // block w of a unit's slot: unit rows 8 w + (lane >> 3), 16-B chunk lane & 7.
  unsigned soff[9];
  {
    const int ur = w * 8 + (lane >> 3);
#pragma unroll
    for (int u = 0; u < 5; ++u) {
      const int r = (ur & 31) + 32 * u + (ur >> 5) * 160;
      int gr = m0 + r; gr = gr < g.M ? gr : g.M - 1;
      soff[u == 0 ? 0 : 4 + u] = (unsigned)gr * (unsigned)g.lda + (((lane & 7) ^ swz_x(r)) << 3);
    }
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int r = h * 64 + ur;
      int gr = n0 + r; gr = gr < g.N ? gr : g.N - 1;
      soff[1 + h] = (unsigned)gr * (unsigned)g.ldb + (((lane & 7) ^ swz_w(r)) << 3);
    }
  }
  const unsigned lds0 = (unsigned)(uintptr_t)LDS_PTR(void, smem) + (unsigned)(w * 1024);
  auto issue = [&](int j, int kt) {  // unit j (a constant where it is called) of K-tile kt; wave-uniform branch
    if (kt >= nk) return;
    const bf16* src = ((j == 0 || j >= 5) ? g.A : g.B) + kt * 64;
    // inline asm on purpose, as in gemm_nt_256_kernel: a direct-to-LDS load the compiler can see is drained in front of every ds_read
    const unsigned lds_addr = lds0 + (unsigned)(((kt & 1) * 9 + j) * UNIT);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src + (size_t)soff[j]), "s"(lds_addr) : "memory", "m0");
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-lane byte offsets of the fragment reads inside a unit's slot (the chunk index ks*4 + lg is XOR-ed with the row swizzle, which
  // only depends on the low row bits the unit row shares with the tile row):
  //   X unit u: tile rows wr*160 + 32u + m*16 + lr -> unit rows wr*32 + m*16 + lr
  //   W unit wc: tile rows wc*64 + np*32 + 4*n + 8*(lr>>2) + (lr&3) -> unit rows np*32 + 4*n + 8*(lr>>2) + (lr&3)
  const int xs = swz_x(lr);
  const int wu = 8 * (lr >> 2) + (lr & 3);
  const int ws = swz_w(wu);
  const int xbase0 = (wr * 32 + lr) * 128 + (((0 + lg) ^ xs) << 4), xbase1 = (wr * 32 + lr) * 128 + (((4 + lg) ^ xs) << 4);
  const int wbase0 = (1 + wc) * UNIT + wu * 128 + (((0 + lg) ^ ws) << 4), wbase1 = (1 + wc) * UNIT + wu * 128 + (((4 + lg) ^ ws) << 4);

  bf16x8 xa[2][2], wf[4][2];
  const int total = 9 * nk;

  // one phase: issue, fragment reads, counted wait | barrier | 16 MFMA | barrier
  auto phase = [&](auto P, int kt) {
    constexpr int p = decltype(P)::v;
    constexpr int cum = p == 4 ? 9 : 2 * (p + 1);                 // units issued by the phases 0..p of a K-tile
    constexpr int need = p == 4 ? 14 : 6 + p;                     // units (counted from the first of kt) the next phase has read from
    if (p == 0) { issue(2, kt + 1); issue(3, kt + 1); }
    if (p == 1) { issue(4, kt + 1); issue(5, kt + 1); }
    if (p == 2) { issue(6, kt + 1); issue(7, kt + 1); }
    if (p == 3) { issue(8, kt + 1); issue(0, kt + 2); }
    if (p == 4) { issue(1, kt + 2); }
    const char* buf = smem + (kt & 1) * 9 * UNIT;
    const char* xslot = buf + (p == 0 ? 0 : 4 + p) * UNIT;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      xa[m][0] = *reinterpret_cast<const bf16x8*>(xslot + xbase0 + m * 2048);
      xa[m][1] = *reinterpret_cast<const bf16x8*>(xslot + xbase1 + m * 2048);
    }
    if (p == 0) {
#pragma unroll
      for (int n = 0; n < 4; ++n) {   // n = np*2 + n': unit rows np*32 + 4 n'
        wf[n][0] = *reinterpret_cast<const bf16x8*>(buf + wbase0 + (n >> 1) * 4096 + (n & 1) * 512);
        wf[n][1] = *reinterpret_cast<const bf16x8*>(buf + wbase1 + (n >> 1) * 4096 + (n & 1) * 512);
      }
    }
    {
      const int rem = total - 9 * kt;                             // units from the first of kt to the end of K
      if (rem >= LEAD + cum) wait_vm<LEAD + cum - need>();        // every unit of the schedule exists: 7, 8, 9, 10, 6 stay in flight
      else nt320_wait(rem - need);                                // the last two K-tiles: what was issued ends at K
    }
    XFM_BAR();
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[2 * p + m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[n][ks], xa[m][ks], acc[2 * p + m][n], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    XFM_BAR();
  };

  // prologue: K-tile 0 and X0, W0 of K-tile 1 in flight; X0 and W0..W3 of K-tile 0 retired and visible
#pragma unroll
  for (int j = 0; j < 9; ++j) issue(j, 0);
  issue(0, 1);
  issue(1, 1);
  nt320_wait((LEAD < total ? LEAD : total) - 5);
  XFM_BAR();
  if (wr == 1) XFM_BAR();  // stagger the second M-wave group by one barrier

  for (int kt = 0; kt < nk; ++kt) {
    phase(Nt320Phase<0>{}, kt);
    phase(Nt320Phase<1>{}, kt);
    phase(Nt320Phase<2>{}, kt);
    phase(Nt320Phase<3>{}, kt);
    phase(Nt320Phase<4>{}, kt);
  }
  if (wr == 0) XFM_BAR();  // both groups are past their last LDS read
  if (EPI == EPI_DGELU) {
    // the gelu'(x) chunks that gemm_epilogue loads up front are 80 registers for 10 m-tiles, which do not fit beside 160 accumulators:
    // two halves of 5 m-tiles (same values, same stores)
    gemm_epilogue<MT / 2, NT, EPI>(g, reinterpret_cast<f32x4(&)[MT / 2][NT]>(acc[0]), m0 + wr * 160, n0 + wc * 64, lr, lg);
    gemm_epilogue<MT / 2, NT, EPI>(g, reinterpret_cast<f32x4(&)[MT / 2][NT]>(acc[MT / 2]), m0 + wr * 160 + 80, n0 + wc * 64, lr, lg);
  } else {
    gemm_epilogue<MT, NT, EPI>(g, acc, m0 + wr * 160, n0 + wc * 64, lr, lg);
  }
}

// ---- host side ----
// One round of one workgroup per tile, whole column tiles and K-tiles, operands inside the 32-bit element offsets
static bool nt320_eligible(int M, long lda, int N, long ldb, int K) {
  static const int cus = xfm_cu_count() > 0 ? xfm_cu_count() : 256;  // (a plan query without a device: the MI355X count, as tn_group_cus)
  return N % 256 == 0 && K % 64 == 0 && (long)cdiv(M, 320) * (N / 256) <= cus && nt256_eligible(M, lda, N, ldb);
}

static int launch_nt_320(const GemmNT& g, int epi, hipStream_t st) {
  if (!nt320_eligible(g.M, g.lda, g.N, g.ldb, g.K)) {
    xfm_set_error("gemm_nt: M=%d N=%d K=%d is no shape of the one-round 320x256 kernel", g.M, g.N, g.K);
    return XFM_E_ARG;
  }
  const int tiles = cdiv(g.M, 320) * (g.N / 256);
  const int rc = nt_with_epilogue(epi, [&](auto e) {
    constexpr int E = decltype(e)::value;
    lds_launch<gemm_nt_320_kernel<E>, NT320_LDS>(dim3(tiles), dim3(512), NT320_LDS, st, g);
  });
  return rc != XFM_OK ? rc : xfm_check_launch("gemm_nt_320");
}
