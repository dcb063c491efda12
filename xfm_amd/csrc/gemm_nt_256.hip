// gemm_nt, 256 x 256 phase pipeline (gemm_common.h): the kernel, its launch and the XFM_DIAG timeline hook.

// ---------------------------------------------------------------------------------------------
// 256 x 256 tile, 8 waves as 2 (M) x 4 (N), each wave a 128 x 64 output block (128 accumulator VGPRs).  Against the
// 256 x 128 ring this halves the LDS fragment bytes read per MFMA (24 ds_read_b128 per 64 MFMA) and the global->LDS
// bytes per FLOP -- the two rates that bound the ring kernel.
//
// LDS = 2 K-tile buffers x (X 256 rows + W 256 rows) x 128 B = 128 KiB, filled by direct-to-LDS loads in UNITS of 128 rows
// (16 KiB = 2 wave-instructions per wave), ordered by when the compute phases need them:
//   U0 = X rows {0-63, 128-191} (the "a0" half of both M-wave rows)      U1 = W rows {wc*64 + 0-31}  ("b0")
//   U2 = W rows {wc*64 + 32-63} ("b1")                                    U3 = X rows {64-127, 192-255} ("a1")
// A K-tile is computed in 4 phases of 16 MFMA: P0 reads a0,b0 -> (a0,b0); P1 reads b1 -> (a0,b1); P2 reads a1 ->
// (a1,b1); P3 reads nothing -> (a1,b0).  Phase index ph = 4*kt + p issues unit ph+5, so every unit flies >= 4 phases and
// three units (6 loads per wave) stay in flight across every barrier: s_waitcnt vmcnt(6) at the end of a phase retires
// exactly the unit(s) the NEXT phase reads.  A unit overwrites the unit 8 places back, whose last ds_read was >= 3
// phases earlier.
// The two M-wave groups (one wave of each per SIMD) run half a phase apart -- group 1 takes one extra barrier up
// front -- so one group's MFMA section overlaps the other's ds_read/glds section (two barriers per phase).
// RAW: a wave's share of a unit is retired by its own counted vmcnt before barrier #1 of phase ph; readers touch it
// in phase ph+1, i.e. after barrier #2 of phase ph, which every wave of both groups reaches after that wait.
// ---------------------------------------------------------------------------------------------
template <int J>
__device__ __forceinline__ int unit_row(int u) {  // row of the X (J = 0, 3) or W (J = 1, 2) tile held by unit row u
  if (J == 0) return u + (u & 64);
  if (J == 3) return u + 64 + (u & 64);
  if (J == 1) return ((u >> 5) << 6) + (u & 31);
  return ((u >> 5) << 6) + 32 + (u & 31);
}

template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// leave the y youngest staging units (2 loads each) in flight, plus NS more memory operations (the previous tile's output stores,
// issued between the staging units of the prologue and those of the K loop)
template <int NS, int YMAX>
__device__ __forceinline__ void wait_units(int y) {
  if (YMAX >= 5 && y == 5) wait_vm<10 + NS>();
  else if (YMAX >= 4 && y == 4) wait_vm<8 + NS>();
  else if (y >= 3) wait_vm<6 + NS>();
  else if (y == 2) wait_vm<4 + NS>();
  else if (y == 1) wait_vm<2 + NS>();
  else wait_vm<NS>();
}
// Ring form of the pipeline above: the staging units live in R = D + 3 slots of 16 KiB (unit s in slot s mod R, its 128 rows
// contiguous), phase ph issues unit ph + D, and D - 2 units (2 (D - 2) loads per wave) stay in flight across every barrier.  D = 5 is
// the schedule described above in 128 KiB.
//
// PERSIST: one workgroup per CU walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... (the same tile -> XCD assignment as one
// workgroup per tile, gridDim.x being a multiple of 8).  The first D units of the NEXT tile are issued before the epilogue of this
// one -- LDS is free once the K loop is over -- so the next tile's first-K-tile latency and this tile's output stores (whose
// acknowledgement a terminating wave would have to wait for) overlap instead of adding up with a workgroup launch in between.
// CDNA counts stores in vmcnt, in issue order with the loads: an interior tile issues exactly NS output stores per lane between
// unit D - 1 and unit D of the next tile, and the waits that retire units 1..3 allow for them; the wait that retires unit 5 (P3 of
// K-tile 0) is the first that needs the stores acknowledged.
constexpr int NT256_D = 5;  // look-ahead in staging units
template <int EPI, bool PERSIST>
__global__ __launch_bounds__(512) void gemm_nt_256_kernel(GemmNT g, int tiles) {
  constexpr int BM = 256, BN = 256, MT = 8, NT = 4;
  constexpr int D = NT256_D, R = D + 3, UNIT = 128 * 128;
  // output stores per lane of an interior tile (16-B stores; fp32 output: two per 8 columns; GELU also stores gelu')
  constexpr int NS = !PERSIST ? 0 : EPI == EPI_GELU || EPI == EPI_F32 ? 32 : EPI == EPI_F32_ACC ? 0 : 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 2, wc = w & 3;
  const int lr = lane & 15, lg = lane >> 4;
  const int tiles_n = (g.N + BN - 1) / BN, tiles_m = (g.M + BM - 1) / BM;
  const int nk = g.K / 64;
  const int total = 4 * nk;  // staging units

  // per-lane global element offsets of the 8 (unit, instruction) loads of a tile; the K offset is added per K-tile.  Instruction i
  // of wave w fills the 1-KiB block (i*8 + w) of the unit's slot: unit rows (i*8 + w)*8 + (lane >> 3), 16-B chunk lane & 7.
  unsigned soff[4][2];
  auto tile_origin = [&](int v, int& m0, int& n0) {
    int tm, tn;
    grouped_tile(xcd_remap(v, tiles), tiles_m, tiles_n, g.group_m, tm, tn);
    m0 = tm * BM;
    n0 = tn * BN;
  };
  auto tile_offsets = [&](int m0, int n0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int u = (i * 8 + w) * 8 + (lane >> 3);
      {
        const int r = unit_row<0>(u);
        int gr = m0 + r; gr = gr < g.M ? gr : g.M - 1;
        soff[0][i] = (unsigned)gr * (unsigned)g.lda + (((lane & 7) ^ swz_x(r)) << 3);
      }
      {
        const int r = unit_row<3>(u);
        int gr = m0 + r; gr = gr < g.M ? gr : g.M - 1;
        soff[3][i] = (unsigned)gr * (unsigned)g.lda + (((lane & 7) ^ swz_x(r)) << 3);
      }
      {
        const int r = unit_row<1>(u);
        int gr = n0 + r; gr = gr < g.N ? gr : g.N - 1;
        soff[1][i] = (unsigned)gr * (unsigned)g.ldb + (((lane & 7) ^ swz_w(r)) << 3);
      }
      {
        const int r = unit_row<2>(u);
        int gr = n0 + r; gr = gr < g.N ? gr : g.N - 1;
        soff[2][i] = (unsigned)gr * (unsigned)g.ldb + (((lane & 7) ^ swz_w(r)) << 3);
      }
    }
  };
  int iss = 0;  // ring slot of the next unit to issue
  auto issue = [&](int s) {  // unit s = (K-tile s >> 2, part s & 3) into slot iss; wave-uniform branch
    char* base = smem + iss * UNIT + w * 1024;
    iss = iss + 1 == R ? 0 : iss + 1;
    if (s >= total) return;
    const int j = s & 3;
    const bf16* src = ((j == 0 || j == 3) ? g.A : g.B) + (s >> 2) * 64;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned so = j == 0 ? soff[0][i] : j == 1 ? soff[1][i] : j == 2 ? soff[2][i] : soff[3][i];
      // inline asm on purpose: a direct-to-LDS load the compiler can see is drained (s_waitcnt vmcnt(0)) in front of the ds_reads
      // it cannot prove disjoint from it -- every read of a ring slot
      const unsigned lds_addr = (unsigned)(uintptr_t)LDS_PTR(void, base) + (unsigned)(i * 8192);
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src + (size_t)so), "s"(lds_addr) : "memory", "m0");
    }
  };

  f32x4 acc[MT][NT];

  // per-lane byte offsets of the fragment reads inside a unit's slot (the 16-B chunk index ks*4 + lg is XOR-ed with the row swizzle,
  // which only depends on the low row bits the unit row shares with the tile row):
  //   X units (a0 / a1): tile rows wr*128 + half*64 + m*16 + lr -> unit rows wr*64 + m*16 + lr
  //   W units (b0 / b1): tile rows wc*64 + half*32 + 4*n + 8*(lr>>2) + (lr&3) -> unit rows wc*32 + 4*n + 8*(lr>>2) + (lr&3)
  const int xs = swz_x(lr);
  const int wu = 8 * (lr >> 2) + (lr & 3);
  const int ws = swz_w(wu);
  const int xbase0 = (wr * 64 + lr) * 128 + (((0 + lg) ^ xs) << 4), xbase1 = (wr * 64 + lr) * 128 + (((4 + lg) ^ xs) << 4);
  const int wbase0 = (wc * 32 + wu) * 128 + (((0 + lg) ^ ws) << 4), wbase1 = (wc * 32 + wu) * 128 + (((4 + lg) ^ ws) << 4);

  bf16x8 xa[4][2], wb0[2][2], wb1[2][2];
  auto read_x = [&](const char* slot) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      xa[m][0] = *reinterpret_cast<const bf16x8*>(slot + xbase0 + m * 2048);
      xa[m][1] = *reinterpret_cast<const bf16x8*>(slot + xbase1 + m * 2048);
    }
  };
  auto read_w = [&](const char* slot, bf16x8 (&wb)[2][2]) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      wb[n][0] = *reinterpret_cast<const bf16x8*>(slot + wbase0 + n * 512);
      wb[n][1] = *reinterpret_cast<const bf16x8*>(slot + wbase1 + n * 512);
    }
  };
#define XFM_QUAD(MH, NH, WB)                                                                                     \
  do {                                                                                                           \
    __builtin_amdgcn_s_setprio(1);                                                                               \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                             \
    _Pragma("unroll") for (int m = 0; m < 4; ++m)                                                                \
    _Pragma("unroll") for (int n = 0; n < 2; ++n)                                                                \
      acc[MH * 4 + m][NH * 2 + n] =                                                                              \
          __builtin_amdgcn_mfma_f32_16x16x32_bf16(WB[n][ks], xa[m][ks], acc[MH * 4 + m][NH * 2 + n], 0, 0, 0);  \
    __builtin_amdgcn_s_setprio(0);                                                                               \
  } while (0)

  int v = blockIdx.x, m0, n0;
  tile_origin(v, m0, n0);
  tile_offsets(m0, n0);
  // prologue: units 0..D-1 in flight
#pragma unroll
  for (int s = 0; s < D; ++s) issue(s);
  bool stores_behind = false;  // NS output stores of the previous tile were issued after the units 0..D-1 of this one

#ifdef XFM_DIAG
  int dbg_n = 0;
#endif
  while (true) {
#ifdef XFM_DIAG
    if (g.dbg != nullptr && tid == 0) {
      long long* d = g.dbg + ((long)blockIdx.x * 8 + dbg_n) * 4;
      d[0] = v; d[1] = wall_clock64();
    }
#endif
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // units 0 and 1 (a0, b0 of K-tile 0) retired and visible
    {
      const int y = (total - 1 < D - 1 ? total - 1 : D - 1) - 1;
      if (NS > 0 && stores_behind) wait_units<NS, D - 2>(y);
      else wait_units<0, D - 2>(y);
    }
    XFM_BAR();
    if (wr == 1) XFM_BAR();  // stagger the second M-wave group by one barrier

    int rs = 0;  // ring slot of unit 4*kt
    for (int kt = 0; kt < nk; ++kt) {
      const int ph = 4 * kt;
      const bool plus = NS > 0 && stores_behind && kt == 0;
      const char* s_a0 = smem + rs * UNIT;
      const char* s_b0 = smem + (rs + 1 >= R ? rs + 1 - R : rs + 1) * UNIT;
      const char* s_b1 = smem + (rs + 2 >= R ? rs + 2 - R : rs + 2) * UNIT;
      const char* s_a1 = smem + (rs + 3 >= R ? rs + 3 - R : rs + 3) * UNIT;
      rs = rs + 4 >= R ? rs + 4 - R : rs + 4;
      int last;
      // ---- P0: (a0, b0)
      issue(ph + D);
      read_x(s_a0);
      read_w(s_b0, wb0);
      last = ph + D < total ? ph + D : total - 1;
      if (plus) wait_units<NS, D - 2>(last - (ph + 2));
      else wait_units<0, D - 2>(last - (ph + 2));
      XFM_BAR();
      XFM_QUAD(0, 0, wb0);
      XFM_BAR();
      // ---- P1: (a0, b1)
      issue(ph + D + 1);
      read_w(s_b1, wb1);
      last = ph + D + 1 < total ? ph + D + 1 : total - 1;
      if (plus) wait_units<NS, D - 2>(last - (ph + 3));
      else wait_units<0, D - 2>(last - (ph + 3));
      XFM_BAR();
      XFM_QUAD(0, 1, wb1);
      XFM_BAR();
      // ---- P2: (a1, b1)
      issue(ph + D + 2);
      read_x(s_a1);
      XFM_BAR();
      XFM_QUAD(1, 1, wb1);
      XFM_BAR();
      // ---- P3: (a1, b0); retire a0, b0 of the next K-tile
      issue(ph + D + 3);
      last = ph + D + 3 < total ? ph + D + 3 : total - 1;
      wait_units<0, D - 2>(last - (ph + 5) < 0 ? 0 : last - (ph + 5));
      XFM_BAR();
      XFM_QUAD(1, 0, wb0);
      XFM_BAR();
    }
    if (wr == 0) XFM_BAR();  // both groups are past their last LDS read
#ifdef XFM_DIAG
    if (g.dbg != nullptr && tid == 0) g.dbg[((long)blockIdx.x * 8 + dbg_n) * 4 + 2] = wall_clock64();
#endif
    const int cm0 = m0, cn0 = n0;
    // The bias goes out BEFORE the next tile's staging loads and is waited for with a count that leaves exactly those in flight
    // (loads return in order): this wave's 64 values, into the last ring slot (free until P2 of the next tile's first K-tile).
    // (DGELU's gelu'(x) chunks are still loaded inside the epilogue, behind the staging loads: 64 more live registers do not fit.)
    float* lds_bias = reinterpret_cast<float*>(smem + (R - 1) * UNIT + w * 256);
    if (g.bias != nullptr) {
      int col = cn0 + wc * 64 + lane;
      col = col < g.N ? col : g.N - 1;
      const unsigned lds_addr = (unsigned)(uintptr_t)LDS_PTR(void, lds_bias);
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(g.bias + col), "s"(lds_addr) : "memory", "m0");
    } else {
      lds_bias[lane] = 0.f;
    }
    v += gridDim.x;
    const bool more = PERSIST && v < tiles;
    int ahead = 0;  // staging units of the next tile in flight
    if (more) {
      tile_origin(v, m0, n0);
      tile_offsets(m0, n0);
      iss = 0;
#pragma unroll
      for (int s = 0; s < D; ++s) issue(s);
      ahead = total < D ? total : D;
    }
    wait_units<0, D>(ahead);
    if (g.bias == nullptr) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    gemm_epilogue<MT, NT, EPI>(g, acc, cm0 + wr * 128, cn0 + wc * 64, lr, lg, lds_bias);
#ifdef XFM_DIAG
    if (g.dbg != nullptr && tid == 0) {
      g.dbg[((long)blockIdx.x * 8 + dbg_n) * 4 + 3] = wall_clock64();
      dbg_n = dbg_n < 7 ? dbg_n + 1 : 7;
    }
#endif
    if (!more) break;
    XFM_FENCE();
    // exactly NS stores per lane only when every lane stored every (mt, np) with one 16-B (2 x 16-B for fp32) instruction
    stores_behind = cm0 + BM <= g.M && cn0 + BN <= g.N && (g.ldc % 8) == 0 && (EPI != EPI_GELU || (g.ldaux % 8) == 0);
  }
#undef XFM_QUAD
}

// ---- host side ----
// the kernel's per-lane staging offsets (row * ld + chunk) are 32-bit element offsets
static bool nt256_eligible(int M, long lda, int N, long ldb) {
  return (unsigned long)M * (unsigned long)lda < (1ul << 32) && (unsigned long)N * (unsigned long)ldb < (1ul << 32);
}

#ifdef XFM_DIAG
// Diagnostic build: where the next launches of the 256 x 256 kernel put their stamps (xfm_diag_set_timeline, capi.hip); ptr NULL = off
static XfmTimeline nt256_timeline = {nullptr, 0, 0};
#endif

static int launch_nt_256(const GemmNT& g_in, int epi, hipStream_t st) {
  GemmNT g = g_in;
  const int tiles = cdiv(g.M, 256) * cdiv(g.N, 256);
  if (!nt256_eligible(g.M, g.lda, g.N, g.ldb)) {
    xfm_set_error("gemm_nt: operand too large for the 256x256 kernel's 32-bit element offsets");
    return XFM_E_ARG;
  }
  // more tiles than CUs: one persistent workgroup per CU (XFM_GEMM_PERSIST=0: one workgroup per tile)
  static const int persist_env = xfm_env_int("XFM_GEMM_PERSIST", 1);
  static const int cus = xfm_cu_count();
  const bool persist = persist_env && cus >= 8 && tiles > cus;
  const int grid = persist ? cus & ~7 : tiles;
#ifdef XFM_DIAG
  g.dbg = nt256_timeline.ptr;
  if (g.dbg != nullptr && nt256_timeline.bytes < (size_t)grid * XFM_NT256_STAMP_BYTES) {   // 8 tiles x 4 stamps per workgroup
    xfm_set_error("gemm_nt_256: timeline buffer of %zu bytes is short of %d workgroups x %d: launched without stamps", nt256_timeline.bytes, grid,
                  XFM_NT256_STAMP_BYTES);
    g.dbg = nullptr;
  }
#endif
  constexpr int lds = (NT256_D + 3) * 128 * 128;
  const int rc = nt_with_epilogue(epi, [&](auto e) {
    constexpr int E = decltype(e)::value;
    if (persist) lds_launch<gemm_nt_256_kernel<E, true>, lds>(dim3(grid), dim3(512), lds, st, g, tiles);
    else lds_launch<gemm_nt_256_kernel<E, false>, lds>(dim3(grid), dim3(512), lds, st, g, tiles);
  });
  return rc != XFM_OK ? rc : xfm_check_launch("gemm_nt_256");
}
