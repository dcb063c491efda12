// Small kernels around attention: the accumulator-layout bias copies (xfm_bias_tile), the fold of per-row dK / dV onto shared
// key/value sources (xfm_rows_index_sum) and the relative-position bias table (xfm_relpos_*).  Included by attention.hip.
// One 64-thread workgroup per (head, tile a, tile b): the tile in the accumulator layout of both kernels (see include/xfm_hip.h).
__global__ __launch_bounds__(64) void bias_tile_kernel(const float* __restrict__ bias, int S, long ld, float inv_scale, float* __restrict__ tiled,
                                                       float* __restrict__ tiled_t) {
  const int T = gridDim.x, a_ = blockIdx.y, b_ = blockIdx.x, h = blockIdx.z;   // a_ in [0, T]: tiled_t has one more key-tile row, all -1e30
  const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
  const float* bh = bias + (long)h * S * ld;
  const long tile = (((long)h * T + a_) * T + b_) * 256 + lane * 4;
  if (tiled != nullptr && a_ < T) {   // query 16a + lr, keys 16b + 4lg + r
    const int q = a_ * 16 + lr;
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = b_ * 16 + 4 * lg + r;
      v[r] = k < S ? (q < S ? bh[(long)q * ld + k] * inv_scale : 0.f) : -1.0e30f;
    }
    *reinterpret_cast<f32x4*>(tiled + tile) = v;
  }
  if (tiled_t != nullptr) {  // key 16a + lr, queries 16b + 4lg + r
    const int k = a_ * 16 + lr;
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = b_ * 16 + 4 * lg + r;
      v[r] = k < S ? (q < S ? bh[(long)q * ld + k] * inv_scale : 0.f) : -1.0e30f;
    }
    *reinterpret_cast<f32x4*>(tiled_t + (((long)h * (T + 1) + a_) * T + b_) * 256 + lane * 4) = v;
  }
}

int xfm_bias_tile_impl(const float* bias, int H, int S, long ld, float scale, float* tiled, float* tiled_t, hipStream_t st) {
  XFM_REQUIRE(bias != nullptr && H > 0 && S > 0 && ld >= S && scale > 0.f, "bias_tile: bad arguments");
  XFM_REQUIRE(((uintptr_t)tiled % 16) == 0 && ((uintptr_t)tiled_t % 16) == 0, "bias_tile: outputs must be 16-byte aligned");
  const int T = cdiv(S, 16);
  hipLaunchKernelGGL(bias_tile_kernel, dim3(T, T + 1, H), dim3(64), 0, st, bias, S, ld, 1.0f / scale, tiled, tiled_t);
  return xfm_check_launch("bias_tile");
}

// ---------------------------------------------------------------------------------------------
// dst[u, :] = sum over r with index[r] == u of src[r, :]   (bf16 in/out, fp32 accumulation; rows of `len` elements).
// Folds the per-query-row dK/dV of deduplicated key/value sources back onto the unique sources.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rows_index_sum_kernel(const bf16* __restrict__ src, const int* __restrict__ index, int R,
                                                             long len, bf16* __restrict__ dst) {
  const int u = blockIdx.y;
  const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (e >= len) return;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < R; ++r) {
    if (index[r] != u) continue;  // block-uniform
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + (long)r * len + e);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += bf2f(v[i]);
  }
  bf16x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = f2bf(acc[i]);
  *reinterpret_cast<bf16x8*>(dst + (long)u * len + e) = o;
}

int xfm_rows_index_sum_impl(const void* src, const int* index, int R, int U, long len, void* dst, hipStream_t st) {
  XFM_REQUIRE(R > 0 && U > 0 && len > 0 && len % 8 == 0 && U <= 65535, "rows_index_sum: bad shape R=%d U=%d len=%ld", R, U, len);
  hipLaunchKernelGGL(rows_index_sum_kernel, dim3(cdiv(len, 256 * 8), U), dim3(256), 0, st, (const bf16*)src, index, R, len, (bf16*)dst);
  return xfm_check_launch("rows_index_sum");
}

// ---------------------------------------------------------------------------------------------
// relative-position bias: dense[h,i,j] = table[index[i,j], h]  (beit2.py:139-145) and its transpose-scatter gradient
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void relpos_gather_kernel(const float* __restrict__ table, const int* __restrict__ index, int H,
                                                            int N, long ld, float* __restrict__ dense, float* __restrict__ dense_t) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)H * N * ld;
  if (t >= total) return;
  const int j = (int)(t % ld);
  const int i = (int)((t / ld) % N);
  const int h = (int)(t / (ld * N));
  dense[t] = (j < N) ? table[(long)index[i * N + j] * H + h] : 0.f;
  if (dense_t != nullptr) dense_t[t] = (j < N) ? table[(long)index[j * N + i] * H + h] : 0.f;  // [h][key i][query j]
}
__global__ __launch_bounds__(256) void relpos_scatter_kernel(const float* __restrict__ ddense, const int* __restrict__ index, int H,
                                                             int N, long ld, float* __restrict__ dtable) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)H * N * N;
  if (t >= total) return;
  const int j = (int)(t % N);
  const int i = (int)((t / N) % N);
  const int h = (int)(t / ((long)N * N));
  atomicAdd(dtable + (long)index[i * N + j] * H + h, ddense[((long)h * N + i) * ld + j]);
}

int xfm_relpos_gather_impl(const float* table, const int* index, int H, int N, long ld, float* dense, float* dense_t, hipStream_t st) {
  XFM_REQUIRE(H > 0 && N > 0 && ld >= N && ld % 4 == 0, "relpos_gather: bad shape H=%d N=%d ld=%ld", H, N, ld);
  const long total = (long)H * N * ld;
  hipLaunchKernelGGL(relpos_gather_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, table, index, H, N, ld, dense, dense_t);
  return xfm_check_launch("relpos_gather");
}
// Gather form of the same gradient: positions (i*N + j) pre-sorted by table entry (order, start[e] .. start[e+1]), one workgroup
// per entry, wave w sums heads w, w+4, ... over the entry's positions -- no atomics (the scatter above piles ~53, and for the
// three cls entries up to 196, colliding fp32 atomics on each of the 732 x H addresses and takes 58 us for 0.5 M elements).
__global__ __launch_bounds__(256) void relpos_gather_grad_kernel(const float* __restrict__ ddense, const int* __restrict__ order,
                                                                 const int* __restrict__ start, int H, int N, long ld,
                                                                 float* __restrict__ dtable) {
  const int e = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p0 = start[e], p1 = start[e + 1];
  for (int h = w; h < H; h += 4) {
    const float* src = ddense + (long)h * N * ld;
    float t = 0.f;
    for (int p = p0 + lane; p < p1; p += 64) {
      const int pos = order[p];
      t += src[(long)(pos / N) * ld + pos % N];
    }
    t = wave_sum(t);
    if (lane == 0) dtable[(long)e * H + h] += t;
  }
}

// The same gradient for the STANDARD index of a G x G patch grid plus a cls token (build_relative_position_index, beit2.py:92-116):
// entry e = (yi - yj + G - 1)(2G - 1) + (xi - xj + G - 1) for patch query (yi, xi) and patch key (yj, xj); the last three entries are
// cls -> patch, patch -> cls, cls -> cls.  The sorted gather above gives every lane one position of an entry: consecutive positions of
// an entry are ld + 1 floats apart, so each 4-byte read costs a 64-byte sector (144 us per layer at 901 tokens).  Here a workgroup is one
// (head, dy) row of the table and lane = dx: for a query (yi, xi) the lanes read the keys (yi - dy, xi - dx), 2G - 1 CONSECUTIVE
// floats of one bias row (reversed) -- every element of ddense is read once, coalesced.  The four waves split the query rows yi and are
// summed in a fixed order (no atomics: a table entry has one owner).
__global__ __launch_bounds__(256) void relpos_grid_grad_kernel(const float* __restrict__ ddense, int H, int G, long ld, float* __restrict__ dtable) {
  __shared__ float red[4][64];
  const int h = blockIdx.y, row = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int N = G * G + 1, W = 2 * G - 1, nrd = W * W + 3;
  const float* src = ddense + (long)h * N * ld;
  if (row == W) {  // the three cls entries
    float a = 0.f, b = 0.f;
    for (int j = 1 + threadIdx.x; j < N; j += 256) a += src[j];
    for (int i = 1 + threadIdx.x; i < N; i += 256) b += src[(long)i * ld];
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) { red[w][0] = a; red[w][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
      dtable[(long)(nrd - 3) * H + h] += (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
      dtable[(long)(nrd - 2) * H + h] += (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
      dtable[(long)(nrd - 1) * H + h] += src[0];
    }
    return;
  }
  const int dy = row - (G - 1);
  const int y0 = dy > 0 ? dy : 0, y1 = dy < 0 ? G + dy : G;  // query rows whose key row yi - dy exists
  for (int dx0 = 0; dx0 < W; dx0 += 64) {  // (2G - 1 <= 64 up to a 32 x 32 grid: one trip)
    const int dxl = dx0 + lane, dx = dxl - (G - 1);
    float acc = 0.f;
    for (int yi = y0 + w; yi < y1; yi += 4) {
      const float* rowp = src + (long)(1 + yi * G) * ld + 1 + (yi - dy) * G - dx;  // + xi * ld + xi per query column
#pragma unroll 6
      for (int xi = 0; xi < G; ++xi) {
        const int xj = xi - dx;
        if (dxl < W && xj >= 0 && xj < G) acc += rowp[(long)xi * ld + xi];
      }
    }
    red[w][lane] = acc;
    __syncthreads();
    if (w == 0 && dxl < W) dtable[((long)row * W + dxl) * H + h] += (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    __syncthreads();
  }
}
int xfm_relpos_grid_grad_impl(const float* ddense, int H, int G, long ld, float* dtable, hipStream_t st) {
  XFM_REQUIRE(H > 0 && G > 0 && ld >= (long)G * G + 1, "relpos_grid_grad: bad shape H=%d G=%d ld=%ld", H, G, ld);
  hipLaunchKernelGGL(relpos_grid_grad_kernel, dim3(2 * G, H), dim3(256), 0, st, ddense, H, G, ld, dtable);
  return xfm_check_launch("relpos_grid_grad");
}

int xfm_relpos_scatter_sorted_impl(const float* ddense, const int* order, const int* start, int entries, int H, int N, long ld,
                                   float* dtable, hipStream_t st) {
  XFM_REQUIRE(H > 0 && N > 0 && ld >= N && entries > 0, "relpos_scatter_sorted: bad shape");
  hipLaunchKernelGGL(relpos_gather_grad_kernel, dim3(entries), dim3(256), 0, st, ddense, order, start, H, N, ld, dtable);
  return xfm_check_launch("relpos_scatter_sorted");
}

int xfm_relpos_scatter_impl(const float* ddense, const int* index, int H, int N, long ld, float* dtable, hipStream_t st) {
  XFM_REQUIRE(H > 0 && N > 0 && ld >= N, "relpos_scatter: bad shape");
  const long total = (long)H * N * N;
  hipLaunchKernelGGL(relpos_scatter_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, ddense, index, H, N, ld, dtable);
  return xfm_check_launch("relpos_scatter");
}
