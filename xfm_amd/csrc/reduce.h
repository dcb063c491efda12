// Wave and workgroup reductions of the small kernels, one copy each (included from common.h), and the 16-byte operand predicates
// of their host sides.
#pragma once

// host side: 16-byte vector loads and stores need a base on 16 bytes ...
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// ... and, for a [R, ld] fp32 operand read by rows, every row starting on 16 bytes
static inline bool rows_aligned16(const void* p, long ld) { return (ld & 3) == 0 && aligned16(p); }

#ifdef __HIPCC__
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One step of an argmin that keeps the LOWEST index among equal values (torch.argmin's rule): (ov, oi) replaces (v, i) when it is smaller
// in (value, index) order.  A NaN on either side replaces nothing.
__device__ __forceinline__ void argmin_merge(float& v, int& i, float ov, int oi) {
  if (ov < v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// Reductions over a 256-lane workgroup (four waves) through red, four floats of LDS that the caller supplies; every lane gets the
// result.  The first barrier waits for earlier readers of red, so calls may follow one another on the same four slots.
__device__ __forceinline__ void block_park256(float wave_value, float* red) {
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = wave_value;
  __syncthreads();
}
__device__ __forceinline__ float block_max256(float v, float* red) {
  block_park256(wave_max(v), red);
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
// The two sums differ in the tree over the four wave sums, and with it in the last bits of the result: a kernel keeps the one it has.
__device__ __forceinline__ float block_sum256(float v, float* red) {   // pairwise
  block_park256(wave_sum(v), red);
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float block_sum256_serial(float v, float* red) {   // left to right
  block_park256(wave_sum(v), red);
  return red[0] + red[1] + red[2] + red[3];
}
#endif
