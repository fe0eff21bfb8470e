// Shared device helpers for the gfx950 (CDNA4) kernels of this framework.
//
// Conventions
//  * bf16 tensors are handled as raw 16-bit words (uint16_t) in global memory and
//    widened to f32 in registers; every kernel accumulates in f32.
//  * Memory-bound kernels move 16 B per lane (8 x bf16) per access (CDNA guide G13).
//  * Wave size is 64 and is hard-coded (gfx950 has no wave32 mode for compute).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

namespace dtg {

constexpr int kWave = 64;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float bf2f(uint16_t v) {
  return __uint_as_float(static_cast<uint32_t>(v) << 16);
}

// Round-to-nearest-even f32 -> bf16; hipcc lowers the cast to v_cvt_pk_bf16_f32 on gfx950
// (NaN stays NaN, unlike integer-trick rounding: MI355X microarch "Correctness boundaries").
__device__ __forceinline__ uint16_t f2bf(float f) {
  __bf16 b = static_cast<__bf16>(f);
  return __builtin_bit_cast(uint16_t, b);
}

__device__ __forceinline__ void widen8(const u16x8& v, float* out) {
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = bf2f(v[i]);
}

__device__ __forceinline__ void load8(const uint16_t* p, float* out) {
  widen8(*reinterpret_cast<const u16x8*>(p), out);
}

__device__ __forceinline__ void store8(uint16_t* p, const float* in) {
  u16x8 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = f2bf(in[i]);
  *reinterpret_cast<u16x8*>(p) = v;
}

// 8 x f32 as two 16-byte accesses (p is 16-byte aligned).
__device__ __forceinline__ void load8f(const float* p, float* out) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w;
  out[4] = b.x; out[5] = b.y; out[6] = b.z; out[7] = b.w;
}

__device__ __forceinline__ void store8f(float* p, const float* v) {
  reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// One element / eight elements of a bf16 (as uint16_t) or f32 buffer, as f32.
__device__ __forceinline__ float ld(const uint16_t* p, int64_t i) { return bf2f(p[i]); }
__device__ __forceinline__ float ld(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ void st(uint16_t* p, int64_t i, float v) { p[i] = f2bf(v); }
__device__ __forceinline__ void st(float* p, int64_t i, float v) { p[i] = v; }
__device__ __forceinline__ void ld8(const uint16_t* p, float* o) { load8(p, o); }
__device__ __forceinline__ void ld8(const float* p, float* o) { load8f(p, o); }
__device__ __forceinline__ void st8(uint16_t* p, const float* v) { store8(p, v); }
__device__ __forceinline__ void st8(float* p, const float* v) { store8f(p, v); }

// Butterfly sum over aligned groups of W lanes (a power of two, at most the wave).
template <int W, typename T>
__device__ __forceinline__ T lanes_sum(T v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  return lanes_sum<kWave>(v);
}

template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

// Block-wide sum for blockDim.x <= 1024; `scratch` must hold blockDim.x/64 floats.
__device__ __forceinline__ float block_sum(float v, float* scratch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  float r = 0.f;
  for (int i = 0; i < nw; ++i) r += scratch[i];
  return r;
}

// Sums of two values over the workgroup; `scratch` holds 2 * blockDim.x / 64 floats.
__device__ __forceinline__ void block_sum2(float& a, float& b, float* scratch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  a = wave_sum(a);
  b = wave_sum(b);
  __syncthreads();
  if (lane == 0) {
    scratch[2 * wid] = a;
    scratch[2 * wid + 1] = b;
  }
  __syncthreads();
  a = b = 0.f;
  for (int i = 0; i < nw; ++i) {
    a += scratch[2 * i];
    b += scratch[2 * i + 1];
  }
}

__device__ __forceinline__ float block_max(float v, float* scratch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = wave_max(v);
  __syncthreads();
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  float r = -INFINITY;
  for (int i = 0; i < nw; ++i) r = fmaxf(r, scratch[i]);
  return r;
}

inline hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

inline const uint16_t* bf16_ptr(const at::Tensor& t) {
  return reinterpret_cast<const uint16_t*>(t.data_ptr());
}
inline uint16_t* bf16_mut(const at::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

#define DTG_CHECK(cond, ...) TORCH_CHECK(cond, "dtg: ", __VA_ARGS__)
#define DTG_CHECK_CUDA_BF16(t)                                                     \
  DTG_CHECK((t).is_cuda() && (t).scalar_type() == at::kBFloat16, #t " must be a bf16 GPU tensor")
#define DTG_LAUNCH_CHECK() C10_HIP_KERNEL_LAUNCH_CHECK()

// 8 x 8 transpose of 16-bit values held in registers: v[i] = row i on entry, column i on exit.
// Three butterfly stages (elements, pairs, quads); only the first needs byte permutes, the other
// two move whole dwords.
__device__ __forceinline__ void transpose8x8(u16x8 (&v)[8]) {
  u16x8 t[8], u[8];
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    t[i] = __builtin_shufflevector(v[i], v[i + 1], 0, 8, 2, 10, 4, 12, 6, 14);
    t[i + 1] = __builtin_shufflevector(v[i], v[i + 1], 1, 9, 3, 11, 5, 13, 7, 15);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = (k & 1) + 4 * (k >> 1);  // 0, 1, 4, 5
    u[i] = __builtin_shufflevector(t[i], t[i + 2], 0, 1, 8, 9, 4, 5, 12, 13);
    u[i + 2] = __builtin_shufflevector(t[i], t[i + 2], 2, 3, 10, 11, 6, 7, 14, 15);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = __builtin_shufflevector(u[i], u[i + 4], 0, 1, 2, 3, 8, 9, 10, 11);
    v[i + 4] = __builtin_shufflevector(u[i], u[i + 4], 4, 5, 6, 7, 12, 13, 14, 15);
  }
}

// LDS staging of the tile-transposing kernels.  A tile of 16-bit values with an even pitch P
// (tile width + 2 halfwords); rows go in as four dwords, columns come out as eight halfwords
// from consecutive rows.  `col` of lds_put8 is a multiple of 8.
template <int P>
__device__ __forceinline__ void lds_put8(uint16_t* tile, int row, int col, u16x8 v) {
  uint32_t* d = reinterpret_cast<uint32_t*>(tile + row * P + col);
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = (uint32_t)v[2 * j] | ((uint32_t)v[2 * j + 1] << 16);
}

template <int P>
__device__ __forceinline__ u16x8 lds_col8(const uint16_t* tile, int row, int col) {
  u16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = tile[(row + j) * P + col];
  return v;
}

// Grid of the tile-transposing streaming kernels: blockIdx.x = column tile (fastest, so the
// workgroups resident at one time read neighbouring segments of the same source rows),
// blockIdx.y = row tile.  A banded 1-D tile walk (column tiles grouped so that the transposed
// output rows are written in long runs) gained 4-8 % on a lone [T, 28672] transpose, was mixed
// on the SwiGLU backward and moved the 8B step < 0.5 % (profiles/r1/s62_tile_order_ab.md); it
// was removed in round 6 with the other opt-in tilings.
inline dim3 tile_grid(int64_t n_row_tiles, int64_t n_col_tiles) {
  DTG_CHECK(n_row_tiles <= 65535 && n_col_tiles < (int64_t(1) << 31), "tile grid: too many tiles");
  return dim3((unsigned)n_col_tiles, (unsigned)n_row_tiles);
}

}  // namespace dtg
