// The MLP activation kernels, shared by gelu.hip and swiglu.hip and parameterised by an
// activation functor:
//
//   struct Act {
//     static constexpr int kIn;   // width-I column blocks of a pre-activation row (= gradient blocks)
//     static __device__ float fwd(const float (&x)[kIn]);                                   // h
//     static __device__ void bwd(const float (&x)[kIn], float d, float (&dx)[kIn], float& h);
//   };
//
// x is [T, kIn * I] with row stride x_stride (block k of row t at x + t * x_stride + k * I), h and
// dh are [T, I], dx is [T, kIn * I], all bf16; f32 math, one rounding on store.  bwd also returns
// the recomputed h = fwd(x), which only the tiled kernel stores.
#pragma once

#include "common.h"

namespace dtg {
namespace mlp_act {

// SwiGLU on a fused gate|up row, x = {gate, up}: h = silu(gate) * up.  Lives here because the skinny GEMM's
// epilogue (skinny_gemm.hip) applies the same functor as swiglu.hip, bit for bit.
struct SwiGLU {
  static constexpr int kIn = 2;  // x = {gate, up}

  static __device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

  static __device__ __forceinline__ float fwd(const float (&x)[2]) {
    const float g = x[0], u = x[1];
    return g * sigmoidf_(g) * u;
  }

  static __device__ __forceinline__ void bwd(const float (&x)[2], float d, float (&dx)[2], float& h) {
    const float g = x[0], u = x[1];
    const float sg = sigmoidf_(g);
    const float silu = g * sg;
    dx[1] = d * silu;
    dx[0] = d * u * sg * (1.f + g * (1.f - sg));
    h = silu * u;
  }
};

template <class Act>
__global__ void act_fwd_kernel(const uint16_t* __restrict__ x, int64_t x_stride, uint16_t* __restrict__ h, int64_t T,
                               int I) {
  constexpr int K = Act::kIn;
  const int chunks = I >> 3;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= T * chunks) return;
  const int64_t t = gid / chunks;
  const int c = (gid % chunks) * 8;
  float v[K][8], o[8];
#pragma unroll
  for (int k = 0; k < K; ++k) load8(x + t * x_stride + k * I + c, v[k]);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float in[K];
#pragma unroll
    for (int k = 0; k < K; ++k) in[k] = v[k][j];
    o[j] = Act::fwd(in);
  }
  store8(h + t * I + c, o);
}

template <class Act>
__global__ void act_bwd_kernel(const uint16_t* __restrict__ dh, const uint16_t* __restrict__ x, int64_t x_stride,
                               uint16_t* __restrict__ dx, int64_t T, int I) {
  constexpr int K = Act::kIn;
  const int chunks = I >> 3;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= T * chunks) return;
  const int64_t t = gid / chunks;
  const int c = (gid % chunks) * 8;
  float v[K][8], d[8], o[K][8];
#pragma unroll
  for (int k = 0; k < K; ++k) load8(x + t * x_stride + k * I + c, v[k]);
  load8(dh + t * I + c, d);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float in[K], g[K], h;
#pragma unroll
    for (int k = 0; k < K; ++k) in[k] = v[k][j];
    Act::bwd(in, d[j], g, h);
#pragma unroll
    for (int k = 0; k < K; ++k) o[k][j] = g[k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) store8(dx + t * K * I + k * I + c, o[k]);
}

// Backward that also emits the operands of the MLP's weight-gradient GEMMs in K-contiguous
// (token-minor) layout, so hipBLASLt runs them as "TN" without separate transpose passes:
//   dx  [T, kIn * I]   (row-major, for dX = dx @ W_in)
//   dxT [kIn * I, T]   (for dW_in = dxT @ X)
//   hT  [I, T]         (h recomputed from x, for dW_out = dY^T @ h)
// One workgroup owns a kTT-token x kTF-feature tile: 16-byte row loads of the kIn blocks of x and
// of dh (kTF x 2-byte segments of kTT token rows); the kIn + 1 transposed tiles are staged through
// LDS (pitch kTF + 2 halfwords) and stored as 16-byte columns (kTT x 2-byte segments of kTF
// feature rows).
// 64 x 128 is the measured best of the 64/128 x 64/128 tiles and of a register-blocked 8 x 8
// form (-2.1 ms per 8B step against 64 x 64, profiles/r3/s32; 4.64 vs 4.52 TB/s against the
// register-blocked one, profiles/r5/transpose/); the others were removed in round 6.  Staging the
// three outputs of SwiGLU one after another through a single 16.6 KB buffer doubled the occupancy
// (6 instead of 3 waves per SIMD) and changed nothing: 5.53 vs 5.50 TB/s, step 581.0 vs 580.7 ms
// (profiles/r6/swiglu_seq/).
constexpr int kTT = 64, kTF = 128;
constexpr int kThreads = 256;

template <class Act>
__global__ __launch_bounds__(kThreads) void act_bwd_t_kernel(const uint16_t* __restrict__ dh,
                                                             const uint16_t* __restrict__ x, int64_t x_stride,
                                                             uint16_t* __restrict__ dx, uint16_t* __restrict__ dxT,
                                                             uint16_t* __restrict__ hT, int64_t T, int I) {
  constexpr int K = Act::kIn;
  constexpr int kPitch = kTF + 2;
  constexpr int kVF = kTF / 8;                  // 16-byte vectors per token row of the tile
  constexpr int kRowsPerPass = kThreads / kVF;  // token rows per phase-1 pass
  constexpr int kVT = kTT / 8;                  // 16-byte vectors per transposed row segment
  constexpr int kOutPerPass = kThreads / kVT;   // feature rows per phase-2 pass
  constexpr int kNP = kTT / kRowsPerPass;
  static_assert(kThreads == 256 && kThreads % kVF == 0 && kThreads % kVT == 0, "one vector per lane and pass");
  static_assert(kTT % kRowsPerPass == 0 && kTF % kOutPerPass == 0, "whole passes");
  static_assert(kPitch % 2 == 0, "lds_put8 writes dwords");
  __shared__ uint16_t tiles[(K + 1) * kTT * kPitch];  // dx block 0 .. K-1, then h
  const int64_t t0 = (int64_t)blockIdx.y * kTT;
  const int c0 = (int)blockIdx.x * kTF;
  const int tid = threadIdx.x;
  // all loads of the tile first ((K + 1) * kNP vectors per lane in flight), then the math
  u16x8 rx[K][kNP], rd[kNP];
#pragma unroll
  for (int i = 0; i < kNP; ++i) {
    const int64_t t = t0 + tid / kVF + kRowsPerPass * i;
    const int c = c0 + (tid % kVF) * 8;
    if (t < T && c < I) {
#pragma unroll
      for (int k = 0; k < K; ++k) rx[k][i] = *reinterpret_cast<const u16x8*>(x + t * x_stride + k * I + c);
      rd[i] = *reinterpret_cast<const u16x8*>(dh + t * I + c);
    }
  }
#pragma unroll
  for (int i = 0; i < kNP; ++i) {
    const int lt = tid / kVF + kRowsPerPass * i;
    const int lc = (tid % kVF) * 8;
    const int64_t t = t0 + lt;
    const int c = c0 + lc;
    u16x8 vdx[K], vh = {0, 0, 0, 0, 0, 0, 0, 0};  // out-of-range vectors reach LDS as zeros
#pragma unroll
    for (int k = 0; k < K; ++k) vdx[k] = vh;
    if (t < T && c < I) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float in[K], g[K], h;
#pragma unroll
        for (int k = 0; k < K; ++k) in[k] = bf2f(rx[k][i][j]);
        Act::bwd(in, bf2f(rd[i][j]), g, h);
#pragma unroll
        for (int k = 0; k < K; ++k) vdx[k][j] = f2bf(g[k]);
        vh[j] = f2bf(h);
      }
#pragma unroll
      for (int k = 0; k < K; ++k) *reinterpret_cast<u16x8*>(dx + t * K * I + k * I + c) = vdx[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) lds_put8<kPitch>(tiles + k * kTT * kPitch, lt, lc, vdx[k]);
    lds_put8<kPitch>(tiles + K * kTT * kPitch, lt, lc, vh);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kTF / kOutPerPass; ++i) {
    const int oc = tid / kVT + kOutPerPass * i;  // feature within the tile -> output row
    const int ot = (tid % kVT) * 8;              // first token of this 8-token vector
    const int c = c0 + oc;
    const int64_t t = t0 + ot;
    if (c >= I || t >= T) continue;
    u16x8 o[K + 1];  // every column first, then the stores
#pragma unroll
    for (int k = 0; k <= K; ++k) o[k] = lds_col8<kPitch>(tiles + k * kTT * kPitch, ot, oc);
#pragma unroll
    for (int k = 0; k < K; ++k) *reinterpret_cast<u16x8*>(dxT + (int64_t)(k * I + c) * T + t) = o[k];
    *reinterpret_cast<u16x8*>(hT + (int64_t)c * T + t) = o[K];
  }
}

// The pre-activation: [T, kIn * I] bf16 on the GPU, unit inner stride, 16-byte aligned rows, whole
// 8-element vectors in every block.  Returns I.
template <class Act>
int check_x(const at::Tensor& x, const char* op) {
  DTG_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2 && x.stride(1) == 1 &&
                x.stride(0) % 8 == 0 && x.size(1) % (8 * Act::kIn) == 0,
            op, ": the pre-activation must be a bf16 GPU tensor [T, ", Act::kIn,
            " * I] with unit inner stride, 16-byte aligned rows and I % 8 == 0");
  return (int)(x.size(1) / Act::kIn);
}

// dh: bf16 [T, I] on the GPU, made contiguous.
inline at::Tensor check_dh(const at::Tensor& dh, int64_t T, int I, const char* op) {
  DTG_CHECK(dh.is_cuda() && dh.scalar_type() == at::kBFloat16, op, ": dh must be a bf16 GPU tensor");
  DTG_CHECK(dh.dim() == 2 && dh.size(0) == T && dh.size(1) == I, op, ": shape mismatch");
  return dh.contiguous();
}

template <class Act>
at::Tensor act_fwd(const at::Tensor& x, const char* op) {
  const int I = check_x<Act>(x, op);
  const int64_t T = x.size(0);
  const c10::DeviceGuard g(x.device());
  auto h = at::empty({T, I}, x.options());
  const int64_t n = T * (I / 8);
  if (n == 0) return h;
  act_fwd_kernel<Act><<<(n + 255) / 256, 256, 0, stream()>>>(bf16_ptr(x), x.stride(0), bf16_mut(h), T, I);
  DTG_LAUNCH_CHECK();
  return h;
}

template <class Act>
at::Tensor act_bwd(const at::Tensor& dh_, const at::Tensor& x, const char* op) {
  const int I = check_x<Act>(x, op);
  const int64_t T = x.size(0);
  const auto dh = check_dh(dh_, T, I, op);
  const c10::DeviceGuard g(x.device());
  auto dx = at::empty({T, Act::kIn * I}, x.options());
  const int64_t n = T * (I / 8);
  if (n == 0) return dx;
  act_bwd_kernel<Act><<<(n + 255) / 256, 256, 0, stream()>>>(bf16_ptr(dh), bf16_ptr(x), x.stride(0), bf16_mut(dx), T,
                                                             I);
  DTG_LAUNCH_CHECK();
  return dx;
}

template <class Act>
std::tuple<at::Tensor, at::Tensor, at::Tensor> act_bwd_t(const at::Tensor& dh_, const at::Tensor& x, const char* op) {
  const int I = check_x<Act>(x, op);
  const int64_t T = x.size(0);
  DTG_CHECK(T % 8 == 0, op, ": T must be a multiple of 8");
  const auto dh = check_dh(dh_, T, I, op);
  const c10::DeviceGuard g(x.device());
  auto dx = at::empty({T, Act::kIn * I}, x.options());
  auto dxT = at::empty({Act::kIn * I, T}, x.options());
  auto hT = at::empty({I, T}, x.options());
  if (T == 0 || I == 0) return {dx, dxT, hT};
  act_bwd_t_kernel<Act><<<tile_grid((T + kTT - 1) / kTT, (I + kTF - 1) / kTF), kThreads, 0, stream()>>>(
      bf16_ptr(dh), bf16_ptr(x), x.stride(0), bf16_mut(dx), bf16_mut(dxT), bf16_mut(hT), T, I);
  DTG_LAUNCH_CHECK();
  return {dx, dxT, hT};
}

}  // namespace mlp_act
}  // namespace dtg
