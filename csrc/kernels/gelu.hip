// GELU-tanh ("gelu_new") of the GPT-2 MLP on the c_fc output (bias already added by the GEMM's
// epilogue), SURVEY K15.
//
//   gelu(x) = 0.5 x (1 + tanh(u)) = x * sigma(2u),   u = sqrt(2/pi) (x + 0.044715 x^3)
//   gelu'(x) = sigma + x sigma (1 - sigma) * 2u',    u' = sqrt(2/pi) (1 + 3 * 0.044715 x^2)
//
// The sigmoid form needs no tanhf and cannot produce inf * 0: exp(-2u) overflows to inf only
// where sigma = 1 / (1 + inf) = 0 exactly, and u' stays finite for every bf16 x that matters
// (|x| < 1e18).  f32 math, one rounding on store.
#include "common.h"

namespace dtg {
namespace gelu {

constexpr float kC = 0.7978845608028654f;  // sqrt(2 / pi)
constexpr float kA = 0.044715f;

__device__ __forceinline__ float sigma2u(float x) {
  const float u = kC * (x + kA * x * x * x);
  return 1.f / (1.f + __expf(-2.f * u));
}

__device__ __forceinline__ float fwd(float x) { return x * sigma2u(x); }

__device__ __forceinline__ float grad(float x) {
  const float s = sigma2u(x);
  const float du2 = 2.f * kC * (1.f + 3.f * kA * x * x);
  return s + x * s * (1.f - s) * du2;
}

__global__ void gelu_fwd_kernel(const uint16_t* __restrict__ x, int64_t x_stride, uint16_t* __restrict__ h,
                                int64_t T, int I) {
  const int chunks = I >> 3;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= T * chunks) return;
  const int64_t t = gid / chunks;
  const int c = (gid % chunks) * 8;
  float v[8], o[8];
  load8(x + t * x_stride + c, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = fwd(v[j]);
  store8(h + t * I + c, o);
}

__global__ void gelu_bwd_kernel(const uint16_t* __restrict__ dh, const uint16_t* __restrict__ x, int64_t x_stride,
                                uint16_t* __restrict__ dx, int64_t T, int I) {
  const int chunks = I >> 3;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= T * chunks) return;
  const int64_t t = gid / chunks;
  const int c = (gid % chunks) * 8;
  float v[8], d[8], o[8];
  load8(x + t * x_stride + c, v);
  load8(dh + t * I + c, d);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = d[j] * grad(v[j]);
  store8(dx + t * I + c, o);
}

// Backward that also emits the operands of the MLP's weight-gradient GEMMs in K-contiguous
// (token-minor) layout, so hipBLASLt runs them as "TN" without separate transpose passes:
//   dx  [T, I]   (row-major, for dX = dx @ W_fc)
//   dxT [I, T]   (for dW_fc = dxT @ X)
//   hT  [I, T]   (h = gelu(x) recomputed, for dW_proj = dY^T @ h)
// The tile scheme of swiglu_bwd_t_kernel: one workgroup owns a 64-token x 128-feature tile,
// 16-byte row loads of x and dh, the two transposed tiles staged through LDS (pitch TF + 2
// halfwords) and stored as 16-byte columns.
constexpr int kTT = 64, kTF = 128;

template <int TT, int TF>
__global__ __launch_bounds__(256) void gelu_bwd_t_kernel(const uint16_t* __restrict__ dh,
                                                         const uint16_t* __restrict__ x, int64_t x_stride,
                                                         uint16_t* __restrict__ dx, uint16_t* __restrict__ dxT,
                                                         uint16_t* __restrict__ hT, int64_t T, int I) {
  static_assert(TT == 64 && TF == 128, "tile");
  constexpr int kPitch = TF + 2;
  constexpr int kVF = TF / 8;              // 16-byte vectors per token row of the tile
  constexpr int kRowsPerPass = 256 / kVF;  // token rows per phase-1 pass
  constexpr int kVT = TT / 8;              // 16-byte vectors per transposed row segment
  constexpr int kOutPerPass = 256 / kVT;   // feature rows per phase-2 pass
  __shared__ uint16_t s_dx[TT * kPitch];
  __shared__ uint16_t s_h[TT * kPitch];
  const int64_t t0 = (int64_t)blockIdx.y * TT;
  const int c0 = (int)blockIdx.x * TF;
  const int tid = threadIdx.x;
  constexpr int kNP = TT / kRowsPerPass;
  u16x8 rx[kNP], rd[kNP];
#pragma unroll
  for (int i = 0; i < kNP; ++i) {
    const int64_t t = t0 + tid / kVF + kRowsPerPass * i;
    const int c = c0 + (tid % kVF) * 8;
    if (t < T && c < I) {
      rx[i] = *reinterpret_cast<const u16x8*>(x + t * x_stride + c);
      rd[i] = *reinterpret_cast<const u16x8*>(dh + t * I + c);
    }
  }
#pragma unroll
  for (int i = 0; i < kNP; ++i) {
    const int lt = tid / kVF + kRowsPerPass * i;
    const int lc = (tid % kVF) * 8;
    const int64_t t = t0 + lt;
    const int c = c0 + lc;
    u16x8 vdx = {0, 0, 0, 0, 0, 0, 0, 0}, vh = vdx;
    if (t < T && c < I) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = bf2f(rx[i][j]);
        vdx[j] = f2bf(bf2f(rd[i][j]) * grad(v));
        vh[j] = f2bf(fwd(v));
      }
      *reinterpret_cast<u16x8*>(dx + t * I + c) = vdx;
    }
    uint32_t* a = reinterpret_cast<uint32_t*>(s_dx + lt * kPitch + lc);
    uint32_t* b = reinterpret_cast<uint32_t*>(s_h + lt * kPitch + lc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = (uint32_t)vdx[2 * j] | ((uint32_t)vdx[2 * j + 1] << 16);
      b[j] = (uint32_t)vh[2 * j] | ((uint32_t)vh[2 * j + 1] << 16);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < TF / kOutPerPass; ++i) {
    const int oc = tid / kVT + kOutPerPass * i;  // feature within the tile -> output row
    const int ot = (tid % kVT) * 8;              // first token of this 8-token vector
    const int c = c0 + oc;
    const int64_t t = t0 + ot;
    if (c >= I || t >= T) continue;
    u16x8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = s_dx[(ot + j) * kPitch + oc];
      b[j] = s_h[(ot + j) * kPitch + oc];
    }
    *reinterpret_cast<u16x8*>(dxT + (int64_t)c * T + t) = a;
    *reinterpret_cast<u16x8*>(hT + (int64_t)c * T + t) = b;
  }
}

static void check_x(const at::Tensor& x, const char* op) {
  DTG_CHECK_CUDA_BF16(x);
  DTG_CHECK(x.dim() == 2 && x.stride(1) == 1 && x.stride(0) % 8 == 0 && x.size(1) % 8 == 0, op,
            ": x must be [T, I] with unit inner stride, 16-byte aligned rows and I % 8 == 0");
}

}  // namespace gelu

at::Tensor gelu_fwd(const at::Tensor& x) {
  gelu::check_x(x, "gelu_fwd");
  const int64_t T = x.size(0);
  const int I = x.size(1);
  const c10::DeviceGuard g(x.device());
  auto h = at::empty({T, I}, x.options());
  const int64_t n = T * (I / 8);
  if (n == 0) return h;
  gelu::gelu_fwd_kernel<<<(n + 255) / 256, 256, 0, stream()>>>(bf16_ptr(x), x.stride(0), bf16_mut(h), T, I);
  DTG_LAUNCH_CHECK();
  return h;
}

at::Tensor gelu_bwd(const at::Tensor& dh_, const at::Tensor& x) {
  auto dh = dh_.contiguous();
  gelu::check_x(x, "gelu_bwd");
  DTG_CHECK_CUDA_BF16(dh);
  const int64_t T = x.size(0);
  const int I = x.size(1);
  DTG_CHECK(dh.dim() == 2 && dh.size(0) == T && dh.size(1) == I, "gelu_bwd: shape mismatch");
  const c10::DeviceGuard g(x.device());
  auto dx = at::empty({T, I}, x.options());
  const int64_t n = T * (I / 8);
  if (n == 0) return dx;
  gelu::gelu_bwd_kernel<<<(n + 255) / 256, 256, 0, stream()>>>(bf16_ptr(dh), bf16_ptr(x), x.stride(0), bf16_mut(dx),
                                                               T, I);
  DTG_LAUNCH_CHECK();
  return dx;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> gelu_bwd_t(const at::Tensor& dh_, const at::Tensor& x) {
  auto dh = dh_.contiguous();
  gelu::check_x(x, "gelu_bwd_t");
  DTG_CHECK_CUDA_BF16(dh);
  const int64_t T = x.size(0);
  const int I = x.size(1);
  DTG_CHECK(T % 8 == 0, "gelu_bwd_t: T must be a multiple of 8");
  DTG_CHECK(dh.dim() == 2 && dh.size(0) == T && dh.size(1) == I, "gelu_bwd_t: shape mismatch");
  const c10::DeviceGuard g(x.device());
  auto dx = at::empty({T, I}, x.options());
  auto dxT = at::empty({I, T}, x.options());
  auto hT = at::empty({I, T}, x.options());
  if (T == 0 || I == 0) return {dx, dxT, hT};
  gelu::gelu_bwd_t_kernel<gelu::kTT, gelu::kTF>
      <<<tile_grid((T + gelu::kTT - 1) / gelu::kTT, (I + gelu::kTF - 1) / gelu::kTF), 256, 0, stream()>>>(
          bf16_ptr(dh), bf16_ptr(x), x.stride(0), bf16_mut(dx), bf16_mut(dxT), bf16_mut(hT), T, I);
  DTG_LAUNCH_CHECK();
  return {dx, dxT, hT};
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) {
  m.impl("gelu_fwd", &gelu_fwd);
  m.impl("gelu_bwd", &gelu_bwd);
  m.impl("gelu_bwd_t", &gelu_bwd_t);
}

}  // namespace dtg
