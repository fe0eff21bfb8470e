// Sum of squares of a flat gradient buffer (global-norm gradient clipping, grad-norm logging).
//
// A purely streaming read: 16-byte vectors per lane, U of them in flight per lane per iteration
// (each one grid-stride away from the last, as in adamw_kernel), f32 accumulation.  The result is
// bitwise reproducible run to run: no floating-point atomics, two plain launches --
//   1. sumsq_partial_kernel: grid-stride over the buffer, one f32 partial per workgroup written
//      to a workspace (lane sums -> wave butterfly -> the waves' sums in wave order);
//   2. sumsq_final_kernel: ONE workgroup sums the partials in a fixed order (lane t takes
//      partials t, t + 256, ... in that order, then the same block sum) and adds to acc[slot].
// The launch shape depends only on n and the pointer's alignment, so the summation order does too.
//
// A buffer whose data pointer is not 16-byte aligned (a slice starting at an odd element) or whose
// length is not a multiple of the vector is split on the host into a scalar head (up to the first
// 16-byte boundary), the vector body and a scalar tail; head and tail are each shorter than one
// vector and are read by the first lanes of workgroup 0.
#include "common.h"

namespace dtg {

constexpr int kSqThreads = 256;
constexpr int kSqVec = 8;          // elements per lane per vector: 16 B of bf16, 32 B of f32
constexpr int kSqMaxBlocks = 2048;  // 8 workgroups of 256 per CU on 256 CUs: every wave slot filled

// g: `head` scalar elements, then `nbody` (a multiple of 8) elements from a 16-byte boundary,
// then `tail` scalar elements; head, tail < 8.
template <typename T, int U>
__global__ __launch_bounds__(kSqThreads) void sumsq_partial_kernel(const T* __restrict__ g, int head, int64_t nbody,
                                                                   int tail, float* __restrict__ partials) {
  __shared__ float scratch[kSqThreads / kWave];
  const T* body = g + head;
  float s[U];
#pragma unroll
  for (int u = 0; u < U; ++u) s[u] = 0.f;
  const int64_t stride = (int64_t)gridDim.x * kSqThreads * kSqVec;
  int64_t i = ((int64_t)blockIdx.x * kSqThreads + threadIdx.x) * kSqVec;
  for (; i + (U - 1) * stride < nbody; i += U * stride) {
    float x[U][kSqVec];
#pragma unroll
    for (int u = 0; u < U; ++u) ld8(body + i + u * stride, x[u]);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < kSqVec; ++j) s[u] += x[u][j] * x[u][j];
  }
  for (; i < nbody; i += stride) {
    float x[kSqVec];
    ld8(body + i, x);
#pragma unroll
    for (int j = 0; j < kSqVec; ++j) s[0] += x[j] * x[j];
  }
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    if (t < head) {
      const float x = ld(g, t);
      s[0] += x * x;
    } else if (t >= kWave && t - kWave < tail) {
      const float x = ld(body, nbody + (t - kWave));
      s[0] += x * x;
    }
  }
  float r = s[0];
#pragma unroll
  for (int u = 1; u < U; ++u) r += s[u];
  r = block_sum(r, scratch);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

__global__ __launch_bounds__(kSqThreads) void sumsq_final_kernel(const float* __restrict__ partials, int np,
                                                                 float* __restrict__ acc) {
  __shared__ float scratch[kSqThreads / kWave];
  float r = 0.f;
  for (int i = threadIdx.x; i < np; i += kSqThreads) r += partials[i];
  r = block_sum(r, scratch);
  if (threadIdx.x == 0) acc[0] += r;
}

void grad_sumsq_(const at::Tensor& g, const at::Tensor& acc, int64_t slot) {
  DTG_CHECK(g.is_cuda() && g.dim() == 1 && g.is_contiguous(), "grad_sumsq_: g must be a contiguous 1-D GPU tensor");
  const bool gb = g.scalar_type() == at::kBFloat16;
  DTG_CHECK(gb || g.scalar_type() == at::kFloat, "grad_sumsq_: g must be bf16 or f32");
  DTG_CHECK(acc.is_cuda() && acc.scalar_type() == at::kFloat && acc.dim() == 1 && acc.is_contiguous() &&
                acc.device() == g.device(), "grad_sumsq_: acc must be a contiguous f32 vector on g's device");
  DTG_CHECK(slot >= 0 && slot < acc.numel(), "grad_sumsq_: slot out of range");
  const int64_t n = g.numel();
  if (n == 0) return;
  const c10::DeviceGuard gd(g.device());
  const int64_t esz = gb ? 2 : 4;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(g.data_ptr());
  DTG_CHECK(addr % esz == 0, "grad_sumsq_: g is not aligned to its element size");
  const int64_t head = std::min<int64_t>(n, (int64_t)((16 - (addr & 15)) & 15) / esz);  // < 8
  const int64_t nbody = (n - head) / kSqVec * kSqVec;
  const int64_t tail = n - head - nbody;  // < 8
  const int64_t want = (nbody + kSqThreads * kSqVec - 1) / (kSqThreads * kSqVec);
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(want, kSqMaxBlocks));
  // workspace from torch's caching allocator: stream-ordered reuse, and a capture-pool block
  // under HIP-graph capture
  at::Tensor ws = at::empty({blocks}, acc.options());
  float* wp = ws.data_ptr<float>();
  if (gb)
    sumsq_partial_kernel<uint16_t, 4><<<blocks, kSqThreads, 0, stream()>>>(bf16_ptr(g), (int)head, nbody, (int)tail, wp);
  else
    sumsq_partial_kernel<float, 4><<<blocks, kSqThreads, 0, stream()>>>(g.data_ptr<float>(), (int)head, nbody,
                                                                        (int)tail, wp);
  DTG_LAUNCH_CHECK();
  sumsq_final_kernel<<<1, kSqThreads, 0, stream()>>>(wp, blocks, acc.data_ptr<float>() + slot);
  DTG_LAUNCH_CHECK();
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) { m.impl("grad_sumsq_", &grad_sumsq_); }

}  // namespace dtg
