// What the norm kernels (rmsnorm.hip, layernorm.hip, qk_norm.hip) share beyond common.h: the
// fixed-order column sum that finishes their weight gradients, the PER dispatch and the argument
// checks of their host wrappers.  The objects are linked without relocatable device code, so the
// kernel and its launcher are `static` (one copy per including file): host stubs with external
// linkage would collide at link time.
#pragma once

#include "common.h"
#include "norm_plan.h"

namespace dtg {
namespace norm {

// Column sums of the [gridDim.y, nrows, W] f32 partials -> bf16 [gridDim.y, W], fixed summation
// order (deterministic).  16 columns x 16 row groups per workgroup: W / 16 workgroups (256 at
// W = 4096, one per CU) each walking nrows / 16 rows -- the 32-column form had half the chip idle
// and twice the dependent-load depth.  Group g adds rows g, g + 16, ... in order; group 0 then adds
// the 16 group sums in order through LDS; one bf16 rounding at the end.
static __global__ __launch_bounds__(kThreads) void colsum_to_bf16_kernel(const float* __restrict__ part, int nrows,
                                                                         int W, uint16_t* __restrict__ out) {
  constexpr int G = kThreads / kColsumCols;
  __shared__ float red[G][kColsumCols + 1];
  const int lane = threadIdx.x % kColsumCols, grp = threadIdx.x / kColsumCols;
  const int c = blockIdx.x * kColsumCols + lane;
  part += (int64_t)blockIdx.y * nrows * W;
  float s = 0.f;
  if (c < W)
    for (int r = grp; r < nrows; r += G) s += part[(int64_t)r * W + c];
  red[grp][lane] = s;
  __syncthreads();
  if (grp == 0 && c < W) {
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < G; ++g) t += red[g][lane];
    out[(int64_t)blockIdx.y * W + c] = f2bf(t);
  }
}

static void colsum_to_bf16(const float* part, int n_mat, int nrows, int W, uint16_t* out) {
  colsum_to_bf16_kernel<<<dim3((W + kColsumCols - 1) / kColsumCols, n_mat), kThreads, 0, stream()>>>(part, nrows, W,
                                                                                                   out);
  DTG_LAUNCH_CHECK();
}

// Runs the statement with `constexpr int P` = per (1, 2, 4, 8); `op` names the operator in the error.
#define DTG_PER_DISPATCH(op, per, ...)                                 \
  switch (per) {                                                       \
    case 1: { constexpr int P = 1; __VA_ARGS__; break; }               \
    case 2: { constexpr int P = 2; __VA_ARGS__; break; }               \
    case 4: { constexpr int P = 4; __VA_ARGS__; break; }               \
    case 8: { constexpr int P = 8; __VA_ARGS__; break; }               \
    default: DTG_CHECK(false, op ": unsupported hidden size");         \
  }

inline void check_rows(const at::Tensor& t, const char* name) {
  DTG_CHECK_CUDA_BF16(t);
  DTG_CHECK(t.dim() == 2 && t.stride(1) == 1 && t.stride(0) % 8 == 0, name,
            " must be 2-D with unit inner stride and 16-byte aligned rows");
}

// A saved f32 statistic (mean, rstd) of `n` elements that a kernel reads by index.
inline void check_stat(const at::Tensor& t, int64_t n, const char* what) {
  DTG_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.numel() == n && t.is_contiguous(), what);
}

// The optional residual gradient as a contiguous [T, H] bf16 GPU tensor; undefined if there is none.
inline at::Tensor checked_dres(const c10::optional<at::Tensor>& dres_, int64_t T, int64_t H, const char* what) {
  if (!dres_.has_value() || !dres_->defined()) return {};
  auto dres = dres_->contiguous();
  DTG_CHECK_CUDA_BF16(dres);
  DTG_CHECK(dres.dim() == 2 && dres.size(0) == T && dres.size(1) == H, what);
  return dres;
}

}  // namespace norm
}  // namespace dtg
