// What the skinny GEMMs (skinny_gemm.hip, skinny_mfma.hip) share beyond common.h: the host checks on the
// operands, with the grid.  The store epilogue stays in each kernel: written as one inlined function it left
// the compiler a different pairing of the packed f32 operations throughout skinny_gemm_kernel's act = 1
// instantiations (other registers, other schedule), in every form of passing the sums and the scale that was
// tried.
#pragma once

#include "common.h"

namespace dtg {
namespace skinny {

struct Plan {
  int64_t M, N, K;
  const uint16_t* bias = nullptr;
  unsigned grid;
};

// What the operators share on the host: the checks on x, act, M, K, the weight matrix's layout and the bias, and
// the grid.  `x_bf16` = false: x is a matrix of another element type (FP8 codes), whose dtype the operator has checked.
// `w_layout` is the operator's own message for the layout of w, an [N, K / w_per_elem] matrix of
// elements that hold w_per_elem weights each; a workgroup owns cols_per_wg output columns.  `bias_msg`, where
// given, is the operator's one message for everything about the bias.  The operators check the weights' dtype
// before and the scales after.
inline Plan plan(const char* name, const char* w_layout, int max_m, int k_multiple, int w_per_elem,
                 int64_t cols_per_wg, const at::Tensor& x, const at::Tensor& w,
                 const c10::optional<at::Tensor>& bias, int64_t act, const char* bias_msg = nullptr,
                 bool x_bf16 = true) {
  Plan p;
  if (x_bf16) DTG_CHECK_CUDA_BF16(x);
  DTG_CHECK(act == 0 || act == 1, name, ": act must be 0 (none) or 1 (SwiGLU)");
  DTG_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.size(0) <= max_m, name, ": x must be [M, K] with 1 <= M <= ", max_m);
  p.M = x.size(0), p.K = x.size(1);
  DTG_CHECK(p.K % k_multiple == 0, name, ": K must be a multiple of ", k_multiple);
  DTG_CHECK(x.stride(1) == 1 && x.stride(0) % (16 / (int64_t)x.element_size()) == 0 &&
                reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
            name,
            ": x must have unit inner stride and 16-B aligned rows");
  DTG_CHECK(w.dim() == 2 && w.size(1) == p.K / w_per_elem && w.size(0) >= 1 && w.is_contiguous() &&
                w.device() == x.device() && reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
            name, w_layout);
  p.N = w.size(0);
  DTG_CHECK(act == 0 || p.N % 2 == 0, name, ": the SwiGLU epilogue needs an even N (gate rows, then up rows)");
  DTG_CHECK(p.N < (int64_t(1) << 32) && p.K < (int64_t(1) << 40), name, ": matrix too large");
  if (bias.has_value() && bias->defined()) {
    const bool layout =
        bias->dim() == 1 && bias->size(0) == p.N && bias->is_contiguous() && bias->device() == x.device();
    if (bias_msg != nullptr) {
      DTG_CHECK(bias->is_cuda() && bias->scalar_type() == at::kBFloat16 && layout, name, bias_msg);
    } else {
      DTG_CHECK_CUDA_BF16(*bias);
      DTG_CHECK(layout, name, ": bias must be a contiguous [N]");
    }
    p.bias = bf16_ptr(*bias);
  }
  const int64_t nwg = ((act ? p.N / 2 : p.N) + cols_per_wg - 1) / cols_per_wg;
  DTG_CHECK(nwg < (int64_t(1) << 31), name, ": too many workgroups");
  p.grid = (unsigned)nwg;
  return p;
}

}  // namespace skinny
}  // namespace dtg
