// SwiGLU on the fused gate|up projection output.
//
//   gu = x @ [W_gate; W_up]^T   ->  [T, 2I]  (gate = gu[:, :I], up = gu[:, I:])
//   h  = silu(gate) * up        ->  [T, I]
//
// One fused GEMM replaces the two HF Linear calls; the kernels (mlp_act.h) read gu once and write
// h once (forward) and read dh + gu once to write dgu (backward).  f32 math, one rounding.
#include "mlp_act.h"

namespace dtg {

using mlp_act::SwiGLU;

at::Tensor swiglu_fwd(const at::Tensor& gu) { return mlp_act::act_fwd<SwiGLU>(gu, "swiglu_fwd"); }
at::Tensor swiglu_bwd(const at::Tensor& dh, const at::Tensor& gu) {
  return mlp_act::act_bwd<SwiGLU>(dh, gu, "swiglu_bwd");
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> swiglu_bwd_t(const at::Tensor& dh, const at::Tensor& gu) {
  return mlp_act::act_bwd_t<SwiGLU>(dh, gu, "swiglu_bwd_t");
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) {
  m.impl("swiglu_fwd", &swiglu_fwd);
  m.impl("swiglu_bwd", &swiglu_bwd);
  m.impl("swiglu_bwd_t", &swiglu_bwd_t);
}

}  // namespace dtg
