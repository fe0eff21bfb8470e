// SwiGLU on the fused gate|up projection output.
//
//   gu = x @ [W_gate; W_up]^T   ->  [T, 2I]  (gate = gu[:, :I], up = gu[:, I:])
//   h  = silu(gate) * up        ->  [T, I]
//
// One fused GEMM replaces the two HF Linear calls; the kernels (mlp_act.h) read gu once and write
// h once (forward) and read dh + gu once to write dgu (backward).  f32 math, one rounding.
#include "mlp_act.h"

namespace dtg {

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
