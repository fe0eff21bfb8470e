// GELU-tanh ("gelu_new") of the GPT-2 MLP on the c_fc output (bias already added by the GEMM's
// epilogue), SURVEY K15.
//
//   gelu(x) = 0.5 x (1 + tanh(u)) = x * sigma(2u),   u = sqrt(2/pi) (x + 0.044715 x^3)
//   gelu'(x) = sigma + x sigma (1 - sigma) * 2u',    u' = sqrt(2/pi) (1 + 3 * 0.044715 x^2)
//
// The sigmoid form needs no tanhf and cannot produce inf * 0: exp(-2u) overflows to inf only
// where sigma = 1 / (1 + inf) = 0 exactly, and u' stays finite for every bf16 x that matters
// (|x| < 1e18).  f32 math, one rounding on store.  The kernels are those of mlp_act.h.
#include "mlp_act.h"

namespace dtg {

struct Gelu {
  static constexpr int kIn = 1;
  static constexpr float kC = 0.7978845608028654f;  // sqrt(2 / pi)
  static constexpr float kA = 0.044715f;

  static __device__ __forceinline__ float sigma2u(float x) {
    const float u = kC * (x + kA * x * x * x);
    return 1.f / (1.f + __expf(-2.f * u));
  }

  static __device__ __forceinline__ float fwd(const float (&x)[1]) { return x[0] * sigma2u(x[0]); }

  static __device__ __forceinline__ float grad(float x) {
    const float s = sigma2u(x);
    const float du2 = 2.f * kC * (1.f + 3.f * kA * x * x);
    return s + x * s * (1.f - s) * du2;
  }

  static __device__ __forceinline__ void bwd(const float (&x)[1], float d, float (&dx)[1], float& h) {
    dx[0] = d * grad(x[0]);
    h = fwd(x);
  }
};

at::Tensor gelu_fwd(const at::Tensor& x) { return mlp_act::act_fwd<Gelu>(x, "gelu_fwd"); }
at::Tensor gelu_bwd(const at::Tensor& dh, const at::Tensor& x) { return mlp_act::act_bwd<Gelu>(dh, x, "gelu_bwd"); }
std::tuple<at::Tensor, at::Tensor, at::Tensor> gelu_bwd_t(const at::Tensor& dh, const at::Tensor& x) {
  return mlp_act::act_bwd_t<Gelu>(dh, x, "gelu_bwd_t");
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) {
  m.impl("gelu_fwd", &gelu_fwd);
  m.impl("gelu_bwd", &gelu_bwd);
  m.impl("gelu_bwd_t", &gelu_bwd_t);
}

}  // namespace dtg
