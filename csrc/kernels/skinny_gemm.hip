// Skinny GEMM for the decode step's projections: y[M, N] = x[M, K] @ float(w[N, K])^T (* scale[N]) (+ bias),
// 1 <= M <= 16, x, bias and y bf16, f32 accumulation, one rounding.  At these M the product is a
// weight-streaming GEMV: every weight is read once and used M times, so the kernel is shaped by the guide's
// "GEMV / M <= 16 decode weights" row -- weights straight to VGPRs in 16-B pieces, several loads in flight
// per lane, no LDS, no barrier, non-temporal loads (the stream is read once; x, which every wave re-reads,
// keeps the default policy and stays in L1 / L2).  One kernel template serves every weight format; a format
// (below) says how 16 B of weights become floats and nothing else.
//
// Mapping: a wave owns kRows = 4 weight rows (output columns n0 .. n0 + 3; with the SwiGLU epilogue the gate
// rows n0, n0 + 1 and the up rows I + n0, I + n0 + 1), a workgroup 4 waves.  Lane l walks the K dimension in
// chunks of one 16-B weight load, l, l + 64, l + 128, ...; a chunk is widened and consumed in pieces of 8
// elements: one 16-B x load per row of x meets all four weight rows (M * 4 * 8 FMAs for (M + 4) * 8
// conversions), so 4 x 8 widened weights are held at once.  The loop is unrolled unroll(M) passes deep:
// unroll(M) * 4 weight loads are issued before the first is consumed.
//
// Summation order of one output (m, n): the lane's chunks in ascending order, one fmaf per element in element
// order, then the xor butterfly over the 64 lanes (offsets 32, 16, ..., 1).  It depends on neither M nor the
// other rows nor on which slot of the wave the weight row sits in: M is a template parameter for unrolling
// only, so row m of a batched call equals the single-row call bit for bit.  No atomics, no split-K across
// workgroups.  Lanes past K load nothing and add nothing; weight rows past N are clamped to row N - 1
// (loaded, never stored).
//
// Epilogue, in this order: the sum times the row's scale (scaled formats), plus the bias, one rounding to
// bf16.  act = 1 (SwiGLU): the gate and the up sums are each scaled, biased and rounded exactly as the plain
// form stores them, widened again and passed through mlp_act::SwiGLU::fwd, the functor of swiglu_fwd: the
// result equals swiglu_fwd of the plain product bit for bit, without the [M, 2I] round trip and the second
// launch.
//
// Bf16Weights (skinny_linear): 8 weights per load, widened by a shift.
//
// E4m3Weights (skinny_linear_fp8): OCP e4m3fn (the format gfx950 converts in hardware, not MI300's fnuz), one
// byte per weight, 16 per load, widened two dwords per piece through v_cvt_pk_f32_fp8; scale f32, one per
// weight row.  At M = 1 the bf16 form streams its weights at the copy rate, so the only lever left is the
// number of bytes: this form reads half of them.  bf16 x e4m3 products are exact in f32 (8 + 4 significand
// bits).  More than 8 rows of x run one pass deep.
#include "mlp_act.h"

namespace dtg {

namespace {

constexpr int kSkinnyMaxM = 16;
constexpr int kSkinnyThreads = 256;
constexpr int kSkinnyWaves = kSkinnyThreads / kWave;
constexpr int kRows = 4;  // weight rows per wave

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct NoScale {};  // an empty kernel argument: the unscaled kernels keep their argument layout

struct Bf16Weights {
  using Elem = uint16_t;
  using Vec = u16x8;
  using Scale = NoScale;
  static constexpr int kChunk = 8;  // weights per 16-B load
  static constexpr int unroll(int M) { return M <= 4 ? 4 : 2; }
  static __device__ __forceinline__ int64_t chunks(int64_t K) { return K >> 3; }
  static __device__ __forceinline__ void widen(const Vec& v, int, float* out) { widen8(v, out); }
};

struct E4m3Weights {
  using Elem = uint8_t;
  using Vec = u32x4;
  using Scale = const float* __restrict__;
  static constexpr int kChunk = 16;
  static constexpr int unroll(int M) { return M <= 4 ? 4 : (M <= 8 ? 2 : 1); }
  static __device__ __forceinline__ int64_t chunks(int64_t K) { return K / kChunk; }
  // Elements 8 h .. 8 h + 7 of the chunk: four e4m3 bytes of a dword (memory order = ascending byte) through
  // v_cvt_pk_f32_fp8, low then high half.
  static __device__ __forceinline__ void widen(const Vec& v, int h, float* out) {
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[2 * h + d], false);
      const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[2 * h + d], true);
      out[4 * d] = lo[0];
      out[4 * d + 1] = lo[1];
      out[4 * d + 2] = hi[0];
      out[4 * d + 3] = hi[1];
    }
  }
};

template <class Fmt, int M, int ACT>
__global__ __launch_bounds__(kSkinnyThreads) void skinny_gemm_kernel(
    const uint16_t* __restrict__ x, int64_t x_stride, const typename Fmt::Elem* __restrict__ w,
    typename Fmt::Scale scale, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int64_t N,
    int64_t K) {
  using Vec = typename Fmt::Vec;
  constexpr int kChunk = Fmt::kChunk;
  constexpr int kUnroll = Fmt::unroll(M);
  constexpr int kCols = ACT ? kRows / 2 : kRows;  // output columns per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n_out = ACT ? N / 2 : N;
  const int64_t n0 = ((int64_t)blockIdx.x * kSkinnyWaves + wave) * kCols;
  if (n0 >= n_out) return;  // wave-uniform; the kernel has no barrier

  int64_t wrow[kRows];  // weight row of slot r, clamped into the matrix
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int64_t c = n0 + (ACT ? r % kCols : r);
    const int64_t cc = c < n_out ? c : n_out - 1;
    wrow[r] = ACT && r >= kCols ? n_out + cc : cc;
  }

  float acc[M][kRows];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[m][r] = 0.f;

  const int64_t chunks = Fmt::chunks(K);
  for (int64_t c0 = 0; c0 < chunks; c0 += (int64_t)kWave * kUnroll) {
    Vec wv[kUnroll][kRows];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t c = c0 + u * kWave + lane;
      if (c < chunks) {
#pragma unroll
        for (int r = 0; r < kRows; ++r)
          wv[u][r] = __builtin_nontemporal_load(reinterpret_cast<const Vec*>(w + wrow[r] * K + c * kChunk));
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t c = c0 + u * kWave + lane;
      if (c < chunks) {
#pragma unroll
        for (int h = 0; h < kChunk / 8; ++h) {  // elements 8 h .. 8 h + 7 of the chunk
          float wf[kRows][8];
#pragma unroll
          for (int r = 0; r < kRows; ++r) Fmt::widen(wv[u][r], h, wf[r]);
#pragma unroll
          for (int m = 0; m < M; ++m) {
            float xf[8];
            load8(x + m * x_stride + c * kChunk + h * 8, xf);
#pragma unroll
            for (int r = 0; r < kRows; ++r)
#pragma unroll
              for (int j = 0; j < 8; ++j) acc[m][r] = __builtin_fmaf(xf[j], wf[r][j], acc[m][r]);
          }
        }
      }
    }
  }

#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[m][r] = wave_sum(acc[m][r]);

  // lane m * kCols + c stores output (m, n0 + c): one store per lane
  float a = 0.f, b = 0.f;
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int c = 0; c < kCols; ++c)
      if (lane == m * kCols + c) {
        a = acc[m][c];
        if (ACT) b = acc[m][kCols + c];
      }
  if (lane >= M * kCols) return;
  const int m = lane / kCols, c = lane % kCols;
  const int64_t n = n0 + c;
  if (n >= n_out) return;
  if constexpr (!std::is_same<typename Fmt::Scale, NoScale>::value) {
    a *= scale[n];
    if (ACT) b *= scale[n_out + n];
  }
  if (bias != nullptr) {
    a += bf2f(bias[n]);
    if (ACT) b += bf2f(bias[n_out + n]);
  }
  if (ACT) {
    const float in[2] = {bf2f(f2bf(a)), bf2f(f2bf(b))};
    y[m * n_out + n] = f2bf(mlp_act::SwiGLU::fwd(in));
  } else {
    y[m * n_out + n] = f2bf(a);
  }
}

// What the operators share on the host: the checks on x, act, M, K, the weight matrix's layout (`w_layout` is
// the operator's own message for it) and the bias, and the grid.  The operators check the weights' dtype
// before and the scale after.
struct SkinnyPlan {
  int64_t M, N, K;
  const uint16_t* bias = nullptr;
  unsigned grid;
};

template <class Fmt>
SkinnyPlan skinny_plan(const char* name, const char* w_layout, const at::Tensor& x, const at::Tensor& w,
                       const c10::optional<at::Tensor>& bias, int64_t act) {
  SkinnyPlan p;
  DTG_CHECK_CUDA_BF16(x);
  DTG_CHECK(act == 0 || act == 1, name, ": act must be 0 (none) or 1 (SwiGLU)");
  DTG_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.size(0) <= kSkinnyMaxM, name, ": x must be [M, K] with 1 <= M <= ",
            kSkinnyMaxM);
  p.M = x.size(0), p.K = x.size(1);
  DTG_CHECK(p.K % Fmt::kChunk == 0, name, ": K must be a multiple of ", Fmt::kChunk);
  DTG_CHECK(x.stride(1) == 1 && x.stride(0) % 8 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, name,
            ": x must have unit inner stride and 16-B aligned rows");
  DTG_CHECK(w.dim() == 2 && w.size(1) == p.K && w.size(0) >= 1 && w.is_contiguous() && w.device() == x.device() &&
                reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
            name, w_layout);
  p.N = w.size(0);
  DTG_CHECK(act == 0 || p.N % 2 == 0, name, ": the SwiGLU epilogue needs an even N (gate rows, then up rows)");
  DTG_CHECK(p.N < (int64_t(1) << 32) && p.K < (int64_t(1) << 40), name, ": matrix too large");
  if (bias.has_value() && bias->defined()) {
    DTG_CHECK_CUDA_BF16(*bias);
    DTG_CHECK(bias->dim() == 1 && bias->size(0) == p.N && bias->is_contiguous() && bias->device() == x.device(), name,
              ": bias must be a contiguous [N]");
    p.bias = bf16_ptr(*bias);
  }
  const int64_t cols_per_wg = (int64_t)kSkinnyWaves * (act ? kRows / 2 : kRows);
  const int64_t nwg = ((act ? p.N / 2 : p.N) + cols_per_wg - 1) / cols_per_wg;
  DTG_CHECK(nwg < (int64_t(1) << 31), name, ": too many workgroups");
  p.grid = (unsigned)nwg;
  return p;
}

// Launches the instantiation for p.M rows of x: M counts down from the largest.
template <class Fmt, int ACT, int M = kSkinnyMaxM>
void skinny_launch(const SkinnyPlan& p, const at::Tensor& x, const at::Tensor& w, typename Fmt::Scale scale,
                   at::Tensor& y) {
  if constexpr (M >= 1) {
    if (p.M != M) return skinny_launch<Fmt, ACT, M - 1>(p, x, w, scale, y);
    skinny_gemm_kernel<Fmt, M, ACT><<<p.grid, kSkinnyThreads, 0, stream()>>>(
        bf16_ptr(x), x.stride(0), static_cast<const typename Fmt::Elem*>(w.data_ptr()), scale, p.bias, bf16_mut(y),
        p.N, p.K);
  }
}

template <class Fmt>
at::Tensor skinny_run(const SkinnyPlan& p, const at::Tensor& x, const at::Tensor& w, typename Fmt::Scale scale,
                      int64_t act) {
  const c10::DeviceGuard g(x.device());
  auto y = at::empty({p.M, act ? p.N / 2 : p.N}, x.options());
  if (act)
    skinny_launch<Fmt, 1>(p, x, w, scale, y);
  else
    skinny_launch<Fmt, 0>(p, x, w, scale, y);
  DTG_LAUNCH_CHECK();
  return y;
}

}  // namespace

at::Tensor skinny_linear(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias,
                         int64_t act) {
  DTG_CHECK_CUDA_BF16(w);
  const auto p = skinny_plan<Bf16Weights>("skinny_linear", ": w must be a contiguous [N, K] on x's device", x, w,
                                          bias, act);
  return skinny_run<Bf16Weights>(p, x, w, NoScale{}, act);
}

at::Tensor skinny_linear_fp8(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& scale,
                             const c10::optional<at::Tensor>& bias, int64_t act) {
  const char* name = "skinny_linear_fp8";
  DTG_CHECK(wq.is_cuda() && wq.scalar_type() == at::kFloat8_e4m3fn, name, ": wq must be a float8_e4m3fn GPU tensor");
  const auto p = skinny_plan<E4m3Weights>(name, ": wq must be a contiguous 16-B aligned [N, K] on x's device", x, wq,
                                          bias, act);
  DTG_CHECK(scale.is_cuda() && scale.scalar_type() == at::kFloat && scale.dim() == 1 && scale.size(0) == p.N &&
                scale.is_contiguous() && scale.device() == x.device(),
            name, ": scale must be a contiguous f32 [N] on x's device");
  return skinny_run<E4m3Weights>(p, x, wq, scale.data_ptr<float>(), act);
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) {
  m.impl("skinny_linear", &skinny_linear);
  m.impl("skinny_linear_fp8", &skinny_linear_fp8);
}

}  // namespace dtg
