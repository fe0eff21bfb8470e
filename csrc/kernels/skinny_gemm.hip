// Skinny GEMM for the decode step's projections: y[M, N] = x[M, K] @ w[N, K]^T (+ bias), 1 <= M <= 16,
// bf16 in and out, f32 accumulation, one rounding.  At these M the product is a weight-streaming GEMV:
// every weight is read once and used M times, so the kernel is shaped by the guide's "GEMV / M <= 16
// decode weights" row -- weights straight to VGPRs in 16-B pieces, several loads in flight per lane,
// no LDS round trip, non-temporal loads (the stream is read once; x, which every wave re-reads, keeps
// the default policy and stays in L1 / L2).
//
// Mapping: a wave owns kRows = 4 weight rows (output columns n0 .. n0 + 3; with the SwiGLU epilogue
// the gate rows n0, n0 + 1 and the up rows I + n0, I + n0 + 1), a workgroup 4 waves.  Lane l walks
// the K dimension in 8-element chunks l, l + 64, l + 128, ...; an x chunk is loaded and widened
// once and meets all four weight rows (M * 4 * 8 FMAs for (M + 4) * 8 conversions).  The loop is
// unrolled kUnroll passes deep: kUnroll * 4 weight loads are issued before the first is consumed.
//
// Summation order of one output (m, n): the lane's chunks in ascending order, eight fmaf per chunk in
// element order, then the xor butterfly over the 64 lanes (offsets 32, 16, ..., 1).  It depends on
// neither M nor the other rows nor on which slot of the wave the weight row sits in: M is a template
// parameter for unrolling only, so row m of a batched call equals the single-row call bit for bit.
// No atomics, no split-K across workgroups.  Lanes past K load nothing and add nothing; weight rows
// past N are clamped to row N - 1 (loaded, never stored).
//
// act = 1 (SwiGLU): the gate and the up sums are each rounded to bf16 (+ bias first) exactly as the
// plain form stores them, widened again and passed through mlp_act::SwiGLU::fwd, the functor of
// swiglu_fwd: the result equals swiglu_fwd(skinny_linear(x, w)) bit for bit, without the [M, 2I]
// round trip and the second launch.
#include "mlp_act.h"

namespace dtg {

namespace {

constexpr int kSkinnyMaxM = 16;
constexpr int kSkinnyThreads = 256;
constexpr int kSkinnyWaves = kSkinnyThreads / kWave;
constexpr int kRows = 4;  // weight rows per wave

template <int M, int ACT>
__global__ __launch_bounds__(kSkinnyThreads) void skinny_gemm_kernel(
    const uint16_t* __restrict__ x, int64_t x_stride, const uint16_t* __restrict__ w,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int64_t N, int64_t K) {
  constexpr int kUnroll = M <= 4 ? 4 : 2;
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

  const int64_t chunks = K >> 3;
  for (int64_t c0 = 0; c0 < chunks; c0 += (int64_t)kWave * kUnroll) {
    u16x8 wv[kUnroll][kRows];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t c = c0 + u * kWave + lane;
      if (c < chunks) {
#pragma unroll
        for (int r = 0; r < kRows; ++r)
          wv[u][r] = __builtin_nontemporal_load(reinterpret_cast<const u16x8*>(w + wrow[r] * K + c * 8));
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t c = c0 + u * kWave + lane;
      if (c < chunks) {
        float wf[kRows][8];
#pragma unroll
        for (int r = 0; r < kRows; ++r)
#pragma unroll
          for (int j = 0; j < 8; ++j) wf[r][j] = bf2f(wv[u][r][j]);
#pragma unroll
        for (int m = 0; m < M; ++m) {
          float xf[8];
          load8(x + m * x_stride + c * 8, xf);
#pragma unroll
          for (int r = 0; r < kRows; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[m][r] = __builtin_fmaf(xf[j], wf[r][j], acc[m][r]);
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

template <int ACT>
void skinny_launch(int64_t M, unsigned grid, const at::Tensor& x, const at::Tensor& w, const uint16_t* bias,
                   at::Tensor& y, int64_t N, int64_t K) {
#define DTG_SKINNY_CASE(M_)                                                                                  \
  case M_:                                                                                                   \
    skinny_gemm_kernel<M_, ACT><<<grid, kSkinnyThreads, 0, stream()>>>(bf16_ptr(x), x.stride(0), bf16_ptr(w), \
                                                                        bias, bf16_mut(y), N, K);             \
    break;
  switch (M) {
    DTG_SKINNY_CASE(1) DTG_SKINNY_CASE(2) DTG_SKINNY_CASE(3) DTG_SKINNY_CASE(4)
    DTG_SKINNY_CASE(5) DTG_SKINNY_CASE(6) DTG_SKINNY_CASE(7) DTG_SKINNY_CASE(8)
    DTG_SKINNY_CASE(9) DTG_SKINNY_CASE(10) DTG_SKINNY_CASE(11) DTG_SKINNY_CASE(12)
    DTG_SKINNY_CASE(13) DTG_SKINNY_CASE(14) DTG_SKINNY_CASE(15) DTG_SKINNY_CASE(16)
    default: DTG_CHECK(false, "skinny_linear: unreachable M");
  }
#undef DTG_SKINNY_CASE
}

}  // namespace

at::Tensor skinny_linear(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias,
                         int64_t act) {
  const char* name = "skinny_linear";
  DTG_CHECK_CUDA_BF16(x);
  DTG_CHECK_CUDA_BF16(w);
  DTG_CHECK(act == 0 || act == 1, name, ": act must be 0 (none) or 1 (SwiGLU)");
  DTG_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.size(0) <= kSkinnyMaxM, name, ": x must be [M, K] with 1 <= M <= ",
            kSkinnyMaxM);
  const int64_t M = x.size(0), K = x.size(1);
  DTG_CHECK(K % 8 == 0, name, ": K must be a multiple of 8");
  DTG_CHECK(x.stride(1) == 1 && x.stride(0) % 8 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, name,
            ": x must have unit inner stride and 16-B aligned rows");
  DTG_CHECK(w.dim() == 2 && w.size(1) == K && w.size(0) >= 1 && w.is_contiguous() && w.device() == x.device() &&
                reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
            name, ": w must be a contiguous [N, K] on x's device");
  const int64_t N = w.size(0);
  DTG_CHECK(act == 0 || N % 2 == 0, name, ": the SwiGLU epilogue needs an even N (gate rows, then up rows)");
  DTG_CHECK(N < (int64_t(1) << 32) && K < (int64_t(1) << 40), name, ": matrix too large");
  const uint16_t* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    DTG_CHECK_CUDA_BF16(*bias);
    DTG_CHECK(bias->dim() == 1 && bias->size(0) == N && bias->is_contiguous() && bias->device() == x.device(), name,
              ": bias must be a contiguous [N]");
    bp = bf16_ptr(*bias);
  }
  const c10::DeviceGuard g(x.device());
  const int64_t n_out = act ? N / 2 : N;
  auto y = at::empty({M, n_out}, x.options());
  const int64_t cols_per_wg = (int64_t)kSkinnyWaves * (act ? kRows / 2 : kRows);
  const int64_t nwg = (n_out + cols_per_wg - 1) / cols_per_wg;
  DTG_CHECK(nwg < (int64_t(1) << 31), name, ": too many workgroups");
  if (act)
    skinny_launch<1>(M, (unsigned)nwg, x, w, bp, y, N, K);
  else
    skinny_launch<0>(M, (unsigned)nwg, x, w, bp, y, N, K);
  DTG_LAUNCH_CHECK();
  return y;
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) { m.impl("skinny_linear", &skinny_linear); }

}  // namespace dtg
