// Weight-only FP8 skinny GEMM for the decode step's projections:
//   y[M, N] = (x[M, K] @ float(wq[N, K])^T) * scale[N] (+ bias),   1 <= M <= 16,
// x, bias, y bf16; wq OCP e4m3fn (the format gfx950 converts in hardware, not MI300's fnuz), one byte per
// weight; scale f32, one per weight row.  f32 accumulation, one multiply by the scale after the
// reduction, then the bias, then one rounding.  At M = 1 the bf16 kernel (skinny_gemm.hip) streams its
// weights at the copy rate, so the only lever left is the number of bytes: this kernel reads half of them.
//
// The shape is skinny_gemm.hip's (the guide's "GEMV / M <= 16 decode weights" row): weights straight to
// VGPRs in 16-B non-temporal loads -- 16 weights per load here --, several loads in flight per lane, no
// LDS, no barrier; x, which every wave re-reads, keeps the default cache policy.  A wave owns kRows = 4
// weight rows (with the SwiGLU epilogue the gate rows n0, n0 + 1 and the up rows I + n0, I + n0 + 1), a
// workgroup 4 waves.  Lane l walks K in 16-element chunks l, l + 64, l + 128, ...  A chunk is widened
// and consumed in two halves of 8 elements (two dwords per weight row through v_cvt_pk_f32_fp8, one
// 16-B x load per row of x), so the widened weights held at once are the bf16 kernel's 4 x 8 floats.
// bf16 x e4m3 products are exact in f32 (8 + 4 significand bits).
//
// Summation order of one output (m, n): the lane's chunks in ascending order, sixteen fmaf per chunk in
// element order, then the xor butterfly over the 64 lanes (offsets 32, 16, ..., 1).  It depends on
// neither M nor the other rows nor on the slot of the wave the weight row sits in: M is a template
// parameter for unrolling only, so row m of a batched call equals the single-row call bit for bit.
// No atomics, no split-K across workgroups.  Lanes past K load nothing and add nothing; weight rows
// past N are clamped to row N - 1 (loaded, never stored).
//
// act = 1 (SwiGLU): the gate and the up sums are each scaled by their own row's scale, biased and
// rounded to bf16 exactly as the plain form stores them, widened again and passed through
// mlp_act::SwiGLU::fwd: the result equals swiglu_fwd(skinny_linear_fp8(x, wq, scale)) bit for bit.
#include "mlp_act.h"

namespace dtg {

namespace {

constexpr int kFp8MaxM = 16;
constexpr int kFp8Threads = 256;
constexpr int kFp8Waves = kFp8Threads / kWave;
constexpr int kFp8Rows = 4;    // weight rows per wave
constexpr int kFp8Chunk = 16;  // weights per 16-B load

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Four e4m3 bytes of `word` (memory order = ascending byte) as f32: v_cvt_pk_f32_fp8, low then high half.
__device__ __forceinline__ void widen4_e4m3(uint32_t word, float* out) {
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)word, false);
  const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)word, true);
  out[0] = lo[0];
  out[1] = lo[1];
  out[2] = hi[0];
  out[3] = hi[1];
}

template <int M, int ACT>
__global__ __launch_bounds__(kFp8Threads) void skinny_gemm_fp8_kernel(
    const uint16_t* __restrict__ x, int64_t x_stride, const uint8_t* __restrict__ w,
    const float* __restrict__ scale, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int64_t N,
    int64_t K) {
  constexpr int kUnroll = M <= 4 ? 4 : (M <= 8 ? 2 : 1);
  constexpr int kCols = ACT ? kFp8Rows / 2 : kFp8Rows;  // output columns per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n_out = ACT ? N / 2 : N;
  const int64_t n0 = ((int64_t)blockIdx.x * kFp8Waves + wave) * kCols;
  if (n0 >= n_out) return;  // wave-uniform; the kernel has no barrier

  int64_t wrow[kFp8Rows];  // weight row of slot r, clamped into the matrix
#pragma unroll
  for (int r = 0; r < kFp8Rows; ++r) {
    const int64_t c = n0 + (ACT ? r % kCols : r);
    const int64_t cc = c < n_out ? c : n_out - 1;
    wrow[r] = ACT && r >= kCols ? n_out + cc : cc;
  }

  float acc[M][kFp8Rows];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < kFp8Rows; ++r) acc[m][r] = 0.f;

  const int64_t chunks = K / kFp8Chunk;
  for (int64_t c0 = 0; c0 < chunks; c0 += (int64_t)kWave * kUnroll) {
    u32x4 wv[kUnroll][kFp8Rows];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t c = c0 + u * kWave + lane;
      if (c < chunks) {
#pragma unroll
        for (int r = 0; r < kFp8Rows; ++r)
          wv[u][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(w + wrow[r] * K + c * kFp8Chunk));
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t c = c0 + u * kWave + lane;
      if (c < chunks) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {  // elements 8 h .. 8 h + 7 of the chunk
          float wf[kFp8Rows][8];
#pragma unroll
          for (int r = 0; r < kFp8Rows; ++r) {
            widen4_e4m3(wv[u][r][2 * h], wf[r]);
            widen4_e4m3(wv[u][r][2 * h + 1], wf[r] + 4);
          }
#pragma unroll
          for (int m = 0; m < M; ++m) {
            float xf[8];
            load8(x + m * x_stride + c * kFp8Chunk + h * 8, xf);
#pragma unroll
            for (int r = 0; r < kFp8Rows; ++r)
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
    for (int r = 0; r < kFp8Rows; ++r) acc[m][r] = wave_sum(acc[m][r]);

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
  a *= scale[n];
  if (ACT) b *= scale[n_out + n];
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
void skinny_fp8_launch(int64_t M, unsigned grid, const at::Tensor& x, const at::Tensor& wq, const at::Tensor& scale,
                       const uint16_t* bias, at::Tensor& y, int64_t N, int64_t K) {
#define DTG_SKINNY_FP8_CASE(M_)                                                                            \
  case M_:                                                                                                 \
    skinny_gemm_fp8_kernel<M_, ACT><<<grid, kFp8Threads, 0, stream()>>>(                                   \
        bf16_ptr(x), x.stride(0), reinterpret_cast<const uint8_t*>(wq.data_ptr()), scale.data_ptr<float>(), \
        bias, bf16_mut(y), N, K);                                                                          \
    break;
  switch (M) {
    DTG_SKINNY_FP8_CASE(1) DTG_SKINNY_FP8_CASE(2) DTG_SKINNY_FP8_CASE(3) DTG_SKINNY_FP8_CASE(4)
    DTG_SKINNY_FP8_CASE(5) DTG_SKINNY_FP8_CASE(6) DTG_SKINNY_FP8_CASE(7) DTG_SKINNY_FP8_CASE(8)
    DTG_SKINNY_FP8_CASE(9) DTG_SKINNY_FP8_CASE(10) DTG_SKINNY_FP8_CASE(11) DTG_SKINNY_FP8_CASE(12)
    DTG_SKINNY_FP8_CASE(13) DTG_SKINNY_FP8_CASE(14) DTG_SKINNY_FP8_CASE(15) DTG_SKINNY_FP8_CASE(16)
    default: DTG_CHECK(false, "skinny_linear_fp8: unreachable M");
  }
#undef DTG_SKINNY_FP8_CASE
}

}  // namespace

at::Tensor skinny_linear_fp8(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& scale,
                             const c10::optional<at::Tensor>& bias, int64_t act) {
  const char* name = "skinny_linear_fp8";
  DTG_CHECK_CUDA_BF16(x);
  DTG_CHECK(wq.is_cuda() && wq.scalar_type() == at::kFloat8_e4m3fn, name, ": wq must be a float8_e4m3fn GPU tensor");
  DTG_CHECK(act == 0 || act == 1, name, ": act must be 0 (none) or 1 (SwiGLU)");
  DTG_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.size(0) <= kFp8MaxM, name, ": x must be [M, K] with 1 <= M <= ",
            kFp8MaxM);
  const int64_t M = x.size(0), K = x.size(1);
  DTG_CHECK(K % kFp8Chunk == 0, name, ": K must be a multiple of 16");
  DTG_CHECK(x.stride(1) == 1 && x.stride(0) % 8 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, name,
            ": x must have unit inner stride and 16-B aligned rows");
  DTG_CHECK(wq.dim() == 2 && wq.size(1) == K && wq.size(0) >= 1 && wq.is_contiguous() && wq.device() == x.device() &&
                reinterpret_cast<uintptr_t>(wq.data_ptr()) % 16 == 0,
            name, ": wq must be a contiguous 16-B aligned [N, K] on x's device");
  const int64_t N = wq.size(0);
  DTG_CHECK(scale.is_cuda() && scale.scalar_type() == at::kFloat && scale.dim() == 1 && scale.size(0) == N &&
                scale.is_contiguous() && scale.device() == x.device(),
            name, ": scale must be a contiguous f32 [N] on x's device");
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
  const int64_t cols_per_wg = (int64_t)kFp8Waves * (act ? kFp8Rows / 2 : kFp8Rows);
  const int64_t nwg = (n_out + cols_per_wg - 1) / cols_per_wg;
  DTG_CHECK(nwg < (int64_t(1) << 31), name, ": too many workgroups");
  if (act)
    skinny_fp8_launch<1>(M, (unsigned)nwg, x, wq, scale, bp, y, N, K);
  else
    skinny_fp8_launch<0>(M, (unsigned)nwg, x, wq, scale, bp, y, N, K);
  DTG_LAUNCH_CHECK();
  return y;
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) { m.impl("skinny_linear_fp8", &skinny_linear_fp8); }

}  // namespace dtg
