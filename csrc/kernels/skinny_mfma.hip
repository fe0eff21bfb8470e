// MFMA skinny GEMM for decode and verify steps of up to 64 rows: y[M, N] = x[M, K] @ w[N, K]^T (+ bias),
// 1 <= M <= 64, K % 32 == 0, all bf16, f32 accumulation, one rounding.  At these M the product is still a
// weight-streaming problem (64 flop per weight byte at M = 64), but the fmaf kernel of skinny_gemm.hip runs out
// of VALU and registers long before its 16-row limit.  Here the weights go to v_mfma_f32_16x16x32_bf16: the
// single read of every weight stays, and a row of x costs a quarter of an MFMA per 512 weights instead of
// 512 fmaf.
//
// Operands.  Both matrices are K-contiguous and so is a lane's 8-element slice of a 16x16x32 operand, so
// both go from global memory straight into operand registers with one 16-B load per lane; nothing is staged
// in LDS.  For the 32-wide K slab at k0, lane l loads
//   A (weights): 8 elements of weight row n0 + (l & 15) at k0 + 8 * (l >> 4), non-temporal (read once);
//   B (x):       8 elements of x row m0 + (l & 15) at the same k, default policy (every workgroup re-reads x,
//                it lives in L1 / L2).
// A and B share the k mapping, so the k order inside a slab is the hardware's own business.  The accumulator
// of lane l is C[4 * (l >> 4) + r][l & 15], r = 0..3: output columns n0 + 4 * (l >> 4) + r of x row
// m0 + (l & 15).  Weight rows past N are clamped to row N - 1 and x rows past M to row M - 1: loaded, never
// stored.
//
// Work split.  A workgroup owns one 16-column tile of the output (with the SwiGLU epilogue the gate tile and
// the matching up tile) and all rows of x.  Its kWaves = 8 waves split K: wave v takes slabs v, v + 8, ...
// MT = ceil(M / 16) is a template parameter; per slab a wave issues one weight load (two with act), MT x
// loads and MT (2 MT) MFMAs into MT f32x4 accumulators.  The slab loop runs kUnroll = 8 slabs per pass: the 8
// weight loads of a pass (8 KB per wave, 16 KB with act) are issued before its first MFMA.  A last partial
// pass runs the same body with wave-uniform guards.
//
// Reduction.  Every wave writes its partial accumulators to LDS; after one barrier wave t < MT adds the
// partials of M tile t in ascending wave order, adds the bias, rounds and stores its own outputs.  No atomics,
// no split-K across workgroups.
//
// Summation order of output (m, n): inside a slab the hardware's, slabs ascending within a wave, waves
// ascending.  It depends on K alone: M, MT, the other rows and the slot of the tile do not enter it, so row m
// of a batched call equals the single-row call bit for bit.
//
// Epilogue as skinny_gemm.hip: act = 1 (SwiGLU) biases and rounds the gate and the up sum each as the plain
// form stores them, widens them and passes them through mlp_act::SwiGLU::fwd: bitwise swiglu_fwd of the plain
// product.
//
// Known costs.  A workgroup re-reads all of x: the L1 / L2 traffic for x is M / 16 times the weight traffic
// (4x at M = 64).  The grid is ceil(N / 16) workgroups, so N = 1024 fills a quarter of the CUs.  A K of fewer
// than 32 * 8 * 8 elements never runs a full pass.  See profiles/r8/skinny_mfma/README.md.
#include "mlp_act.h"

namespace dtg {

namespace {

constexpr int kMfmaMaxM = 64;
constexpr int kWaves = 8;   // waves of a workgroup; they split K
constexpr int kUnroll = 8;  // slabs per pass: weight loads in flight per wave
constexpr int kSlab = 32;   // K elements of one MFMA
constexpr int kTile = 16;   // output columns of a workgroup, rows of x per MFMA

__device__ __forceinline__ bf16x8 frag(const uint16_t* p) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u16x8*>(p));
}

__device__ __forceinline__ bf16x8 frag_nt(const uint16_t* p) {
  return __builtin_bit_cast(bf16x8, __builtin_nontemporal_load(reinterpret_cast<const u16x8*>(p)));
}

template <int MT, int ACT>
__global__ __launch_bounds__(kWaves * kWave) void skinny_mfma_kernel(
    const uint16_t* __restrict__ x, int64_t x_stride, const uint16_t* __restrict__ w,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int M, int64_t N, int64_t K) {
  constexpr int NW = ACT ? 2 : 1;  // weight tiles of the workgroup: plain | gate, up
  __shared__ f32x4 part[kWaves][NW * MT][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = lane & 15, kq = lane >> 4;
  const int64_t n_out = ACT ? N / 2 : N;
  const int64_t n0 = (int64_t)blockIdx.x * kTile;

  // this lane's operand rows at k = 8 * kq, clamped into the matrices
  const int64_t c = n0 + row < n_out ? n0 + row : n_out - 1;
  const uint16_t* wp[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) wp[j] = w + (j * n_out + c) * K + 8 * kq;
  const uint16_t* xp[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = kTile * t + row;
    xp[t] = x + (int64_t)(m < M ? m : M - 1) * x_stride + 8 * kq;
  }

  f32x4 acc[NW][MT];
#pragma unroll
  for (int j = 0; j < NW; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int64_t slabs = K / kSlab;
  // One pass: slabs s0, s0 + kWaves, ..., s0 + (kUnroll - 1) * kWaves; FULL = all of them exist.
  auto pass = [&](int64_t s0, auto full) {
    constexpr bool FULL = decltype(full)::value;
    bf16x8 wf[kUnroll][NW];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t s = s0 + u * kWaves;
      if (FULL || s < slabs) {
#pragma unroll
        for (int j = 0; j < NW; ++j) wf[u][j] = frag_nt(wp[j] + s * kSlab);
      }
    }
    // keep the pass's weight loads ahead of its first MFMA: left alone, the scheduler sinks them between the
    // MFMAs to save registers and two are in flight instead of kUnroll
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t s = s0 + u * kWaves;
      if (FULL || s < slabs) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const bf16x8 xf = frag(xp[t] + s * kSlab);
#pragma unroll
          for (int j = 0; j < NW; ++j)
            acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u][j], xf, acc[j][t], 0, 0, 0);
        }
      }
    }
  };
  int64_t s0 = wave;
  for (; s0 + (kUnroll - 1) * kWaves < slabs; s0 += kUnroll * kWaves) pass(s0, std::true_type{});
  if (s0 < slabs) pass(s0, std::false_type{});

#pragma unroll
  for (int j = 0; j < NW; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t) part[wave][j * MT + t][lane] = acc[j][t];
  __syncthreads();
  if (wave >= MT) return;

  // wave t reduces M tile t: lane l holds columns n0 + 4 * kq + r of x row 16 * t + row
  const int t = wave;
  f32x4 sum[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    sum[j] = part[0][j * MT + t][lane];
#pragma unroll
    for (int v = 1; v < kWaves; ++v) sum[j] += part[v][j * MT + t][lane];
  }
  const int m = kTile * t + row;
  if (m >= M) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t n = n0 + 4 * kq + r;
    if (n >= n_out) break;
    float a = sum[0][r], b = ACT ? sum[NW - 1][r] : 0.f;
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
}

// The checks on the operands and the grid.
struct MfmaPlan {
  int64_t M, N, K;
  const uint16_t* bias = nullptr;
  unsigned grid;
};

MfmaPlan mfma_plan(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, int64_t act) {
  const char* name = "skinny_linear_mfma";
  MfmaPlan p;
  DTG_CHECK_CUDA_BF16(x);
  DTG_CHECK_CUDA_BF16(w);
  DTG_CHECK(act == 0 || act == 1, name, ": act must be 0 (none) or 1 (SwiGLU)");
  DTG_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.size(0) <= kMfmaMaxM, name, ": x must be [M, K] with 1 <= M <= ",
            kMfmaMaxM);
  p.M = x.size(0), p.K = x.size(1);
  DTG_CHECK(p.K % kSlab == 0, name, ": K must be a multiple of ", kSlab);
  DTG_CHECK(x.stride(1) == 1 && x.stride(0) % 8 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, name,
            ": x must have unit inner stride and 16-B aligned rows");
  DTG_CHECK(w.dim() == 2 && w.size(1) == p.K && w.size(0) >= 1 && w.is_contiguous() && w.device() == x.device() &&
                reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
            name, ": w must be a contiguous 16-B aligned [N, K] on x's device");
  p.N = w.size(0);
  DTG_CHECK(act == 0 || p.N % 2 == 0, name, ": the SwiGLU epilogue needs an even N (gate rows, then up rows)");
  DTG_CHECK(p.N < (int64_t(1) << 32) && p.K < (int64_t(1) << 40), name, ": matrix too large");
  if (bias.has_value() && bias->defined()) {
    DTG_CHECK_CUDA_BF16(*bias);
    DTG_CHECK(bias->dim() == 1 && bias->size(0) == p.N && bias->is_contiguous() && bias->device() == x.device(), name,
              ": bias must be a contiguous [N]");
    p.bias = bf16_ptr(*bias);
  }
  p.grid = (unsigned)(((act ? p.N / 2 : p.N) + kTile - 1) / kTile);
  return p;
}

// Launches the instantiation for ceil(p.M / 16) M tiles: MT counts down from the largest.
template <int ACT, int MT = kMfmaMaxM / kTile>
void mfma_launch(const MfmaPlan& p, const at::Tensor& x, const at::Tensor& w, at::Tensor& y) {
  if constexpr (MT >= 1) {
    if ((p.M + kTile - 1) / kTile != MT) return mfma_launch<ACT, MT - 1>(p, x, w, y);
    skinny_mfma_kernel<MT, ACT><<<p.grid, kWaves * kWave, 0, stream()>>>(bf16_ptr(x), x.stride(0), bf16_ptr(w), p.bias,
                                                                         bf16_mut(y), (int)p.M, p.N, p.K);
  }
}

}  // namespace

at::Tensor skinny_linear_mfma(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias,
                              int64_t act) {
  const auto p = mfma_plan(x, w, bias, act);
  const c10::DeviceGuard g(x.device());
  auto y = at::empty({p.M, act ? p.N / 2 : p.N}, x.options());
  if (act)
    mfma_launch<1>(p, x, w, y);
  else
    mfma_launch<0>(p, x, w, y);
  DTG_LAUNCH_CHECK();
  return y;
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) { m.impl("skinny_linear_mfma", &skinny_linear_mfma); }

}  // namespace dtg
