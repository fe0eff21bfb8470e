// Weight-only MXFP4 skinny GEMM for decode and verify steps of up to 64 rows:
//   y[M, N] = x[M, K] @ deq(wq, scales)[N, K]^T (+ bias),  1 <= M <= 64, K % 32 == 0,
// x, bias and y bf16, f32 accumulation, one rounding.  The weights are OCP microscaling FP4: e2m1 codes, two per
// byte (element 2 j in the low nibble of byte j), and one e8m0 byte per block of 32 consecutive elements of a
// row, 4.25 bits per weight streamed.  gfx950 widens the format in hardware: v_cvt_scalef32_pk_bf16_fp4 turns the
// two codes of one byte into two bf16 values and multiplies them by the block's scale in the same instruction.
// A code times a power of two is exactly a bf16 value, so the kernel computes the bf16 product of
// skinny_mfma.hip on the dequantised matrix, with the same matrix instruction and the same promises.
//
// Operands.  One 16-B load holds 32 codes: exactly one MX block.  The unit of K is therefore a super-slab of
// 128 elements (four 16x16x32 MFMAs).  For super-slab s, lane l takes
//   A (weights): the block kq = l >> 4 of weight row n0 + (l & 15): one non-temporal 16-B load at byte
//                (128 s + 32 kq) / 2 of the row and one byte load of the block's scale, which becomes a float
//                by uint32(byte) << 23.  Dword i of the load widens, through four conversions with byte selects
//                0..3, into the bf16x8 A fragment of the super-slab's i-th MFMA;
//   B (x):       8 elements of x row m0 + (l & 15) at 128 s + 32 kq + 8 i for that MFMA, default policy.
// A and B share the k mapping (element j of lane group kq of MFMA i is k = 128 s + 32 kq + 8 i + j on both
// sides), so which k the hardware calls which inside a super-slab does not matter.  The accumulator layout, the
// clamping of weight rows past N and x rows past M (loaded, never stored) are those of skinny_mfma.hip.
//
// Work split.  A workgroup owns one 16-column tile of the output (with the SwiGLU epilogue the gate tile and
// the matching up tile) and all rows of x.  Its kWaves = 8 waves split K: wave v takes super-slabs v, v + 8, ...
// MT = ceil(M / 16) is a template parameter.  The loop runs kUnroll super-slabs per pass; every weight load and
// scale load of a pass is issued before its first conversion.  A 16-B load covers four times the K of the bf16
// kernel's, so K = 4096 is only 32 super-slabs, four per wave, and the bf16 kernel's eight per pass do not carry
// over: kUnroll = 2 was measured fastest against 4 and 8 (profiles/r8/skinny_mxfp4/README.md; -DDTG_MXFP4_UNROLL=n
// builds the others).  A last partial
// pass runs the same body with guards: a super-slab that does not exist is skipped (wave-uniform), and in a last
// super-slab that K % 128 != 0 cuts short the lanes whose block lies past K load nothing and put zeros into both
// fragments, so they add exact zeros.
//
// Reduction, summation order and epilogue as skinny_mfma.hip: partials through LDS and one barrier, wave t < MT
// sums M tile t in ascending wave order; no atomics, no split-K across workgroups.  The order of output (m, n)
// is: inside an MFMA the hardware's, the four MFMAs of a super-slab ascending, super-slabs ascending within a
// wave, waves ascending.  It depends on K alone, so row m of a batched call equals the single-row call bit for
// bit.  act = 1 (SwiGLU) biases and rounds the gate and the up sum each as the plain form stores them and passes
// them through mlp_act::SwiGLU::fwd: bitwise swiglu_fwd of the plain product.
//
// The format guarantees the kernel relies on (ops.quantize_mxfp4_rows): scale bytes 0 and 255 never occur, so
// byte << 23 is a normal power of two and never NaN.
//
// Known costs.  16 conversions per four MFMAs and per weight tile run on the VALU in front of the matrix pipe;
// a workgroup re-reads all of x (at 4.25 bits per weight the L1 / L2 traffic for x is 3.8 M / 16 times the
// weight traffic, 15x at M = 64); the grid is ceil(N / 16) workgroups, so N = 1024 fills a quarter of the CUs;
// a scale byte is a 1-B load per lane per super-slab.  See profiles/r8/skinny_mxfp4/README.md.
#include "mlp_act.h"

namespace dtg {

namespace {

constexpr int kMxMaxM = 64;
constexpr int kWaves = 8;    // waves of a workgroup; they split K
#ifndef DTG_MXFP4_UNROLL
#define DTG_MXFP4_UNROLL 2
#endif
constexpr int kUnroll = DTG_MXFP4_UNROLL;  // super-slabs per pass: 16-B weight loads in flight per wave and tile
constexpr int kBlock = 32;   // elements of one MX block: one scale byte, one 16-B load, the K of one MFMA
constexpr int kSuper = 128;  // K elements of a super-slab: the four blocks of the four lane groups
constexpr int kTile = 16;    // output columns of a workgroup, rows of x per MFMA

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bf16x8 frag(const uint16_t* p) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u16x8*>(p));
}

// The 8 codes of one dword (elements 2 b, 2 b + 1 in byte b, low nibble first) times `scale`, as bf16.  The byte
// select of the conversion must be a literal.
__device__ __forceinline__ bf16x8 widen_fp4(uint32_t d, float scale) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3);
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

template <int MT, int ACT>
__global__ __launch_bounds__(kWaves * kWave) void skinny_mxfp4_kernel(
    const uint16_t* __restrict__ x, int64_t x_stride, const uint8_t* __restrict__ wq,
    const uint8_t* __restrict__ scales, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int M, int64_t N,
    int64_t K) {
  constexpr int NW = ACT ? 2 : 1;  // weight tiles of the workgroup: plain | gate, up
  __shared__ f32x4 part[kWaves][NW * MT][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = lane & 15, kq = lane >> 4;
  const int64_t n_out = ACT ? N / 2 : N;
  const int64_t n0 = (int64_t)blockIdx.x * kTile;
  const int64_t blocks = K / kBlock;  // MX blocks of a row

  // this lane's operand rows at block kq, clamped into the matrices
  const int64_t c = n0 + row < n_out ? n0 + row : n_out - 1;
  const uint8_t* wp[NW];
  const uint8_t* sp[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    wp[j] = wq + (j * n_out + c) * (K / 2) + (kBlock / 2) * kq;
    sp[j] = scales + (j * n_out + c) * blocks + kq;
  }
  const uint16_t* xp[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = kTile * t + row;
    xp[t] = x + (int64_t)(m < M ? m : M - 1) * x_stride + kBlock * kq;
  }

  f32x4 acc[NW][MT];
#pragma unroll
  for (int j = 0; j < NW; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int64_t supers = (K + kSuper - 1) / kSuper, whole = K / kSuper;
  // One pass: super-slabs s0, s0 + kWaves, ..., s0 + (kUnroll - 1) * kWaves; FULL = all of them exist and none
  // is cut short by K.  Otherwise lane group kq of super-slab s has a block only when 4 s + kq < blocks.
  auto pass = [&](int64_t s0, auto full) {
    constexpr bool FULL = decltype(full)::value;
    u32x4 wv[kUnroll][NW];
    uint32_t sc[kUnroll][NW];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t s = s0 + u * kWaves;
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        wv[u][j] = u32x4{0u, 0u, 0u, 0u};  // the code of +0
        sc[u][j] = 127u;                   // 2^0
      }
      if (FULL || 4 * s + kq < blocks) {
#pragma unroll
        for (int j = 0; j < NW; ++j) {
          wv[u][j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[j] + s * (kSuper / 2)));
          sc[u][j] = sp[j][4 * s];
        }
      }
    }
    // keep the pass's weight and scale loads ahead of its first conversion, as skinny_mfma.hip does
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t s = s0 + u * kWaves;
      if (FULL || s < supers) {
        const bool mine = FULL || 4 * s + kq < blocks;
        float scale[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) scale[j] = __uint_as_float(sc[u][j] << 23);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          bf16x8 wf[NW];
#pragma unroll
          for (int j = 0; j < NW; ++j) wf[j] = widen_fp4(wv[u][j][i], scale[j]);
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            bf16x8 xf = __builtin_bit_cast(bf16x8, u16x8{0, 0, 0, 0, 0, 0, 0, 0});
            if (mine) xf = frag(xp[t] + s * kSuper + 8 * i);
#pragma unroll
            for (int j = 0; j < NW; ++j)
              acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf, acc[j][t], 0, 0, 0);
          }
        }
      }
    }
  };
  int64_t s0 = wave;
  for (; s0 + (kUnroll - 1) * kWaves < whole; s0 += kUnroll * kWaves) pass(s0, std::true_type{});
  if (s0 < supers) pass(s0, std::false_type{});

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
struct MxPlan {
  int64_t M, N, K;
  const uint16_t* bias = nullptr;
  unsigned grid;
};

MxPlan mx_plan(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& scales,
               const c10::optional<at::Tensor>& bias, int64_t act) {
  const char* name = "skinny_linear_mxfp4";
  MxPlan p;
  DTG_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16, name, ": x must be a bf16 GPU tensor");
  DTG_CHECK(wq.is_cuda() && wq.scalar_type() == at::kByte && scales.is_cuda() && scales.scalar_type() == at::kByte,
            name, ": wq and scales must be uint8 GPU tensors");
  DTG_CHECK(act == 0 || act == 1, name, ": act must be 0 (none) or 1 (SwiGLU)");
  DTG_CHECK(x.dim() == 2 && x.size(0) >= 1 && x.size(0) <= kMxMaxM, name, ": x must be [M, K] with 1 <= M <= ",
            kMxMaxM);
  p.M = x.size(0), p.K = x.size(1);
  DTG_CHECK(p.K % kBlock == 0, name, ": K must be a multiple of ", kBlock);
  DTG_CHECK(x.stride(1) == 1 && x.stride(0) % 8 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, name,
            ": x must have unit inner stride and 16-B aligned rows");
  DTG_CHECK(wq.dim() == 2 && wq.size(1) == p.K / 2 && wq.size(0) >= 1 && wq.is_contiguous() &&
                wq.device() == x.device() && reinterpret_cast<uintptr_t>(wq.data_ptr()) % 16 == 0,
            name, ": wq must be a contiguous 16-B aligned uint8 [N, K / 2] on x's device");
  p.N = wq.size(0);
  DTG_CHECK(scales.dim() == 2 && scales.size(0) == p.N && scales.size(1) == p.K / kBlock && scales.is_contiguous() &&
                scales.device() == x.device(),
            name, ": scales must be a contiguous uint8 [N, K / 32] on x's device");
  DTG_CHECK(act == 0 || p.N % 2 == 0, name, ": the SwiGLU epilogue needs an even N (gate rows, then up rows)");
  DTG_CHECK(p.N < (int64_t(1) << 32) && p.K < (int64_t(1) << 40), name, ": matrix too large");
  if (bias.has_value() && bias->defined()) {
    DTG_CHECK(bias->is_cuda() && bias->scalar_type() == at::kBFloat16 && bias->dim() == 1 && bias->size(0) == p.N &&
                  bias->is_contiguous() && bias->device() == x.device(),
              name, ": bias must be a contiguous bf16 [N] on x's device");
    p.bias = bf16_ptr(*bias);
  }
  p.grid = (unsigned)(((act ? p.N / 2 : p.N) + kTile - 1) / kTile);
  return p;
}

// Launches the instantiation for ceil(p.M / 16) M tiles: MT counts down from the largest.
template <int ACT, int MT = kMxMaxM / kTile>
void mx_launch(const MxPlan& p, const at::Tensor& x, const at::Tensor& wq, const at::Tensor& scales, at::Tensor& y) {
  if constexpr (MT >= 1) {
    if ((p.M + kTile - 1) / kTile != MT) return mx_launch<ACT, MT - 1>(p, x, wq, scales, y);
    skinny_mxfp4_kernel<MT, ACT><<<p.grid, kWaves * kWave, 0, stream()>>>(
        bf16_ptr(x), x.stride(0), wq.data_ptr<uint8_t>(), scales.data_ptr<uint8_t>(), p.bias, bf16_mut(y), (int)p.M,
        p.N, p.K);
  }
}

}  // namespace

at::Tensor skinny_linear_mxfp4(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& scales,
                               const c10::optional<at::Tensor>& bias, int64_t act) {
  const auto p = mx_plan(x, wq, scales, bias, act);
  const c10::DeviceGuard g(x.device());
  auto y = at::empty({p.M, act ? p.N / 2 : p.N}, x.options());
  if (act)
    mx_launch<1>(p, x, wq, scales, y);
  else
    mx_launch<0>(p, x, wq, scales, y);
  DTG_LAUNCH_CHECK();
  return y;
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) { m.impl("skinny_linear_mxfp4", &skinny_linear_mxfp4); }

}  // namespace dtg
