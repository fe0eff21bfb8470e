// MFMA skinny GEMMs for decode and verify steps of up to 64 rows: y[M, N] = x[M, K] @ W[N, K]^T (+ bias),
// 1 <= M <= 64, K % 32 == 0, x, bias and y bf16, f32 accumulation, one rounding.  At these M the product is still
// a weight-streaming problem (64 flop per weight byte at M = 64), but the fmaf kernel of skinny_gemm.hip runs out
// of VALU and registers long before its 16-row limit.  Here the weights go to v_mfma_f32_16x16x32_bf16: the
// single read of every weight stays, and a row of x costs a quarter of an MFMA per 512 weights instead of
// 512 fmaf.  One kernel template serves every weight format; a format (below) says how the weights of one step
// of the K loop reach the A fragments of its MFMAs and nothing else.
//
// Operands.  Both matrices are K-contiguous and so is a lane's 8-element slice of a 16x16x32 operand, so both go
// from global memory straight into registers with 16-B loads; nothing is staged in LDS.  The K loop steps in
// units of kUnit elements, kMfmas = kUnit / 32 MFMAs each, and lane group kq = l >> 4 owns a quarter of a unit:
// elements kq * kUnit / 4 + 8 i + j, j = 0..7, are its slice of MFMA i.  For unit s, lane l loads
//   A (weights): its quarter of weight row n0 + (l & 15), as the format says, non-temporal (read once);
//   B (x):       for MFMA i, 8 elements of x row m0 + (l & 15) at s * kUnit + kq * kUnit / 4 + 8 i, default
//                policy (every workgroup re-reads x, it lives in L1 / L2).
// A and B share the k mapping, so which k the hardware calls which inside an MFMA does not matter.  The
// accumulator of lane l is C[4 * (l >> 4) + r][l & 15], r = 0..3: output columns n0 + 4 * (l >> 4) + r of x row
// m0 + (l & 15).  Weight rows past N are clamped to row N - 1 and x rows past M to row M - 1: loaded, never
// stored.
//
// Work split.  A workgroup owns one 16-column tile of the output (with the SwiGLU epilogue the gate tile and
// the matching up tile) and all rows of x.  Its kWaves = 8 waves split K: wave v takes units v, v + 8, ...
// MT = ceil(M / 16) is a template parameter; per unit a wave issues one weight load (two with act), kMfmas * MT
// x loads and kMfmas * MT (2 MT with act) MFMAs into MT f32x4 accumulators per weight tile.  The loop runs
// kUnroll units per pass: every weight load of a pass is issued before its first conversion or MFMA.  A last
// partial pass runs the same body with guards: a unit that does not exist is skipped (wave-uniform), and in a
// last unit that K cuts short the lanes whose quarter lies past K load nothing and put zeros into both
// fragments, so they add exact zeros.
//
// Reduction.  Every wave writes its partial accumulators to LDS; after one barrier wave t < MT adds the
// partials of M tile t in ascending wave order, adds the bias, rounds and stores its own outputs.  No atomics,
// no split-K across workgroups.
//
// Summation order of output (m, n): inside an MFMA the hardware's, the MFMAs of a unit ascending, units
// ascending within a wave, waves ascending.  It depends on K and the format alone: M, MT, the other rows and the
// slot of the tile do not enter it, so row m of a batched call equals the single-row call bit for bit.
//
// Epilogue as skinny_gemm.hip (skinny::store): act = 1 (SwiGLU) biases and rounds the gate and the up sum each
// as the plain form stores them, widens them and passes them through mlp_act::SwiGLU::fwd: bitwise swiglu_fwd of
// the plain product.
//
// Known costs of every format.  A workgroup re-reads all of x: the L1 / L2 traffic for x is M / 16 times the
// traffic of as many bf16 weights (4x at M = 64).  The grid is ceil(N / 16) workgroups, so N = 1024 fills a
// quarter of the CUs.
//
// Bf16Mfma (skinny_linear_mfma): a unit is one MFMA, and a lane's 16-B load is its A fragment as it stands.
// K % 32 == 0 is the unit, so no unit is cut short.  kUnroll = 8: the 8 weight loads of a pass are 8 KB per
// wave, 16 KB with act.  A K of fewer than 32 * 8 * 8 elements never runs a full pass.  See
// profiles/r8/skinny_mfma/README.md.
//
// Mxfp4Mfma (skinny_linear_mxfp4): weight-only OCP microscaling FP4, y = x @ deq(wq, scales)^T.  e2m1 codes,
// two per byte (element 2 j in the low nibble of byte j), and one e8m0 byte per block of 32 consecutive
// elements of a row, 4.25 bits per weight streamed.  gfx950 widens the format in hardware:
// v_cvt_scalef32_pk_bf16_fp4 turns the two codes of one byte into two bf16 values and multiplies them by the
// block's scale in the same instruction.  A code times a power of two is exactly a bf16 value, so the kernel
// computes the bf16 product of Bf16Mfma on the dequantised matrix, with the same promises.  One 16-B load holds
// 32 codes: exactly one MX block, so a unit is 128 elements (four MFMAs) and a lane's quarter is the block kq of
// its row: one 16-B load at byte (128 s + 32 kq) / 2 of the row and one byte load of the block's scale, which
// becomes a float by uint32(byte) << 23.  Dword i of the load widens, through four conversions with byte selects
// 0..3, into the A fragment of the unit's i-th MFMA.  K % 128 != 0 cuts the last unit short: lane group kq has
// a block only when 4 s + kq < K / 32.  The format guarantees the kernel relies on (ops.quantize_mxfp4_rows):
// scale bytes 0 and 255 never occur, so byte << 23 is a normal power of two and never NaN.  A 16-B load covers
// four times the K of the bf16 form's, so K = 4096 is only 32 units, four per wave, and the bf16 form's eight
// per pass do not carry over: kUnroll = 2 was measured fastest against 4 and 8
// (profiles/r8/skinny_mxfp4/README.md; -DDTG_MXFP4_UNROLL=n builds the others).  Its own costs: 16 conversions
// per four MFMAs and per weight tile run on the VALU in front of the matrix pipe; at 4.25 bits per weight the
// traffic for x is 3.8 M / 16 times the weight traffic, 15x at M = 64; a scale byte is a 1-B load per lane per
// unit.
//
// W4A8 (skinny_linear_mxfp4_a8, a kernel of its own below): the same MXFP4 weights against microscaled FP8
// activations, y = deq(xq, xs) @ deq(wq, scales)^T: xq e4m3 bytes [M, K], xs one e8m0 byte per 32 consecutive
// elements of a row, as quantize_mxfp8_rows (below) makes them from bf16.  v_mfma_scale_f32_16x16x128_f8f6f4
// takes both operands as they lie in memory: with cbsz = 4 (A is FP4) and blgp = 0 (B is e4m3) a lane's A operand
// is four dwords of e2m1 codes, its B operand eight dwords of e4m3 bytes, and each comes with one e8m0 scale in
// byte 0 of a VGPR (both opsels 0).  Lane-to-k mapping, with kq = l >> 4 and both operands' row l & 15: the scale
// of lane l on either side is that of the k 32 kq .. 32 kq + 31 of the MFMA's 128; the FP4 operand of lane l is
// those same 32 k, in memory order (ascending bytes, low nibble first), so on the weight side one lane is one MX
// block.  The FP8 operand is not: its dwords 0-3 are k 16 kq .. + 15 and its dwords 4-7 k 64 + 16 kq .. + 15 (the
// layout of two 16x16x64 steps), so a lane's 32 bytes come from the blocks kq >> 1 and 2 + (kq >> 1) of the unit
// while its scale byte is block kq's.  The operand-layout test (tests/test_skinny_mxfp4_a8_gpu.py) is the proof: 32
// consecutive bytes per lane fail it at every k >= 16 of a block.  So the work split, the unit of 128,
// the weight side (Mxfp4Mfma's at / has_block / preset / load: one non-temporal 16-B load and one scale byte per lane
// and unit) and the accumulator layout are the MXFP4 kernel's; the activation side is two 16-B loads at default
// policy, 64 bytes apart, and one scale byte of xq row m0 + (l & 15); one scaled MFMA per unit, weight tile and M
// tile replaces four bf16 MFMAs and 16 conversions, and no conversion touches either operand.  Where K cuts a unit
// short, what lies past K is code 0 (+0 in both formats) with scale byte 127, on both sides: exact zeros.  FP4 x FP8
// products times powers of two are exact in f32; the summation order of output (m, n) is: inside an MFMA the
// hardware's, units ascending within a wave, waves ascending.  It depends on K alone, so row m of a batched call
// equals the single-row call bit for bit, as in the other formats (and so does the quantiser: a lane's block
// depends on no other).  Reduction and epilogue are the text of skinny_mfma_kernel's, repeated: called as one
// device function from both kernels it changed the register allocation of the existing instantiations.
// kUnroll = 2 (-DDTG_MXFP4_A8_UNROLL=n builds others): level with 1 and ahead of 4, and where the op wins and loses,
// in profiles/r9/skinny_mxfp4_a8/README.md.
#include "mlp_act.h"
#include "skinny_common.h"

namespace dtg {

namespace {

constexpr int kMfmaMaxM = 64;
constexpr int kWaves = 8;  // waves of a workgroup; they split K
constexpr int kTile = 16;  // output columns of a workgroup, rows of x per MFMA
#ifndef DTG_MXFP4_UNROLL
#define DTG_MXFP4_UNROLL 2
#endif
#ifndef DTG_MXFP4_A8_UNROLL
#define DTG_MXFP4_A8_UNROLL 2
#endif

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

struct Bf16Mfma {
  static constexpr int kUnit = 32;     // K elements of one loop step
  static constexpr int kMfmas = 1;     // kUnit / 32
  static constexpr int kUnroll = 8;    // units per pass: weight loads in flight per wave and tile
  static constexpr bool kCut = false;  // K % kUnit != 0 is refused
  struct Ptrs {                        // the weight side's kernel arguments, or a lane's place in a weight row
    const uint16_t* w;
  };
  using Held = bf16x8;  // what a lane holds of a unit between the load and the MFMAs
  static __device__ __forceinline__ Ptrs at(const Ptrs& a, int64_t r, int64_t K, int64_t, int kq) {
    return {a.w + r * K + 8 * kq};
  }
  // whether lane group kq has its quarter of unit s: always, K % 32 == 0 is the unit
  static __device__ __forceinline__ bool has_block(int64_t, int, int64_t) { return true; }
  static __device__ __forceinline__ void preset(Held&) {}  // no MFMA runs without its load
  static __device__ __forceinline__ Held load(const Ptrs& p, int64_t s) {
    return __builtin_bit_cast(bf16x8, __builtin_nontemporal_load(reinterpret_cast<const u16x8*>(p.w + s * kUnit)));
  }
  static __device__ __forceinline__ bf16x8 frag(const Held& h, int) { return h; }
};

struct Mxfp4Mfma {
  static constexpr int kUnit = 128;  // the four blocks of the four lane groups
  static constexpr int kMfmas = 4;
  static constexpr int kUnroll = DTG_MXFP4_UNROLL;
  static constexpr bool kCut = true;  // K % 128 != 0 cuts the last unit short
  static constexpr int kBlock = 32;   // elements of one MX block: one scale byte, one 16-B load, the K of one MFMA
  struct Ptrs {
    const uint8_t* wq;
    const uint8_t* scales;
  };
  struct Held {
    u32x4 v;
    uint32_t sc;
  };
  static __device__ __forceinline__ Ptrs at(const Ptrs& a, int64_t r, int64_t K, int64_t blocks, int kq) {
    return {a.wq + r * (K / 2) + (kBlock / 2) * kq, a.scales + r * blocks + kq};
  }
  // whether lane group kq has a block in unit s; then the unit exists
  static __device__ __forceinline__ bool has_block(int64_t s, int kq, int64_t blocks) { return 4 * s + kq < blocks; }
  // what a lane without a block holds: the code of +0, scale 2^0
  static __device__ __forceinline__ void preset(Held& h) { h = {u32x4{0u, 0u, 0u, 0u}, 127u}; }
  static __device__ __forceinline__ Held load(const Ptrs& p, int64_t s) {
    return {__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.wq + s * (kUnit / 2))), p.scales[4 * s]};
  }
  // The 8 codes of dword i (elements 2 b, 2 b + 1 in byte b, low nibble first) times the scale, as bf16.  The
  // byte select of the conversion must be a literal.
  static __device__ __forceinline__ bf16x8 frag(const Held& h, int i) {
    const uint32_t d = h.v[i];
    const float scale = __uint_as_float(h.sc << 23);
    const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0);
    const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1);
    const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2);
    const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3);
    return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
  }
};

// W...: the element types of the format's weight-side pointers, so that every format keeps its own argument list.
template <class Fmt, int MT, int ACT, class... W>
__global__ __launch_bounds__(kWaves * kWave) void skinny_mfma_kernel(
    const uint16_t* __restrict__ x, int64_t x_stride, const W* __restrict__... w, const uint16_t* __restrict__ bias,
    uint16_t* __restrict__ y, int M, int64_t N, int64_t K) {
  constexpr int NW = ACT ? 2 : 1;  // weight tiles of the workgroup: plain | gate, up
  constexpr int kUnit = Fmt::kUnit, kUnroll = Fmt::kUnroll;
  __shared__ f32x4 part[kWaves][NW * MT][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = lane & 15, kq = lane >> 4;
  const int64_t n_out = ACT ? N / 2 : N;
  const int64_t n0 = (int64_t)blockIdx.x * kTile;
  const int64_t blocks = K / 32;  // 32-element blocks of a row: the K of one MFMA, one MX block

  // this lane's operand rows at its quarter of unit 0, clamped into the matrices
  const int64_t c = n0 + row < n_out ? n0 + row : n_out - 1;
  typename Fmt::Ptrs wp[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) wp[j] = Fmt::at({w...}, j * n_out + c, K, blocks, kq);
  const uint16_t* xp[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = kTile * t + row;
    xp[t] = x + (int64_t)(m < M ? m : M - 1) * x_stride + kq * (kUnit / 4);
  }

  f32x4 acc[NW][MT];
#pragma unroll
  for (int j = 0; j < NW; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // all units, and those that K does not cut short
  const int64_t units = Fmt::kCut ? (K + kUnit - 1) / kUnit : K / kUnit, whole = K / kUnit;
  // One pass: units s0, s0 + kWaves, ..., s0 + (kUnroll - 1) * kWaves; FULL = all of them exist and none is cut
  // short by K.
  auto pass = [&](int64_t s0, auto full) {
    constexpr bool FULL = decltype(full)::value;
    typename Fmt::Held wv[kUnroll][NW];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t s = s0 + u * kWaves;
#pragma unroll
      for (int j = 0; j < NW; ++j) Fmt::preset(wv[u][j]);
      // where K can cut a unit short, a lane's block exists only in a unit that exists
      if (FULL || (Fmt::kCut ? Fmt::has_block(s, kq, blocks) : s < units)) {
#pragma unroll
        for (int j = 0; j < NW; ++j) wv[u][j] = Fmt::load(wp[j], s);
      }
    }
    // keep the pass's weight loads ahead of its first conversion or MFMA: left alone, the scheduler sinks them
    // between the MFMAs to save registers and two are in flight instead of kUnroll
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t s = s0 + u * kWaves;
      if (FULL || s < units) {
        const bool mine = FULL || Fmt::has_block(s, kq, blocks);
#pragma unroll
        for (int i = 0; i < Fmt::kMfmas; ++i) {
          bf16x8 wf[NW];
#pragma unroll
          for (int j = 0; j < NW; ++j) wf[j] = Fmt::frag(wv[u][j], i);
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            bf16x8 xf = __builtin_bit_cast(bf16x8, u16x8{0, 0, 0, 0, 0, 0, 0, 0});
            if (mine) xf = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u16x8*>(xp[t] + s * kUnit + 8 * i));
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
  if (s0 < units) pass(s0, std::false_type{});

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

// W4A8: skinny_mfma_kernel's split with the scaled MFMA (header).  The weight side is Mxfp4Mfma's.
template <int MT, int ACT>
__global__ __launch_bounds__(kWaves * kWave) void skinny_mxfp4_a8_kernel(
    const uint8_t* __restrict__ xq, int64_t x_stride, const uint8_t* __restrict__ xs, const uint8_t* __restrict__ wq,
    const uint8_t* __restrict__ scales, const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int M, int64_t N,
    int64_t K) {
  using Fmt = Mxfp4Mfma;
  constexpr int NW = ACT ? 2 : 1;
  constexpr int kUnit = Fmt::kUnit, kBlock = Fmt::kBlock, kUnroll = DTG_MXFP4_A8_UNROLL;
  __shared__ f32x4 part[kWaves][NW * MT][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = lane & 15, kq = lane >> 4;
  const int64_t n_out = ACT ? N / 2 : N;
  const int64_t n0 = (int64_t)blockIdx.x * kTile;
  const int64_t blocks = K / kBlock;

  // this lane's operand rows at its block of unit 0, clamped into the matrices
  const int64_t c = n0 + row < n_out ? n0 + row : n_out - 1;
  Fmt::Ptrs wp[NW];
#pragma unroll
  for (int j = 0; j < NW; ++j) wp[j] = Fmt::at({wq, scales}, j * n_out + c, K, blocks, kq);
  const uint8_t* xqp[MT];
  const uint8_t* xsp[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = kTile * t + row;
    const int64_t mc = m < M ? m : M - 1;
    xqp[t] = xq + mc * x_stride + kq * (kBlock / 2);  // dwords 0-3; dwords 4-7 lie 64 bytes on
    xsp[t] = xs + mc * blocks + kq;
  }

  f32x4 acc[NW][MT];
#pragma unroll
  for (int j = 0; j < NW; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int64_t units = (K + kUnit - 1) / kUnit, whole = K / kUnit;
  // One pass, as in skinny_mfma_kernel: units s0, s0 + kWaves, ...; FULL = all of them exist and none is cut short.
  auto pass = [&](int64_t s0, auto full) {
    constexpr bool FULL = decltype(full)::value;
    Fmt::Held wv[kUnroll][NW];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t s = s0 + u * kWaves;
#pragma unroll
      for (int j = 0; j < NW; ++j) Fmt::preset(wv[u][j]);
      if (FULL || Fmt::has_block(s, kq, blocks)) {
#pragma unroll
        for (int j = 0; j < NW; ++j) wv[u][j] = Fmt::load(wp[j], s);
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // the pass's weight loads stay ahead of its first MFMA
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t s = s0 + u * kWaves;
      if (FULL || s < units) {
        // this lane's scale, and the two blocks its halves of the FP8 operand lie in
        const bool mine = FULL || Fmt::has_block(s, kq, blocks);
        const bool has_lo = FULL || Fmt::has_block(s, kq >> 1, blocks), has_hi = FULL || Fmt::has_block(s, 2 + (kq >> 1), blocks);
        i32x8 wf[NW];  // the four dwords of codes; with cbsz = 4 the MFMA reads no more
#pragma unroll
        for (int j = 0; j < NW; ++j) {
          const u32x4 v = wv[u][j].v;
          wf[j] = i32x8{(int)v[0], (int)v[1], (int)v[2], (int)v[3], 0, 0, 0, 0};
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          u32x4 lo = {0u, 0u, 0u, 0u}, hi = {0u, 0u, 0u, 0u};
          uint32_t xsc = 127u;
          if (has_lo) lo = *reinterpret_cast<const u32x4*>(xqp[t] + s * kUnit);
          if (has_hi) hi = *reinterpret_cast<const u32x4*>(xqp[t] + s * kUnit + kUnit / 2);
          if (mine) xsc = xsp[t][4 * s];
          const i32x8 xf = {(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
#pragma unroll
          for (int j = 0; j < NW; ++j)
            acc[j][t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[j], xf, acc[j][t], /*cbsz=*/4, /*blgp=*/0, 0,
                                                                         (int)wv[u][j].sc, 0, (int)xsc);
        }
      }
    }
  };
  int64_t s0 = wave;
  for (; s0 + (kUnroll - 1) * kWaves < whole; s0 += kUnroll * kWaves) pass(s0, std::true_type{});
  if (s0 < units) pass(s0, std::false_type{});

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

// quantize_mxfp8_rows: one lane owns one block of 32 consecutive elements of a row of x (bf16): four 16-B loads,
// the amax in the lane, the scale from amax's f32 bits as kv_append_kernel (decode_attn.hip) does it -- the power of
// two 2^k that puts amax into (224, 448]: a significand up to 1.75 = 448 / 256 goes to [256, 448] with k = E - 135, a
// larger one to (224, 256) with k = E - 134; k floored at -100, 0 for an all-zero block -- then x * 2^-k (exact: a bf16
// value times a power of two), clamped to +-448 by comparisons and rounded to nearest even by v_cvt_pk_fp8_f32, which
// that kernel's tests hold to torch's cast bit for bit, subnormal codes included: ops.quantize_fp8_rows(pow2 = True)
// of the block.  (v_cvt_scalef32_pk_fp8_bf16 would fold the multiply and skip the widening; it has not been held
// against the rule and is not used.)  Two 16-B stores of codes and one byte k + 127, in [27, 246].  Finite input is
// the contract, as for the torch rule; a NaN passes the comparisons and stays a NaN code.
constexpr int kQuantThreads = 256;
constexpr int kMinScaleExp = -100;  // ops.FP8_MIN_SCALE_EXP

__global__ __launch_bounds__(kQuantThreads) void quantize_mxfp8_rows_kernel(const uint16_t* __restrict__ x,
                                                                           int64_t x_stride, uint8_t* __restrict__ xq,
                                                                           uint8_t* __restrict__ xs, int64_t blocks,
                                                                           int64_t total) {
  const int64_t gid = (int64_t)blockIdx.x * kQuantThreads + threadIdx.x;  // block gid % blocks of row gid / blocks
  if (gid >= total) return;
  const uint16_t* src = x + (gid / blocks) * x_stride + (gid % blocks) * Mxfp4Mfma::kBlock;
  float v[32];
#pragma unroll
  for (int i = 0; i < 4; ++i) load8(src + 8 * i, v + 8 * i);
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) amax = fmaxf(amax, fabsf(v[i]));
  const uint32_t ab = __float_as_uint(amax);
  int k = (int)(ab >> 23) - ((ab & 0x7fffffu) <= 0x600000u ? 135 : 134);
  k = k < kMinScaleExp ? kMinScaleExp : k;
  if (amax == 0.f) k = 0;
  const float inv = __uint_as_float((uint32_t)(127 - k) << 23);
  u32x4 out[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float f = v[4 * i + j] * inv;
      q[j] = f > 448.f ? 448.f : (f < -448.f ? -448.f : f);
    }
    int d = 0;
    d = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], d, false);
    d = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], d, true);
    out[i >> 2][i & 3] = (uint32_t)d;
  }
  u32x4* dst = reinterpret_cast<u32x4*>(xq + gid * Mxfp4Mfma::kBlock);  // xq is contiguous: row * K + 32 * block
  dst[0] = out[0], dst[1] = out[1];
  xs[gid] = (uint8_t)(k + 127);
}

// The shared checks with this kernel's limits: up to 64 rows, K in whole MFMAs, 16 output columns per workgroup.
skinny::Plan mfma_plan(const char* name, const char* w_layout, int w_per_elem, const at::Tensor& x,
                       const at::Tensor& w, const c10::optional<at::Tensor>& bias, int64_t act,
                       const char* bias_msg = nullptr, bool x_bf16 = true) {
  return skinny::plan(name, w_layout, kMfmaMaxM, 32, w_per_elem, kTile, x, w, bias, act, bias_msg, x_bf16);
}

struct Mxfp4A8 {};  // not a weight format of skinny_mfma_kernel: skinny_mxfp4_a8_kernel, x = xq and w... = xs, wq, scales

// Launches the instantiation for ceil(p.M / 16) M tiles: MT counts down from the largest.
template <class Fmt, int ACT, int MT = kMfmaMaxM / kTile, class... W>
void mfma_launch(const skinny::Plan& p, const at::Tensor& x, at::Tensor& y, const W*... w) {
  if constexpr (MT >= 1) {
    if ((p.M + kTile - 1) / kTile != MT) return mfma_launch<Fmt, ACT, MT - 1>(p, x, y, w...);
    if constexpr (std::is_same_v<Fmt, Mxfp4A8>)
      skinny_mxfp4_a8_kernel<MT, ACT><<<p.grid, kWaves * kWave, 0, stream()>>>(
          static_cast<const uint8_t*>(x.data_ptr()), x.stride(0), w..., p.bias, bf16_mut(y), (int)p.M, p.N, p.K);
    else
      skinny_mfma_kernel<Fmt, MT, ACT, W...><<<p.grid, kWaves * kWave, 0, stream()>>>(
          bf16_ptr(x), x.stride(0), w..., p.bias, bf16_mut(y), (int)p.M, p.N, p.K);
  }
}

template <class Fmt, class... W>
at::Tensor mfma_run(const skinny::Plan& p, const at::Tensor& x, int64_t act, const W*... w) {
  const c10::DeviceGuard g(x.device());
  auto y = at::empty({p.M, act ? p.N / 2 : p.N}, x.options().dtype(at::kBFloat16));
  if (act)
    mfma_launch<Fmt, 1>(p, x, y, w...);
  else
    mfma_launch<Fmt, 0>(p, x, y, w...);
  DTG_LAUNCH_CHECK();
  return y;
}

}  // namespace

at::Tensor skinny_linear_mfma(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias,
                              int64_t act) {
  DTG_CHECK_CUDA_BF16(x);  // ahead of w, as this operator always has
  DTG_CHECK_CUDA_BF16(w);
  const auto p = mfma_plan("skinny_linear_mfma", ": w must be a contiguous 16-B aligned [N, K] on x's device", 1, x, w,
                           bias, act);
  return mfma_run<Bf16Mfma>(p, x, act, bf16_ptr(w));
}

at::Tensor skinny_linear_mxfp4(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& scales,
                               const c10::optional<at::Tensor>& bias, int64_t act) {
  const char* name = "skinny_linear_mxfp4";
  DTG_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16, name, ": x must be a bf16 GPU tensor");
  DTG_CHECK(wq.is_cuda() && wq.scalar_type() == at::kByte && scales.is_cuda() && scales.scalar_type() == at::kByte,
            name, ": wq and scales must be uint8 GPU tensors");
  const auto p = mfma_plan(name, ": wq must be a contiguous 16-B aligned uint8 [N, K / 2] on x's device", 2, x, wq,
                           bias, act, ": bias must be a contiguous bf16 [N] on x's device");
  DTG_CHECK(scales.dim() == 2 && scales.size(0) == p.N && scales.size(1) == p.K / Mxfp4Mfma::kBlock &&
                scales.is_contiguous() && scales.device() == x.device(),
            name, ": scales must be a contiguous uint8 [N, K / 32] on x's device");
  return mfma_run<Mxfp4Mfma>(p, x, act, wq.data_ptr<uint8_t>(), scales.data_ptr<uint8_t>());
}

at::Tensor skinny_linear_mxfp4_a8(const at::Tensor& xq, const at::Tensor& xs, const at::Tensor& wq,
                                  const at::Tensor& scales, const c10::optional<at::Tensor>& bias, int64_t act) {
  const char* name = "skinny_linear_mxfp4_a8";
  DTG_CHECK(xq.is_cuda() && xq.scalar_type() == at::kFloat8_e4m3fn && xs.is_cuda() && xs.scalar_type() == at::kByte, name,
            ": xq must be a float8_e4m3fn and xs a uint8 GPU tensor");
  DTG_CHECK(wq.is_cuda() && wq.scalar_type() == at::kByte && scales.is_cuda() && scales.scalar_type() == at::kByte,
            name, ": wq and scales must be uint8 GPU tensors");
  const auto p = mfma_plan(name, ": wq must be a contiguous 16-B aligned uint8 [N, K / 2] on xq's device", 2, xq, wq,
                           bias, act, ": bias must be a contiguous bf16 [N] on xq's device", /*x_bf16=*/false);
  DTG_CHECK(xs.dim() == 2 && xs.size(0) == p.M && xs.size(1) == p.K / Mxfp4Mfma::kBlock && xs.is_contiguous() &&
                xs.device() == xq.device(),
            name, ": xs must be a contiguous uint8 [M, K / 32] on xq's device");
  DTG_CHECK(scales.dim() == 2 && scales.size(0) == p.N && scales.size(1) == p.K / Mxfp4Mfma::kBlock &&
                scales.is_contiguous() && scales.device() == xq.device(),
            name, ": scales must be a contiguous uint8 [N, K / 32] on xq's device");
  return mfma_run<Mxfp4A8>(p, xq, act, xs.data_ptr<uint8_t>(), wq.data_ptr<uint8_t>(), scales.data_ptr<uint8_t>());
}

std::tuple<at::Tensor, at::Tensor> quantize_mxfp8_rows(const at::Tensor& x) {
  const char* name = "quantize_mxfp8_rows";
  DTG_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16, name, ": x must be a bf16 GPU tensor");
  DTG_CHECK(x.dim() == 2 && x.size(1) % Mxfp4Mfma::kBlock == 0, name, ": x must be [M, K] with K a multiple of 32");
  DTG_CHECK(x.stride(1) == 1 && x.stride(0) % 8 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, name,
            ": x must have unit inner stride and 16-B aligned rows");
  const c10::DeviceGuard g(x.device());
  const int64_t M = x.size(0), blocks = x.size(1) / Mxfp4Mfma::kBlock, total = M * blocks;
  auto xq = at::empty({M, x.size(1)}, x.options().dtype(at::kFloat8_e4m3fn));
  auto xs = at::empty({M, blocks}, x.options().dtype(at::kByte));
  const int64_t nwg = (total + kQuantThreads - 1) / kQuantThreads;
  DTG_CHECK(nwg < (int64_t(1) << 31), name, ": too many workgroups");
  if (total > 0) {
    quantize_mxfp8_rows_kernel<<<(unsigned)nwg, kQuantThreads, 0, stream()>>>(
        bf16_ptr(x), x.stride(0), static_cast<uint8_t*>(xq.data_ptr()), xs.data_ptr<uint8_t>(), blocks, total);
    DTG_LAUNCH_CHECK();
  }
  return {xq, xs};
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) {
  m.impl("skinny_linear_mfma", &skinny_linear_mfma);
  m.impl("skinny_linear_mxfp4", &skinny_linear_mxfp4);
  m.impl("skinny_linear_mxfp4_a8", &skinny_linear_mxfp4_a8);
  m.impl("quantize_mxfp8_rows", &quantize_mxfp8_rows);
}

}  // namespace dtg
