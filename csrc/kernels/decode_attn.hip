// KV-cache generation kernels: the cache append (RoPE + scatter of k / v) and the split-KV decode
// attention of one query token per sequence against its cache row.
//
// Cache layout: one K and one V tensor per layer, bf16 [rows_max, nkv, S_max, D], head-major: the
// keys of one kv head are contiguous along the sequence, so a workgroup streams its chunk linearly.
//
// kv_cache_append_: per token t of the fused projection output qkv [T, (nq + 2 nkv) D], rotates the
// q and k heads in place at pos[t] with the pairing (i, i + D/2), operation order (rope_common.h) and
// single rounding of rope_ (the roped bits equal rope_'s), then copies the roped k and the v heads to
// cache[rows[t], :, pos[t], :].  Empty tables = already roped (Qwen3 ropes in qk_norm_rope_fwd_):
// copy only.  A token whose pos / rows lie outside the cache (or, when roping, whose pos lies past
// the tables) is skipped entirely.  Thread mapping as rope_common.h: one thread per (token, head,
// 8-pair group), two 16-B accesses each way.
//
// decode_attn: grid (sequence, kv head, split), launched flattened.  A workgroup (4 waves) serves all
// G = nq / nkv query heads of its kv head over its chunk of keys, so K and V are read once per
// group.  QK and PV run on the VALU in f32 (the kernel is bound by the K / V stream; P is NOT
// rounded to bf16).  K / V go straight to VGPRs in 16-B pieces: a key is D/8 lanes, a lane keeps
// its 8 dims of q (pre-scaled) and of the G output accumulators, the score is a sub-wave
// butterfly.  Each lane group carries its own online-softmax state over the keys it sees; the
// groups of a wave are merged by shuffles, the 4 waves through LDS, in a fixed order.  With one
// split the workgroup normalises and writes bf16 itself; otherwise it writes the f32 partial
// (max, sum, unnormalised output) and decode_combine_kernel merges the splits in index order.
// No atomics, no arrival counters: bitwise reproducible.  A split without keys for its row leaves
// max = -inf, sum = 0; every exp(m - m_new) is guarded by m == -inf, so the empty partial
// contributes 0 instead of exp(-inf + inf) = NaN.  Keys outside the attended range are never
// loaded (the cache may hold anything there, NaN included).
//
// decode_attn_multi: Q new tokens per sequence (speculative verification), one attended length per token.
// The same kernel template with a query tile: grid (sequence x query tile, kv head, split), a workgroup
// serves decode::q_tile(G) consecutive tokens times the G heads, so a K / V piece is loaded once for up
// to 16 (token, head) pairs.  Partials and output are indexed with the token in the place of the
// sequence, so decode_combine_kernel serves unchanged.  At window 0 a token's output row is, bit for bit,
// decode_attn's for that token alone with the same max_len and splits.  Keys past the largest length of
// a tile's tokens are never loaded; keys between its tokens' ranges are (they score -inf).
//
// Cache formats (the template parameter Fmt of the append and of the attention, the way skinny_gemm.hip
// takes a weight format).  Bf16Cache: everything above.  E4m3Cache (kv_cache_append_fp8_, decode_attn_fp8):
// K / V are OCP e4m3fn bytes in the same [rows_max, nkv, S_max, D] layout, with one f32 scale per key vector,
// [rows_max, nkv, S_max], for K and for V.  The scale is the power of two that puts the vector's largest
// magnitude into (224, 448] (1 for an all-zero vector, floored at 2^-100): ops.quantize_fp8_rows(pow2=True)
// of the D-vector, bit for bit.  The append takes amax over the head's D/16 lanes with a sub-wave butterfly
// (all lanes of a head belong to one token and return together), builds the scale from amax's exponent bits,
// divides exactly, clamps to +-448 (a NaN stays NaN: code 0x7f), converts with v_cvt_pk_fp8_f32 (round to
// nearest even), stores two 8-byte pieces of codes per thread and the scale from the group's first lane,
// and writes the DEQUANTISED k / v back into qkv, so a prefill that attends qkv sees what the cache holds.
// code * scale is exactly a bf16 value: the FP8 cache is exactly some bf16 cache.  The attention keeps the
// lane map (a lane loads 8 bytes per key and tensor instead of 16), widens with v_cvt_pk_f32_fp8 and
// multiplies by the key's scale (exact) before first use; from there on the arithmetic is the bf16
// kernel's, expression for expression, so decode_attn_fp8(codes, scales) equals decode_attn(dequantised
// cache) bit for bit (for scales whose products stay in the normal f32 range).  A key's scale is loaded
// only where the key is.  Plan, partial workspace and combine kernel are shared.
#include "decode_attn_plan.h"
#include "rope_common.h"

#include <ATen/hip/HIPContext.h>

namespace dtg {

namespace {

// exp(m - m_new) of a running max that may still be -inf (nothing seen): weight 0, never NaN
__device__ __forceinline__ float rescale(float m, float m_new) { return m == -INFINITY ? 0.f : __expf(m - m_new); }

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kFp8MinScaleExp = -100;  // ops.FP8_MIN_SCALE_EXP

struct NoScale {};  // an empty kernel argument: the bf16 kernels carry no scale pointers

// A cache format: the element type, the scale arguments of the kernels, and a lane's 8 dims of one key
// (Piece) with its load and its widening to f32.
struct Bf16Cache {
  static constexpr bool kFp8 = false;
  using Elem = uint16_t;
  using Scale = NoScale;     // read by the attention
  using ScaleOut = NoScale;  // written by the append
  using Piece = u16x8;
  static __device__ __forceinline__ Scale at(Scale s, int64_t) { return s; }
  static __device__ __forceinline__ Piece zero() { return u16x8{0, 0, 0, 0, 0, 0, 0, 0}; }
  static __device__ __forceinline__ Piece load(const Elem* p, Scale, int64_t) {
    return *reinterpret_cast<const u16x8*>(p);
  }
  static __device__ __forceinline__ void widen(const Piece& v, float* out) { widen8(v, out); }
};

struct E4m3Cache {
  static constexpr bool kFp8 = true;
  using Elem = uint8_t;
  using Scale = const float*;
  using ScaleOut = float*;
  struct Piece {
    uint2 v;
    float s;
  };
  static __device__ __forceinline__ Scale at(Scale s, int64_t off) { return s + off; }
  static __device__ __forceinline__ Piece zero() { return Piece{make_uint2(0u, 0u), 1.f}; }
  // `s` points at the scales of the kv head's row, j is the key
  static __device__ __forceinline__ Piece load(const Elem* p, Scale s, int64_t j) {
    return Piece{*reinterpret_cast<const uint2*>(p), s[j]};
  }
  // eight e4m3 bytes (memory order = ascending byte) through v_cvt_pk_f32_fp8
  static __device__ __forceinline__ void codes(uint2 v, float* out) {
    const uint32_t w[2] = {v.x, v.y};
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], false);
      const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], true);
      out[4 * d] = lo[0];
      out[4 * d + 1] = lo[1];
      out[4 * d + 2] = hi[0];
      out[4 * d + 3] = hi[1];
    }
  }
  // code * 2^k is exact: the values are those of the bf16 cache this one stands for
  static __device__ __forceinline__ void widen(const Piece& p, float* out) {
    codes(p.v, out);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] *= p.s;
  }
};

// The e4m3 codes of 8 values already divided by the scale: clamped to +-448 by comparisons, which a NaN
// passes (it becomes the code 0x7f), rounded to nearest even by v_cvt_pk_fp8_f32.
__device__ __forceinline__ uint2 e4m3_pack8(const float* x) {
  float c[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) c[i] = x[i] > 448.f ? 448.f : (x[i] < -448.f ? -448.f : x[i]);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(c[4], c[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(c[6], c[7], hi, true);
  return make_uint2((uint32_t)lo, (uint32_t)hi);
}

template <class Fmt, int D, bool ROPE>
__global__ __launch_bounds__(256) void kv_append_kernel(
    uint16_t* __restrict__ qkv, int64_t row_stride, typename Fmt::Elem* __restrict__ kc,
    typename Fmt::Elem* __restrict__ vc, typename Fmt::ScaleOut ksc, typename Fmt::ScaleOut vsc,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t, int64_t max_pos,
    const int64_t* __restrict__ pos, const int32_t* __restrict__ rows, int nq, int nkv, int64_t T, int64_t rows_max,
    int64_t S_max) {
  constexpr int HALF = D / 2;
  const int nh = nq + 2 * nkv;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= rope::items(T, nh, D)) return;
  const rope::Item<D> it(gid, nh);
  const int64_t p = pos[it.tok];
  const int64_t r = rows[it.tok];
  if (p < 0 || p >= S_max || r < 0 || r >= rows_max) return;
  if (ROPE && p >= max_pos) return;
  uint16_t* base = it.in(qkv, row_stride);
  u16x8 b1 = *reinterpret_cast<const u16x8*>(base);
  u16x8 b2 = *reinterpret_cast<const u16x8*>(base + HALF);
  if (ROPE && it.head < nq + nkv) {
    float x1[8], x2[8], c[8], s[8];
    widen8(b1, x1);
    widen8(b2, x2);
    rope::load_cs<D>(cos_t, sin_t, p, it.grp, c, s);
    rope::rotate(x1, x2, c, s, x1, x2);  // rope_kernel's call: the same bits
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      b1[j] = f2bf(x1[j]);
      b2[j] = f2bf(x2[j]);
    }
    if (!Fmt::kFp8 || it.head < nq) {  // the FP8 form stores a k head once, dequantised, below
      *reinterpret_cast<u16x8*>(base) = b1;
      *reinterpret_cast<u16x8*>(base + HALF) = b2;
    }
  }
  if (it.head >= nq) {
    const bool is_k = it.head < nq + nkv;
    const int kvh = is_k ? it.head - nq : it.head - nq - nkv;
    const int64_t slot = (r * nkv + kvh) * S_max + p;
    if constexpr (Fmt::kFp8) {
      // The head's D/16 lanes are consecutive, aligned, and all here: they share the token, so they passed
      // the early returns together, and the head, so they took this branch together.
      float x1[8], x2[8];
      widen8(b1, x1);
      widen8(b2, x2);
      float amax = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fmaxf(fabsf(x1[j]), fabsf(x2[j])));
#pragma unroll
      for (int o = D / 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, kWave));
      // amax = (1 + f) 2^(E - 127): a significand up to 1.75 (= 448 / 256) goes to [256, 448] with the scale
      // 2^(E - 135), a larger one to (224, 256) with 2^(E - 134); subnormals end at the floor
      const uint32_t ab = __float_as_uint(amax);
      const int E = (int)(ab >> 23);
      int k = E - ((ab & 0x7fffffu) <= 0x600000u ? 135 : 134);
      k = k < kFp8MinScaleExp ? kFp8MinScaleExp : k;
      if (amax == 0.f) k = 0;
      const float sc = __uint_as_float((uint32_t)(k + 127) << 23);
      const float inv = __uint_as_float((uint32_t)(127 - k) << 23);  // exact: the product is the quotient
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x1[j] *= inv;
        x2[j] *= inv;
      }
      const uint2 c1 = e4m3_pack8(x1), c2 = e4m3_pack8(x2);
      uint8_t* dst = (is_k ? kc : vc) + slot * D + it.grp * 8;
      *reinterpret_cast<uint2*>(dst) = c1;
      *reinterpret_cast<uint2*>(dst + HALF) = c2;
      if (it.grp == 0) (is_k ? ksc : vsc)[slot] = sc;
      // what the cache now holds goes back into qkv, for the prefill's attention
      E4m3Cache::widen(E4m3Cache::Piece{c1, sc}, x1);
      E4m3Cache::widen(E4m3Cache::Piece{c2, sc}, x2);
      store8(base, x1);
      store8(base + HALF, x2);
    } else {
      uint16_t* dst = (is_k ? kc : vc) + slot * D + it.grp * 8;
      *reinterpret_cast<u16x8*>(dst) = b1;
      *reinterpret_cast<u16x8*>(dst + HALF) = b2;
    }
  }
}

// QT = 1 is decode_attn; QT > 1 serves decode_attn_multi: a tile of QT consecutive tokens of sequence b
// (tokens t0 .. t0 + QT - 1 of its Q, row b * Q + t of qkv / lens) shares the workgroup's K / V stream.
// The QT * G (token, head) pairs are laid out as the G heads of the one-token form; a pair's arithmetic
// is that form's, expression for expression.  The key loop starts at the smallest k0 of the tile's
// tokens that hold keys in this split (all equal split * chunk without a window, so key j sits in the
// same lane whatever the query) and runs to their largest k1; a key outside a token's own [k0, k1)
// scores -inf for it, which leaves its (m, l, acc) as they were: alpha = exp(m - m) = 1, p = 0.
template <class Fmt, int D, int G, int QT>
__global__ __launch_bounds__(decode::kThreads) void decode_attn_kernel(
    const uint16_t* __restrict__ qkv, int64_t q_stride, const typename Fmt::Elem* __restrict__ kc,
    const typename Fmt::Elem* __restrict__ vc, const int32_t* __restrict__ rows, const int32_t* __restrict__ lens,
    float* __restrict__ ws_o, float* __restrict__ ws_ml, uint16_t* __restrict__ out, int nkv, int splits,
    int64_t chunk, int64_t window, int64_t rows_max, int64_t S_max, float scale, int Q, typename Fmt::Scale ksc,
    typename Fmt::Scale vsc) {
  // Every multiply-add below is written out (fmaf, or a product and a sum that stay apart): left to the
  // compiler, which products fuse with which sums differed from element to element and from one
  // instantiation to the next, and the bits of the QT > 1 forms would not be those of QT = 1.
#pragma clang fp contract(off)
  constexpr int LPK = D / 8;                      // lanes per key
  constexpr int KPW = kWave / LPK;                // keys per wave per load
  constexpr int NW = decode::kThreads / kWave;    // waves
  constexpr int KSTEP = NW * KPW;                 // keys per workgroup per load
  constexpr int UN = decode::kKeyTile / KSTEP;    // loads in flight per lane and tensor
  constexpr int H = QT * G;                       // (token, head) pairs of the workgroup
  static_assert(UN >= 1 && UN * KSTEP == decode::kKeyTile, "key tile");
  static_assert(H <= decode::kMaxPairs, "register budget");
  __shared__ float sm_o[NW][H][D];
  __shared__ float sm_m[NW][H], sm_l[NW][H];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = lane / LPK, li = lane % LPK;
  const int split = blockIdx.x % splits;
  const int h = (blockIdx.x / splits) % nkv;
  const int64_t z = blockIdx.x / ((int64_t)splits * nkv);
  const int qtiles = (Q + QT - 1) / QT;
  const int64_t b = z / qtiles;
  const int t0 = (int)(z % qtiles) * QT;
  const int64_t row = rows[b];
  // per token: its attended keys of this split, [tk0, tk1); the workgroup walks [k0, k1), their hull
  int64_t tk0[QT], tk1[QT], k0 = S_max, k1 = 0;
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    int64_t len = t0 + t < Q ? lens[b * Q + t0 + t] : 0;
    if (row < 0 || row >= rows_max || len < 0) len = 0;
    if (len > S_max) len = S_max;
    const int64_t lo = window > 0 && len > window ? len - window : 0;
    tk0[t] = lo > split * chunk ? lo : split * chunk;
    // the last split runs to the end of the row even if max_len understated it: slow, never wrong
    tk1[t] = split == splits - 1 || len < (split + 1) * chunk ? len : (split + 1) * chunk;
    if (tk1[t] > tk0[t]) {
      k0 = tk0[t] < k0 ? tk0[t] : k0;
      k1 = tk1[t] > k1 ? tk1[t] : k1;
    }
  }

  float q[H][8], acc[H][8], m[H], l[H];
#pragma unroll
  for (int x = 0; x < H; ++x) {
    const int t = x / G, g = x % G;
    if (QT == 1 || t0 + t < Q) {
      load8(qkv + (b * Q + t0 + t) * q_stride + ((int64_t)h * G + g) * D + li * 8, q[x]);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) q[x][i] = 0.f;
    }
    m[x] = -INFINITY;
    l[x] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      q[x][i] *= scale;
      acc[x][i] = 0.f;
    }
  }

  const int64_t head_off = ((k1 > k0 ? row : 0) * nkv + h) * S_max * D + li * 8;
  const typename Fmt::Elem* kb = kc + head_off;
  const typename Fmt::Elem* vb = vc + head_off;
  // the head's scales: its offset in keys
  const typename Fmt::Scale ksb = Fmt::at(ksc, head_off / D), vsb = Fmt::at(vsc, head_off / D);
  for (int64_t j0 = k0; j0 < k1; j0 += decode::kKeyTile) {
    typename Fmt::Piece kr[UN], vr[UN];
    unsigned ok[UN];  // bit t: token t of the tile attends the key
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t j = j0 + u * KSTEP + wave * KPW + sub;
      ok[u] = 0;
#pragma unroll
      for (int t = 0; t < QT; ++t) ok[u] |= (unsigned)(j >= tk0[t] && j < tk1[t]) << t;
      kr[u] = Fmt::zero();
      vr[u] = kr[u];
      if (QT == 1 ? ok[u] != 0 : j < k1) {  // the hull: a key between two tokens' ranges is loaded
        kr[u] = Fmt::load(kb + j * D, ksb, j);
        vr[u] = Fmt::load(vb + j * D, vsb, j);
      }
    }
    float sc[UN][H];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      float kf[8];
      if constexpr (Fmt::kFp8) {
        Fmt::widen(kr[u], kf);
      } else {  // written out: through widen() the 16 x 128 instantiations of the bf16 format spilled
#pragma unroll
        for (int i = 0; i < 8; ++i) kf[i] = bf2f(kr[u][i]);
      }
#pragma unroll
      for (int x = 0; x < H; ++x) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) d = fmaf(q[x][i], kf[i], d);
        d = lanes_sum<LPK>(d);
        sc[u][x] = (ok[u] >> (x / G)) & 1u ? d : -INFINITY;
      }
    }
    float vf[UN][8];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      if constexpr (Fmt::kFp8) {
        Fmt::widen(vr[u], vf[u]);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) vf[u][i] = bf2f(vr[u][i]);
      }
    }
#pragma unroll
    for (int x = 0; x < H; ++x) {
      float mn = m[x];
#pragma unroll
      for (int u = 0; u < UN; ++u) mn = fmaxf(mn, sc[u][x]);
      const float alpha = rescale(m[x], mn);
      float p[UN], ps = 0.f;
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        p[u] = rescale(sc[u][x], mn);
        ps += p[u];
      }
      m[x] = mn;
      l[x] = fmaf(l[x], alpha, ps);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float a = acc[x][i] * alpha;
#pragma unroll
        for (int u = 0; u < UN; ++u) a = fmaf(p[u], vf[u][i], a);
        acc[x][i] = a;
      }
    }
  }

  // merge the lane groups of the wave (butterfly over the group index), then the waves through LDS
#pragma unroll
  for (int x = 0; x < H; ++x) {
#pragma unroll
    for (int o = LPK; o < kWave; o <<= 1) {
      const float mo = __shfl_xor(m[x], o, kWave), lo_ = __shfl_xor(l[x], o, kWave);
      const float mn = fmaxf(m[x], mo);
      const float a = rescale(m[x], mn), bw = rescale(mo, mn);
      l[x] = fmaf(l[x], a, lo_ * bw);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[x][i] = fmaf(acc[x][i], a, __shfl_xor(acc[x][i], o, kWave) * bw);
      m[x] = mn;
    }
    if (sub == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) sm_o[wave][x][li * 8 + i] = acc[x][i];
      if (li == 0) {
        sm_m[wave][x] = m[x];
        sm_l[wave][x] = l[x];
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < H * D; e += decode::kThreads) {
    const int x = e / D, d = e % D, t = x / G, g = x % G;
    if (QT > 1 && t0 + t >= Q) break;  // the tile's tokens past Q (x grows with e)
    const int64_t bh = (b * Q + t0 + t) * nkv + h;
    float mn = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW; ++w) mn = fmaxf(mn, sm_m[w][x]);
    float o = 0.f, ls = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float wt = rescale(sm_m[w][x], mn);
      o = fmaf(sm_o[w][x][d], wt, o);
      ls = fmaf(sm_l[w][x], wt, ls);
    }
    if (splits == 1) {
      out[(bh * G + g) * D + d] = f2bf(ls > 0.f ? o / ls : 0.f);
    } else {
      const int64_t pi = (bh * splits + split) * G + g;
      ws_o[pi * D + d] = o;
      if (d == 0) {
        ws_ml[pi * 2] = mn;
        ws_ml[pi * 2 + 1] = ls;
      }
    }
  }
}

// One workgroup per (sequence, kv head): the partials of the splits merged in index order.
template <int D>
__global__ __launch_bounds__(decode::kThreads) void decode_combine_kernel(
    const float* __restrict__ ws_o, const float* __restrict__ ws_ml, uint16_t* __restrict__ out, int G, int splits) {
  const int64_t bh = blockIdx.x;
  for (int e = threadIdx.x; e < G * D; e += decode::kThreads) {
    const int g = e / D, d = e % D;
    float mn = -INFINITY;
    for (int s = 0; s < splits; ++s) mn = fmaxf(mn, ws_ml[((bh * splits + s) * G + g) * 2]);
    float o = 0.f, ls = 0.f;
    for (int s = 0; s < splits; ++s) {
      const int64_t pi = (bh * splits + s) * G + g;
      const float ms = ws_ml[pi * 2];
      if (ms == -INFINITY) continue;  // an empty split: nothing to add, and its output is not read
      const float wt = __expf(ms - mn);
      o += ws_o[pi * D + d] * wt;
      ls += ws_ml[pi * 2 + 1] * wt;
    }
    out[(bh * G + g) * D + d] = f2bf(ls > 0.f ? o / ls : 0.f);
  }
}

// The caches of a call and, for E4m3Cache, their scales (null for Bf16Cache).
struct Caches {
  const at::Tensor &k, &v;
  const at::Tensor *k_scale = nullptr, *v_scale = nullptr;
  template <class Fmt>
  typename Fmt::Elem* data(const at::Tensor& t) const {
    return reinterpret_cast<typename Fmt::Elem*>(t.data_ptr());
  }
  template <class Fmt>
  typename Fmt::ScaleOut scale(const at::Tensor* t) const {
    if constexpr (Fmt::kFp8) {
      return t->data_ptr<float>();
    } else {
      return NoScale{};
    }
  }
};

template <class Fmt>
void check_cache(const Caches& c, int64_t nkv, int64_t D, const char* name) {
  const at::Tensor &k_cache = c.k, &v_cache = c.v;
  if constexpr (Fmt::kFp8) {
    DTG_CHECK(k_cache.is_cuda() && v_cache.is_cuda() && k_cache.scalar_type() == at::kFloat8_e4m3fn &&
                  v_cache.scalar_type() == at::kFloat8_e4m3fn,
              name, ": caches must be float8_e4m3fn GPU tensors");
  } else {
    DTG_CHECK_CUDA_BF16(k_cache);
    DTG_CHECK_CUDA_BF16(v_cache);
  }
  DTG_CHECK(k_cache.dim() == 4 && k_cache.is_contiguous() && v_cache.is_contiguous() &&
                k_cache.sizes() == v_cache.sizes() && k_cache.size(1) == nkv && k_cache.size(3) == D,
            name, ": caches must be contiguous ", Fmt::kFp8 ? "float8_e4m3fn" : "bf16",
            " [rows_max, nkv, S_max, head_dim]");
  DTG_CHECK(k_cache.numel() < (int64_t(1) << 46), name, ": cache too large");
  if constexpr (Fmt::kFp8) {
    for (const at::Tensor* s : {c.k_scale, c.v_scale})
      DTG_CHECK(s->is_cuda() && s->scalar_type() == at::kFloat && s->is_contiguous() && s->dim() == 3 &&
                    s->sizes() == k_cache.sizes().slice(0, 3),
                name, ": scales must be contiguous f32 GPU tensors [rows_max, nkv, S_max]");
    DTG_CHECK(reinterpret_cast<uintptr_t>(k_cache.data_ptr()) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(v_cache.data_ptr()) % 8 == 0,
              name, ": caches must be 8-B aligned");
  }
}

void check_qkv(const at::Tensor& qkv, int64_t nq, int64_t nkv, int64_t D, const char* name) {
  DTG_CHECK(nq >= 1 && nkv >= 1 && nq % nkv == 0, name, ": bad head counts");
  rope::check_qkv(qkv, nq + 2 * nkv, D, name);
}

void check_index(const at::Tensor& t, int64_t n, const char* name, const char* what, const char* per = "token") {
  DTG_CHECK(t.is_cuda() && t.scalar_type() == at::kInt && t.is_contiguous() && t.numel() == n, name, ": ", what,
            " must be an int32 GPU tensor with one entry per ", per);
}

template <class Fmt>
void append_launch(const char* name, const at::Tensor& qkv, const Caches& c, const at::Tensor& cos_t,
                   const at::Tensor& sin_t, const at::Tensor& pos, const at::Tensor& rows, int64_t nq, int64_t nkv,
                   int64_t D) {
  const at::Tensor &k_cache = c.k, &v_cache = c.v;
  check_qkv(qkv, nq, nkv, D, name);
  check_cache<Fmt>(c, nkv, D, name);
  const int64_t T = qkv.size(0);
  check_index(rows, T, name, "rows");
  rope::check_pos(pos, T, name);
  const bool rope = rope::enabled(cos_t, sin_t, name);  // empty tables: the copy-only form
  const int64_t max_pos = rope ? rope::check_tables(cos_t, sin_t, D, name) : 0;
  if (T == 0) return;
  const c10::DeviceGuard g(qkv.device());
  const int64_t nblk = (rope::items(T, nq + 2 * nkv, D) + 255) / 256;
  DTG_CHECK(nblk < (int64_t(1) << 31), name, ": too many tokens");
  const float* cp = rope ? cos_t.data_ptr<float>() : nullptr;
  const float* sp = rope ? sin_t.data_ptr<float>() : nullptr;
  DTG_HD_RP_DISPATCH(D, rope, kv_append_kernel<Fmt, HD, RP><<<(unsigned)nblk, 256, 0, stream()>>>(
                                  bf16_mut(qkv), qkv.stride(0), c.data<Fmt>(k_cache), c.data<Fmt>(v_cache),
                                  c.scale<Fmt>(c.k_scale), c.scale<Fmt>(c.v_scale), cp, sp, max_pos,
                                  pos.data_ptr<int64_t>(), rows.data_ptr<int32_t>(), (int)nq, (int)nkv, T,
                                  k_cache.size(0), k_cache.size(2)));
  DTG_LAUNCH_CHECK();
}

// decode_attn (Q = 1) and decode_attn_multi: qkv holds Q tokens for each of rows.numel() sequences, lens
// one entry per token.  Q = 1 runs the one-token kernel, Q > 1 the tile of decode::q_tile(G) tokens.
template <class Fmt>
at::Tensor decode_launch(const char* name, const at::Tensor& qkv, const Caches& c, const at::Tensor& rows,
                         const at::Tensor& lens, int64_t Q, int64_t nq, int64_t nkv, int64_t D, double scale,
                         int64_t max_len, int64_t window, int64_t splits) {
  const at::Tensor &k_cache = c.k, &v_cache = c.v;
  check_qkv(qkv, nq, nkv, D, name);
  const int64_t G = nq / nkv;
  DTG_CHECK(decode::group_ok(G), name, ": query heads per kv head must be one of 1, 2, 3, 4, 7, 8, 16");
  check_cache<Fmt>(c, nkv, D, name);
  const int64_t T = qkv.size(0), S_max = k_cache.size(2);
  DTG_CHECK(Q >= 1 && Q < (int64_t(1) << 20) && T % Q == 0, name, ": q_len must be >= 1 and divide the rows of qkv");
  const int64_t B = T / Q;
  check_index(rows, B, name, "rows", Q == 1 ? "token" : "sequence");
  check_index(lens, T, name, "lens");
  DTG_CHECK(max_len >= 0 && max_len <= S_max, name, ": max_len must lie in [0, S_max]");
  DTG_CHECK(window >= 0 && splits >= 0, name, ": window and splits must not be negative");
  const c10::DeviceGuard dg(qkv.device());
  auto out = at::empty({T, nq * D}, qkv.options());
  if (T == 0) return out;
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const decode::Plan p = decode::plan_multi({B, (int)nkv, (int)G, (int)D, max_len, window, cus, (int)splits}, (int)Q);
  const int64_t nwg = (int64_t)p.grid.x * p.grid.y * p.grid.z;
  DTG_CHECK(nwg < (int64_t(1) << 31), name, ": too many workgroups");
  float *ws_o = nullptr, *ws_ml = nullptr;
  at::Tensor ws;
  if (p.splits > 1) {  // [T nkv splits G D] outputs, then [T nkv splits G 2] max | sum
    ws = at::empty({(int64_t)(p.ws_bytes / sizeof(float))}, qkv.options().dtype(at::kFloat));
    ws_o = ws.data_ptr<float>();
    ws_ml = ws_o + T * nkv * p.splits * G * D;
  }
#define DTG_DECODE_LAUNCH(D_, G_, QT_)                                                                              \
  decode_attn_kernel<Fmt, D_, G_, QT_><<<(unsigned)nwg, decode::kThreads, 0, stream()>>>(                           \
      bf16_ptr(qkv), qkv.stride(0), c.data<Fmt>(k_cache), c.data<Fmt>(v_cache), rows.data_ptr<int32_t>(),           \
      lens.data_ptr<int32_t>(), ws_o, ws_ml, bf16_mut(out), (int)nkv, p.splits, p.chunk, window, k_cache.size(0),   \
      S_max, (float)scale, (int)Q, c.scale<Fmt>(c.k_scale), c.scale<Fmt>(c.v_scale))
#define DTG_DECODE_GQ(D_, G_, QT_)                \
  if (Q == 1) {                                   \
    DTG_DECODE_LAUNCH(D_, G_, 1);                 \
  } else {                                        \
    static_assert(QT_ == decode::q_tile(G_), "q tile"); \
    DTG_DECODE_LAUNCH(D_, G_, QT_);               \
  }                                               \
  break
#define DTG_DECODE_G(D_)                          \
  switch (G) {                                    \
    case 1: DTG_DECODE_GQ(D_, 1, 8);              \
    case 2: DTG_DECODE_GQ(D_, 2, 8);              \
    case 3: DTG_DECODE_GQ(D_, 3, 4);              \
    case 4: DTG_DECODE_GQ(D_, 4, 4);              \
    case 7: DTG_DECODE_GQ(D_, 7, 2);              \
    case 8: DTG_DECODE_GQ(D_, 8, 2);              \
    default: DTG_DECODE_GQ(D_, 16, 1);            \
  }
  DTG_HD_DISPATCH(D, DTG_DECODE_G(HD))
#undef DTG_DECODE_G
#undef DTG_DECODE_GQ
#undef DTG_DECODE_LAUNCH
  DTG_LAUNCH_CHECK();
  if (p.splits > 1) {
    DTG_HD_DISPATCH(D, decode_combine_kernel<HD><<<(unsigned)(T * nkv), decode::kThreads, 0, stream()>>>(
                           ws_o, ws_ml, bf16_mut(out), (int)G, p.splits));
    DTG_LAUNCH_CHECK();
  }
  return out;
}

}  // namespace

void kv_cache_append_(const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                      const at::Tensor& cos_t, const at::Tensor& sin_t, const at::Tensor& pos, const at::Tensor& rows,
                      int64_t nq, int64_t nkv, int64_t head_dim) {
  append_launch<Bf16Cache>("kv_cache_append_", qkv, {k_cache, v_cache}, cos_t, sin_t, pos, rows, nq, nkv, head_dim);
}

void kv_cache_append_fp8_(const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                          const at::Tensor& k_scale, const at::Tensor& v_scale, const at::Tensor& cos_t,
                          const at::Tensor& sin_t, const at::Tensor& pos, const at::Tensor& rows, int64_t nq,
                          int64_t nkv, int64_t head_dim) {
  append_launch<E4m3Cache>("kv_cache_append_fp8_", qkv, {k_cache, v_cache, &k_scale, &v_scale}, cos_t, sin_t, pos,
                           rows, nq, nkv, head_dim);
}

at::Tensor decode_attn(const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                       const at::Tensor& rows, const at::Tensor& lens, int64_t nq, int64_t nkv, int64_t head_dim,
                       double scale, int64_t max_len, int64_t window, int64_t splits) {
  return decode_launch<Bf16Cache>("decode_attn", qkv, {k_cache, v_cache}, rows, lens, 1, nq, nkv, head_dim, scale,
                                  max_len, window, splits);
}

at::Tensor decode_attn_multi(const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                             const at::Tensor& rows, const at::Tensor& lens, int64_t q_len, int64_t nq, int64_t nkv,
                             int64_t head_dim, double scale, int64_t max_len, int64_t window, int64_t splits) {
  return decode_launch<Bf16Cache>("decode_attn_multi", qkv, {k_cache, v_cache}, rows, lens, q_len, nq, nkv, head_dim,
                                  scale, max_len, window, splits);
}

// q_len = 1: the one-token kernel; q_len > 1: the tile of decode::q_tile(G) tokens
at::Tensor decode_attn_fp8(const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                           const at::Tensor& k_scale, const at::Tensor& v_scale, const at::Tensor& rows,
                           const at::Tensor& lens, int64_t q_len, int64_t nq, int64_t nkv, int64_t head_dim,
                           double scale, int64_t max_len, int64_t window, int64_t splits) {
  return decode_launch<E4m3Cache>("decode_attn_fp8", qkv, {k_cache, v_cache, &k_scale, &v_scale}, rows, lens, q_len,
                                  nq, nkv, head_dim, scale, max_len, window, splits);
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) {
  m.impl("kv_cache_append_", &kv_cache_append_);
  m.impl("kv_cache_append_fp8_", &kv_cache_append_fp8_);
  m.impl("decode_attn", &decode_attn);
  m.impl("decode_attn_multi", &decode_attn_multi);
  m.impl("decode_attn_fp8", &decode_attn_fp8);
}

}  // namespace dtg
