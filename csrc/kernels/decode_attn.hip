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
#include "decode_attn_plan.h"
#include "rope_common.h"

#include <ATen/hip/HIPContext.h>

namespace dtg {

namespace {

// exp(m - m_new) of a running max that may still be -inf (nothing seen): weight 0, never NaN
__device__ __forceinline__ float rescale(float m, float m_new) { return m == -INFINITY ? 0.f : __expf(m - m_new); }

template <int D, bool ROPE>
__global__ __launch_bounds__(256) void kv_append_kernel(
    uint16_t* __restrict__ qkv, int64_t row_stride, uint16_t* __restrict__ kc, uint16_t* __restrict__ vc,
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
    *reinterpret_cast<u16x8*>(base) = b1;
    *reinterpret_cast<u16x8*>(base + HALF) = b2;
  }
  if (it.head >= nq) {
    const bool is_k = it.head < nq + nkv;
    const int kvh = is_k ? it.head - nq : it.head - nq - nkv;
    uint16_t* dst = (is_k ? kc : vc) + ((r * nkv + kvh) * S_max + p) * D + it.grp * 8;
    *reinterpret_cast<u16x8*>(dst) = b1;
    *reinterpret_cast<u16x8*>(dst + HALF) = b2;
  }
}

// QT = 1 is decode_attn; QT > 1 serves decode_attn_multi: a tile of QT consecutive tokens of sequence b
// (tokens t0 .. t0 + QT - 1 of its Q, row b * Q + t of qkv / lens) shares the workgroup's K / V stream.
// The QT * G (token, head) pairs are laid out as the G heads of the one-token form; a pair's arithmetic
// is that form's, expression for expression.  The key loop starts at the smallest k0 of the tile's
// tokens that hold keys in this split (all equal split * chunk without a window, so key j sits in the
// same lane whatever the query) and runs to their largest k1; a key outside a token's own [k0, k1)
// scores -inf for it, which leaves its (m, l, acc) as they were: alpha = exp(m - m) = 1, p = 0.
template <int D, int G, int QT>
__global__ __launch_bounds__(decode::kThreads) void decode_attn_kernel(
    const uint16_t* __restrict__ qkv, int64_t q_stride, const uint16_t* __restrict__ kc,
    const uint16_t* __restrict__ vc, const int32_t* __restrict__ rows, const int32_t* __restrict__ lens,
    float* __restrict__ ws_o, float* __restrict__ ws_ml, uint16_t* __restrict__ out, int nkv, int splits,
    int64_t chunk, int64_t window, int64_t rows_max, int64_t S_max, float scale, int Q) {
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
  const uint16_t* kb = kc + head_off;
  const uint16_t* vb = vc + head_off;
  for (int64_t j0 = k0; j0 < k1; j0 += decode::kKeyTile) {
    u16x8 kr[UN], vr[UN];
    unsigned ok[UN];  // bit t: token t of the tile attends the key
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t j = j0 + u * KSTEP + wave * KPW + sub;
      ok[u] = 0;
#pragma unroll
      for (int t = 0; t < QT; ++t) ok[u] |= (unsigned)(j >= tk0[t] && j < tk1[t]) << t;
      kr[u] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      vr[u] = kr[u];
      if (QT == 1 ? ok[u] != 0 : j < k1) {  // the hull: a key between two tokens' ranges is loaded
        kr[u] = *reinterpret_cast<const u16x8*>(kb + j * D);
        vr[u] = *reinterpret_cast<const u16x8*>(vb + j * D);
      }
    }
    float sc[UN][H];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      float kf[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) kf[i] = bf2f(kr[u][i]);
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
    for (int u = 0; u < UN; ++u)
#pragma unroll
      for (int i = 0; i < 8; ++i) vf[u][i] = bf2f(vr[u][i]);
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

void check_cache(const at::Tensor& k_cache, const at::Tensor& v_cache, int64_t nkv, int64_t D, const char* name) {
  DTG_CHECK_CUDA_BF16(k_cache);
  DTG_CHECK_CUDA_BF16(v_cache);
  DTG_CHECK(k_cache.dim() == 4 && k_cache.is_contiguous() && v_cache.is_contiguous() &&
                k_cache.sizes() == v_cache.sizes() && k_cache.size(1) == nkv && k_cache.size(3) == D,
            name, ": caches must be contiguous bf16 [rows_max, nkv, S_max, head_dim]");
  DTG_CHECK(k_cache.numel() < (int64_t(1) << 46), name, ": cache too large");
}

void check_qkv(const at::Tensor& qkv, int64_t nq, int64_t nkv, int64_t D, const char* name) {
  DTG_CHECK(nq >= 1 && nkv >= 1 && nq % nkv == 0, name, ": bad head counts");
  rope::check_qkv(qkv, nq + 2 * nkv, D, name);
}

void check_index(const at::Tensor& t, int64_t n, const char* name, const char* what, const char* per = "token") {
  DTG_CHECK(t.is_cuda() && t.scalar_type() == at::kInt && t.is_contiguous() && t.numel() == n, name, ": ", what,
            " must be an int32 GPU tensor with one entry per ", per);
}

}  // namespace

void kv_cache_append_(const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                      const at::Tensor& cos_t, const at::Tensor& sin_t, const at::Tensor& pos, const at::Tensor& rows,
                      int64_t nq, int64_t nkv, int64_t head_dim) {
  const char* name = "kv_cache_append_";
  const int64_t D = head_dim;
  check_qkv(qkv, nq, nkv, D, name);
  check_cache(k_cache, v_cache, nkv, D, name);
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
  DTG_HD_RP_DISPATCH(D, rope, kv_append_kernel<HD, RP><<<(unsigned)nblk, 256, 0, stream()>>>(
                                  bf16_mut(qkv), qkv.stride(0), bf16_mut(k_cache), bf16_mut(v_cache), cp, sp, max_pos,
                                  pos.data_ptr<int64_t>(), rows.data_ptr<int32_t>(), (int)nq, (int)nkv, T,
                                  k_cache.size(0), k_cache.size(2)));
  DTG_LAUNCH_CHECK();
}

namespace {

// decode_attn (Q = 1) and decode_attn_multi: qkv holds Q tokens for each of rows.numel() sequences, lens
// one entry per token.  Q = 1 runs the one-token kernel, Q > 1 the tile of decode::q_tile(G) tokens.
at::Tensor decode_launch(const char* name, const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                         const at::Tensor& rows, const at::Tensor& lens, int64_t Q, int64_t nq, int64_t nkv, int64_t D,
                         double scale, int64_t max_len, int64_t window, int64_t splits) {
  check_qkv(qkv, nq, nkv, D, name);
  const int64_t G = nq / nkv;
  DTG_CHECK(decode::group_ok(G), name, ": query heads per kv head must be one of 1, 2, 3, 4, 7, 8, 16");
  check_cache(k_cache, v_cache, nkv, D, name);
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
  decode_attn_kernel<D_, G_, QT_><<<(unsigned)nwg, decode::kThreads, 0, stream()>>>(                                \
      bf16_ptr(qkv), qkv.stride(0), bf16_ptr(k_cache), bf16_ptr(v_cache), rows.data_ptr<int32_t>(),                 \
      lens.data_ptr<int32_t>(), ws_o, ws_ml, bf16_mut(out), (int)nkv, p.splits, p.chunk, window, k_cache.size(0), \
      S_max, (float)scale, (int)Q)
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

at::Tensor decode_attn(const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                       const at::Tensor& rows, const at::Tensor& lens, int64_t nq, int64_t nkv, int64_t head_dim,
                       double scale, int64_t max_len, int64_t window, int64_t splits) {
  return decode_launch("decode_attn", qkv, k_cache, v_cache, rows, lens, 1, nq, nkv, head_dim, scale, max_len, window,
                       splits);
}

at::Tensor decode_attn_multi(const at::Tensor& qkv, const at::Tensor& k_cache, const at::Tensor& v_cache,
                             const at::Tensor& rows, const at::Tensor& lens, int64_t q_len, int64_t nq, int64_t nkv,
                             int64_t head_dim, double scale, int64_t max_len, int64_t window, int64_t splits) {
  return decode_launch("decode_attn_multi", qkv, k_cache, v_cache, rows, lens, q_len, nq, nkv, head_dim, scale, max_len,
                       window, splits);
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) {
  m.impl("kv_cache_append_", &kv_cache_append_);
  m.impl("decode_attn", &decode_attn);
  m.impl("decode_attn_multi", &decode_attn_multi);
}

}  // namespace dtg
