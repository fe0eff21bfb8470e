// Per-head QK RMSNorm fused with RoPE (Qwen3), in place on the q and k heads of a fused QKV
// activation [T, (nq + 2*nkv) * D]; the v heads are never touched.
//
// Forward, per (token, head < nq + nkv):  y = w * x * rsqrt(mean(x^2) + eps)  in f32 (w = the q weight
// for heads below nq, the k weight otherwise; both [D], shared by all heads), then the rotation of
// rope_common.h (pairs (i, i + D/2), f32 tables [max_pos, D/2], int64 pos[T]), one bf16 rounding on the
// store.  The same pass copies the pre-norm q|k bits to a contiguous xqk [T, (nq + nkv) * D]: the
// backward needs x, and x cannot be recovered from y (weights may be zero).
//
// Backward, in place on the q and k columns of dqkv (the gradient w.r.t. the rotated q and k, as
// flash_attn_bwd_qkv leaves it):  dy = inverse rotation of the gradient (f32),
//   dx = rstd * (w*dy - xh * mean(w*dy*xh)),  xh = x * rstd,   dw[q|k][D] = sum over tokens and heads dy * xh.
// rstd (f32 [T, nq + nkv]) is SAVED by the forward and read here, not recomputed: 4 B per head against
// the 2 * 2 * D B the backward streams anyway, and the backward keeps a single group reduction.
// dw goes through per-workgroup f32 partials and the fixed-order column sum of norm_common.h (as
// rmsnorm.hip / layernorm.hip): no atomics, bitwise reproducible for a given shape.
//
// Layout: a head is D/16 lanes (8 at D = 128, 4 at D = 64); a lane owns 8 elements of the first half
// and the matching 8 of the second half (two 16-B accesses), so the rotation is lane-local and the
// mean is a 3- or 2-step sub-wave butterfly.  A wave therefore carries 8 (16) heads.  ROPE = false
// is the norm-only form (empty tables), used before the Ulysses all-to-all.
#include "norm_common.h"
#include "rope_common.h"

namespace dtg {

// One lane group per (token, head); every lane reaches the butterfly (lanes past the end carry zeros).
template <int D, bool ROPE>
__global__ __launch_bounds__(norm::kThreads) void qk_norm_rope_fwd_kernel(
    uint16_t* __restrict__ qkv, int64_t row_stride, const uint16_t* __restrict__ wq,
    const uint16_t* __restrict__ wk, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const int64_t* __restrict__ pos, uint16_t* __restrict__ xqk, float* __restrict__ rstd_out, int nq, int nh,
    int64_t T, float eps) {
  constexpr int HALF = D / 2;
  const int64_t gid = (int64_t)blockIdx.x * norm::kThreads + threadIdx.x;
  const bool valid = gid < rope::items(T, nh, D);
  const rope::Item<D> it(gid, nh);
  const int grp = it.grp;
  uint16_t* base = nullptr;
  u16x8 r1{0, 0, 0, 0, 0, 0, 0, 0}, r2{0, 0, 0, 0, 0, 0, 0, 0};
  if (valid) {
    base = it.in(qkv, row_stride);
    r1 = *reinterpret_cast<const u16x8*>(base);
    r2 = *reinterpret_cast<const u16x8*>(base + HALF);
    uint16_t* xo = xqk + it.th * D + grp * 8;
    *reinterpret_cast<u16x8*>(xo) = r1;
    *reinterpret_cast<u16x8*>(xo + HALF) = r2;
  }
  float x1[8], x2[8];
  widen8(r1, x1);
  widen8(r2, x2);
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) ss += x1[j] * x1[j] + x2[j] * x2[j];
  ss = lanes_sum<rope::Item<D>::GROUPS>(ss);
  if (!valid) return;
  const float rstd = rsqrtf(ss * (1.0f / D) + eps);
  if (grp == 0) rstd_out[it.th] = rstd;
  const uint16_t* w = (it.head < nq ? wq : wk) + grp * 8;
  float w1[8], w2[8], y1[8], y2[8];
  load8(w, w1);
  load8(w + HALF, w2);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    y1[j] = w1[j] * (x1[j] * rstd);
    y2[j] = w2[j] * (x2[j] * rstd);
  }
  if constexpr (ROPE) {
    float c[8], s[8];
    rope::load_cs<D>(cos_t, sin_t, pos[it.tok], grp, c, s);
    rope::rotate(y1, y2, c, s, y1, y2);
  }
  store8(base, y1);
  store8(base + HALF, y2);
}

// A workgroup owns `tok_per_block` tokens; its 256 / GROUPS lane groups walk their (token, head) items
// in a loop every lane runs the same number of times.  dw accumulates in registers (q and k apart), is
// summed over the lane groups through LDS in a fixed order and written as one row of `part`
// [gridDim.x, 2 * D] (q columns, then k columns).
template <int D, bool ROPE>
__global__ __launch_bounds__(norm::kThreads) void qk_norm_rope_bwd_kernel(
    uint16_t* __restrict__ dqkv, int64_t row_stride, const uint16_t* __restrict__ xqk,
    const float* __restrict__ rstd_in, const uint16_t* __restrict__ wq, const uint16_t* __restrict__ wk,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t, const int64_t* __restrict__ pos,
    float* __restrict__ part, int nq, int nh, int64_t T, int tok_per_block) {
  constexpr int HALF = D / 2;
  constexpr int GROUPS = HALF / 8;
  constexpr int SLOTS = norm::kThreads / GROUPS;
  __shared__ float red[2][SLOTS][D];
  const int slot = threadIdx.x / GROUPS, grp = threadIdx.x % GROUPS;
  const int64_t t0 = (int64_t)blockIdx.x * tok_per_block;
  const int64_t t1 = t0 + tok_per_block < T ? t0 + tok_per_block : T;
  const int nitems = t1 > t0 ? (int)(t1 - t0) * nh : 0;
  const int niter = (nitems + SLOTS - 1) / SLOTS;
  float accq[16], acck[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) accq[j] = acck[j] = 0.f;
  for (int it = 0; it < niter; ++it) {
    const int i = it * SLOTS + slot;
    const bool valid = i < nitems;
    const int64_t tok = t0 + (valid ? i / nh : 0);
    const int head = valid ? i % nh : 0;
    const int64_t th = tok * nh + head;
    uint16_t* base = dqkv + tok * row_stride + (int64_t)head * D + grp * 8;
    const uint16_t* xb = xqk + th * D + grp * 8;
    u16x8 g1{0, 0, 0, 0, 0, 0, 0, 0}, g2 = g1, r1 = g1, r2 = g1;
    float rstd = 0.f;
    if (valid) {
      g1 = *reinterpret_cast<const u16x8*>(base);
      g2 = *reinterpret_cast<const u16x8*>(base + HALF);
      r1 = *reinterpret_cast<const u16x8*>(xb);
      r2 = *reinterpret_cast<const u16x8*>(xb + HALF);
      rstd = rstd_in[th];
    }
    const bool isq = head < nq;
    const uint16_t* w = (isq ? wq : wk) + grp * 8;
    float w1[8], w2[8], d1[8], d2[8], x1[8], x2[8];
    load8(w, w1);
    load8(w + HALF, w2);
    widen8(g1, d1);
    widen8(g2, d2);
    widen8(r1, x1);
    widen8(r2, x2);
    if constexpr (ROPE) {
      if (valid) {  // dy = R(-theta) g
        float c[8], s[8];
        rope::load_cs<D>(cos_t, sin_t, pos[tok], grp, c, s);
        rope::rotate_inv(d1, d2, c, s, d1, d2);
      }
    }
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x1[j] *= rstd;  // xh
      x2[j] *= rstd;
      const float e1 = d1[j] * x1[j], e2 = d2[j] * x2[j];  // dy * xh: the dw summand
      if (isq) {
        accq[j] += e1;
        accq[8 + j] += e2;
      } else {
        acck[j] += e1;
        acck[8 + j] += e2;
      }
      d1[j] *= w1[j];  // w * dy
      d2[j] *= w2[j];
      dot += d1[j] * x1[j] + d2[j] * x2[j];
    }
    dot = lanes_sum<GROUPS>(dot) * (1.0f / D);
    if (valid) {
      float o1[8], o2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        o1[j] = rstd * (d1[j] - x1[j] * dot);
        o2[j] = rstd * (d2[j] - x2[j] * dot);
      }
      store8(base, o1);
      store8(base + HALF, o2);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[0][slot][grp * 8 + j] = accq[j];
    red[0][slot][HALF + grp * 8 + j] = accq[8 + j];
    red[1][slot][grp * 8 + j] = acck[j];
    red[1][slot][HALF + grp * 8 + j] = acck[8 + j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * D; c += norm::kThreads) {
    const int kind = c / D, col = c % D;
    float t = 0.f;
    for (int s = 0; s < SLOTS; ++s) t += red[kind][s][col];
    part[(int64_t)blockIdx.x * (2 * D) + c] = t;
  }
}

// Shared argument checks; returns true for the rotating form.
static bool qk_check(const at::Tensor& qkv, const at::Tensor& wq, const at::Tensor& wk, const at::Tensor& cos_t,
                     const at::Tensor& sin_t, const at::Tensor& pos, int64_t nq, int64_t nkv, int64_t D,
                     const char* name) {
  DTG_CHECK(nq >= 1 && nkv >= 1, name, ": bad head counts");
  rope::check_qkv(qkv, nq + nkv, D, name);
  DTG_CHECK_CUDA_BF16(wq);
  DTG_CHECK_CUDA_BF16(wk);
  DTG_CHECK(wq.numel() == D && wk.numel() == D && wq.is_contiguous() && wk.is_contiguous(), name,
            ": weights must be contiguous [head_dim]");
  const bool rope = rope::enabled(cos_t, sin_t, name);  // empty tables: the norm-only form
  if (rope) {
    rope::check_tables(cos_t, sin_t, D, name);
    rope::check_pos(pos, qkv.size(0), name);
  }
  return rope;
}

std::tuple<at::Tensor, at::Tensor> qk_norm_rope_fwd_(const at::Tensor& qkv, const at::Tensor& wq,
                                                     const at::Tensor& wk, const at::Tensor& cos_t,
                                                     const at::Tensor& sin_t, const at::Tensor& pos, int64_t nq,
                                                     int64_t nkv, int64_t head_dim, double eps) {
  const bool rope = qk_check(qkv, wq, wk, cos_t, sin_t, pos, nq, nkv, head_dim, "qk_norm_rope_fwd_");
  const int64_t T = qkv.size(0), nh = nq + nkv;
  const c10::DeviceGuard g(qkv.device());
  auto xqk = at::empty({T, nh * head_dim}, qkv.options());
  auto rstd = at::empty({T, nh}, qkv.options().dtype(at::kFloat));
  if (T == 0) return {xqk, rstd};
  const int64_t nblk = (rope::items(T, nh, head_dim) + norm::kThreads - 1) / norm::kThreads;
  DTG_CHECK(nblk < (int64_t(1) << 31), "qk_norm_rope_fwd_: too many tokens");
  const float* cp = rope ? cos_t.data_ptr<float>() : nullptr;
  const float* sp = rope ? sin_t.data_ptr<float>() : nullptr;
  const int64_t* pp = rope ? pos.data_ptr<int64_t>() : nullptr;
  DTG_HD_RP_DISPATCH(head_dim, rope,
                  qk_norm_rope_fwd_kernel<HD, RP><<<(unsigned)nblk, norm::kThreads, 0, stream()>>>(
                      bf16_mut(qkv), qkv.stride(0), bf16_ptr(wq), bf16_ptr(wk), cp, sp, pp, bf16_mut(xqk),
                      rstd.data_ptr<float>(), (int)nq, (int)nh, T, (float)eps));
  DTG_LAUNCH_CHECK();
  return {xqk, rstd};
}

std::tuple<at::Tensor, at::Tensor> qk_norm_rope_bwd_(const at::Tensor& dqkv, const at::Tensor& xqk,
                                                     const at::Tensor& rstd, const at::Tensor& wq,
                                                     const at::Tensor& wk, const at::Tensor& cos_t,
                                                     const at::Tensor& sin_t, const at::Tensor& pos, int64_t nq,
                                                     int64_t nkv, int64_t head_dim) {
  const bool rope = qk_check(dqkv, wq, wk, cos_t, sin_t, pos, nq, nkv, head_dim, "qk_norm_rope_bwd_");
  const int64_t T = dqkv.size(0), nh = nq + nkv, D = head_dim;
  DTG_CHECK_CUDA_BF16(xqk);
  DTG_CHECK(xqk.dim() == 2 && xqk.is_contiguous() && xqk.size(0) == T && xqk.size(1) == nh * D,
            "qk_norm_rope_bwd_: xqk must be contiguous [T, (nq + nkv) * head_dim]");
  norm::check_stat(rstd, T * nh, "qk_norm_rope_bwd_: rstd must be f32 [T, nq + nkv]");
  const c10::DeviceGuard g(dqkv.device());
  auto dw = at::empty({2 * D}, wq.options());
  if (T == 0) {
    dw.zero_();
    return {dw.narrow(0, 0, D), dw.narrow(0, D, D)};
  }
  const norm::Split s = norm::qk_bwd_split(T);
  const int64_t tpb = s.per_block, nb = s.n_blocks;
  DTG_CHECK(tpb * nh < (int64_t(1) << 30), "qk_norm_rope_bwd_: too many tokens");
  auto part = at::empty({nb, 2 * D}, dqkv.options().dtype(at::kFloat));
  const float* cp = rope ? cos_t.data_ptr<float>() : nullptr;
  const float* sp = rope ? sin_t.data_ptr<float>() : nullptr;
  const int64_t* pp = rope ? pos.data_ptr<int64_t>() : nullptr;
  DTG_HD_RP_DISPATCH(head_dim, rope,
                  qk_norm_rope_bwd_kernel<HD, RP><<<(unsigned)nb, norm::kThreads, 0, stream()>>>(
                      bf16_mut(dqkv), dqkv.stride(0), bf16_ptr(xqk), rstd.data_ptr<float>(), bf16_ptr(wq),
                      bf16_ptr(wk), cp, sp, pp, part.data_ptr<float>(), (int)nq, (int)nh, T, (int)tpb));
  DTG_LAUNCH_CHECK();
  norm::colsum_to_bf16(part.data_ptr<float>(), 1, (int)nb, (int)(2 * D), bf16_mut(dw));
  return {dw.narrow(0, 0, D), dw.narrow(0, D, D)};
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) {
  m.impl("qk_norm_rope_fwd_", &qk_norm_rope_fwd_);
  m.impl("qk_norm_rope_bwd_", &qk_norm_rope_bwd_);
}

}  // namespace dtg
