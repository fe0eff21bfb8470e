// What the rotary kernels (rope.hip, the append of decode_attn.hip, qk_norm.hip, the flash-attention
// host code) share beyond common.h: the (token, head, 8-pair group) work item, the table load, the
// rotation itself and the argument checks and head-dim dispatch of their host wrappers.  Only inline
// entities and templates: the objects are linked without relocatable device code.
//
// Convention (HF Llama): q' = q*cos + rotate_half(q)*sin with rotate_half(x) = [-x2, x1], so the pair
// (x1, x2) = (x[i], x[i + D/2]) turns by +theta = pos * freq[i].  The tables hold the D/2 distinct
// frequencies in f32, [max_pos, D/2]; positions are int64, one per token.
#pragma once

#include "common.h"

namespace dtg {

// csrc/kernels/rope.hip: the rotation of `nheads` heads per row on raw pointers, for other files.
void rope_rows_launch(uint16_t* x, int64_t row_stride, int nheads, int head_dim, const float* cos_t,
                      const float* sin_t, const int64_t* pos, int64_t T, bool inverse, hipStream_t st);

namespace rope {

// Work items of T tokens x nheads heads: a head is D/16 items of 8 pairs each.
__host__ __device__ inline int64_t items(int64_t T, int64_t nheads, int D) { return T * nheads * (D / 16); }

// Item `gid` of items(T, nheads, D): its 8 elements of the first half start at in(x, row_stride), the
// matching 8 of the second half HALF elements further.
template <int D>
struct Item {
  static constexpr int HALF = D / 2, GROUPS = HALF / 8;
  int grp;
  int64_t th;  // tok * nheads + head
  int head;
  int64_t tok;
  __device__ __forceinline__ Item(int64_t gid, int nheads)
      : grp(gid % GROUPS), th(gid / GROUPS), head(th % nheads), tok(th / nheads) {}
  __device__ __forceinline__ uint16_t* in(uint16_t* x, int64_t row_stride) const {
    return x + tok * row_stride + (int64_t)head * D + grp * 8;
  }
};

// cos / sin of position p for pair group grp.
template <int D>
__device__ __forceinline__ void load_cs(const float* cos_t, const float* sin_t, int64_t p, int grp, float* c,
                                        float* s) {
  load8f(cos_t + p * (D / 2) + grp * 8, c);
  load8f(sin_t + p * (D / 2) + grp * 8, s);
}

// (x1, x2) turned by +theta.  The ONE definition of the forward expression order: kernels whose bits
// must agree (rope_, kv_cache_append_) both call it.  o may alias x.
__device__ __forceinline__ void rotate(const float* x1, const float* x2, const float* c, const float* s, float* o1,
                                       float* o2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a = x1[j] * c[j] - x2[j] * s[j];
    const float b = x2[j] * c[j] + x1[j] * s[j];
    o1[j] = a;
    o2[j] = b;
  }
}

// (x1, x2) turned by -theta (the backward of rotate: its Jacobian is orthogonal), written out with
// the signs in place.  rotate() with s negated is the same value but not necessarily the same FMA
// contraction; rope_kernel, whose direction is a runtime flag, uses that form.
__device__ __forceinline__ void rotate_inv(const float* x1, const float* x2, const float* c, const float* s, float* o1,
                                           float* o2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a = x1[j] * c[j] + x2[j] * s[j];
    const float b = x2[j] * c[j] - x1[j] * s[j];
    o1[j] = a;
    o2[j] = b;
  }
}

// A fused-QKV activation (or its gradient) whose first nheads * D columns a kernel reads or writes
// with 16-byte accesses.
inline void check_qkv(const at::Tensor& qkv, int64_t nheads, int64_t D, const char* name) {
  DTG_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16, name, ": qkv must be a bf16 GPU tensor");
  DTG_CHECK(D == 64 || D == 128, name, ": head_dim must be 64 or 128");
  DTG_CHECK(nheads >= 1 && nheads < (1 << 20), name, ": bad head counts");
  DTG_CHECK(qkv.dim() == 2 && qkv.stride(1) == 1 && qkv.stride(0) % 8 == 0 &&
                reinterpret_cast<uintptr_t>(qkv.data_ptr()) % 16 == 0,
            name, ": qkv must be [T, C] with 16-B aligned rows");
  DTG_CHECK(qkv.size(1) >= nheads * D, name, ": not enough columns for the heads");
  DTG_CHECK(qkv.size(0) == 0 || qkv.stride(0) >= qkv.size(1), name, ": overlapping rows");
}

// Returns max_pos.
inline int64_t check_tables(const at::Tensor& cos_t, const at::Tensor& sin_t, int64_t D, const char* name) {
  DTG_CHECK(cos_t.is_cuda() && sin_t.is_cuda() && cos_t.scalar_type() == at::kFloat &&
                sin_t.scalar_type() == at::kFloat && cos_t.dim() == 2 && cos_t.is_contiguous() &&
                sin_t.is_contiguous() && cos_t.size(1) == D / 2 && sin_t.sizes() == cos_t.sizes(),
            name, ": tables must be contiguous f32 GPU tensors [max_pos, D/2]");
  return cos_t.size(0);
}

inline void check_pos(const at::Tensor& pos, int64_t T, const char* name) {
  DTG_CHECK(pos.is_cuda() && pos.scalar_type() == at::kLong && pos.is_contiguous() && pos.numel() == T, name,
            ": position ids must be an int64 GPU tensor [T]");
}

// The operators with an optional rotation take empty tables for "none": both, or neither.
inline bool enabled(const at::Tensor& cos_t, const at::Tensor& sin_t, const char* name) {
  if (cos_t.numel() > 0) return true;
  DTG_CHECK(sin_t.numel() == 0, name, ": cos and sin must both be empty for the form without RoPE");
  return false;
}

}  // namespace rope

// Runs the statement with `constexpr int HD` = D_, which the caller has checked to be 64 or 128 ...
#define DTG_HD_DISPATCH(D_, ...)                     \
  if (D_ == 128) { constexpr int HD = 128; __VA_ARGS__; } \
  else { constexpr int HD = 64; __VA_ARGS__; }
// ... and with `constexpr bool RP` = rope as well.
#define DTG_HD_RP_DISPATCH(D_, rope, ...)                                \
  DTG_HD_DISPATCH(D_, if (rope) { constexpr bool RP = true; __VA_ARGS__; } \
                      else { constexpr bool RP = false; __VA_ARGS__; })

}  // namespace dtg
