// Rotary position embedding applied in place to the q and k heads of a fused QKV
// activation [T, (Hq + 2*Hkv) * D].
//
// HF Llama semantics: q' = q*cos + rotate_half(q)*sin with rotate_half(x) = [-x2, x1],
// cos/sin = cat(freqs, freqs) evaluated at position_ids.  The tables here hold the D/2
// distinct frequencies in f32 ([max_pos, D/2]); the kernel rotates pairs (i, i + D/2) in
// f32 (rope_common.h) and rounds once.  `inverse` rotates by -theta, which is exactly the
// backward of the forward rotation (the Jacobian is orthogonal), so the same kernel serves
// both passes.
//
// Positions come from a per-token int64 vector, so packed sequences whose position ids
// restart at every EOS need no special path.
#include "rope_common.h"

namespace dtg {

// One thread per (token, head, 8-pair group): two 16-B loads of x and two 32-B table loads.
template <int D>
__global__ void rope_kernel(uint16_t* __restrict__ qkv, int64_t row_stride, int nheads,
                            const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                            const int64_t* __restrict__ pos, int64_t T, bool inverse) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= rope::items(T, nheads, D)) return;
  const rope::Item<D> it(gid, nheads);
  const int64_t p = pos[it.tok];
  uint16_t* base = it.in(qkv, row_stride);
  float x1[8], x2[8], c[8], s[8];
  load8(base, x1);
  load8(base + it.HALF, x2);
  rope::load_cs<D>(cos_t, sin_t, p, it.grp, c, s);
  if (inverse) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = -s[j];
  }
  rope::rotate(x1, x2, c, s, x1, x2);
  store8(base, x1);
  store8(base + it.HALF, x2);
}

void rope_rows_launch(uint16_t* x, int64_t row_stride, int nheads, int head_dim, const float* cos_t,
                      const float* sin_t, const int64_t* pos, int64_t T, bool inverse, hipStream_t st) {
  if (T == 0) return;
  DTG_CHECK(head_dim == 64 || head_dim == 128, "rope: head_dim must be 64 or 128");
  const int threads = 256;
  const int64_t total = rope::items(T, nheads, head_dim);
  DTG_HD_DISPATCH(head_dim, rope_kernel<HD><<<(total + threads - 1) / threads, threads, 0, st>>>(
                                x, row_stride, nheads, cos_t, sin_t, pos, T, inverse));
  DTG_LAUNCH_CHECK();
}

void rope_(const at::Tensor& qkv, const at::Tensor& cos_t, const at::Tensor& sin_t,
           const at::Tensor& pos, int64_t nheads, int64_t head_dim, bool inverse) {
  rope::check_qkv(qkv, nheads, head_dim, "rope_");
  rope::check_tables(cos_t, sin_t, head_dim, "rope_");
  rope::check_pos(pos, qkv.size(0), "rope_");
  const c10::DeviceGuard g(qkv.device());
  rope_rows_launch(bf16_mut(qkv), qkv.stride(0), nheads, head_dim, cos_t.data_ptr<float>(), sin_t.data_ptr<float>(),
                   pos.data_ptr<int64_t>(), qkv.size(0), inverse, stream());
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) { m.impl("rope_", &rope_); }

}  // namespace dtg
