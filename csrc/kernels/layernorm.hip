// LayerNorm (+ fused dropout + residual add) forward/backward for gfx950: the GPT-2 block's
// streaming passes over [T, n_embd].
//
// Semantics follow ATen's bf16 layer_norm: statistics in f32, one rounding on store,
//     y = bf16((h - mean) * rstd * w + b),   mean, rstd f32 [T].
// The fused variant first forms h = bf16(residual + keep * x * scale) -- the block's residual
// dropout and add -- and normalises h, so one HBM pass replaces three and no mask is stored.
// The variance is two-pass over the registers that hold the row (mean, then the centred sum of
// squares), never E[x^2] - mean^2: with a row mean of 64 and a spread of 0.5 the one-pass form
// loses the variance's leading digits to the rounding of two numbers near 4096.
//
// Dropout keep mask (regenerated in the backward): element (row, col) is kept iff byte (col & 3)
// of word ((col >> 2) & 1) of
//     Philox4x32-10(counter = {col >> 3, row, offset lo, kStreamTag}, key = {seed lo, seed hi ^ offset hi})
// is < thr = round((1 - p) * 256); kept values are scaled by 256 / thr (the byte-threshold
// convention of the attention dropout).  {seed, offset} is the int64 [2] device tensor of
// dtg::philox_rng, read from memory by the kernel, so a captured HIP graph redraws it every
// replay.  One Philox call covers the 8 columns of one 16-byte chunk (words 2 and 3 are not
// used); nothing in the function depends on the launch geometry.  dtg.ops._cpu.ln_dropout_keep is
// the same function.
//
// Layout (that of rmsnorm.hip): one 256-thread workgroup per row; each lane owns PER 16-byte
// chunks of the row and keeps them in registers between the reductions and the write.  The
// backward walks rows_per_block rows per workgroup, software-pipelined, and writes f32 partials
// of dw and db that a second kernel column-reduces in a fixed order (no atomics, bitwise
// reproducible).
#include "norm_common.h"
#include "philox.h"

namespace dtg {
namespace ln {

using norm::kThreads;
constexpr uint32_t kStreamTag = 0x4C4E4452u;  // "LNDR": keeps this stream apart from the attention mask's

// The 8 keep decisions of chunk `chunk` of row `row`: bit j = column 8 * chunk + j is kept.
__device__ __forceinline__ uint32_t keep_bits(const philox::Key& k, int row, int chunk, int thr) {
  uint32_t c[4] = {(uint32_t)chunk, (uint32_t)row, k.off, kStreamTag};
  philox::rounds10(c, k.k0, k.k1);
  uint32_t bits = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) bits |= ((int)((c[j >> 2] >> (8 * (j & 3))) & 255u) < thr ? 1u : 0u) << j;
  return bits;
}

// MODE 0: h = x.  MODE 1: h = bf16(x + residual).  MODE 2: h = bf16(residual + keep * x * scale).
template <int PER, int MODE>
__global__ __launch_bounds__(kThreads) void layernorm_fwd_kernel(
    const uint16_t* __restrict__ x, int64_t x_stride, const uint16_t* __restrict__ res, int64_t res_stride,
    const uint16_t* __restrict__ w, const uint16_t* __restrict__ b, uint16_t* __restrict__ y,
    uint16_t* __restrict__ h_out, float* __restrict__ mean_out, float* __restrict__ rstd_out, int H, float eps,
    int thr, float scale, const uint32_t* __restrict__ rng) {
  __shared__ float scratch[kThreads / 64];
  const int row = blockIdx.x;
  const int nch = H >> 3;
  const uint16_t* xr = x + row * x_stride;
  philox::Key key{};
  if constexpr (MODE == 2) key = philox::load_key(rng);
  float v[PER][8];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = threadIdx.x + i * kThreads;
    if (c < nch) {
      load8(xr + c * 8, v[i]);
      if constexpr (MODE != 0) {
        float r[8];
        load8(res + row * res_stride + c * 8, r);
        if constexpr (MODE == 2) {
          const uint32_t keep = keep_bits(key, row, c, thr);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[i][j] = (keep >> j) & 1u ? v[i][j] * scale : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] = bf2f(f2bf(r[j] + v[i][j]));
        store8(h_out + (int64_t)row * H + c * 8, v[i]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[i][j];
    }
  }
  const float mean = block_sum(s, scratch) / H;
  // lanes past the end of the row add nothing here either (0, not (0 - mean)^2)
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = threadIdx.x + i * kThreads;
    if (c < nch) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[i][j] -= mean;
        ss += v[i][j] * v[i][j];
      }
    }
  }
  ss = block_sum(ss, scratch);
  const float rstd = rsqrtf(ss / H + eps);
  if (threadIdx.x == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = threadIdx.x + i * kThreads;
    if (c < nch) {
      float wv[8], bv[8], o[8];
      load8(w + c * 8, wv);
      load8(b + c * 8, bv);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = v[i][j] * rstd * wv[j] + bv[j];
      store8(y + (int64_t)row * H + c * 8, o);
    }
  }
}

// dh = rstd * (g - mean(g) - n * mean(g * n)) (+ dres),  g = dy * w,  n = (h - mean) * rstd
// dx = bf16(keep * scale * dh) from the f32 dh (DROP only; without dropout dx is dh)
// dw_partial[block][col] = sum over this block's rows of dy * n,  db_partial likewise of dy
// Rows are software-pipelined as in rmsnorm_bwd_kernel: the next row's h / dy / dres vectors are
// loaded (as raw 16-byte words) before the current row's block reduction.  The current row is
// kept as raw words too and widened twice, which holds PER = 8 within the register file next to
// the dw and db accumulators.
template <int PER, bool DRES, bool DROP>
__global__ __launch_bounds__(kThreads) void layernorm_bwd_kernel(
    const uint16_t* __restrict__ dy, const uint16_t* __restrict__ h, int64_t h_stride,
    const uint16_t* __restrict__ w, const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    const uint16_t* __restrict__ dres, uint16_t* __restrict__ dh, uint16_t* __restrict__ dx,
    float* __restrict__ dw_part, float* __restrict__ db_part, int T, int H, int rows_per_block, int thr,
    float scale, const uint32_t* __restrict__ rng) {
  __shared__ float scratch[2 * kThreads / 64];
  const int nch = H >> 3;
  philox::Key key{};
  if constexpr (DROP) key = philox::load_key(rng);
  float dwacc[PER][8], dbacc[PER][8], wv[PER][8];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = threadIdx.x + i * kThreads;
#pragma unroll
    for (int j = 0; j < 8; ++j) dwacc[i][j] = dbacc[i][j] = wv[i][j] = 0.f;
    if (c < nch) load8(w + c * 8, wv[i]);
  }
  const int r0 = blockIdx.x * rows_per_block;
  const int r1 = min(T, r0 + rows_per_block);
  const u16x8 z{0, 0, 0, 0, 0, 0, 0, 0};
  u16x8 nh[PER], nd[PER], nr[PER];
  auto fetch = [&](int row) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = threadIdx.x + i * kThreads;
      const bool ok = c < nch && row < r1;
      nh[i] = ok ? *reinterpret_cast<const u16x8*>(h + row * h_stride + c * 8) : z;
      nd[i] = ok ? *reinterpret_cast<const u16x8*>(dy + (int64_t)row * H + c * 8) : z;
      if constexpr (DRES) nr[i] = ok ? *reinterpret_cast<const u16x8*>(dres + (int64_t)row * H + c * 8) : z;
    }
  };
  if (r0 < r1) fetch(r0);
  for (int row = r0; row < r1; ++row) {
    const float mean = mean_in[row], rstd = rstd_in[row];
    u16x8 ch[PER], cd[PER], cr[PER];
    float sg = 0.f, sgn = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = threadIdx.x + i * kThreads;
      ch[i] = nh[i];
      cd[i] = nd[i];
      if constexpr (DRES) cr[i] = nr[i];
      // lanes past the end of the row add 0 to both sums (their n would be -mean * rstd)
      if (c < nch) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = bf2f(cd[i][j]);
          const float n = (bf2f(ch[i][j]) - mean) * rstd;
          const float g = d * wv[i][j];
          sg += g;
          sgn += g * n;
          dwacc[i][j] += d * n;
          dbacc[i][j] += d;
        }
      }
    }
    fetch(row + 1);  // in flight across the reduction below
    block_sum2(sg, sgn, scratch);
    sg /= H;
    sgn /= H;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = threadIdx.x + i * kThreads;
      if (c < nch) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float n = (bf2f(ch[i][j]) - mean) * rstd;
          o[j] = rstd * (bf2f(cd[i][j]) * wv[i][j] - sg - n * sgn);
          if constexpr (DRES) o[j] += bf2f(cr[i][j]);
        }
        store8(dh + (int64_t)row * H + c * 8, o);
        if constexpr (DROP) {
          const uint32_t keep = keep_bits(key, row, c, thr);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (keep >> j) & 1u ? o[j] * scale : 0.f;
          store8(dx + (int64_t)row * H + c * 8, o);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = threadIdx.x + i * kThreads;
    if (c < nch) {
      store8f(dw_part + (int64_t)blockIdx.x * H + c * 8, dwacc[i]);
      store8f(db_part + (int64_t)blockIdx.x * H + c * 8, dbacc[i]);
    }
  }
}

static void check_affine(const at::Tensor& w, const at::Tensor* b, int H) {
  DTG_CHECK_CUDA_BF16(w);
  DTG_CHECK(H % 8 == 0 && w.numel() == H && w.is_contiguous(), "layernorm: bad weight/hidden");
  if (b != nullptr) {
    DTG_CHECK_CUDA_BF16(*b);
    DTG_CHECK(b->numel() == H && b->is_contiguous(), "layernorm: bad bias");
  }
}

struct Drop {
  int thr = 256;
  float scale = 1.f;
  const uint32_t* rng = nullptr;
};

// p == 0: no dropout and `rng` must be None.  p > 0: rng is the int64 [2] tensor {seed, offset}.
static Drop make_drop(double p, const c10::optional<at::Tensor>& rng, const at::Tensor& like) {
  DTG_CHECK(p >= 0.0 && p < 1.0, "layernorm dropout: p must be in [0, 1)");
  const bool has = rng.has_value() && rng->defined();
  Drop d;
  if (p == 0.0) {
    DTG_CHECK(!has, "layernorm dropout: rng given with p == 0");
    return d;
  }
  DTG_CHECK(has && rng->is_cuda() && rng->scalar_type() == at::kLong && rng->numel() == 2 && rng->is_contiguous() &&
                rng->device() == like.device(),
            "layernorm dropout: rng must be a contiguous int64 [2] tensor {seed, offset} on the inputs' device");
  d.thr = std::max(1, std::min(256, (int)std::lround((1.0 - p) * 256.0)));
  d.scale = 256.f / (float)d.thr;
  d.rng = reinterpret_cast<const uint32_t*>(rng->data_ptr<int64_t>());
  return d;
}

}  // namespace ln

template <int MODE>
static void launch_layernorm_fwd(int per, const at::Tensor& x, const at::Tensor& res, const at::Tensor& w,
                                 const at::Tensor& b, at::Tensor& y, at::Tensor& h, at::Tensor& mean, at::Tensor& rstd,
                                 int T, int H, double eps, const ln::Drop& d) {
  DTG_PER_DISPATCH("layernorm", per,
                   ln::layernorm_fwd_kernel<P, MODE><<<T, ln::kThreads, 0, stream()>>>(
                       bf16_ptr(x), x.stride(0), MODE ? bf16_ptr(res) : nullptr, MODE ? res.stride(0) : 0, bf16_ptr(w),
                       bf16_ptr(b), bf16_mut(y), MODE ? bf16_mut(h) : nullptr, mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), H, (float)eps, d.thr, d.scale, d.rng));
}

// layernorm_fwd (ADD = false: `res` is not read, h stays undefined, no dropout) and
// dropout_add_layernorm_fwd: y, h, mean, rstd.
template <bool ADD>
static std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> layernorm_fwd_impl(
    const at::Tensor& x, const at::Tensor& res, const at::Tensor& w, const at::Tensor& b, double eps, double p,
    const c10::optional<at::Tensor>& rng) {
  norm::check_rows(x, "x");
  if (ADD) norm::check_rows(res, "residual");
  const int T = x.size(0), H = x.size(1);
  if (ADD) DTG_CHECK(res.size(0) == T && res.size(1) == H, "dropout_add_layernorm: shape mismatch");
  ln::check_affine(w, &b, H);
  const ln::Drop d = ln::make_drop(p, rng, x);
  const c10::DeviceGuard g(x.device());
  auto y = at::empty({T, H}, x.options());
  auto h = ADD ? at::empty({T, H}, x.options()) : at::Tensor();
  auto mean = at::empty({T}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({T}, x.options().dtype(at::kFloat));
  if (T == 0) return {y, h, mean, rstd};
  const int per = norm::pick_per(H);
  if (!ADD) launch_layernorm_fwd<0>(per, x, res, w, b, y, h, mean, rstd, T, H, eps, d);
  else if (d.rng == nullptr) launch_layernorm_fwd<1>(per, x, res, w, b, y, h, mean, rstd, T, H, eps, d);
  else launch_layernorm_fwd<2>(per, x, res, w, b, y, h, mean, rstd, T, H, eps, d);
  DTG_LAUNCH_CHECK();
  return {y, h, mean, rstd};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> layernorm_fwd(const at::Tensor& x, const at::Tensor& w,
                                                             const at::Tensor& b, double eps) {
  auto [y, h, mean, rstd] = layernorm_fwd_impl<false>(x, at::Tensor(), w, b, eps, 0.0, c10::nullopt);
  return {y, mean, rstd};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> dropout_add_layernorm_fwd(
    const at::Tensor& x, const at::Tensor& res, const at::Tensor& w, const at::Tensor& b, double eps, double p,
    const c10::optional<at::Tensor>& rng) {
  return layernorm_fwd_impl<true>(x, res, w, b, eps, p, rng);
}

template <bool DRES, bool DROP>
static void launch_layernorm_bwd(int per, const norm::Split& s, const at::Tensor& dy, const at::Tensor& h,
                                 const at::Tensor& w, const at::Tensor& mean, const at::Tensor& rstd,
                                 const at::Tensor& dres, at::Tensor& dh, at::Tensor& dx, at::Tensor& part, int T, int H,
                                 const ln::Drop& d) {
  float* dw_part = part.data_ptr<float>();
  DTG_PER_DISPATCH("layernorm", per,
                   ln::layernorm_bwd_kernel<P, DRES, DROP><<<(unsigned)s.n_blocks, ln::kThreads, 0, stream()>>>(
                       bf16_ptr(dy), bf16_ptr(h), h.stride(0), bf16_ptr(w), mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), DRES ? bf16_ptr(dres) : nullptr, bf16_mut(dh),
                       DROP ? bf16_mut(dx) : nullptr, dw_part, dw_part + s.n_blocks * H, T, H, (int)s.per_block, d.thr,
                       d.scale, d.rng));
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> layernorm_bwd(
    const at::Tensor& dy_, const at::Tensor& h, const at::Tensor& w, const at::Tensor& mean, const at::Tensor& rstd,
    const c10::optional<at::Tensor>& dres_, double p, const c10::optional<at::Tensor>& rng) {
  auto dy = dy_.contiguous();
  norm::check_rows(h, "h");
  DTG_CHECK_CUDA_BF16(dy);
  const int T = h.size(0), H = h.size(1);
  ln::check_affine(w, nullptr, H);
  DTG_CHECK(dy.dim() == 2 && dy.size(0) == T && dy.size(1) == H, "layernorm_bwd: dy shape");
  norm::check_stat(mean, T, "layernorm_bwd: mean");
  norm::check_stat(rstd, T, "layernorm_bwd: rstd");
  const ln::Drop d = ln::make_drop(p, rng, h);
  const bool drop = d.rng != nullptr;
  const c10::DeviceGuard g(h.device());
  auto dh = at::empty({T, H}, h.options());
  auto dx = drop ? at::empty({T, H}, h.options()) : dh;
  auto dwb = at::empty({2, H}, w.options());
  if (T == 0) {
    dwb.zero_();
    return {dh, dx, dwb.select(0, 0), dwb.select(0, 1)};
  }
  const at::Tensor dres = norm::checked_dres(dres_, T, H, "layernorm_bwd: dres shape");
  const bool has_dres = dres.defined();
  const int per = norm::pick_per(H);
  DTG_CHECK(per > 0, "layernorm: unsupported hidden size");
  const norm::Split s = norm::row_bwd_split(T);
  auto part = at::empty({2, s.n_blocks, H}, h.options().dtype(at::kFloat));  // dw partials, then db partials
  if (has_dres && drop) launch_layernorm_bwd<true, true>(per, s, dy, h, w, mean, rstd, dres, dh, dx, part, T, H, d);
  else if (has_dres) launch_layernorm_bwd<true, false>(per, s, dy, h, w, mean, rstd, dres, dh, dx, part, T, H, d);
  else if (drop) launch_layernorm_bwd<false, true>(per, s, dy, h, w, mean, rstd, dres, dh, dx, part, T, H, d);
  else launch_layernorm_bwd<false, false>(per, s, dy, h, w, mean, rstd, dres, dh, dx, part, T, H, d);
  DTG_LAUNCH_CHECK();
  norm::colsum_to_bf16(part.data_ptr<float>(), 2, (int)s.n_blocks, H, bf16_mut(dwb));
  return {dh, dx, dwb.select(0, 0), dwb.select(0, 1)};
}

TORCH_LIBRARY_IMPL(dtg, CUDA, m) {
  m.impl("layernorm_fwd", &layernorm_fwd);
  m.impl("dropout_add_layernorm_fwd", &dropout_add_layernorm_fwd);
  m.impl("layernorm_bwd", &layernorm_bwd);
}

}  // namespace dtg
