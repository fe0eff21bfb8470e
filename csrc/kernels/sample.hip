// Fused top-k / top-p / min-p sampling: [n, V] logits -> n ids, one 1,024-thread workgroup per row.
//
// Per row (the definition is in ops/functional.py::sample_logits; dtg.ops._cpu.sample_logits is the
// f64 form of it):
//   pass 1   max M and the lowest index of M; -inf / +inf / greedy rows finish here
//   select   top-k: radix select of the k-th largest logit over the order-preserving integer image
//            ("key") of the f32 bits, 11 bits per level through a 2,048-bin LDS histogram of counts
//            (bf16 rows: two levels, f32 rows: three)
//   select   top-p: the same radix select over a histogram of MASS restricted to the top-k set; the
//            first level's total is Z_A, from which the target top_p * Z_A follows
//   final    kept = {key >= max(t_k, t_p, t_m)}: every wave sums the kept mass of one contiguous
//            slice of the row, thread 0 finds the slice in which the running sum crosses
//            u * Z_K, and that wave walks its slice tile by tile with a lane scan
//
// Masses are 64-bit fixed point: w = exp((x - M) / T) <= 1 is truncated to w * 2^40 (less when V is
// so large that V * 2^40 would not fit), and every sum is an integer sum -- histograms by LDS integer
// atomics, the rest by shuffles in a fixed pattern.  Integer addition is associative, so a row's
// result does not depend on the arrival order of the atomics, on the row's place in the batch or on
// the other rows: it is bitwise reproducible.  An id lighter than 2^-40 of the favourite has mass 0
// and is never drawn.
//
// Rows need not be 16-B aligned (a contiguous bf16 [n, 156939] has 2-B aligned rows): the elements
// before the first 16-B boundary and after the last whole vector are peeled, the body moves 16 B per
// lane.  Nothing is read on the host; all per-row parameters are device tensors.
#include "common.h"
#include "philox.h"

namespace dtg {
namespace {

using u64 = unsigned long long;

constexpr int kThreads = 1024;  // 16 waves: one row is one workgroup, and only waves in flight hide the load latency
constexpr int kWaves = kThreads / kWave;
constexpr int kBins = 2048;  // 11 bits per radix level
constexpr int kBinsPerThread = kBins / kThreads;

// Order-preserving image of a logit: NaN counts as -inf, -0 as +0 (they compare equal as floats).
__device__ __forceinline__ float canonical(float x) {
  if (x != x) x = -INFINITY;
  if (x == 0.f) x = 0.f;
  return x;
}

__device__ __forceinline__ uint32_t key_of(float x) {
  const uint32_t b = __float_as_uint(x);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

template <typename T>
struct Row;

template <>
struct Row<uint16_t> {  // bf16: the low 16 key bits are zero
  static constexpr int VEC = 8, LEVELS = 2;
  __device__ static constexpr int shift(int l) { return l == 0 ? 21 : 16; }
  __device__ static constexpr int bits(int l) { return l == 0 ? 11 : 5; }
  __device__ static __forceinline__ float one(const uint16_t* p) { return canonical(bf2f(*p)); }
  __device__ static __forceinline__ void vec(const uint16_t* p, float* out) {
    load8(p, out);
#pragma unroll
    for (int j = 0; j < VEC; ++j) out[j] = canonical(out[j]);
  }
};

template <>
struct Row<float> {
  static constexpr int VEC = 4, LEVELS = 3;
  __device__ static constexpr int shift(int l) { return l == 0 ? 21 : (l == 1 ? 10 : 0); }
  __device__ static constexpr int bits(int l) { return l == 2 ? 10 : 11; }
  __device__ static __forceinline__ float one(const float* p) { return canonical(*p); }
  __device__ static __forceinline__ void vec(const float* p, float* out) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < VEC; ++j) out[j] = canonical(v[j]);
  }
};

// A row as peeled head [0, h), nv whole 16-B vectors, and a tail up to V.
template <typename T>
struct Span {
  const T* row;
  int V, h, nv;
  __device__ int tail_begin() const { return h + nv * Row<T>::VEC; }
};

template <typename T>
__device__ __forceinline__ Span<T> make_span(const T* row, int V) {
  constexpr int VEC = Row<T>::VEC;
  const int mis = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) / (int)sizeof(T);
  Span<T> s;
  s.row = row;
  s.V = V;
  s.h = mis < V ? mis : V;
  s.nv = (V - s.h) / VEC;
  return s;
}

// f(index, canonical value) for every element of the row, in no particular order.
template <typename T, typename F>
__device__ __forceinline__ void for_all(const Span<T>& s, F f) {
  constexpr int VEC = Row<T>::VEC;
  const int tid = threadIdx.x;
  if (tid < s.h) f(tid, Row<T>::one(s.row + tid));
  const int t = s.tail_begin() + tid;
  if (t < s.V) f(t, Row<T>::one(s.row + t));
  for (int v = tid; v < s.nv; v += kThreads) {
    float x[VEC];
    const int i0 = s.h + v * VEC;
    Row<T>::vec(s.row + i0, x);
#pragma unroll
    for (int j = 0; j < VEC; ++j) f(i0 + j, x[j]);
  }
}

struct Weight {
  float M, inv_t, scale;
  // fixed-point mass of a canonical logit x <= M
  __device__ __forceinline__ u64 operator()(float x) const {
    if (x == -INFINITY) return 0;
    float w = x == M ? 1.f : __expf((x - M) * inv_t);
    w = w == w ? w : 0.f;
    return (u64)(w * scale);
  }
};

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = __shfl_xor(v, o, kWave);
    v = t > v ? t : v;
  }
  return v;
}

// Wave reduce, then a fixed-order sum of the wave results; `red` holds kWaves words.
template <bool MAX>
__device__ __forceinline__ u64 block_reduce(u64 v, u64* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  v = MAX ? wave_max_u64(v) : wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  u64 r = red[0];
#pragma unroll
  for (int i = 1; i < kWaves; ++i) r = MAX ? (red[i] > r ? red[i] : r) : r + red[i];
  return r;
}

__device__ __forceinline__ u64 wave_incl_scan(u64 v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const u64 t = __shfl_up(v, o, kWave);
    if (lane >= o) v += t;
  }
  return v;
}

__device__ __forceinline__ u64 block_excl_scan(u64 v, u64* red, u64& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const u64 incl = wave_incl_scan(v);
  __syncthreads();
  if (lane == kWave - 1) red[wid] = incl;
  __syncthreads();
  u64 base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    if (i < wid) base += red[i];
    total += red[i];
  }
  return base + incl - v;
}

// target = ceil(top_p * Z) clamped to [1, Z]; f64 holds Z < 2^63 to 2^-53, far below the masses' own error
__device__ __forceinline__ u64 mass_target(float top_p, u64 Z) {
  const double t = ceil((double)top_p * (double)Z);
  u64 r = t >= 9.2e18 ? Z : (u64)t;
  r = r < 1 ? 1 : r;
  return r > Z ? Z : r;
}

// Radix select from the top.  MASS = false: the key of the `target`-th largest element.  MASS = true:
// among the elements with key >= lo_key, the largest key t whose mass {key >= t} reaches
// top_p * (their total mass).  Every thread returns the same key.
template <typename T, bool MASS>
__device__ uint32_t radix_select(const Span<T>& s, const Weight& wt, uint32_t lo_key, u64 target, float top_p, u64* hist,
                                 u64* red, u64* bc) {
  using R = Row<T>;
  const int tid = threadIdx.x;
  uint32_t prefix = 0;
#pragma unroll
  for (int l = 0; l < R::LEVELS; ++l) {
    const int shift = R::shift(l);
    const uint32_t mask = (1u << R::bits(l)) - 1u;
    const int up = l ? R::shift(l - 1) : 32;  // bits at and above `up` are decided
    for (int b = tid; b < kBins; b += kThreads) hist[b] = 0;
    if (tid == 0) bc[0] = bc[1] = 0;
    __syncthreads();
    for_all(s, [&](int, float x) {
      const uint32_t k = key_of(x);
      if (k < lo_key) return;
      if (l && (k >> up) != (prefix >> up)) return;
      const u64 add = MASS ? wt(x) : 1ull;
      if (add) atomicAdd(&hist[(k >> shift) & mask], add);
    });
    __syncthreads();
    // thread t owns the kBinsPerThread bins below kBins - kBinsPerThread t, walked downwards
    u64 mine = 0;
#pragma unroll
    for (int j = 0; j < kBinsPerThread; ++j) mine += hist[kBins - 1 - (kBinsPerThread * tid + j)];
    u64 total;
    const u64 excl = block_excl_scan(mine, red, total);
    if (MASS && l == 0) target = mass_target(top_p, total);
    if (excl < target && target <= excl + mine) {
      u64 c = excl;
      for (int j = 0; j < kBinsPerThread; ++j) {
        const int b = kBins - 1 - (kBinsPerThread * tid + j);
        const u64 hb = hist[b];
        if (c + hb >= target) {
          bc[0] = (u64)b;
          bc[1] = c;
          break;
        }
        c += hb;
      }
    }
    __syncthreads();
    prefix |= ((uint32_t)bc[0] & mask) << shift;
    target -= bc[1];
    __syncthreads();  // every wave has read bc before thread 0 resets it for the next level / select
  }
  return prefix;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void sample_kernel(const T* __restrict__ logits, int64_t stride, int V,
                                                          const float* __restrict__ params,
                                                          const int* __restrict__ top_k,
                                                          const int64_t* __restrict__ rng, const float* __restrict__ u_in,
                                                          int64_t* __restrict__ ids, int* __restrict__ kept) {
  using R = Row<T>;
  constexpr int VEC = R::VEC;
  __shared__ u64 hist[kBins];
  __shared__ u64 red[kWaves];
  __shared__ u64 bc[4];
  __shared__ u64 wsum[kWaves];
  __shared__ int wcnt[kWaves], wlast[kWaves];

  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const Span<T> s = make_span(logits + (int64_t)r * stride, V);
  const float temp = params[3 * r], top_p = params[3 * r + 1], min_p = params[3 * r + 2];
  const int k = top_k[r];

  // ---- pass 1: max and its lowest index, packed {key, ~index} so that one max finds both
  u64 best = 0;
  for_all(s, [&](int i, float x) {
    const u64 c = ((u64)key_of(x) << 32) | (u64)(0xFFFFFFFFu - (uint32_t)i);
    best = c > best ? c : best;
  });
  best = block_reduce<true>(best, red);
  const uint32_t key_max = (uint32_t)(best >> 32);
  const int arg_max = (int)(0xFFFFFFFFu - (uint32_t)best);
  const uint32_t key_ninf = key_of(-INFINITY), key_pinf = key_of(INFINITY);
  if (key_max == key_ninf) {
    if (tid == 0) {
      ids[r] = -1;
      kept[r] = 0;
    }
    return;
  }
  if (key_max == key_pinf) {
    u64 c = 0;
    for_all(s, [&](int, float x) { c += key_of(x) == key_pinf; });
    c = block_reduce<false>(c, red);
    if (tid == 0) {
      ids[r] = arg_max;
      kept[r] = (int)c;
    }
    return;
  }
  if (!(temp > 0.f)) {  // T <= 0 or NaN: greedy
    if (tid == 0) {
      ids[r] = arg_max;
      kept[r] = 1;
    }
    return;
  }
  const uint32_t bm = (key_max & 0x80000000u) ? key_max ^ 0x80000000u : ~key_max;
  Weight wt;
  wt.M = __uint_as_float(bm);
  wt.inv_t = 1.f / temp;
  // 2^40 per id while V * 2^40 < 2^63; a longer row gets a coarser scale, never an overflow
  const int vbits = 32 - __clz(V);
  wt.scale = __uint_as_float((uint32_t)(127 + min(40, 62 - vbits)) << 23);

  // ---- thresholds, as keys (0 = filter off)
  uint32_t thr = 0;
  if (k > 0 && k < V) thr = radix_select<T, false>(s, wt, 0u, (u64)k, 0.f, hist, red, bc);
  if (top_p <= 0.f) {
    thr = key_max;
  } else if (top_p < 1.f) {
    const uint32_t tp = radix_select<T, true>(s, wt, thr, 0, top_p, hist, red, bc);
    thr = tp > thr ? tp : thr;
  }
  if (min_p > 0.f) {
    float tm = wt.M + temp * logf(min_p);  // w >= min_p  <=>  x >= M + T ln(min_p)
    if (tm == tm) {
      tm = canonical(fminf(tm, wt.M));
      const uint32_t km = key_of(tm);
      thr = km > thr ? km : thr;
    }
  }
  thr = thr > key_max ? key_max : thr;  // the argmax is always kept

  // ---- final pass A: kept mass, count and last kept index of each wave's slice of the body
  const int ntiles = (s.nv + kWave - 1) / kWave;
  const int tpw = (ntiles + kWaves - 1) / kWaves;
  const int tile0 = wid * tpw, tile1 = min(ntiles, tile0 + tpw);
  u64 msum = 0;
  int cnt = 0, last = -1;
  for (int t = tile0; t < tile1; ++t) {
    const int v = t * kWave + lane;
    if (v < s.nv) {
      float x[VEC];
      const int i0 = s.h + v * VEC;
      R::vec(s.row + i0, x);
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (key_of(x[j]) >= thr) {
          msum += wt(x[j]);
          ++cnt;
          last = i0 + j;
        }
    }
  }
  msum = wave_sum(msum);
  cnt = wave_sum(cnt);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, kWave));
  if (lane == 0) {
    wsum[wid] = msum;
    wcnt[wid] = cnt;
    wlast[wid] = last;
  }
  __syncthreads();

  // ---- thread 0: Z_K, the draw, and the region (head, a wave's slice, tail) of the crossing
  if (tid == 0) {
    u64 z = 0;
    int n_kept = 0, last_kept = -1;
    auto edge = [&](int i0, int i1, u64 base, u64 target, bool find) -> int {  // head / tail, serially
      for (int i = i0; i < i1; ++i) {
        const float x = R::one(s.row + i);
        if (key_of(x) < thr) continue;
        if (find) {
          base += wt(x);
          if (base > target) return i;
        } else {
          z += wt(x);
          ++n_kept;
          last_kept = i;
        }
      }
      return -1;
    };
    edge(0, s.h, 0, 0, false);
    const u64 z_head = z;
    for (int w = 0; w < kWaves; ++w) {
      z += wsum[w];
      n_kept += wcnt[w];
      last_kept = max(last_kept, wlast[w]);
    }
    const u64 z_body = z;
    edge(s.tail_begin(), V, 0, 0, false);

    float u;
    if (u_in) {
      u = u_in[r];
    } else {
      const uint32_t* g = reinterpret_cast<const uint32_t*>(rng + 3 * r);  // seed, stream, step: lo, hi each
      uint32_t c[4] = {g[4], g[5], g[2], g[3]};
      philox::rounds10(c, g[0], g[1]);
      u = (float)(c[0] >> 8) * 0x1p-24f;
    }
    u = u >= 0.f ? fminf(u, 1.f) : 0.f;
    // smallest i with cum_i > u Z_K  <=>  cum_i > floor(u Z_K), cum being an integer
    const double td = floor((double)u * (double)z);
    const u64 target = td >= 9.2e18 ? z : (u64)td;

    int found = -1, seg = -1;
    u64 base = 0;
    if (target < z_head) {
      found = edge(0, s.h, 0, target, true);
    } else if (target < z_body) {
      base = z_head;
      for (int w = 0; w < kWaves; ++w) {
        if (base + wsum[w] > target) {
          seg = w;
          break;
        }
        base += wsum[w];
      }
    } else if (target < z) {
      found = edge(s.tail_begin(), V, z_body, target, true);
    }
    kept[r] = n_kept;
    if (seg < 0) ids[r] = found >= 0 ? found : last_kept;  // no crossing left by rounding: the last kept id
    bc[0] = (u64)(int64_t)seg;
    bc[1] = base;
    bc[2] = target;
    bc[3] = (u64)(int64_t)last_kept;
  }
  __syncthreads();

  // ---- final pass B: the wave that owns the crossing walks its slice in index order
  const int seg = (int)(int64_t)bc[0];
  if (wid != seg) return;
  u64 base = bc[1];
  const u64 target = bc[2];
  for (int t = tile0; t < tile1; ++t) {
    const int v = t * kWave + lane;
    const int i0 = v < s.nv ? s.h + v * VEC : 0;
    u64 q[VEC];
    u64 mine = 0;
#pragma unroll
    for (int j = 0; j < VEC; ++j) q[j] = 0;
    if (v < s.nv) {
      float x[VEC];
      R::vec(s.row + i0, x);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        q[j] = key_of(x[j]) >= thr ? wt(x[j]) : 0ull;
        mine += q[j];
      }
    }
    const u64 incl = wave_incl_scan(mine);
    const u64 tile_sum = __shfl(incl, kWave - 1, kWave);
    if (base + tile_sum > target) {
      const u64 crossed = __ballot(base + incl > target);
      if (lane == __ffsll((long long)crossed) - 1) {
        u64 c = base + incl - mine;
        int id = i0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          c += q[j];
          if (c > target) {
            id = i0 + j;
            break;
          }
        }
        ids[r] = id;
      }
      return;
    }
    base += tile_sum;
  }
  if (lane == 0) ids[r] = (int64_t)bc[3];  // not reached: the slice's sum is exact
}

std::tuple<at::Tensor, at::Tensor> sample_logits(const at::Tensor& logits, const at::Tensor& params,
                                                 const at::Tensor& top_k, const at::Tensor& rng,
                                                 const c10::optional<at::Tensor>& u) {
  const char* name = "sample_logits";
  DTG_CHECK(logits.is_cuda() && logits.dim() == 2, name, ": logits must be a GPU tensor [n, V]");
  DTG_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat, name,
            ": logits must be bf16 or f32");
  const int64_t n = logits.size(0), V = logits.size(1);
  DTG_CHECK(V >= 1 && V < (int64_t(1) << 31), name, ": V must lie in [1, 2^31)");
  DTG_CHECK(n < (int64_t(1) << 31), name, ": too many rows");
  auto same = [&](const at::Tensor& t) { return t.is_cuda() && t.device() == logits.device() && t.is_contiguous(); };
  DTG_CHECK(same(params) && params.scalar_type() == at::kFloat && params.dim() == 2 && params.size(0) == n &&
                params.size(1) == 3, name, ": params must be a contiguous f32 [n, 3] on the logits' device");
  DTG_CHECK(same(top_k) && top_k.scalar_type() == at::kInt && top_k.dim() == 1 && top_k.size(0) == n, name,
            ": top_k must be a contiguous int32 [n] on the logits' device");
  DTG_CHECK(same(rng) && rng.scalar_type() == at::kLong && rng.dim() == 2 && rng.size(0) == n && rng.size(1) == 3,
            name, ": rng must be a contiguous int64 [n, 3] on the logits' device");
  if (u.has_value())
    DTG_CHECK(same(*u) && u->scalar_type() == at::kFloat && u->dim() == 1 && u->size(0) == n, name,
              ": u must be a contiguous f32 [n] on the logits' device");
  const c10::DeviceGuard g(logits.device());
  at::Tensor ids = at::empty({n}, logits.options().dtype(at::kLong));
  at::Tensor kept = at::empty({n}, logits.options().dtype(at::kInt));
  if (n == 0) return {ids, kept};
  DTG_CHECK(logits.stride(1) == 1 && (n == 1 || logits.stride(0) >= V), name,
            ": logits need unit inner stride and rows that do not overlap");
  const float* up = u.has_value() ? u->data_ptr<float>() : nullptr;
  if (logits.scalar_type() == at::kBFloat16) {
    sample_kernel<uint16_t><<<(unsigned)n, kThreads, 0, stream()>>>(
        bf16_ptr(logits), logits.stride(0), (int)V, params.data_ptr<float>(), top_k.data_ptr<int>(),
        rng.data_ptr<int64_t>(), up, ids.data_ptr<int64_t>(), kept.data_ptr<int>());
  } else {
    sample_kernel<float><<<(unsigned)n, kThreads, 0, stream()>>>(
        logits.data_ptr<float>(), logits.stride(0), (int)V, params.data_ptr<float>(), top_k.data_ptr<int>(),
        rng.data_ptr<int64_t>(), up, ids.data_ptr<int64_t>(), kept.data_ptr<int>());
  }
  DTG_LAUNCH_CHECK();
  return {ids, kept};
}

}  // namespace
}  // namespace dtg

TORCH_LIBRARY_IMPL(dtg, CUDA, m) { m.impl("sample_logits", dtg::sample_logits); }
