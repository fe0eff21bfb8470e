// Launch plan of the flash-attention kernels (csrc/kernels/flash_attn.hip): which instantiation,
// grid and dynamic-LDS size a call gets, as pure functions of the call and the tuning knobs.
// Plain C++17 with no HIP and no ATen, so the rules are pinned on a CPU
// (tests/native/fa_plan_check.cpp, run by tests/test_fa_plan_cpu.py).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace dtg {
namespace fa {

constexpr int kFwdBQ = 128;  // forward: query rows per work item (4 waves x 32)
constexpr int kFwdBK = 64;   // forward: keys per K/V tile
constexpr int kDqBQ = 128;   // dQ: query rows per workgroup (4 waves x 32)
constexpr int kDqBK = 64;    // dQ: keys per K/V tile
constexpr int kKvBK = 128;   // dK/dV: keys per workgroup (4 waves x 32)
constexpr int kKvBQ = 32;    // dK/dV: query rows per item

// Dynamic LDS in bytes: two K/V tile pairs of bf16 (+ the per-row delta in dQ); dK/dV holds two
// sets of Q/dO slices of `qb` rows plus their lse / delta.
constexpr size_t fwd_lds_bytes(int D) { return 4 * (size_t)kFwdBK * D * 2; }
constexpr size_t dq_lds_bytes(int D) { return 4 * (size_t)kDqBK * D * 2 + kDqBQ * 4; }
constexpr size_t kv_lds_bytes(int D, int qb) { return 4 * (size_t)qb * D * 2 + 2 * 2 * qb * 4; }

// Backward launch knobs (DTG_FA_KV_SPLIT, DTG_FA_KV_QB, DTG_FA_OCC, DTG_FA_KV_PF; see flash_attn.hip).
struct Tuning {
  int kv_split, kv_qb, dq_occ, kv_pf;
};
// What one attention call asks for.
struct Call {
  int D;
  bool causal;
  int64_t window;  // as passed; it takes effect on causal calls only (window_eff)
  bool drop, key_ranges, rope;
  int hq, hkv, nseq;
  int64_t max_seqlen, max_seqlen_k;
};
enum class Variant { PLAIN, WIN, DROP };
struct Grid {
  unsigned x, y, z;
};
struct Plan {  // every launch: <D, causal> x variant, grid and dynamic LDS bytes
  Variant var;
  bool causal;
  Grid grid;
  size_t lds;
};
using FwdPlan = Plan;   // fwd_kernel<D, causal, WIN, DROP>
struct DqPlan : Plan {  // bwd_dq_kernel<D, causal, occ, WIN, DROP>
  int occ;
};
struct KvPlan : Plan {  // bwd_dkdv_kernel<D, causal, pf, WIN, qb, DROP>, then the combine if nsplit > 1
  int pf, qb, nsplit;
};

inline int window_eff(const Call& c) { return c.causal ? (int)c.window : 0; }
inline Variant variant(const Call& c) {
  return c.drop ? Variant::DROP : window_eff(c) > 0 ? Variant::WIN : Variant::PLAIN;
}
// Combinations no kernel implements: the error message, or nullptr.
inline const char* conflict(const Call& c) {
  if (c.rope && (c.key_ranges || c.drop)) return "flash_attn rope: self-attention without dropout only";
  if (c.drop && (window_eff(c) != 0 || c.key_ranges)) return "flash_attn dropout: no sliding window / key ranges";
  return nullptr;
}
inline unsigned nblocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

inline FwdPlan plan_fwd(const Call& c) {
  return {variant(c), c.causal, {(unsigned)c.hq, (unsigned)c.nseq, nblocks(c.max_seqlen, kFwdBQ)}, fwd_lds_bytes(c.D)};
}
// dQ runs two waves per SIMD at head_dim 64; at 128 only the plain kernels have that form (Tuning::dq_occ).
inline DqPlan plan_dq(const Call& c, const Tuning& t) {
  const Variant var = variant(c);
  const int occ = c.D == 64 || (var == Variant::PLAIN && t.dq_occ == 2) ? 2 : 1;
  return {{var, c.causal, {(unsigned)c.hq, (unsigned)c.nseq, nblocks(c.max_seqlen, kDqBQ)}, dq_lds_bytes(c.D)}, occ};
}

inline KvPlan plan_kv(const Call& c, const Tuning& t) {
  const Variant var = variant(c);
  // Items staged ahead (Tuning::kv_pf).  Equal on MI355X once the kernel's false vmcnt waits were
  // gone (bwd 0.767 vs 0.768 ms at the 8B shape, profiles/r1_s51_*), so the single-set form with
  // fewer registers is the default; dropout and sliding windows have only that form.  Key ranges
  // take it too: a range with keys but no queries (context parallelism emits them) gives a key
  // block zero items, and the two-ahead prologue loads items 0 and 1 unconditionally -- item
  // indices it divides by the per-head item count, 0 there.  The single-set loop loads nothing.
  const int pf = var == Variant::PLAIN && !c.key_ranges ? t.kv_pf : 1;
  // Query rows per item (Tuning::kv_qb).  64 (the two-half software pipeline) is the default:
  // backward 2-4 % faster on every benchmarked shape, -1.9 ms per 8B step (profiles/r3_s39).
  // Dropout always uses it; sliding windows and the two-item prefetch keep 32.
  const int qb = c.drop || (t.kv_qb != 32 && window_eff(c) == 0 && t.kv_pf == 1) ? 64 : 32;
  // Split the query items of each key block over several workgroups when the grid cannot fill
  // the chip (e.g. TP = 8: one KV head per rank -> 16 x 8 workgroups for 256 CUs): aim for
  // >= 2 workgroups per CU.  Tuning::kv_split = N forces N (1 = off).  No split form: key ranges, WIN, PF 2.
  const unsigned nkb = nblocks(c.max_seqlen_k, kKvBK);
  const int64_t wgs = (int64_t)c.hkv * c.nseq * nkb;
  int nsplit = 1;
  if (t.kv_split > 0) nsplit = std::min(8, t.kv_split);
  else if (wgs > 0 && wgs < 512) nsplit = (int)std::min<int64_t>(4, (512 + wgs - 1) / wgs);
  if (c.key_ranges || window_eff(c) != 0 || (c.drop ? 1 : t.kv_pf) != 1) nsplit = 1;
  return {{var, c.causal, {(unsigned)c.hkv, (unsigned)c.nseq, nkb * nsplit}, kv_lds_bytes(c.D, qb)}, pf, qb, nsplit};
}

}  // namespace fa
}  // namespace dtg
