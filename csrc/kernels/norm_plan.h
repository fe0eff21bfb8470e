// Integer launch rules of the norm kernels (rmsnorm.hip, layernorm.hip, qk_norm.hip): registers per
// lane, the backward's row split and the column-sum tile, as pure functions of the shape.
// Plain C++17 with no HIP and no ATen, so the rules are pinned on a CPU
// (tests/native/norm_plan_check.cpp, run by tests/test_norm_plan_cpu.py).
#pragma once

#include <algorithm>
#include <cstdint>

namespace dtg {
namespace norm {

constexpr int kThreads = 256;      // every norm kernel and the column sum
constexpr int kColsumCols = 16;    // columns per column-sum workgroup (x 16 row groups)
constexpr int kQkMaxBlocks = 1024; // QK-norm backward workgroups = rows of its dw partial matrix

// 16-byte chunks of a row each lane holds in registers (a row is H / 8 chunks over 256 lanes),
// rounded up to an instantiated PER; -1: the row does not fit (H > 16384).
inline int pick_per(int H) {
  const int per = (H / 8 + kThreads - 1) / kThreads;
  return per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : per <= 8 ? 8 : -1;
}

struct Split {
  int64_t per_block, n_blocks;  // rows (tokens) per backward workgroup; workgroups = partial rows
};
inline Split split(int64_t T, int64_t max_blocks) {
  const int64_t per = (T + std::min(T, max_blocks) - 1) / std::min(T, max_blocks);
  return {per, (T + per - 1) / per};
}

// RMSNorm / LayerNorm backward, T >= 1.  ~2 workgroups per CU worth of blocks keeps the partial
// matrices (and their column sum) small; the kernels' row pipelining provides the memory-level
// parallelism (2048 blocks measured 103 us + 84 us colsum vs 128 + 18 at 512 unpipelined,
// Llama-8B shape).
inline Split row_bwd_split(int T) { return split(T, 512); }
// QK-norm backward, T >= 1.
inline Split qk_bwd_split(int64_t T) { return split(T, kQkMaxBlocks); }

}  // namespace norm
}  // namespace dtg
