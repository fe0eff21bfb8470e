// Launch plan of the split-KV decode attention (csrc/kernels/decode_attn.hip): how many splits a
// call's keys are divided into, the chunk of keys one workgroup walks, the grid and the f32
// workspace of the partials, as a pure function of the call and the CU count.
// Plain C++17 with no HIP and no ATen, so the rules are pinned on a CPU
// (tests/native/decode_plan_check.cpp, run by tests/test_decode_plan_cpu.py).
//
// Keys are divided by ABSOLUTE position: split s of every sequence owns keys [s * chunk, (s + 1) * chunk),
// cut to the sequence's attended range [max(0, len - window), len).  A split can therefore be empty
// for a row (a short sequence beside a long one, splits before a sliding window's start); it then
// contributes a neutral partial.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace dtg {
namespace decode {

constexpr int kThreads = 256;    // 4 waves
constexpr int kKeyTile = 64;     // keys per workgroup iteration; a chunk is a multiple of it
constexpr int kMaxSplits = 64;   // hard cap: bounds the workspace and the combine's serial loop
constexpr int kMinChunk = 256;   // keys: a split pays the q load, the cross-wave merge and a partial
                                 // of G * (D + 2) floats; below this it would not be worth its share
constexpr int kWgsPerCu = 2;     // workgroups per CU the plan aims for before it stops splitting

inline bool head_dim_ok(int64_t D) { return D == 64 || D == 128; }
// group sizes G = nq / nkv the kernel is instantiated for (what the bundled configs need)
inline bool group_ok(int64_t G) { return G == 1 || G == 2 || G == 3 || G == 4 || G == 7 || G == 8 || G == 16; }

struct Call {
  int64_t B;        // sequences (one query token each)
  int nkv, G, D;    // kv heads, query heads per kv head, head dim
  int64_t max_len;  // host upper bound of lens[]
  int64_t window;   // 0 = all keys
  int cus;          // compute units of the device
  int splits;       // 0 = planned; > 0 overrides (tests reach the multi-split paths at tiny lengths)
};
struct Grid {
  unsigned x, y, z;
};
struct Plan {
  int splits;
  int64_t chunk;    // keys per split, a multiple of kKeyTile
  Grid grid;        // (split, kv head, sequence); launched flattened, split fastest
  size_t ws_bytes;  // f32 partials: per (sequence, kv head, split, query head) D outputs + max + sum; 0 at one split
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The length the splits must cover.  Splits are laid over absolute positions, so a window does not
// shorten it; the window only changes how many of a row's splits hold keys (below).
inline int64_t effective_len(const Call& c) { return std::max<int64_t>(c.max_len, 1); }

inline Plan plan(const Call& c) {
  const int64_t L = effective_len(c);
  int64_t splits = 1;
  if (c.splits > 0) {
    splits = std::min<int64_t>(c.splits, kMaxSplits);
  } else {
    const int64_t base = std::max<int64_t>(c.B * c.nkv, 1), target = (int64_t)kWgsPerCu * c.cus;
    if (base < target && L > kMinChunk) {
      int64_t want = ceil_div(target, base);  // busy workgroups wanted per (sequence, kv head)
      // with a sliding window only about window / L of a row's splits hold keys
      if (c.window > 0 && c.window < L) want = ceil_div(want * L, c.window);
      splits = std::min<int64_t>({want, ceil_div(L, kMinChunk), (int64_t)kMaxSplits});
    }
  }
  const int64_t chunk = ceil_div(ceil_div(L, splits), kKeyTile) * kKeyTile;
  if (c.splits <= 0) splits = ceil_div(L, chunk);  // rounding the chunk up may have emptied the last splits
  Plan p;
  p.splits = (int)splits;
  p.chunk = chunk;
  p.grid = {(unsigned)splits, (unsigned)c.nkv, (unsigned)c.B};
  p.ws_bytes = splits > 1 ? (size_t)c.B * c.nkv * splits * c.G * (c.D + 2) * sizeof(float) : 0;
  return p;
}

// decode_attn_multi: Q new tokens per sequence (speculative verification).  A workgroup serves a tile of
// q_tile(G) consecutive tokens of one sequence times the G query heads of its kv head, so a K / V piece
// is used G * q_tile(G) times.  16 (token, head) pairs per lane is what the G = 16 form of the
// one-token kernel already keeps in registers (16 x 8 q and 16 x 8 accumulators, 1 wave per SIMD).
constexpr int kMaxPairs = 16;
constexpr int q_tile(int G) {
  int qt = 1;
  while (qt < 8 && G * qt * 2 <= kMaxPairs) qt *= 2;
  return qt;
}

// Splits and chunk are plan(c)'s: c.B stays the number of sequences, so a token's keys are divided
// exactly as decode_attn divides them for that token alone with the same max_len and splits (the
// bitwise contract of decode_attn_multi).  Q only adds a query-tile dimension to the grid, folded into
// grid.z = sequence * ceil(Q / q_tile) + tile, and multiplies the partials, which are indexed with the
// token in the place of the sequence.
inline Plan plan_multi(const Call& c, int Q) {
  Plan p = plan(c);
  p.grid.z = (unsigned)(c.B * ceil_div(Q, q_tile(c.G)));
  p.ws_bytes *= (size_t)Q;
  return p;
}

}  // namespace decode
}  // namespace dtg
