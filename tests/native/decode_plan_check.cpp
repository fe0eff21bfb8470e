// Pins the split-KV decode attention launch plan (csrc/kernels/decode_attn_plan.h) on a CPU: for a
// table of calls, the split count, chunk, grid and workspace bytes the launcher gets.  Every expected
// value is a literal worked out from the rules (256 CUs -> 512 workgroups wanted, chunks of at least
// 256 keys in multiples of 64, at most 64 splits), never recomputed with the header's own functions.
// Built and run by tests/test_decode_plan_cpu.py.
#include <cstdio>

#include "kernels/decode_attn_plan.h"

using namespace dtg::decode;

static int failures = 0;

#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::printf("FAIL line %d [%s]: %s\n", __LINE__, what, #cond);          \
      ++failures;                                                             \
    }                                                                         \
  } while (0)

static void expect(const char* what, const Call& c, int splits, int64_t chunk, size_t ws) {
  const Plan p = plan(c);
  EXPECT(p.splits == splits);
  EXPECT(p.chunk == chunk);
  EXPECT(p.ws_bytes == ws);
  EXPECT(p.grid.x == (unsigned)splits && p.grid.y == (unsigned)c.nkv && p.grid.z == (unsigned)c.B);
  if (p.splits != splits || p.chunk != chunk || p.ws_bytes != ws)
    std::printf("  got splits %d chunk %lld ws %zu\n", p.splits, (long long)p.chunk, p.ws_bytes);
}

// Llama-3-8B head shape: nkv 8, G 4, D 128, on 256 CUs
static Call l8(int64_t B, int64_t max_len, int64_t window = 0, int splits = 0) {
  return Call{B, 8, 4, 128, max_len, window, 256, splits};
}

int main() {
  static_assert(kKeyTile == 64 && kMaxSplits == 64 && kMinChunk == 256 && kWgsPerCu == 2 && kThreads == 256, "constants");
  // batch 1: 8 workgroups per split -> 64 splits wanted; the 256-key minimum chunk, then the cap, bind
  expect("b1 1k", l8(1, 1024), 4, 256, 66560);
  expect("b1 8k", l8(1, 8192), 32, 256, 532480);
  expect("b1 32k", l8(1, 32768), 64, 512, 1064960);
  // batch 8: 64 workgroups -> 8 splits
  expect("b8 8k", l8(8, 8192), 8, 1024, 8 * 532480 / 4);
  expect("b8 1k", l8(8, 1024), 4, 256, 8 * 66560);
  // B * nkv already fills the machine (512 workgroups): one split, no workspace, whatever the length
  expect("b64 32k", l8(64, 32768), 1, 32768, 0);
  expect("b64 1k", l8(64, 1024), 1, 1024, 0);
  expect("b63 32k", l8(63, 32768), 2, 16384, 63 * 8 * 2 * 4 * 130 * 4);
  // the length fits one chunk
  expect("fits 256", l8(1, 256), 1, 256, 0);
  expect("fits 200", l8(1, 200), 1, 256, 0);
  expect("fits 1", l8(1, 1), 1, 64, 0);
  expect("len 0", l8(1, 0), 1, 64, 0);
  expect("just over", l8(1, 257), 2, 192, 1 * 8 * 2 * 4 * 130 * 4);
  // rounding the chunk up to the key tile empties the last split: 2112 keys, 8 wanted -> 320-key chunks -> 7
  expect("b8 2112", l8(8, 2112), 7, 320, 8 * 8 * 7 * 4 * 130 * 4);
  // sliding window: only window / max_len of a row's splits hold keys, so more are made
  expect("b16 32k", l8(16, 32768), 4, 8192, 16 * 8 * 4 * 4 * 130 * 4);
  expect("b16 32k w4k", l8(16, 32768, 4096), 32, 1024, 16 * 8 * 32 * 4 * 130 * 4);
  expect("b1 32k w4k", l8(1, 32768, 4096), 64, 512, 1064960);
  expect("window >= len", l8(16, 4096, 8192), 4, 1024, 16 * 8 * 4 * 4 * 130 * 4);
  // the override: taken as given (trailing splits may be empty), capped, the chunk still covers the length
  expect("override 5", Call{5, 2, 2, 128, 65, 0, 256, 5}, 5, 64, 52000);
  expect("override 2", Call{5, 2, 2, 128, 65, 0, 256, 2}, 2, 64, 5 * 2 * 2 * 2 * 130 * 4);
  expect("override 1", l8(1, 32768, 0, 1), 1, 32768, 0);
  expect("override 3 of 300", Call{3, 2, 2, 128, 300, 64, 256, 3}, 3, 128, 3 * 2 * 3 * 2 * 130 * 4);
  expect("override capped", Call{1, 1, 1, 64, 300, 0, 256, 100}, 64, 64, 64 * 66 * 4);
  // other shapes: Qwen2.5 (G 7, D 64), GPT-2-like nq == nkv, Llama-3.1-405B (G 16)
  expect("g7 d64", Call{2, 4, 7, 64, 1024, 0, 256, 0}, 4, 256, 59136);
  expect("g1", Call{1, 12, 1, 64, 1024, 0, 256, 0}, 4, 256, 12 * 4 * 66 * 4);
  expect("g16", Call{1, 8, 16, 128, 4096, 0, 256, 0}, 16, 256, 8 * 16 * 16 * 130 * 4);
  // fewer CUs: 32 -> 64 workgroups wanted
  expect("32 cus", Call{1, 8, 4, 128, 8192, 0, 32, 0}, 8, 1024, 8 * 8 * 4 * 130 * 4);

  // invariants over a sweep
  const char* what = "sweep";
  for (int64_t B : {1, 3, 8, 64, 1000})
    for (int nkv : {1, 8})
      for (int64_t L : {0, 1, 63, 64, 65, 255, 256, 257, 1000, 4097, 32768, 131072})
        for (int64_t w : {0, 64, 4096})
          for (int s : {0, 1, 3, 64, 65}) {
            const Plan p = plan(Call{B, nkv, 4, 128, L, w, 256, s});
            EXPECT(p.splits >= 1 && p.splits <= kMaxSplits);
            EXPECT(p.chunk > 0 && p.chunk % kKeyTile == 0);
            EXPECT((int64_t)p.splits * p.chunk >= L);
            EXPECT(s > 0 || B * nkv < 512 || p.splits == 1);
            EXPECT(s > 0 || L > 256 || p.splits == 1);
            EXPECT(s > 0 || (int64_t)(p.splits - 1) * p.chunk < (L > 1 ? L : 1));  // no planned split is wholly past the end
            EXPECT((p.ws_bytes == 0) == (p.splits == 1));
          }
  if (failures == 0) std::printf("OK\n");
  return failures != 0;
}
