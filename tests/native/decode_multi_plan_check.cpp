// Pins the launch plan of decode_attn_multi (csrc/kernels/decode_attn_plan.h: q_tile, plan_multi) on a CPU.
// The query tile of every group size, and for the calls of tests/native/decode_plan_check.cpp at Q = 1, 3, 4
// and 16 tokens per sequence: the splits and the chunk of the one-token plan (the bitwise contract needs a
// token's keys divided exactly as decode_attn divides them), the grid with its query-tile dimension and the
// workspace.  Every expected value is a literal, never recomputed with the header's own functions.
// Built and run by tests/test_decode_multi_plan_cpu.py.
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

struct Row {
  const char* what;
  Call c;
  int splits;
  int64_t chunk;
  size_t ws;     // of one token per sequence
  int tile;      // q_tile(c.G)
};

int main() {
  const char* what = "q_tile";
  static_assert(kMaxPairs == 16, "constants");
  // the largest of 1, 2, 4, 8 with G * QT <= 16
  EXPECT(q_tile(1) == 8);
  EXPECT(q_tile(2) == 8);
  EXPECT(q_tile(3) == 4);
  EXPECT(q_tile(4) == 4);
  EXPECT(q_tile(7) == 2);
  EXPECT(q_tile(8) == 2);
  EXPECT(q_tile(16) == 1);

  // splits, chunk and one-token workspace: the literals of decode_plan_check.cpp
  const Row table[] = {
      {"b1 1k", Call{1, 8, 4, 128, 1024, 0, 256, 0}, 4, 256, 66560, 4},
      {"b1 8k", Call{1, 8, 4, 128, 8192, 0, 256, 0}, 32, 256, 532480, 4},
      {"b1 32k", Call{1, 8, 4, 128, 32768, 0, 256, 0}, 64, 512, 1064960, 4},
      {"b8 8k", Call{8, 8, 4, 128, 8192, 0, 256, 0}, 8, 1024, 1064960, 4},
      {"b8 1k", Call{8, 8, 4, 128, 1024, 0, 256, 0}, 4, 256, 532480, 4},
      {"b64 32k", Call{64, 8, 4, 128, 32768, 0, 256, 0}, 1, 32768, 0, 4},
      {"b64 1k", Call{64, 8, 4, 128, 1024, 0, 256, 0}, 1, 1024, 0, 4},
      {"b63 32k", Call{63, 8, 4, 128, 32768, 0, 256, 0}, 2, 16384, 2096640, 4},
      {"fits 256", Call{1, 8, 4, 128, 256, 0, 256, 0}, 1, 256, 0, 4},
      {"fits 1", Call{1, 8, 4, 128, 1, 0, 256, 0}, 1, 64, 0, 4},
      {"len 0", Call{1, 8, 4, 128, 0, 0, 256, 0}, 1, 64, 0, 4},
      {"just over", Call{1, 8, 4, 128, 257, 0, 256, 0}, 2, 192, 33280, 4},
      {"b8 2112", Call{8, 8, 4, 128, 2112, 0, 256, 0}, 7, 320, 931840, 4},
      {"b16 32k w4k", Call{16, 8, 4, 128, 32768, 4096, 256, 0}, 32, 1024, 8519680, 4},
      {"b1 32k w4k", Call{1, 8, 4, 128, 32768, 4096, 256, 0}, 64, 512, 1064960, 4},
      {"override 5", Call{5, 2, 2, 128, 65, 0, 256, 5}, 5, 64, 52000, 8},
      {"override 2", Call{5, 2, 2, 128, 65, 0, 256, 2}, 2, 64, 20800, 8},
      {"override 1", Call{1, 8, 4, 128, 32768, 0, 256, 1}, 1, 32768, 0, 4},
      {"override 3 of 300", Call{3, 2, 2, 128, 300, 64, 256, 3}, 3, 128, 18720, 8},
      {"override capped", Call{1, 1, 1, 64, 300, 0, 256, 100}, 64, 64, 16896, 8},
      {"g7 d64", Call{2, 4, 7, 64, 1024, 0, 256, 0}, 4, 256, 59136, 2},
      {"g1", Call{1, 12, 1, 64, 1024, 0, 256, 0}, 4, 256, 12672, 8},
      {"g16", Call{1, 8, 16, 128, 4096, 0, 256, 0}, 16, 256, 1064960, 1},
      {"g3", Call{2, 4, 3, 128, 1024, 0, 256, 0}, 4, 256, 49920, 4},
      {"g8", Call{2, 4, 8, 64, 1024, 0, 256, 0}, 4, 256, 67584, 2},
      {"32 cus", Call{1, 8, 4, 128, 8192, 0, 32, 0}, 8, 1024, 133120, 4},
  };
  for (const Row& r : table) {
    what = r.what;
    for (int Q : {1, 3, 4, 16}) {
      const Plan p = plan_multi(r.c, Q);
      EXPECT(p.splits == r.splits);
      EXPECT(p.chunk == r.chunk);
      EXPECT(p.ws_bytes == r.ws * (size_t)Q);
      const int tiles = (Q + r.tile - 1) / r.tile;
      EXPECT(p.grid.x == (unsigned)r.splits && p.grid.y == (unsigned)r.c.nkv);
      EXPECT(p.grid.z == (unsigned)(r.c.B * tiles));
    }
    // one token per sequence: the one-token plan itself
    const Plan a = plan_multi(r.c, 1), b = plan(r.c);
    EXPECT(a.splits == b.splits && a.chunk == b.chunk && a.ws_bytes == b.ws_bytes);
    EXPECT(a.grid.x == b.grid.x && a.grid.y == b.grid.y && a.grid.z == b.grid.z);
  }

  // grid and workspace, spelled out
  what = "literals";
  {
    // Llama-3-8B heads, 2 sequences x 4 tokens at 1k: tile 4 -> one query tile per sequence
    const Plan p = plan_multi(Call{2, 8, 4, 128, 1024, 0, 256, 0}, 4);
    EXPECT(p.splits == 4 && p.chunk == 256);
    EXPECT(p.grid.x == 4 && p.grid.y == 8 && p.grid.z == 2);
    EXPECT(p.ws_bytes == (size_t)8 * 8 * 4 * 4 * 130 * 4);  // 8 tokens, 8 kv heads, 4 splits, 4 heads, D + 2 floats
  }
  {
    // 5 tokens: two tiles of 4, the second with one real token
    const Plan p = plan_multi(Call{2, 8, 4, 128, 1024, 0, 256, 0}, 5);
    EXPECT(p.grid.x == 4 && p.grid.y == 8 && p.grid.z == 4);
    EXPECT(p.ws_bytes == (size_t)10 * 8 * 4 * 4 * 130 * 4);
  }
  {
    // Qwen2.5 heads (G 7, tile 2), 3 sequences x 8 tokens, the 512 bucket: 2 splits
    const Plan p = plan_multi(Call{3, 4, 7, 64, 512, 0, 256, 0}, 8);
    EXPECT(p.splits == 2 && p.chunk == 256);
    EXPECT(p.grid.x == 2 && p.grid.y == 4 && p.grid.z == 12);
    EXPECT(p.ws_bytes == (size_t)24 * 4 * 2 * 7 * 66 * 4);
  }
  {
    // G 16: tile 1, a workgroup per token; one split -> no workspace
    const Plan p = plan_multi(Call{1, 8, 16, 128, 200, 0, 256, 0}, 16);
    EXPECT(p.splits == 1 && p.chunk == 256 && p.ws_bytes == 0);
    EXPECT(p.grid.x == 1 && p.grid.y == 8 && p.grid.z == 16);
  }
  if (failures == 0) std::printf("OK\n");
  return failures != 0;
}
