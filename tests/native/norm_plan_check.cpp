// Pins the integer launch rules of the norm kernels (csrc/kernels/norm_plan.h) on a CPU: registers
// per lane, the two backward splits and the constants.  Every expected value is a literal, never
// recomputed with the header's own functions.  Built and run by tests/test_norm_plan_cpu.py.
#include <cstdio>

#include "kernels/norm_plan.h"

using namespace dtg::norm;

static int failures = 0;

#define EXPECT(cond)                                                 \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAIL line %d [%s]: %s\n", __LINE__, what, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static void expect_split(const char* what, const Split& s, int64_t per_block, int64_t n_blocks) {
  EXPECT(s.per_block == per_block);
  EXPECT(s.n_blocks == n_blocks);
}

int main() {
  const char* what = "constants";
  EXPECT(kThreads == 256 && kColsumCols == 16 && kQkMaxBlocks == 1024);

  what = "pick_per";  // a row is H / 8 chunks over 256 lanes: 2048 columns per PER
  EXPECT(pick_per(8) == 1);
  EXPECT(pick_per(2048) == 1);
  EXPECT(pick_per(2056) == 2);
  EXPECT(pick_per(4096) == 2);
  EXPECT(pick_per(4104) == 4);
  EXPECT(pick_per(8192) == 4);
  EXPECT(pick_per(8200) == 8);
  EXPECT(pick_per(16384) == 8);
  EXPECT(pick_per(16392) == -1);

  // (rows per block, blocks): at most 512 blocks, none of them empty, the last one possibly short
  expect_split("row split T 1", row_bwd_split(1), 1, 1);
  expect_split("row split T 512", row_bwd_split(512), 1, 512);
  expect_split("row split T 513", row_bwd_split(513), 2, 257);
  expect_split("row split T 1025", row_bwd_split(1025), 3, 342);
  expect_split("row split T 1537", row_bwd_split(1537), 4, 385);
  expect_split("row split T 16384", row_bwd_split(16384), 32, 512);

  // (tokens per block, blocks): at most 1024 blocks
  expect_split("qk split T 1", qk_bwd_split(1), 1, 1);
  expect_split("qk split T 1024", qk_bwd_split(1024), 1, 1024);
  expect_split("qk split T 1025", qk_bwd_split(1025), 2, 513);
  expect_split("qk split T 1031", qk_bwd_split(1031), 2, 516);

  if (failures == 0) std::printf("OK\n");
  return failures == 0 ? 0 : 1;
}
