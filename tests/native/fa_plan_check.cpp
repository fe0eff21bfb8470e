// Pins the flash-attention launch plan (csrc/kernels/flash_attn_plan.h) on a CPU: for a table of
// calls and tuning knobs, the kernel variant, template arguments, grid, split and dynamic-LDS
// bytes each launcher gets.  Every expected value is a literal worked out from the rules, never
// recomputed with the header's own functions.  Built and run by tests/test_fa_plan_cpu.py.
#include <cstdio>
#include <cstring>

#include "kernels/flash_attn_plan.h"

using namespace dtg::fa;

static int failures = 0;

#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::printf("FAIL line %d [%s]: %s\n", __LINE__, what, #cond);          \
      ++failures;                                                             \
    }                                                                         \
  } while (0)

static const Variant PLAIN = Variant::PLAIN, WIN = Variant::WIN, DROP = Variant::DROP;

// hq 4, hkv 2, 4 sequences of up to 130 tokens: 2 query blocks, 2 key blocks, 16 dK/dV workgroups.
static Call call(int D, bool causal, int64_t window = 0, bool drop = false, bool key_ranges = false) {
  return Call{D, causal, window, drop, key_ranges, false, 4, 2, 4, 130, 130};
}

static void expect_grid(const char* what, const Grid& g, unsigned x, unsigned y, unsigned z) {
  EXPECT(g.x == x && g.y == y && g.z == z);
}

static void expect_fwd(const char* what, const Call& c, Variant var, bool causal, size_t lds) {
  const FwdPlan p = plan_fwd(c);
  EXPECT(p.var == var);
  EXPECT(p.causal == causal);
  EXPECT(p.lds == lds);
  expect_grid(what, p.grid, 4, 4, 2);
}

static void expect_dq(const char* what, const Call& c, const Tuning& t, Variant var, bool causal, int occ, size_t lds) {
  const DqPlan p = plan_dq(c, t);
  EXPECT(p.var == var);
  EXPECT(p.causal == causal);
  EXPECT(p.occ == occ);
  EXPECT(p.lds == lds);
  expect_grid(what, p.grid, 4, 4, 2);
}

static void expect_kv(const char* what, const Call& c, const Tuning& t, Variant var, bool causal, int pf, int qb,
                      int nsplit, unsigned gz, size_t lds) {
  const KvPlan p = plan_kv(c, t);
  EXPECT(p.var == var);
  EXPECT(p.causal == causal);
  EXPECT(p.pf == pf);
  EXPECT(p.qb == qb);
  EXPECT(p.nsplit == nsplit);
  EXPECT(p.lds == lds);
  expect_grid(what, p.grid, (unsigned)c.hkv, (unsigned)c.nseq, gz);
}

static void expect_conflict(const char* what, const Call& c, const char* msg) {
  const char* got = conflict(c);
  EXPECT((msg == nullptr) == (got == nullptr));
  if (msg != nullptr && got != nullptr) EXPECT(std::strcmp(got, msg) == 0);
}

int main() {
  const Tuning dflt{0, 64, 1, 1};  // kv_split auto, kv_qb 64, dq_occ 1, kv_pf 1
  const char* what = "constants";
  EXPECT(kFwdBQ == 128 && kFwdBK == 64 && kDqBQ == 128 && kDqBK == 64 && kKvBK == 128 && kKvBQ == 32);
  EXPECT(fwd_lds_bytes(64) == 32768 && fwd_lds_bytes(128) == 65536);
  EXPECT(dq_lds_bytes(64) == 33280 && dq_lds_bytes(128) == 66048);
  EXPECT(kv_lds_bytes(64, 32) == 16896 && kv_lds_bytes(128, 32) == 33280);
  EXPECT(kv_lds_bytes(64, 64) == 33792 && kv_lds_bytes(128, 64) == 66560);

  // ---- forward: <D, causal, WIN, DROP>, grid (hq, nseq, ceil(130 / 128)), 512 * D bytes
  expect_fwd("fwd 128 causal", call(128, true), PLAIN, true, 65536);
  expect_fwd("fwd 128 non-causal", call(128, false), PLAIN, false, 65536);
  expect_fwd("fwd 64 causal", call(64, true), PLAIN, true, 32768);
  expect_fwd("fwd 64 non-causal", call(64, false), PLAIN, false, 32768);
  expect_fwd("fwd 128 window", call(128, true, 64), WIN, true, 65536);
  expect_fwd("fwd 64 window", call(64, true, 64), WIN, true, 32768);
  expect_fwd("fwd 128 window non-causal", call(128, false, 64), PLAIN, false, 65536);
  expect_fwd("fwd 128 dropout causal", call(128, true, 0, true), DROP, true, 65536);
  expect_fwd("fwd 64 dropout non-causal", call(64, false, 0, true), DROP, false, 32768);
  expect_fwd("fwd 128 key ranges", call(128, true, 0, false, true), PLAIN, true, 65536);
  {
    what = "fwd grid edges";
    Call c = call(128, true);
    c.max_seqlen = 128;
    EXPECT(plan_fwd(c).grid.z == 1);
    c.max_seqlen = 129;
    EXPECT(plan_fwd(c).grid.z == 2);
    c.max_seqlen = 1;
    EXPECT(plan_fwd(c).grid.z == 1);
  }

  // ---- dQ: <D, causal, OCC, WIN, DROP>, 512 * D + 512 bytes; OCC 2 at D 64, at D 128 only PLAIN with dq_occ 2
  const Tuning occ2{0, 64, 2, 1};
  expect_dq("dq 128 causal", call(128, true), dflt, PLAIN, true, 1, 66048);
  expect_dq("dq 128 non-causal", call(128, false), dflt, PLAIN, false, 1, 66048);
  expect_dq("dq 64 causal", call(64, true), dflt, PLAIN, true, 2, 33280);
  expect_dq("dq 64 non-causal", call(64, false), dflt, PLAIN, false, 2, 33280);
  expect_dq("dq 128 causal occ 2", call(128, true), occ2, PLAIN, true, 2, 66048);
  expect_dq("dq 128 non-causal occ 2", call(128, false), occ2, PLAIN, false, 2, 66048);
  expect_dq("dq 64 occ 2", call(64, true), occ2, PLAIN, true, 2, 33280);
  expect_dq("dq 128 window", call(128, true, 64), dflt, WIN, true, 1, 66048);
  expect_dq("dq 128 window occ 2", call(128, true, 64), occ2, WIN, true, 1, 66048);
  expect_dq("dq 64 window", call(64, true, 64), dflt, WIN, true, 2, 33280);
  expect_dq("dq 128 window non-causal occ 2", call(128, false, 64), occ2, PLAIN, false, 2, 66048);
  expect_dq("dq 128 dropout", call(128, true, 0, true), dflt, DROP, true, 1, 66048);
  expect_dq("dq 128 dropout occ 2", call(128, false, 0, true), occ2, DROP, false, 1, 66048);
  expect_dq("dq 64 dropout", call(64, true, 0, true), dflt, DROP, true, 2, 33280);
  expect_dq("dq 128 key ranges", call(128, true, 0, false, true), dflt, PLAIN, true, 1, 66048);

  // ---- dK/dV: <D, causal, PF, WIN, QB, DROP>, grid (hkv, nseq, nkb * nsplit), 8 * qb * D + 16 * qb bytes.
  // The default call has wgs = 2 * 4 * 2 = 16: auto split min(4, ceil(512 / 16)) = 4, grid z = 2 * 4.
  expect_kv("kv 128 causal", call(128, true), dflt, PLAIN, true, 1, 64, 4, 8, 66560);
  expect_kv("kv 128 non-causal", call(128, false), dflt, PLAIN, false, 1, 64, 4, 8, 66560);
  expect_kv("kv 64 causal", call(64, true), dflt, PLAIN, true, 1, 64, 4, 8, 33792);
  expect_kv("kv 64 non-causal", call(64, false), dflt, PLAIN, false, 1, 64, 4, 8, 33792);
  const Tuning qb32{0, 32, 1, 1}, pf2{0, 64, 1, 2}, pf2qb32{0, 32, 1, 2};
  expect_kv("kv 128 qb 32", call(128, true), qb32, PLAIN, true, 1, 32, 4, 8, 33280);
  expect_kv("kv 64 qb 32", call(64, false), qb32, PLAIN, false, 1, 32, 4, 8, 16896);
  expect_kv("kv 128 pf 2: no split, qb 32", call(128, true), pf2, PLAIN, true, 2, 32, 1, 2, 33280);
  expect_kv("kv 64 pf 2 non-causal", call(64, false), pf2, PLAIN, false, 2, 32, 1, 2, 16896);
  expect_kv("kv 128 pf 2 qb 32", call(128, false), pf2qb32, PLAIN, false, 2, 32, 1, 2, 33280);
  expect_kv("kv 128 window: no split, qb 32", call(128, true, 64), dflt, WIN, true, 1, 32, 1, 2, 33280);
  expect_kv("kv 64 window", call(64, true, 64), dflt, WIN, true, 1, 32, 1, 2, 16896);
  expect_kv("kv 128 window pf 2", call(128, true, 64), pf2, WIN, true, 1, 32, 1, 2, 33280);
  expect_kv("kv 128 window non-causal", call(128, false, 64), dflt, PLAIN, false, 1, 64, 4, 8, 66560);
  expect_kv("kv 128 key ranges: no split", call(128, true, 0, false, true), dflt, PLAIN, true, 1, 64, 1, 2, 66560);
  expect_kv("kv 64 key ranges qb 32", call(64, false, 0, false, true), qb32, PLAIN, false, 1, 32, 1, 2, 16896);
  // key ranges never take the two-ahead prefetch (a range with keys and no queries has zero items)
  expect_kv("kv 128 key ranges pf 2: PF 1, qb 32", call(128, true, 0, false, true), pf2, PLAIN, true, 1, 32, 1, 2, 33280);
  expect_kv("kv 64 key ranges pf 2 non-causal", call(64, false, 0, false, true), pf2qb32, PLAIN, false, 1, 32, 1, 2, 16896);
  expect_kv("kv 128 dropout", call(128, true, 0, true), dflt, DROP, true, 1, 64, 4, 8, 66560);
  expect_kv("kv 64 dropout non-causal", call(64, false, 0, true), dflt, DROP, false, 1, 64, 4, 8, 33792);
  expect_kv("kv 128 dropout qb 32", call(128, true, 0, true), qb32, DROP, true, 1, 64, 4, 8, 66560);
  expect_kv("kv 128 dropout pf 2: split, qb 64, PF 1", call(128, true, 0, true), pf2, DROP, true, 1, 64, 4, 8, 66560);
  expect_kv("kv 64 dropout pf 2", call(64, false, 0, true), pf2, DROP, false, 1, 64, 4, 8, 33792);

  // forced split: kv_split 1 = off, 4, 9 clamps to 8; suppressed like the automatic one
  const Tuning s1{1, 64, 1, 1}, s4{4, 64, 1, 1}, s9{9, 64, 1, 1}, s4pf2{4, 64, 1, 2};
  expect_kv("kv split 1", call(128, true), s1, PLAIN, true, 1, 64, 1, 2, 66560);
  expect_kv("kv split 4", call(128, true), s4, PLAIN, true, 1, 64, 4, 8, 66560);
  expect_kv("kv split 9", call(128, true), s9, PLAIN, true, 1, 64, 8, 16, 66560);
  expect_kv("kv split 4 window", call(128, true, 64), s4, WIN, true, 1, 32, 1, 2, 33280);
  expect_kv("kv split 4 key ranges", call(128, true, 0, false, true), s4, PLAIN, true, 1, 64, 1, 2, 66560);
  expect_kv("kv split 4 pf 2", call(128, true), s4pf2, PLAIN, true, 2, 32, 1, 2, 33280);
  expect_kv("kv split 4 dropout pf 2", call(128, true, 0, true), s4pf2, DROP, true, 1, 64, 4, 8, 66560);
  {
    // automatic split by workgroup count: the key blocks come from max_seqlen_k, not max_seqlen
    Call c = call(128, true);
    c.hkv = 7, c.nseq = 73, c.max_seqlen_k = 128;  // wgs 511 -> ceil(512 / 511) = 2
    expect_kv("kv wgs 511", c, dflt, PLAIN, true, 1, 64, 2, 2, 66560);
    c.hkv = 8, c.nseq = 64;  // wgs 512 -> no split
    expect_kv("kv wgs 512", c, dflt, PLAIN, true, 1, 64, 1, 1, 66560);
    expect_kv("kv wgs 512 split 4", c, s4, PLAIN, true, 1, 64, 4, 4, 66560);
    c.hkv = 2, c.nseq = 100;  // wgs 200 -> ceil(512 / 200) = 3
    expect_kv("kv wgs 200", c, dflt, PLAIN, true, 1, 64, 3, 3, 66560);
    c.max_seqlen_k = 0;  // wgs 0 -> no split (and an empty grid)
    expect_kv("kv wgs 0", c, dflt, PLAIN, true, 1, 64, 1, 0, 66560);
    c = call(64, false);
    c.max_seqlen_k = 300;  // 3 key blocks: wgs 24 -> min(4, 22) = 4
    expect_kv("kv max_seqlen_k 300", c, dflt, PLAIN, false, 1, 64, 4, 12, 33792);
    what = "dq ignores max_seqlen_k";
    EXPECT(plan_dq(c, dflt).grid.z == 2);
  }

  // ---- combinations that stay errors
  const char* kDropMsg = "flash_attn dropout: no sliding window / key ranges";
  const char* kRopeMsg = "flash_attn rope: self-attention without dropout only";
  expect_conflict("plain", call(128, true), nullptr);
  expect_conflict("window", call(128, true, 64), nullptr);
  expect_conflict("key ranges", call(128, true, 0, false, true), nullptr);
  expect_conflict("dropout", call(128, true, 0, true), nullptr);
  expect_conflict("dropout + window", call(128, true, 64, true), kDropMsg);
  expect_conflict("dropout + window, non-causal", call(128, false, 64, true), nullptr);
  expect_conflict("dropout + key ranges", call(128, true, 0, true, true), kDropMsg);
  Call r = call(128, true, 64);
  r.rope = true;
  expect_conflict("rope + window", r, nullptr);
  r.key_ranges = true;
  expect_conflict("rope + key ranges", r, kRopeMsg);
  r.key_ranges = false, r.drop = true;
  expect_conflict("rope + dropout", r, kRopeMsg);

  if (failures == 0) std::printf("OK\n");
  return failures == 0 ? 0 : 1;
}
