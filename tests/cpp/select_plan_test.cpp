// Host-only check of tostore_amd/csrc/tsh_select_plan.h: which instantiation of the K2 select a search takes and every
// path predicate of the kernel, on both sides of each edge.  Prints "select plan ok"; exit status 1 on a miss.
#include <cstdio>

#include "../../tostore_amd/csrc/tsh_select_plan.h"

using namespace tsh;

static int fails = 0;
#define CHECK(cond, ...)      \
  do {                        \
    if (!(cond)) {            \
      printf("MISS: ");       \
      printf(__VA_ARGS__);    \
      printf("\n");           \
      ++fails;                \
    }                         \
  } while (0)

int main() {
  static_assert(SEL_THREADS == 1024 && SEL_VPT == 16 && SEL_LIST_CAP == 4096 && SEL_PREFILTER_MIN == 512, "the four constants");
  static_assert(SEL_THREADS % 64 == 0 && SEL_THREADS_SMALL % 64 == 0, "whole waves");
  static_assert(SEL_LIST_CAP % 64 == 0 && SEL_SHORT_SMALL % 64 == 0, "the short list is bisected as whole values per lane");
  static_assert(SEL_SMALL_REGS_TILES == SEL_THREADS_SMALL / 64 * SEL_REFINE_RV, "what four waves hold in registers");

  // ---- the variant -------------------------------------------------------------------------------------------------
  // tiles 64 / 65: nothing changes for k <= tiles; fewer tiles than k (all hit) leaves the four waves above 64 tiles
  CHECK(select_variant(64, 10, false) == SEL_NT256_REGS && select_variant(65, 10, false) == SEL_NT256_REGS, "k = 10 at 64 / 65 tiles");
  CHECK(select_variant(64, 100, false) == SEL_NT256_REGS && select_variant(65, 100, false) == SEL_NT1024_REGS, "all hit at 64 / 65 tiles");
  CHECK(select_variant(65, 65, false) == SEL_NT256_REGS && select_variant(65, 66, false) == SEL_NT1024_REGS, "all hit at k = M / M + 1");
  // a list scan leaves them above 64 tiles whatever k
  CHECK(select_variant(64, 10, true) == SEL_NT256_REGS && select_variant(65, 10, true) == SEL_NT1024_REGS, "a list scan at 64 / 65 tiles");
  CHECK(select_variant(21, 1301, true) == SEL_NT1024_REGS && select_variant(21, 100, true) == SEL_NT256_REGS, "a list scan of 21 tiles");
  // tiles 512 / 513, k 256 / 257
  CHECK(select_variant(512, 10, false) == SEL_NT256_REGS && select_variant(513, 10, false) == SEL_NT1024_REGS, "512 / 513 tiles");
  CHECK(select_variant(512, 256, false) == SEL_NT256_REGS && select_variant(512, 257, false) == SEL_NT1024_REGS, "k = 256 / 257");
  CHECK(select_variant(1, 1, false) == SEL_NT256_REGS && select_variant(1, 257, false) == SEL_NT1024_REGS, "one tile");
  // tiles 16384 / 16385
  CHECK(select_variant(16384, 100, false) == SEL_NT1024_REGS && select_variant(16385, 100, false) == SEL_NT1024_MEM, "16384 / 16385 tiles");
  CHECK(select_variant(16384, 5000, true) == SEL_NT1024_REGS && select_variant(16385, 1, true) == SEL_NT1024_MEM, "16384 / 16385 tiles, list");
  CHECK(select_variant_threads(SEL_NT256_REGS) == 256 && select_variant_threads(SEL_NT1024_REGS) == 1024 &&
            select_variant_threads(SEL_NT1024_MEM) == 1024,
        "threads of the variants");
  CHECK(select_variant_in_regs(SEL_NT256_REGS) && select_variant_in_regs(SEL_NT1024_REGS) && !select_variant_in_regs(SEL_NT1024_MEM),
        "IN_REGS of the variants");
  // every search the four waves take fits them: k values, one per thread, and 512 tiles, two per thread of SEL_VPT
  for (int m = 1; m <= 600; ++m)
    for (int k = 1; k <= 300; ++k)
      for (int l = 0; l < 2; ++l)
        if (select_variant(m, k, l) == SEL_NT256_REGS)
          CHECK(m <= SEL_THREADS_SMALL * SEL_VPT && k <= SEL_THREADS_SMALL && (m >= k || m <= 64), "NT256 at %d tiles, k = %d", m, k);

  // ---- select_tau --------------------------------------------------------------------------------------------------
  // narrow: M < k, M == k; k 1024 / 1025 of sixteen waves, 256 / 257 of four
  CHECK(!sel_narrow(1024, 1023, 1024, false) && sel_narrow(1024, 1024, 1024, false) && sel_narrow(1024, 1100, 1024, false), "narrow at M = k");
  CHECK(sel_narrow(1024, 4097, 1024, false) && !sel_narrow(1024, 4097, 1025, false), "narrow at k = 1024 / 1025");
  CHECK(sel_narrow(256, 512, 256, false) && !sel_narrow(256, 512, 257, false), "narrow at k = 256 / 257, four waves");
  CHECK(!sel_narrow(1024, 1100, 10, true) && !sel_narrow(256, 100, 10, true), "safe mode is never narrow");
  CHECK(!sel_narrow(1024, 0, 1, false) && sel_narrow(1024, 1, 1, false), "no tiles");
  // prefilter: tiles 512 / 513, and only when narrow
  CHECK(!sel_prefilter(true, 512) && sel_prefilter(true, 513) && !sel_prefilter(false, 513) && !sel_prefilter(false, 512), "prefilter at 512 / 513");
  // groups4: k 128 / 129, sixteen waves only; groups2k: k 512 / 513
  CHECK(sel_groups4(1024, 128) && !sel_groups4(1024, 129) && !sel_groups4(256, 128) && !sel_groups4(256, 1), "groups4 at k = 128 / 129");
  CHECK(!sel_groups2k(512) && sel_groups2k(513) && sel_groups2k(1024) && !sel_groups2k(1), "groups2k at k = 512 / 513");
  for (unsigned k = 1; k <= 1024; ++k) CHECK(!(sel_groups4(1024, k) && sel_groups2k(k)), "groups4 and groups2k at k = %u", k);
  // the bisects have k values or more to count: 256 group minima, NT thread minima, 2 NT half-thread minima
  for (unsigned k = 1; k <= 1024; ++k) {
    const unsigned groups = sel_groups2k(k) ? 2048u : (sel_groups4(1024, k) ? 256u : 1024u);
    CHECK(k <= groups, "k = %u of %u group minima", k, groups);
  }
  // the short list: 512 / 513 entries, 4096 / 4097
  CHECK(sel_short_small(512) && !sel_short_small(513) && sel_short_small(0), "the short list at 512 / 513");
  CHECK(!sel_flooded(4096) && sel_flooded(4097) && !sel_flooded(0), "the short list at 4096 / 4097");

  // ---- select_body -------------------------------------------------------------------------------------------------
  CHECK(!sel_over(4096) && sel_over(4097) && !sel_over(0), "over at 4096 / 4097 hit tiles");
  CHECK(!sel_refines(192, 192) && sel_refines(193, 192) && !sel_refines(0, 0) && sel_refines(1, 0), "refinement at the block's capacity");
  // step (f) from registers: 64 / 65 tiles of four waves, 256 / 257 of sixteen
  CHECK(sel_refine_in_regs(256, 64) && !sel_refine_in_regs(256, 65), "in registers at 64 / 65 tiles, four waves");
  CHECK(sel_refine_in_regs(1024, 256) && !sel_refine_in_regs(1024, 257), "in registers at 256 / 257 tiles, sixteen waves");
  CHECK(sel_refine_in_regs(1024, 0) && !sel_refine_in_regs(1024, 4096), "in registers at the ends");
  // the list shortcut: M < k, M == k, 64 M == k, 64 M < k
  CHECK(sel_list_shortcut(21, 100) && !sel_list_shortcut(21, 21) && !sel_list_shortcut(21, 10), "the list shortcut at M < k / M == k / M > k");
  CHECK(sel_list_shortcut(21, 1344) && !sel_list_shortcut(21, 1345) && sel_list_shortcut(21, 1343), "the list shortcut at 64 M == k / 64 M < k");
  CHECK(sel_list_shortcut(79, 100) && sel_list_shortcut(1, 64) && !sel_list_shortcut(1, 65) && !sel_list_shortcut(0, 1), "the list shortcut, small");
  // the block: k + 156 in whole lines of 64, one at least, 2^20 at most
  CHECK(select_default_entries(10) == 192 && select_default_entries(100) == 256 && select_default_entries(1000) == 1216, "default entries");
  CHECK(select_default_entries(36) == 192 && select_default_entries(37) == 256 && select_default_entries(0) == 192 &&
            select_default_entries(-5) == 192,
        "default entries at a line's edge, and without k");
  CHECK(select_default_entries(1 << 20) == (1 << 20) && select_default_entries(0x7FFFFFFF) == (1 << 20), "default entries, capped");
  for (int k = 1; k <= 5000; ++k) CHECK(select_default_entries(k) >= k + 156 && select_default_entries(k) % 64 == 0, "default entries of %d", k);

  if (fails) return 1;
  printf("select plan ok\n");
  return 0;
}
