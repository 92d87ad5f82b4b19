// The batched key passes' tile order (tostore_amd/csrc/tsh_batch_tiles.h, no HIP in it) on the CPU, for q_tiles 1-8 and
// n_tiles 1-300:
//   1. slot -> (query tile, row tile) is a bijection onto q_tiles x n_tiles;
//   2. in the full rounds (8 q_tiles slots each) the slots of one XCD (b % 8) come in runs of q_tiles consecutive ones
//      that share a row tile and take every query tile once -- and the eight XCDs of a round take eight row tiles;
//   3. the persistent fp16 kernel (grid G, workgroup b scores slots b, b + G, b + 2 G ...): with G a multiple of
//      8 q_tiles a workgroup keeps its query tile through all its full-round slots; with q_tiles = 3 and G = 256
//      (256 % 24 != 0) EVERY workgroup changes it between two consecutive full-round slots -- what
//      tests/test_gpu_batch_shapes.py relies on to reach the kernel's reload of its thresholds.
// Prints "batch tiles ok" and returns 0, or one line per miss and 1.
#include <cstdio>
#include <vector>

#include "../../tostore_amd/csrc/tsh_batch_tiles.h"

static int fails = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      if (++fails <= 20) {          \
        std::printf("MISS: ");      \
        std::printf(__VA_ARGS__);   \
        std::printf("\n");          \
      }                             \
    }                               \
  } while (0)

int main() {
  for (int qt = 1; qt <= 8; ++qt)
    for (int nt = 1; nt <= 300; ++nt) {
      const int total = qt * nt, per_round = 8 * qt, full = total / per_round * per_round;
      std::vector<int> seen((size_t)total, 0), qo((size_t)total), no((size_t)total);
      for (int b = 0; b < total; ++b) {
        int q = -1, n = -1;
        tsh::batch_tile_of(qt, nt, b, &q, &n);
        CHECK(q >= 0 && q < qt && n >= 0 && n < nt, "q_tiles %d n_tiles %d slot %d -> (%d, %d) outside", qt, nt, b, q, n);
        if (q >= 0 && q < qt && n >= 0 && n < nt) ++seen[(size_t)(n * qt + q)];
        qo[(size_t)b] = q;
        no[(size_t)b] = n;
      }
      for (int t = 0; t < total; ++t) CHECK(seen[(size_t)t] == 1, "q_tiles %d n_tiles %d: tile %d taken %d times", qt, nt, t, seen[(size_t)t]);
      // 2. the runs of an XCD: slots xcd + 8 i, i = q_tiles j .. q_tiles j + q_tiles - 1
      for (int b0 = 0; b0 < full; b0 += per_round)
        for (int xcd = 0; xcd < 8; ++xcd) {
          std::vector<int> qs((size_t)qt, 0);
          for (int u = 0; u < qt; ++u) {
            const int b = b0 + xcd + 8 * u;
            CHECK(no[(size_t)b] == no[(size_t)(b0 + xcd)], "q_tiles %d n_tiles %d: slots %d and %d of XCD %d differ in row tile", qt, nt, b0 + xcd, b, xcd);
            ++qs[(size_t)qo[(size_t)b]];
          }
          for (int u = 0; u < qt; ++u) CHECK(qs[(size_t)u] == 1, "q_tiles %d n_tiles %d: run at %d of XCD %d takes query tile %d %d times", qt, nt, b0, xcd, u, qs[(size_t)u]);
          CHECK(no[(size_t)(b0 + xcd)] == b0 / per_round * 8 + xcd, "q_tiles %d n_tiles %d: round %d, XCD %d scores row tile %d", qt, nt, b0 / per_round, xcd, no[(size_t)(b0 + xcd)]);
        }
      // 3. persistent grids
      for (int g = per_round; g <= 256; g += per_round)
        for (int b = 0; b < g && b < full; ++b)
          for (int t = b + g; t < full; t += g)
            CHECK(qo[(size_t)t] == qo[(size_t)b], "q_tiles %d n_tiles %d grid %d: workgroup %d changes its query tile at slot %d", qt, nt, g, b, t);
      if (qt == 3)
        for (int t = 0; t + 256 < full; ++t)
          CHECK(qo[(size_t)t] != qo[(size_t)(t + 256)], "q_tiles 3 n_tiles %d grid 256: slots %d and %d share query tile %d", nt, t, t + 256, qo[(size_t)t]);
    }
  // (the shape test_persistent_loop_changes_query_tile runs at 256 CUs: 3 x 89 slots, eight second slots in full rounds)
  {
    int q0, n0, q1, n1;
    tsh::batch_tile_of(3, 89, 0, &q0, &n0);
    tsh::batch_tile_of(3, 89, 256, &q1, &n1);
    CHECK(q0 == 0 && n0 == 0 && q1 == 2 && n1 == 80, "3 x 89: slots 0 and 256 are (%d, %d) and (%d, %d)", q0, n0, q1, n1);
  }
  if (fails) {
    std::printf("%d misses\n", fails);
    return 1;
  }
  std::printf("batch tiles ok\n");
  return 0;
}
