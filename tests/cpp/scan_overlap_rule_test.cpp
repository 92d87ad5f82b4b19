// Host-only check of tostore_amd/csrc/tsh_scan_overlap.h: which scans alternate between the two scan streams.
// Decisions at 240 scan CUs for the shapes the rule was made for, the small-shard edge for every store, the drain share
// written out at the first big-shard tile count, and monotonicity in the tiles a scan reads.
// Prints "overlap rule ok"; exit status 1 on a miss.
#include <cmath>
#include <cstdio>
#include <initializer_list>

#include "../../tostore_amd/csrc/tsh_scan_overlap.h"

using namespace tsh;

static int fails = 0;
static const int CUS = 240;
static const RowStore STORES[3] = {RowStore::F32, RowStore::F16, RowStore::I8};
static const char *NAMES[3] = {"f32", "fp16", "int8"};

static int nch_of(int64_t ld) { return (int)((ld / 4 + 63) / 64); }
static int64_t tiles_of(int64_t rows) { return (rows + 63) / 64; }

static void expect(const char *what, RowStore st, int64_t ld, int64_t tiles, bool two) {
  const bool got = scan_two_streams(st, nch_of(ld), ld, tiles, CUS);
  printf("%-44s share %.4f -> %s\n", what, scan_drain_share(st, nch_of(ld), ld, tiles, CUS), got ? "two" : "one");
  if (got != two) {
    printf("  MISS: expected %s\n", two ? "two" : "one");
    ++fails;
  }
}

static void expect_share(const char *what, RowStore st, int64_t ld, int64_t tiles, double share) {
  const double got = scan_drain_share(st, nch_of(ld), ld, tiles, CUS);
  printf("%-44s share %.6f (expected %.6f)\n", what, got, share);
  if (std::fabs(got - share) > 1e-6) {
    printf("  MISS\n");
    ++fails;
  }
}

int main() {
  static_assert(SMALL_SHARD_TILES == 6144, "the small-shard edge");
  static_assert(SCAN_OVERLAP_MIN_SHARE > 0.030 && SCAN_OVERLAP_MIN_SHARE < 0.059, "between the two measured shares");
  // the launch shape's waves per CU: d = 768 -- f32 four, fp16 and int8 eight; d = 1536 int8 four
  if (scan_shape_waves_per_cu(row_store_shape_chunks(RowStore::F32, 3)) != 4 ||
      scan_shape_waves_per_cu(row_store_shape_chunks(RowStore::F16, 3)) != 8 ||
      scan_shape_waves_per_cu(row_store_shape_chunks(RowStore::I8, 3)) != 8 ||
      scan_shape_waves_per_cu(row_store_shape_chunks(RowStore::I8, 6)) != 4) {
    printf("MISS: waves per CU\n");
    ++fails;
  }

  expect("f32, 1 M x 768", RowStore::F32, 768, tiles_of(1000000), false);
  expect("int8, 1 M x 768", RowStore::I8, 768, tiles_of(1000000), true);
  expect("fp16, 1 M x 768", RowStore::F16, 768, tiles_of(1000000), true);
  expect("int8, 10 M x 1536", RowStore::I8, 1536, tiles_of(10000000), false);
  expect("fp16, 1 M x 768, a mask keeping 100 k", RowStore::F16, 768, tiles_of(100000), true);
  // (the f32 scan of 250 k x 768, where the second stream measured + 12 %: a small shard, as ever)
  expect("f32, 250 k x 768", RowStore::F32, 768, tiles_of(250000), true);

  for (int s = 0; s < 3; ++s)
    for (int64_t ld : {32, 128, 256, 768, 1536, 4096}) {
      char what[64];
      snprintf(what, sizeof what, "%s, d = %d, 6143 tiles", NAMES[s], (int)ld);
      expect(what, STORES[s], ld, 6143, true);
    }

  // 6144 tiles at d = 256: one-chunk shapes, 32 waves per CU in every store --
  //   share = 64 row_bytes x 32 x 240 / 2 / (6144 x 64 x (row_bytes + side)) = 0.625 row_bytes / (row_bytes + side)
  // f32: 0.625 x 1024 / 1032; fp16: 0.625 x 512 / 520; int8: 0.625 x 256 / 268.  All far above the threshold: two.
  expect_share("f32, d = 256, 6144 tiles", RowStore::F32, 256, 6144, 0.620155);
  expect_share("fp16, d = 256, 6144 tiles", RowStore::F16, 256, 6144, 0.615385);
  expect_share("int8, d = 256, 6144 tiles", RowStore::I8, 256, 6144, 0.597015);
  for (int s = 0; s < 3; ++s) expect("d = 256, 6144 tiles", STORES[s], 256, 6144, true);
  // ... and the shares the rule is calibrated on (the row, its norm term, its key; int8: its scale too)
  expect_share("f32, 1 M x 768", RowStore::F32, 768, 15625, 196608.0 * 4 * 240 / 2 / (15625.0 * 64 * 3080));
  expect_share("int8, 1 M x 768", RowStore::I8, 768, 15625, 49152.0 * 8 * 240 / 2 / (15625.0 * 64 * 780));
  expect_share("fp16, 1 M x 768", RowStore::F16, 768, 15625, 98304.0 * 8 * 240 / 2 / (15625.0 * 64 * 1544));

  // monotone: at a fixed store and width, fewer tiles never turn two into one
  for (int s = 0; s < 3; ++s)
    for (int64_t ld : {32, 100, 256, 512, 768, 1000, 1536, 2048, 4096}) {
      bool seen_two = false;
      for (int64_t tiles = 400000; tiles >= 1; tiles -= (tiles > 20000 ? 997 : 1)) {
        const bool two = scan_two_streams(STORES[s], nch_of(ld), ld, tiles, CUS);
        if (seen_two && !two) {
          printf("MISS: %s, d = %d: two above %lld tiles, one at it\n", NAMES[s], (int)ld, (long long)tiles);
          ++fails;
          break;
        }
        seen_two = seen_two || two;
      }
      if (!seen_two) {
        printf("MISS: %s, d = %d: never two\n", NAMES[s], (int)ld);
        ++fails;
      }
    }

  if (fails) return 1;
  printf("overlap rule ok\n");
  return 0;
}
