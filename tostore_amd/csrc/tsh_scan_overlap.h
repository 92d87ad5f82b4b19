// tsh_scan_overlap.h -- when consecutive single-query scans of a shard alternate between the two scan streams, and the
// launch-shape facts that decision shares with the launcher (tsh_scan_tu.hip).  Pure host arithmetic, no HIP: compiled
// into the library and, on its own, by tests/cpp/scan_overlap_rule_test.cpp.
//
// The drain of a launch.  A dense big-shard scan runs one tile per wave, W waves per CU on C CUs, so a wave lives for
// its tile's share of the HBM rate: tile_bytes W C / rate (int8, 1 M x 768: 48 KB x 1920 / 6.63 TB/s = 13.9 us; f32:
// 192 KB x 960 / 6.97 TB/s = 26.4 us).  At the end of a launch the slots empty over one wave life and, on one in-order
// stream, nothing refills them: half a wave life is lost per scan, whatever the scan's length.  As a share of the scan:
//
//   drain share = tile_bytes W C / 2 / bytes_the_scan_moves
//
// 3.1 % for the f32 scan of 1 M x 768 (a second stream measured + 1.4 %: not kept), 6.1 % for the int8 and fp16 scans
// of the same rows, 12 % for the f32 scan of 250 k x 768 (a second stream measured + 12 %: kept), 0.3 % for the int8 scan
// of 10 M x 1536.  With a second stream the next scan's workgroups fill the slots as they empty.  The two launches then
// run side by side: each one's own duration (tsh_counters.scan_us_*) is about twice its share of the HBM time.
#pragma once
#include <cstdint>

namespace tsh {

enum class RowStore { F32, F16, I8 };  // which copy of the rows a tile scan reads

constexpr int SMALL_SHARD_TILES = 6 * 4 * 256;  // below this: one-wave workgroups, two scan streams
constexpr int TILE_ROWS = 64;                   // a tile: the 64 rows one wave scans

// The launch shape of a dense big-shard scan whose row is `chunks` 1 KiB chunks wide (ScanShape, tsh_scan_tu.hip, where
// the measurements behind it are): waves per workgroup, the dynamic LDS that holds the occupancy down, and the waves that
// then share a CU.  One-chunk rows keep the registers' occupancy: eight waves per SIMD in every family
// (profiles/r04_kernel_resources.txt, profiles/scan_i8_resources.txt).
constexpr int scan_shape_wpb(int chunks) { return chunks == 1 ? 4 : 2; }
constexpr int scan_shape_lds(int chunks) { return chunks == 1 ? 0 : (chunks == 2 ? 32768 : 65536); }  // 160 KB per CU: 4 resp. 2 workgroups
constexpr int scan_shape_waves_per_cu(int chunks) { return chunks == 1 ? 32 : (chunks == 2 ? 4 : 2) * scan_shape_wpb(chunks); }

// ... and per store: bytes of an element, the 1 KiB chunks the shape goes by (the fp16 and int8 scans are launched in
// the shape of a row of half as many chunks), and what a scan moves per row beside the row itself: the row's norm term
// and the key it writes, 4 B each, and the int8 copy's scale.
constexpr int row_store_elem_bytes(RowStore st) { return st == RowStore::F32 ? 4 : (st == RowStore::F16 ? 2 : 1); }
constexpr int row_store_shape_chunks(RowStore st, int nch) { return st == RowStore::F32 ? nch : (nch + 1) / 2; }
constexpr int row_store_side_bytes(RowStore st) { return st == RowStore::I8 ? 12 : 8; }

// Below this drain share a second stream does not pay.  Bracketed by measurement (64-query calls, one against two
// streams; profiles/scan_overlap_ab.json): two streams lost 0.4 % at a share of 3.1 % and won
// 0.8 % at 4.5 %, 2.2-3.4 % at 6 %, 11 % at 12 %.
constexpr double SCAN_OVERLAP_MIN_SHARE = 0.045;

// The drain share of a tile scan that reads tiles_read tiles of rows of ld elements (nch chunks of f32) from `store`,
// in the dense big-shard shape on scan_cus CUs.  (A scattered masked scan -- one that keeps less than 60 % of the rows --
// is launched on more waves per CU than this: its share is larger than the figure here, which then errs towards one
// stream, the rule before this one.)
inline double scan_drain_share(RowStore store, int nch, int64_t ld, int64_t tiles_read, int scan_cus) {
  if (tiles_read <= 0) return 1.0;
  const double row_bytes = (double)ld * row_store_elem_bytes(store);
  const double tile_bytes = TILE_ROWS * row_bytes;
  const double moved = (double)tiles_read * TILE_ROWS * (row_bytes + row_store_side_bytes(store));
  return tile_bytes * scan_shape_waves_per_cu(row_store_shape_chunks(store, nch)) * scan_cus / 2.0 / moved;
}

// Two scan streams?  Small shards as ever (one-wave workgroups: the rule they were given when every scan read f32 rows);
// big ones when the drain is a large enough share of the scan.  tiles_read: a mask's kept rows count, not the shard's.
inline bool scan_two_streams(RowStore store, int nch, int64_t ld, int64_t tiles_read, int scan_cus) {
  if (tiles_read < SMALL_SHARD_TILES) return true;
  return scan_drain_share(store, nch, ld, tiles_read, scan_cus) >= SCAN_OVERLAP_MIN_SHARE;
}

}  // namespace tsh
