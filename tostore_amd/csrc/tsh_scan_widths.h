// tsh_scan_widths.h -- which tile-scan instantiation a row width takes, and which widths each family of tile scans
// serves.  Pure host arithmetic, no HIP: compiled into the library and, on its own, by tests/cpp/scan_widths_test.cpp,
// which holds the width list of tests/test_gpu_scan_widths.py to the set of instantiations these functions can reach.
//
// A row of d elements is stored as ld = round_up(d, 4) floats, d4 = ld / 4 groups of four: a lane holds one group per
// chunk of 64 groups (256 elements).  The tile scans are instantiated for a short list of chunk counts, so a row takes
// the smallest listed count at or above its need -- FULL when d4 == 64 NCH, otherwise a row that ends inside a chunk
// and, from ten chunks on, possibly one chunk short of the kernel's (a wholly empty chunk).
#pragma once

namespace tsh {

// the chunk counts the tile scans are instantiated for (tsh_scan_tu.hip: one `case` each), ascending
inline constexpr int SCAN_NCH_OPTS[] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16};
constexpr int SCAN_NCH_COUNT = (int)(sizeof(SCAN_NCH_OPTS) / sizeof(SCAN_NCH_OPTS[0]));

// the widest row of each family (ScanF32 / ScanF16 / ScanI8 in tsh_scan_tu.hip assert theirs against these)
constexpr int SCAN_F32_MAX_NCH = 16;
constexpr int SCAN_F16_MAX_NCH = 14;  // (wider rows that end inside a chunk would spill: they stay on f32)
constexpr int SCAN_I8_MAX_NCH = 8;    // (beyond that two buffers of eight rows and the query leave the register budget)

// rows of ld = 128 / 64 / 32 floats: the f32 scan packs several whole rows into one wave load (scan_packed_kernel)
constexpr bool scan_packed_ld(long long ld) { return ld == 128 || ld == 64 || ld == 32; }

// d4 groups of four elements -> the chunk count of the instantiation that scans them; -1: wider than any
inline int pick_nch(int d4) {
  int need = (d4 + 63) / 64;
  for (int o : SCAN_NCH_OPTS)
    if (o >= need) return o;
  return -1;
}

// the fp16 tile scans: rows of at least 256 elements, a multiple of 8, of up to SCAN_F16_MAX_NCH chunks
inline bool scan_f16_supported(int nch, int dim) { return dim >= 256 && dim % 8 == 0 && nch >= 1 && nch <= SCAN_F16_MAX_NCH; }

// the int8 tile scans: rows of up to SCAN_I8_MAX_NCH chunks (d <= 2048)
inline bool scan_i8_supported(int nch) { return nch >= 1 && nch <= SCAN_I8_MAX_NCH; }

}  // namespace tsh
