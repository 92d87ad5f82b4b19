// tsh_scan_tu.hip -- the single-query scan kernels' instantiations and their launcher (K1, tsh_kernels.hip.h).
// A translation unit of its own: the instantiations compile in parallel with the rest of the library.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>

#include "../../include/tostore_hip.h"
#include "tsh_launch.h"

namespace tsh {
namespace {

#define TSH_LAUNCH(KERN, GRID, BLOCK, LDS, ST, EV, ARG)                                                  \
  do {                                                                                                  \
    if ((EV).start || (EV).stop)                                                                        \
      hipExtLaunchKernelGGL(KERN, dim3((unsigned)(GRID)), dim3((unsigned)(BLOCK)), (unsigned)(LDS), ST, \
                            (EV).start, (EV).stop, 0, ARG);                                             \
    else                                                                                                \
      KERN<<<(GRID), (BLOCK), (unsigned)(LDS), ST>>>(ARG);                                              \
  } while (0)

// How many waves of a dense scan share a CU.  The registers would allow 8 to 16, and that is slower: every wave
// streams its own tile, and HBM serves fewer, longer streams better than many short ones -- measured per width with
// the occupancy held down by an (unused) dynamic LDS allocation, two-wave workgroups (tools/dims_probe.sh; scan time
// at the default occupancy -> at the one chosen here): d = 768 457 -> 439 us (0.840 -> 0.875 of the HBM peak), 1536
// 562 -> 537, 2048 740 -> 705, 1000 367 -> 357, 512 191 -> 184, 384 147 -> 139.  Four waves per CU from three chunks
// per row on, eight for two; one-chunk rows (d <= 256) keep the registers' occupancy (d = 200: 76 us against 79 / 113
// at eight / four waves); two waves per CU are as good as four at d = 768 and one is far too few (657 us).  Masked
// scans that keep most rows (tombstones, mild filters: scan_mostly_live) stream like dense ones and take the same shape
// (keep 100 / 95 / 80 %: 481 / 460 / 385 -> 441-454 / 426-434 / 370 us); selective ones walk scattered rows and live on many
// waves (keep 50 %: +2 % at eight waves, keep 10 %: -8 %): theirs stays.  One
// tile per wave and a workgroup per two tiles stays: a grid of 480 / 960 / 1920 workgroups striding over the tiles
// takes 560 / 500 / 457 us against 439-445.
// (the figures live in tsh_scan_overlap.h, where the two-stream rule reads them too)
template <int NCH> struct ScanShape {
  static constexpr int WPB = scan_shape_wpb(NCH);  // waves per workgroup
  static constexpr int LDS = scan_shape_lds(NCH);  // 160 KB per CU: 4 resp. 2 workgroups
};

// A family of tile-scan kernels, as the launcher below sees it: the kernel for (NCH, METRIC, FULL, MASKED) with its
// (rows per group R, min waves per SIMD) per row width, the ScanShape it is launched in, whether masked instantiations
// exist, and the widest NCH (widths: 1-8, 10, 12, 14, 16 up to MAX_NCH).
struct ScanF32 {
  // two register buffers of R*NCH*4 VGPRs plus NCH*4 for the query must fit 512/MINW registers.
  template <int NCH, bool MASKED> struct Tune {
    static constexpr int R = (NCH <= 2) ? 4 : (NCH == 3 ? (MASKED ? 2 : 4) : 2);
    static constexpr int MINW =
        (NCH <= 2) ? 4 : (NCH == 3 ? (MASKED ? 4 : 3) : (NCH == 4 ? 4 : (NCH <= 6 ? 3 : (NCH <= 8 ? 2 : 1))));
  };
  template <int NCH> using Shape = ScanShape<row_store_shape_chunks(RowStore::F32, NCH)>;
  static constexpr bool HAS_MASKED = true;
  static constexpr int MAX_NCH = 16;
  static_assert(MAX_NCH == SCAN_F32_MAX_NCH, "tsh_scan_widths.h names this family's widest row");
  template <int NCH, int METRIC, bool FULL, bool MASKED> static constexpr auto kernel() {
    using T = Tune<NCH, MASKED>;
    return &scan_kernel<NCH, METRIC, FULL, MASKED, T::R, true, 4, T::MINW>;
  }
};
// The fp16 scan: a row is half the bytes, so two register buffers of R rows are R*NCH*2 VGPRs each, and the launch shape
// is ScanShape's for a row of half as many 1 KiB chunks (d = 768: 1.5 KiB rows, eight waves per CU; d = 1536: four).
// MASKED: the same (R, MINW) at every width -- the masked instantiations fit the dense ones' register budgets without
// scratch (the compiler's resource-usage remarks: profiles/scan_f16_masked_resources.txt).
struct ScanF16 {
  template <int NCH, bool MASKED> struct Tune {
    static constexpr int R = NCH <= 6 ? 4 : 2;
    static constexpr int MINW = NCH <= 4 ? 4 : (NCH <= 8 ? 3 : 2);
  };
  template <int NCH> using Shape = ScanShape<row_store_shape_chunks(RowStore::F16, NCH)>;
  static constexpr bool HAS_MASKED = true;
  static constexpr int MAX_NCH = 14;  // (wider rows that end inside a chunk would spill: they stay on f32)
  static_assert(MAX_NCH == SCAN_F16_MAX_NCH, "tsh_scan_widths.h names this family's widest row");
  template <int NCH, int METRIC, bool FULL, bool MASKED> static constexpr auto kernel() {
    using T = Tune<NCH, MASKED>;
    return &scan_f16_kernel<NCH, METRIC, FULL, MASKED, T::R, 4, T::MINW>;
  }
};
// The int8 scan: a row is a quarter of the bytes, two register buffers of eight rows are 16 * NCH VGPRs, and the launch
// shape is the fp16 scan's (ScanShape of half as many chunks: as many bytes in flight per CU as there).  Rows of up to
// eight chunks (d <= 2048): beyond that the two buffers and the query leave the register budget.
// MASKED: buffers of four rows (two groups per batch, so a tile's odd batch count needs no tail of its own) within the
// dense instantiations' MINW -- no scratch, at least their occupancy (profiles/scan_i8_masked_resources.txt).
struct ScanI8 {
  template <int NCH, bool MASKED> struct Tune {
    static constexpr int R = MASKED ? 4 : 8;
    static constexpr int MINW = NCH <= 4 ? 4 : (NCH <= 6 ? 3 : 2);
  };
  template <int NCH> using Shape = ScanShape<row_store_shape_chunks(RowStore::I8, NCH)>;
  static constexpr bool HAS_MASKED = true;
  static constexpr int MAX_NCH = 8;
  static_assert(MAX_NCH == SCAN_I8_MAX_NCH, "tsh_scan_widths.h names this family's widest row");
  template <int NCH, int METRIC, bool FULL, bool MASKED> static constexpr auto kernel() {
    using T = Tune<NCH, MASKED>;
    return &scan_i8_kernel<NCH, METRIC, FULL, MASKED, T::R, 4, T::MINW>;
  }
};

// grid > 0: a big shard -- dense and mostly-live scans in the shape of ScanShape, scattered masked ones in `grid` 4-wave
// workgroups; grid < 0: -grid one-wave workgroups (small shards)
// (the middle branch is never taken by a dense instantiation)
template <class F, int NCH, int METRIC, bool FULL, bool MASKED>
void launch_tile_scan_t(const ScanArgsQ &a, int grid, hipStream_t s, const LaunchEv &ev, bool mostly_live) {
  using S = typename F::template Shape<NCH>;
  constexpr auto kern = F::template kernel<NCH, METRIC, FULL, MASKED>();
  if (grid > 0 && (!MASKED || mostly_live))
    TSH_LAUNCH(kern, (a.a.n_tiles + S::WPB - 1) / S::WPB, 64 * S::WPB, S::LDS, s, ev, a);
  else if (grid > 0) TSH_LAUNCH(kern, grid, 256, 0, s, ev, a);
  else TSH_LAUNCH(kern, -grid, 64, 0, s, ev, a);
}
template <class F, int NCH, int METRIC>
void launch_tile_scan_m(const ScanArgsQ &a, bool masked, int grid, hipStream_t s, const LaunchEv &ev, bool ml) {
  const bool full = a.a.d4 == NCH * 64;
  if constexpr (F::HAS_MASKED) {
    if (masked) {
      if (full) launch_tile_scan_t<F, NCH, METRIC, true, true>(a, grid, s, ev, ml);
      else launch_tile_scan_t<F, NCH, METRIC, false, true>(a, grid, s, ev, ml);
      return;
    }
  }
  if (full) launch_tile_scan_t<F, NCH, METRIC, true, false>(a, grid, s, ev, ml);
  else launch_tile_scan_t<F, NCH, METRIC, false, false>(a, grid, s, ev, ml);
}
// grid: launch_tile_scan_t's, for a shard of SMALL_SHARD_TILES tiles or more (smaller ones: one-wave workgroups --
// fewer than ~6 four-wave workgroups per CU and tile counts per CU differ by tens of percent; one tile per workgroup
// lets the dispatcher even them out)
template <class F>
void launch_tile_scan(const ScanArgsQ &a, int nch, int metric, bool masked, int grid, hipStream_t s, const LaunchEv &ev, bool ml) {
  if (a.a.n_tiles < SMALL_SHARD_TILES) grid = -std::max(1, (int)a.a.n_tiles);
#define TSH_NCH_DO(N)                                                                                  \
  do {                                                                                                 \
    if (metric == TSH_METRIC_L2) launch_tile_scan_m<F, N, METRIC_L2>(a, masked, grid, s, ev, ml);      \
    else if (metric == TSH_METRIC_IP) launch_tile_scan_m<F, N, METRIC_IP>(a, masked, grid, s, ev, ml); \
    else launch_tile_scan_m<F, N, METRIC_COS>(a, masked, grid, s, ev, ml);                             \
  } while (0)
// (a width the family does not have falls through to its widest: the cases below must stay in ascending order, a new
// width goes in its place in the list)
#define TSH_NCH(N)                  \
  case N:                           \
    if constexpr (N < F::MAX_NCH) { \
      TSH_NCH_DO(N);                \
      break;                        \
    }                               \
    [[fallthrough]];
  switch (nch) {
    TSH_NCH(1) TSH_NCH(2) TSH_NCH(3) TSH_NCH(4) TSH_NCH(5) TSH_NCH(6) TSH_NCH(7) TSH_NCH(8)
    TSH_NCH(10) TSH_NCH(12) TSH_NCH(14)
    default: TSH_NCH_DO(F::MAX_NCH);
  }
#undef TSH_NCH
#undef TSH_NCH_DO
}

template <int SPLIT>
void launch_packed(const ScanArgsQ &a, int metric, bool masked, int grid, int threads, hipStream_t s,
                   const LaunchEv &ev) {
#define TSH_PK(M, MK) TSH_LAUNCH((scan_packed_kernel<SPLIT, M, MK, true>), grid, threads, 0, s, ev, a)
  if (metric == TSH_METRIC_L2) { if (masked) TSH_PK(METRIC_L2, true); else TSH_PK(METRIC_L2, false); }
  else if (metric == TSH_METRIC_IP) { if (masked) TSH_PK(METRIC_IP, true); else TSH_PK(METRIC_IP, false); }
  else { if (masked) TSH_PK(METRIC_COS, true); else TSH_PK(METRIC_COS, false); }
#undef TSH_PK
}

template <int NCH>
void launch_scan_list_n(const ScanArgsQ &a, int metric, hipStream_t s, const LaunchEv &ev) {
  constexpr int R = NCH <= 5 ? 4 : 2;  // two register buffers of R rows: all eight rows of a wave in flight up to d = 1280
  const int grid = a.a.n_tiles;
  if (metric == TSH_METRIC_L2) TSH_LAUNCH((scan_list_kernel<NCH, METRIC_L2, R, true>), grid, 512, 0, s, ev, a);
  else if (metric == TSH_METRIC_IP) TSH_LAUNCH((scan_list_kernel<NCH, METRIC_IP, R, true>), grid, 512, 0, s, ev, a);
  else TSH_LAUNCH((scan_list_kernel<NCH, METRIC_COS, R, true>), grid, 512, 0, s, ev, a);
}

}  // namespace

// (scan_f16_supported, scan_i8_supported: tsh_scan_widths.h)
void launch_scan_f16(const ScanArgsQ &a, int nch, int metric, bool masked, hipStream_t s, const LaunchEv &ev, bool ml) {
  if (a.a.n_tiles <= 0) return;
  launch_tile_scan<ScanF16>(a, nch, metric, masked, std::max(1, (a.a.n_tiles + 3) / 4), s, ev, ml);
}

void launch_scan_i8(const ScanArgsQ &a, int nch, int metric, bool masked, hipStream_t s, const LaunchEv &ev, bool ml) {
  if (a.a.n_tiles <= 0) return;
  launch_tile_scan<ScanI8>(a, nch, metric, masked, std::max(1, (a.a.n_tiles + 3) / 4), s, ev, ml);
}

bool scan_list_supported(int nch, int64_t ld) { return nch >= 1 && nch <= 8 && ld != 128 && ld != 64 && ld != 32; }

void launch_scan_list(const ScanArgsQ &a, int nch, int metric, hipStream_t s, const LaunchEv &ev) {
  if (a.a.n_tiles <= 0) return;
  switch (nch) {
    case 1: launch_scan_list_n<1>(a, metric, s, ev); break;
    case 2: launch_scan_list_n<2>(a, metric, s, ev); break;
    case 3: launch_scan_list_n<3>(a, metric, s, ev); break;
    case 4: launch_scan_list_n<4>(a, metric, s, ev); break;
    case 5: launch_scan_list_n<5>(a, metric, s, ev); break;
    case 6: launch_scan_list_n<6>(a, metric, s, ev); break;
    case 7: launch_scan_list_n<7>(a, metric, s, ev); break;
    default: launch_scan_list_n<8>(a, metric, s, ev); break;
  }
}

void launch_scan(const ScanArgsQ &a, int nch, int metric, bool masked, hipStream_t s, const LaunchEv &ev, bool ml) {
  int grid = (a.a.n_tiles + 3) / 4;
  if (grid < 1) grid = 1;
  if (a.a.ld == 128 || a.a.ld == 64 || a.a.ld == 32) {
    // narrow rows: several whole rows per 1 KiB wave load (scan_packed_kernel)
    int threads = 256;
    if (a.a.n_tiles < SMALL_SHARD_TILES) {
      grid = std::max(1, (int)a.a.n_tiles);
      threads = 64;
    }
    if (a.a.ld == 128) launch_packed<1>(a, metric, masked, grid, threads, s, ev);
    else if (a.a.ld == 64) launch_packed<2>(a, metric, masked, grid, threads, s, ev);
    else launch_packed<3>(a, metric, masked, grid, threads, s, ev);
    return;
  }
  launch_tile_scan<ScanF32>(a, nch, metric, masked, grid, s, ev, ml);
}

}  // namespace tsh
