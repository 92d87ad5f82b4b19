// tsh_select_plan.h -- which instantiation of the K2 select (select_kernel, tsh_kernels.hip.h) a search takes, and the
// conditions under which the kernel goes one way or the other.  Pure arithmetic, no HIP: compiled into the library --
// launch_select (tsh_lib.hip), select_tau / select_body and the int8 route's i8_list_kernel call these functions and spell
// none of the conditions out themselves -- and, on its own, by tests/cpp/select_plan_test.cpp and by
// tests/cpp/select_plan_lib.cpp, through which the NumPy model of the select (tests/select_model.py) takes its branches.
//
// M: the tile count of the scan (64 rows a tile; a list scan's tiles are tiles of list positions).  NT: the threads of the
// workgroup, 256 or 1024.  k: neighbours asked for.
#pragma once
#include <stdint.h>

namespace tsh {

// (inlined where they are called, before anything else is done to the caller: the kernels' code is what it was when they
// spelled these conditions out -- profiles/select_plan_isa.txt)
#define TSH_SEL_FN constexpr __attribute__((always_inline))

constexpr int SEL_THREADS = 1024;   // one whole CU; tile minima stay in registers
constexpr int SEL_VPT = 16;         // tile minima a thread keeps in registers (16384 tiles = 1M rows)
constexpr int SEL_LIST_CAP = 4096;  // LDS lists (short list of tile minima / tile ids)
constexpr int SEL_PREFILTER_MIN = 512;  // above this many tiles, bound the list by the thread-minima bisect first

constexpr int SEL_THREADS_SMALL = 256;    // the four-wave instantiation ...
constexpr int SEL_SMALL_MAX_TILES = 512;  // ... serves up to this many tiles
constexpr int SEL_SMALL_MAX_K = 256;      // ... and up to this k
constexpr int SEL_SMALL_REGS_TILES = 64;  // tiles step (f) of the four-wave instantiation holds in registers
constexpr int SEL_REFINE_RV = 16;         // step (f): tiles a wave keeps in registers
constexpr int SEL_SHORT_SMALL = 512;      // short lists up to here are bisected as 8 values a lane, longer ones as 64

// the three instantiations of select_kernel<NT, IN_REGS>
enum SelectVariant { SEL_NT256_REGS = 0, SEL_NT1024_REGS = 1, SEL_NT1024_MEM = 2 };

// launch_select's choice.
// A few hundred tiles (an index of some ten thousand rows): four waves instead of sixteen synchronise faster (10 k x 128:
// p50 42.8 -> 39.8 us); from a few thousand tiles on the wide workgroup wins.
// all_hit -- fewer tiles than k: the tile-minimum bound says nothing, every tile is a hit and step (f) bisects over all of
// them, from registers only while they fit a workgroup's: 64 tiles for four waves, 256 for sixteen.  A list scan of a
// few thousand kept rows lands exactly there: 79 tiles, k = 100 took 85 us per query instead of 30.
// list_many_hits -- a list scan's tile minima bound the k-th key loosely (its tiles hold the kept rows in id order, every
// one of them a mix of near and far rows: a 1 % mask of 1 M rows is 157 tiles of which ~100 are hits), and step (f)
// bisects over them from registers only with sixteen waves.
inline SelectVariant select_variant(int32_t n_tiles, int32_t k, bool has_list) {
  const bool all_hit = n_tiles < k && n_tiles > SEL_SMALL_REGS_TILES;
  const bool list_many_hits = has_list && n_tiles > SEL_SMALL_REGS_TILES;
  if (n_tiles <= SEL_SMALL_MAX_TILES && k <= SEL_SMALL_MAX_K && !all_hit && !list_many_hits) return SEL_NT256_REGS;
  if (n_tiles <= SEL_VPT * SEL_THREADS) return SEL_NT1024_REGS;
  return SEL_NT1024_MEM;
}
constexpr int select_variant_threads(SelectVariant v) { return v == SEL_NT256_REGS ? SEL_THREADS_SMALL : SEL_THREADS; }
constexpr bool select_variant_in_regs(SelectVariant v) { return v != SEL_NT1024_MEM; }

// select_tau: the tile minima bound the k-th key (k tiles or more, k within one value per thread); otherwise tau = KEY_NAN
TSH_SEL_FN bool sel_narrow(int NT, int M, uint32_t k, bool force_all) { return !force_all && (uint32_t)M >= k && k <= (uint32_t)NT; }
// ... and the short list is bounded by the bisect over thread (group) minima first; at or below, it holds every tile
TSH_SEL_FN bool sel_prefilter(bool narrow, int M) { return narrow && M > SEL_PREFILTER_MIN; }
// 256 four-thread group minima are plenty for small k
TSH_SEL_FN bool sel_groups4(int NT, uint32_t k) { return NT == 1024 && k <= 128; }
// above k = 512 the k-th of 1024 thread minima gets loose (G ln(G/(G-k)) entries below it): split every thread into its
// even and odd elements, 2048 groups
TSH_SEL_FN bool sel_groups2k(uint32_t k) { return k > 512; }
// the short list of n tile minima: bisected as 8 values a lane, or as SEL_LIST_CAP / 64; beyond the list, tau = U
TSH_SEL_FN bool sel_short_small(uint32_t n) { return n <= (uint32_t)SEL_SHORT_SMALL; }
TSH_SEL_FN bool sel_flooded(uint32_t n) { return n > (uint32_t)SEL_LIST_CAP; }
// select_body, step (d): more hit tiles than the list holds -- nothing is emitted, the host's wide-band pass follows
TSH_SEL_FN bool sel_over(uint32_t tiles_hit) { return tiles_hit > (uint32_t)SEL_LIST_CAP; }
// step (f) runs (not when over, not in safe mode) when the first emit found more than the block holds
TSH_SEL_FN bool sel_refines(uint32_t first_count, int32_t cand_cap) { return first_count > (uint32_t)cand_cap; }
// ... from registers while the hit tiles fit the workgroup's: SEL_REFINE_RV a wave
TSH_SEL_FN bool sel_refine_in_regs(int NT, uint32_t tiles_hit) { return tiles_hit <= (uint32_t)(NT / 64 * SEL_REFINE_RV); }
// A list scan (not in safe mode) of fewer tiles than k whose M * 64 list positions reach k: the k-th smallest KEY, by block_kth_radix
TSH_SEL_FN bool sel_list_shortcut(int M, uint32_t k) { return (uint32_t)M < k && (uint32_t)M * 64u >= k; }

// tsh_default_block_entries: room for k and the usual surplus of the band, in whole lines of 64
inline int32_t select_default_entries(int32_t k) {
  int64_t e = (int64_t)(k > 1 ? k : 1) + 156;
  e = (e + 63) / 64 * 64;
  return (int32_t)(e < (1 << 20) ? e : (1 << 20));
}

#undef TSH_SEL_FN

}  // namespace tsh
