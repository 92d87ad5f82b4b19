// tsh_group.hip.h -- device side of a grouped search (tsh_search_grouped, include/tostore_hip.h): the nearest row of each
// of the k nearest groups, for one query.  gfx950, wave = 64.  The rules and their proof are in tsh_group_rule.h.
//
// A grouped job is an f32 tile scan or list scan like a count's; then, around the unchanged select and re-rank, three
// passes over what the scan left in the context -- a key per row, a minimum per tile -- and the context's head table
// gm[n_groups] of 64-bit words, all-ones in front of every job (cleared on the job's stream):
//   G1 group_min_kernel    a wave per tile.  Every live grouped position offers its word  key << 32 | position  to
//                          gm[group] by a 64-bit atomicMin: the minimum does not depend on arrival order.  Rows of one
//                          document are inserted together, so a RUN of equal group ids inside the wave is reduced in
//                          registers first (a segmented min by shuffles, six steps) and its first lane issues ONE atomic.
//                          Ungrouped rows issue none; tiles whose gmin is KEY_DEAD are skipped unread; list scans map
//                          positions through the list and skip its padding.
//   G2 group_heads_kernel  a wave per tile writes the HEADS array -- the row's key where the row is its group's head (the
//                          table holds its own word) or ungrouped, KEY_DEAD elsewhere -- and that array's tile minima.
//                          Every position of every tile is written (dead tiles: KEY_DEAD, their keys unread).
//   (select_kernel, rerank_kernel and on overflow the wide-band pass run over the heads array and its minima: the k-th
//   smallest tile minimum of heads names k distinct groups)
//   G3 group_side_kernel   the rows that are not heads but may be their group's exact best: a live grouped key at or
//                          below band_of(its head's key) and at or below the band_key the select left in the device
//                          header.  Their ids go to the context's side list (the cursor searches' own: an atomic count,
//                          ids past the capacity counted, not written); after_side_kernel (tsh_after.hip.h) takes their
//                          exact sums by the re-rank's own code.
// Bounds: group ids are checked against n_groups where they are read (group_valid), rows at or beyond group_rows are
// ungrouped, positions stay below n_tiles * 64.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsh_group_rule.h"
#include "tsh_kernels.hip.h"

namespace tsh {

struct GroupArgs {
  const uint32_t *keys;    // n_tiles * 64, as the scan left them (list scans: in list order)
  const uint32_t *gmin;    // n_tiles
  const uint32_t *list;    // list scans: position -> local row id (0xFFFFFFFF: padding); NULL: position = row
  const int32_t *group_of;  // local row -> group, group_rows entries
  unsigned long long *gm;   // n_groups head words
  uint32_t *heads, *hmin;  // G2's outputs: n_tiles * 64 and n_tiles
  int64_t group_rows;
  int32_t n_groups;
  int32_t n_tiles;
};

// one position's view: its key, whether it is a live grouped row, its group and word
struct GroupPos {
  uint32_t key;
  int32_t group;
  bool live, grouped;
  uint64_t word;
};
__device__ __forceinline__ GroupPos group_pos(const GroupArgs &a, int t, int lane) {
  GroupPos p;
  const int64_t i = (int64_t)t * 64 + lane;
  p.key = a.keys[i];
  const uint32_t row = a.list ? a.list[i] : (uint32_t)i;
  p.live = p.key != KEY_DEAD && row != 0xFFFFFFFFu;
  p.group = p.live && (int64_t)row < a.group_rows ? a.group_of[row] : -1;
  p.grouped = p.live && group_valid(p.group, a.n_groups);
  p.word = group_head_word(p.key, (uint32_t)i);
  return p;
}

// G1
static __global__ void __launch_bounds__(256) group_min_kernel(GroupArgs a) {
  const int lane = threadIdx.x & 63;
  const int t = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));  // a wave's tile: wave-uniform
  if (t >= a.n_tiles) return;
  if (a.gmin[t] == KEY_DEAD) return;
  const GroupPos p = group_pos(a, t, lane);
  const int32_t g = p.grouped ? p.group : -1;  // (-1: every ungrouped or dead lane; runs of them offer nothing)
  unsigned long long w = p.grouped ? p.word : GROUP_WORD_NONE;
  // runs of equal group ids: a lane starts one where its left neighbour's id differs
  const int32_t g_left = __shfl_up(g, 1);
  const uint64_t starts = __ballot(lane == 0 || g_left != g);
  const int my_start = 63 - __builtin_clzll(starts & (~0ull >> (63 - lane)));
  // segmented suffix minimum: after the step of width o, a lane holds the minimum of its run over [lane, lane + 2 o)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long w2 = __shfl_down(w, o);
    const int s2 = __shfl_down(my_start, o);
    if (lane + o < 64 && s2 == my_start && w2 < w) w = w2;
  }
  if (lane == my_start && w != GROUP_WORD_NONE) atomicMin(a.gm + g, w);
}

// G2
static __global__ void __launch_bounds__(256) group_heads_kernel(GroupArgs a) {
  const int lane = threadIdx.x & 63;
  const int t = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
  if (t >= a.n_tiles) return;
  const int64_t i = (int64_t)t * 64 + lane;
  if (a.gmin[t] == KEY_DEAD) {  // (stale keys by contract: the heads array is written whole all the same)
    a.heads[i] = KEY_DEAD;
    if (lane == 0) a.hmin[t] = KEY_DEAD;
    return;
  }
  const GroupPos p = group_pos(a, t, lane);
  const bool head = p.live && group_is_head(p.grouped, p.word, p.grouped ? a.gm[p.group] : 0ull);
  const uint32_t h = head ? p.key : KEY_DEAD;
  a.heads[i] = h;
  const uint32_t m = wave_min_u32(h);
  if (lane == 0) a.hmin[t] = m;
}

struct GroupSideArgs {
  GroupArgs g;
  const BlockHeader *hdr;  // the device header the select wrote: its band_key
  uint32_t *side_rows;     // local ids of the SIDE rows, side_cap of them at most
  uint32_t *side_count;    // all of them, written or not
  uint32_t side_cap;
  float eps_rel, delta_abs;
};

// G3
static __global__ void __launch_bounds__(256) group_side_kernel(GroupSideArgs s) {
  const GroupArgs &a = s.g;
  const int lane = threadIdx.x & 63;
  const int t = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
  if (t >= a.n_tiles) return;
  if (a.gmin[t] == KEY_DEAD) return;
  const uint32_t select_band = s.hdr->band_key;
  const GroupPos p = group_pos(a, t, lane);
  bool side = false;
  if (p.grouped && p.key <= select_band) {
    const unsigned long long hw = a.gm[p.group];
    side = hw != p.word && group_side(p.key, band_of(group_word_key(hw), s.eps_rel, s.delta_abs), select_band);
  }
  const uint64_t bm = __ballot(side);
  if (bm) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(s.side_count, (uint32_t)__popcll(bm));
    base = (uint32_t)__shfl((int)base, 0);
    if (side) {
      const uint32_t pos = base + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
      if (pos < s.side_cap) s.side_rows[pos] = a.list ? a.list[(int64_t)t * 64 + lane] : (uint32_t)((int64_t)t * 64 + lane);
    }
  }
}

}  // namespace tsh
