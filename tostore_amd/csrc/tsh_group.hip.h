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

#include "tsh_group_after_rule.h"
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

// ---- grouped cursor searches and group counts (tsh_search_grouped_after, tsh_search_grouped_count) ----------------------
// The rules and their proof are in tsh_group_after_rule.h.  G1 runs unchanged -- the head table is built over ALL live
// rows, whatever the cursor: a group whose best row is at or before the cursor is consumed, rows past the cursor included --
// and the passes below take the places of G2 and G3, or of select, re-rank and G3 altogether for a count:
//   G2a group_heads_after_kernel   G2 with the cursor's floor keys: a head certainly AFTER the cursor keeps its key in the
//                                  heads array, a head certainly BEFORE it becomes KEY_DEAD (its group is consumed), an
//                                  AMBIGUOUS head becomes KEY_DEAD and its id goes to the side list.
//   G3a group_side_after_kernel    G3 with the floor keys: rows of an AFTER group are SIDE as in G3, rows of a BEFORE group
//                                  go nowhere, rows of an AMBIGUOUS group at or below band_of(head key) go to the side
//                                  list whatever the select's band says.
//   GC  group_count_window_kernel  count_window_kernel's shape (four tiles per wave, one LDS-reduced atomic per workgroup,
//                                  for the reason written there) over heads: a head certainly IN the window counts one
//                                  group, a head certainly OUT none; an AMBIGUOUS head and its group's rows at or below
//                                  band_of(head key) go to the side list.
// All of them draw places in the context's one side list through the job's one count word (a ballot, one atomic per tile
// that has such rows); after_side_kernel / count_side_kernel take the exact sums.  Every branch around a ballot or a
// shuffle is wave-uniform (a wave's tile, a tile's gmin).

// the lanes with `side` set append `row` to the side list: ids past the capacity are counted, not written
__device__ __forceinline__ void group_side_push(bool side, uint32_t row, int lane, uint32_t *side_rows, uint32_t *side_count, uint32_t side_cap) {
  const uint64_t bm = __ballot(side);
  if (bm) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(side_count, (uint32_t)__popcll(bm));
    base = (uint32_t)__shfl((int)base, 0);
    if (side) {
      const uint32_t pos = base + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
      if (pos < side_cap) side_rows[pos] = row;
    }
  }
}

struct GroupHeadsAfterArgs {
  GroupArgs g;
  uint32_t *side_rows;   // local ids of the AMBIGUOUS heads, side_cap of them at most
  uint32_t *side_count;  // all of them, written or not
  uint32_t side_cap;
  uint32_t floor_lo, floor_hi;  // AfterFloor
};

// G2a
static __global__ void __launch_bounds__(256) group_heads_after_kernel(GroupHeadsAfterArgs h) {
  const GroupArgs &a = h.g;
  const int lane = threadIdx.x & 63;
  const int t = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
  if (t >= a.n_tiles) return;
  const int64_t i = (int64_t)t * 64 + lane;
  if (a.gmin[t] == KEY_DEAD) {
    a.heads[i] = KEY_DEAD;
    if (lane == 0) a.hmin[t] = KEY_DEAD;
    return;
  }
  const GroupPos p = group_pos(a, t, lane);
  const bool head = p.live && group_is_head(p.grouped, p.word, p.grouped ? a.gm[p.group] : 0ull);
  const int cls = group_after_class(p.key, h.floor_lo, h.floor_hi);
  const uint32_t hk = head && cls == GROUP_AFTER ? p.key : KEY_DEAD;
  a.heads[i] = hk;
  group_side_push(head && cls == GROUP_AMBIGUOUS, a.list ? a.list[i] : (uint32_t)i, lane, h.side_rows, h.side_count, h.side_cap);
  const uint32_t m = wave_min_u32(hk);
  if (lane == 0) a.hmin[t] = m;
}

struct GroupSideAfterArgs {
  GroupSideArgs s;
  uint32_t floor_lo, floor_hi;  // AfterFloor
};

// G3a
static __global__ void __launch_bounds__(256) group_side_after_kernel(GroupSideAfterArgs sa) {
  const GroupSideArgs &s = sa.s;
  const GroupArgs &a = s.g;
  const int lane = threadIdx.x & 63;
  const int t = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
  if (t >= a.n_tiles) return;
  if (a.gmin[t] == KEY_DEAD) return;
  const uint32_t select_band = s.hdr->band_key;
  // (an AMBIGUOUS group's head key is at most floor_hi, band_of is monotone: no row above both bands can be wanted)
  const uint32_t floor_band = band_of(sa.floor_hi, s.eps_rel, s.delta_abs);
  const GroupPos p = group_pos(a, t, lane);
  bool side = false;
  if (p.grouped && (p.key <= select_band || p.key <= floor_band)) {
    const unsigned long long hw = a.gm[p.group];
    const uint32_t hk = group_word_key(hw);
    side = hw != p.word &&
           group_after_side(group_after_class(hk, sa.floor_lo, sa.floor_hi), p.key, band_of(hk, s.eps_rel, s.delta_abs), select_band);
  }
  group_side_push(side, a.list ? a.list[(int64_t)t * 64 + lane] : (uint32_t)((int64_t)t * 64 + lane), lane, s.side_rows, s.side_count, s.side_cap);
}

struct GroupCountArgs {
  GroupArgs g;           // (heads / hmin unused)
  uint32_t *side_rows;   // local ids of the AMBIGUOUS groups' rows, side_cap of them at most
  uint32_t *side_count;  // all of them, written or not
  uint32_t *certain;     // the groups certainly IN
  uint32_t side_cap;
  uint32_t in_lo, in_hi, out_lo, out_hi;  // CountWindow
  float eps_rel, delta_abs;
};

constexpr int GROUP_COUNT_WAVE_TILES = 4;  // as COUNT_WAVE_TILES (tsh_count.hip.h)

// GC
static __global__ void __launch_bounds__(256) group_count_window_kernel(GroupCountArgs c) {
  __shared__ uint32_t s_in[4];
  const GroupArgs &a = c.g;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t0 = (int)(blockIdx.x * 4u + (uint32_t)wave) * GROUP_COUNT_WAVE_TILES;  // a wave's first tile: wave-uniform
  uint32_t n_in = 0;
#pragma unroll
  for (int u = 0; u < GROUP_COUNT_WAVE_TILES; ++u) {
    const int t = t0 + u;
    if (t >= a.n_tiles) break;
    if (a.gmin[t] == KEY_DEAD) continue;
    const GroupPos p = group_pos(a, t, lane);
    const unsigned long long hw = p.grouped ? a.gm[p.group] : p.word;  // (ungrouped: its own head)
    const bool head = p.live && hw == p.word;
    const uint32_t hk = group_word_key(hw);
    const int cls = group_count_class(hk, c.in_lo, c.in_hi, c.out_lo, c.out_hi);
    const bool in = head && cls == 0;
    const bool side = p.live && cls == 2 && (head || p.key <= band_of(hk, c.eps_rel, c.delta_abs));
    n_in += (uint32_t)__popcll(__ballot(in));
    group_side_push(side, a.list ? a.list[(int64_t)t * 64 + lane] : (uint32_t)((int64_t)t * 64 + lane), lane, c.side_rows, c.side_count, c.side_cap);
  }
  if (lane == 0) s_in[wave] = n_in;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t sum = s_in[0] + s_in[1] + s_in[2] + s_in[3];
    if (sum) atomicAdd(c.certain, sum);
  }
}

}  // namespace tsh
