// tsh_group_rows.hip.h -- device side of a grouped search with several rows per group (tsh_search_grouped_rows,
// include/tostore_hip.h): the m nearest rows of each of the k nearest groups, for one query.  gfx950, wave = 64.  The rules
// and their proof are in tsh_group_rows_rule.h.
//
// A rows job is a grouped job (tsh_group.hip.h) up to its re-rank: scan, G1, G2, select, re-rank.  In G3's place five small
// passes follow on the job's stream, over the keys, the heads array and the head table gm[] the job has on the device:
//   R1 group_rows_mark_kernel    a wave per tile.  A grouped head (heads[i] alive) whose key is at or below the band_key
//                                the select left marks its group: the marking heads of a tile draw slot numbers through a
//                                ballot and ONE atomic, and each overwrites its group's gm[] word with the slot word.  One
//                                head per group, so one writer per word.  Slots past the capacity are counted, not written.
//   R2 group_rows_member_kernel<false>   a wave per tile counts every live row of a slotted group into cnt[slot].  Rows of a
//                                document are inserted together: a RUN of equal slots inside the wave issues one atomic.
//   R3 group_rows_alloc_kernel   a thread per slot draws its segment's offset from the member total (one atomic add each:
//                                the order of the segments is whatever it comes to, the contents do not depend on it).
//   R4 group_rows_member_kernel<true>    R2 again, now writing  key << 32 | position  at off[slot] + the run's place (one
//                                atomic per run on cur[slot]).  Words past the segment space are counted (R3's total),
//                                not written.
//   R5 group_rows_pick_kernel    a workgroup per slot.  A segment of at most m rows goes on whole; else tau_g, the m-th
//                                smallest key, by a radix select in LDS (four passes over the segment), and the rows at or
//                                below band_of(tau_g) go on -- to the context's side list, by group_side_push.  A segment
//                                that did not fit is left alone: the host redoes the job with room for R3's total.
//   (after_side_kernel, tsh_after.hip.h, then takes the side rows' exact sums by the re-rank's own code)
// The host reads the marked groups and the member total beside the side list's count and redoes a job whose lists
// overflowed once, with lists sized from these counts; a job with more marked groups than slots runs again on the
// exact-all route.
// Bounds: a group is read through group_pos (checked against n_groups), a slot against slot_cap where its word is read
// (group_word_is_slot), a segment index against seg_cap, a position against n_tiles * 64 before the list is read.  Every
// branch around a ballot or a shuffle is wave-uniform (a wave's tile, a tile's gmin, a workgroup's slot).  Dead tiles are
// skipped unread; list scans map positions through the list and skip its padding.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsh_group.hip.h"
#include "tsh_group_rows_rule.h"

namespace tsh {

constexpr int GROUP_ROWS_CTL = 4;  // control words in front of the slot arrays: [0] marked groups, [1] member rows

struct GroupRowsArgs {
  GroupArgs g;
  const BlockHeader *hdr;   // the device header the select wrote: its band_key
  uint32_t *ctl;            // GROUP_ROWS_CTL words, zero in front of a job
  uint32_t *cnt, *cur;      // per slot: live rows (R2), rows placed (R4); zero in front of a job
  uint32_t *off;            // per slot: where its segment starts (R3)
  unsigned long long *seg;  // seg_cap words
  uint32_t slot_cap, seg_cap;
  uint32_t m;               // rows per group
  uint32_t *side_rows;      // the context's side list, as in GroupSideArgs
  uint32_t *side_count;
  uint32_t side_cap;
  float eps_rel, delta_abs;
  BlockEntry *report;       // pinned host memory, the side list's [0]: s0 = marked groups, s1 = member rows
};

// R1
static __global__ void __launch_bounds__(256) group_rows_mark_kernel(GroupRowsArgs r) {
  const GroupArgs &a = r.g;
  const int lane = threadIdx.x & 63;
  const int t = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));  // a wave's tile: wave-uniform
  if (t >= a.n_tiles) return;
  if (a.gmin[t] == KEY_DEAD) return;
  const uint32_t band_key = r.hdr->band_key;
  const GroupPos p = group_pos(a, t, lane);
  const bool head = p.grouped && a.heads[(int64_t)t * 64 + lane] != KEY_DEAD;
  const bool mark = group_rows_marked(head, p.key, band_key);
  const uint64_t bm = __ballot(mark);
  if (bm) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(r.ctl, (uint32_t)__popcll(bm));
    base = (uint32_t)__shfl((int)base, 0);
    if (mark) {
      const uint32_t slot = base + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
      if (slot < r.slot_cap) a.gm[p.group] = group_slot_word(slot);
    }
  }
}

// R2 (FILL == false) and R4 (FILL == true)
template <bool FILL>
static __global__ void __launch_bounds__(256) group_rows_member_kernel(GroupRowsArgs r) {
  const GroupArgs &a = r.g;
  const int lane = threadIdx.x & 63;
  const int t = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));
  if (t >= a.n_tiles) return;
  if (a.gmin[t] == KEY_DEAD) return;
  const GroupPos p = group_pos(a, t, lane);
  const unsigned long long w = p.grouped ? a.gm[p.group] : GROUP_WORD_NONE;
  const bool member = p.grouped && group_word_is_slot(w, r.slot_cap);
  const int32_t s = member ? (int32_t)group_word_slot(w) : -1;  // (-1: runs of other lanes place nothing)
  // runs of equal slots, as G1 has them: a lane starts one where its left neighbour's slot differs
  const int32_t s_left = __shfl_up(s, 1);
  const uint64_t starts = __ballot(lane == 0 || s_left != s);
  const int my_start = 63 - __builtin_clzll(starts & (~0ull >> (63 - lane)));
  const uint64_t above = lane == 63 ? 0ull : starts & (~0ull << (lane + 1));
  const uint32_t run_len = (uint32_t)((above ? __builtin_ctzll(above) : 64) - my_start);
  if (!FILL) {
    if (member && lane == my_start) atomicAdd(r.cnt + s, run_len);
  } else {
    uint32_t base = 0;
    if (member && lane == my_start) base = atomicAdd(r.cur + s, run_len);
    base = (uint32_t)__shfl((int)base, my_start);
    if (member) {
      const uint64_t at = (uint64_t)r.off[s] + base + (uint32_t)(lane - my_start);
      if (at < (uint64_t)r.seg_cap) r.seg[at] = p.word;
    }
  }
}

// R3
static __global__ void __launch_bounds__(256) group_rows_alloc_kernel(GroupRowsArgs r) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  const uint32_t marked = r.ctl[0] < r.slot_cap ? r.ctl[0] : r.slot_cap;
  if (s >= marked) return;
  r.off[s] = atomicAdd(r.ctl + 1, r.cnt[s]);
}

// R5
static __global__ void __launch_bounds__(256) group_rows_pick_kernel(GroupRowsArgs r) {
  __shared__ uint32_t hist[256];
  const GroupArgs &a = r.g;
  const int lane = threadIdx.x & 63;
  const uint32_t s = blockIdx.x;  // a workgroup's slot: everything below is uniform over the workgroup
  const uint32_t marked = r.ctl[0];
  if (s == 0 && threadIdx.x == 0) {
    r.report[0].s0 = (double)marked;
    r.report[0].s1 = (double)r.ctl[1];
  }
  if (s >= (marked < r.slot_cap ? marked : r.slot_cap)) return;
  const uint32_t n = r.cnt[s], o = r.off[s];
  if (n == 0 || (uint64_t)o + n > (uint64_t)r.seg_cap) return;
  const unsigned long long *sg = r.seg + o;
  const bool all = group_rows_takes_all(n, r.m);
  uint32_t band = KEY_NAN;
  if (!all) {
    uint32_t prefix = 0, remaining = r.m;
    for (int shift = 24; shift >= 0; shift -= 8) {
      const uint32_t mask = shift == 24 ? 0u : ~0u << (shift + 8);
      hist[threadIdx.x] = 0;
      __syncthreads();
      for (uint32_t i = threadIdx.x; i < n; i += 256u) {
        const uint32_t key = group_word_key(sg[i]);
        if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      prefix |= group_rows_radix_digit(hist, &remaining) << shift;  // (every thread takes the same step)
      __syncthreads();
    }
    band = band_of(prefix, r.eps_rel, r.delta_abs);
  }
  const uint64_t n_pos = (uint64_t)a.n_tiles * 64u;
  for (uint32_t i0 = 0; i0 < n; i0 += 256u) {
    const uint32_t i = i0 + threadIdx.x;
    const unsigned long long w = i < n ? sg[i] : GROUP_WORD_NONE;
    const uint32_t pos = (uint32_t)w;
    bool take = i < n && (all || group_rows_member(group_word_key(w), band)) && (uint64_t)pos < n_pos;
    const uint32_t row = take ? (a.list ? a.list[pos] : pos) : 0xFFFFFFFFu;
    take = take && row != 0xFFFFFFFFu;
    group_side_push(take, row, lane, r.side_rows, r.side_count, r.side_cap);
  }
}

}  // namespace tsh
