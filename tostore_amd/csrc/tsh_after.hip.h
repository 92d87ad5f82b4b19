// tsh_after.hip.h -- device side of a cursor search (tsh_search_after, include/tostore_hip.h): the next k rows past a
// (distance, id) the caller saw last.  gfx950, wave = 64.
//
// A cursor job is an f32 tile scan or list scan like any other; between the scan and the select one pass over what the
// scan left in the context -- a key per row, a minimum per tile: 4 MB + 64 KB at 1 M rows, against the scan's 3 GB --
// takes the rows at or before the cursor out of the select's sight:
//   A1 after_floor_kernel   one wave per tile.  The host turned the cursor's distance into two keys floor_lo <= floor_hi
//                           (tsh_after_band.h, where the proof is).  key < floor_lo: BEFORE the cursor for certain, the key
//                           becomes KEY_DEAD.  key > floor_hi: AFTER it for certain, untouched.  In between, AMBIGUOUS:
//                           KEY_DEAD as well, and the row's id goes to the context's side list (an atomic count; ids
//                           past the list's capacity are counted, not written, as mask_compact_kernel does).  gmin[t]
//                           becomes the minimum over the tile's AFTER rows.  A tile whose gmin is KEY_DEAD already is
//                           skipped unread: its keys are stale by contract.
//   (select_kernel, rerank_kernel and on overflow the wide-band pass then see the AFTER rows only, with every guarantee
//   they give today)
//   A2 after_side_kernel    the AMBIGUOUS rows' exact f64 sums, a wave per row, by the re-rank's own code (rerank_rows:
//                           strictly in element order), into pinned host memory with their count; the finaliser
//                           decides them by (distance, id).  (A lane per row, the quarantine kernel's shape, was
//                           measured first: its one dependent load chain per row cost a lone 1 M x 768 page 45 us more.)
// The side count alternates between two words: A2 leaves the one the context's NEXT cursor job counts in at zero, so no
// launch is spent on clearing it.
//
// Out of scope here: cursors on the fp16 / int8 routes and on the exact path (a cursor job always takes the f32 tile
// scan or the list scan); the batched matrix-core path (several queries per call run as the usual pipeline of
// single-query scans); tsh_search_shard* / tsh_search_sharded (a sharded caller pages per shard and merges).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsh_kernels.hip.h"

namespace tsh {

struct AfterFloorArgs {
  uint32_t *keys;        // n_tiles * 64, as the scan left them (list scans: in list order)
  uint32_t *gmin;        // n_tiles
  const uint32_t *list;  // list scans: position -> local row id (0xFFFFFFFF: padding); NULL: position = row
  uint32_t *side_rows;   // local ids of the AMBIGUOUS rows, side_cap of them at most
  uint32_t *side_count;  // all of them, written or not
  int32_t n_tiles;
  uint32_t side_cap;
  uint32_t floor_lo, floor_hi;
};

// A1
static __global__ void __launch_bounds__(256) after_floor_kernel(AfterFloorArgs a) {
  const int lane = threadIdx.x & 63;
  const int t = (int)(blockIdx.x * 4u + (threadIdx.x >> 6));  // a wave's tile: everything below is wave-uniform
  if (t >= a.n_tiles) return;
  if (a.gmin[t] == KEY_DEAD) return;
  const int64_t i = (int64_t)t * 64 + lane;
  const uint32_t key = a.keys[i];
  const uint32_t row = a.list ? a.list[i] : (uint32_t)i;
  const bool live = key != KEY_DEAD && row != 0xFFFFFFFFu;
  const bool after = live && key > a.floor_hi;
  const bool side = live && !after && key >= a.floor_lo;
  if (live && !after) a.keys[i] = KEY_DEAD;
  const uint64_t bm = __ballot(side);
  if (bm) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(a.side_count, (uint32_t)__popcll(bm));
    base = (uint32_t)__shfl((int)base, 0);
    if (side) {
      const uint32_t p = base + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull));
      if (p < a.side_cap) a.side_rows[p] = row;
    }
  }
  const uint32_t m = wave_min_u32(after ? key : KEY_DEAD);
  if (lane == 0) a.gmin[t] = m;
}

struct AfterSideArgs {
  const float *rows;
  const float *query;          // the context's device copy, ld floats
  const uint32_t *side_rows;
  const uint32_t *side_count;  // this job's word ...
  uint32_t *next_count;        // ... and the other one, left at zero for the context's next cursor job
  BlockEntry *out;             // pinned host memory: [0].id = the count (capacity or not), [1 + c] = row c's entry
  int64_t ld, row_base;
  int32_t dim, metric;
  uint32_t side_cap;
};

// A2: a wave per row, as the re-rank has it
static __global__ void __launch_bounds__(64) after_side_kernel(AfterSideArgs a) {
  __shared__ __attribute__((aligned(16))) double t0[RR_CHUNK];
  __shared__ __attribute__((aligned(16))) double t1[RR_CHUNK];
  const uint32_t total = *a.side_count;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.out[0].id = (int64_t)total;
    *a.next_count = 0u;
  }
  const RerankArgs r{a.rows, a.query, a.side_rows, a.side_count, a.out + 1, a.ld, a.row_base, a.dim, (int32_t)a.side_cap, a.metric};
  rerank_rows(r, total < a.side_cap ? total : a.side_cap, t0, t1);
}

}  // namespace tsh
