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
//                           past the list's capacity are counted, not written, as i8_list_kernel does).  gmin[t]
//                           becomes the minimum over the tile's AFTER rows.  A tile whose gmin is KEY_DEAD already is
//                           skipped unread: its keys are stale by contract.
//   (select_kernel, rerank_kernel and on overflow the wide-band pass then see the AFTER rows only, with every guarantee
//   they give today)
//   A2 after_side_kernel    the AMBIGUOUS rows' exact f64 sums, a wave per row, by the re-rank's own code (rerank_rows:
//                           strictly in element order), into pinned host memory with their count; the finaliser
//                           decides them by (distance, id).  (A lane per row, the quarantine kernel's shape, was
//                           measured first: its one dependent load chain per row cost a lone 1 M x 768 page 45 us more.)
//   A2' after_side_append_kernel   shard mode (tsh_search_shard_after, tsh_search_sharded_after): the job's block lives
//                           in device memory and is all-gathered device to device, so the AMBIGUOUS rows' entries are
//                           APPENDED to it -- the same sums by the same code, a wave per row; the position comes from an
//                           atomic add on BlockHeader.count, as quarantine_append_kernel has it: a position at or
//                           beyond `entries` is counted, not written, which is the blocks' own overflow protocol.  The
//                           merge (tsh_merge_candidates_after) decides every entry by (distance, id).
// The side count alternates between two words: A2 / A2' leave the one the context's NEXT cursor job counts in at zero,
// so no launch is spent on clearing it; both report the list's total to the pinned word the host reads (a list that
// overflowed is redone with room for that many).
//
// Out of scope here: cursors on the fp16 / int8 routes and on the exact path (a cursor job always takes the f32 tile
// scan or the list scan); the batched matrix-core path (several queries per call run as the usual pipeline of
// single-query scans, in shard mode too).
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

struct AfterSideAppendArgs {
  const float *rows;
  const float *query;          // the context's device copy, ld floats
  const uint32_t *side_rows;
  const uint32_t *side_count;  // this job's word ...
  uint32_t *next_count;        // ... and the other one, left at zero for the context's next cursor job
  int64_t *total_out;          // pinned host memory: the count (capacity or not), for the host's redo
  uint8_t *block;              // the job's device block: header, then `entries` entries
  int64_t ld, row_base;
  int32_t dim, metric;
  uint32_t side_cap;
  int32_t entries;
};

// A2': a wave per row, the re-rank's own sums (rerank_row_sums); lane 0 draws the entry's place in the block
static __global__ void __launch_bounds__(64) after_side_append_kernel(AfterSideAppendArgs a) {
  __shared__ __attribute__((aligned(16))) double t0[RR_CHUNK];
  __shared__ __attribute__((aligned(16))) double t1[RR_CHUNK];
  const uint32_t total = *a.side_count;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *a.total_out = (int64_t)total;
    *a.next_count = 0u;
  }
  BlockHeader *hdr = reinterpret_cast<BlockHeader *>(a.block);
  BlockEntry *out = reinterpret_cast<BlockEntry *>(a.block + sizeof(BlockHeader));
  const RerankArgs r{a.rows, a.query, a.side_rows, a.side_count, out, a.ld, a.row_base, a.dim, a.entries, a.metric};
  const uint32_t count = total < a.side_cap ? total : a.side_cap;
  const int lane = threadIdx.x;
  const int chains = a.metric == METRIC_COS ? 2 : 1;  // lane 0: s0, lane 1: row norm
  for (uint32_t c = blockIdx.x; c < count; c += gridDim.x) {  // (wave-uniform: the sums synchronise the workgroup)
    const uint32_t row = a.side_rows[c];
    const double s = rerank_row_sums(r, a.rows + (int64_t)row * a.ld, lane, chains, t0, t1);
    const double s1 = __shfl(s, 1);
    if (lane == 0) {
      const uint32_t pos = atomicAdd(&hdr->count, 1u);
      if (pos < (uint32_t)a.entries) {
        out[pos].id = a.row_base + (int64_t)row;
        out[pos].s0 = s;
        out[pos].s1 = a.metric == METRIC_COS ? s1 : 0.0;
      }
    }
  }
}

}  // namespace tsh
