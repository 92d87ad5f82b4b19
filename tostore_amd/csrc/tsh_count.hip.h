// tsh_count.hip.h -- device side of a count (tsh_search_count, include/tostore_hip.h): how many rows the list of
// tsh_search_after holds, for one query, threshold, mask and cursor.  gfx950, wave = 64.
//
// A count job is an f32 tile scan or list scan like any other; then, in place of select and re-rank, one pass over what
// the scan left in the context -- a key per row, a minimum per tile: 4 MB + 64 KB at 1 M rows -- and a handful of exact rows:
//   C1 count_window_kernel  a wave per tile at a time, after_floor_kernel's shape, four tiles per wave.  The host turned cursor and
//                           threshold into the window's four keys (tsh_count_band.h, where the proof is).  in_lo <= key <=
//                           in_hi: IN the list for certain -- the wave sums the popcounts of their ballots, the workgroup
//                           adds its sixteen tiles' sum to the job's count word.
//                           key < out_lo, or beyond out_hi and finite: OUT for certain.  Everything else is AMBIGUOUS: the
//                           row's id goes to the context's side list (the cursor searches' own: an atomic count, ids past
//                           the list's capacity counted, not written).  Tiles whose gmin is KEY_DEAD are skipped unread,
//                           dead keys and list padding are skipped; keys and gmin are only read.
//   C2 count_side_kernel    after_side_kernel's sibling: the AMBIGUOUS rows' exact f64 sums, a wave per row, by the
//                           re-rank's own code (rerank_rows), into pinned host memory with their count -- and the certain
//                           count with them ([0].s0: a u32 as a double, exact).  The finaliser decides the side rows by the
//                           exact predicate (count_passes) and adds.
// No select, no re-rank, no wide-band pass, no candidate block: the output is one integer however many rows qualify.
// The side count alternates between the context's two words as for cursor jobs (C2 leaves the one the context's NEXT
// cursor or count job counts in at zero); the certain count has one word, which C2's first lane reads and clears -- a
// context runs one job at a time -- so a count adds two dispatches and no clear.
//
// Out of scope here, as for cursors: the fp16 / int8 routes and the exact path (a count job always takes the f32 tile
// scan or the list scan); the batched matrix-core path.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsh_kernels.hip.h"

namespace tsh {

constexpr uint32_t COUNT_KEY_INF_DEV = 0xFF800000u;  // f2key(+inf): tsh_count_band.h's COUNT_KEY_INF

struct CountWindowArgs {
  const uint32_t *keys;  // n_tiles * 64, as the scan left them (list scans: in list order)
  const uint32_t *gmin;  // n_tiles
  const uint32_t *list;  // list scans: position -> local row id (0xFFFFFFFF: padding); NULL: position = row
  uint32_t *side_rows;   // local ids of the AMBIGUOUS rows, side_cap of them at most
  uint32_t *side_count;  // all of them, written or not
  uint32_t *certain;     // the IN rows
  int32_t n_tiles;
  uint32_t side_cap;
  uint32_t in_lo, in_hi, out_lo, out_hi;  // CountWindow
};

constexpr int COUNT_WAVE_TILES = 4;  // tiles a wave of C1 classifies: a workgroup of four waves covers 16 tiles

// C1.  Every tile's IN rows added straight to the one count word was measured first: 15 625 atomic adds on one address at
// 1 M rows and a threshold at the corpus' median distance, 180 us of a 646 us count.  Hence a register per wave, LDS
// across the four waves and one add per workgroup (the side list's adds stay per tile: it has a few rows per search)
static __global__ void __launch_bounds__(256) count_window_kernel(CountWindowArgs a) {
  __shared__ uint32_t s_in[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t0 = (int)(blockIdx.x * 4u + (uint32_t)wave) * COUNT_WAVE_TILES;  // a wave's first tile: everything below is wave-uniform
  uint32_t n_in = 0;
#pragma unroll
  for (int u = 0; u < COUNT_WAVE_TILES; ++u) {
    const int t = t0 + u;
    if (t >= a.n_tiles) break;
    if (a.gmin[t] == KEY_DEAD) continue;
    const int64_t i = (int64_t)t * 64 + lane;
    const uint32_t key = a.keys[i];
    const uint32_t row = a.list ? a.list[i] : (uint32_t)i;
    const bool live = key != KEY_DEAD && row != 0xFFFFFFFFu;
    // (count_window_class, tsh_count_band.h)
    const bool in = live && key >= a.in_lo && key <= a.in_hi;
    const bool out = key < a.out_lo || (key > a.out_hi && key < COUNT_KEY_INF_DEV);
    const bool side = live && !in && !out;
    n_in += (uint32_t)__popcll(__ballot(in));
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
  }
  if (lane == 0) s_in[wave] = n_in;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t sum = s_in[0] + s_in[1] + s_in[2] + s_in[3];
    if (sum) atomicAdd(a.certain, sum);
  }
}

struct CountSideArgs {
  const float *rows;
  const float *query;          // the context's device copy, ld floats
  const uint32_t *side_rows;
  const uint32_t *side_count;  // this job's word ...
  uint32_t *next_count;        // ... and the other one, left at zero for the context's next cursor or count job
  uint32_t *certain;           // read and cleared
  BlockEntry *out;             // pinned host memory: [0].id = the side count (capacity or not), [0].s0 = the certain count,
                               // [1 + c] = side row c's entry
  int64_t ld, row_base;
  int32_t dim, metric;
  uint32_t side_cap;
};

// C2: a wave per row, as the re-rank has it
static __global__ void __launch_bounds__(64) count_side_kernel(CountSideArgs a) {
  __shared__ __attribute__((aligned(16))) double t0[RR_CHUNK];
  __shared__ __attribute__((aligned(16))) double t1[RR_CHUNK];
  const uint32_t total = *a.side_count;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.out[0].id = (int64_t)total;
    a.out[0].s0 = (double)*a.certain;
    *a.certain = 0u;
    *a.next_count = 0u;
  }
  const RerankArgs r{a.rows, a.query, a.side_rows, a.side_count, a.out + 1, a.ld, a.row_base, a.dim, (int32_t)a.side_cap, a.metric};
  rerank_rows(r, total < a.side_cap ? total : a.side_cap, t0, t1);
}

}  // namespace tsh
