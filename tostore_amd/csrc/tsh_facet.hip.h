// tsh_facet.hip.h -- FACET counts ON the device: how many of the rows a search could return fall into each of the caller's
// buckets of an attribute column or hold each of the caller's keys in a tag column (tsh_attr_facets, tsh_tags_facets,
// include/tostore_hip.h; gfx950, wave = 64).
//
// The columns lie in HBM beside the rows (tsh_where.hip.h, tsh_tags.hip.h), the mask's words and the live bitmap too.  The
// mask makers W1 / W2 / T1 ballot a word per 64 rows; these two COUNT instead, in the same outer shape: one wave per
// 64-row word, grid-strided.  The host side -- the keys' normalisation, the bucket rule these kernels include, a model of
// one word, the quarantined rows' share -- is tsh_facet_plan.h.
//   F1 attr_facets_kernel   per workgroup the set S (sorted, at most 4096 keys: 32 KB) is staged in LDS once and |S| + 3
//                           32-bit counters are zeroed beside it (16 KB).  Per word: the word of d_live, and-ed with the
//                           mask's word if one is given (wave-uniform loads); lane l with its bit set and 64 w + l < rows
//                           loads vals[64 w + l] (one coalesced 512 B request per wave), finds its counter by
//                           facet_bucket -- a branch-free lower bound of <= 12 steps, then == (VALUES) or <= (EDGES) --
//                           and adds 1 to it in LDS; lane 0 adds the word's popcount to the total.  After its last word
//                           the workgroup adds every nonzero counter to the call's 64-bit counter in global memory.
//   F2 tags_facets_kernel   T1's span walk: the word's 65 offsets in LDS, the wave streams its rows' contiguous span of
//                           values 64 per pass, a lane finds its element's owner row by the 6-step search and, when the
//                           owner's bit of live & mask & valid is set and the value is a key, adds 1 to the key's LDS
//                           counter and to the owner's match counter.  After the span ballot(count == 0) over those rows
//                           is the word's `other` rows; live & mask & ~valid its NULL rows.
// Integer adds only: the counts do not depend on the order of arrival, two runs agree bit for bit.  The grid is capped at
// FACET_MAX_BLOCKS workgroups, far below W1's: every workgroup ends with up to |S| + 3 global atomics, and the column of
// 1 M rows is 8 MB ("facet counts").  The adds to one hot LDS counter (a column of one value) are left plain.
// No reference counterpart: the reference filters and counts on the host (lib/src/core/vector_index_manager.dart:1223-1378).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsh_facet_plan.h"
#include "tsh_tags.hip.h"

namespace tsh {

constexpr int FACET_BLOCK = WHERE_BLOCK;      // threads per workgroup: four waves, four words per pass
constexpr int FACET_WAVES = FACET_BLOCK / 64;
#ifndef TSH_FACET_MAX_BLOCKS
#define TSH_FACET_MAX_BLOCKS 256              // (A/B builds: -DTSH_FACET_MAX_BLOCKS=n, a variant library of its own)
#endif
constexpr int FACET_MAX_BLOCKS = TSH_FACET_MAX_BLOCKS;  // grid cap: one workgroup per CU

inline int facet_grid(int32_t n_words) {
  const int blocks = (n_words + FACET_WAVES - 1) / FACET_WAVES;
  return blocks < 1 ? 1 : (blocks > FACET_MAX_BLOCKS ? FACET_MAX_BLOCKS : blocks);
}
// dynamic shared memory of either kernel: S, then its counters
inline size_t facet_lds_bytes(int32_t n_set) { return (size_t)n_set * 8 + ((size_t)n_set + FACET_REST) * 4; }

// S into LDS and its counters zeroed (every thread of the workgroup calls it); -> the counters
static __device__ __forceinline__ uint32_t *facet_stage(int64_t *set, const int64_t *__restrict__ d_set, int32_t n_set) {
  uint32_t *cnt = reinterpret_cast<uint32_t *>(set + n_set);
  for (int32_t i = (int32_t)threadIdx.x; i < n_set; i += FACET_BLOCK) set[i] = d_set[i];
  for (int32_t i = (int32_t)threadIdx.x; i < n_set + FACET_REST; i += FACET_BLOCK) cnt[i] = 0u;
  __syncthreads();
  return cnt;
}
// ... and, after the workgroup's last word, every nonzero counter added to the call's
static __device__ __forceinline__ void facet_flush(const uint32_t *cnt, int32_t n_set, unsigned long long *__restrict__ d_cnt) {
  __syncthreads();
  for (int32_t i = (int32_t)threadIdx.x; i < n_set + FACET_REST; i += FACET_BLOCK) {
    const uint32_t c = cnt[i];
    if (c) atomicAdd(&d_cnt[i], (unsigned long long)c);
  }
}

// F1: d_cnt[b] += the rows of [0, rows) whose bit of live (& mask_words, if given) is set and whose value's counter is b.
// vals: rows values; live, mask_words: n_words words; d_set: n_set keys ascending; facet_lds_bytes(n_set) of dynamic LDS
static __global__ void __launch_bounds__(FACET_BLOCK) attr_facets_kernel(const int64_t *__restrict__ vals,
                                                                          const uint64_t *__restrict__ live,
                                                                          const uint64_t *__restrict__ mask_words, int64_t rows,
                                                                          int32_t n_words, const int64_t *__restrict__ d_set,
                                                                          int32_t n_set, int32_t kind,
                                                                          unsigned long long *__restrict__ d_cnt) {
  extern __shared__ int64_t facet_set[];
  uint32_t *cnt = facet_stage(facet_set, d_set, n_set);
  const int lane = threadIdx.x & 63;
  const int32_t step = (int32_t)gridDim.x * FACET_WAVES;
  for (int32_t w = (int32_t)blockIdx.x * FACET_WAVES + (int32_t)(threadIdx.x >> 6); w < n_words; w += step) {
    uint64_t act = live[w];
    if (mask_words) act &= mask_words[w];
    const int64_t r = (int64_t)w * 64 + lane;
    const bool on = ((act >> lane) & 1ull) && r < rows;
    if (on) atomicAdd(&cnt[facet_bucket(kind, facet_set, n_set, vals[r])], 1u);
    const uint64_t counted = __ballot(on);
    if (lane == 0 && counted) atomicAdd(&cnt[n_set + FACET_TOTAL], (uint32_t)__popcll(counted));
  }
  facet_flush(cnt, n_set, d_cnt);
}

// F2: the same over a tag column's part (off: rows + 1 offsets into vals; valid: n_words words): d_cnt[slot] += the
// counted rows that are valid and hold the key, `other` those that hold none, `null` the counted rows that are not valid
static __global__ void __launch_bounds__(FACET_BLOCK) tags_facets_kernel(const uint32_t *__restrict__ off,
                                                                          const int64_t *__restrict__ vals,
                                                                          const uint64_t *__restrict__ valid,
                                                                          const uint64_t *__restrict__ live,
                                                                          const uint64_t *__restrict__ mask_words, int64_t rows,
                                                                          int32_t n_words, const int64_t *__restrict__ d_set,
                                                                          int32_t n_set, unsigned long long *__restrict__ d_cnt) {
  extern __shared__ int64_t facet_set[];
  __shared__ uint32_t facet_off[FACET_WAVES][65];
  __shared__ uint32_t facet_hits[FACET_WAVES][64];
  uint32_t *cnt = facet_stage(facet_set, d_set, n_set);
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t *woff = facet_off[wv], *whit = facet_hits[wv];
  const int32_t step = (int32_t)gridDim.x * FACET_WAVES;
  whit[lane] = 0;
  for (int32_t w = (int32_t)blockIdx.x * FACET_WAVES + wv; w < n_words; w += step) {
    const int64_t r0 = (int64_t)w * 64;
    uint64_t act = live[w] & __ballot(r0 + lane < rows);
    if (mask_words) act &= mask_words[w];
    const uint64_t ok = act & valid[w];  // the rows whose lists count
    if (n_set > 0 && ok) {
      // the word's 65 offsets in one request (+ lane 0's second); rows at or past `rows` repeat the last offset
      woff[lane] = off[r0 + lane < rows ? r0 + lane : rows];
      if (lane == 0) woff[64] = off[r0 + 64 < rows ? r0 + 64 : rows];
      tags_wave_sync();
      const uint32_t base = __builtin_amdgcn_readfirstlane(woff[0]);
      const uint32_t end = __builtin_amdgcn_readfirstlane(woff[64]);
      for (uint32_t p = base; p < end; p += 64) {
        const uint32_t e = p + (uint32_t)lane;
        if (e < end) {
          const int64_t v = vals[e];
          // the owner: the last row of the word whose list starts at or before e (its list ends past e, as e < end)
          int32_t own = 0;
#pragma unroll
          for (int32_t half = 32; half > 0; half >>= 1) own = woff[own + half] <= e ? own + half : own;
          const int32_t b = facet_bucket(FACET_VALUES, facet_set, n_set, v);
          if (b < n_set && ((ok >> own) & 1ull)) {
            atomicAdd(&cnt[b], 1u);
            atomicAdd(&whit[own], 1u);
          }
        }
      }
      tags_wave_sync();
    }
    const uint32_t c = whit[lane];
    whit[lane] = 0;  // (for the wave's next word)
    const uint64_t other = __ballot(c == 0) & ok, nulls = act & ~valid[w];
    if (lane == 0) {
      if (other) atomicAdd(&cnt[n_set + FACET_OTHER], (uint32_t)__popcll(other));
      if (nulls) atomicAdd(&cnt[n_set + FACET_NULLS], (uint32_t)__popcll(nulls));
      if (act) atomicAdd(&cnt[n_set + FACET_TOTAL], (uint32_t)__popcll(act));
    }
    tags_wave_sync();  // (the offsets and the match counters are overwritten next)
  }
  facet_flush(cnt, n_set, d_cnt);
}

}  // namespace tsh
