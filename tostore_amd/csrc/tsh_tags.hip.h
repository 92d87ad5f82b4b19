// tsh_tags.hip.h -- a HAS ANY / HAS ALL term over a TAG column evaluated ON the device: one array-valued attribute, kept
// beside the rows as CSR by local row id, made into the words of a mask handle (gfx950, wave = 64).
//
// A tag column (tsh_tags_create, include/tostore_hip.h) holds a SET of int64 per row: `acl HAS ANY (the caller's group
// ids)`, `tags HAS ALL ('gpu', 'rocm')`.  No scalar column can hold it, and on the host the ragged walk per query is worse
// than the scalar routes W1 / W2 (tsh_where.hip.h) replaced.  A part keeps, per shard: 32-bit offsets (rows + 1), the
// values (every row's list sorted and deduplicated by the host, tsh_tags_plan.h), and VALID words (bit r of word t: local
// row 64 t + r exists in the column and is not NULL).
//   T1 mask_tags_kernel   the outer shape of W1 / W2: one wave per 64-row word, grid-strided.  The ragged data does not
//                         become per-lane pointer chasing: a wave's 64 rows are consecutive, so their values are ONE
//                         contiguous span vals[off[64 w] .. off[64 w + 64]), which the wave streams 64 elements per
//                         pass -- lane l reads element base + 64 p + l, one coalesced 512 B request.  The wave's up to
//                         65 offsets lie in LDS; a lane finds its element's owner row by a branch-free search of 6
//                         steps over them, tests the value against the term's set S (sorted, in LDS, staged once per
//                         workgroup: where_in_set) and on a match adds 1 to the owner's 32-bit LDS counter.  Rows are
//                         sets, so counter i ends as c_i = |row_i n S|.  Then lane l reads counter l and
//                           word = (ballot(c >= t) ^ (negate ? ~0 : 0)) & valid[w]
//                         combined with the other handle's word if one is given; lane 0 stores it.
// The span's bounds and pass count are wave-uniform and held in scalar registers.  t = 0 (HAS ALL of nothing) needs no
// special case; an empty S skips the span loop.  Lanes at or past `rows` have valid bit 0, so the tail word needs no
// trimming.  The words come back to the host in one copy and mask_finish_part does the rest, as for W1 / W2.
// No reference counterpart: the reference has the field type (DataType.array, lib/src/model/table_schema.dart:1896) and
// would filter on the host (lib/src/core/vector_index_manager.dart:1223-1378).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsh_tags_plan.h"
#include "tsh_where.hip.h"

namespace tsh {

constexpr int TAGS_WAVES = WHERE_BLOCK / 64;  // waves per workgroup, each with its own offsets and counters in LDS

// Orders a wave's own LDS traffic: what its lanes wrote before is what its lanes read after (LDS operations of one wave
// complete in order; this keeps the compiler from moving them across)
static __device__ __forceinline__ void tags_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// T1: words[w] = the rows of [64 w, 64 w + 64) that are valid and whose count of set values reaches t (or, negated, does
// not), combined with with_words[w] if given.  off: rows + 1 offsets into vals; valid: n_words words; d_set: n_set values
// ascending, staged in n_set * 8 bytes of dynamic shared memory
static __global__ void __launch_bounds__(WHERE_BLOCK) mask_tags_kernel(const uint32_t *__restrict__ off,
                                                                        const int64_t *__restrict__ vals,
                                                                        const uint64_t *__restrict__ valid, int64_t rows,
                                                                        int32_t n_words, const int64_t *__restrict__ d_set,
                                                                        int32_t n_set, uint32_t t, int32_t negate,
                                                                        const uint64_t *__restrict__ with_words,
                                                                        int32_t combine, uint64_t *__restrict__ words) {
  extern __shared__ int64_t tags_set[];
  __shared__ uint32_t tags_off[TAGS_WAVES][65];
  __shared__ uint32_t tags_cnt[TAGS_WAVES][64];
  if (n_set > 0) {
    for (int32_t i = (int32_t)threadIdx.x; i < n_set; i += WHERE_BLOCK) tags_set[i] = d_set[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t *woff = tags_off[wv], *wcnt = tags_cnt[wv];
  const int32_t step = (int32_t)gridDim.x * TAGS_WAVES;
  wcnt[lane] = 0;
  for (int32_t w = (int32_t)blockIdx.x * TAGS_WAVES + wv; w < n_words; w += step) {
    // the word's 65 offsets in one request (+ lane 0's second); rows at or past `rows` repeat the last offset
    const int64_t r0 = (int64_t)w * 64;
    woff[lane] = off[r0 + lane < rows ? r0 + lane : rows];
    if (lane == 0) woff[64] = off[r0 + 64 < rows ? r0 + 64 : rows];
    tags_wave_sync();
    if (n_set > 0) {
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
          if (where_in_set(tags_set, n_set, v)) atomicAdd(&wcnt[own], 1u);
        }
      }
      tags_wave_sync();
    }
    const uint32_t c = wcnt[lane];
    wcnt[lane] = 0;  // (for the wave's next word)
    uint64_t word = (__ballot(c >= t) ^ (negate ? ~0ull : 0ull)) & valid[w];
    if (with_words) {
      const uint64_t o = with_words[w];
      word = combine == MASK_COMBINE_OR ? (word | o) : (word & o);
    }
    if (lane == 0) words[w] = word;
    tags_wave_sync();  // (the offsets are overwritten next)
  }
}

}  // namespace tsh
