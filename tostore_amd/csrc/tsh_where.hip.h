// tsh_where.hip.h -- a WHERE range term evaluated ON the device: one scalar attribute column, kept beside the rows by
// local row id, made into the words of a mask handle (gfx950, wave = 64).
//
// tsh_mask_create (tsh_mask.hip.h) takes a bitmap the HOST made: for `tenant = 7` or `ts BETWEEN a AND b` the caller
// evaluates the predicate row by row, packs the bits and hands them over, and the library slices, counts and uploads
// them again -- with a predicate per query that is the whole cost of a lone filtered query.  An attribute handle
// (tsh_attr_create, include/tostore_hip.h) keeps the column on the device, 8 B per row; a range term over it is
//   W1 mask_range_kernel   one wave per 64-row word, grid-strided: lane l loads vals[64 w + l] (one coalesced 512 B
//                          request per wave), evaluates  v != NULL && ((lo <= v && v <= hi) != negate),  and the
//                          wave's __ballot of that IS word w.  An optional second handle's word is and-ed / or-ed in,
//                          and lane 0 stores the word straight into the new handle's part: nothing is uploaded.
//   W2 mask_where_kernel   a whole clause in the same shape (tsh_mask_create_where): up to 32 range / IN terms over up
//                          to 8 columns, planned on the host (tsh_where_plan.h).  The term table and the column
//                          pointers travel in the kernel arguments; a lane loads each distinct column once; every
//                          term's ballot is or-ed into its clause's word and the clause's word and-ed into the result
//                          -- 64-bit scalar arithmetic, no per-lane state across terms.  The IN sets, sorted, lie in
//                          LDS (at most 4096 values, staged once per workgroup) and a lane finds its value by a
//                          branch-free binary search of at most 12 steps.
// Lanes at or past `rows` ballot 0, so the tail word needs no trimming (and under OR the other handle's own tail is 0
// already: every handle's words hold that).  The words come back to the host in one copy -- the batched path and the
// quarantined-row match read them there -- and a selective mask's list is M1 + M2 of tsh_mask.hip.h, unchanged.
// No reference counterpart: the reference filters on the host and maps primary keys to node ids
// (lib/src/core/vector_index_manager.dart:1223-1378) before its vector search, which itself takes no filter.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsh_where_plan.h"

namespace tsh {

constexpr int64_t ATTR_NULL = INT64_MIN;  // TSH_ATTR_NULL: the row has no value; kept by no term, negated or not
constexpr int WHERE_BLOCK = 256;          // threads per workgroup of W1: four waves, four words per pass
constexpr int WHERE_MAX_BLOCKS = 2048;    // grid cap (8 workgroups per CU of 256): 1 M rows are 4096 workgroups' worth

constexpr int MASK_COMBINE_AND = 0, MASK_COMBINE_OR = 1;  // TSH_MASK_AND / TSH_MASK_OR

// W1: words[w] = the rows of [64 w, 64 w + 64) below `rows` that the term keeps, combined with with_words[w] if given
static __global__ void __launch_bounds__(WHERE_BLOCK) mask_range_kernel(const int64_t *__restrict__ vals, int64_t rows,
                                                                         int32_t n_words, int64_t lo, int64_t hi,
                                                                         int32_t negate,
                                                                         const uint64_t *__restrict__ with_words,
                                                                         int32_t combine,
                                                                         uint64_t *__restrict__ words) {
  const int lane = threadIdx.x & 63;
  const int32_t step = (int32_t)gridDim.x * (WHERE_BLOCK / 64);
  for (int32_t w = (int32_t)blockIdx.x * (WHERE_BLOCK / 64) + (int32_t)(threadIdx.x >> 6); w < n_words; w += step) {
    const int64_t r = (int64_t)w * 64 + lane;
    bool keep = false;
    if (r < rows) {
      const int64_t v = vals[r];
      keep = v != ATTR_NULL && ((lo <= v && v <= hi) != (negate != 0));
    }
    uint64_t word = __ballot(keep);
    if (with_words) {
      const uint64_t o = with_words[w];
      word = combine == MASK_COMBINE_OR ? (word | o) : (word & o);
    }
    if (lane == 0) words[w] = word;
  }
}

inline int where_grid(int32_t n_words) {
  const int blocks = (n_words + WHERE_BLOCK / 64 - 1) / (WHERE_BLOCK / 64);
  return blocks < 1 ? 1 : (blocks > WHERE_MAX_BLOCKS ? WHERE_MAX_BLOCKS : blocks);
}

// W2's arguments besides the words: the plan's term records and the shard's slice of every distinct column (unused
// slots nullptr), about 1.1 KB, uniform for every wave -- a term's fields are scalar loads from the kernel arguments
struct WhereArgs {
  const int64_t *cols[WHERE_MAX_COLUMNS];
  WhereTerm terms[WHERE_MAX_TERMS];
  int32_t n_terms, n_cols, n_set, combine;
};

// v in set[0, n)?  n >= 1 and uniform, so every lane takes the same <= 12 steps: a lower bound without a branch on v
static __device__ __forceinline__ bool where_in_set(const int64_t *set, int32_t n, int64_t v) {
  int32_t base = 0;
  while (n > 1) {
    const int32_t half = n >> 1;
    base = set[base + half] <= v ? base + half : base;
    n -= half;
  }
  return set[base] == v;
}

// W2: words[w] = the rows of [64 w, 64 w + 64) below `rows` that the clauses keep, combined with with_words[w] if given.
// The sets (a.n_set values at d_set, sorted term by term) are staged in LDS once per workgroup: a.n_set * 8 bytes of
// dynamic shared memory, none for a call without IN terms
static __global__ void __launch_bounds__(WHERE_BLOCK) mask_where_kernel(const WhereArgs a, int64_t rows, int32_t n_words,
                                                                         const int64_t *__restrict__ d_set,
                                                                         const uint64_t *__restrict__ with_words,
                                                                         uint64_t *__restrict__ words) {
  extern __shared__ int64_t where_set[];
  if (a.n_set > 0) {
    for (int32_t i = (int32_t)threadIdx.x; i < a.n_set; i += WHERE_BLOCK) where_set[i] = d_set[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int32_t step = (int32_t)gridDim.x * (WHERE_BLOCK / 64);
  for (int32_t w = (int32_t)blockIdx.x * (WHERE_BLOCK / 64) + (int32_t)(threadIdx.x >> 6); w < n_words; w += step) {
    const int64_t r = (int64_t)w * 64 + lane;
    // every distinct column once, whatever number of terms names it; lanes past the rows read as NULL: kept by no term
    int64_t v[WHERE_MAX_COLUMNS];
#pragma unroll
    for (int c = 0; c < WHERE_MAX_COLUMNS; ++c) v[c] = (c < a.n_cols && r < rows) ? a.cols[c][r] : ATTR_NULL;
    uint64_t result = ~0ull, clause = 0;
    for (int32_t t = 0; t < a.n_terms; ++t) {
      const WhereTerm &tm = a.terms[t];
      int64_t x = v[0];  // (tm.col is uniform: a chain of selects, no indexed register array)
#pragma unroll
      for (int c = 1; c < WHERE_MAX_COLUMNS; ++c) x = tm.col == c ? v[c] : x;
      bool hit;
      if (tm.flags & WHERE_F_IN)
        hit = tm.set_n > 0 && where_in_set(where_set + tm.set_off, tm.set_n, x);
      else
        hit = tm.lo <= x && x <= tm.hi;
      clause |= __ballot(x != ATTR_NULL && hit != ((tm.flags & WHERE_F_NEGATE) != 0));
      if (tm.flags & WHERE_F_LAST) {
        result &= clause;
        clause = 0;
      }
    }
    if (with_words) {
      const uint64_t o = with_words[w];
      result = a.combine == MASK_COMBINE_OR ? (result | o) : (result & o);
    }
    if (lane == 0) words[w] = result;
  }
}

}  // namespace tsh
