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
// Lanes at or past `rows` ballot 0, so the tail word needs no trimming (and under OR the other handle's own tail is 0
// already: every handle's words hold that).  The words come back to the host in one copy -- the batched path and the
// quarantined-row match read them there -- and a selective mask's list is M1 + M2 of tsh_mask.hip.h, unchanged.
// No reference counterpart: the reference filters on the host and maps primary keys to node ids
// (lib/src/core/vector_index_manager.dart:1223-1378) before its vector search, which itself takes no filter.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

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

}  // namespace tsh
