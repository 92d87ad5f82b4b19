// tsh_facet_plan.h -- the host side of a FACET count (tsh_attr_facets, tsh_tags_facets, include/tostore_hip.h; the kernels
// are F1 attr_facets_kernel and F2 tags_facets_kernel of tsh_facet.hip.h).  Plain C++17, no HIP, no handles, no devices:
// tests/cpp/facet_plan_test.cpp compiles it alone.
//
// A facet call counts, over the rows a search under the same mask could return (the population P), how many fall into each
// of the caller's buckets.  What lives here, and the library calls it for all of it:
//   facet_keys          the caller's keys made into what the kernels stage in LDS: for FACET_VALUES the set S sorted,
//                       deduplicated and NULL-free with slot_of[j] = the place of keys[j] in S (or FACET_NO_SLOT); for
//                       FACET_EDGES the edges as they come, after the check that they ascend strictly and hold no NULL
//   facet_bucket        which counter a value adds to: a slot of S, `other` or `null`.  ONE function for both kinds, and
//                       the kernels include it: a branch-free lower bound over S (where_in_set's search), then == for
//                       VALUES and <= for EDGES
//   facet_attr_word /   one 64-row word of F1 / F2, row by row: the counters a wave adds for it, given the word of
//   facet_tags_word     live & mask bits
//   facet_quar_attr /   the host's share of the count: the quarantined rows, whose bits the device live bitmap has clear.
//   facet_quar_tags     Matched against the mask's words as quarantine_select does, read from the handle's own copy of the
//                       column by GLOBAL row id
//   facet_add /         the sum over shards, and the counters scattered back to the caller's order: a repeated key repeats
//   facet_scatter       its count, a NULL key counts nothing
// Counters: n = |S| of them, then FACET_OTHER, FACET_NULLS and FACET_TOTAL behind them: n + 3 in all.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "tsh_tags_plan.h"

#if defined(__HIPCC__)
#define TSH_FACET_HD __host__ __device__ __forceinline__
#else
#define TSH_FACET_HD inline
#endif

namespace tsh {

constexpr int32_t FACET_VALUES = 0;        // TSH_FACET_VALUES
constexpr int32_t FACET_EDGES = 1;         // TSH_FACET_EDGES
constexpr int FACET_MAX_KEYS = 4096;       // TSH_FACET_MAX_KEYS: 32 KB of keys + 16 KB of counters in LDS
constexpr int64_t FACET_NULL = INT64_MIN;  // TSH_ATTR_NULL
constexpr int32_t FACET_NO_SLOT = -1;      // slot_of: the key counts nothing (a NULL among the keys)
constexpr int FACET_OTHER = 0, FACET_NULLS = 1, FACET_TOTAL = 2;  // counters n + 0 .. n + 2; out_rest[0 .. 2]
constexpr int FACET_REST = 3;

struct FacetKeys {
  int32_t kind = FACET_VALUES;
  std::vector<int64_t> set;      // S ascending, distinct, no FACET_NULL (EDGES: the caller's edges)
  std::vector<int32_t> slot_of;  // n_keys entries: the caller's j -> S, or FACET_NO_SLOT
  int32_t n() const { return (int32_t)set.size(); }
  size_t counters() const { return set.size() + FACET_REST; }
};

enum FacetPlanError {
  FACET_PLAN_OK = 0,
  FACET_PLAN_KIND,        // kind is neither FACET_VALUES nor FACET_EDGES
  FACET_PLAN_KEYS,        // n_keys < 0, or NULL keys with n_keys > 0
  FACET_PLAN_MAX_KEYS,    // more than FACET_MAX_KEYS distinct non-NULL keys
  FACET_PLAN_EDGE_NULL,   // EDGES: keys[0] is FACET_NULL
  FACET_PLAN_EDGE_ORDER,  // EDGES: keys[j + 1] <= keys[j]
};

inline const char *facet_plan_error(int e) {
  switch (e) {
    case FACET_PLAN_OK: return "ok";
    case FACET_PLAN_KIND: return "kind is neither TSH_FACET_VALUES nor TSH_FACET_EDGES";
    case FACET_PLAN_KEYS: return "n_keys < 0, or keys is NULL with n_keys > 0";
    case FACET_PLAN_MAX_KEYS: return "more than TSH_FACET_MAX_KEYS distinct keys";
    case FACET_PLAN_EDGE_NULL: return "edges: keys[0] is TSH_ATTR_NULL";
    case FACET_PLAN_EDGE_ORDER: return "edges must ascend strictly";
  }
  return "?";
}

// The caller's keys -> *out.  *out is untouched unless FACET_PLAN_OK comes back (may throw std::bad_alloc)
inline int facet_keys(int32_t kind, const int64_t *keys, int64_t n_keys, FacetKeys *out) {
  if (kind != FACET_VALUES && kind != FACET_EDGES) return FACET_PLAN_KIND;
  if (n_keys < 0 || (n_keys > 0 && !keys)) return FACET_PLAN_KEYS;
  FacetKeys k;
  k.kind = kind;
  if (kind == FACET_EDGES) {
    if (n_keys > 0 && keys[0] == FACET_NULL) return FACET_PLAN_EDGE_NULL;
    for (int64_t j = 0; j + 1 < n_keys; ++j)  // (read before the limit is judged: it stops at the first fault)
      if (keys[j + 1] <= keys[j]) return FACET_PLAN_EDGE_ORDER;
    if (n_keys > FACET_MAX_KEYS) return FACET_PLAN_MAX_KEYS;
    k.set.assign(keys, keys + n_keys);
    k.slot_of.resize((size_t)n_keys);
    for (int64_t j = 0; j < n_keys; ++j) k.slot_of[(size_t)j] = (int32_t)j;
  } else {
    k.set.assign(keys, keys + n_keys);
    std::sort(k.set.begin(), k.set.end());
    k.set.erase(std::unique(k.set.begin(), k.set.end()), k.set.end());
    if (!k.set.empty() && k.set.front() == FACET_NULL) k.set.erase(k.set.begin());
    if (k.set.size() > (size_t)FACET_MAX_KEYS) return FACET_PLAN_MAX_KEYS;
    k.slot_of.resize((size_t)n_keys);
    for (int64_t j = 0; j < n_keys; ++j)
      k.slot_of[(size_t)j] = keys[j] == FACET_NULL
                                 ? FACET_NO_SLOT
                                 : (int32_t)(std::lower_bound(k.set.begin(), k.set.end(), keys[j]) - k.set.begin());
  }
  *out = std::move(k);
  return FACET_PLAN_OK;
}

// The counter of a value v over set[0, n), n uniform: a slot in [0, n), n + FACET_OTHER or n + FACET_NULLS.  The lower
// bound takes the same <= 12 steps in every lane and has no branch on v; `base` ends as the last entry <= v, or 0.
//   VALUES  the slot whose key == v              EDGES  the last edge <= v: keys[j] <= v < keys[j + 1], the last bucket open
TSH_FACET_HD int32_t facet_bucket(int32_t kind, const int64_t *set, int32_t n, int64_t v) {
  if (v == FACET_NULL) return n + FACET_NULLS;
  if (n <= 0) return n + FACET_OTHER;
  int32_t base = 0, m = n;
  while (m > 1) {
    const int32_t half = m >> 1;
    base = set[base + half] <= v ? base + half : base;
    m -= half;
  }
  const bool hit = kind == FACET_EDGES ? set[base] <= v : set[base] == v;
  return hit ? base : n + FACET_OTHER;
}

// F1, one word: vals = the word's first value, act = live & mask for the word, have = rows left from the word's first row
// (lanes at or past it count nothing, whatever act says).  cnt: n + FACET_REST counters, added to
inline void facet_attr_word(const FacetKeys &k, const int64_t *vals, uint64_t act, int64_t have, uint64_t *cnt) {
  const int32_t n = k.n();
  for (int l = 0; l < 64 && l < have; ++l) {
    if (!((act >> l) & 1ull)) continue;
    ++cnt[facet_bucket(k.kind, k.set.data(), n, vals[l])];
    ++cnt[n + FACET_TOTAL];
  }
}

// F2, one word: off = the word's up to 65 offsets into vals (off[l] .. off[l + 1]: the normalised list of lane l's row),
// valid = the column's word (bit l: the row exists in the column and is not NULL), act and have as above.  A row's keys
// count once each (a row is a set); a valid row that holds none is `other`, the empty set included
inline void facet_tags_word(const FacetKeys &k, const uint32_t *off, const int64_t *vals, uint64_t valid, uint64_t act, int64_t have,
                            uint64_t *cnt) {
  const int32_t n = k.n();
  for (int l = 0; l < 64 && l < have; ++l) {
    if (!((act >> l) & 1ull)) continue;
    ++cnt[n + FACET_TOTAL];
    if (!((valid >> l) & 1ull)) {
      ++cnt[n + FACET_NULLS];
      continue;
    }
    uint32_t c = 0;
    for (uint32_t e = off[l]; e < off[l + 1]; ++e) {
      const int32_t b = facet_bucket(FACET_VALUES, k.set.data(), n, vals[e]);
      if (b < n) {
        ++cnt[b];
        ++c;
      }
    }
    if (c == 0) ++cnt[n + FACET_OTHER];
  }
}

// Is local row r kept by the shard's slice of the mask (bit r of the words; NULL: no mask)?
inline bool facet_mask_keeps(const uint64_t *mask_words, uint32_t r) {
  return !mask_words || ((mask_words[r >> 6] >> (r & 63)) & 1ull);
}

// The quarantined rows of one shard (local ids quar[0, n_quar), none tombstoned: a delete takes a row off the list), read
// from the handle's copy of the column by GLOBAL id row_base + r; rows beyond the column are NULL
inline void facet_quar_attr(const FacetKeys &k, const uint32_t *quar, size_t n_quar, const uint64_t *mask_words, const int64_t *col,
                            int64_t col_rows, int64_t row_base, uint64_t *cnt) {
  const int32_t n = k.n();
  for (size_t i = 0; i < n_quar; ++i) {
    if (!facet_mask_keeps(mask_words, quar[i])) continue;
    const int64_t g = row_base + (int64_t)quar[i];
    ++cnt[facet_bucket(k.kind, k.set.data(), n, g < col_rows ? col[g] : FACET_NULL)];
    ++cnt[n + FACET_TOTAL];
  }
}

inline void facet_quar_tags(const FacetKeys &k, const uint32_t *quar, size_t n_quar, const uint64_t *mask_words, const TagsColumn &col,
                            int64_t row_base, uint64_t *cnt) {
  const int32_t n = k.n();
  for (size_t i = 0; i < n_quar; ++i) {
    if (!facet_mask_keeps(mask_words, quar[i])) continue;
    const int64_t g = row_base + (int64_t)quar[i];
    ++cnt[n + FACET_TOTAL];
    if (g >= col.rows() || col.null[(size_t)g]) {
      ++cnt[n + FACET_NULLS];
      continue;
    }
    uint32_t c = 0;
    for (int64_t e = col.off[(size_t)g]; e < col.off[(size_t)g + 1]; ++e) {
      const int32_t b = facet_bucket(FACET_VALUES, k.set.data(), n, col.vals[(size_t)e]);
      if (b < n) {
        ++cnt[b];
        ++c;
      }
    }
    if (c == 0) ++cnt[n + FACET_OTHER];
  }
}

// acc += part, n_cnt counters each: one shard's answer into the call's
inline void facet_add(uint64_t *acc, const uint64_t *part, size_t n_cnt) {
  for (size_t i = 0; i < n_cnt; ++i) acc[i] += part[i];
}

// The call's counters in the caller's order: out_counts[j] for every key as given (not written when there are none),
// out_rest[0 .. 2] = other, NULL rows, |P|
inline void facet_scatter(const FacetKeys &k, const uint64_t *cnt, int64_t *out_counts, int64_t *out_rest) {
  for (size_t j = 0; j < k.slot_of.size(); ++j)
    out_counts[j] = k.slot_of[j] == FACET_NO_SLOT ? 0 : (int64_t)cnt[(size_t)k.slot_of[j]];
  for (int i = 0; i < FACET_REST; ++i) out_rest[i] = (int64_t)cnt[k.set.size() + (size_t)i];
}

}  // namespace tsh
