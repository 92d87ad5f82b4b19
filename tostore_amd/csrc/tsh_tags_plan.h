// tsh_tags_plan.h -- the host side of a TAG column and of a HAS ANY / HAS ALL term over it (tsh_tags_create, tsh_tags_set,
// tsh_mask_create_tags, include/tostore_hip.h; the kernel is T1 mask_tags_kernel of tsh_tags.hip.h).  Plain C++17, no
// HIP, no handles, no devices: tests/cpp/tags_plan_test.cpp compiles it alone.
//
// A tag column is ragged: row i holds a SET of int64 values, given by the caller as CSR (offsets[n + 1], values).  Four
// things live here, and the library calls them for all of it:
//   tags_normalise / tags_splice   the caller's CSR made into the handle's own copy -- every row's list sorted and
//                                  deduplicated, a NULL flag per row (a list that holds TAGS_NULL anywhere; its values are
//                                  dropped) -- and tsh_tags_set's overwrite / extension of a row range of that copy
//   tags_slice                     what one shard's part uploads for its local rows [row_base, row_base + rows): rows + 1
//                                  offsets rebased to the slice's first value, as uint32_t; the span of values; and the
//                                  VALID words in the mask-word layout (bit r of word t: local row 64 t + r exists in the
//                                  column and is not NULL; 0 at or past `rows`).  Rows beyond the column are empty spans
//   tags_query                     the term's set sorted, deduplicated, NULL dropped, at most TAGS_MAX_SET_VALUES values
//                                  (what the kernel stages in LDS), and `need` resolved to the threshold t
//   tags_plan_keeps                the kernel's arithmetic, one row at a time: c = |row n S|, kept iff not NULL and
//                                  (c >= t) != negate
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace tsh {

constexpr int TAGS_MAX_SET_VALUES = 4096;     // TSH_TAGS_MAX_SET_VALUES: 32 KB of LDS
constexpr int32_t TAGS_NEED_ALL = 0;          // TSH_TAGS_ALL: every value of the set (any n >= 1: at least n of them)
constexpr int64_t TAGS_NULL = INT64_MIN;      // TSH_ATTR_NULL
constexpr int64_t TAGS_MAX_SLICE_VALUES = 0x7FFFFFFFll;  // a part's offsets are 32-bit

// the handle's copy of the column: rows() rows by GLOBAL row id; a NULL row has an empty list and null[i] = 1
struct TagsColumn {
  std::vector<int64_t> off{0};    // rows() + 1 entries, off[0] = 0, never decreasing
  std::vector<int64_t> vals;      // every row's list, ascending, without duplicates and without TAGS_NULL
  std::vector<uint8_t> null;      // rows() flags
  int64_t rows() const { return (int64_t)null.size(); }
};

// what a shard's part uploads (vals: a span of the column's own array, not copied)
struct TagsSlice {
  std::vector<uint32_t> off;      // rows + 1 entries, off[0] = 0
  std::vector<uint64_t> valid;    // (rows + 63) / 64 words
  const int64_t *vals = nullptr;  // off[rows] values (nullptr when there are none)
  int64_t n_vals = 0;
};

// the term, as the kernel takes it
struct TagsQuery {
  std::vector<int64_t> set;       // S: ascending, distinct, no TAGS_NULL
  int32_t t = 0;                  // the threshold: |S| for TAGS_NEED_ALL, else need
};

enum TagsPlanError {
  TAGS_PLAN_OK = 0,
  TAGS_PLAN_ROWS,          // n < 0 (or first_row_id < 0)
  TAGS_PLAN_OFFSETS,       // offsets is NULL with n > 0
  TAGS_PLAN_OFFSETS_START, // offsets[0] != 0
  TAGS_PLAN_OFFSETS_ORDER, // an offset smaller than the one before it
  TAGS_PLAN_VALUES,        // values is NULL with offsets[n] > 0
  TAGS_PLAN_NEED,          // need < 0
  TAGS_PLAN_SET,           // n_set < 0, or a NULL set with n_set > 0
  TAGS_PLAN_SET_VALUES,    // more than TAGS_MAX_SET_VALUES distinct non-NULL set values
  TAGS_PLAN_SLICE_VALUES,  // a shard's slice holds more than TAGS_MAX_SLICE_VALUES values
};

inline const char *tags_plan_error(int e) {
  switch (e) {
    case TAGS_PLAN_OK: return "ok";
    case TAGS_PLAN_ROWS: return "n < 0 / first_row_id < 0";
    case TAGS_PLAN_OFFSETS: return "offsets is NULL with n > 0";
    case TAGS_PLAN_OFFSETS_START: return "offsets[0] is not 0";
    case TAGS_PLAN_OFFSETS_ORDER: return "offsets must never decrease";
    case TAGS_PLAN_VALUES: return "values is NULL with offsets[n] > 0";
    case TAGS_PLAN_NEED: return "need < 0";
    case TAGS_PLAN_SET: return "n_set < 0, or set is NULL with n_set > 0";
    case TAGS_PLAN_SET_VALUES: return "more than TSH_TAGS_MAX_SET_VALUES distinct set values";
    case TAGS_PLAN_SLICE_VALUES: return "a shard's rows hold more than 2^31 - 1 tag values (the device offsets are 32-bit)";
  }
  return "?";
}

// Is the caller's CSR well-formed?  Reads offsets[0 .. n] and nothing of values
inline int tags_check_csr(const int64_t *offsets, int64_t n, const int64_t *values) {
  if (n < 0) return TAGS_PLAN_ROWS;
  if (n == 0) return TAGS_PLAN_OK;  // (neither array is read: offsets may be NULL)
  if (!offsets) return TAGS_PLAN_OFFSETS;
  if (offsets[0] != 0) return TAGS_PLAN_OFFSETS_START;
  for (int64_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i]) return TAGS_PLAN_OFFSETS_ORDER;
  if (offsets[n] > 0 && !values) return TAGS_PLAN_VALUES;
  return TAGS_PLAN_OK;
}

// The caller's CSR -> *out, every list sorted and deduplicated, NULL rows flagged and emptied.  *out is untouched unless
// TAGS_PLAN_OK comes back (may throw std::bad_alloc, *out untouched then too)
inline int tags_normalise(const int64_t *offsets, int64_t n, const int64_t *values, TagsColumn *out) {
  if (const int e = tags_check_csr(offsets, n, values)) return e;
  TagsColumn c;
  c.off.resize((size_t)n + 1);
  c.null.assign((size_t)n, 0);
  if (n > 0) c.vals.reserve((size_t)offsets[n]);
  std::vector<int64_t> row;
  for (int64_t i = 0; i < n; ++i) {
    row.assign(values + offsets[i], values + offsets[i + 1]);
    std::sort(row.begin(), row.end());
    if (!row.empty() && row.front() == TAGS_NULL) {  // (the smallest int64: wherever it stood, it is first now)
      c.null[(size_t)i] = 1;
    } else {
      row.erase(std::unique(row.begin(), row.end()), row.end());
      c.vals.insert(c.vals.end(), row.begin(), row.end());
    }
    c.off[(size_t)i + 1] = (int64_t)c.vals.size();
  }
  *out = std::move(c);
  return TAGS_PLAN_OK;
}

// tsh_tags_set: rows [first, first + n) of *col become the caller's lists (offsets relative to its own values, from 0);
// rows between the column's old end and `first` become NULL rows; everything else stays.  *col is untouched unless
// TAGS_PLAN_OK comes back
inline int tags_splice(TagsColumn *col, int64_t first, int64_t n, const int64_t *offsets, const int64_t *values) {
  if (first < 0) return TAGS_PLAN_ROWS;
  TagsColumn in;
  if (const int e = tags_normalise(offsets, n, values, &in)) return e;
  if (n == 0) return TAGS_PLAN_OK;
  const int64_t old_rows = col->rows(), new_rows = std::max(old_rows, first + n);
  const int64_t head = std::min(old_rows, first);  // rows [0, head) stay
  const int64_t tail = std::min(old_rows, first + n);  // rows [tail, old_rows) stay, behind the new ones
  TagsColumn c;
  c.off.reserve((size_t)new_rows + 1);
  c.null.reserve((size_t)new_rows);
  c.vals.reserve((size_t)(col->off[(size_t)head] + (int64_t)in.vals.size() + col->off[(size_t)old_rows] - col->off[(size_t)tail]));
  c.vals.assign(col->vals.begin(), col->vals.begin() + col->off[(size_t)head]);
  c.off.assign(col->off.begin(), col->off.begin() + head + 1);
  c.null.assign(col->null.begin(), col->null.begin() + head);
  for (int64_t i = head; i < first; ++i) {  // the gap
    c.null.push_back(1);
    c.off.push_back((int64_t)c.vals.size());
  }
  for (int64_t i = 0; i < n; ++i) {
    c.vals.insert(c.vals.end(), in.vals.begin() + in.off[(size_t)i], in.vals.begin() + in.off[(size_t)i + 1]);
    c.null.push_back(in.null[(size_t)i]);
    c.off.push_back((int64_t)c.vals.size());
  }
  for (int64_t i = tail; i < old_rows; ++i) {
    c.vals.insert(c.vals.end(), col->vals.begin() + col->off[(size_t)i], col->vals.begin() + col->off[(size_t)i + 1]);
    c.null.push_back(col->null[(size_t)i]);
    c.off.push_back((int64_t)c.vals.size());
  }
  *col = std::move(c);
  return TAGS_PLAN_OK;
}

// How many values local rows [row_base, row_base + rows) of the column hold (rows beyond it: none)
inline int64_t tags_slice_values(const TagsColumn &col, int64_t row_base, int64_t rows) {
  const int64_t n = col.rows();
  const int64_t lo = std::min(std::max<int64_t>(row_base, 0), n), hi = std::min(std::max<int64_t>(row_base + rows, 0), n);
  return hi > lo ? col.off[(size_t)hi] - col.off[(size_t)lo] : 0;
}

// Does a slice of n_vals values fit the part's 32-bit offsets?
inline bool tags_slice_fits(int64_t n_vals) { return n_vals >= 0 && n_vals <= TAGS_MAX_SLICE_VALUES; }

// What the part of a shard with local rows [row_base, row_base + rows) uploads.  TAGS_PLAN_SLICE_VALUES when its values
// do not fit 32-bit offsets (nothing is built then)
inline int tags_slice(const TagsColumn &col, int64_t row_base, int64_t rows, TagsSlice *out) {
  out->off.clear();
  out->valid.clear();
  out->vals = nullptr;
  out->n_vals = 0;
  if (row_base < 0 || rows < 0) return TAGS_PLAN_ROWS;
  const int64_t n_vals = tags_slice_values(col, row_base, rows);
  if (!tags_slice_fits(n_vals)) return TAGS_PLAN_SLICE_VALUES;
  const int64_t n = col.rows();
  const int64_t have = std::min(rows, std::max<int64_t>(n - row_base, 0));  // local rows the column names
  const int64_t first = have > 0 ? col.off[(size_t)row_base] : 0;
  out->off.assign((size_t)rows + 1, (uint32_t)n_vals);  // (rows beyond the column: empty spans at the end)
  out->valid.assign((size_t)((rows + 63) / 64), 0);
  for (int64_t r = 0; r < have; ++r) {
    out->off[(size_t)r] = (uint32_t)(col.off[(size_t)(row_base + r)] - first);
    if (!col.null[(size_t)(row_base + r)]) out->valid[(size_t)(r >> 6)] |= 1ull << (r & 63);
  }
  out->n_vals = n_vals;
  out->vals = n_vals > 0 ? col.vals.data() + first : nullptr;
  return TAGS_PLAN_OK;
}

// The term's set and threshold.  need: TAGS_NEED_ALL, or n >= 1 for "at least n distinct values of the set"
inline int tags_query(const int64_t *set, int64_t n_set, int32_t need, TagsQuery *out) {
  out->set.clear();
  out->t = 0;
  if (need < 0) return TAGS_PLAN_NEED;
  if (n_set < 0 || (n_set > 0 && !set)) return TAGS_PLAN_SET;
  std::vector<int64_t> v(set, set + n_set);
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  if (!v.empty() && v.front() == TAGS_NULL) v.erase(v.begin());
  if (v.size() > (size_t)TAGS_MAX_SET_VALUES) return TAGS_PLAN_SET_VALUES;
  out->t = need == TAGS_NEED_ALL ? (int32_t)v.size() : need;
  out->set = std::move(v);
  return TAGS_PLAN_OK;
}

// What the term keeps of a row whose normalised list is row[0, n_row) (is_null: the row's flag, or a row beyond the
// column): the kernel's arithmetic, one row at a time
inline bool tags_plan_keeps(const TagsQuery &q, const int64_t *row, int64_t n_row, bool is_null, bool negate) {
  uint32_t c = 0;
  for (int64_t j = 0; j < n_row; ++j) c += std::binary_search(q.set.begin(), q.set.end(), row[j]) ? 1u : 0u;
  return !is_null && ((c >= (uint32_t)q.t) != negate);
}

}  // namespace tsh
