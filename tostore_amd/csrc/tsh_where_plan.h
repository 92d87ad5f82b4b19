// tsh_where_plan.h -- the host plan of a WHERE clause made into mask words in one launch (tsh_mask_create_where,
// include/tostore_hip.h; the kernel is W2 mask_where_kernel of tsh_where.hip.h).  Plain C++17, no HIP, no handles, no
// devices: tests/cpp/where_plan_test.cpp compiles it alone.
//
// where_plan() takes the caller's terms as they come -- an opaque column key each (the library passes the attribute
// handle's address), the bounds of a range term or the values of an IN term, negate, and the clause number -- and makes
// what the kernel takes in its arguments:
//   columns[]  the distinct column keys in order of first appearance, at most WHERE_MAX_COLUMNS; every term carries the
//              index of its own, so the kernel loads a column once per row however many terms name it
//   set[]      every IN term's values, sorted ascending, duplicates and the NULL dropped, one term after the other in one
//              array of at most WHERE_MAX_SET_VALUES values (what the kernel stages in LDS); a term holds offset + count
//   terms[]    one 32-byte record per term: lo, hi, column, flags (IN / negate / last term of its clause), set offset,
//              set count
// Terms of equal clause number are OR-ed, the clauses AND-ed; the numbers start at 0 and never decrease or skip.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace tsh {

constexpr int WHERE_MAX_TERMS = 32;          // TSH_WHERE_MAX_TERMS
constexpr int WHERE_MAX_COLUMNS = 8;         // TSH_WHERE_MAX_COLUMNS
constexpr int WHERE_MAX_SET_VALUES = 4096;   // TSH_WHERE_MAX_SET_VALUES: 32 KB of LDS
constexpr int WHERE_KIND_RANGE = 0, WHERE_KIND_IN = 1;  // TSH_TERM_RANGE / TSH_TERM_IN
constexpr int64_t WHERE_NULL = INT64_MIN;    // TSH_ATTR_NULL

constexpr int32_t WHERE_F_IN = 1;      // the term is a set term: hit = v in set[set_off, set_off + set_n)
constexpr int32_t WHERE_F_NEGATE = 2;  // keep = v != NULL && !hit
constexpr int32_t WHERE_F_LAST = 4;    // the last term of its clause: the clause word is and-ed into the result here

// a term as the caller wrote it (tsh_where_term without the handle type)
struct WhereTermIn {
  const void *column = nullptr;
  int64_t lo = 0, hi = 0;
  const int64_t *set = nullptr;
  int64_t n_set = 0;
  int32_t kind = WHERE_KIND_RANGE, negate = 0, clause = 0;
};

// a term as the kernel reads it (uniform per wave: scalar loads from the kernel arguments)
struct WhereTerm {
  int64_t lo, hi;
  int32_t col, flags;
  int32_t set_off, set_n;
};
static_assert(sizeof(WhereTerm) == 32, "the kernel's term record is 32 bytes");

struct WherePlan {
  WhereTerm terms[WHERE_MAX_TERMS];
  const void *columns[WHERE_MAX_COLUMNS];
  int32_t n_terms = 0, n_cols = 0;
  std::vector<int64_t> set;  // all IN terms' values, staged by the kernel as they lie here
};

enum WherePlanError {
  WHERE_PLAN_OK = 0,
  WHERE_PLAN_N_TERMS,     // n_terms < 1 or > WHERE_MAX_TERMS, or no terms
  WHERE_PLAN_KIND,        // a kind that is neither constant
  WHERE_PLAN_SET,         // n_set < 0, or a NULL set with n_set > 0
  WHERE_PLAN_COLUMN,      // a NULL column key
  WHERE_PLAN_CLAUSE,      // clause numbers that do not start at 0, decrease or skip
  WHERE_PLAN_COLUMNS,     // more than WHERE_MAX_COLUMNS distinct columns
  WHERE_PLAN_SET_VALUES,  // more than WHERE_MAX_SET_VALUES set values after sort + dedupe
};

inline const char *where_plan_error(int e) {
  switch (e) {
    case WHERE_PLAN_OK: return "ok";
    case WHERE_PLAN_N_TERMS: return "terms is NULL / n_terms is not in 1 .. TSH_WHERE_MAX_TERMS";
    case WHERE_PLAN_KIND: return "a term's kind is neither TSH_TERM_RANGE nor TSH_TERM_IN";
    case WHERE_PLAN_SET: return "a term's n_set < 0, or its set is NULL with n_set > 0";
    case WHERE_PLAN_COLUMN: return "a term's attr is NULL";
    case WHERE_PLAN_CLAUSE: return "clause numbers must start at 0 and go up without a gap";
    case WHERE_PLAN_COLUMNS: return "more than TSH_WHERE_MAX_COLUMNS distinct attribute handles";
    case WHERE_PLAN_SET_VALUES: return "more than TSH_WHERE_MAX_SET_VALUES distinct set values";
  }
  return "?";
}

// WHERE_PLAN_OK and *out filled, or the first thing that is wrong (checked term by term in the order of the enum's
// first five, then the two totals); nothing a column key points to is read
inline int where_plan(const WhereTermIn *in, int32_t n_terms, WherePlan *out) {
  out->n_terms = out->n_cols = 0;
  out->set.clear();
  if (!in || n_terms < 1 || n_terms > WHERE_MAX_TERMS) return WHERE_PLAN_N_TERMS;
  for (int32_t t = 0; t < n_terms; ++t) {
    const WhereTermIn &a = in[t];
    if (a.kind != WHERE_KIND_RANGE && a.kind != WHERE_KIND_IN) return WHERE_PLAN_KIND;
    if (a.n_set < 0 || (a.n_set > 0 && !a.set)) return WHERE_PLAN_SET;  // (of a range term too, though it reads neither)
    if (!a.column) return WHERE_PLAN_COLUMN;
    const int32_t prev = t == 0 ? 0 : in[t - 1].clause;
    if (a.clause != prev && (t == 0 || a.clause != prev + 1)) return WHERE_PLAN_CLAUSE;
  }
  for (int32_t t = 0; t < n_terms; ++t) {
    const WhereTermIn &a = in[t];
    WhereTerm &w = out->terms[t];
    int32_t c = 0;
    while (c < out->n_cols && out->columns[c] != a.column) ++c;
    if (c == out->n_cols) {
      if (c == WHERE_MAX_COLUMNS) return WHERE_PLAN_COLUMNS;
      out->columns[out->n_cols++] = a.column;
    }
    w.col = c;
    w.flags = (a.kind == WHERE_KIND_IN ? WHERE_F_IN : 0) | (a.negate ? WHERE_F_NEGATE : 0) |
              (t + 1 == n_terms || in[t + 1].clause != a.clause ? WHERE_F_LAST : 0);
    w.lo = w.hi = 0;
    w.set_off = w.set_n = 0;
    if (a.kind == WHERE_KIND_RANGE) {
      w.lo = a.lo;
      w.hi = a.hi;
      continue;
    }
    std::vector<int64_t> v(a.set, a.set + a.n_set);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    if (!v.empty() && v.front() == WHERE_NULL) v.erase(v.begin());
    if (out->set.size() + v.size() > (size_t)WHERE_MAX_SET_VALUES) return WHERE_PLAN_SET_VALUES;
    w.set_off = (int32_t)out->set.size();
    w.set_n = (int32_t)v.size();
    out->set.insert(out->set.end(), v.begin(), v.end());
  }
  out->n_terms = n_terms;
  return WHERE_PLAN_OK;
}

// What the plan keeps of rows whose values in the plan's columns are v[0 .. n_cols): the kernel's arithmetic, one row
// at a time (the stand-alone test holds the plan to it; the kernel does the same with a wave's ballots)
inline bool where_plan_keeps(const WherePlan &p, const int64_t *v) {
  bool result = true, clause = false;
  for (int32_t t = 0; t < p.n_terms; ++t) {
    const WhereTerm &w = p.terms[t];
    const int64_t x = v[w.col];
    bool hit;
    if (w.flags & WHERE_F_IN)
      hit = std::binary_search(p.set.begin() + w.set_off, p.set.begin() + w.set_off + w.set_n, x);
    else
      hit = w.lo <= x && x <= w.hi;
    clause = clause || (x != WHERE_NULL && hit != ((w.flags & WHERE_F_NEGATE) != 0));
    if (w.flags & WHERE_F_LAST) {
      result = result && clause;
      clause = false;
    }
  }
  return result;
}

}  // namespace tsh
