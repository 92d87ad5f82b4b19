// The host side of a facet count (tostore_amd/csrc/tsh_facet_plan.h), alone: no HIP, no handles.  Built by
// tests/test_host_facet_plan.py with g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined and run; prints
// "facet plan ok" when every check holds.
#include "../../tostore_amd/csrc/tsh_facet_plan.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>

using namespace tsh;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

typedef std::vector<int64_t> V;
static const int64_t NUL = INT64_MIN;

static FacetKeys keys_of(int32_t kind, const V &k) {
  FacetKeys out;
  CHECK(facet_keys(kind, k.data(), (int64_t)k.size(), &out) == FACET_PLAN_OK);
  return out;
}

// the specification of a bucket, by a loop over the caller's keys: the index into the sorted distinct set, or -1 (other),
// or -2 (NULL)
static int brute_bucket(int32_t kind, const V &set, int64_t v) {
  if (v == NUL) return -2;
  if (kind == FACET_VALUES) {
    for (size_t j = 0; j < set.size(); ++j)
      if (set[j] == v) return (int)j;
    return -1;
  }
  int at = -1;
  for (size_t j = 0; j < set.size(); ++j) {
    const bool last = j + 1 == set.size();
    if (set[j] <= v && (last || v < set[j + 1])) at = (int)j;
  }
  return at;
}

static void test_normalisation() {
  // duplicates, NULL keys, any order
  const V k = {7, 3, NUL, 7, INT64_MAX, INT64_MIN + 1, 3, NUL};
  FacetKeys f = keys_of(FACET_VALUES, k);
  CHECK((f.set == V{INT64_MIN + 1, 3, 7, INT64_MAX}));
  CHECK((f.slot_of == std::vector<int32_t>{2, 1, FACET_NO_SLOT, 2, 3, 0, 1, FACET_NO_SLOT}));
  CHECK(f.counters() == 7 && f.n() == 4);
  // none, and only NULLs
  f = keys_of(FACET_VALUES, {});
  CHECK(f.set.empty() && f.slot_of.empty() && f.counters() == 3);
  CHECK(facet_keys(FACET_VALUES, nullptr, 0, &f) == FACET_PLAN_OK);
  f = keys_of(FACET_VALUES, {NUL, NUL});
  CHECK(f.set.empty() && f.slot_of.size() == 2 && f.slot_of[0] == FACET_NO_SLOT);
  // 4096 distinct keys with duplicates and a NULL pass, 4097 do not; the output is untouched by a refusal
  V big;
  for (int i = 0; i < FACET_MAX_KEYS; ++i) big.push_back(5000 - i);
  big.push_back(NUL);
  big.push_back(1000);
  big.push_back(4999);
  f = keys_of(FACET_VALUES, big);
  CHECK(f.n() == FACET_MAX_KEYS && f.slot_of.size() == big.size());
  big.push_back(5001);
  FacetKeys keep = keys_of(FACET_VALUES, {1, 2});
  CHECK(facet_keys(FACET_VALUES, big.data(), (int64_t)big.size(), &keep) == FACET_PLAN_MAX_KEYS);
  CHECK((keep.set == V{1, 2}));
  // arguments
  CHECK(facet_keys(2, big.data(), 1, &keep) == FACET_PLAN_KIND);
  CHECK(facet_keys(-1, big.data(), 1, &keep) == FACET_PLAN_KIND);
  CHECK(facet_keys(FACET_VALUES, big.data(), -1, &keep) == FACET_PLAN_KEYS);
  CHECK(facet_keys(FACET_VALUES, nullptr, 1, &keep) == FACET_PLAN_KEYS);
  CHECK(facet_keys(FACET_EDGES, nullptr, 3, &keep) == FACET_PLAN_KEYS);
  CHECK((keep.set == V{1, 2}));
  for (int e = FACET_PLAN_OK; e <= FACET_PLAN_EDGE_ORDER; ++e) CHECK(facet_plan_error(e)[0] != '?');
}

static void test_edges() {
  FacetKeys f = keys_of(FACET_EDGES, {INT64_MIN + 1, 0, 10, INT64_MAX});
  CHECK((f.set == V{INT64_MIN + 1, 0, 10, INT64_MAX}) && (f.slot_of == std::vector<int32_t>{0, 1, 2, 3}) && f.kind == FACET_EDGES);
  f = keys_of(FACET_EDGES, {5});
  CHECK(f.n() == 1);
  f = keys_of(FACET_EDGES, {});
  CHECK(f.n() == 0);
  FacetKeys keep = keys_of(FACET_EDGES, {1, 2});
  const V bad[] = {{1, 1}, {2, 1}, {0, 5, 5, 9}, {0, 5, 4}, {3, NUL}};
  for (const V &b : bad) CHECK(facet_keys(FACET_EDGES, b.data(), (int64_t)b.size(), &keep) == FACET_PLAN_EDGE_ORDER);
  const V nul = {NUL, 4};
  CHECK(facet_keys(FACET_EDGES, nul.data(), 2, &keep) == FACET_PLAN_EDGE_NULL);
  CHECK(facet_keys(FACET_EDGES, nul.data(), 1, &keep) == FACET_PLAN_EDGE_NULL);
  V many;
  for (int i = 0; i <= FACET_MAX_KEYS; ++i) many.push_back(i);
  CHECK(facet_keys(FACET_EDGES, many.data(), FACET_MAX_KEYS + 1, &keep) == FACET_PLAN_MAX_KEYS);
  CHECK(facet_keys(FACET_EDGES, many.data(), FACET_MAX_KEYS, &keep) == FACET_PLAN_OK && keep.n() == FACET_MAX_KEYS);
}

static void test_bucket_rule() {
  std::mt19937_64 rng(11);
  const int sizes[] = {0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 1000, 4095, 4096};
  for (int32_t kind : {FACET_VALUES, FACET_EDGES})
    for (int n : sizes) {
      std::set<int64_t> s;
      if (n >= 2) {
        s.insert(INT64_MIN + 1);
        s.insert(INT64_MAX);
      }
      while ((int)s.size() < n) s.insert((int64_t)(rng() % 20000) - 10000);
      const V set(s.begin(), s.end());
      V probe = {NUL, INT64_MIN + 1, INT64_MIN + 2, -1, 0, 1, INT64_MAX - 1, INT64_MAX};
      for (int64_t v : set) {
        probe.push_back(v);
        if (n <= 65) {
          if (v > INT64_MIN + 1) probe.push_back(v - 1);
          if (v < INT64_MAX) probe.push_back(v + 1);
        }
      }
      for (int i = 0; i < 300; ++i) probe.push_back((int64_t)(rng() % 22000) - 11000);
      for (int64_t v : probe) {
        const int want = brute_bucket(kind, set, v);
        const int32_t got = facet_bucket(kind, set.data(), n, v);
        CHECK(got == (want == -2 ? n + FACET_NULLS : want == -1 ? n + FACET_OTHER : want));
      }
    }
  // a value equal to an edge falls in the bucket that edge opens; below the first edge is `other`; the last is open
  const V e = {10, 20, INT64_MAX};
  CHECK(facet_bucket(FACET_EDGES, e.data(), 3, 9) == 3 + FACET_OTHER);
  CHECK(facet_bucket(FACET_EDGES, e.data(), 3, 10) == 0 && facet_bucket(FACET_EDGES, e.data(), 3, 19) == 0);
  CHECK(facet_bucket(FACET_EDGES, e.data(), 3, 20) == 1 && facet_bucket(FACET_EDGES, e.data(), 3, INT64_MAX - 1) == 1);
  CHECK(facet_bucket(FACET_EDGES, e.data(), 3, INT64_MAX) == 2);
  CHECK(facet_bucket(FACET_EDGES, e.data(), 1, INT64_MAX) == 0);  // (one edge)
}

static void test_attr_word() {
  const FacetKeys f = keys_of(FACET_VALUES, {5, 9});
  V vals(64);
  for (int l = 0; l < 64; ++l) vals[l] = l % 3 == 0 ? 5 : (l % 3 == 1 ? 9 : 100 + l);
  vals[7] = NUL;  // a NULL row (7 % 3 == 1: one 9 fewer)
  std::vector<uint64_t> cnt(f.counters(), 0);
  facet_attr_word(f, vals.data(), ~0ull, 64, cnt.data());
  CHECK(cnt[0] == 22 && cnt[1] == 20 && cnt[2 + FACET_OTHER] == 21 && cnt[2 + FACET_NULLS] == 1 && cnt[2 + FACET_TOTAL] == 64);
  // a tail word: 5 rows left, the bits past them set all the same; only 5 values exist (the sanitizer watches the rest)
  V tail(vals.begin(), vals.begin() + 5);
  cnt.assign(f.counters(), 0);
  facet_attr_word(f, tail.data(), ~0ull, 5, cnt.data());
  CHECK(cnt[0] == 2 && cnt[1] == 2 && cnt[2 + FACET_OTHER] == 1 && cnt[2 + FACET_TOTAL] == 5);
  // the active word: only its rows count, and it adds to what is there
  facet_attr_word(f, vals.data(), (1ull << 0) | (1ull << 7) | (1ull << 63), 64, cnt.data());
  CHECK(cnt[0] == 4 && cnt[2 + FACET_NULLS] == 1 && cnt[2 + FACET_TOTAL] == 8);
  // no keys: every non-NULL row is other
  const FacetKeys none = keys_of(FACET_VALUES, {});
  std::vector<uint64_t> c0(none.counters(), 0);
  facet_attr_word(none, vals.data(), ~0ull, 64, c0.data());
  CHECK(c0[FACET_OTHER] == 63 && c0[FACET_NULLS] == 1 && c0[FACET_TOTAL] == 64);
  // edges against the brute-force loop
  const FacetKeys e = keys_of(FACET_EDGES, {9, 100, 130});
  std::vector<uint64_t> ce(e.counters(), 0), want(e.counters(), 0);
  facet_attr_word(e, vals.data(), 0xF0F0F0F0F0F0F0F0ull, 64, ce.data());
  for (int l = 0; l < 64; ++l)
    if ((0xF0F0F0F0F0F0F0F0ull >> l) & 1) {
      const int b = brute_bucket(FACET_EDGES, e.set, vals[l]);
      ++want[b == -2 ? 3 + FACET_NULLS : b == -1 ? 3 + FACET_OTHER : b];
      ++want[3 + FACET_TOTAL];
    }
  CHECK(ce == want);
}

static void test_tags_word() {
  // rows: 0 {1,2}; 1 {} (empty set); 2 NULL; 3 a row of 70 values 0..69 (more than one pass of 64); 4 {2}; 5 beyond the column
  typedef std::vector<V> Lists;
  Lists lists = {{2, 1, 2}, {}, {4, NUL}, {}, {2}};
  for (int i = 0; i < 70; ++i) lists[3].push_back(69 - i);
  std::vector<int64_t> off{0}, flat;
  for (const V &r : lists) {
    flat.insert(flat.end(), r.begin(), r.end());
    off.push_back((int64_t)flat.size());
  }
  TagsColumn col;
  CHECK(tags_normalise(off.data(), 5, flat.data(), &col) == TAGS_PLAN_OK);
  TagsSlice sl;
  CHECK(tags_slice(col, 0, 6, &sl) == TAGS_PLAN_OK);
  CHECK(sl.valid.size() == 1 && sl.valid[0] == 0b011011ull && sl.n_vals == 73);
  const FacetKeys f = keys_of(FACET_VALUES, {2, 69, 1000, NUL, 2});
  std::vector<uint64_t> cnt(f.counters(), 0);
  facet_tags_word(f, sl.off.data(), sl.vals, sl.valid[0], ~0ull, 6, cnt.data());
  // key 2: rows 0, 3, 4; key 69: row 3; key 1000: none; other: row 1 (the empty set); NULL: rows 2 and 5
  CHECK(cnt[0] == 3 && cnt[1] == 1 && cnt[2] == 0);
  CHECK(cnt[3 + FACET_OTHER] == 1 && cnt[3 + FACET_NULLS] == 2 && cnt[3 + FACET_TOTAL] == 6);
  // rows taken out by the active word count nowhere
  cnt.assign(f.counters(), 0);
  facet_tags_word(f, sl.off.data(), sl.vals, sl.valid[0], 0b110110ull, 6, cnt.data());
  CHECK(cnt[0] == 1 && cnt[1] == 0 && cnt[3 + FACET_OTHER] == 1 && cnt[3 + FACET_NULLS] == 2 && cnt[3 + FACET_TOTAL] == 4);
  // no keys: every valid row is other
  const FacetKeys none = keys_of(FACET_VALUES, {});
  std::vector<uint64_t> c0(none.counters(), 0);
  facet_tags_word(none, sl.off.data(), sl.vals, sl.valid[0], ~0ull, 6, c0.data());
  CHECK(c0[FACET_OTHER] == 4 && c0[FACET_NULLS] == 2 && c0[FACET_TOTAL] == 6);
  // the caller's order
  int64_t out[5], rest[3];
  cnt.assign(f.counters(), 0);
  facet_tags_word(f, sl.off.data(), sl.vals, sl.valid[0], ~0ull, 6, cnt.data());
  facet_scatter(f, cnt.data(), out, rest);
  CHECK(out[0] == 3 && out[1] == 1 && out[2] == 0 && out[3] == 0 && out[4] == 3 && rest[0] == 1 && rest[1] == 2 && rest[2] == 6);

  // the quarantined rows of a shard with row_base 2: local rows 0 (NULL), 1 (the long row), 3 (beyond the column) and 2
  // (taken out by the mask)
  const uint32_t quar[] = {0, 1, 2, 3};
  const uint64_t mask_words[] = {0b1011ull};
  cnt.assign(f.counters(), 0);
  facet_quar_tags(f, quar, 4, mask_words, col, 2, cnt.data());
  CHECK(cnt[0] == 1 && cnt[1] == 1 && cnt[3 + FACET_OTHER] == 0 && cnt[3 + FACET_NULLS] == 2 && cnt[3 + FACET_TOTAL] == 3);
  cnt.assign(f.counters(), 0);
  facet_quar_tags(f, quar, 4, nullptr, col, 0, cnt.data());  // rows 0 .. 3, no mask
  CHECK(cnt[0] == 2 && cnt[1] == 1 && cnt[3 + FACET_OTHER] == 1 && cnt[3 + FACET_NULLS] == 1 && cnt[3 + FACET_TOTAL] == 4);
}

static void test_quarantine_and_scatter() {
  const V col = {5, 9, NUL, 5, 7, 9, 9};
  const FacetKeys f = keys_of(FACET_VALUES, {9, 5, 9, NUL, 6});
  std::vector<uint64_t> cnt(f.counters(), 0);
  const uint32_t quar[] = {0, 2, 3, 64, 70};
  std::vector<uint64_t> mask = {0b1101ull, 1ull << 6};  // keeps local rows 0, 2, 3 and 70
  // a shard at row_base 1: local 0 -> 9, 2 -> 5, 3 -> 7 (other), 64 masked out, 70 beyond the column -> NULL
  facet_quar_attr(f, quar, 5, mask.data(), col.data(), (int64_t)col.size(), 1, cnt.data());
  CHECK(cnt[0] == 1 && cnt[1] == 0 && cnt[2] == 1 && cnt[3 + FACET_OTHER] == 1 && cnt[3 + FACET_NULLS] == 1 && cnt[3 + FACET_TOTAL] == 4);
  // no mask, row_base 0: rows 0 (5), 2 (NULL), 3 (5), 64 and 70 (beyond: NULL)
  std::vector<uint64_t> c2(f.counters(), 0);
  facet_quar_attr(f, quar, 5, nullptr, col.data(), (int64_t)col.size(), 0, c2.data());
  CHECK(c2[0] == 2 && c2[3 + FACET_NULLS] == 3 && c2[3 + FACET_TOTAL] == 5);
  // edges
  const FacetKeys e = keys_of(FACET_EDGES, {6, 9});
  std::vector<uint64_t> ce(e.counters(), 0);
  facet_quar_attr(e, quar, 3, nullptr, col.data(), (int64_t)col.size(), 1, ce.data());  // 9, 5, 7
  CHECK(ce[0] == 1 && ce[1] == 1 && ce[2 + FACET_OTHER] == 1 && ce[2 + FACET_TOTAL] == 3);
  // the sum over shards and the scatter: repeated keys repeat their count, a NULL key counts nothing
  facet_add(cnt.data(), c2.data(), f.counters());
  int64_t out[5] = {-1, -1, -1, -1, -1}, rest[3];
  facet_scatter(f, cnt.data(), out, rest);
  CHECK(out[0] == 1 && out[1] == 3 && out[2] == 1 && out[3] == 0 && out[4] == 0);
  CHECK(rest[0] == 1 && rest[1] == 4 && rest[2] == 9);
  // (the counts of the DISTINCT keys + other + NULL = the total)
  CHECK((int64_t)(cnt[0] + cnt[1] + cnt[2]) + rest[0] + rest[1] == rest[2]);
  // no keys: out_counts is not touched (it may be NULL)
  const FacetKeys none = keys_of(FACET_VALUES, {});
  std::vector<uint64_t> c0 = {3, 1, 4};
  facet_scatter(none, c0.data(), nullptr, rest);
  CHECK(rest[0] == 3 && rest[1] == 1 && rest[2] == 4);
}

// many words against a map-based count: the word model is the per-row rule, word by word
static void test_words_against_brute_force() {
  std::mt19937_64 rng(5);
  const int64_t rows = 64 * 7 + 13;
  V vals((size_t)rows);
  for (auto &v : vals) v = rng() % 9 == 0 ? NUL : (int64_t)(rng() % 12);
  std::vector<uint64_t> act((size_t)((rows + 63) / 64));
  for (auto &w : act) w = rng();
  for (int32_t kind : {FACET_VALUES, FACET_EDGES}) {
    const FacetKeys f = keys_of(kind, kind == FACET_VALUES ? V{11, 3, 5, 3, 40} : V{2, 3, 8});
    std::vector<uint64_t> cnt(f.counters(), 0), want(f.counters(), 0);
    for (int64_t w = 0; w * 64 < rows; ++w) facet_attr_word(f, vals.data() + w * 64, act[(size_t)w], rows - w * 64, cnt.data());
    for (int64_t r = 0; r < rows; ++r)
      if ((act[(size_t)(r >> 6)] >> (r & 63)) & 1) {
        const int b = brute_bucket(kind, f.set, vals[(size_t)r]);
        ++want[b == -2 ? f.n() + FACET_NULLS : b == -1 ? f.n() + FACET_OTHER : b];
        ++want[f.n() + FACET_TOTAL];
      }
    CHECK(cnt == want);
  }
}

int main() {
  test_normalisation();
  test_edges();
  test_bucket_rule();
  test_attr_word();
  test_tags_word();
  test_quarantine_and_scatter();
  test_words_against_brute_force();
  std::printf("facet plan ok\n");
  return 0;
}
