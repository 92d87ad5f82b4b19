// The host side of a tag column and its HAS ANY / HAS ALL term (tostore_amd/csrc/tsh_tags_plan.h), alone: no HIP, no
// handles.  Built by tests/test_host_tags_plan.py with g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined and run;
// prints "tags plan ok" when every check holds.
#include "../../tostore_amd/csrc/tsh_tags_plan.h"

#include <cstdio>
#include <cstdlib>
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

typedef std::vector<std::vector<int64_t>> Lists;
static const int64_t NUL = INT64_MIN;

// a caller's CSR of some lists, as they come
struct Csr {
  std::vector<int64_t> off{0}, vals;
  explicit Csr(const Lists &l) {
    for (const auto &r : l) {
      vals.insert(vals.end(), r.begin(), r.end());
      off.push_back((int64_t)vals.size());
    }
  }
  int64_t n() const { return (int64_t)off.size() - 1; }
};

// the specification of a normalised row: (is NULL, its sorted distinct values)
static std::pair<bool, std::vector<int64_t>> norm_row(const std::vector<int64_t> &r) {
  std::set<int64_t> s(r.begin(), r.end());
  if (s.count(NUL)) return {true, {}};
  return {false, std::vector<int64_t>(s.begin(), s.end())};
}

static void check_column(const TagsColumn &c, const Lists &want) {
  CHECK(c.rows() == (int64_t)want.size());
  CHECK(c.off.size() == want.size() + 1 && c.off[0] == 0);
  for (size_t i = 0; i < want.size(); ++i) {
    const auto w = norm_row(want[i]);
    CHECK((c.null[i] != 0) == w.first);
    CHECK(c.off[i + 1] >= c.off[i]);
    CHECK(std::vector<int64_t>(c.vals.begin() + c.off[i], c.vals.begin() + c.off[i + 1]) == w.second);
  }
  CHECK(c.off.back() == (int64_t)c.vals.size());
}

static TagsColumn make(const Lists &l) {
  Csr in(l);
  TagsColumn c;
  CHECK(tags_normalise(in.off.data(), in.n(), in.vals.data(), &c) == TAGS_PLAN_OK);
  return c;
}

// a NULL list: {NUL} in the specification's terms
static const std::vector<int64_t> NULL_ROW{NUL};

static void check_slice(const TagsColumn &c, const Lists &lists, int64_t row_base, int64_t rows) {
  TagsSlice s;
  CHECK(tags_slice(c, row_base, rows, &s) == TAGS_PLAN_OK);
  CHECK((int64_t)s.off.size() == rows + 1 && s.off[0] == 0);
  CHECK((int64_t)s.valid.size() == (rows + 63) / 64);
  CHECK((int64_t)s.off[(size_t)rows] == s.n_vals);
  CHECK(s.n_vals == tags_slice_values(c, row_base, rows));
  CHECK((s.vals == nullptr) == (s.n_vals == 0));
  for (int64_t r = 0; r < rows; ++r) {
    const int64_t g = row_base + r;
    const bool beyond = g >= (int64_t)lists.size();
    const auto w = beyond ? std::make_pair(true, std::vector<int64_t>()) : norm_row(lists[(size_t)g]);
    CHECK(s.off[(size_t)r + 1] >= s.off[(size_t)r]);
    const std::vector<int64_t> got(s.vals ? s.vals + s.off[(size_t)r] : nullptr, s.vals ? s.vals + s.off[(size_t)r + 1] : nullptr);
    if (s.vals) CHECK(got == w.second);
    else CHECK(w.second.empty() && s.off[(size_t)r + 1] == s.off[(size_t)r]);
    CHECK(((s.valid[(size_t)(r >> 6)] >> (r & 63)) & 1) == (w.first ? 0u : 1u));
  }
  for (int64_t b = rows; b < (int64_t)s.valid.size() * 64; ++b)  // no bit at or past `rows`
    CHECK(((s.valid[(size_t)(b >> 6)] >> (b & 63)) & 1) == 0);
}

int main() {
  // ---- normalisation: unsorted lists, duplicates, NULL first / last / alone, empty lists, extremes
  {
    const Lists l{{5, 3, 9, 3, 5}, {}, {NUL, 4, 2}, {4, 2, NUL}, {NUL}, {7, 7, 7, 7, 7}, {INT64_MAX, INT64_MIN + 1, 0}, {}, {1}};
    const TagsColumn c = make(l);
    check_column(c, l);
    CHECK(c.null[1] == 0 && c.off[2] == c.off[1]);  // the empty set is a value, not NULL
    CHECK(c.null[2] && c.null[3] && c.null[4] && c.off[5] == c.off[2]);  // NULL rows keep no values
    CHECK(c.off[6] - c.off[5] == 1);  // five times the same value: once
    CHECK(c.vals[(size_t)c.off[6]] == INT64_MIN + 1 && c.vals[(size_t)c.off[7] - 1] == INT64_MAX);
  }
  // n = 0: neither array is read
  {
    TagsColumn c;
    CHECK(tags_normalise(nullptr, 0, nullptr, &c) == TAGS_PLAN_OK);
    CHECK(c.rows() == 0 && c.off.size() == 1 && c.off[0] == 0 && c.vals.empty());
    const int64_t off0[1] = {0};
    CHECK(tags_normalise(off0, 0, nullptr, &c) == TAGS_PLAN_OK && c.rows() == 0);
  }
  // rows that are all empty need no values array
  {
    const int64_t off[4] = {0, 0, 0, 0};
    TagsColumn c;
    CHECK(tags_normalise(off, 3, nullptr, &c) == TAGS_PLAN_OK);
    CHECK(c.rows() == 3 && c.vals.empty() && !c.null[0] && !c.null[2]);
  }
  // ---- every offsets error; the column given is left as it was
  {
    TagsColumn c = make({{1, 2}, {3}});
    const TagsColumn before = c;
    const int64_t v[4] = {1, 2, 3, 4};
    const int64_t ok[3] = {0, 2, 4}, start[3] = {1, 2, 4}, down[3] = {0, 3, 2}, neg[3] = {0, -1, 4};
    CHECK(tags_normalise(ok, -1, v, &c) == TAGS_PLAN_ROWS);
    CHECK(tags_normalise(nullptr, 2, v, &c) == TAGS_PLAN_OFFSETS);
    CHECK(tags_normalise(start, 2, v, &c) == TAGS_PLAN_OFFSETS_START);
    CHECK(tags_normalise(down, 2, v, &c) == TAGS_PLAN_OFFSETS_ORDER);
    CHECK(tags_normalise(neg, 2, v, &c) == TAGS_PLAN_OFFSETS_ORDER);
    CHECK(tags_normalise(ok, 2, nullptr, &c) == TAGS_PLAN_VALUES);
    CHECK(tags_check_csr(ok, 2, v) == TAGS_PLAN_OK);
    CHECK(tags_splice(&c, -1, 2, ok, v) == TAGS_PLAN_ROWS);
    CHECK(tags_splice(&c, 0, -1, ok, v) == TAGS_PLAN_ROWS);
    CHECK(tags_splice(&c, 0, 2, nullptr, v) == TAGS_PLAN_OFFSETS);
    CHECK(tags_splice(&c, 0, 2, start, v) == TAGS_PLAN_OFFSETS_START);
    CHECK(tags_splice(&c, 0, 2, down, v) == TAGS_PLAN_OFFSETS_ORDER);
    CHECK(tags_splice(&c, 0, 2, ok, nullptr) == TAGS_PLAN_VALUES);
    CHECK(c.off == before.off && c.vals == before.vals && c.null == before.null);
    for (int e = 0; e <= TAGS_PLAN_SLICE_VALUES; ++e) CHECK(tags_plan_error(e)[0] != '?');
  }
  // ---- the tsh_tags_set splice
  {
    Lists l{{1, 2, 3}, {4}, {}, {5, 6}, {NUL}, {7}};
    TagsColumn c = make(l);
    auto set = [&](int64_t first, const Lists &in) {
      Csr s(in);
      CHECK(tags_splice(&c, first, s.n(), s.off.data(), s.vals.data()) == TAGS_PLAN_OK);
      if ((int64_t)l.size() < first) l.resize((size_t)first, NULL_ROW);  // the gap's rows become NULL rows
      for (size_t i = 0; i < in.size(); ++i) {
        if (first + i < l.size()) l[first + i] = in[i];
        else l.push_back(in[i]);
      }
      check_column(c, l);
    };
    set(1, {{9, 8}, {7}});                         // overwrite inside, same row count, other lengths
    set(0, {{}});                                  // a list shrinks to the empty set
    set(3, {{3, 1, 2, 1, 40, 50, 60, 70}});        // ... and one grows: the rows behind move
    set(4, {{11}, {NUL, 12}, {13, 13}});           // overwrite the end and extend by one
    set(7, {{14}});                                // extend exactly at the end: no gap
    set(12, {{15, 16}, {}});                       // extend over a gap: rows 8 .. 11 are NULL rows
    CHECK(c.rows() == 14 && c.null[8] && c.null[11] && !c.null[12] && !c.null[13]);
    set(2, {});                                    // n = 0 changes nothing
    CHECK(tags_splice(&c, 100, 0, nullptr, nullptr) == TAGS_PLAN_OK && c.rows() == 14);
    set(0, {{NUL}});                               // a row made NULL loses its values
    TagsColumn e;                                  // into an empty column, with a gap in front
    Csr s({{2, 1}});
    CHECK(tags_splice(&e, 3, 1, s.off.data(), s.vals.data()) == TAGS_PLAN_OK);
    check_column(e, {NULL_ROW, NULL_ROW, NULL_ROW, {1, 2}});
  }
  // ---- slices: row_base x rows against columns shorter than, equal to, longer than, and ending inside the slice
  {
    std::mt19937_64 rng(7);
    const int64_t bases[] = {0, 5, 64, 67}, counts[] = {0, 1, 63, 64, 65, 130};
    for (int64_t row_base : bases)
      for (int64_t rows : counts) {
        const int64_t lens[] = {0, row_base / 2, row_base, row_base + rows / 2, row_base + rows - 1, row_base + rows,
                                row_base + rows + 1, row_base + rows + 77};
        for (int64_t n : lens) {
          if (n < 0) continue;
          Lists l((size_t)n);
          for (auto &r : l) {
            const int kind = (int)(rng() % 8);
            if (kind == 0) r = NULL_ROW;
            else if (kind > 1) for (int j = (int)(rng() % 6); j > 0; --j) r.push_back((int64_t)(rng() % 20));
          }
          const TagsColumn c = make(l);
          check_slice(c, l, row_base, rows);
        }
      }
    // a slice that starts mid-array has its offsets rebased to its own first value
    const Lists l{{1, 2, 3}, {4, 5}, {6}, {}, {7, 8}};
    const TagsColumn c = make(l);
    TagsSlice s;
    CHECK(tags_slice(c, 1, 3, &s) == TAGS_PLAN_OK);
    CHECK((s.off == std::vector<uint32_t>{0, 2, 3, 3}) && s.vals == c.vals.data() + 3 && s.n_vals == 3 && s.valid[0] == 7);
    CHECK(tags_slice(c, 4, 3, &s) == TAGS_PLAN_OK);  // the column ends inside: rows 5, 6 are empty spans, bits 0
    CHECK((s.off == std::vector<uint32_t>{0, 2, 2, 2}) && s.valid[0] == 1);
    CHECK(tags_slice(c, 9, 2, &s) == TAGS_PLAN_OK && s.n_vals == 0 && s.vals == nullptr && s.valid[0] == 0);
    CHECK(tags_slice(c, -1, 2, &s) == TAGS_PLAN_ROWS && tags_slice(c, 0, -2, &s) == TAGS_PLAN_ROWS);
    // 32-bit offsets: 2^31 - 1 values fit, 2^31 do not
    CHECK(tags_slice_fits(0) && tags_slice_fits(0x7FFFFFFFll) && !tags_slice_fits(0x80000000ll) && !tags_slice_fits(-1));
  }
  // ---- set normalisation, the 4096 / 4097 limit, need
  {
    TagsQuery q;
    const std::vector<int64_t> raw{9, NUL, 3, 9, INT64_MAX, 3, INT64_MIN + 1, NUL};
    CHECK(tags_query(raw.data(), (int64_t)raw.size(), TAGS_NEED_ALL, &q) == TAGS_PLAN_OK);
    CHECK((q.set == std::vector<int64_t>{INT64_MIN + 1, 3, 9, INT64_MAX}) && q.t == 4);
    CHECK(tags_query(raw.data(), (int64_t)raw.size(), 1, &q) == TAGS_PLAN_OK && q.t == 1 && q.set.size() == 4);
    CHECK(tags_query(raw.data(), (int64_t)raw.size(), 5, &q) == TAGS_PLAN_OK && q.t == 5);  // more than |S|: keeps none
    CHECK(tags_query(raw.data(), (int64_t)raw.size(), INT32_MAX, &q) == TAGS_PLAN_OK && q.t == INT32_MAX);
    CHECK(tags_query(nullptr, 0, TAGS_NEED_ALL, &q) == TAGS_PLAN_OK && q.set.empty() && q.t == 0);  // ALL of nothing
    CHECK(tags_query(nullptr, 0, 1, &q) == TAGS_PLAN_OK && q.set.empty() && q.t == 1);              // ANY of nothing
    const int64_t only_null[2] = {NUL, NUL};
    CHECK(tags_query(only_null, 2, TAGS_NEED_ALL, &q) == TAGS_PLAN_OK && q.set.empty() && q.t == 0);
    CHECK(tags_query(raw.data(), 3, -1, &q) == TAGS_PLAN_NEED);
    CHECK(tags_query(raw.data(), -1, 1, &q) == TAGS_PLAN_SET);
    CHECK(tags_query(nullptr, 2, 1, &q) == TAGS_PLAN_SET);
    std::vector<int64_t> big;
    for (int64_t i = 0; i < 4097; ++i) big.push_back(i * 3 - 100);
    CHECK(tags_query(big.data(), 4096, 1, &q) == TAGS_PLAN_OK && q.set.size() == 4096);
    CHECK(tags_query(big.data(), 4097, 1, &q) == TAGS_PLAN_SET_VALUES && q.set.empty());
    big.insert(big.end(), big.begin(), big.begin() + 4096);  // duplicates and NULL do not count against the limit
    big[4096] = NUL;
    CHECK(tags_query(big.data(), (int64_t)big.size(), TAGS_NEED_ALL, &q) == TAGS_PLAN_OK && q.set.size() == 4096 && q.t == 4096);
  }
  // ---- tags_plan_keeps against a brute-force loop
  {
    std::mt19937_64 rng(11);
    for (int trial = 0; trial < 2000; ++trial) {
      std::vector<int64_t> row, set;
      const int universe = 1 + (int)(rng() % 40);
      for (int j = (int)(rng() % 30); j > 0; --j) row.push_back((int64_t)(rng() % universe));
      if (rng() % 10 == 0) row.push_back(NUL);
      for (int j = (int)(rng() % 12); j > 0; --j) set.push_back(rng() % 9 == 0 ? NUL : (int64_t)(rng() % universe));
      const int32_t need = (int32_t)(rng() % 6);  // 0 = ALL
      const bool negate = rng() % 2;
      Csr in({row});
      TagsColumn c;
      CHECK(tags_normalise(in.off.data(), 1, in.vals.data(), &c) == TAGS_PLAN_OK);
      TagsQuery q;
      CHECK(tags_query(set.data(), (int64_t)set.size(), need, &q) == TAGS_PLAN_OK);
      // brute force, from the caller's own arrays
      bool is_null = false;
      for (int64_t v : row) is_null = is_null || v == NUL;
      std::set<int64_t> S(set.begin(), set.end()), R(row.begin(), row.end());
      S.erase(NUL);
      int64_t cnt = 0;
      for (int64_t v : R) cnt += S.count(v) ? 1 : 0;
      const int64_t t = need == 0 ? (int64_t)S.size() : need;
      const bool want = !is_null && ((cnt >= t) != negate);
      CHECK(tags_plan_keeps(q, c.vals.data(), c.off[1], c.null[0] != 0, negate) == want);
    }
    TagsQuery q;  // a row beyond the column: NULL whatever the term
    CHECK(tags_query(nullptr, 0, TAGS_NEED_ALL, &q) == TAGS_PLAN_OK);
    CHECK(!tags_plan_keeps(q, nullptr, 0, true, false) && !tags_plan_keeps(q, nullptr, 0, true, true));
    CHECK(tags_plan_keeps(q, nullptr, 0, false, false));  // ALL of nothing keeps the empty set
  }
  std::printf("tags plan ok\n");
  return 0;
}
