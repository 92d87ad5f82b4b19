// The host plan of a WHERE clause (tostore_amd/csrc/tsh_where_plan.h), alone: no HIP, no handles.  Built by
// tests/test_host_where_plan.py with g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined and run; prints
// "where plan ok" when every check holds.
#include "../../tostore_amd/csrc/tsh_where_plan.h"

#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>

using namespace tsh;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

static char g_cols[16];  // sixteen distinct column keys (only their addresses are used)

static WhereTermIn range(int col, int64_t lo, int64_t hi, int clause, bool negate = false) {
  WhereTermIn t;
  t.column = &g_cols[col];
  t.lo = lo;
  t.hi = hi;
  t.clause = clause;
  t.negate = negate;
  return t;
}

static WhereTermIn in_set(int col, const std::vector<int64_t> &v, int clause, bool negate = false) {
  WhereTermIn t;
  t.column = &g_cols[col];
  t.kind = WHERE_KIND_IN;
  t.set = v.empty() ? nullptr : v.data();
  t.n_set = (int64_t)v.size();
  t.clause = clause;
  t.negate = negate;
  return t;
}

static int last_flags(const WherePlan &p) {
  int bits = 0;
  for (int t = 0; t < p.n_terms; ++t) bits += (p.terms[t].flags & WHERE_F_LAST) ? 1 : 0;
  return bits;
}

int main() {
  WherePlan p;
  // ---- columns: the same handle in terms 0, 5 and 31 is one column; first appearance orders the table
  {
    std::vector<WhereTermIn> in;
    for (int t = 0; t < 32; ++t) in.push_back(range(t == 0 || t == 5 || t == 31 ? 3 : 4 + t % 7, t, t + 1, 0));
    CHECK(where_plan(in.data(), 32, &p) == WHERE_PLAN_OK);
    CHECK(p.n_terms == 32 && p.n_cols == 8);
    CHECK(p.columns[0] == &g_cols[3]);
    CHECK(p.terms[0].col == 0 && p.terms[5].col == 0 && p.terms[31].col == 0);
    for (int t = 0; t < 32; ++t) {
      CHECK(p.columns[p.terms[t].col] == in[(size_t)t].column);
      CHECK(p.terms[t].lo == t && p.terms[t].hi == t + 1 && p.terms[t].set_n == 0);
    }
    for (int a = 0; a < p.n_cols; ++a)
      for (int b = a + 1; b < p.n_cols; ++b) CHECK(p.columns[a] != p.columns[b]);
    CHECK(p.set.empty());
  }
  // ---- eight distinct columns pass, nine are refused (wherever the ninth comes)
  {
    std::vector<WhereTermIn> in;
    for (int t = 0; t < 8; ++t) in.push_back(range(t, 0, 1, t));
    CHECK(where_plan(in.data(), 8, &p) == WHERE_PLAN_OK && p.n_cols == 8);
    in.push_back(range(2, 0, 1, 8));  // a ninth TERM over a column already named
    CHECK(where_plan(in.data(), 9, &p) == WHERE_PLAN_OK && p.n_cols == 8 && p.terms[8].col == 2);
    in.push_back(range(8, 0, 1, 9));
    CHECK(where_plan(in.data(), 10, &p) == WHERE_PLAN_COLUMNS);
    CHECK(p.n_terms == 0);
  }
  // ---- term counts, kinds, sets, column keys
  {
    WhereTermIn one = range(0, 1, 2, 0);
    CHECK(where_plan(nullptr, 1, &p) == WHERE_PLAN_N_TERMS);
    CHECK(where_plan(&one, 0, &p) == WHERE_PLAN_N_TERMS && where_plan(&one, -1, &p) == WHERE_PLAN_N_TERMS);
    std::vector<WhereTermIn> many(33, one);
    CHECK(where_plan(many.data(), 33, &p) == WHERE_PLAN_N_TERMS && where_plan(many.data(), 32, &p) == WHERE_PLAN_OK);
    WhereTermIn bad = one;
    bad.kind = 2;
    CHECK(where_plan(&bad, 1, &p) == WHERE_PLAN_KIND);
    bad.kind = -1;
    CHECK(where_plan(&bad, 1, &p) == WHERE_PLAN_KIND);
    bad = one;
    bad.column = nullptr;
    CHECK(where_plan(&bad, 1, &p) == WHERE_PLAN_COLUMN);
    bad = one;
    bad.kind = WHERE_KIND_IN;
    bad.n_set = -1;
    CHECK(where_plan(&bad, 1, &p) == WHERE_PLAN_SET);
    bad.n_set = 3;  // (and set is NULL)
    CHECK(where_plan(&bad, 1, &p) == WHERE_PLAN_SET);
    bad = one;
    bad.n_set = -5;  // a range term's set fields are held to the same
    CHECK(where_plan(&bad, 1, &p) == WHERE_PLAN_SET);
  }
  // ---- a set comes out sorted, without duplicates, without the NULL; the empty set and the NULL-only set are empty
  {
    const std::vector<int64_t> v = {7, INT64_MAX, 3, 7, WHERE_NULL, -2, INT64_MIN + 1, 3, 3, WHERE_NULL, 0};
    const std::vector<int64_t> none, nulls = {WHERE_NULL, WHERE_NULL};
    WhereTermIn in[3] = {in_set(0, v, 0), in_set(0, none, 0, true), in_set(1, nulls, 1)};
    CHECK(where_plan(in, 3, &p) == WHERE_PLAN_OK);
    const std::vector<int64_t> want = {INT64_MIN + 1, -2, 0, 3, 7, INT64_MAX};
    CHECK(p.set == want);
    CHECK(p.terms[0].set_off == 0 && p.terms[0].set_n == 6 && p.terms[0].flags == WHERE_F_IN);
    CHECK(p.terms[1].set_n == 0 && p.terms[1].flags == (WHERE_F_IN | WHERE_F_NEGATE | WHERE_F_LAST));
    CHECK(p.terms[2].set_n == 0 && p.terms[2].col == 1 && p.terms[2].flags == (WHERE_F_IN | WHERE_F_LAST));
  }
  // ---- 4096 distinct values pass, 4097 do not; 5000 values that dedupe to 4096 pass; the budget is the call's
  {
    std::vector<int64_t> v(4096);
    std::iota(v.begin(), v.end(), -2000);
    WhereTermIn t = in_set(0, v, 0);
    CHECK(where_plan(&t, 1, &p) == WHERE_PLAN_OK && p.set.size() == 4096 && p.terms[0].set_n == 4096);
    v.push_back(5000);
    t = in_set(0, v, 0);
    CHECK(where_plan(&t, 1, &p) == WHERE_PLAN_SET_VALUES && p.n_terms == 0);
    v.pop_back();
    std::mt19937_64 rng(5);
    for (int i = 0; i < 903; ++i) v.push_back(v[(size_t)(rng() % 4096)]);  // 4999 values, 4096 distinct ...
    v.push_back(WHERE_NULL);                                               // ... and a NULL: 5000
    std::shuffle(v.begin(), v.end(), rng);
    CHECK(v.size() == 5000);
    t = in_set(0, v, 0);
    CHECK(where_plan(&t, 1, &p) == WHERE_PLAN_OK && p.set.size() == 4096);
    CHECK(std::is_sorted(p.set.begin(), p.set.end()) && p.set.front() == -2000 && p.set.back() == 2095);
    v.push_back(2096);  // 5001 values, 4097 distinct
    t = in_set(0, v, 0);
    CHECK(where_plan(&t, 1, &p) == WHERE_PLAN_SET_VALUES);
    // three terms share the budget: 2000 + 2000 + 96 pass, one more value anywhere does not
    std::vector<int64_t> a(2000), b(2000), c(96);
    std::iota(a.begin(), a.end(), 0);
    std::iota(b.begin(), b.end(), 1000);  // (overlapping a: a value counts once per term that holds it)
    std::iota(c.begin(), c.end(), -50);
    WhereTermIn three[3] = {in_set(0, a, 0), in_set(1, b, 0), in_set(0, c, 1)};
    CHECK(where_plan(three, 3, &p) == WHERE_PLAN_OK && p.set.size() == 4096);
    c.push_back(4711);
    three[2] = in_set(0, c, 1);
    CHECK(where_plan(three, 3, &p) == WHERE_PLAN_SET_VALUES);
  }
  // ---- offsets of several sets in the one array, range terms between them
  {
    const std::vector<int64_t> a = {5, 1, 3}, b = {}, c = {9, 9, 8}, d = {WHERE_NULL, 2};
    WhereTermIn in[6] = {in_set(0, a, 0), range(1, 4, 6, 0), in_set(1, b, 1), in_set(2, c, 1), range(0, 0, 0, 2), in_set(0, d, 2)};
    CHECK(where_plan(in, 6, &p) == WHERE_PLAN_OK);
    const std::vector<int64_t> want = {1, 3, 5, 8, 9, 2};
    CHECK(p.set == want);
    CHECK(p.terms[0].set_off == 0 && p.terms[0].set_n == 3);
    CHECK(p.terms[1].set_off == 0 && p.terms[1].set_n == 0 && p.terms[1].lo == 4 && p.terms[1].hi == 6);
    CHECK(p.terms[2].set_off == 3 && p.terms[2].set_n == 0);
    CHECK(p.terms[3].set_off == 3 && p.terms[3].set_n == 2);
    CHECK(p.terms[5].set_off == 5 && p.terms[5].set_n == 1);
    CHECK(p.n_cols == 3 && p.terms[3].col == 2 && p.terms[5].col == 0);
    CHECK(last_flags(p) == 3 && (p.terms[1].flags & WHERE_F_LAST) && (p.terms[3].flags & WHERE_F_LAST) && (p.terms[5].flags & WHERE_F_LAST));
  }
  // ---- clause flags: 1 clause of 32 terms, 32 clauses of 1 term, 3 + 1 + 2
  {
    std::vector<WhereTermIn> in;
    for (int t = 0; t < 32; ++t) in.push_back(range(0, t, t, 0));
    CHECK(where_plan(in.data(), 32, &p) == WHERE_PLAN_OK && last_flags(p) == 1 && (p.terms[31].flags & WHERE_F_LAST));
    for (int t = 0; t < 32; ++t) in[(size_t)t].clause = t;
    CHECK(where_plan(in.data(), 32, &p) == WHERE_PLAN_OK && last_flags(p) == 32);
    const int split[6] = {0, 0, 0, 1, 2, 2};
    for (int t = 0; t < 6; ++t) in[(size_t)t].clause = split[t];
    CHECK(where_plan(in.data(), 6, &p) == WHERE_PLAN_OK && last_flags(p) == 3);
    for (int t = 0; t < 6; ++t) CHECK(((p.terms[t].flags & WHERE_F_LAST) != 0) == (t == 2 || t == 3 || t == 5));
    // out of order: 0, 0, 2 skips; 1 does not start at 0; 0, 1, 0 goes back; a negative number
    const int bad[4][3] = {{0, 0, 2}, {1, 1, 1}, {0, 1, 0}, {0, -1, 0}};
    for (const auto &b : bad) {
      for (int t = 0; t < 3; ++t) in[(size_t)t].clause = b[t];
      CHECK(where_plan(in.data(), 3, &p) == WHERE_PLAN_CLAUSE);
    }
  }
  // ---- the plan's arithmetic against the definition, row by row: (tenant IN S OR NOT ts in [10, 20]) AND flag != 1
  {
    const std::vector<int64_t> S = {4, 2, 2, 9};
    WhereTermIn in[3] = {in_set(0, S, 0), range(1, 10, 20, 0, true), range(2, 1, 1, 1, true)};
    CHECK(where_plan(in, 3, &p) == WHERE_PLAN_OK);
    const int64_t vals[] = {WHERE_NULL, 1, 2, 4, 9, 10, 15, 20, 21, INT64_MAX};
    for (int64_t a : vals)
      for (int64_t b : vals)
        for (int64_t c : vals) {
          const bool t0 = a != WHERE_NULL && (a == 2 || a == 4 || a == 9);
          const bool t1 = b != WHERE_NULL && !(10 <= b && b <= 20);
          const bool t2 = c != WHERE_NULL && c != 1;
          const int64_t row[3] = {a, b, c};
          CHECK(where_plan_keeps(p, row) == ((t0 || t1) && t2));
        }
  }
  for (int e = WHERE_PLAN_OK; e <= WHERE_PLAN_SET_VALUES; ++e) CHECK(where_plan_error(e)[0] != '?');
  std::printf("where plan ok\n");
  return 0;
}
