// Host-only check of tostore_amd/csrc/tsh_finalize.h: the finaliser (finalize_query, count_entries) against a reference
// written out here -- the distance of every entry, the two predicates stated on their own, ONE std::sort by
// (after_order_key(distance), id), the cut:
//   threshold  an entry is dropped iff d > thr under IEEE > (a NaN threshold drops nothing, a NaN distance passes any)
//   cursor     an entry is dropped unless its (key, id) is strictly greater than the cursor's; a cursor at -inf is
//              "from the start" and drops nothing, whatever its id
// The finaliser gets there by a bucket sort (sort_hits: std::sort below 24 and above 60000 entries), an nth_element when
// k is small beside the candidates, vectorised distances and thread-local buffers; none of that may show.
// Seeded cases: list sizes 0, 1, 23, 24, 25, 300, 700 and 60500; k in {0, 1, n / 8, n, n + 5}; distances at random, in
// exact ties under different and repeated ids, with NaN, +-0, +inf and denormals among them, all keys within 512 of one
// another (shift 0), and from 1e-300 to 1e300; L2, inner product, cosine (rows with s1 == 0, a zero query); no
// threshold, one equal to a present distance, one in between; no cursor, -inf, one equal to a present (distance, id), NaN,
// +inf; every case as one list and split over two.  Also: unused output slots read -1 / NaN, count_entries is the
// reference's count before the cut, and Cursors::at / from give what the hand-written blocks gave.  Exit status 1 on a miss.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../tostore_amd/csrc/tsh_finalize.h"

using namespace tsh;

static int fails = 0;
static long checks = 0;

static void miss(const char *what, int metric, size_t n, int k, int flavour) {
  if (++fails <= 20) printf("MISS %s: metric %d n %zu k %d flavour %d\n", what, metric, n, k, flavour);
}
static bool same_double(double a, double b) {  // bit for bit, every NaN alike
  if (a != a || b != b) return a != a && b != b;
  return memcmp(&a, &b, 8) == 0;
}

// ---- the reference ------------------------------------------------------------------------------------------------
static double ref_distance(int metric, const BlockEntry &e, double mag_a) {
  if (metric == 0) return std::sqrt(e.s0);
  if (metric == 1) return -e.s0;
  const double denom = std::sqrt(mag_a) * std::sqrt(e.s1);
  const double sim = denom > 0 ? e.s0 / denom : 0;
  return 1.0 - sim;
}
struct RefRow {
  uint64_t key;
  int64_t id;
  double d;
};
struct RefOut {
  std::vector<RefRow> rows;  // the first min(k, passed) in order
  int64_t passed = 0;        // before the cut
};
static RefOut reference(int metric, int dim, const float *q, int k, double thr, const std::vector<BlockEntry> &e,
                        const Cursor *cur) {
  double mag_a = 0;
  for (int i = 0; i < dim; ++i) mag_a = mag_a + (double)q[i] * (double)q[i];
  std::vector<RefRow> rows;
  for (const BlockEntry &x : e) {
    const double d = ref_distance(metric, x, mag_a);
    if (thr == thr && d > thr) continue;
    const uint64_t key = after_order_key(d);
    if (cur && cur->dist != -INFINITY) {
      const uint64_t ck = after_order_key(cur->dist);
      const bool follows = key > ck || (key == ck && x.id > cur->id);
      if (!follows) continue;
    }
    rows.push_back({key, x.id, d});
  }
  std::sort(rows.begin(), rows.end(), [](const RefRow &a, const RefRow &b) { return a.key != b.key ? a.key < b.key : a.id < b.id; });
  RefOut out;
  out.passed = (int64_t)rows.size();
  rows.resize(std::min(rows.size(), (size_t)std::max(k, 0)));
  out.rows = rows;
  return out;
}

// ---- entries ------------------------------------------------------------------------------------------------------
enum { RANDOM = 0, TIES = 1, SPECIALS = 2, NARROW = 3, WIDE = 4, N_FLAVOURS = 5 };
static const int DIM = 8;

static std::vector<BlockEntry> make_entries(std::mt19937_64 &rng, size_t n, int metric, int flavour, double mag_a) {
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::vector<BlockEntry> e(n);
  const double tie_vals[5] = {0.25, 1.0, 1.0000000000000002, 3.5, 0.0};
  const double specials[10] = {std::nan(""), 0.0, -0.0, INFINITY, 4.9406564584124654e-324, 2.2250738585072009e-308,
                               -1.0, 1.0, -INFINITY, 1e-320};
  double narrow_base = 1.0 + u(rng);
  for (size_t i = 0; i < n; ++i) {
    BlockEntry &x = e[i];
    x.id = flavour == TIES ? (int64_t)(rng() % 7) : (int64_t)(rng() % (4 * n + 16));
    x.s1 = 0;
    double v;  // the value the metric's distance is made of
    switch (flavour) {
      case TIES: v = tie_vals[rng() % 5]; break;
      case SPECIALS: v = (rng() % 3) ? u(rng) * 4.0 : specials[rng() % 10]; break;
      case NARROW: {
        v = narrow_base;
        for (int s = (int)(rng() % 200); s > 0; --s) v = std::nextafter(v, INFINITY);
        break;
      }
      case WIDE: v = std::pow(10.0, u(rng) * 600.0 - 300.0) * ((rng() & 1) && metric == 1 ? -1.0 : 1.0); break;
      default: v = u(rng) * 10.0; break;
    }
    if (metric == 2) {
      // d = 1 - s0 / (sqrt(mag_a) sqrt(s1)): one row in eight is a zero row (s1 == 0)
      x.s1 = (rng() % 8) == 0 ? 0.0 : 0.5 + u(rng) * 3.0;
      if (flavour == WIDE) x.s1 = std::pow(10.0, u(rng) * 40.0 - 20.0);
      const double scale = std::sqrt(mag_a) * std::sqrt(x.s1);
      x.s0 = flavour == RANDOM || flavour == WIDE ? (u(rng) * 2.0 - 1.0) * scale : v * 0.25 * scale;
      if (flavour == TIES) x.s1 = 2.0, x.s0 = v * 0.25;  // (the same sums: the same distance)
    } else {
      x.s0 = metric == 1 && (flavour == RANDOM || flavour == TIES) ? v - 5.0 : v;  // (inner product: both signs)
    }
  }
  return e;
}

// ---- one case: the finaliser, as one list and as two, against the reference -----------------------------------------
static void run_case(int metric, const float *q, int k, double thr, const std::vector<BlockEntry> &e, const Cursor *cur,
                     size_t split, int flavour) {
  const size_t n = e.size();
  const RefOut ref = reference(metric, DIM, q, k, thr, e, cur);
  const double mag_a = query_mag_a(q, DIM);
  for (int form = 0; form < 3; ++form) {
    // 0: one list; 1: two lists, mag_a handed in; 2: the vector overload over two lists
    std::vector<int64_t> ids((size_t)std::max(k, 0) + 1, 12345);
    std::vector<double> dist((size_t)std::max(k, 0) + 1, 7.0);
    const EntryList one[1] = {{e.data(), (uint32_t)n}};
    const EntryList two[2] = {{e.data(), (uint32_t)split}, {e.data() + split, (uint32_t)(n - split)}};
    int32_t r;
    if (form == 0) r = finalize_query(metric, DIM, q, k, thr, one, 1, ids.data(), dist.data(), nullptr, cur);
    else if (form == 1) r = finalize_query(metric, DIM, q, k, thr, two, 2, ids.data(), dist.data(), &mag_a, cur);
    else r = finalize_query(metric, DIM, q, k, thr, std::vector<EntryList>(two, two + 2), ids.data(), dist.data(), cur);
    ++checks;
    if ((size_t)r != ref.rows.size()) {
      miss("count of results", metric, n, k, flavour);
      continue;
    }
    bool ok = true;
    for (size_t i = 0; i < ref.rows.size(); ++i)
      if (ids[i] != ref.rows[i].id || !same_double(dist[i], ref.rows[i].d)) ok = false;
    if (!ok) miss("order", metric, n, k, flavour);
    ok = true;
    for (size_t i = ref.rows.size(); i < (size_t)std::max(k, 0); ++i)
      if (ids[i] != -1 || dist[i] == dist[i]) ok = false;
    if (ids.back() != 12345 || dist.back() != 7.0) ok = false;  // (nothing past k is touched)
    if (!ok) miss("unused slots", metric, n, k, flavour);
    const int64_t cnt = form == 0 ? count_entries(metric, DIM, q, thr, one, 1, cur) : count_entries(metric, DIM, q, thr, two, 2, cur);
    if (cnt != ref.passed) miss("count_entries", metric, n, k, flavour);
  }
}

static void sweep(std::mt19937_64 &rng, int metric, size_t n, int flavour, const float *q) {
  const double mag_a = query_mag_a(q, DIM);
  const std::vector<BlockEntry> e = make_entries(rng, n, metric, flavour, mag_a);
  if (flavour == NARROW && metric == 1 && n > 1) {  // the case is what it says: one bucket per key, shift 0
    uint64_t lo = ~0ull, hi = 0;
    for (const BlockEntry &x : e) {
      lo = std::min(lo, after_order_key(-x.s0));
      hi = std::max(hi, after_order_key(-x.s0));
    }
    if (hi - lo >= 512) miss("narrow keys are not narrow", metric, n, 0, flavour);
  }
  const BlockEntry *pick = n ? &e[rng() % n] : nullptr;
  const double d_pick = pick ? ref_distance(metric, *pick, mag_a) : 1.0;
  const int ks[5] = {0, 1, (int)(n / 8), (int)n, (int)n + 5};  // (n / 8: candidates > 4 k, the nth_element branch)
  const double thrs[3] = {std::nan(""), d_pick, 2.5};           // none, a present distance (that row stays), in between
  Cursor curs[5];
  curs[1].dist = -INFINITY, curs[1].id = 3;
  curs[2].dist = d_pick, curs[2].id = pick ? pick->id : 0;      // a present (distance, id): that row goes, larger ids stay
  curs[3].dist = std::nan(""), curs[3].id = (int64_t)(rng() % 7);
  curs[4].dist = INFINITY, curs[4].id = (int64_t)(rng() % 7);
  for (int k : ks)
    for (double thr : thrs)
      for (int c = 0; c < 5; ++c) {
        if (n > 1000 && (k == 1 || c == 3)) continue;  // (the one large list: a few of the combinations)
        run_case(metric, q, k, thr, e, c ? &curs[c] : nullptr, n ? rng() % (n + 1) : 0, flavour);
      }
}

// ---- the two edges, spelled out -------------------------------------------------------------------------------------
static void edges() {
  const float q[DIM] = {1, 0, 0, 0, 0, 0, 0, 0};
  // inner product: d = -s0.  Three rows at the same distance, one before, one after
  const std::vector<BlockEntry> e = {{7, -2.0, 0}, {5, -2.0, 0}, {6, -2.0, 0}, {1, -1.0, 0}, {9, -3.0, 0}};
  const EntryList l[1] = {{e.data(), (uint32_t)e.size()}};
  int64_t ids[8];
  double dist[8];
  Cursor cur;
  cur.dist = 2.0, cur.id = 6;  // the row (2.0, 6) itself is excluded, (2.0, 7) follows, (2.0, 5) and (1.0, 1) do not
  int32_t r = finalize_query(1, DIM, q, 8, std::nan(""), l, 1, ids, dist, nullptr, &cur);
  ++checks;
  if (r != 2 || ids[0] != 7 || dist[0] != 2.0 || ids[1] != 9 || dist[1] != 3.0) miss("cursor at a present row", 1, e.size(), 8, -1);
  if (count_entries(1, DIM, q, std::nan(""), l, 1, &cur) != 2) miss("count at a present row", 1, e.size(), 8, -1);
  // a threshold equal to a present distance keeps that distance's rows
  r = finalize_query(1, DIM, q, 8, 2.0, l, 1, ids, dist, nullptr, nullptr);
  ++checks;
  if (r != 4 || ids[0] != 1 || ids[1] != 5 || ids[2] != 6 || ids[3] != 7 || ids[4] != -1) miss("threshold at a present distance", 1, e.size(), 8, -1);
  if (count_entries(1, DIM, q, 2.0, l, 1, nullptr) != 4) miss("count at a present distance", 1, e.size(), 8, -1);
}

// ---- Cursors: what the hand-written blocks gave ---------------------------------------------------------------------
static void cursors() {
  const double dist[5] = {0.5, -INFINITY, std::nan(""), 3.0, -0.0};
  const int64_t id[5] = {11, 12, 13, 14, 15};
  const Cursors c{dist, id};
  const Cursors none;
  ++checks;
  if (!c || none) miss("Cursors bool", 0, 0, 0, -1);
  for (int64_t q0 = 0; q0 < 5; ++q0)
    for (int64_t q = 0; q0 + q < 5; ++q) {
      Cursor want;  // (the block every call site wrote out)
      want.dist = dist[q0 + q];
      want.id = id[q0 + q];
      Cursor tmp;
      const Cursor *got = c.from(q0).at(q, &tmp);
      if (got != &tmp || !same_double(got->dist, want.dist) || got->id != want.id) miss("Cursors at / from", 0, 0, (int)q, -1);
    }
  Cursor tmp;
  if (none.at(3, &tmp) != nullptr || none.from(2) || none.from(2).at(0, &tmp) != nullptr) miss("no cursors", 0, 0, 0, -1);
  if (half_cursor(dist, id) || half_cursor(nullptr, nullptr) || !half_cursor(dist, nullptr) || !half_cursor(nullptr, id))
    miss("half_cursor", 0, 0, 0, -1);
}

int main() {
  std::mt19937_64 rng(20261019);
  float q_rand[DIM], q_zero[DIM] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::uniform_real_distribution<float> uf(-1.f, 1.f);
  for (float &x : q_rand) x = uf(rng);
  const size_t sizes[7] = {0, 1, 23, 24, 25, 300, 700};
  for (int metric = 0; metric < 3; ++metric)
    for (int flavour = 0; flavour < N_FLAVOURS; ++flavour) {
      for (size_t n : sizes) sweep(rng, metric, n, flavour, q_rand);
      if (metric == 2) sweep(rng, metric, 300, flavour, q_zero);  // a zero query: every denominator is zero
    }
  for (int metric = 0; metric < 3; ++metric) sweep(rng, metric, 60500, metric == 0 ? RANDOM : (metric == 1 ? TIES : SPECIALS), q_rand);
  edges();
  cursors();
  printf("%ld checks, %d misses\n", checks, fails);
  if (fails) return 1;
  printf("finalize ok\n");
  return 0;
}
