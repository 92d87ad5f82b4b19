// Host-only check of tostore_amd/csrc/tsh_group_rule.h, the rules of a grouped search, in three parts.
// (a) A software model of the scan: exact sums per row, the f32 key of every row pushed to EITHER end of the per-key bound
//     the error model claims (compute_band's arithmetic is repeated here) and rounded inwards, the three metrics, dead
//     rows, six group layouts -- through the rule header's head word, head test, band and side predicate exactly as the
//     kernels apply them (tiles of 64, tau = the k-th smallest tile minimum of heads, or the exact k-th head key, or no
//     bound) and through finalize_grouped, against a brute-force grouped list over ALL live rows written from the
//     specification.
// (b) The finaliser's step against the specification written a second time: ties, -0.0 / +0.0, NaN distances, thresholds.
// (c) The cross-shard merge claim: ranks answer for their own rows; concatenating, ordering, dropping repeated groups and
//     cutting to k gives the global answer, on random splits.
// Exit status 1 on a miss.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../tostore_amd/csrc/tsh_group_rule.h"

using namespace tsh;

static int fails = 0;
static long checks = 0, n_side = 0, n_heads_taken = 0;

// Dart double.compareTo, from its documentation: NaN greatest and equal to itself, -0.0 < +0.0
static int dart_compare(double a, double b) {
  if (a < b) return -1;
  if (a > b) return 1;
  if (a == b) {
    if (a == 0.0) {
      const bool na = std::signbit(a), nb = std::signbit(b);
      return na == nb ? 0 : (na ? -1 : 1);
    }
    return 0;
  }
  const bool an = a != a, bn = b != b;
  return an && bn ? 0 : (an ? 1 : -1);
}
static uint64_t bits(double d) {
  uint64_t b;
  memcpy(&b, &d, 8);
  return b;
}

struct Res {
  int64_t id;
  double d;
  int32_t g;
};
// the specification, a second time: L (threshold applied: dropped iff d > T, a NaN T drops nothing) in (compareTo, id)
// order, the first entry of each group, cut to k
static std::vector<Res> spec_grouped(std::vector<Res> rows, double T, size_t k) {
  std::vector<Res> L;
  for (const Res &r : rows)
    if (T != T || !(r.d > T)) L.push_back(r);
  std::sort(L.begin(), L.end(), [](const Res &a, const Res &b) {
    const int c = dart_compare(a.d, b.d);
    return c != 0 ? c < 0 : a.id < b.id;
  });
  std::vector<Res> G;
  std::set<int32_t> seen;
  for (const Res &r : L) {
    if (G.size() >= k) break;
    if (r.g >= 0 && !seen.insert(r.g).second) continue;
    G.push_back(r);
  }
  return G;
}
static bool same(const char *what, const std::vector<Res> &want, const int64_t *ids, const double *dist, const int32_t *grp, int32_t cnt) {
  ++checks;
  bool ok = (size_t)cnt == want.size();
  for (size_t i = 0; ok && i < want.size(); ++i)
    ok = ids[i] == want[i].id && (bits(dist[i]) == bits(want[i].d) || (dist[i] != dist[i] && want[i].d != want[i].d)) && grp[i] == want[i].g;
  if (!ok && fails++ < 10) {
    printf("%s: got %d entries, want %zu\n", what, cnt, want.size());
    for (size_t i = 0; i < std::max<size_t>(want.size(), (size_t)std::max(cnt, 0)) && i < 12; ++i)
      printf("  [%zu] got (%lld, %.17g, %d) want (%lld, %.17g, %d)\n", i, i < (size_t)cnt ? (long long)ids[i] : -9LL, i < (size_t)cnt ? dist[i] : 0.0,
             i < (size_t)cnt ? grp[i] : -9, i < want.size() ? (long long)want[i].id : -9LL, i < want.size() ? want[i].d : 0.0, i < want.size() ? want[i].g : -9);
  }
  return ok;
}

// ---- (a) ----------------------------------------------------------------------------------------------------------------
struct Row {
  BlockEntry e;     // what the re-rank would hand the finaliser
  double dist;      // the finaliser's distance, written here again
  long double val;  // what the key stands for
  double bound;     // the per-key bound at this value
  bool live;
};
static bool model_key(const Row &r, bool upper, float *out) {
  const long double lo = r.val - (long double)r.bound, hi = r.val + (long double)r.bound;
  float a = (float)lo, b = (float)hi;
  if ((long double)a < lo) a = std::nextafter(a, INFINITY);
  if ((long double)b > hi) b = std::nextafter(b, -INFINITY);
  if (!((long double)a <= hi && (long double)b >= lo)) return false;  // no f32 inside: take the nearest
  *out = upper ? b : a;
  return true;
}

static std::vector<int32_t> layout(int kind, size_t n, std::mt19937_64 &rng, int32_t *n_groups) {
  std::vector<int32_t> g(n);
  *n_groups = std::max<int32_t>((int32_t)n + 1, 8);  // (every id below it, as tsh_groups_create demands)
  for (size_t i = 0; i < n; ++i) {
    switch (kind) {
      case 0: g[i] = (int32_t)(i / 7); break;                                        // runs of 7: straddle tiles
      case 1: g[i] = (int32_t)(rng() % std::max<size_t>(n / 5, 1)); break;           // random: equal ids not adjacent
      case 2: g[i] = 3; break;                                                       // one group holding every row
      case 3: g[i] = -1; break;                                                      // all ungrouped
      case 4: g[i] = (int32_t)i; break;                                              // every row its own group
      default: g[i] = rng() % 3 == 0 ? -(int32_t)(rng() % 5) - 1 : (int32_t)(rng() % std::max<size_t>(n / 9, 1)); break;  // a mix
    }
  }
  return g;
}

static void run_model(const char *what, int metric, int dim, const float *query, float eps_rel, float delta_abs, std::vector<Row> rows,
                      std::mt19937_64 &rng) {
  const size_t n = rows.size();
  const size_t n_tiles = (n + 63) / 64;
  for (int kind = 0; kind < 6; ++kind)
    for (int key_mode = 0; key_mode < 3; ++key_mode) {  // every key at the lower end, the upper end, a random end
      int32_t n_groups;
      const std::vector<int32_t> grp = layout(kind, n, rng, &n_groups);
      const GroupTable table{grp.data(), (int64_t)(kind == 5 ? n - n / 10 : n)};  // (the mix: the array ends before the rows do)
      std::vector<uint32_t> keys(n_tiles * 64, GROUP_KEY_DEAD);
      for (size_t i = 0; i < n; ++i) {
        if (!rows[i].live) continue;
        float kf;
        const bool upper = key_mode == 1 || (key_mode == 2 && (rng() & 1));
        if (!model_key(rows[i], upper, &kf)) kf = (float)rows[i].val;
        keys[i] = group_f2key(kf);
      }
      // G1: the head table (any arrival order: a minimum)
      std::vector<uint64_t> gm((size_t)n_groups, GROUP_WORD_NONE);
      auto group_at = [&](size_t i) { return table.at((int64_t)i); };
      for (size_t i = 0; i < n; ++i) {
        const int32_t g = group_at(i);
        if (keys[i] == GROUP_KEY_DEAD || !group_valid(g, n_groups)) continue;
        gm[(size_t)g] = std::min(gm[(size_t)g], group_head_word(keys[i], (uint32_t)i));
      }
      // G2: heads and their tile minima
      std::vector<uint32_t> heads(n_tiles * 64, GROUP_KEY_DEAD), hmin(n_tiles, GROUP_KEY_DEAD);
      for (size_t i = 0; i < n; ++i) {
        if (keys[i] == GROUP_KEY_DEAD) continue;
        const int32_t g = group_at(i);
        const bool grouped = group_valid(g, n_groups);
        if (group_is_head(grouped, group_head_word(keys[i], (uint32_t)i), grouped ? gm[(size_t)g] : 0)) heads[i] = keys[i];
        hmin[i / 64] = std::min(hmin[i / 64], heads[i]);
      }
      std::vector<Res> all;
      for (size_t i = 0; i < n; ++i)
        if (rows[i].live) all.push_back({(int64_t)i, rows[i].dist, group_at(i)});
      const size_t n_distinct = spec_grouped(all, std::nan(""), n + 1).size();
      for (size_t k : {(size_t)1, (size_t)10, (size_t)100, n_distinct + 5}) {
        std::vector<uint32_t> sorted_hmin(hmin), sorted_heads(heads);
        std::sort(sorted_hmin.begin(), sorted_hmin.end());
        std::sort(sorted_heads.begin(), sorted_heads.end());
        // the bounds a job may end up with: the k-th smallest tile minimum of heads, the exact k-th head key, none
        const uint32_t taus[3] = {k <= n_tiles && sorted_hmin[k - 1] != GROUP_KEY_DEAD ? sorted_hmin[k - 1] : GROUP_KEY_NAN,
                                  k <= sorted_heads.size() && sorted_heads[k - 1] != GROUP_KEY_DEAD ? sorted_heads[k - 1] : GROUP_KEY_NAN, GROUP_KEY_NAN};
        for (uint32_t tau : taus) {
          const uint32_t band = group_band_of(tau, eps_rel, delta_abs);
          std::vector<BlockEntry> cand, side;
          for (size_t i = 0; i < n; ++i) {
            if (keys[i] == GROUP_KEY_DEAD) continue;
            if (heads[i] != GROUP_KEY_DEAD) {
              if (heads[i] <= band) {  // the select
                cand.push_back(rows[i].e);
                ++n_heads_taken;
              }
              continue;
            }
            const uint64_t hw = gm[(size_t)group_at(i)];
            if (group_side(keys[i], group_band_of(group_word_key(hw), eps_rel, delta_abs), band)) {  // G3
              side.push_back(rows[i].e);
              ++n_side;
            }
          }
          const EntryList lists[2] = {{cand.data(), (uint32_t)cand.size()}, {side.data(), (uint32_t)side.size()}};
          std::vector<double> thrs = {std::nan("")};
          const std::vector<Res> free_list = spec_grouped(all, std::nan(""), k);
          if (!free_list.empty()) {
            const double dk = free_list.back().d;
            thrs.push_back(dk);
            thrs.push_back(std::nextafter(dk, -INFINITY));
            thrs.push_back(std::nextafter(dk, INFINITY));
          }
          for (double T : thrs) {
            std::vector<int64_t> ids(k);
            std::vector<double> dist(k);
            std::vector<int32_t> og(k);
            const int32_t cnt = finalize_grouped(metric, dim, query, (int32_t)k, T, lists, 2, table, ids.data(), dist.data(), og.data());
            char tag[160];
            snprintf(tag, sizeof tag, "(a) %s layout %d keys %d k %zu tau %08x T %.17g", what, kind, key_mode, k, tau, T);
            same(tag, spec_grouped(all, T, k), ids.data(), dist.data(), og.data(), cnt);
          }
        }
      }
    }
}

static void part_a() {
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> G(0.0, 1.0);
  const double u2 = 1.1920928955078125e-07;
  for (size_t n : {(size_t)1, (size_t)65, (size_t)700}) {
    for (int dim : {4, 768}) {
      const int nch = ((dim + 3) / 4 + 63) / 64;
      {  // L2: sums given directly, crowds a few key-bounds apart and exact ties
        const double eps = (4.0 * nch + 8.0) * u2;
        const float eps_rel = (float)(3.0 * eps), delta_abs = (float)((double)dim * 7.9e-31);
        std::vector<Row> rows;
        for (size_t i = 0; i < n; ++i) {
          double s;
          const int kind = (int)(rng() % 6);
          if (kind == 0) s = 1536.0;                                           // exact ties
          else if (kind == 1) s = 1536.0 * (1.0 + (double)((int)(rng() % 9) - 4) * eps * 0.5);  // inside one another's bands
          else if (kind == 2) s = 0.0;
          else s = std::exp((U(rng) - 0.5) * 8.0) * 1500.0;
          Row r{};
          r.e = BlockEntry{(int64_t)i, s, 0.0};
          r.dist = std::sqrt(s);
          r.val = s;
          r.bound = eps * s + (double)dim * 7.9e-31 * 0.5;
          r.live = rng() % 8 != 0;
          rows.push_back(r);
        }
        run_model("L2", 0, dim, nullptr, eps_rel, delta_abs, rows, rng);
      }
      {  // inner product: both signs, +0.0 / -0.0
        const double qn = 1.3, max_norm = 2.0;
        const double gam = (4.0 * nch + 6.0) * u2;
        const double delta = gam * (qn * (1.0 + 1e-6)) * max_norm * (1.0 + 1e-6) + (double)dim * 7.5e-37;
        const float delta_abs = (float)(2.0 * delta * 1.0001);
        std::vector<Row> rows;
        for (size_t i = 0; i < n; ++i) {
          double s0;
          const int kind = (int)(rng() % 6);
          if (kind == 0) s0 = 0.75;
          else if (kind == 1) s0 = 0.75 + (double)((int)(rng() % 9) - 4) * delta * 0.5;
          else if (kind == 2) s0 = (rng() & 1) ? 0.0 : -0.0;
          else s0 = G(rng) * qn * max_norm * 0.5;
          Row r{};
          r.e = BlockEntry{(int64_t)i, s0, 0.0};
          r.dist = -s0;
          r.val = -(long double)s0;
          r.bound = delta;
          r.live = rng() % 8 != 0;
          rows.push_back(r);
        }
        run_model("IP", 1, dim, nullptr, 0.f, delta_abs, rows, rng);
      }
      if (dim <= 16) {  // cosine: the finaliser's arithmetic on real vectors
        std::vector<float> q(dim);
        for (auto &x : q) x = (float)G(rng);
        double mag_a = 0;
        for (int i = 0; i < dim; ++i) mag_a = mag_a + (double)q[i] * (double)q[i];
        const double qn = std::sqrt(mag_a) * (1.0 + 1e-6);
        const double gam = (4.0 * nch + 6.0) * u2;
        const double delta = qn * (gam + 4.76837158203125e-07) + (double)dim * 7.5e-37;
        const float delta_abs = (float)(2.0 * delta * 1.0001);
        std::vector<Row> rows;
        std::vector<float> prev(dim, 1.f);
        for (size_t i = 0; i < n; ++i) {
          std::vector<float> v(dim);
          const int kind = (int)(rng() % 6);
          const double sc = std::exp((U(rng) - 0.5) * 6.0);
          for (int j = 0; j < dim; ++j) {
            if (kind == 0) v[j] = prev[j];                                  // a duplicate: exact ties
            else if (kind == 1) v[j] = (float)(prev[j] * 2.0);              // parallel to it: the same distance but for rounding
            else if (kind == 2) v[j] = (float)(q[j] * sc + G(rng) * sc * 1e-6);  // nearly parallel to the query: a crowd near 0
            else v[j] = (float)(G(rng) * sc);
          }
          prev = v;
          double s0 = 0, s1 = 0;
          long double dot = 0, vv = 0;
          for (int j = 0; j < dim; ++j) {
            s0 = s0 + (double)q[j] * (double)v[j];
            s1 = s1 + (double)v[j] * (double)v[j];
            dot += (long double)q[j] * (long double)v[j];
            vv += (long double)v[j] * (long double)v[j];
          }
          const double denom = std::sqrt(mag_a) * std::sqrt(s1);
          const double sim = denom > 0 ? s0 / denom : 0;
          Row r{};
          r.e = BlockEntry{(int64_t)i, s0, s1};
          r.dist = 1.0 - sim;
          r.val = vv > 0 ? -dot / sqrtl(vv) : 0.0L;
          r.bound = delta;
          r.live = rng() % 8 != 0;
          rows.push_back(r);
        }
        run_model("cosine", 2, dim, q.data(), 0.f, delta_abs, rows, rng);
      }
    }
  }
}

// ---- (b) ----------------------------------------------------------------------------------------------------------------
static void part_b() {
  std::mt19937_64 rng(7);
  const double nan = std::nan(""), inf = INFINITY;
  const double ladder[] = {-inf, -3.5, -4.9406564584124654e-324, -0.0, 0.0, 4.9406564584124654e-324, 1.0, 1.0000000000000002, 2.5, inf, nan};
  const int nl = (int)(sizeof ladder / sizeof *ladder);
  for (int round = 0; round < 400; ++round) {
    const size_t n = 1 + rng() % 40;
    const int32_t n_groups = 1 + (int32_t)(rng() % 8);
    std::vector<int32_t> grp(n);
    std::vector<BlockEntry> e(n);
    std::vector<Res> all;
    const size_t n_table = rng() % 4 == 0 ? n / 2 : n;  // rows beyond the array are ungrouped
    for (size_t i = 0; i < n; ++i) {
      grp[i] = rng() % 4 == 0 ? -1 - (int32_t)(rng() % 3) : (int32_t)(rng() % (uint32_t)n_groups);
      const double d = ladder[rng() % (uint32_t)nl];
      e[i] = BlockEntry{(int64_t)(i * 3 + 1), -d, 0.0};  // inner product: distance = -s0 exactly (-(-0.0) = +0.0, NaN stays NaN)
    }
    std::shuffle(e.begin(), e.end(), rng);
    const GroupTable table{grp.data(), (int64_t)n_table};
    // (ids are 3 i + 1: most lie beyond a table of n entries -- ungrouped --, the rest hit it)
    for (size_t i = 0; i < n; ++i) all.push_back({e[i].id, -e[i].s0, table.at(e[i].id)});
    const EntryList lists[2] = {{e.data(), (uint32_t)(n / 2)}, {e.data() + n / 2, (uint32_t)(n - n / 2)}};
    for (int t = -1; t < nl; ++t)
      for (size_t k : {(size_t)0, (size_t)1, (size_t)3, n, n + 2}) {
        const double T = t < 0 ? nan : ladder[t];
        std::vector<int64_t> ids(k + 1);
        std::vector<double> dist(k + 1);
        std::vector<int32_t> og(k + 1);
        const int32_t cnt = finalize_grouped(1, 4, nullptr, (int32_t)k, T, lists, 2, table, ids.data(), dist.data(), og.data());
        char tag[96];
        snprintf(tag, sizeof tag, "(b) round %d T %g k %zu", round, T, k);
        const std::vector<Res> want = spec_grouped(all, T, k);
        same(tag, want, ids.data(), dist.data(), og.data(), cnt);
        for (size_t i = want.size(); i < k; ++i)
          if (!(ids[i] == -1 && dist[i] != dist[i] && og[i] == -1) && fails++ < 10) printf("%s: unused slot %zu is not (-1, NaN, -1)\n", tag, i);
      }
  }
  // the ids of the small table: a direct case where ids index the table, so that grouped rows tie and the id decides the head
  {
    const int32_t grp[6] = {0, 0, 1, 1, -1, -1};
    const GroupTable table{grp, 6};
    const BlockEntry e[6] = {{1, -1.0, 0}, {0, -1.0, 0}, {3, -0.0, 0}, {2, 0.0, 0}, {5, -1.0, 0}, {4, -1.0, 0}};
    const EntryList l[1] = {{e, 6}};
    int64_t ids[6];
    double dist[6];
    int32_t og[6];
    const int32_t cnt = finalize_grouped(1, 4, nullptr, 6, nan, l, 1, table, ids, dist, og);
    // distances: rows 0, 1, 4, 5 at 1.0; row 2 at -0.0 (s0 = +0.0), row 3 at +0.0: L = 2, 3, 0, 1, 4, 5 -> G = 2, 0, 4, 5
    const std::vector<Res> want = {{2, -0.0, 1}, {0, 1.0, 0}, {4, 1.0, -1}, {5, 1.0, -1}};
    same("(b) ties by id", want, ids, dist, og, cnt);
  }
}

// ---- (c) ----------------------------------------------------------------------------------------------------------------
static void part_c() {
  std::mt19937_64 rng(9);
  for (int round = 0; round < 600; ++round) {
    const size_t n = 1 + rng() % 120;
    const int ranks = 1 + (int)(rng() % 5);
    const int32_t n_groups = 1 + (int32_t)(rng() % 25);
    std::vector<Res> all;
    for (size_t i = 0; i < n; ++i)
      all.push_back({(int64_t)i, (double)(rng() % 12) * 0.25 - 1.0, rng() % 5 == 0 ? -1 : (int32_t)(rng() % (uint32_t)n_groups)});
    std::vector<std::vector<Res>> part((size_t)ranks);
    const bool ranges = round & 1;  // row ranges, as the shards are cut, or any split at all
    for (size_t i = 0; i < n; ++i) part[ranges ? i * (size_t)ranks / n : rng() % (size_t)ranks].push_back(all[i]);
    for (size_t k : {(size_t)1, (size_t)4, (size_t)17, n}) {
      std::vector<Res> cat;
      for (auto &p : part) {
        const std::vector<Res> mine = spec_grouped(p, std::nan(""), k);
        cat.insert(cat.end(), mine.begin(), mine.end());
      }
      const std::vector<Res> merged = spec_grouped(cat, std::nan(""), k), want = spec_grouped(all, std::nan(""), k);
      ++checks;
      bool ok = merged.size() == want.size();
      for (size_t i = 0; ok && i < want.size(); ++i) ok = merged[i].id == want[i].id && bits(merged[i].d) == bits(want[i].d);
      if (!ok && fails++ < 10) printf("(c) round %d k %zu: the merge of %d ranks' answers is not the global answer\n", round, k, ranks);
    }
  }
}

int main() {
  // the head word orders by key first, then by position; band_of is monotone and never below its argument
  {
    if (!(group_head_word(5, 9) < group_head_word(6, 0) && group_head_word(5, 3) < group_head_word(5, 4))) {
      printf("group_head_word does not order by (key, position)\n");
      ++fails;
    }
    uint32_t prev = 0;
    for (float f : {-3.0e38f, -1.5f, -1e-30f, -0.f, 0.f, 1e-40f, 1e-30f, 0.5f, 1536.f, 3.0e38f, INFINITY}) {
      const uint32_t key = group_f2key(f), b = group_band_of(key, 3e-6f, 1e-20f);
      if (b < key || b < prev) {
        printf("group_band_of(%g) is below its argument or not monotone\n", f);
        ++fails;
      }
      prev = b;
    }
    if (group_band_of(GROUP_KEY_NAN, 1e-6f, 0.f) != GROUP_KEY_NAN || group_valid(-1, 4) || group_valid(4, 4) || !group_valid(3, 4)) {
      printf("group_band_of(NaN key) / group_valid\n");
      ++fails;
    }
  }
  part_a();
  part_b();
  part_c();
  printf("%ld checks, %ld heads taken, %ld side rows, %d failures\n", checks, n_heads_taken, n_side, fails);
  if (fails) return 1;
  if (n_side == 0 || n_heads_taken == 0) {
    printf("the side predicate or the select never took a row\n");
    return 1;
  }
  printf("group rule ok\n");
  return 0;
}
