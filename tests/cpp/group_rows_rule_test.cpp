// Host-only check of tostore_amd/csrc/tsh_group_rows_rule.h, the rules of a grouped search with several rows per group,
// in four parts.
// (a) A software model of the job: exact sums per row, the f32 key of every row pushed to EITHER end of the per-key bound
//     the error model claims and rounded inwards, dead rows, six group layouts -- through the head table, the heads, a
//     bound tau with at least k heads at or below it (the k-th smallest tile minimum of heads, the exact k-th head key, or
//     none), and then through the rule header exactly as the kernels apply it: the marked groups and their slot words,
//     the segments, the radix select for tau_g, the members.  Shown on every instance: the marked groups contain every
//     winning group; the members (with the select's candidates) contain every row of the answer; finalize_grouped_rows
//     over them equals a brute-force answer over ALL live rows written from the specification.
// (b) The finaliser's step against the specification written a second time, over any superset of candidates, a row
//     twice among them: m = 1, m at or above the largest group, ties, ungrouped rows, -0.0 / +0.0, NaN, thresholds.
// (c) The radix select against std::nth_element.
// (d) The counter-example: a group spanning two shards breaks the per-shard rule, which is why exact-all exists.
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

#include "../../tostore_amd/csrc/tsh_group_rows_rule.h"

using namespace tsh;

static int fails = 0;
static long checks = 0, n_marked = 0, n_members = 0, n_unmarked = 0, n_not_member = 0;

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
struct Answer {
  std::vector<int32_t> group;          // per winning group
  std::vector<std::vector<Res>> rows;  // its rows, in L's order
};
// The specification, a second time.  L: the rows the threshold keeps (dropped iff d > T, a NaN T drops nothing) in
// (compareTo, id) order.  The winners: the groups of the first k entries of "L without entries whose group occurred
// earlier".  Of each, the first m entries of L that belong to it.
static Answer spec_rows(std::vector<Res> rows, double T, size_t k, size_t m) {
  std::vector<Res> L;
  for (const Res &r : rows)
    if (T != T || !(r.d > T)) L.push_back(r);
  std::sort(L.begin(), L.end(), [](const Res &a, const Res &b) {
    const int c = dart_compare(a.d, b.d);
    return c != 0 ? c < 0 : a.id < b.id;
  });
  Answer A;
  std::vector<int64_t> first_id;  // what tells two ungrouped winners apart
  std::set<int32_t> seen;
  for (const Res &r : L) {
    if (A.group.size() >= k) break;
    if (r.g >= 0 && !seen.insert(r.g).second) continue;
    A.group.push_back(r.g);
    first_id.push_back(r.id);
  }
  A.rows.resize(A.group.size());
  for (size_t w = 0; w < A.group.size(); ++w)
    for (const Res &r : L) {
      if (A.rows[w].size() >= m) break;
      if (A.group[w] >= 0 ? r.g == A.group[w] : r.id == first_id[w]) A.rows[w].push_back(r);
    }
  return A;
}
static bool same(const char *what, const Answer &want, size_t k, size_t m, const int64_t *ids, const double *dist, const int32_t *grp,
                 const int32_t *rows, int32_t cnt) {
  ++checks;
  bool ok = (size_t)cnt == want.group.size();
  for (size_t w = 0; ok && w < k; ++w) {
    const size_t have = w < want.group.size() ? want.rows[w].size() : 0;
    ok = grp[w] == (w < want.group.size() ? want.group[w] : -1) && (size_t)rows[w] == have;
    for (size_t j = 0; ok && j < m; ++j) {
      const int64_t id = ids[w * m + j];
      const double d = dist[w * m + j];
      if (j < have) ok = id == want.rows[w][j].id && (bits(d) == bits(want.rows[w][j].d) || (d != d && want.rows[w][j].d != want.rows[w][j].d));
      else ok = id == -1 && d != d;
    }
  }
  if (!ok && fails++ < 10) {
    printf("%s: got %d groups, want %zu\n", what, cnt, want.group.size());
    for (size_t w = 0; w < k && w < 6; ++w) {
      printf("  [%zu] group %d rows %d:", w, grp[w], rows[w]);
      for (size_t j = 0; j < m && j < 6; ++j) printf(" (%lld, %.17g)", (long long)ids[w * m + j], dist[w * m + j]);
      printf("  want group %d:", w < want.group.size() ? want.group[w] : -9);
      for (size_t j = 0; w < want.group.size() && j < want.rows[w].size() && j < 6; ++j)
        printf(" (%lld, %.17g)", (long long)want.rows[w][j].id, want.rows[w][j].d);
      printf("\n");
    }
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
  *n_groups = std::max<int32_t>((int32_t)n + 1, 8);
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
      auto group_at = [&](size_t i) { return table.at((int64_t)i); };
      // G1 and G2
      std::vector<uint64_t> gm0((size_t)n_groups, GROUP_WORD_NONE);
      for (size_t i = 0; i < n; ++i) {
        const int32_t g = group_at(i);
        if (keys[i] == GROUP_KEY_DEAD || !group_valid(g, n_groups)) continue;
        gm0[(size_t)g] = std::min(gm0[(size_t)g], group_head_word(keys[i], (uint32_t)i));
      }
      std::vector<uint32_t> heads(n_tiles * 64, GROUP_KEY_DEAD), hmin(n_tiles, GROUP_KEY_DEAD);
      for (size_t i = 0; i < n; ++i) {
        if (keys[i] == GROUP_KEY_DEAD) continue;
        const int32_t g = group_at(i);
        const bool grouped = group_valid(g, n_groups);
        if (group_is_head(grouped, group_head_word(keys[i], (uint32_t)i), grouped ? gm0[(size_t)g] : 0)) heads[i] = keys[i];
        hmin[i / 64] = std::min(hmin[i / 64], heads[i]);
      }
      std::vector<Res> all;
      for (size_t i = 0; i < n; ++i)
        if (rows[i].live) all.push_back({(int64_t)i, rows[i].dist, group_at(i)});
      const size_t n_distinct = spec_rows(all, std::nan(""), n + 1, 1).group.size();
      size_t largest = 1;
      {
        std::map<int32_t, size_t> sz;
        for (const Res &r : all)
          if (r.g >= 0) largest = std::max(largest, ++sz[r.g]);
      }
      for (size_t k : {(size_t)1, (size_t)10, n_distinct + 5})
        for (size_t m : {(size_t)1, (size_t)2, (size_t)3, std::min<size_t>(largest + 1, (size_t)GROUP_ROWS_MAX)}) {
          std::vector<uint32_t> sorted_hmin(hmin), sorted_heads(heads);
          std::sort(sorted_hmin.begin(), sorted_hmin.end());
          std::sort(sorted_heads.begin(), sorted_heads.end());
          const uint32_t taus[3] = {k <= n_tiles && sorted_hmin[k - 1] != GROUP_KEY_DEAD ? sorted_hmin[k - 1] : GROUP_KEY_NAN,
                                    k <= sorted_heads.size() && sorted_heads[k - 1] != GROUP_KEY_DEAD ? sorted_heads[k - 1] : GROUP_KEY_NAN, GROUP_KEY_NAN};
          for (uint32_t tau : taus) {
            const uint32_t band = group_band_of(tau, eps_rel, delta_abs);
            std::vector<uint64_t> gm(gm0);
            // the select: the heads at or below the band
            std::vector<BlockEntry> cand, side;
            for (size_t i = 0; i < n; ++i)
              if (heads[i] != GROUP_KEY_DEAD && heads[i] <= band) cand.push_back(rows[i].e);
            // R1: the marked groups get slots (capacity: every group, the overflow route is the host's)
            const uint32_t slot_cap = (uint32_t)n_groups;
            uint32_t slots = 0;
            for (size_t i = 0; i < n; ++i) {
              const bool grouped_head = keys[i] != GROUP_KEY_DEAD && group_valid(group_at(i), n_groups) && heads[i] != GROUP_KEY_DEAD;
              if (!group_rows_marked(grouped_head, keys[i], band)) continue;
              gm[(size_t)group_at(i)] = group_slot_word(slots++);
            }
            n_marked += slots;
            // R2 - R4: the segments
            std::vector<std::vector<uint64_t>> seg(slots);
            for (size_t i = 0; i < n; ++i) {
              const int32_t g = group_at(i);
              if (keys[i] == GROUP_KEY_DEAD || !group_valid(g, n_groups)) continue;
              if (!group_word_is_slot(gm[(size_t)g], slot_cap)) {
                ++n_unmarked;
                continue;
              }
              seg[group_word_slot(gm[(size_t)g])].push_back(group_head_word(keys[i], (uint32_t)i));
            }
            // R5: the pick
            std::set<int64_t> member;
            for (auto &sg : seg) {
              std::shuffle(sg.begin(), sg.end(), rng);  // (segments fill in any order)
              uint32_t tb = GROUP_KEY_NAN;
              if (!group_rows_takes_all((uint32_t)sg.size(), (uint32_t)m)) {
                std::vector<uint32_t> ks;
                for (uint64_t w : sg) ks.push_back(group_word_key(w));
                tb = group_band_of(group_rows_mth_key(ks.data(), ks.size(), (uint32_t)m), eps_rel, delta_abs);
              }
              for (uint64_t w : sg) {
                if (!group_rows_takes_all((uint32_t)sg.size(), (uint32_t)m) && !group_rows_member(group_word_key(w), tb)) {
                  ++n_not_member;
                  continue;
                }
                side.push_back(rows[(uint32_t)w].e);
                member.insert((int64_t)(uint32_t)w);
                ++n_members;
              }
            }
            const Answer free_ans = spec_rows(all, std::nan(""), k, m);
            // the two claims, on their own: every winning group is marked; every row of the answer is a member (grouped)
            // or a candidate of the select (ungrouped)
            for (size_t w = 0; w < free_ans.group.size(); ++w) {
              ++checks;
              const int32_t g = free_ans.group[w];
              if (g >= 0 && !group_word_is_slot(gm[(size_t)g], slot_cap) && fails++ < 10)
                printf("(a) %s layout %d keys %d k %zu m %zu tau %08x: winning group %d is not marked\n", what, kind, key_mode, k, m, tau, g);
              for (const Res &r : free_ans.rows[w])
                if (g >= 0 && !member.count(r.id) && fails++ < 10)
                  printf("(a) %s layout %d keys %d k %zu m %zu tau %08x: row %lld of group %d is no member\n", what, kind, key_mode, k, m, tau,
                         (long long)r.id, g);
            }
            const EntryList lists[2] = {{cand.data(), (uint32_t)cand.size()}, {side.data(), (uint32_t)side.size()}};
            std::vector<double> thrs = {std::nan("")};
            if (!free_ans.group.empty()) {  // thresholds that cut inside the winning groups
              const double d0 = free_ans.rows.back().front().d, d1 = free_ans.rows.front().back().d;
              for (double d : {d0, d1}) {
                thrs.push_back(d);
                thrs.push_back(std::nextafter(d, -INFINITY));
                thrs.push_back(std::nextafter(d, INFINITY));
              }
            }
            for (double T : thrs) {
              std::vector<int64_t> ids(k * m);
              std::vector<double> dist(k * m);
              std::vector<int32_t> og(k), orows(k);
              const int32_t cnt = finalize_grouped_rows(metric, dim, query, (int32_t)k, (int32_t)m, T, lists, 2, table, ids.data(), dist.data(),
                                                        og.data(), orows.data());
              char tag[200];
              snprintf(tag, sizeof tag, "(a) %s layout %d keys %d k %zu m %zu tau %08x T %.17g", what, kind, key_mode, k, m, tau, T);
              same(tag, spec_rows(all, T, k, m), k, m, ids.data(), dist.data(), og.data(), orows.data(), cnt);
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
  for (size_t n : {(size_t)1, (size_t)65, (size_t)300}) {
    for (int dim : {4, 768}) {
      const int nch = ((dim + 3) / 4 + 63) / 64;
      {  // L2: sums given directly, crowds a few key-bounds apart and exact ties
        const double eps = (4.0 * nch + 8.0) * u2;
        const float eps_rel = (float)(3.0 * eps), delta_abs = (float)((double)dim * 7.9e-31);
        std::vector<Row> rows;
        for (size_t i = 0; i < n; ++i) {
          double s;
          const int kind = (int)(rng() % 6);
          if (kind == 0) s = 1536.0;                                                           // exact ties
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
            if (kind == 0) v[j] = prev[j];                                       // a duplicate: exact ties
            else if (kind == 1) v[j] = (float)(prev[j] * 2.0);                   // parallel to it
            else if (kind == 2) v[j] = (float)(q[j] * sc + G(rng) * sc * 1e-6);  // nearly parallel to the query
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
    std::vector<int32_t> grp(3 * n + 2);
    std::vector<BlockEntry> e(n);
    std::vector<Res> all;
    const size_t n_table = rng() % 4 == 0 ? n : 3 * n + 2;  // rows beyond the array are ungrouped
    for (size_t i = 0; i < grp.size(); ++i) grp[i] = rng() % 4 == 0 ? -1 - (int32_t)(rng() % 3) : (int32_t)(rng() % (uint32_t)n_groups);
    for (size_t i = 0; i < n; ++i) {
      const double d = ladder[rng() % (uint32_t)nl];
      e[i] = BlockEntry{(int64_t)(i * 3 + 1), -d, 0.0};  // inner product: distance = -s0 exactly
    }
    std::shuffle(e.begin(), e.end(), rng);
    const GroupTable table{grp.data(), (int64_t)n_table};
    size_t largest = 1;
    std::map<int32_t, size_t> sz;
    for (size_t i = 0; i < n; ++i) {
      all.push_back({e[i].id, -e[i].s0, table.at(e[i].id)});
      if (all.back().g >= 0) largest = std::max(largest, ++sz[all.back().g]);
    }
    // the candidates: every row, some of them twice (a marked head is a member and a candidate of the select)
    std::vector<BlockEntry> twice(e);
    for (size_t i = 0; i < n; ++i)
      if (rng() % 3 == 0) twice.push_back(e[i]);
    const size_t h = twice.size() / 2;
    const EntryList lists[2] = {{twice.data(), (uint32_t)h}, {twice.data() + h, (uint32_t)(twice.size() - h)}};
    for (int t = -1; t < nl; ++t)
      for (size_t k : {(size_t)0, (size_t)1, (size_t)3, n, n + 2})
        for (size_t m : {(size_t)1, (size_t)2, largest, largest + 3}) {
          const double T = t < 0 ? nan : ladder[t];
          std::vector<int64_t> ids(k * m + 1);
          std::vector<double> dist(k * m + 1);
          std::vector<int32_t> og(k + 1), orows(k + 1);
          const int32_t cnt = finalize_grouped_rows(1, 4, nullptr, (int32_t)k, (int32_t)m, T, lists, 2, table, ids.data(), dist.data(), og.data(),
                                                    orows.data());
          char tag[96];
          snprintf(tag, sizeof tag, "(b) round %d T %g k %zu m %zu", round, T, k, m);
          same(tag, spec_rows(all, T, k, m), k, m, ids.data(), dist.data(), og.data(), orows.data(), cnt);
        }
  }
  // a direct case: ties decided by id, -0.0 before +0.0, an ungrouped row between the groups
  {
    const int32_t grp[7] = {0, 0, 1, 1, -1, 0, 1};
    const GroupTable table{grp, 7};
    const BlockEntry e[7] = {{1, -1.0, 0}, {0, -1.0, 0}, {3, -0.0, 0}, {2, 0.0, 0}, {4, -0.5, 0}, {5, -1.0, 0}, {6, -7.0, 0}};
    const EntryList l[1] = {{e, 7}};
    int64_t ids[6];
    double dist[6];
    int32_t og[3], orows[3];
    const int32_t cnt = finalize_grouped_rows(1, 4, nullptr, 3, 2, nan, l, 1, table, ids, dist, og, orows);
    // distances: row 2 at -0.0, row 3 at +0.0, row 4 at 0.5, rows 0, 1, 5 at 1.0, row 6 at 7.0
    // L = 2, 3, 4, 0, 1, 5, 6: winners 1 (rows 2, 3), ungrouped 4, 0 (rows 0, 1)
    Answer want;
    want.group = {1, -1, 0};
    want.rows = {{{2, -0.0, 1}, {3, 0.0, 1}}, {{4, 0.5, -1}}, {{0, 1.0, 0}, {1, 1.0, 0}}};
    same("(b) ties by id", want, 3, 2, ids, dist, og, orows, cnt);
  }
}

// ---- (c) ----------------------------------------------------------------------------------------------------------------
static void part_c() {
  std::mt19937_64 rng(11);
  for (int round = 0; round < 2000; ++round) {
    const size_t n = 1 + rng() % 300;
    std::vector<uint32_t> keys(n);
    const int kind = (int)(rng() % 4);
    for (auto &x : keys)
      x = kind == 0 ? (uint32_t)rng() : kind == 1 ? 0x80000000u + (uint32_t)(rng() % 5) : kind == 2 ? (uint32_t)(rng() % 3) << 24 | (uint32_t)(rng() % 4) : 0xFFFFFFFEu - (uint32_t)(rng() % 2);
    for (uint32_t m : {1u, std::min(2u, (uint32_t)n), (uint32_t)n, (uint32_t)(1 + rng() % n)}) {  // (1 <= m <= n: the pick's own condition)
      std::vector<uint32_t> s(keys);
      std::sort(s.begin(), s.end());
      ++checks;
      const uint32_t got = group_rows_mth_key(keys.data(), n, m);
      if (got != s[m - 1] && fails++ < 10) printf("(c) round %d n %zu m %u: radix select %08x, sorted %08x\n", round, n, m, got, s[m - 1]);
    }
  }
}

// ---- (d) ----------------------------------------------------------------------------------------------------------------
// Two shards.  Group 0 has its best row on shard A and its second-best on shard B, where it is that shard's WORST head;
// shard B holds k other groups that are far nearer.  On shard B the bound tau names its k nearest heads, group 0's head
// lies far above band_of(tau), so group 0 is not marked there and its second row is no candidate: the per-shard rule
// returns one row for the winning group 0 where the specification has two.
static void part_d() {
  const float eps_rel = 3e-6f, delta_abs = 1e-20f;
  struct R {
    int64_t id;
    double s;
    int32_t g;
    int shard;
  };
  const R rows[] = {{0, 1.0, 0, 0}, {1, 50.0, 1, 0}, {2, 4.0, 2, 1}, {3, 9.0, 3, 1}, {4, 900.0, 0, 1}};
  const int32_t grp[5] = {0, 1, 2, 3, 0};
  const GroupTable table{grp, 5};
  const size_t k = 2, m = 2;
  std::vector<Res> all;
  std::vector<BlockEntry> cands;
  bool marked_on_b = false;
  for (int shard = 0; shard < 2; ++shard) {
    std::map<int32_t, uint32_t> head;  // the shard's heads: one row per group here
    for (const R &r : rows)
      if (r.shard == shard) {
        const uint32_t key = group_f2key((float)r.s);
        if (!head.count(r.g) || key < head[r.g]) head[r.g] = key;
      }
    std::vector<uint32_t> hk;
    for (auto &h : head) hk.push_back(h.second);
    std::sort(hk.begin(), hk.end());
    const uint32_t band = group_band_of(hk[std::min(k, hk.size()) - 1], eps_rel, delta_abs);
    for (const R &r : rows) {
      if (r.shard != shard) continue;
      const bool marked = group_rows_marked(true, head[r.g], band);
      if (shard == 1 && r.g == 0) marked_on_b = marked;
      if (marked) cands.push_back(BlockEntry{r.id, r.s, 0.0});  // (a marked group's rows, all of them: fewer than m)
    }
  }
  for (const R &r : rows) all.push_back({r.id, std::sqrt(r.s), r.g});
  const Answer want = spec_rows(all, std::nan(""), k, m);
  const EntryList l[1] = {{cands.data(), (uint32_t)cands.size()}};
  int64_t ids[4];
  double dist[4];
  int32_t og[2], orows[2];
  finalize_grouped_rows(0, 4, nullptr, (int32_t)k, (int32_t)m, std::nan(""), l, 1, table, ids, dist, og, orows);
  ++checks;
  const bool broken = !marked_on_b && want.group[0] == 0 && want.rows[0].size() == 2 && want.rows[0][1].id == 4 && og[0] == 0 && orows[0] == 1;
  if (!broken) {
    printf("(d) the spanning group did not break the per-shard rule as claimed (marked on B %d, rows %d)\n", (int)marked_on_b, orows[0]);
    ++fails;
  }
  // ... and the exact-all route, every row a candidate, has it right
  std::vector<BlockEntry> every;
  for (const R &r : rows) every.push_back(BlockEntry{r.id, r.s, 0.0});
  const EntryList le[1] = {{every.data(), (uint32_t)every.size()}};
  const int32_t cnt = finalize_grouped_rows(0, 4, nullptr, (int32_t)k, (int32_t)m, std::nan(""), le, 1, table, ids, dist, og, orows);
  same("(d) exact-all", want, k, m, ids, dist, og, orows, cnt);
}

int main() {
  {  // the slot words: no head word and not the empty word look like one
    bool ok = group_word_is_slot(group_slot_word(0), 1) && group_word_is_slot(group_slot_word(73), 74) && !group_word_is_slot(group_slot_word(74), 74) &&
              !group_word_is_slot(GROUP_WORD_NONE, 0x7FFFFFFFu) && !group_word_is_slot(group_head_word(GROUP_KEY_NAN, 5), 64) &&
              group_word_slot(group_slot_word(12345)) == 12345u && !group_word_is_slot(group_head_word(0, 0), 64);
    ok = ok && group_rows_marked(true, 5, 5) && !group_rows_marked(true, 6, 5) && !group_rows_marked(false, 1, 5) && group_rows_marked(true, 7, GROUP_KEY_NAN);
    ok = ok && group_rows_takes_all(3, 3) && !group_rows_takes_all(4, 3) && group_rows_slots(5) == 74 && group_rows_slots(100) == 264;
    if (!ok) {
      printf("slot words / marked / takes_all / slots\n");
      ++fails;
    }
  }
  part_a();
  part_b();
  part_c();
  part_d();
  printf("%ld checks, %ld marked groups, %ld members, %ld rows of unmarked groups, %ld rows above their group's band, %d failures\n", checks, n_marked,
         n_members, n_unmarked, n_not_member, fails);
  if (fails) return 1;
  if (n_marked == 0 || n_members == 0 || n_unmarked == 0 || n_not_member == 0) {
    printf("the mark or the pick never took, or never left, a row\n");
    return 1;
  }
  printf("group rows rule ok\n");
  return 0;
}
