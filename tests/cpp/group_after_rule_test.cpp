// Host-only check of tostore_amd/csrc/tsh_group_after_rule.h, the rules of a grouped cursor search and of a group count.
// A software model of the scan as in group_rule_test.cpp: exact sums per row, the f32 key of every row pushed to EITHER end
// of the per-key bound the error model claims and rounded inwards, three metrics, dead rows, six group layouts.  The head
// table is built over all live rows; heads and rows are classified by the rule header's predicates exactly as the kernels
// apply them (tiles of 64; tau = the k-th smallest tile minimum of the floored heads, or the exact k-th floored head key, or
// no bound); the candidates go through finalize_grouped_after resp. group_count_entries.  Against a brute-force "G after
// the cursor" over ALL live rows, written from the specification, for cursors on existing rows, beside them, midway
// between entries, -inf, -0.0 / +0.0, on ties and beyond every row:
//   (1) the page for k in {1, 10, all} is brute force's;
//   (2) the certain count plus the group-count step is brute force's count, with and without a threshold;
//   (3) a group classified BEFORE is consumed and one classified AFTER is not (so no consumed group ever yields a
//       candidate from the "certainly before" case, and no group is lost to it);
//   (4) pages, each started from the last entry of the page before, concatenate to G.
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

#include "../../tostore_amd/csrc/tsh_group_after_rule.h"

using namespace tsh;

static int fails = 0;
static long checks = 0, n_side = 0, n_heads_taken = 0, n_before = 0, n_ambiguous = 0, n_count_in = 0, n_count_side = 0;

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
struct Cur {
  double d;
  int64_t id;
};
static bool follows(const Cur &c, const Res &r) {
  if (c.d == -INFINITY) return true;
  const int x = dart_compare(r.d, c.d);
  return x != 0 ? x > 0 : r.id > c.id;
}
// the specification: L (dropped iff d > T, a NaN T drops nothing) in (compareTo, id) order, the first entry of each group
static std::vector<Res> spec_G(std::vector<Res> rows, double T) {
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
    if (r.g >= 0 && !seen.insert(r.g).second) continue;
    G.push_back(r);
  }
  return G;
}
static std::vector<Res> spec_after(const std::vector<Res> &G, const Cur &c, size_t k) {
  std::vector<Res> out;
  for (const Res &r : G)
    if (out.size() < k && follows(c, r)) out.push_back(r);
  return out;
}
static bool same(const char *what, const std::vector<Res> &want, const int64_t *ids, const double *dist, const int32_t *grp, int32_t cnt) {
  ++checks;
  bool ok = (size_t)cnt == want.size();
  for (size_t i = 0; ok && i < want.size(); ++i)
    ok = ids[i] == want[i].id && (bits(dist[i]) == bits(want[i].d) || (dist[i] != dist[i] && want[i].d != want[i].d)) && grp[i] == want[i].g;
  if (!ok && fails++ < 10) {
    printf("%s: got %d entries, want %zu\n", what, cnt, want.size());
    for (size_t i = 0; i < std::max<size_t>(want.size(), (size_t)std::max(cnt, 0)) && i < 8; ++i)
      printf("  [%zu] got (%lld, %.17g, %d) want (%lld, %.17g, %d)\n", i, i < (size_t)cnt ? (long long)ids[i] : -9LL, i < (size_t)cnt ? dist[i] : 0.0,
             i < (size_t)cnt ? grp[i] : -9, i < want.size() ? (long long)want[i].id : -9LL, i < want.size() ? want[i].d : 0.0, i < want.size() ? want[i].g : -9);
  }
  return ok;
}

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
      case 0: g[i] = (int32_t)(i / 7); break;
      case 1: g[i] = (int32_t)(rng() % std::max<size_t>(n / 5, 1)); break;
      case 2: g[i] = 3; break;
      case 3: g[i] = -1; break;
      case 4: g[i] = (int32_t)i; break;
      default: g[i] = rng() % 3 == 0 ? -(int32_t)(rng() % 5) - 1 : (int32_t)(rng() % std::max<size_t>(n / 9, 1)); break;
    }
  }
  return g;
}

// one data set under one layout and one choice of keys: everything the passes read
struct Model {
  int metric, dim;
  const float *query;
  float eps_rel, delta_abs;
  double mag_a;
  const std::vector<Row> *rows;
  GroupTable table;
  int32_t n_groups;
  std::vector<uint32_t> keys;
  std::vector<uint64_t> gm;
  size_t n, n_tiles;
  int32_t group_at(size_t i) const { return table.at((int64_t)i); }
  bool is_head(size_t i) const {
    const int32_t g = group_at(i);
    const bool grouped = group_valid(g, n_groups);
    return group_is_head(grouped, group_head_word(keys[i], (uint32_t)i), grouped ? gm[(size_t)g] : 0);
  }
  uint32_t head_key(size_t i) const {
    const int32_t g = group_at(i);
    return group_valid(g, n_groups) ? group_word_key(gm[(size_t)g]) : keys[i];
  }
};

// a page as the device and the finaliser compute it.  tau_mode: 0 the k-th smallest tile minimum of the floored heads, 1 the
// exact k-th floored head key, 2 no bound
static int32_t model_page(const Model &m, const Cur &cur, size_t k, int tau_mode, double T, int64_t *ids, double *dist, int32_t *og) {
  const AfterFloor f = after_floor(m.metric, m.dim, m.eps_rel, m.delta_abs, m.mag_a, cur.d);
  std::vector<uint32_t> heads(m.n_tiles * 64, GROUP_KEY_DEAD), hmin(m.n_tiles, GROUP_KEY_DEAD);
  std::vector<BlockEntry> cand, side;
  for (size_t i = 0; i < m.n; ++i) {  // G2a
    if (m.keys[i] == GROUP_KEY_DEAD || !m.is_head(i)) continue;
    const int cls = group_after_class(m.keys[i], f.lo, f.hi);
    if (cls == GROUP_AFTER) heads[i] = m.keys[i];
    else if (cls == GROUP_AMBIGUOUS) {
      side.push_back((*m.rows)[i].e);
      ++n_ambiguous;
    } else {
      ++n_before;
    }
    hmin[i / 64] = std::min(hmin[i / 64], heads[i]);
  }
  uint32_t tau = GROUP_KEY_NAN;
  if (tau_mode == 0) {
    std::vector<uint32_t> s(hmin);
    std::sort(s.begin(), s.end());
    if (k <= s.size() && s[k - 1] != GROUP_KEY_DEAD) tau = s[k - 1];
  } else if (tau_mode == 1) {
    std::vector<uint32_t> s(heads);
    std::sort(s.begin(), s.end());
    if (k <= s.size() && s[k - 1] != GROUP_KEY_DEAD) tau = s[k - 1];
  }
  const uint32_t band = group_band_of(tau, m.eps_rel, m.delta_abs);
  for (size_t i = 0; i < m.n; ++i) {
    if (m.keys[i] == GROUP_KEY_DEAD) continue;
    if (m.is_head(i)) {
      if (heads[i] != GROUP_KEY_DEAD && heads[i] <= band) {  // the select
        cand.push_back((*m.rows)[i].e);
        ++n_heads_taken;
      }
      continue;
    }
    const uint32_t hk = m.head_key(i);  // G3a
    if (group_after_side(group_after_class(hk, f.lo, f.hi), m.keys[i], group_band_of(hk, m.eps_rel, m.delta_abs), band)) {
      side.push_back((*m.rows)[i].e);
      ++n_side;
    }
  }
  const EntryList lists[2] = {{cand.data(), (uint32_t)cand.size()}, {side.data(), (uint32_t)side.size()}};
  Cursor c;
  c.dist = cur.d;
  c.id = cur.id;
  return finalize_grouped_after(m.metric, m.dim, m.query, (int32_t)k, T, lists, 2, m.table, c, ids, dist, og);
}

// a count as the device and the finaliser compute it
static int64_t model_count(const Model &m, bool has_cursor, const Cur &cur, double T) {
  const CountWindow w = count_window(m.metric, m.dim, m.eps_rel, m.delta_abs, m.mag_a, has_cursor, cur.d, T);
  if (w.skip) return 0;
  int64_t certain = 0;
  std::vector<BlockEntry> side;
  for (size_t i = 0; i < m.n; ++i) {
    if (m.keys[i] == GROUP_KEY_DEAD) continue;
    const bool head = m.is_head(i);
    const uint32_t hk = m.head_key(i);
    const int cls = group_count_class(hk, w.in_lo, w.in_hi, w.out_lo, w.out_hi);
    if (head && cls == 0) {
      ++certain;
      ++n_count_in;
    }
    if (cls == 2 && (head || m.keys[i] <= group_band_of(hk, m.eps_rel, m.delta_abs))) {
      side.push_back((*m.rows)[i].e);
      ++n_count_side;
    }
  }
  const EntryList lists[1] = {{side.data(), (uint32_t)side.size()}};
  Cursor c;
  c.dist = cur.d;
  c.id = cur.id;
  return certain + group_count_entries(m.metric, m.dim, m.query, T, lists, 1, m.table, has_cursor ? &c : nullptr);
}

static void run_model(const char *what, int metric, int dim, const float *query, double mag_a, float eps_rel, float delta_abs, const std::vector<Row> &rows,
                      std::mt19937_64 &rng) {
  const size_t n = rows.size();
  for (int kind = 0; kind < 6; ++kind)
    for (int key_mode = 0; key_mode < 3; ++key_mode) {  // every key at the lower end, the upper end, a random end
      Model m;
      m.metric = metric;
      m.dim = dim;
      m.query = query;
      m.eps_rel = eps_rel;
      m.delta_abs = delta_abs;
      m.mag_a = mag_a;
      m.rows = &rows;
      m.n = n;
      m.n_tiles = (n + 63) / 64;
      const std::vector<int32_t> grp = layout(kind, n, rng, &m.n_groups);
      m.table = GroupTable{grp.data(), (int64_t)(kind == 5 ? n - n / 10 : n)};
      m.keys.assign(m.n_tiles * 64, GROUP_KEY_DEAD);
      for (size_t i = 0; i < n; ++i) {
        if (!rows[i].live) continue;
        float kf;
        const bool upper = key_mode == 1 || (key_mode == 2 && (rng() & 1));
        if (!model_key(rows[i], upper, &kf)) kf = (float)rows[i].val;
        m.keys[i] = group_f2key(kf);
      }
      m.gm.assign((size_t)m.n_groups, GROUP_WORD_NONE);  // G1: over ALL live rows
      for (size_t i = 0; i < n; ++i) {
        const int32_t g = m.group_at(i);
        if (m.keys[i] == GROUP_KEY_DEAD || !group_valid(g, m.n_groups)) continue;
        m.gm[(size_t)g] = std::min(m.gm[(size_t)g], group_head_word(m.keys[i], (uint32_t)i));
      }
      std::vector<Res> all;
      for (size_t i = 0; i < n; ++i)
        if (rows[i].live) all.push_back({(int64_t)i, rows[i].dist, m.group_at(i)});
      const std::vector<Res> G = spec_G(all, std::nan(""));
      // the cursors
      std::vector<Cur> curs = {{-INFINITY, 0}, {-0.0, 0}, {0.0, (int64_t)(n / 2)}, {-0.0, (int64_t)n + 3}};
      for (int c = 0; c < 6 && !all.empty(); ++c) {
        const Res &r = all[rng() % all.size()];  // an existing row (a group's best or not), and beside it
        curs.push_back({r.d, r.id});
        if (c < 2) curs.push_back({r.d, r.id - 1});
        if (c == 2) curs.push_back({r.d, (int64_t)n + 10});
        if (c == 3) curs.push_back({std::nextafter(r.d, INFINITY), -1});
      }
      for (int c = 0; c < 3 && G.size() > 1; ++c) {  // midway between two entries of G
        const size_t i = rng() % (G.size() - 1);
        curs.push_back({G[i].d * 0.5 + G[i + 1].d * 0.5, (int64_t)(rng() % (n + 1))});
      }
      if (!G.empty()) {
        curs.push_back({G.back().d, G.back().id});                           // on the last entry: nothing follows
        curs.push_back({std::fabs(G.back().d) * 2.0 + 1.0, 0});              // beyond every row
        curs.push_back({G.front().d, G.front().id});                         // on the first entry
      }
      // (3): classes against brute force
      for (const Cur &cur : curs) {
        const AfterFloor f = after_floor(metric, dim, eps_rel, delta_abs, mag_a, cur.d);
        std::map<int64_t, bool> best_follows;  // by the id of a group's entry in G
        for (const Res &r : G) best_follows[r.id] = follows(cur, r);
        std::map<int32_t, int64_t> best_of;
        for (const Res &r : G)
          if (r.g >= 0) best_of[r.g] = r.id;
        for (size_t i = 0; i < n; ++i) {
          if (m.keys[i] == GROUP_KEY_DEAD || !m.is_head(i)) continue;
          const int cls = group_after_class(m.keys[i], f.lo, f.hi);
          const int32_t g = m.group_at(i);
          const bool fol = best_follows[g >= 0 ? best_of[g] : (int64_t)i];
          ++checks;
          if (((cls == GROUP_BEFORE && fol) || (cls == GROUP_AFTER && !fol)) && fails++ < 10)
            printf("(3) %s layout %d keys %d cursor (%.17g, %lld): the head at row %zu is classified %d, its group's best %s the cursor\n", what, kind,
                   key_mode, cur.d, (long long)cur.id, i, cls, fol ? "follows" : "does not follow");
        }
      }
      // (1): pages
      for (const Cur &cur : curs)
        for (size_t k : {(size_t)1, (size_t)10, G.size() + 5})
          for (int tau_mode = 0; tau_mode < 3; ++tau_mode) {
            std::vector<double> thrs = {std::nan("")};
            if (tau_mode == 1 && !G.empty()) thrs.push_back(G[G.size() / 2].d);  // a threshold inside the list
            for (double T : thrs) {
              std::vector<int64_t> ids(k);
              std::vector<double> dist(k);
              std::vector<int32_t> og(k);
              const int32_t cnt = model_page(m, cur, k, tau_mode, T, ids.data(), dist.data(), og.data());
              char tag[200];
              snprintf(tag, sizeof tag, "(1) %s layout %d keys %d k %zu tau mode %d T %.17g cursor (%.17g, %lld)", what, kind, key_mode, k, tau_mode, T, cur.d,
                       (long long)cur.id);
              same(tag, spec_after(T != T ? G : spec_G(all, T), cur, k), ids.data(), dist.data(), og.data(), cnt);
            }
          }
      // (2): counts
      for (size_t ci = 0; ci <= curs.size(); ++ci) {
        const bool has_cursor = ci < curs.size();
        const Cur cur = has_cursor ? curs[ci] : Cur{0, 0};
        std::vector<double> thrs = {std::nan("")};
        if (!G.empty()) {
          thrs.push_back(G[G.size() / 2].d);
          thrs.push_back(std::nextafter(G[G.size() / 3].d, -INFINITY));
        }
        for (double T : thrs) {
          const int64_t got = model_count(m, has_cursor, cur, T);
          const int64_t want = (int64_t)spec_after(T != T ? G : spec_G(all, T), has_cursor ? cur : Cur{-INFINITY, 0}, n + 1).size();
          ++checks;
          if (got != want && fails++ < 10)
            printf("(2) %s layout %d keys %d T %.17g cursor %d (%.17g, %lld): count %lld, want %lld\n", what, kind, key_mode, T, (int)has_cursor, cur.d,
                   (long long)cur.id, (long long)got, (long long)want);
        }
      }
      // (4): pages concatenate to G, and the count identity after every page
      for (size_t k : {(size_t)1, (size_t)7}) {
        if (k == 1 && n > 100) continue;
        std::vector<Res> cat;
        Cur cur{-INFINITY, 0};
        const int64_t total = model_count(m, false, cur, std::nan(""));
        for (size_t page = 0; page <= G.size() + 1; ++page) {
          std::vector<int64_t> ids(k);
          std::vector<double> dist(k);
          std::vector<int32_t> og(k);
          const int32_t cnt = model_page(m, cur, k, (int)(page % 3), std::nan(""), ids.data(), dist.data(), og.data());
          for (int32_t i = 0; i < cnt; ++i) cat.push_back({ids[i], dist[i], og[i]});
          if (cnt > 0) {
            cur = Cur{dist[cnt - 1], ids[cnt - 1]};
            ++checks;
            const int64_t left = model_count(m, true, cur, std::nan(""));
            if (left != total - (int64_t)cat.size() && fails++ < 10)
              printf("(4) %s layout %d keys %d k %zu: after %zu entries the count is %lld of %lld\n", what, kind, key_mode, k, cat.size(), (long long)left,
                     (long long)total);
          }
          if ((size_t)cnt < k) break;
        }
        ++checks;
        bool ok = cat.size() == G.size();
        for (size_t i = 0; ok && i < G.size(); ++i) ok = cat[i].id == G[i].id && bits(cat[i].d) == bits(G[i].d) && cat[i].g == G[i].g;
        if (!ok && fails++ < 10) printf("(4) %s layout %d keys %d k %zu: %zu paged entries are not G's %zu\n", what, kind, key_mode, k, cat.size(), G.size());
      }
    }
}

static void part_a() {
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> Gs(0.0, 1.0);
  const double u2 = 1.1920928955078125e-07;
  for (size_t n : {(size_t)1, (size_t)65, (size_t)400}) {
    for (int dim : {4, 768}) {
      const int nch = ((dim + 3) / 4 + 63) / 64;
      {  // L2: sums given directly, crowds a few key-bounds apart and exact ties
        const double eps = (4.0 * nch + 8.0) * u2;
        const float eps_rel = (float)(3.0 * eps), delta_abs = (float)((double)dim * 7.9e-31);
        std::vector<Row> rows;
        for (size_t i = 0; i < n; ++i) {
          double s;
          const int kind = (int)(rng() % 6);
          if (kind == 0) s = 1536.0;
          else if (kind == 1) s = 1536.0 * (1.0 + (double)((int)(rng() % 9) - 4) * eps * 0.5);
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
        run_model("L2", 0, dim, nullptr, 0.0, eps_rel, delta_abs, rows, rng);
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
          else s0 = Gs(rng) * qn * max_norm * 0.5;
          Row r{};
          r.e = BlockEntry{(int64_t)i, s0, 0.0};
          r.dist = -s0;
          r.val = -(long double)s0;
          r.bound = delta;
          r.live = rng() % 8 != 0;
          rows.push_back(r);
        }
        run_model("IP", 1, dim, nullptr, 0.0, 0.f, delta_abs, rows, rng);
      }
      if (dim <= 16) {  // cosine: the finaliser's arithmetic on real vectors
        std::vector<float> q(dim);
        for (auto &x : q) x = (float)Gs(rng);
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
            if (kind == 0) v[j] = prev[j];
            else if (kind == 1) v[j] = (float)(prev[j] * 2.0);
            else if (kind == 2) v[j] = (float)(q[j] * sc + Gs(rng) * sc * 1e-6);
            else v[j] = (float)(Gs(rng) * sc);
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
        run_model("cosine", 2, dim, q.data(), mag_a, 0.f, delta_abs, rows, rng);
      }
    }
  }
}

// the two finaliser steps on their own: -0.0 / +0.0, NaN and infinite distances, ties by id, any cursor, any threshold
static void part_b() {
  std::mt19937_64 rng(13);
  const double nan = std::nan(""), inf = INFINITY;
  const double ladder[] = {-inf, -3.5, -0.0, 0.0, 4.9406564584124654e-324, 1.0, 1.0000000000000002, 2.5, inf, nan};
  const int nl = (int)(sizeof ladder / sizeof *ladder);
  for (int round = 0; round < 300; ++round) {
    const size_t n = 1 + rng() % 40;
    const int32_t n_groups = 1 + (int32_t)(rng() % 8);
    std::vector<int32_t> grp(n * 3 + 2, -1);
    std::vector<BlockEntry> e(n);
    for (size_t i = 0; i < n; ++i) {
      grp[i * 3 + 1] = rng() % 4 == 0 ? -1 - (int32_t)(rng() % 3) : (int32_t)(rng() % (uint32_t)n_groups);
      e[i] = BlockEntry{(int64_t)(i * 3 + 1), -ladder[rng() % (uint32_t)nl], 0.0};  // inner product: distance = -s0 exactly
    }
    std::shuffle(e.begin(), e.end(), rng);
    const GroupTable table{grp.data(), (int64_t)(rng() % 4 == 0 ? grp.size() / 2 : grp.size())};
    std::vector<Res> all;
    for (size_t i = 0; i < n; ++i) all.push_back({e[i].id, -e[i].s0, table.at(e[i].id)});
    const EntryList lists[2] = {{e.data(), (uint32_t)(n / 2)}, {e.data() + n / 2, (uint32_t)(n - n / 2)}};
    for (int t = -1; t < nl; ++t) {
      const double T = t < 0 ? nan : ladder[t];
      const std::vector<Res> G = spec_G(all, T);
      for (int c = 0; c < nl; ++c) {
        const Cur cur{ladder[c], (int64_t)(rng() % (3 * n + 3)) - 1};
        Cursor cc;
        cc.dist = cur.d;
        cc.id = cur.id;
        for (size_t k : {(size_t)0, (size_t)1, (size_t)3, n + 2}) {
          std::vector<int64_t> ids(k + 1);
          std::vector<double> dist(k + 1);
          std::vector<int32_t> og(k + 1);
          const int32_t cnt = finalize_grouped_after(1, 4, nullptr, (int32_t)k, T, lists, 2, table, cc, ids.data(), dist.data(), og.data());
          char tag[128];
          snprintf(tag, sizeof tag, "(b) round %d T %g k %zu cursor (%g, %lld)", round, T, k, cur.d, (long long)cur.id);
          const std::vector<Res> want = spec_after(G, cur, k);
          same(tag, want, ids.data(), dist.data(), og.data(), cnt);
          for (size_t i = want.size(); i < k; ++i)
            if (!(ids[i] == -1 && dist[i] != dist[i] && og[i] == -1) && fails++ < 10) printf("%s: unused slot %zu is not (-1, NaN, -1)\n", tag, i);
          if (cur.d == -inf) {  // from the start: finalize_grouped's answer bit for bit
            std::vector<int64_t> ids2(k + 1);
            std::vector<double> dist2(k + 1);
            std::vector<int32_t> og2(k + 1);
            const int32_t cnt2 = finalize_grouped(1, 4, nullptr, (int32_t)k, T, lists, 2, table, ids2.data(), dist2.data(), og2.data());
            ++checks;
            bool ok = cnt2 == cnt;
            for (size_t i = 0; ok && i < k; ++i) ok = ids[i] == ids2[i] && bits(dist[i]) == bits(dist2[i]) && og[i] == og2[i];
            if (!ok && fails++ < 10) printf("%s: not finalize_grouped's answer\n", tag);
          }
        }
        ++checks;
        const int64_t got = group_count_entries(1, 4, nullptr, T, lists, 2, table, &cc), want = (int64_t)spec_after(G, cur, n + 1).size();
        if (got != want && fails++ < 10) printf("(b) round %d T %g cursor (%g, %lld): group count %lld, want %lld\n", round, T, cur.d, (long long)cur.id, (long long)got, (long long)want);
      }
      ++checks;
      if (group_count_entries(1, 4, nullptr, T, lists, 2, table, nullptr) != (int64_t)G.size() && fails++ < 10)
        printf("(b) round %d T %g: group count without a cursor is not |G|\n", round, T);
    }
  }
}

int main() {
  // the classes: no floor is AFTER; below lo BEFORE; above hi and finite AFTER; everything else AMBIGUOUS
  if (group_after_class(5, 0, 0) != GROUP_AFTER || group_after_class(4, 5, 9) != GROUP_BEFORE || group_after_class(5, 5, 9) != GROUP_AMBIGUOUS ||
      group_after_class(9, 5, 9) != GROUP_AMBIGUOUS || group_after_class(10, 5, 9) != GROUP_AFTER || group_after_class(GROUP_KEY_INF, 5, 9) != GROUP_AMBIGUOUS ||
      group_after_class(GROUP_KEY_NAN, 5, 9) != GROUP_AMBIGUOUS || group_after_side(GROUP_BEFORE, 1, 9, 9) || !group_after_side(GROUP_AMBIGUOUS, 7, 8, 3) ||
      group_after_side(GROUP_AMBIGUOUS, 9, 8, GROUP_KEY_NAN) || group_after_side(GROUP_AFTER, 7, 8, 3) || !group_after_side(GROUP_AFTER, 7, 8, 7)) {
    printf("group_after_class / group_after_side\n");
    ++fails;
  }
  for (uint32_t key : {0u, 3u, 5u, 7u, 9u, 11u, 0xFF7FFFFFu, GROUP_KEY_INF, GROUP_KEY_NAN}) {  // group_count_class is count_window_class
    CountWindow w;
    w.in_lo = 5, w.in_hi = 7, w.out_lo = 4, w.out_hi = 9;
    if (group_count_class(key, w.in_lo, w.in_hi, w.out_lo, w.out_hi) != (int)count_window_class(w, key)) {
      printf("group_count_class(%08x) is not count_window_class\n", key);
      ++fails;
    }
  }
  part_a();
  part_b();
  printf("%ld checks, %ld heads taken, %ld side rows, %ld heads before, %ld ambiguous, %ld groups counted in, %ld count side rows, %d failures\n", checks,
         n_heads_taken, n_side, n_before, n_ambiguous, n_count_in, n_count_side, fails);
  if (fails) return 1;
  if (n_side == 0 || n_heads_taken == 0 || n_before == 0 || n_ambiguous == 0 || n_count_in == 0 || n_count_side == 0) {
    printf("a class of the rule never occurred\n");
    return 1;
  }
  printf("group after rule ok\n");
  return 0;
}
