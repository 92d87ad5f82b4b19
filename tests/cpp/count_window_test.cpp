// Host-only check of tostore_amd/csrc/tsh_count_band.h: the window of a count never calls a row that belongs in the list
// certainly OUT, nor a row that does not belong certainly IN -- for the software model of the scan's f32 key that
// after_band_test.cpp uses: the exact value the key stands for, moved to BOTH ends of the per-key bound the error model
// claims (compute_band's arithmetic is repeated here) and rounded inwards to f32.  The distances are the finaliser's:
// sqrt(s0), -s0, 1 - s0 / (sqrt(mag_a) sqrt(s1)) in f64.  "Belongs" is written here a second time, from the
// specification: not (d > T) under IEEE >, a NaN T drops nothing; and (d, id) strictly after the cursor under Dart's
// double.compareTo, ties by id.
//   L2      sums given directly: 0.0, f64-denormal sums, sums below the f32 range, crowds a few ulps apart, large sums
//   IP      sums given directly, both signs (negative distances), +0.0 and -0.0 (distances -0.0 and +0.0)
//   cosine  vectors, d = 4, 100, 768: random rows, parallel, antiparallel, duplicates, a zero row; random and zero queries
// Thresholds T and cursors D: every row's distance, one ulp below and above it, 0.0, -0.0, values off every row, +-inf,
// NaN; T alone, D alone, and T with D at T, one ulp beside it and elsewhere (the bands overlap).  Row ids 6, 7, 8 against
// the cursor id 7: a row is certainly IN only if it belongs whatever its id, certainly OUT only if it does not.
// Also: without threshold and cursor every key is IN (a window that calls everything ambiguous fails), `skip` is set only
// where no modelled row belongs, and count_passes equals the second writing on a ladder of -0.0 / 0.0 / NaN / +-inf with
// id ties.  Exit status 1 on a miss.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../tostore_amd/csrc/tsh_count_band.h"

using namespace tsh;

static int fails = 0;
static long checks = 0, n_in = 0, n_out = 0, n_amb = 0;

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
// the specification, a second time
static bool belongs(double T, bool has_cursor, double D, int64_t cid, double d, int64_t id) {
  if (!(T != T) && d > T) return false;
  if (!has_cursor || D == -INFINITY) return true;
  const int c = dart_compare(d, D);
  return c > 0 || (c == 0 && id > cid);
}

struct Row {
  double dist;      // the finaliser's distance
  long double val;  // what the key stands for: s (L2), -s0 (IP), -(q.v) / |v| (cosine)
  double bound;     // the per-key bound at this value
};

// the f32 keys at both ends of [val - bound, val + bound], rounded inwards; false: no f32 lies inside
static bool model_keys(const Row &r, float *k_lo, float *k_hi) {
  const long double lo = r.val - (long double)r.bound, hi = r.val + (long double)r.bound;
  float a = (float)lo, b = (float)hi;
  if ((long double)a < lo) a = std::nextafter(a, INFINITY);
  if ((long double)b > hi) b = std::nextafter(b, -INFINITY);
  *k_lo = a;
  *k_hi = b;
  return (long double)a <= hi && (long double)b >= lo;
}

static const int64_t CID = 7;

static void check_one(const char *what, int metric, int dim, float eps_rel, float delta_abs, double mag_a, const std::vector<Row> &rows,
                      double T, bool has_cursor, double D) {
  const CountWindow w = count_window(metric, dim, eps_rel, delta_abs, mag_a, has_cursor, D, T);
  const bool from_start = !has_cursor || D == -INFINITY;
  const uint64_t ckey = after_order_key(D);
  for (const Row &r : rows) {
    float kk[2];
    if (!model_keys(r, &kk[0], &kk[1])) continue;
    bool all = true, any = false;
    for (int64_t id : {(int64_t)6, (int64_t)7, (int64_t)8}) {
      const bool b = belongs(T, has_cursor, D, CID, r.dist, id);
      all = all && b;
      any = any || b;
      if (count_passes(T, from_start, ckey, CID, r.dist, id) != b && fails++ < 10)
        printf("%s: count_passes(T %.17g, D %.17g, d %.17g, id %lld) != %d\n", what, T, D, r.dist, (long long)id, (int)b);
    }
    if (w.skip) {
      ++checks;
      if (any && fails++ < 10) printf("%s d=%d: T %.17g cursor %d %.17g skips the scan, row dist %.17g belongs\n", what, dim, T, (int)has_cursor, D, r.dist);
      continue;
    }
    for (float kf : kk) {
      const CountClass c = count_window_class(w, after_f2key(kf));
      ++checks;
      (c == COUNT_IN ? n_in : c == COUNT_OUT ? n_out : n_amb)++;
      if (c == COUNT_IN && !all && fails++ < 10)
        printf("%s d=%d: row dist %.17g key %.9g is IN, T %.17g cursor %d %.17g\n", what, dim, r.dist, kf, T, (int)has_cursor, D);
      if (c == COUNT_OUT && any && fails++ < 10)
        printf("%s d=%d: row dist %.17g key %.9g is OUT, T %.17g cursor %d %.17g\n", what, dim, r.dist, kf, T, (int)has_cursor, D);
      if (T != T && from_start && c != COUNT_IN && fails++ < 10)
        printf("%s d=%d: row dist %.17g key %.9g is not IN without threshold and cursor\n", what, dim, r.dist, kf);
    }
  }
}

static void check(const char *what, int metric, int dim, float eps_rel, float delta_abs, double mag_a, const std::vector<Row> &rows) {
  const double nan = std::nan("");
  std::vector<double> pts = {0.0, -0.0, 1e-3, 0.77, 1.0, 1.5, 123.456, -2.5, 1e-200, 3e30, 4.9406564584124654e-324, -4.9406564584124654e-324,
                             INFINITY, -INFINITY, nan};
  for (const Row &r : rows) {
    if (r.dist != r.dist || std::isinf(r.dist)) continue;
    pts.push_back(r.dist);
    pts.push_back(std::nextafter(r.dist, -INFINITY));
    pts.push_back(std::nextafter(r.dist, INFINITY));
  }
  check_one(what, metric, dim, eps_rel, delta_abs, mag_a, rows, nan, false, 0.0);
  size_t i = 0;
  for (double x : pts) {
    check_one(what, metric, dim, eps_rel, delta_abs, mag_a, rows, x, false, 0.0);  // a threshold alone
    check_one(what, metric, dim, eps_rel, delta_abs, mag_a, rows, nan, true, x);   // a cursor alone
    // both: the cursor at the threshold, an ulp beside it, and at another point of the set
    check_one(what, metric, dim, eps_rel, delta_abs, mag_a, rows, x, true, x);
    if (x == x && !std::isinf(x)) {
      check_one(what, metric, dim, eps_rel, delta_abs, mag_a, rows, x, true, std::nextafter(x, -INFINITY));
      check_one(what, metric, dim, eps_rel, delta_abs, mag_a, rows, x, true, std::nextafter(x, INFINITY));
      check_one(what, metric, dim, eps_rel, delta_abs, mag_a, rows, x, true, -x);
    }
    check_one(what, metric, dim, eps_rel, delta_abs, mag_a, rows, x, true, pts[(i * 7 + 3) % pts.size()]);
    ++i;
  }
}

int main() {
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> G(0.0, 1.0);
  const double u2 = 1.1920928955078125e-07;

  for (int dim : {4, 100, 768, 4073}) {
    const int nch = ((dim + 3) / 4 + 63) / 64;
    // ---- L2 (compute_band: eps = (4 nch + 8) 2^-23 per key, the band takes 3 eps; d 2^-100 of underflow slack) -------
    {
      const double eps = (4.0 * nch + 8.0) * u2;
      const float eps_rel = (float)(3.0 * eps), delta_abs = (float)((double)dim * 7.9e-31);
      std::vector<double> sums = {0.0, 4.9406564584124654e-324, 1e-310, 2.2250738585072014e-308, 1e-300, 1e-291, 1e-290, 1e-289,
                                  1e-60, 1e-46, 1.4e-45, 1e-40, 1.1754943508222875e-38, 1e-30, 1.0, 2.0, 768.0,
                                  (double)dim * 4e30, (double)dim * 4e30 * 0.999999, 3.0e38};
      for (int i = 0; i < 30; ++i) sums.push_back(std::exp((U(rng) - 0.5) * 120.0));
      for (double base : {1.0, 1536.123, 1e-20, 2.5e33})  // crowds: sums a few f64 ulps apart, and a few f32 ulps apart
        for (int j = -2; j <= 2; ++j) {
          sums.push_back(base * (1.0 + j * 2.2204460492503131e-16));
          sums.push_back(base * (1.0 + j * 1.1920928955078125e-07));
          sums.push_back(base * (1.0 + j * eps));
        }
      std::vector<Row> rows;
      for (double s : sums) rows.push_back({std::sqrt(s), (long double)s, eps * s + (double)dim * 7.9e-31 * 0.5});
      check("L2", 0, dim, eps_rel, delta_abs, 0.0, rows);
    }
    // ---- inner product (delta = gam |q| max|v| per key) ----------------------------------------------------------------
    for (double scale : {1.0, 1e-12, 1e9}) {
      const double qn = 1.3 * scale, max_norm = 2.0 * scale;
      const double gam = (4.0 * nch + 6.0) * u2;
      const double delta = gam * (qn * (1.0 + 1e-6)) * max_norm * (1.0 + 1e-6) + (double)dim * 7.5e-37;
      const float delta_abs = (float)(2.0 * delta * 1.0001);
      std::vector<double> s0 = {0.0, -0.0, 1e-300, -1e-300, 1e-45, -1e-45};
      for (int i = 0; i < 40; ++i) s0.push_back(G(rng) * qn * max_norm);
      for (double base : {0.5 * qn * max_norm, -0.25 * qn * max_norm})
        for (int j = -2; j <= 2; ++j) {
          s0.push_back(base * (1.0 + j * 2.2204460492503131e-16));
          s0.push_back(base + j * delta);
          s0.push_back(base + j * delta * 0.5);
        }
      std::vector<Row> rows;
      for (double s : s0) rows.push_back({-s, -(long double)s, delta});
      check("IP", 1, dim, 0.f, delta_abs, 0.0, rows);
    }
    // ---- cosine (delta = |q| (gam + 2^-21) per key; the finaliser's arithmetic on real vectors) -------------------------
    if (dim <= 768)
      for (int qkind = 0; qkind < 3; ++qkind) {
        std::vector<float> q(dim);
        for (auto &x : q) x = qkind == 2 ? 0.f : (float)(G(rng) * (qkind == 1 ? 37.5 : 1.0));
        double mag_a = 0;
        for (int i = 0; i < dim; ++i) mag_a = mag_a + (double)q[i] * (double)q[i];
        const double qn = std::sqrt(mag_a) * (1.0 + 1e-6);
        const double gam = (4.0 * nch + 6.0) * u2;
        const double delta = qn * (gam + 4.76837158203125e-07) + (double)dim * 7.5e-37;
        const float delta_abs = (float)(2.0 * delta * 1.0001);
        std::vector<Row> rows;
        for (int i = 0; i < 60; ++i) {
          std::vector<float> v(dim);
          const double sc = std::exp((U(rng) - 0.5) * 20.0);
          const int kind = i % 12;
          for (int j = 0; j < dim; ++j) {
            if (kind == 0) v[j] = (float)(q[j] * sc);                          // parallel: d ~ 0
            else if (kind == 1) v[j] = (float)(-q[j] * sc);                    // antiparallel: d ~ 2
            else if (kind == 2) v[j] = (float)(q[j] * sc + G(rng) * sc * 1e-4);  // nearly parallel
            else if (kind == 3) v[j] = 0.f;                                    // a zero row: d = 1
            else v[j] = (float)(G(rng) * sc);
          }
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
          rows.push_back({1.0 - sim, vv > 0 ? -dot / sqrtl(vv) : 0.0L, delta});
          if (kind == 5) rows.push_back(rows.back());  // duplicates
        }
        check("cosine", 2, dim, 0.f, delta_abs, mag_a, rows);
      }
  }
  // keys outside the model are never decided by the window
  {
    const CountWindow w = count_window(0, 8, 1e-6f, 1e-30f, 0.0, true, 1.0, 2.0);
    for (uint32_t key : {COUNT_KEY_INF, 0xFFFFFFFEu /* the scan's NaN key */})
      if (count_window_class(w, key) != COUNT_AMBIGUOUS) {
        printf("an infinite or NaN key must be AMBIGUOUS\n");
        ++fails;
      }
    if (count_threshold(-0.0) != 0.0 || std::signbit(count_threshold(-0.0)) || count_threshold(-1.5) != -1.5) {
      printf("count_threshold must turn -0.0 into +0.0 and nothing else\n");
      ++fails;
    }
  }
  // the exact predicate on a ladder of distances with -0.0 / 0.0 / NaN and id ties
  {
    const double nan = std::nan(""), inf = INFINITY;
    const double ladder[] = {-inf, -3.5, -4.9406564584124654e-324, -0.0, 0.0, 4.9406564584124654e-324, 1.0, 1.0000000000000002, inf, nan};
    const int n = (int)(sizeof ladder / sizeof *ladder);
    for (int t = 0; t < n; ++t)
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
          for (int has = 0; has < 2; ++has)
            for (int64_t ci : {(int64_t)-1, (int64_t)7, (int64_t)1 << 62})
              for (int64_t ri : {(int64_t)0, (int64_t)7, (int64_t)8, (int64_t)1 << 41}) {
                const double T = ladder[t], D = ladder[i], d = ladder[j];
                // thresholds by rank on the ladder, except that -0.0 / 0.0 are one value and NaN is none or, as a
                // distance, beyond no threshold
                const bool dropped = T == T && d == d && (j > t) && !(T == 0.0 && d == 0.0);
                const bool follows = !has || i == 0 || j > i || (j == i && ri > ci);
                ++checks;
                if (count_passes(T, !has || D == -inf, after_order_key(D), ci, d, ri) != (!dropped && follows) && fails++ < 10)
                  printf("T %g cursor %d (%g, %lld) entry (%g, %lld): passes != %d\n", T, has, D, (long long)ci, d, (long long)ri, (int)(!dropped && follows));
              }
  }
  printf("%ld checks: %ld IN, %ld OUT, %ld AMBIGUOUS, %d failures\n", checks, n_in, n_out, n_amb, fails);
  if (fails) return 1;
  if (n_in == 0 || n_out == 0 || n_amb == 0) {
    printf("a class never occurred\n");
    return 1;
  }
  printf("window ok\n");
  return 0;
}
