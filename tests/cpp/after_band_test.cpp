// Host-only check of tostore_amd/csrc/tsh_after_band.h: the floor of a cursor search never puts a row that follows the
// cursor BEFORE it, nor a row at or before the cursor AFTER it -- for a software model of the scan's f32 key: the exact
// value the key stands for, moved to BOTH ends of the per-key bound the error model claims (compute_band's arithmetic is
// repeated here) and rounded inwards to f32.  The distances are the finaliser's: sqrt(s0), -s0,
// 1 - s0 / (sqrt(mag_a) sqrt(s1)) in f64, compared like Dart's double.compareTo.
//   L2      sums given directly: 0.0, f64-denormal sums, sums below the f32 range, crowds a few f64 ulps apart, random
//           magnitudes, sums near the f32 overflow guard (dim x (2e15)^2)
//   IP      sums given directly, both signs (negative distances), +0.0 and -0.0 (distances -0.0 and +0.0)
//   cosine  vectors, d = 4, 100, 768: random rows, rows parallel and antiparallel to the query, duplicates, a zero row;
//           random and zero queries
// Cursors: every row's distance, one ulp below and one ulp above it, 0.0, -0.0 and a few values off every row.
// Also: the AMBIGUOUS interval is no wider than 4 x the per-key bound -- the same bound the row model is moved by -- plus
// one f32 ulp per floor key (lo and hi are rounded outwards to keys the scan can store, which the bound knows nothing of;
// it matters only where a cursor is so large that an f32 ulp exceeds the bound), so a floor that calls everything
// ambiguous fails.  Last, the finaliser's cursor filter (after_order_key /
// after_follows) on a ladder of distances with -0.0 / 0.0 / NaN and id ties.  Exit status 1 on a miss.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../tostore_amd/csrc/tsh_after_band.h"

using namespace tsh;

static int fails = 0;
static long checks = 0;

static uint64_t order_key(double d) {  // double.compareTo as an integer order
  if (d != d) return ~0ull;
  uint64_t b;
  memcpy(&b, &d, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
static float key2f(uint32_t k) {
  uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float f;
  memcpy(&f, &b, 4);
  return f;
}
static double ulp32(double x) {
  const float f = (float)std::fabs(x);
  if (!(f < INFINITY)) return 0.0;
  return (double)std::nextafter(f, INFINITY) - (double)f;
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

static void check(const char *what, int metric, int dim, float eps_rel, float delta_abs, double mag_a,
                  const std::vector<Row> &rows, const std::vector<double> &cursors) {
  for (double D : cursors) {
    const AfterFloor f = after_floor(metric, dim, eps_rel, delta_abs, mag_a, D);
    const uint64_t kD = order_key(D);
    for (const Row &r : rows) {
      float kk[2];
      if (!model_keys(r, &kk[0], &kk[1])) continue;
      const uint64_t kd = order_key(r.dist);
      for (float kf : kk) {
        const uint32_t key = after_f2key(kf);
        const bool before = !f.none() && key < f.lo, after = f.none() || key > f.hi;
        ++checks;
        if (kd >= kD && before) {
          if (fails++ < 10) printf("%s d=%d: row dist %.17g is BEFORE cursor %.17g (key %.9g, lo %.9g)\n", what, dim, r.dist, D, kf, key2f(f.lo));
        }
        if (kd <= kD && after) {
          if (fails++ < 10) printf("%s d=%d: row dist %.17g is AFTER cursor %.17g (key %.9g, hi %.9g)\n", what, dim, r.dist, D, kf, key2f(f.hi));
        }
      }
    }
  }
}

static std::vector<double> cursors_of(const std::vector<Row> &rows) {
  std::vector<double> c = {0.0, -0.0, 1e-3, 0.77, 1.0, 1.5, 123.456, -2.5, 1e-200, 3e30};
  for (const Row &r : rows) {
    if (r.dist != r.dist || std::isinf(r.dist)) continue;
    c.push_back(r.dist);
    c.push_back(std::nextafter(r.dist, -INFINITY));
    c.push_back(std::nextafter(r.dist, INFINITY));
  }
  return c;
}

int main() {
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> G(0.0, 1.0);
  const double u2 = 1.1920928955078125e-07;
  double worst_width = 0.0;

  for (int dim : {4, 100, 768, 4073}) {
    const int nch = ((dim + 3) / 4 + 63) / 64;
    // ---- L2 (compute_band: eps = (4 nch + 8) 2^-23 per key, the band takes 3 eps; d 2^-100 of underflow slack) -------
    {
      const double eps = (4.0 * nch + 8.0) * u2;
      const float eps_rel = (float)(3.0 * eps), delta_abs = (float)((double)dim * 7.9e-31);
      std::vector<double> sums = {0.0, 4.9406564584124654e-324, 1e-310, 2.2250738585072014e-308, 1e-300, 1e-291, 1e-290, 1e-289,
                                  1e-60, 1e-46, 1.4e-45, 1e-40, 1.1754943508222875e-38, 1e-30, 1.0, 2.0, 768.0,
                                  (double)dim * 4e30, (double)dim * 4e30 * 0.999999, 3.0e38};
      for (int i = 0; i < 60; ++i) sums.push_back(std::exp((U(rng) - 0.5) * 120.0));
      for (double base : {1.0, 1536.123, 1e-20, 2.5e33})  // crowds: sums a few f64 ulps apart, and a few f32 ulps apart
        for (int j = -3; j <= 3; ++j) {
          sums.push_back(base * (1.0 + j * 2.2204460492503131e-16));
          sums.push_back(base * (1.0 + j * 1.1920928955078125e-07));
          sums.push_back(base * (1.0 + j * eps));
        }
      std::vector<Row> rows;
      for (double s : sums) rows.push_back({std::sqrt(s), (long double)s, eps * s + (double)dim * 7.9e-31 * 0.5});
      const std::vector<double> cur = cursors_of(rows);
      check("L2", 0, dim, eps_rel, delta_abs, 0.0, rows, cur);
      for (double D : cur) {
        const AfterFloor f = after_floor(0, dim, eps_rel, delta_abs, 0.0, D);
        if (f.none() || !(D * D < 3e38)) continue;
        // (the per-key bound the row model above is moved by: eps s + half the band's underflow term)
        const double width = (double)key2f(f.hi) - (double)key2f(f.lo), bound = eps * D * D + (double)dim * 7.9e-31 * 0.5;
        const double allowed = 4.0 * bound + 2.0 * ulp32(D * D);
        worst_width = std::fmax(worst_width, width / allowed);
        if (!(width <= allowed) && fails++ < 10) printf("L2 d=%d: cursor %.17g: interval %.9g wider than 4 x the per-key bound %.9g + the floor keys' own two f32 roundings = %.9g\n", dim, D, width, bound, allowed);
      }
    }
    // ---- inner product (delta = gam |q| max|v| per key) ----------------------------------------------------------------
    for (double scale : {1.0, 1e-12, 1e9}) {
      const double qn = 1.3 * scale, max_norm = 2.0 * scale;
      const double gam = (4.0 * nch + 6.0) * u2;
      const double delta = gam * (qn * (1.0 + 1e-6)) * max_norm * (1.0 + 1e-6) + (double)dim * 7.5e-37;
      const float delta_abs = (float)(2.0 * delta * 1.0001);
      std::vector<double> s0 = {0.0, -0.0, 1e-300, -1e-300, 1e-45, -1e-45};
      for (int i = 0; i < 80; ++i) s0.push_back(G(rng) * qn * max_norm);
      for (double base : {0.5 * qn * max_norm, -0.25 * qn * max_norm})
        for (int j = -3; j <= 3; ++j) {
          s0.push_back(base * (1.0 + j * 2.2204460492503131e-16));
          s0.push_back(base + j * delta);
          s0.push_back(base + j * delta * 0.5);
        }
      std::vector<Row> rows;
      for (double s : s0) rows.push_back({-s, -(long double)s, delta});
      std::vector<double> cur = cursors_of(rows);
      for (double c : {0.1, -0.3, 0.5000001, 7.0}) cur.push_back(c * qn * max_norm);  // (off every row, at the rows' scale)
      check("IP", 1, dim, 0.f, delta_abs, 0.0, rows, cur);
      for (double D : cur) {
        const AfterFloor f = after_floor(1, dim, 0.f, delta_abs, 0.0, D);
        if (f.none() || !(std::fabs(D) < 3e38)) continue;
        const double width = (double)key2f(f.hi) - (double)key2f(f.lo), allowed = 4.0 * delta + 2.0 * ulp32(D);
        worst_width = std::fmax(worst_width, width / allowed);
        if (!(width <= allowed) && fails++ < 10) printf("IP d=%d: cursor %.17g: interval %.9g wider than 4 x the per-key bound %.9g + the floor keys' own two f32 roundings = %.9g\n", dim, D, width, delta, allowed);
      }
    }
    // ---- cosine (delta = |q| (gam + 2^-21) per key; the finaliser's arithmetic on real vectors) -------------------------
    if (dim <= 768)
      for (int qkind = 0; qkind < 3; ++qkind) {
        std::vector<float> q(dim);
        for (auto &x : q) x = qkind == 2 ? 0.f : (float)(G(rng) * (qkind == 1 ? 37.5 : 1.0));
        double mag_a = 0;
        for (int i = 0; i < dim; ++i) mag_a = mag_a + (double)q[i] * (double)q[i];
        long double qn_l = 0;
        for (int i = 0; i < dim; ++i) qn_l += (long double)q[i] * (long double)q[i];
        qn_l = sqrtl(qn_l);
        const double qn = std::sqrt(mag_a) * (1.0 + 1e-6);
        const double gam = (4.0 * nch + 6.0) * u2;
        const double delta = qn * (gam + 4.76837158203125e-07) + (double)dim * 7.5e-37;
        const float delta_abs = (float)(2.0 * delta * 1.0001);
        std::vector<std::vector<float>> vs;
        for (int i = 0; i < 120; ++i) {
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
          vs.push_back(v);
          if (kind == 5) vs.push_back(v);  // duplicates
        }
        std::vector<Row> rows;
        for (const auto &v : vs) {
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
        }
        const std::vector<double> cur = cursors_of(rows);
        check("cosine", 2, dim, 0.f, delta_abs, mag_a, rows, cur);
        for (double D : cur) {
          const AfterFloor f = after_floor(2, dim, 0.f, delta_abs, mag_a, D);
          if (f.none() || !(std::fabs(D) < 1e30)) continue;
          const double width = (double)key2f(f.hi) - (double)key2f(f.lo);
          const double allowed = 4.0 * delta + 2.0 * ulp32((D - 1.0) * (double)qn_l);
          worst_width = std::fmax(worst_width, width / allowed);
          if (!(width <= allowed) && fails++ < 10) printf("cosine d=%d: cursor %.17g: interval %.9g wider than 4 x the per-key bound %.9g + the floor keys' own two f32 roundings = %.9g\n", dim, D, width, delta, allowed);
        }
      }
  }
  // "from the start", and cursors nothing inside the model can follow
  if (!after_floor(0, 8, 1e-6f, 1e-30f, 0.0, -INFINITY).none() || !after_floor(0, 8, 1e-6f, 1e-30f, 0.0, -0.0).none()) {
    printf("-inf / -0.0 (L2) must leave every row AFTER\n");
    ++fails;
  }
  for (int metric = 0; metric < 3; ++metric) {
    const AfterFloor f = after_floor(metric, 8, 1e-6f, 1e-6f, 2.0, INFINITY);
    if (f.none() || f.lo != after_f2key(INFINITY)) {
      printf("a +inf cursor must leave no finite key AFTER\n");
      ++fails;
    }
  }
  // the finaliser's cursor filter: strictly greater in (compareTo key, id)
  {
    const double nan = std::nan(""), inf = INFINITY;
    const double ladder[] = {-inf, -3.5, -4.9406564584124654e-324, -0.0, 0.0, 4.9406564584124654e-324, 1.0, 1.0000000000000002, inf, nan};
    const int n = (int)(sizeof ladder / sizeof *ladder);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j)
        for (int64_t ci : {(int64_t)-1, (int64_t)0, (int64_t)7, (int64_t)1 << 40})
          for (int64_t ri : {(int64_t)0, (int64_t)6, (int64_t)7, (int64_t)8, (int64_t)1 << 41}) {
            const bool want = j > i || (j == i && ri > ci);
            if (after_follows(after_order_key(ladder[i]), ci, after_order_key(ladder[j]), ri) != want) {
              if (fails++ < 10) printf("cursor (%g, %lld) / entry (%g, %lld): follows != %d\n", ladder[i], (long long)ci, ladder[j], (long long)ri, (int)want);
            }
          }
    if (after_order_key(-nan) != after_order_key(nan) || after_order_key(nan) != ~0ull) {  // every NaN is the one last key
      printf("NaNs must share the last key\n");
      ++fails;
    }
  }
  printf("%ld classifications, widest interval / allowed = %.3f, %d failures\n", checks, worst_width, fails);
  if (fails) return 1;
  printf("band ok\n");
  return 0;
}
