// Host-only check of tostore_amd/csrc/tsh_scan_i8_band.h: the band claimed for the coarse int8 scan's key holds for a
// software model of the kernel's arithmetic (per-row scale, biased byte codes, f32 FMA chain over the codes, the bias
// correction, the scale and the epilogue's roundings) against long-double sums, on
//   pattern 0  random rows
//   pattern 1  rows whose elements sit at quantisation midpoints (codes +/- 1/2), every error of the sign of its q_j
//   pattern 2  rows with one dominant element (every other code is 0 or +/- 1)
//   pattern 3  rows so small that their scale is at the floor (elements below 2^-126 / subnormal), among normal ones
// with mixed-sign and all-negative queries, d = 100, 768, 1000.  Both stored sides are checked: lower <= exact <= upper --
// and, for L2, lower <= the ORACLE's key <= upper: its f64 sum of (q_j - v_ij)^2 in element order less |q|^2, the number
// the ids are decided by (also with queries 2^40 above and below the rows, where that sum's own rounding is the whole band).
// Prints the largest observed / claimed ratio; exit status 1 on a miss.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../../tostore_amd/csrc/tsh_scan_i8_band.h"

static int fails = 0;

static double run(int metric, int dim, int pattern, int qsign, unsigned seed, int qexp = 0) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> G(0.0, 1.0);
  const int n = 300, nch = ((dim + 3) / 4 + 63) / 64;
  std::vector<float> q(dim);
  for (auto &x : q) x = std::ldexp(qsign ? -(float)std::fabs(G(rng)) - 0.01f : (float)G(rng), qexp);
  std::vector<std::vector<float>> rows(n, std::vector<float>(dim));
  float max_abs = 0.f, max_norm = 0.f, min_norm = INFINITY;
  std::vector<double> nrm(n);
  for (int i = 0; i < n; ++i) {
    const double s0 = std::ldexp(1.0, -(int)(U(rng) * 12));
    for (int j = 0; j < dim; ++j) {
      double v;
      if (pattern == 1) {
        const int c = 2 * ((int)(U(rng) * 126) - 63);  // even: a tie rounds back to it
        v = (c + (q[j] > 0 ? 0.5 : -0.5)) * s0;
        if (j == i % dim) v = 127.0 * s0;  // pins the scale to s0
      } else if (pattern == 2) {
        v = j == i % dim ? 50.0 : 0.3 * G(rng);
      } else if (pattern == 3) {
        v = G(rng) * ((i & 1) ? 3e-39 : (i & 2) ? 2e-37 : 1.0);
      } else {
        v = G(rng) * (0.5 + 1.5 * U(rng));
      }
      rows[i][j] = (float)v;
      max_abs = std::fmax(max_abs, std::fabs(rows[i][j]));
    }
    double s = 0;
    for (int j = 0; j < dim; ++j) s += (double)rows[i][j] * rows[i][j];
    nrm[i] = std::sqrt(s);
    max_norm = std::fmax(max_norm, std::nextafter((float)nrm[i], INFINITY));
    min_norm = std::fmin(min_norm, std::nextafter((float)nrm[i], 0.f));
  }
  const tsh::ScanI8Band b = tsh::scan_i8_band(metric, dim, nch, q.data(), max_norm, min_norm, max_abs);
  if (!b.ok) return ++fails, 9.0;
  double worst = 0;
  for (int i = 0; i < n; ++i) {
    float mx = 0.f;
    for (int j = 0; j < dim; ++j) mx = std::fmax(mx, std::fabs(rows[i][j]));
    const float sc = tsh::scan_i8_scale(mx);
    float lane[64] = {0};  // 64 FMA chains, then a pairwise tree: the kernel's shape
    long double dot = 0, qq = 0;
    double oracle = 0;  // the oracle's sum: f64, element order
    for (int j = 0; j < dim; ++j) {
      const double diff = (double)q[j] - (double)rows[i][j];
      oracle += diff * diff;
      qq += (long double)q[j] * q[j];
      float c = std::nearbyint(rows[i][j] / sc);
      c = std::fmin(std::fmax(c, -127.f), 127.f);
      const float byte = c + 128.f;
      const int l = (j / 4) % 64;
      lane[l] = std::fmaf(q[j], byte, lane[l]);
      dot += (long double)q[j] * rows[i][j];
    }
    for (int w = 32; w > 0; w >>= 1)
      for (int l = 0; l < w; ++l) lane[l] = lane[l] + lane[l + w];
    const float t = lane[0] - b.qbias;
    const float d = sc * t;
    const float sq = (float)(nrm[i] * nrm[i]), inv = (float)(1.0 / nrm[i]);
    float key, w;
    long double exact;
    if (metric == 0) key = std::fmaf(-2.f, d, sq), exact = (long double)nrm[i] * nrm[i] - 2 * dot;
    else if (metric == 1) key = -d, exact = -dot;
    else key = -(d * inv), exact = -dot / nrm[i];
    if (metric == 2) w = std::fmaf(b.a_s * sc, inv, b.beta);
    else w = std::fmaf(b.a_s, sc, std::fmaf(b.a_v, std::sqrt(sq), b.beta));
    const float lo = key - w, up = key + w;  // what the kernel stores / folds into the tile's minimum
    if (!((long double)lo <= exact && exact <= (long double)up)) ++fails;
    if (metric == 0 && !((long double)lo <= (long double)oracle - qq && (long double)oracle - qq <= (long double)up)) ++fails;
    const double ratio = (double)std::fabs((long double)key - exact) / w;
    if (ratio > worst) worst = ratio;
  }
  if (!(worst <= 1.0)) ++fails;
  return worst;
}

int main() {
  for (int metric = 0; metric < 3; ++metric)
    for (int dim : {100, 768, 1000})
      for (int pattern = 0; pattern < 4; ++pattern)
        for (int qsign = 0; qsign < 2; ++qsign)
          printf("metric %d dim %4d pattern %d query %s: max observed / claimed = %.4f\n", metric, dim, pattern, qsign ? "negative" : "mixed   ",
                 run(metric, dim, pattern, qsign, 31u * dim + 7u * pattern + metric));
  for (int dim : {100, 768})
    for (int qexp : {-40, 30, 40, 46})
      printf("metric 0 dim %4d queries x 2^%d: max observed / claimed = %.4f\n", dim, qexp, run(0, dim, 0, 0, 29u * dim + qexp, qexp));
  // outside the model: a non-finite or huge query element, a cosine shard with a zero row, scales outside f32
  std::vector<float> q(256, 1.f);
  q[3] = INFINITY;
  if (tsh::scan_i8_band(0, 256, 1, q.data(), 1.f, 1.f, 1.f).ok) ++fails;
  q[3] = 1e20f;
  if (tsh::scan_i8_band(0, 256, 1, q.data(), 1.f, 1.f, 1.f).ok) ++fails;
  q[3] = 1.f;
  if (!tsh::scan_i8_band(0, 256, 1, q.data(), 1.f, 1.f, 1.f).ok) ++fails;
  if (tsh::scan_i8_band(2, 256, 1, q.data(), 1.f, 0.f, 1.f).ok) ++fails;
  if (tsh::scan_i8_band(1, 256, 1, q.data(), 1e-36f, 1e-37f, 1e-37f).ok) ++fails;  // max_abs / 127 is subnormal
  if (tsh::scan_i8_band(1, 256, 1, q.data(), 3e38f, 1.f, 3e38f).ok) ++fails;
  if (tsh::scan_i8_band(1, 256, 1, q.data(), INFINITY, 1.f, INFINITY).ok) ++fails;
  if (tsh::scan_i8_scale(127.f) != 1.f || tsh::scan_i8_scale(0.f) != 1.17549435e-38f || tsh::scan_i8_scale(1.f) * 127.0 < 1.0) ++fails;
  printf(fails ? "FAILED: %d\n" : "band ok\n", fails);
  return fails ? 1 : 0;
}
