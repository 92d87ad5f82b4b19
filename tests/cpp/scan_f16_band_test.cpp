// Host-only check of tostore_amd/csrc/tsh_scan_f16_band.h: the band claimed for the fp16 scan's key holds for a software
// model of the kernel's arithmetic (operands rounded to fp16 after the power-of-two scale, f32 FMA chain, the epilogue's
// roundings), on random rows, on rows whose operands sit at fp16 rounding midpoints -/+ 1 ulp with products of one sign,
// and on rows deep in fp16's subnormal steps -- and, for L2, that the band also reaches the ORACLE's key of the row: its
// f64 sum of (q_j - v_ij)^2 in element order less |q|^2, the number the ids are decided by (queries 2^40 above and below
// the rows, where that sum's own rounding is the whole band).  Prints the largest observed / claimed ratio; exit status 1 on a miss.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../../tostore_amd/csrc/tsh_scan_f16_band.h"

static int fails = 0;

// round to nearest even onto fp16's grid (normal and subnormal steps; no overflow in this test)
static float to_f16(float x) {
  if (x == 0.f) return x;
  int e = 0;
  std::frexp(x, &e);  // |x| = m 2^e, m in [0.5, 1): the leading bit is 2^(e - 1)
  const int lead = e - 1 < -14 ? -14 : e - 1;
  const double step = std::ldexp(1.0, lead - 10);
  return (float)(std::nearbyint((double)x / step) * step);
}

static double run(int metric, int dim, int pattern, unsigned seed, int qexp = 0) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> G(0.0, 1.0);
  const int n = 400, nch = (dim / 4 + 63) / 64;
  auto pat = [&](bool up) {  // 2^e (1 + m), low mantissa bits just below / above the fp16 midpoint
    const int e = U(rng) < 0.5 ? -1 : 0;
    const int j = 200 + (int)(U(rng) * 48);
    return (float)std::ldexp(1.0 + j * std::ldexp(1.0, -10) + std::ldexp(1.0, -11) + (up ? 1 : -1) * std::ldexp(1.0, -21), e);
  };
  std::vector<float> q(dim);
  for (auto &x : q) x = std::ldexp(pattern ? pat(false) : (float)G(rng), qexp);
  std::vector<std::vector<float>> rows(n, std::vector<float>(dim));
  float max_abs = 0.f, max_norm = 0.f, min_norm = INFINITY;
  std::vector<double> nrm(n);
  for (int i = 0; i < n; ++i) {
    const double sc = pattern == 2 ? std::ldexp(1.0, -(int)(U(rng) * 27)) : (pattern ? std::ldexp(1.0, -(int)(U(rng) * 5)) : 0.5 + 1.5 * U(rng));
    double s = 0;
    for (int j = 0; j < dim; ++j) {
      rows[i][j] = (float)((pattern ? (double)pat(i & 1) : G(rng)) * sc);
      max_abs = std::fmax(max_abs, std::fabs(rows[i][j]));
      s += (double)rows[i][j] * rows[i][j];
    }
    nrm[i] = std::sqrt(s);
    max_norm = std::fmax(max_norm, std::nextafter((float)nrm[i], INFINITY));
    min_norm = std::fmin(min_norm, std::nextafter((float)nrm[i], 0.f));
  }
  int v_exp = 0;
  if (!tsh::scan_f16_exp(max_abs, &v_exp)) return ++fails, 9.0;
  const tsh::ScanF16Band b = tsh::scan_f16_band(metric, dim, nch, q.data(), max_norm, min_norm, v_exp);
  if (!b.ok) return ++fails, 9.0;
  const float S = std::ldexp(1.0f, v_exp), inv_scale = std::ldexp(1.0f, -v_exp);
  double worst = 0;
  for (int i = 0; i < n; ++i) {
    float lane[64] = {0};  // 64 FMA chains, then a pairwise tree: the kernel's shape
    long double dot = 0, qq = 0;
    double oracle = 0;  // the oracle's sum: f64, element order
    for (int j = 0; j < dim; ++j) {
      const double diff = (double)q[j] - (double)rows[i][j];
      oracle += diff * diff;
      qq += (long double)q[j] * q[j];
      const float h = to_f16(rows[i][j] * S);
      const int l = (j / 4) % 64;
      lane[l] = std::fmaf(q[j], h, lane[l]);
      dot += (long double)q[j] * rows[i][j];
    }
    for (int w = 32; w > 0; w >>= 1)
      for (int l = 0; l < w; ++l) lane[l] = lane[l] + lane[l + w];
    const float d = lane[0] * inv_scale;
    const float sq = (float)(nrm[i] * nrm[i]);
    float key;
    long double exact;
    float w = std::fmaf(b.alpha, std::sqrt(sq), b.beta);
    if (metric == 0) key = std::fmaf(-2.f, d, sq), exact = (long double)nrm[i] * nrm[i] - 2 * dot;
    else if (metric == 1) key = -d, exact = -dot;
    else key = -(d * (float)(1.0 / nrm[i])), exact = -dot / nrm[i], w = b.beta;
    const float up = key + w;  // what the kernel stores
    const double ratio = (double)std::fabs((long double)up - w - exact) / w;
    if (ratio > worst) worst = ratio;
    if (metric == 0) {
      const double r2 = (double)std::fabs((long double)up - w - ((long double)oracle - qq)) / w;
      if (r2 > worst) worst = r2;
    }
    if (!(w <= b.w_max)) ++fails;
  }
  if (!(worst <= 1.0)) ++fails;
  return worst;
}

int main() {
  for (int metric = 0; metric < 3; ++metric)
    for (int dim : {256, 768, 1000, 1536, 3584})
      for (int pattern = 0; pattern < 3; ++pattern)
        printf("metric %d dim %4d pattern %d: max observed / claimed = %.4f\n", metric, dim, pattern, run(metric, dim, pattern, 17u * dim + metric));
  for (int dim : {256, 768})
    for (int qexp : {-40, 30, 40, 46})
      printf("metric 0 dim %4d queries x 2^%d: max observed / claimed = %.4f\n", dim, qexp, run(0, dim, 0, 23u * dim + qexp, qexp));
  // outside the model: a non-finite query, a cosine shard with a zero row
  std::vector<float> q(256, 1.f);
  q[3] = INFINITY;
  if (tsh::scan_f16_band(0, 256, 1, q.data(), 1.f, 1.f, 14).ok) ++fails;
  q[3] = 1.f;
  if (tsh::scan_f16_band(2, 256, 1, q.data(), 1.f, 0.f, 14).ok) ++fails;
  int e = 0;
  if (!tsh::scan_f16_exp(1.0f, &e) || e != 13 || !tsh::scan_f16_exp(0.f, &e) || tsh::scan_f16_exp(1e-30f, &e)) ++fails;
  printf(fails ? "FAILED: %d\n" : "band ok\n", fails);
  return fails ? 1 : 0;
}
