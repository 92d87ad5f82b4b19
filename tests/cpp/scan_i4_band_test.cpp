// A software model of scan_i4_kernel's arithmetic (tostore_amd/csrc/tsh_scan_i4.hip.h) against the band of
// tsh_scan_i4_band.h: observed / claimed <= 1 everywhere, and >= 0.9 on the adversarial rows, so that a slack band fails
// too.  Plain C++17, no HIP: g++ -O2 -std=c++17 -ffp-contract=off.  Prints "band ok" and exits 0, or says what broke.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../tostore_amd/csrc/tsh_scan_i4_band.h"
#include "../../tostore_amd/csrc/tsh_scan_i8_band.h"

using tsh::ScanI4Band;

struct Row {
  std::vector<float> v;
  float s = 0.f, rho = 0.f, sq = 0.f;
  std::vector<int> h;
};

// rows8_convert_kernel and rows4_convert_kernel
static void convert(Row &r) {
  const int d = (int)r.v.size();
  float mx = 0.f;
  for (float x : r.v) mx = std::fmax(mx, std::fabs(x));
  r.s = tsh::scan_i8_scale(mx);
  r.h.resize(d);
  double ss = 0.0, n2 = 0.0;
  for (int j = 0; j < d; ++j) {
    const float c = std::fmin(std::fmax(std::rint(r.v[j] / r.s), -127.0f), 127.0f) + 128.0f;
    r.h[j] = (int)c >> 4;
    const double diff = (double)r.v[j] - (double)r.s * (double)(16 * r.h[j] + 8 - 128);
    ss += diff * diff;
    n2 += (double)r.v[j] * (double)r.v[j];
  }
  const double x = std::sqrt(ss) * (1.0 + 1e-6);
  r.rho = (float)x;
  if ((double)r.rho < x) r.rho = std::nextafter(r.rho, INFINITY);
  r.sq = (float)n2;
}

// the kernel: four chains over the elements j = c (mod 4), added up pairwise; the epilogue.  Returns |key - exact| / w.
static double ratio_of(const Row &r, const std::vector<float> &q, const ScanI4Band &b, bool *inside) {
  const int d = (int)q.size();
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < d; ++j) acc[j & 3] = std::fmaf((float)r.h[j], q[j], acc[j & 3]);
  const float sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  const float dot = r.s * std::fmaf(16.f, sum, -b.qbias);
  const float x = std::fmaf(-2.f, dot, r.sq);
  const float w = std::fmin(b.a_s * r.s, std::fmaf(b.a_r, r.rho, b.a_c * r.s)) + std::fmaf(b.a_v, std::sqrt(r.sq), b.beta);
  long double n2 = 0, qv = 0;
  for (int j = 0; j < d; ++j) {
    n2 += (long double)r.v[j] * r.v[j];
    qv += (long double)r.v[j] * q[j];
  }
  const long double exact = n2 - 2 * qv;
  const float lower = x - w, upper = x + w;
  *inside = std::isfinite(w) && (long double)lower <= exact && exact <= (long double)upper;
  return (double)(std::fabs((double)((long double)x - exact)) / (double)w);
}

int main() {
  std::mt19937_64 rng(4);
  std::normal_distribution<float> gauss(0.f, 1.f);
  const int dims[] = {4, 256, 264, 768, 1000, 2048};
  const float scales[] = {1.f, 1e15f / 256.f, 1e-30f};
  double worst = 0.0, adv_l1_min = 1e9, adv_cs_min = 1e9;
  for (int d : dims) {
    const int groups = tsh::scan_i4_groups((d + 3) / 4 * 4);
    for (float scale : scales) {
      for (int kind = 0; kind < 3; ++kind) {  // 0: Gaussian rows; 1: adversarial, L1 side; 2: adversarial, Cauchy-Schwarz side
        std::vector<float> q(d);
        for (float &x : q) x = kind == 2 ? (gauss(rng) > 0 ? 0.37f : -0.37f) : gauss(rng);
        std::vector<Row> rows(24);
        float max_norm = 0.f, max_abs = 0.f;
        for (Row &r : rows) {
          r.v.resize(d);
          if (kind == 0) {
            const float len = 0.5f + 1.5f * (float)(rng() % 1000) / 1000.f;
            for (float &x : r.v) x = gauss(rng) * len * scale;
          } else {
            // every element 8.49 codes below its nibble's midpoint where q_j > 0, 7.49 above where q_j < 0 -- all errors of
            // one sign in q.v; element 0 pins the scale to s0
            const float s0 = std::ldexp(scale, -(int)(rng() % 8));
            for (int j = 0; j < d; ++j) {
              const int nib = 1 + (int)(rng() % 14);
              r.v[j] = (float)((16 * nib + 8 - 128) + (q[j] > 0 ? -8.49 : 7.49)) * s0;
            }
            if (d > 4) r.v[0] = 127.0f * s0;
          }
          convert(r);
          max_norm = std::fmax(max_norm, (float)(std::sqrt((double)r.sq) * (1 + 1e-6)));
          for (float x : r.v) max_abs = std::fmax(max_abs, std::fabs(x));
        }
        const ScanI4Band b = tsh::scan_i4_band(d, groups, q.data(), max_norm, max_abs);
        if (!b.ok) {
          std::printf("band not ok: d=%d scale=%g kind=%d\n", d, scale, kind);
          return 1;
        }
        double best = 0.0;
        for (const Row &r : rows) {
          bool inside;
          const double ratio = ratio_of(r, q, b, &inside);
          if (!inside || !(ratio <= 1.0)) {
            std::printf("outside the band: d=%d scale=%g kind=%d ratio=%.6f\n", d, scale, kind, ratio);
            return 1;
          }
          worst = std::fmax(worst, ratio);
          best = std::fmax(best, ratio);
        }
        // (at huge scales the rounding of |v|^2, a term the rows cannot steer, is most of the band: unit scale only.  d = 4
        // has no element to spare for pinning the scale, so its rows' codes do not sit where they were aimed: it is held to
        // <= 1 like every case, not to >= 0.9)
        if (scale != 1.f) continue;
        if (kind == 1 && d > 4) adv_l1_min = std::fmin(adv_l1_min, best);
        if (kind == 2 && d > 4) adv_cs_min = std::fmin(adv_cs_min, best);
      }
    }
  }
  std::printf("observed / claimed: worst %.4f; adversarial rows at least %.4f (L1 side) and %.4f (Cauchy-Schwarz side)\n", worst,
              adv_l1_min, adv_cs_min);
  if (adv_l1_min < 0.9 || adv_cs_min < 0.9) {
    std::printf("the band is slack on the adversarial rows\n");
    return 1;
  }
  // outside the model: the same cases as the int8 band
  std::vector<float> q(768, 1.f);
  q[5] = 2e15f;
  if (tsh::scan_i4_band(768, 24, q.data(), 1.f, 1.f).ok) return std::printf("a huge query element passed\n"), 1;
  q[5] = NAN;
  if (tsh::scan_i4_band(768, 24, q.data(), 1.f, 1.f).ok) return std::printf("a NaN query element passed\n"), 1;
  q[5] = 1.f;
  if (tsh::scan_i4_band(768, 24, q.data(), INFINITY, 1.f).ok) return std::printf("an infinite norm passed\n"), 1;
  if (tsh::scan_i4_band(768, 24, q.data(), 1.f, 0.f).ok) return std::printf("a zero shard passed\n"), 1;
  if (tsh::scan_i4_band(768, 24, q.data(), 1e37f, 1e35f).ok) return std::printf("overflowing scales passed\n"), 1;
  std::printf("band ok\n");
  return 0;
}
