// tsh_scan_f16_band.h -- the error band of scan_f16_kernel's ranking key (tsh_kernels.hip.h), per row and proven.
// Pure host arithmetic, no HIP: compiled into the library and, on its own, by tests/cpp/scan_f16_band_test.cpp.
//
// The kernel forms  acc = sum_j q_j * float(h_ij)  in f32 FMAs, h_ij = fp16(S v_ij), S = 2^v_exp, and from it
//   L2      key_i = fl(sq_i - 2 acc / S)       exact_i = |v_i|^2 - 2 q.v_i       (the common |q|^2 is left out)
//   IP      key_i = -acc / S                   exact_i = -q.v_i
//   cosine  key_i = -fl((acc / S) inv_i)       exact_i = -q.v_i / |v_i|
// with sq_i = fl(|v_i|^2) and inv_i = fl(1 / |v_i|) from the ingest pass (f64 sums, one rounding).  Then
//   |key_i - exact_i| <= w_i = alpha |v_i| + beta
// where, with u = 2^-24, e = 2^-11 (fp16 round to nearest of a normal number), m = 4 nch + 6 roundings on a row's way
// through a lane's FMA chain and the butterfly, gam = m 2^-23 (>= m u / (1 - m u), twice over), |q|_1 = sum |q_j|:
//   operand   |sum q_j (h_ij / S - v_ij)| <= e |q| |v_i| + sub |q|_1,   sub = 2^-14 / S: an element whose scaled value
//             is below fp16's smallest normal number is off by at most that much, rounded OR flushed to zero
//   chain     |acc / S - sum q_j h_ij / S| <= gam (1 + e) |q| |v_i| + gam sub |q|_1, plus `under` for f32 underflow
//             (acc / S is exact: a power of two)
//   L2        twice the above; |sq_i - |v_i|^2| <= u |v_i|^2; the subtraction rounds once, u |key_i|, and so does the
//             addition of w_i: together <= 2^-23 (3 |v_i|^2 + 4 |q| |v_i|) -- and |v_i|^2 <= max|v| |v_i|, which keeps
//             the band linear in |v_i|
//             The ids are the ORACLE's, which ranks by its own f64 sum S_i = fl(sum_j (q_j - v_ij)^2), taken in element
//             order: |S_i - |q - v_i|^2| <= g |q - v_i|^2 with g = (d + 4) 2^-52 (the differences, the squares and the
//             additions round once each; the square root behind them merges sums less than 2^-52 apart).  A key that is
//             to bound the oracle's order has to be near S_i - |q|^2, not only near its exact value: g (|q|^2 + 2 |q|
//             |v_i| + |v_i|^2) more.  Nothing beside 2^-11 |q| |v_i| while |q| < 2^30 |v_i|; with queries 2^40 above the
//             rows it is the whole band -- every distance of the oracle is then the same number, its ids the lowest
//             ones, and the scan has to hand every row on (tests/test_gpu_scales.py found ids of the exact reduced
//             ranking returned there instead)
//   IP        the addition of w_i: <= 2^-23 |q| |v_i|
//   cosine    divided by |v_i| >= min|v| the operand and chain terms are uniform; inv_i, the product and the addition of
//             w round once each: 2^-21 |q| covers them (the f32 kernel's model takes the same term)
// Every sum is multiplied by 1.001: the device recomputes |v_i| as sqrtf(sq_i) (a few ulp) and adds w_i in f32.
// The scan stores the UPPER side key_i + w_i; the select kernel picks tiles with the uniform 2 w_max and emits a row
// iff its lower side key_i - w_i is at or below the bound (SelectArgs::w_sq).
#pragma once
#include <cmath>

namespace tsh {

struct ScanF16Band {
  float alpha = 0.f, beta = 0.f;  // w_i = alpha |v_i| + beta
  float w_max = 0.f;              // w at the longest row, rounded up
  bool ok = false;                // false: outside the model (the scan stays on f32)
};

// metric: 0 L2, 1 inner product, 2 cosine.  q: dim floats.  max_norm / min_norm: over the shard's rows (min_norm = 0:
// unknown or a zero row).  v_exp: the copy holds fp16(2^v_exp v).
inline ScanF16Band scan_f16_band(int metric, int dim, int nch, const float *q, float max_norm, float min_norm, int v_exp) {
  ScanF16Band b;
  double qn2 = 0.0, q1 = 0.0;
  for (int i = 0; i < dim; ++i) {
    const double a = std::fabs((double)q[i]);
    if (!(a <= 1.0e15)) return b;
    qn2 += a * a;
    q1 += a;
  }
  const double qn = std::sqrt(qn2) * (1.0 + 1e-6);
  const double e = 4.8828125e-04;                               // 2^-11
  const double gam = (4.0 * nch + 6.0) * 1.1920928955078125e-07;  // 2^-23 per rounding
  const double u2 = 1.1920928955078125e-07;
  const double sub = std::ldexp(1.0, -14 - v_exp);
  const double under = (double)dim * 8.1e-28;  // d 2^-90: f32 underflow on the way, |v_exp| <= 55
  const double dot_rel = e + gam * (1.0 + e);
  const double dot_abs = sub * q1 * (1.0 + gam) + under;
  const double mx = (double)max_norm * (1.0 + 1e-6);
  double alpha, beta;
  if (metric == 0) {
    const double g64 = ((double)dim + 4.0) * 2.220446049250313e-16;  // (d + 4) 2^-52: the oracle's own f64 sum
    alpha = 2.0 * dot_rel * qn + u2 * (3.0 * mx + 4.0 * qn) + g64 * mx;
    beta = 2.0 * dot_abs + g64 * qn * (qn + 2.0 * mx);
  } else if (metric == 1) {
    alpha = dot_rel * qn + u2 * qn;
    beta = dot_abs;
  } else {
    if (!(min_norm > 0.f)) return b;
    alpha = 0.0;
    beta = (dot_rel + 4.76837158203125e-07 /*2^-21*/) * qn + dot_abs / ((double)min_norm * (1.0 - 1e-6));
  }
  alpha *= 1.001;
  beta *= 1.001;
  auto up = [](double x) {
    float f = (float)x;
    if ((double)f < x) f = std::nextafter(f, INFINITY);
    return f;
  };
  b.alpha = up(alpha);
  b.beta = up(beta);
  b.w_max = up(((double)b.alpha * mx + (double)b.beta) * 1.0001);
  b.ok = std::isfinite(b.alpha) && std::isfinite(b.beta) && b.w_max < 1.0e37f;
  return b;
}

// the scale of the fp16 copy: 2^v_exp puts the largest |element| into [2^13, 2^14) (cosine rows are stored as they
// are, too: the kernel divides by the norm afterwards).  false: too close to the edge of f32's exponent range
inline bool scan_f16_exp(float max_abs, int *v_exp) {
  int e = 0;
  if (max_abs > 0.f) std::frexp(max_abs, &e);  // max_abs = m 2^e, m in [0.5, 1)
  else e = 1;
  *v_exp = 14 - e;
  return *v_exp <= 55 && *v_exp >= -55 && std::isfinite(max_abs);
}

}  // namespace tsh
