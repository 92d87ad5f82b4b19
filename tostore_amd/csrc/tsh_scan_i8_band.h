// tsh_scan_i8_band.h -- the error band of scan_i8_kernel's ranking key (tsh_kernels.hip.h), per row and proven.
// Pure host arithmetic, no HIP: compiled into the library and, on its own, by tests/cpp/scan_i8_band_test.cpp.
//
// The copy (rows8_convert_kernel): per row a scale s_i = max(roundup(max_j |v_ij| / 127), 2^-126) and codes
// c_ij = rint(fl(v_ij / s_i)) in [-127, 127], stored as the biased bytes b_ij = c_ij + 128 in [1, 255].  With u = 2^-24:
//   |v_ij - s_i c_ij| <= s_i (1/2 + 127 u)      (the division rounds once, rint moves by at most 1/2)
// The kernel forms  acc = sum_j q_j * float(b_ij)  in f32 FMAs (m = 4 nch + 6 roundings on a row's way through a lane's
// chain and the butterfly, gam = m 2^-23), t = fl(acc - qb) with qb = fl(128 sum_j q_j) from the host (f64 sum, one
// rounding), dot = fl(s_i t), and from it
//   L2      key_i = fl(sq_i - 2 dot)        exact_i = |v_i|^2 - 2 q.v_i       (the common |q|^2 is left out)
//   IP      key_i = -dot                    exact_i = -q.v_i
//   cosine  key_i = -fl(dot inv_i)          exact_i = -q.v_i / |v_i|
// with sq_i = fl(|v_i|^2), inv_i = fl(1 / |v_i|) from the ingest pass.  |q|_1 = sum |q_j|.  Then
//   operand   |sum q_j (v_ij - s_i c_ij)| <= s_i |q|_1 (1/2 + 2^-16)   -- the tight term: |q|_1 <= sqrt(d) |q|
//   chain     |acc - sum q_j b_ij| <= gam sum |q_j| b_ij <= 255 gam |q|_1
//   bias      |qb - 128 sum q_j| <= 128 u |q|_1; the subtraction rounds once: |acc - qb| <= 128 |q|_1, so 128 u |q|_1
//   scale     fl(s_i t): u s_i |t| <= 128 u s_i |q|_1
//   => |dot - q.v_i| <= kap s_i |q|_1,  kap = 1/2 + 2^-16 + 256 gam + 512 u
//   underflow every operation on the way may lose up to 2^-126 (flushed or gradual), the codes of a row whose elements
//             are below 2^-126 as much per element: `under`
//   L2        twice the above; sq_i, the subtraction and the addition of -/+ w_i round once each:
//             <= 2^-23 (3 |v_i|^2 + 4 |q| |v_i|), and |v_i|^2 <= max|v| |v_i| keeps the band linear in |v_i|
//             and the oracle's own f64 sum of |q - v_i|^2, which decides the ids: g (|q|^2 + 2 |q| |v_i| + |v_i|^2),
//             g = (d + 4) 2^-52 (tsh_scan_f16_band.h)
//   IP        the addition of -/+ w_i: <= 2^-23 |q| |v_i|
//   cosine    dot's error divided by |v_i|; inv_i, the product and the addition round once each: 2^-21 |q| covers them
// so that |key_i - exact_i| <= w_i with
//   L2 / IP   w_i = a_s s_i + a_v |v_i| + beta           cosine   w_i = a_s s_i inv_i + beta
// Every coefficient is multiplied by 1.001: the device recomputes |v_i| as sqrtf(sq_i) and forms w_i in f32.
// The scan stores the LOWER side key_i - w_i per row and the tile's minimum of the UPPER sides key_i + w_i.
#pragma once
#include <cmath>

namespace tsh {

struct ScanI8Band {
  float a_s = 0.f, a_v = 0.f, beta = 0.f;
  float qbias = 0.f;  // fl(128 sum q_j): what the kernel takes off the biased sum
  bool ok = false;    // false: outside the model (the route is not taken)
};

// the scale of one row of the int8 copy, from its largest |element| (finite): at least mx / 127, never below 2^-126
inline float scan_i8_scale(float mx) {
  float s = mx / 127.0f;
  if ((double)s * 127.0 < (double)mx) s = std::nextafter(s, INFINITY);  // (the product is exact in f64)
  return s < 1.17549435e-38f ? 1.17549435e-38f : s;
}

// metric: 0 L2, 1 inner product, 2 cosine.  q: dim floats.  max_norm / min_norm: over the shard's rows (min_norm = 0:
// unknown or a zero row).  max_abs: the shard's largest |element|.
inline ScanI8Band scan_i8_band(int metric, int dim, int nch, const float *q, float max_norm, float min_norm, float max_abs) {
  ScanI8Band b;
  double qn2 = 0.0, q1 = 0.0, qs = 0.0;
  for (int i = 0; i < dim; ++i) {
    const double a = std::fabs((double)q[i]);
    if (!(a <= 1.0e15)) return b;
    qn2 += a * a;
    q1 += a;
    qs += (double)q[i];
  }
  if (!std::isfinite(max_abs) || !std::isfinite(max_norm)) return b;
  const double smax = (double)max_abs / 127.0 * (1.0 + 1e-6);
  if (!(smax >= 1.17549435e-38) || !(smax < 1.0e30)) return b;  // the shard's scales under- or overflow f32
  const double qn = std::sqrt(qn2) * (1.0 + 1e-6);
  const double u = 5.9604644775390625e-08, u2 = 1.1920928955078125e-07;
  const double gam = (4.0 * nch + 6.0) * u2;
  const double kap = 0.5 + 1.52587890625e-05 + 256.0 * gam + 512.0 * u;
  const double tiny = 1.17549435e-38;  // 2^-126
  const double under = tiny * (((double)dim + 4.0) * smax + 2.0 + 2.0 * q1);
  const double mx = (double)max_norm * (1.0 + 1e-6);
  double a_s, a_v, beta;
  if (metric == 0) {
    const double g64 = ((double)dim + 4.0) * 2.220446049250313e-16;  // (d + 4) 2^-52: the oracle's own f64 sum
    a_s = 2.0 * kap * q1;
    a_v = u2 * (3.0 * mx + 4.0 * qn) + g64 * mx;
    beta = 2.0 * under + g64 * qn * (qn + 2.0 * mx);
  } else if (metric == 1) {
    a_s = kap * q1;
    a_v = u2 * qn;
    beta = under;
  } else {
    if (!(min_norm > 0.f)) return b;
    a_s = kap * q1;
    a_v = 0.0;
    beta = 4.76837158203125e-07 /*2^-21*/ * qn + under / ((double)min_norm * (1.0 - 1e-6));
  }
  auto up = [](double x) {
    float f = (float)x;
    if ((double)f < x) f = std::nextafter(f, INFINITY);
    return f;
  };
  b.a_s = up(a_s * 1.001);
  b.a_v = up(a_v * 1.001);
  b.beta = up(beta * 1.001);
  b.qbias = (float)(128.0 * qs);
  // the widest band of any row (cosine: s_i <= |v_i| / 127 rounded up, or the floor 2^-126)
  const double w_top = metric == 2 ? (double)b.a_s * std::fmax(0.008, tiny / ((double)min_norm * (1.0 - 1e-6))) + b.beta
                                   : (double)b.a_s * smax + (double)b.a_v * mx + b.beta;
  b.ok = std::isfinite(b.a_s) && std::isfinite(b.a_v) && std::isfinite(b.beta) && std::isfinite(b.qbias) && w_top < 1.0e37;
  return b;
}

}  // namespace tsh
