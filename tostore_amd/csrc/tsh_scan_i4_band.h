// tsh_scan_i4_band.h -- the error band of scan_i4_kernel's ranking key (tsh_scan_i4.hip.h), per row and proven.
// Pure host arithmetic, no HIP: compiled into the library and, on its own, by tests/cpp/scan_i4_band_test.cpp.
//
// The copy (rows4_convert_kernel) is made from the int8 copy (tsh_scan_i8_band.h): a row keeps its scale s_i, and the code
// of an element is the high nibble h_ij = b_ij >> 4 of its biased byte b_ij = c_ij + 128 in [1, 255].  Its value is
// recon4_ij = (16 h_ij + 8 - 128) s_i.  With u = 2^-24:
//   |b_ij - (16 h_ij + 8)| <= 8          and          |v_ij - s_i c_ij| <= s_i (1/2 + 127 u)   (the int8 copy's)
//   => |v_ij - recon4_ij| <= s_i (8 + 1/2 + 127 u)
// Beside the nibbles a row has rho_i >= |v_i - recon4_i|_2, formed in f64 at conversion and rounded up: over the row's dim
// elements -- the pad elements up to ld hold the code of zero, meet no query element and are no part of rho.
// L2 only.  The kernel forms  acc = sum_j q_j * float(h_ij)  in f32 FMAs, in SCAN_I4_ACC chains of 8 FMAs per group of 32
// elements, added up at the end (m = 8 groups + 8 roundings at the most on an element's way, gam = m 2^-23),
// t = fma(16, acc, -qb) with qb = fl((128 - 8) sum_j q_j) from the host (f64 sum, one rounding), dot = fl(s_i t), and
//   key_i = fma(-2, dot, sq_i)              exact_i = |v_i|^2 - 2 q.v_i       (the common |q|^2 is left out)
// |q|_1 = sum |q_j|, |q|_2^ = the query's norm rounded up.  Then
//   operand   |sum q_j (v_ij - recon4_ij)| <= min(s_i |q|_1 (8 + 1/2 + 2^-16), |q|_2^ rho_i)     (Cauchy-Schwarz)
//   chain     |acc - sum q_j h_ij| <= gam sum |q_j| h_ij <= 15 gam |q|_1, sixteen times that in t
//   bias      |qb - 120 sum q_j| <= 120 u |q|_1; the fma rounds once: |t| <= 128 |q|_1, so 128 u |q|_1
//   scale     fl(s_i t): u s_i |t| <= 128 u s_i |q|_1
//   => |dot - q.v_i| <= min(kap4 s_i |q|_1, |q|_2^ rho_i + kar s_i |q|_1)
//      kar = 256 gam + 512 u,  kap4 = 8 + 1/2 + 2^-16 + kar
//   underflow, the L2 cancellation and epilogue terms and the oracle's own (d + 4) 2^-52 (|q| + |v_i|)^2: the int8 band's
// so that |key_i - exact_i| <= w_i = min(a_s s_i, a_r rho_i + a_c s_i) + a_v |v_i| + beta.
// Both alternatives are per-row quantities times per-query factors: the kernel takes the min.
// Every coefficient is multiplied by 1.001: the device recomputes |v_i| as sqrtf(sq_i) and forms w_i in f32.
// The scan stores the LOWER side key_i - w_i per row and the tile's minimum of the UPPER sides key_i + w_i.
#pragma once
#include <cmath>

namespace tsh {

constexpr int SCAN_I4_GROUP = 32;  // elements of a row per 16-byte load
constexpr int SCAN_I4_ACC = 4;     // FMA chains per row

struct ScanI4Band {
  float a_s = 0.f, a_r = 0.f, a_c = 0.f, a_v = 0.f, beta = 0.f;
  float qbias = 0.f;  // fl(120 sum q_j): what the kernel takes off sixteen times the nibble sum
  bool ok = false;    // false: outside the model (the route is not taken)
};

// groups of SCAN_I4_GROUP elements a row of ld elements takes in the plane
inline int scan_i4_groups(long long ld) { return (int)((ld + SCAN_I4_GROUP - 1) / SCAN_I4_GROUP); }

// q: dim floats.  max_norm: over the shard's rows.  max_abs: the shard's largest |element|.
inline ScanI4Band scan_i4_band(int dim, int groups, const float *q, float max_norm, float max_abs) {
  ScanI4Band b;
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
  const double gam = (8.0 * groups + 8.0) * u2;
  const double kar = 256.0 * gam + 512.0 * u;
  const double kap4 = 8.5 + 1.52587890625e-05 + kar;
  const double tiny = 1.17549435e-38;  // 2^-126
  // (as the int8 band's, and rho_i itself may be flushed: |q|_2^ 2^-126)
  const double under = tiny * (((double)dim + 4.0) * smax + 2.0 + 2.0 * q1 + qn);
  const double mx = (double)max_norm * (1.0 + 1e-6);
  const double g64 = ((double)dim + 4.0) * 2.220446049250313e-16;  // (d + 4) 2^-52: the oracle's own f64 sum
  const double a_s = 2.0 * kap4 * q1;
  const double a_r = 2.0 * qn;
  const double a_c = 2.0 * kar * q1;
  const double a_v = u2 * (3.0 * mx + 4.0 * qn) + g64 * mx;
  const double beta = 2.0 * under + g64 * qn * (qn + 2.0 * mx);
  auto up = [](double x) {
    float f = (float)x;
    if ((double)f < x) f = std::nextafter(f, INFINITY);
    return f;
  };
  b.a_s = up(a_s * 1.001);
  b.a_r = up(a_r * 1.001);
  b.a_c = up(a_c * 1.001);
  b.a_v = up(a_v * 1.001);
  b.beta = up(beta * 1.001);
  b.qbias = (float)(120.0 * qs);
  const double w_top = (double)b.a_s * smax + (double)b.a_v * mx + b.beta;  // the widest band of any row
  b.ok = std::isfinite(b.a_s) && std::isfinite(b.a_r) && std::isfinite(b.a_c) && std::isfinite(b.a_v) && std::isfinite(b.beta) &&
         std::isfinite(b.qbias) && w_top < 1.0e37;
  return b;
}

}  // namespace tsh
