// tsh_after_band.h -- the floor of a cursor search (tsh_search_after) in the f32 scan's key space, proven.
// Pure host arithmetic, no HIP: compiled into the library and, on its own, by tests/cpp/after_band_test.cpp.
//
// A cursor search returns the rows whose (distance, id) orders strictly after the cursor's (D, id) -- Dart
// double.compareTo on the distance, ties by id.  The scan leaves one f32 key k_i per live row; after_floor_kernel
// (tsh_after.hip.h) sorts the rows into three classes by two keys lo <= hi:
//   BEFORE     k_i < lo         the row's distance d_i is certainly below D: it cannot follow the cursor
//   AFTER      k_i > hi         d_i is certainly above D: it follows the cursor whatever its id
//   AMBIGUOUS  lo <= k_i <= hi  the key cannot tell (d_i == D, where the id decides, is always here): the row's exact
//                               sums are taken and the finaliser decides
// What after_floor() guarantees: no row with d_i >= D (compareTo) is BEFORE and no row with d_i <= D is AFTER.
//
// What is known about a key (compute_band): with s_i the f64 sum the finaliser gets for the row --
//   L2      k_i ~ s_i = sum (q - v)^2        |k_i - s_i| <= e s_i + a    e = eps_rel / 3, a = delta_abs / 2 (underflow)
//   IP      k_i ~ x_i = -s_i = -sum q v      |k_i - x_i| <= w            w = delta_abs / 2
//   cosine  k_i ~ x_i = -(q.v) / |v|         |k_i - x_i| <= w            w = delta_abs / 2   (x_i = 0 for a zero row)
// (the select's band is the two-key form of the same bound: tau (1 + 3 e) >= tau (1 + e) / (1 - e), tau + 2 w; compute_band
// rounds 2 w 1.0001 to f32, so half of it is still at least w).  And from the sums to the distance (finalize_query):
//
// L2: d = fl(sqrt(s)), correctly rounded and monotone.  D < 0 or D = -0.0: every d = +0.0 or more follows, no floor.
//   Else with P = fl(D D) in f64 (relative error 2^-53), S_lo = P (1 - 2^-50), S_hi = P (1 + 2^-50):
//   s < S_lo            =>  s < pred(D)^2 (pred(D) >= D (1 - 2^-52), its square >= D^2 (1 - 2^-51))
//                       =>  sqrt(s) < pred(D)  =>  d <= pred(D) < D
//   s > S_hi            =>  s > succ(D)^2  =>  sqrt(s) > succ(D)  =>  d >= succ(D) > D
//   (P < 1e-290, D below ~1e-145: the square loses bits or underflows; then S_lo is taken as 0 -- nothing is BEFORE --
//   and S_hi as 2e-290 > D^2 (1 + 2^-50): rows with a larger sum are certainly AFTER.)
//   k < lo := down_f32(S_lo (1 - e) - a)  =>  s < S_lo: else k >= s (1 - e) - a >= S_lo (1 - e) - a >= lo.
//   k > hi := up_f32(S_hi (1 + e) + a)    =>  s > S_hi: else k <= s (1 + e) + a <= hi.
//
// IP: d = -s exactly, so d = x as reals, and two distances that differ as reals compare the same way under compareTo
//   (only +0.0 / -0.0 are equal reals that compareTo tells apart, and equal reals are never outside [lo, hi]: w > 0).
//   k < lo := down_f32(D - w)  =>  x < D (else k >= x - w >= D - w >= lo)  =>  d < D;   k > hi := up_f32(D + w)  =>  d > D.
//
// cosine: d = fl(1 - sim), sim = fl(s0 / fl(fl(sqrt(mag_a)) fl(sqrt(s1)))) (0 when the denominator is not positive:
//   a zero row or a zero query, for which x = 0 and d = 1 = 1 + x / |q| as well).  s0, s1, mag_a are sequential f64
//   sums of dim exact products: relative error dim 2^-53 of sum |q v| <= |q| |v| resp. of the sum itself; two square
//   roots, a product, a division and a subtraction round once each; |sim| <= 1 + 2^-40.  Altogether
//     |d - (1 + x / |q|)| <= eta := (dim + 16) 2^-52
//   (f64 underflow: no product of two f32 values underflows in f64; a quotient that does is below 2^-1022, far inside eta).
//   So with c = (D - 1) |q|:  d <= D  =>  x <= (D - 1 + eta) |q|  =>  k <= c + eta |q| + w;
//                             d >= D  =>  x >= (D - 1 - eta) |q|  =>  k >= c - eta |q| - w.
//   |q| = sqrt(mag_a) is known to dim 2^-53 relative: c and eta |q| are widened by 2^-40 relative.
//   lo := down_f32(c - eta |q| - w - 2^-40 |c|),  hi := up_f32(c + eta |q| + w + 2^-40 |c|).
//
// Keys are compared as the scan's order-preserving integers (f2key); a key that is NaN (KEY_NAN, not inside the model)
// is above every hi, so such a row stays a candidate and the finaliser decides.  hi is capped at the key of +inf.
// D = +inf or NaN never gets here (no row inside the model has such a distance: the scan is skipped); D = -inf is
// "from the start": no floor.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace tsh {

constexpr int AFTER_SIDE_CAP = 1024;  // AMBIGUOUS rows a context's side list holds before a search is redone with a larger one

struct AfterFloor {
  uint32_t lo = 0, hi = 0;  // scan keys (f2key order); lo == hi == 0: no floor, every row is AFTER
  bool none() const { return lo == 0 && hi == 0; }
};

// The order a cursor lives in: Dart double.compareTo on the distance as an integer order (-0.0 just below +0.0, every
// NaN the one largest key -- the finaliser's dart_order_key), ties by row id.  An entry follows the cursor iff it is
// strictly greater; "-inf with any id" is from the start and filters nothing (the callers' business).
inline uint64_t after_order_key(double d) {
  if (d != d) return ~0ull;
  uint64_t b;
  memcpy(&b, &d, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline bool after_follows(uint64_t cursor_key, int64_t cursor_id, uint64_t key, int64_t id) {
  return key != cursor_key ? key > cursor_key : id > cursor_id;
}

// host copy of f2key (tsh_kernels.hip.h) for finite or infinite f
inline uint32_t after_f2key(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// the largest float <= x / the smallest float >= x (x not NaN; beyond the f32 range: -+inf resp. +-FLT_MAX).  A zero
// comes back as the zero on the far side: keys order -0.0 below +0.0, the reals they stand for are equal.
inline float after_down_f32(double x) {
  float f = (float)x;
  if ((double)f > x) f = std::nextafter(f, -INFINITY);
  return f == 0.f ? -0.f : f;
}
inline float after_up_f32(double x) {
  float f = (float)x;
  if ((double)f < x) f = std::nextafter(f, INFINITY);
  return f == 0.f ? 0.f : f;
}

// metric: 0 L2, 1 inner product, 2 cosine.  eps_rel / delta_abs: compute_band's (not force_all).  mag_a: the query's
// sum q_i^2 in f64 (query_mag_a; cosine only).  after_dist: the cursor's distance, not NaN.
inline AfterFloor after_floor(int metric, int dim, float eps_rel, float delta_abs, double mag_a, double after_dist) {
  AfterFloor f;
  const double D = after_dist;
  if (D == -INFINITY) return f;
  const uint32_t key_inf = after_f2key(INFINITY);
  if (!(D < INFINITY)) {  // (+inf or NaN: callers skip the scan; every finite key is BEFORE)
    f.lo = f.hi = key_inf;
    return f;
  }
  double lo, hi;
  if (metric == 0) {
    if (std::signbit(D)) return f;  // below every L2 distance
    const double e = (double)eps_rel / 3.0, a = (double)delta_abs * 0.5;
    const double P = D * D;
    double s_lo = P * (1.0 - 8.8817841970012523e-16 /*2^-50*/), s_hi = P * (1.0 + 8.8817841970012523e-16);
    if (!(P >= 1.0e-290)) {  // (D below ~1e-145: the square loses bits or underflows)
      s_lo = 0.0;
      s_hi = 2.0e-290;
    }
    lo = s_lo * (1.0 - e) - a;
    hi = s_hi * (1.0 + e) + a;
    if (!(hi < INFINITY)) hi = INFINITY;  // (D^2 beyond f64)
    if (!(lo < INFINITY)) lo = INFINITY;
  } else if (metric == 1) {
    const double w = (double)delta_abs * 0.5;
    lo = D - w;
    hi = D + w;
  } else {
    const double w = (double)delta_abs * 0.5;
    const double qn = std::sqrt(mag_a);
    const double eta = ((double)dim + 16.0) * 2.2204460492503131e-16;  // 2^-52
    const double c = (D - 1.0) * qn;  // (one rounding each: inside the 2^-40 below)
    double slack = eta * qn + w + std::fabs(c) * 9.0949470177292824e-13;  // 2^-40
    if (!(slack < INFINITY)) slack = INFINITY;
    lo = c - slack;
    hi = c + slack;
    if (lo != lo) lo = -INFINITY;  // (inf - inf: a cursor beyond everything a key can say)
    if (hi != hi) hi = INFINITY;
  }
  const float flo = after_down_f32(lo), fhi = after_up_f32(hi);
  f.lo = after_f2key(flo);
  f.hi = after_f2key(fhi);
  if (f.hi > key_inf) f.hi = key_inf;
  if (f.lo > f.hi) f.lo = f.hi;
  if (f.lo == 0 && f.hi == 0) f.hi = 1;  // (never: key 0 is a NaN's bit pattern; keeps none() to the cases above)
  return f;
}

}  // namespace tsh
