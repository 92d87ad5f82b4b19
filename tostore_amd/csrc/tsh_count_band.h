// tsh_count_band.h -- the window of a count (tsh_search_count) in the f32 scan's key space, proven.
// Pure host arithmetic, no HIP: compiled into the library and, on its own, by tests/cpp/count_window_test.cpp.
//
// A count is the length of the list tsh_search_after would return with k = infinity: the live rows whose distance d_i
// is not beyond the threshold T (dropped iff d_i > T under IEEE >, a NaN T drops nothing) and whose (d_i, id) orders
// strictly after the cursor's (D, id) (Dart double.compareTo, ties by id; no cursor or D = -inf: every row).  The scan
// leaves one f32 key k_i per live row; count_window_kernel (tsh_count.hip.h) sorts the rows into three classes:
//   IN         in_lo <= k_i <= in_hi                     the row is in the list for certain: counted on the device
//   OUT        k_i < out_lo  or  k_i > out_hi            the row is not in the list for certain: ignored
//   AMBIGUOUS  everything else                           the row's exact sums are taken and the finaliser decides
//
// The window is made of two results of after_floor() (tsh_after_band.h, unchanged): F = after_floor(D) for the cursor
// and C = after_floor(T') for the threshold, T' = T with -0.0 replaced by +0.0.  What after_floor(X) = (lo <= hi)
// guarantees for a row inside the error model (its distance is finite, its key obeys the bound proven there):
//   (a) k_i < lo  =>  d_i < X in compareTo order          (b) k_i > hi  =>  d_i > X in compareTo order
// The window:  in_lo = F.hi + 1, in_hi = C.lo - 1, out_lo = F.lo, out_hi = C.hi.
//
// IN is right.  k_i > F.hi: by (b) d_i follows D whatever the ids, so the row follows the cursor.  k_i < C.lo: by (a)
//   d_i < T' in compareTo order; for two non-NaN doubles that means d_i < T' as reals, or d_i = -0.0 and T' = +0.0:
//   either way d_i > T' is false under IEEE >, and d_i > T is the same predicate (-0.0 and +0.0 are one threshold).
// OUT is right.  k_i < F.lo: by (a) d_i is before D, the row does not follow the cursor.  k_i > C.hi: by (b) d_i > T'
//   in compareTo order: d_i > T' as reals -- dropped -- or d_i = +0.0 and T' = -0.0, which T' never is.  That is why
//   -0.0 is replaced first: under after_floor(-0.0) a row at distance +0.0 could be OUT although +0.0 > -0.0 is false.
// IN and OUT are disjoint (F.lo <= F.hi, C.lo <= C.hi).  When the bands overlap (the cursor sits at the threshold:
//   F.hi >= C.lo) IN is empty and every key of [F.lo, C.hi], the union of the two bands, is AMBIGUOUS.
//
// The ends that are not a band:
//   no cursor, D = -inf, or F.none() (L2: D below every distance): every row follows; out_lo = 0, in_lo = 0.
//   D = +inf or NaN: no row inside the model follows (their distances are finite): `skip`, no scan runs, as for a
//     cursor search; only rows outside the model (quarantined: decided by their exact distances) can count.
//   T = NaN (none) or +inf: no row inside the model is beyond it; in_hi = the largest finite key, out_hi = all ones.
//   C.none(): T = -inf, or L2 with T < 0 -- at the cursor end the same value means "every row follows", here it means
//     every row inside the model is beyond T (d_i is finite resp. d_i >= 0 > T): `skip` as well.
// A key that is +inf or NaN (not inside the model: at or above COUNT_KEY_INF) is never IN and never OUT: in_hi stays
// below COUNT_KEY_INF and the kernel tests OUT only below it (count_window_class is the one definition of the classes;
// the kernel's three compares are its body).
#pragma once
#include <cmath>
#include <cstdint>

#include "tsh_after_band.h"

namespace tsh {

constexpr uint32_t COUNT_KEY_INF = 0xFF800000u;  // after_f2key(+inf): keys at or above it stand for no finite value

struct CountWindow {
  uint32_t in_lo = 1, in_hi = 0;            // IN: in_lo <= key <= in_hi (empty when in_lo > in_hi)
  uint32_t out_lo = 0, out_hi = 0xFFFFFFFFu;  // OUT: key < out_lo or out_hi < key < COUNT_KEY_INF
  bool skip = false;                        // no row inside the model can count: no scan, no window pass
};

enum CountClass { COUNT_IN = 0, COUNT_OUT = 1, COUNT_AMBIGUOUS = 2 };
inline CountClass count_window_class(const CountWindow &w, uint32_t key) {
  if (key >= w.in_lo && key <= w.in_hi) return COUNT_IN;
  if (key < w.out_lo || (key > w.out_hi && key < COUNT_KEY_INF)) return COUNT_OUT;
  return COUNT_AMBIGUOUS;
}

// -0.0 and +0.0 are one threshold (the predicate is IEEE >): the band is taken of +0.0
inline double count_threshold(double thr) { return thr == 0.0 ? 0.0 : thr; }

// has_cursor / after_dist: the cursor, if any; thr: the threshold as the caller gave it (NaN: none).  The other
// arguments are after_floor()'s.
inline CountWindow count_window(int metric, int dim, float eps_rel, float delta_abs, double mag_a, bool has_cursor,
                                double after_dist, double thr) {
  CountWindow w;
  if (has_cursor && !(after_dist < INFINITY)) {  // +inf or NaN
    w.skip = true;
    return w;
  }
  uint32_t in_lo = 0;
  if (has_cursor && after_dist != -INFINITY) {
    const AfterFloor f = after_floor(metric, dim, eps_rel, delta_abs, mag_a, after_dist);
    if (!f.none()) {
      w.out_lo = f.lo;
      in_lo = f.hi + 1;  // (f.hi <= COUNT_KEY_INF: no wrap)
    }
  }
  uint32_t in_hi = COUNT_KEY_INF - 1;
  if (thr == thr && thr != INFINITY) {
    const AfterFloor c = after_floor(metric, dim, eps_rel, delta_abs, mag_a, count_threshold(thr));
    if (c.none()) {
      w.skip = true;
      return w;
    }
    w.out_hi = c.hi;
    if (c.lo == 0) return w;  // (nothing is below key 0: IN stays empty)
    in_hi = c.lo - 1 < in_hi ? c.lo - 1 : in_hi;
  }
  if (in_lo <= in_hi) {
    w.in_lo = in_lo;
    w.in_hi = in_hi;
  }
  return w;
}

// The exact predicate, as the finaliser applies it to a row's f64 distance: the threshold by IEEE > (a NaN threshold
// is none, a NaN distance passes any), the cursor by after_follows (cursor_key = after_order_key(D)); from_start: no
// cursor, or D = -inf.
inline bool count_passes(double thr, bool from_start, uint64_t cursor_key, int64_t cursor_id, double d, int64_t id) {
  if (thr == thr && d > thr) return false;
  return from_start || after_follows(cursor_key, cursor_id, after_order_key(d), id);
}

}  // namespace tsh
