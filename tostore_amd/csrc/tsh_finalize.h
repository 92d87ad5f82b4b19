// tsh_finalize.h -- the finaliser: what decides the order of every result the library returns.  From candidate
// entries (exact f64 sums, tsh_block.h) to distances, threshold, cursor, order and cut -- and the cursors of a call.
// Pure host arithmetic, no HIP: compiled into the library and, on its own, by tests/cpp/finalize_test.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/tostore_hip.h"
#include "tsh_after_band.h"
#include "tsh_block.h"
#include "tsh_count_band.h"

namespace tsh {

// ---- Dart double.compareTo ([external] Dart SDK): NaN greatest (and equal to itself), -0 < +0 ------
// double.compareTo as an integer order: key(a) < key(b)  <=>  dart_compare(a, b) < 0, equal keys <=> compareTo == 0
// (every NaN maps to the one largest key; -0.0 sorts just below +0.0).  Sorting (key, id) pairs with integer
// compares is what the finaliser does for every query.
// (the function itself lives in tsh_after_band.h, where tests/cpp/after_band_test.cpp holds it to the order)
inline uint64_t dart_order_key(double d) { return after_order_key(d); }
struct Hit {
  uint64_t key;  // dart_order_key(distance)
  int64_t id;
};
inline bool hit_less(const Hit &a, const Hit &b) { return a.key != b.key ? a.key < b.key : a.id < b.id; }
// The cursor of a search-after (tsh_search_after): the last (distance, id) the caller saw.  A row follows it iff its
// (order key, id) is strictly greater
struct Cursor {
  double dist = 0;
  int64_t id = 0;
  Hit hit() const { return Hit{dart_order_key(dist), id}; }
  bool from_start() const { return dist == -INFINITY; }  // "-inf with any id": nothing is at or before it
};
// A cursor per query of a call (tsh_search_after and its kin: the caller's two arrays), or none.  A further per-query
// input of the searches belongs here
struct Cursors {
  const double *dist = nullptr;
  const int64_t *id = nullptr;
  explicit operator bool() const { return dist != nullptr; }
  // the same view for queries [q0, ...) of the call
  Cursors from(int64_t q0) const { return dist ? Cursors{dist + q0, id + q0} : Cursors{}; }
  // query q's cursor: fills *tmp and returns it; NULL when the call has no cursors
  const Cursor *at(int64_t q, Cursor *tmp) const {
    if (!dist) return nullptr;
    tmp->dist = dist[q];
    tmp->id = id[q];
    return tmp;
  }
};
// the _masked entries' cursor is optional: both arrays or neither
inline bool half_cursor(const double *after_dist, const int64_t *after_id) { return (after_dist == nullptr) != (after_id == nullptr); }

// Ascending by (key, id).  A query's candidates are k plus a band's worth of rows whose distances share their
// leading bits, and std::sort spends 3-4 us on 127 of them (two thirds of a query's finalisation, mostly
// mispredicted branches): one counting pass over 512 buckets of the key RANGE (a shift, so the bucket is monotone in
// the key) leaves runs of a few entries to put in order -- 1 us.  Ties, NaNs or a wild range only mean longer runs.
inline void sort_hits(Hit *h, size_t n) {
  constexpr int BITS = 9, NB = 1 << BITS;
  if (n < 24 || n > 60000) {
    std::sort(h, h + n, hit_less);
    return;
  }
  static thread_local std::vector<Hit> tmp;
  static thread_local std::vector<uint16_t> bucket;
  if (tmp.size() < n) {
    tmp.resize(n);
    bucket.resize(n);
  }
  uint64_t kmin = ~0ull, kmax = 0;
  for (size_t i = 0; i < n; ++i) {
    kmin = std::min(kmin, h[i].key);
    kmax = std::max(kmax, h[i].key);
  }
  const uint64_t range = kmax - kmin;
  const int shift = range < (uint64_t)NB ? 0 : (64 - __builtin_clzll(range)) - BITS;  // (range >> shift) < NB
  uint16_t pos[NB + 1];
  memset(pos, 0, sizeof(pos));
  for (size_t i = 0; i < n; ++i) {
    const uint16_t b = (uint16_t)((h[i].key - kmin) >> shift);
    bucket[i] = b;
    pos[b + 1]++;
  }
  for (int b = 0; b < NB; ++b) pos[b + 1] += pos[b];
  for (size_t i = 0; i < n; ++i) tmp[pos[bucket[i]]++] = h[i];
  size_t start = 0;
  for (size_t i = 1; i <= n; ++i) {
    if (i < n && ((tmp[i].key - kmin) >> shift) == ((tmp[start].key - kmin) >> shift)) continue;
    const size_t len = i - start;  // a bucket's run
    if (len > 12) {
      std::sort(tmp.begin() + start, tmp.begin() + i, hit_less);
    } else {
      for (size_t a = start + 1; a < i; ++a) {
        const Hit x = tmp[a];
        size_t j = a;
        for (; j > start && hit_less(x, tmp[j - 1]); --j) tmp[j] = tmp[j - 1];
        tmp[j] = x;
      }
    }
    start = i;
  }
  memcpy(h, tmp.data(), n * sizeof(Hit));
}
// the distance an order key stands for (every NaN comes back as the one quiet NaN)
inline double dart_order_key_to_double(uint64_t key) {
  if (key == ~0ull) return std::nan("");
  const uint64_t b = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
  double d;
  memcpy(&d, &b, 8);
  return d;
}

// Final per-candidate arithmetic of ngh_graph_engine.dart:908-946 given the exact f64 sums (L2 :926 sqrt(s0);
// IP :914 -s0; cosine :944-945,:916 1 - s0 / (sqrt(mag_a) * sqrt(s1)), similarity 0 when the denominator is not
// positive), mag_a = sum q[i]*q[i] accumulated in element order --
// over a whole list: a plain loop over arrays, so the compiler's vector square roots and
// divisions (IEEE-exact, like the scalar ones; no contraction: -ffp-contract=off) do four or eight at a time on
// hosts that have AVX2 / AVX-512 -- the square root and the division were a third of a query's finalisation.
#define TSH_FINAL_KEYS_BODY                                                                   \
  for (uint32_t i = 0; i < n; ++i) {                                                          \
    const double s0 = e[i].s0, s1 = e[i].s1;                                                  \
    double d;                                                                                 \
    if (metric == TSH_METRIC_L2) {                                                            \
      d = std::sqrt(s0);                                                                      \
    } else if (metric == TSH_METRIC_IP) {                                                     \
      d = -s0;                                                                                \
    } else {                                                                                  \
      const double denom = sqrt_mag_a * std::sqrt(s1);                                        \
      const double sim = denom > 0 ? s0 / denom : 0;                                          \
      d = 1.0 - sim;                                                                          \
    }                                                                                         \
    dist[i] = d;                                                                              \
  }
#if defined(__x86_64__)
__attribute__((target("avx2"))) inline void final_distances_avx2(int metric, const BlockEntry *e, uint32_t n, double sqrt_mag_a,
                                                                 double *dist) {
  TSH_FINAL_KEYS_BODY
}
#endif
inline void final_distances_base(int metric, const BlockEntry *e, uint32_t n, double sqrt_mag_a, double *dist) {
  TSH_FINAL_KEYS_BODY
}
#undef TSH_FINAL_KEYS_BODY
inline void final_distances(int metric, const BlockEntry *e, uint32_t n, double sqrt_mag_a, double *dist) {
#if defined(__x86_64__)
  static const bool avx2 = __builtin_cpu_supports("avx2");
  if (avx2) return final_distances_avx2(metric, e, n, sqrt_mag_a, dist);
#endif
  final_distances_base(metric, e, n, sqrt_mag_a, dist);
}

inline double query_mag_a(const float *q, int dim) {
#pragma clang fp contract(off)
  double m = 0;
  for (int i = 0; i < dim; ++i) m = m + (double)q[i] * (double)q[i];
  return m;
}

// threshold + order + cut of ngh_graph_engine.dart:127,133-134 over candidate
// entries from any number of blocks.  mag_a: query_mag_a(query) when the caller has it already (the batched path
// computes it while it prepares the queries), else nullptr.  after: a cursor search's cursor -- entries at or before it
// are dropped first, wherever they came from -- else nullptr.
inline int32_t finalize_query(int metric, int dim, const float *query, int32_t k, double thr, const EntryList *lists_p,
                              size_t n_lists, int64_t *out_ids, double *out_dist, const double *mag_a_known = nullptr,
                              const Cursor *after = nullptr) {
  struct {
    const EntryList *b, *e;
    const EntryList *begin() const { return b; }
    const EntryList *end() const { return e; }
  } lists{lists_p, lists_p + n_lists};
  const double mag_a = metric != TSH_METRIC_COSINE ? 0.0 : (mag_a_known ? *mag_a_known : query_mag_a(query, dim));
  const double sqrt_mag_a = std::sqrt(mag_a);
  static thread_local std::vector<Hit> hits;  // (one allocation per thread, not per query)
  static thread_local std::vector<double> dist;
  hits.clear();
  size_t total = 0;
  for (auto &l : lists) total += l.second;
  hits.reserve(total);
  const bool has_thr = !std::isnan(thr);
  if (after && after->from_start()) after = nullptr;
  const Hit cur = after ? after->hit() : Hit{0, 0};
  for (auto &l : lists) {
    if (dist.size() < l.second) dist.resize(l.second);
    final_distances(metric, l.first, l.second, sqrt_mag_a, dist.data());
    for (uint32_t i = 0; i < l.second; ++i) {
      const double d = dist[i];
      const Hit h{dart_order_key(d), l.first[i].id};
      if (after && !after_follows(cur.key, cur.id, h.key, h.id)) continue;
      if (has_thr && d > thr) continue;
      hits.push_back(h);
    }
  }
  size_t r = std::min<size_t>(hits.size(), (size_t)std::max(k, 0));
  if (hits.size() <= 4 * r) {  // the usual case (k + a band's worth of candidates): one sort is cheapest
    sort_hits(hits.data(), hits.size());
  } else {
    std::nth_element(hits.begin(), hits.begin() + r, hits.end(), hit_less);
    std::sort(hits.begin(), hits.begin() + r, hit_less);
  }
  for (size_t i = 0; i < r; ++i) {
    out_ids[i] = hits[i].id;
    out_dist[i] = dart_order_key_to_double(hits[i].key);
  }
  for (size_t i = r; i < (size_t)std::max(k, 0); ++i) {  // unused slots read as "no row" (callers need not pre-fill)
    out_ids[i] = -1;
    out_dist[i] = std::nan("");
  }
  return (int32_t)r;
}
inline int32_t finalize_query(int metric, int dim, const float *query, int32_t k, double thr,
                              const std::vector<EntryList> &lists, int64_t *out_ids, double *out_dist,
                              const Cursor *after = nullptr) {
  return finalize_query(metric, dim, query, k, thr, lists.data(), lists.size(), out_ids, out_dist, nullptr, after);
}

// A count's share of the finaliser (tsh_search_count): how many of the entries pass the threshold and follow the cursor
// -- finalize_query's distances and predicate (count_passes, tsh_count_band.h), no order, no cut
inline int64_t count_entries(int metric, int dim, const float *query, double thr, const EntryList *lists, size_t n_lists, const Cursor *after) {
  const double sqrt_mag_a = metric != TSH_METRIC_COSINE ? 0.0 : std::sqrt(query_mag_a(query, dim));
  static thread_local std::vector<double> dist;
  const bool from_start = !after || after->from_start();
  const Hit cur = after ? after->hit() : Hit{0, 0};
  int64_t n = 0;
  for (size_t l = 0; l < n_lists; ++l) {
    if (dist.size() < lists[l].second) dist.resize(lists[l].second);
    final_distances(metric, lists[l].first, lists[l].second, sqrt_mag_a, dist.data());
    for (uint32_t i = 0; i < lists[l].second; ++i)
      if (count_passes(thr, from_start, cur.key, cur.id, dist[i], lists[l].first[i].id)) ++n;
  }
  return n;
}

}  // namespace tsh
