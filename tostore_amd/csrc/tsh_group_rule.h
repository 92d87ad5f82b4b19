// tsh_group_rule.h -- the rules of a grouped search (tsh_search_grouped, include/tostore_hip.h): the nearest row of each
// of the k nearest groups.  Pure arithmetic, no HIP: compiled into the library (the kernels of tsh_group.hip.h use the
// functions marked TSH_GROUP_HD as they stand) and, on its own, by tests/cpp/group_rule_test.cpp.
//
// The specification.  L: the list tsh_search returns for k = infinity (mask, tombstones, gaps, quarantined rows and the
// threshold applied; ordered by Dart double.compareTo on the distance, ties by row id).  A row's group is its entry of the
// caller's array; a negative entry, or a row beyond the array, is UNGROUPED: a group of its own.  G = L without every entry
// whose group occurred earlier in L; the answer is G's first k entries.
//
// What the device does with the f32 keys the scan left (one per live row; DESIGN.md section 4's band lemma: a row that
// orders at or before a row with key t has a key of at most band_of(t)):
//   HEAD   the row of a group with the smallest word  key << 32 | position  (group_head_word): smallest key, ties by
//          position -- which is id order, in tile scans and list scans alike.  An ungrouped row is its own head.  One
//          head per group: the k-th smallest head key tau names k DISTINCT groups.
//   SIDE   a live grouped row that is not the head, with  key <= band_of(its head's key)  and  key <= band_of(tau)
//          (group_side).  Its exact sums are taken beside the select's candidates (the heads at or below band_of(tau)).
// Why these candidates hold every row of the answer:
//   1. the k heads at or below tau belong to k distinct groups;
//   2. each of those groups has its exact best at or before its head, so G's k-th entry orders at or before the farthest
//      of the k heads, a row with a key of at most tau;
//   3. every row of the answer orders at or before G's k-th entry: its key is at most band_of(tau) (the lemma, band_of
//      monotone).  It is its group's exact best, so it orders at or before its group's head too: its key is at most
//      band_of(head key).  So it is a head the select takes, or a SIDE row;
//   4. a candidate of a group that does not belong in the answer orders after G's k-th entry -- every candidate is a live
//      row of L, and the finaliser's step below keeps the first of each group among exact distances -- and is cut.
// The same holds for ANY tau with at least k heads at or below it (the select's tile-minimum bound, its refined bound,
// the wide-band pass' radix bound) and for "no bound" (KEY_NAN: every head, every row at or below its head's band).
// Quarantined rows (outside the error model) always reach the finaliser with their exact sums; safe mode hands it every
// live row.  The finaliser (group_first_cut) then IS the specification over the candidates.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <unordered_set>
#include <vector>

#include "tsh_finalize.h"

#if defined(__HIPCC__)
#define TSH_GROUP_HD __host__ __device__ __forceinline__
#else
#define TSH_GROUP_HD inline
#endif

namespace tsh {

constexpr int32_t GROUP_MAX_GROUPS = 1 << 26;      // 8 B of head table per group and context: 512 MB at the limit
constexpr uint64_t GROUP_WORD_NONE = ~0ull;        // a group no live row was seen in (the table reads all-ones before a job)
constexpr uint32_t GROUP_KEY_DEAD = 0xFFFFFFFFu;   // KEY_DEAD / KEY_NAN of tsh_kernels.hip.h
constexpr uint32_t GROUP_KEY_NAN = 0xFFFFFFFEu;

// the head word: the minimum over a group's live rows does not depend on the order they arrive in
TSH_GROUP_HD uint64_t group_head_word(uint32_t key, uint32_t position) { return ((uint64_t)key << 32) | (uint64_t)position; }
TSH_GROUP_HD uint32_t group_word_key(uint64_t word) { return (uint32_t)(word >> 32); }
// an entry of the caller's array as the kernels see it: below 0, or at or beyond the table, is ungrouped
TSH_GROUP_HD bool group_valid(int32_t group, int32_t n_groups) { return (uint32_t)group < (uint32_t)n_groups; }
// a live row is its group's head iff the table holds its own word (ungrouped: always)
TSH_GROUP_HD bool group_is_head(bool grouped, uint64_t word, uint64_t table_word) { return !grouped || word == table_word; }
// the two-condition side predicate, for a live grouped row that is not the head.  head_band: band_of(key of its group's
// head); select_band: the band the select left in the block's header (KEY_NAN: no bound)
TSH_GROUP_HD bool group_side(uint32_t key, uint32_t head_band, uint32_t select_band) { return key <= head_band && key <= select_band; }

// host copies of f2key / key2f / band_of (tsh_kernels.hip.h): tau widened by the error band, rounded up
inline uint32_t group_f2key(float f) {
  if (f != f) return GROUP_KEY_NAN;
  uint32_t b;
  memcpy(&b, &f, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float group_key2f(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float f;
  memcpy(&f, &b, 4);
  return f;
}
inline uint32_t group_band_of(uint32_t tau_key, float eps_rel, float delta_abs) {
  if (tau_key >= GROUP_KEY_NAN) return GROUP_KEY_NAN;
  const float t = group_key2f(tau_key);
  if (t == INFINITY) return GROUP_KEY_NAN;
  const double w = (double)t + std::fabs((double)t) * (double)eps_rel + (double)delta_abs;
  float f = (float)w;
  if ((double)f < w) f = std::nextafter(f, INFINITY);
  if (!(f < INFINITY)) return GROUP_KEY_NAN;
  return group_f2key(f);
}

// The caller's array as the finaliser reads it: entry of GLOBAL row id, -1 for "ungrouped"
struct GroupTable {
  const int32_t *group_of = nullptr;
  int64_t n = 0;
  int32_t at(int64_t id) const {
    if (id < 0 || id >= n) return -1;
    const int32_t g = group_of[id];
    return g < 0 ? -1 : g;
  }
};

// The finaliser's step: hits in ascending (order key, id) order, the threshold applied already -> the first entry of each
// group (ungrouped rows are distinct), cut to k.  Writes positions into `hits`; -> how many
inline size_t group_first_cut(const Hit *hits, size_t n, size_t k, const GroupTable &t, std::vector<uint32_t> *keep) {
  keep->clear();
  if (k == 0) return 0;
  std::unordered_set<int32_t> seen;
  seen.reserve(std::min(n, k) * 2 + 1);
  for (size_t i = 0; i < n && keep->size() < k; ++i) {
    const int32_t g = t.at(hits[i].id);
    if (g >= 0 && !seen.insert(g).second) continue;
    keep->push_back((uint32_t)i);
  }
  return keep->size();
}

// finalize_query's grouped sibling: distances, threshold and order as there, then group_first_cut.  The lists may come
// from any number of shards -- groups span shards, so the step runs once over all of them.  out_group: nullable
inline int32_t finalize_grouped(int metric, int dim, const float *query, int32_t k, double thr, const EntryList *lists, size_t n_lists,
                                const GroupTable &t, int64_t *out_ids, double *out_dist, int32_t *out_group) {
  const double sqrt_mag_a = metric != TSH_METRIC_COSINE ? 0.0 : std::sqrt(query_mag_a(query, dim));
  static thread_local std::vector<Hit> hits;
  static thread_local std::vector<double> dist;
  static thread_local std::vector<uint32_t> keep;
  hits.clear();
  const bool has_thr = !std::isnan(thr);
  for (size_t l = 0; l < n_lists; ++l) {
    if (dist.size() < lists[l].second) dist.resize(lists[l].second);
    final_distances(metric, lists[l].first, lists[l].second, sqrt_mag_a, dist.data());
    for (uint32_t i = 0; i < lists[l].second; ++i) {
      const double d = dist[i];
      if (has_thr && d > thr) continue;
      hits.push_back(Hit{dart_order_key(d), lists[l].first[i].id});
    }
  }
  sort_hits(hits.data(), hits.size());
  const size_t kk = (size_t)std::max(k, 0);
  const size_t r = group_first_cut(hits.data(), hits.size(), kk, t, &keep);
  for (size_t i = 0; i < r; ++i) {
    const Hit &h = hits[keep[i]];
    out_ids[i] = h.id;
    out_dist[i] = dart_order_key_to_double(h.key);
    if (out_group) out_group[i] = t.at(h.id);
  }
  for (size_t i = r; i < kk; ++i) {  // unused slots read as "no row", as finalize_query leaves them
    out_ids[i] = -1;
    out_dist[i] = std::nan("");
    if (out_group) out_group[i] = -1;
  }
  return (int32_t)r;
}

}  // namespace tsh
