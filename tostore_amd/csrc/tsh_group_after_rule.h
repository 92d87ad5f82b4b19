// tsh_group_after_rule.h -- the rules of a grouped cursor search (tsh_search_grouped_after) and of a group count
// (tsh_search_grouped_count), include/tostore_hip.h.  Pure arithmetic, no HIP: compiled into the library (the kernels of
// tsh_group.hip.h use the functions marked TSH_GROUP_HD as they stand) and, on its own, by
// tests/cpp/group_after_rule_test.cpp.  It builds on tsh_group_rule.h (L, G, HEAD, SIDE, the band lemma), on
// tsh_after_band.h (the cursor's floor keys lo <= hi) and on tsh_count_band.h (the count's window), all unchanged.
//
// The specification.  G as in tsh_group_rule.h: L without every entry whose group occurred earlier.  A grouped cursor
// search returns the first k entries of G that follow the cursor (D, id) strictly (Dart double.compareTo, ties by id); a
// group count is the number of entries of G that follow it (all of them without a cursor).  An entry of G is its group's
// exact best row b -- the first row of the group in L -- so a group whose b is at or before the cursor is CONSUMED: none
// of its rows may appear, those after the cursor included.  That is why the rule is not "floor, then group": flooring the
// rows first would make the best of the remaining rows the group's head, and the group would come back.
//
// What the device does.  The head table (G1, group_min_kernel) is built over ALL live rows, whatever the cursor.  With h
// the key of a group's head (an ungrouped row is its own head) two facts hold for the group's exact best b:
//   (i)  b orders at or before the head (it is the best);        (ii) key(b) >= h (the head has the smallest key).
// The group is classified by h against the floor keys (group_after_class):
//   AFTER      h > hi, h a finite key.  The head is certainly after the cursor; by (ii) key(b) > hi, so b is too.  The
//              head stays in the heads array for select and re-rank; the group's other rows are SIDE by group_side, as in
//              a grouped search without a cursor.
//   BEFORE     h < lo.  The head is certainly before the cursor, by (i) so is b: the group is consumed.  The head becomes
//              KEY_DEAD in the heads array and no row of the group goes anywhere.
//   AMBIGUOUS  lo <= h <= hi, or h not a finite key.  The head becomes KEY_DEAD in the heads array and its id goes to the
//              side list; every other live row of the group with  key <= band_of(h)  goes there too, with no select-band
//              condition.  By (i) and the band lemma key(b) <= band_of(h): b is among them, and the finaliser decides.
// Why the candidates (the select's heads at or below band_of(tau), the SIDE rows, the side list) hold the answer, points
// 1-4 of tsh_group_rule.h restated:
//   1. tau is taken over the heads array, which holds heads of AFTER groups only: the k heads at or below tau belong to k
//      distinct groups none of which is consumed;
//   2. each of those groups has its exact best at or before its head and after the cursor, so the k-th entry of "G after
//      the cursor" orders at or before the farthest of the k heads, a row with a key of at most tau;
//   3. every row of the answer orders at or before that k-th entry: its key is at most band_of(tau).  It is its group's
//      exact best.  In an AFTER group it orders at or before its head, so it is a head the select takes or a SIDE row; in
//      an AMBIGUOUS group it is on the side list (above); it is never in a BEFORE group, which is consumed;
//   4. every candidate is a live row of L.  Among the candidates of an AMBIGUOUS group the first in exact order is b
//      itself, so the finaliser's "first entry decides" is the specification.  Every row of an AFTER group follows the
//      cursor (its key is above hi), so the group's first candidate is kept: it is b where the group belongs in the answer
//      (point 3) and otherwise orders at or after b, which orders after the k-th entry, and is cut.
// The same holds for ANY tau with at least k AFTER heads at or below it (the select's tile-minimum bound, its refined
// bound, the wide-band pass' radix bound -- that pass runs over the floored heads array) and for "no bound" (KEY_NAN:
// every AFTER head, every row at or below its head's band).  The side-list redo: the three passes draw places in one list
// through one count word; a list that overflowed is redone with room for the count it reported, and the same passes over
// the same keys report the same count.
//
// The count.  The same h against the window's four keys (group_count_class; count_window, tsh_count_band.h):
//   IN         in_lo <= h <= in_hi: the group counts 1.  The head passes the threshold and b orders at or before it, so
//              b passes too; key(b) >= h > F.hi, so b follows the cursor.
//   OUT        h < out_lo, or h beyond out_hi and finite: the group counts 0.  Either the head is certainly before the
//              cursor and so is b, or key(b) >= h > C.hi: b is beyond the threshold, and with it every row of the group.
//   AMBIGUOUS  the head and the group's live rows with key <= band_of(h) go to the side list; the finaliser counts the
//              distinct groups among them whose exact best passes count_passes (group_count_entries).
//
// Where the rule does not hold -- quarantined rows (outside the error model and not in the head table, yet able to be a
// group's best or to consume it) and groups with rows on several shards (one shard consumes, another offers) -- the job
// takes the exact-all route: every live row's exact sums reach the finaliser, whose two steps below ARE the specification.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <unordered_set>
#include <vector>

#include "tsh_count_band.h"
#include "tsh_finalize.h"
#include "tsh_group_rule.h"

namespace tsh {

enum GroupAfterClass { GROUP_AFTER = 0, GROUP_BEFORE = 1, GROUP_AMBIGUOUS = 2 };
constexpr uint32_t GROUP_KEY_INF = 0xFF800000u;  // f2key(+inf): COUNT_KEY_INF; keys at or above it stand for no finite value

// a group by its head's key h against the cursor's floor keys (after_floor; lo == hi == 0: no floor, every group AFTER)
TSH_GROUP_HD int group_after_class(uint32_t h, uint32_t lo, uint32_t hi) {
  if (lo == 0u && hi == 0u) return GROUP_AFTER;
  if (h < lo) return GROUP_BEFORE;
  return h > hi && h < GROUP_KEY_INF ? GROUP_AFTER : GROUP_AMBIGUOUS;
}
// a live grouped row that is not its group's head: does it go to the side list?  cls: its group's class; head_band:
// band_of(key of its group's head); select_band: the band the select left (KEY_NAN: no bound)
TSH_GROUP_HD bool group_after_side(int cls, uint32_t key, uint32_t head_band, uint32_t select_band) {
  if (cls == GROUP_BEFORE) return false;
  if (cls == GROUP_AMBIGUOUS) return key <= head_band;
  return group_side(key, head_band, select_band);
}
// a group by its head's key against the count's window: COUNT_IN / COUNT_OUT / COUNT_AMBIGUOUS (count_window_class's body)
TSH_GROUP_HD int group_count_class(uint32_t h, uint32_t in_lo, uint32_t in_hi, uint32_t out_lo, uint32_t out_hi) {
  if (h >= in_lo && h <= in_hi) return 0;
  if (h < out_lo || (h > out_hi && h < GROUP_KEY_INF)) return 1;
  return 2;
}

// The finaliser's step of a grouped cursor search: hits in ascending (order key, id) order, the threshold applied already.
// The first entry of each group decides the group -- kept iff it follows the cursor -- and every later entry of the group is
// skipped either way; cut to k.  from_start: no cursor to apply.  Writes positions into `hits`; -> how many
inline size_t group_first_cut_after(const Hit *hits, size_t n, size_t k, const GroupTable &t, bool from_start, const Hit &cur,
                                    std::vector<uint32_t> *keep) {
  keep->clear();
  if (k == 0) return 0;
  std::unordered_set<int32_t> seen;
  seen.reserve(std::min(n, (size_t)4096) * 2 + 1);
  for (size_t i = 0; i < n && keep->size() < k; ++i) {
    const int32_t g = t.at(hits[i].id);
    if (g >= 0 && !seen.insert(g).second) continue;
    if (!from_start && !after_follows(cur.key, cur.id, hits[i].key, hits[i].id)) continue;
    keep->push_back((uint32_t)i);
  }
  return keep->size();
}

// finalize_grouped's sibling with a cursor (after: never NULL; "-inf with any id" is from the start and gives
// finalize_grouped's answer bit for bit)
inline int32_t finalize_grouped_after(int metric, int dim, const float *query, int32_t k, double thr, const EntryList *lists, size_t n_lists,
                                      const GroupTable &t, const Cursor &after, int64_t *out_ids, double *out_dist, int32_t *out_group) {
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
  const size_t r = group_first_cut_after(hits.data(), hits.size(), kk, t, after.from_start(), after.hit(), &keep);
  for (size_t i = 0; i < r; ++i) {
    const Hit &h = hits[keep[i]];
    out_ids[i] = h.id;
    out_dist[i] = dart_order_key_to_double(h.key);
    if (out_group) out_group[i] = t.at(h.id);
  }
  for (size_t i = r; i < kk; ++i) {  // unused slots read as "no row", as finalize_grouped leaves them
    out_ids[i] = -1;
    out_dist[i] = std::nan("");
    if (out_group) out_group[i] = -1;
  }
  return (int32_t)r;
}

// The group-count step: the threshold first, as finalize_grouped_after applies it (a NaN distance passes any threshold and
// orders last: a group may be represented by such a row), then how many distinct groups among the entries left have a
// first entry in (distance, id) order that follows the cursor (count_passes; after: NULL for none).  The lists may come
// from any number of shards: the step runs once over all of them
inline int64_t group_count_entries(int metric, int dim, const float *query, double thr, const EntryList *lists, size_t n_lists,
                                   const GroupTable &t, const Cursor *after) {
  const double sqrt_mag_a = metric != TSH_METRIC_COSINE ? 0.0 : std::sqrt(query_mag_a(query, dim));
  static thread_local std::vector<Hit> hits;
  static thread_local std::vector<double> dist;
  hits.clear();
  for (size_t l = 0; l < n_lists; ++l) {
    if (dist.size() < lists[l].second) dist.resize(lists[l].second);
    final_distances(metric, lists[l].first, lists[l].second, sqrt_mag_a, dist.data());
    for (uint32_t i = 0; i < lists[l].second; ++i)
      if (count_passes(thr, true, 0, 0, dist[i], lists[l].first[i].id)) hits.push_back(Hit{dart_order_key(dist[i]), lists[l].first[i].id});
  }
  sort_hits(hits.data(), hits.size());
  const bool from_start = !after || after->from_start();
  const Hit cur = after ? after->hit() : Hit{0, 0};
  std::unordered_set<int32_t> seen;
  int64_t n = 0;
  for (const Hit &h : hits) {
    const int32_t g = t.at(h.id);
    if (g >= 0 && !seen.insert(g).second) continue;
    if (from_start || after_follows(cur.key, cur.id, h.key, h.id)) ++n;
  }
  return n;
}

}  // namespace tsh
