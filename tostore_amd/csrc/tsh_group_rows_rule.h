// tsh_group_rows_rule.h -- the rules of a grouped search with several rows per group (tsh_search_grouped_rows,
// include/tostore_hip.h): the m nearest rows of each of the k nearest groups.  Pure arithmetic, no HIP: compiled into the
// library (the kernels of tsh_group_rows.hip.h use the functions marked TSH_GROUP_HD as they stand) and, on its own, by
// tests/cpp/group_rows_rule_test.cpp.  It builds on tsh_group_rule.h, whose L, G, HEAD, band lemma and steps 1 - 4 are
// taken as given.
//
// The specification.  The k winning groups are the groups of G's first k entries, in that order.  For the i-th winning
// group the answer holds the first m entries of L that belong to it, in L's order (an ungrouped row is a group of one row;
// a group with fewer than m rows in L gives what it has).
//
// What the device does behind G1, G2, the select over the heads and the re-rank, which leave band_key = band_of(tau) in
// the block's header with at least k heads at or below tau:
//   MARKED   a group whose head key is at or below band_key (group_rows_marked).  A winning group's exact best row has a
//            key of at most band_of(tau) (tsh_group_rule.h, step 3); the head has the group's smallest key; so every
//            winning group is marked.  Usually k groups plus a handful.  An ungrouped head needs no mark: its one row is
//            a candidate of the select already.
//   MEMBER   a live row of a marked group g with  key <= band_of(tau_g),  tau_g the m-th smallest key among g's live rows
//            (group_rows_member); every live row where g has at most m of them (group_rows_takes_all).
// Why the members hold every row of the answer.  Let g be a winning group with more than m live rows.  m rows of g have
// keys of at most tau_g, so the m-th entry of L that belongs to g orders at or before the farthest of those m rows: a row
// with a key of at most tau_g.  Every one of g's first m entries in L orders at or before that entry, so by the band
// lemma its key is at most band_of(tau_g).  (A row the threshold cuts is a candidate that the finaliser drops; the
// threshold only shortens L from its far end, so it moves none of the first m that survive.)
// The members take the place of G3's SIDE rows: tau_g is at least the head's key, so band_of(tau_g) >= band_of(head key),
// and a SIDE row's group is marked (its key is at or below band_key, its head's key no larger).  The head of a marked
// group is a member too and may be a candidate of the select as well: the finaliser's step drops the second copy of a row
// (equal id: equal sums, so the copies are neighbours in the order).
// The same holds for ANY tau with at least k heads at or below it and for "no bound" (KEY_NAN marks every group).
//
// Where the per-shard rule does not hold: exactly where the grouped cursor search's does not (tsh_group_after_rule.h), by
// the same predicate.  A handle over several devices whose groups span two shards' row ranges -- a winning group's second
// row can lie on a shard where the group's head is far above that shard's band, so the group is never marked there
// (tests/cpp/group_rows_rule_test.cpp carries the counter-example) -- and a shard with a live quarantined row, through
// which a group can win without a head in the table.  Such calls, safe mode, and a job that marked more groups than it has
// slots for take the EXACT-ALL route: a plain search job whose every live row reaches the finaliser with its exact sums.
// The finaliser's step (group_rows_cut) then IS the specification over the candidates.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "tsh_group_rule.h"

namespace tsh {

constexpr int32_t GROUP_ROWS_MAX = 64;  // rows per group of one call: an interface limit

// ---- the slots of the marked groups ----------------------------------------------------------------------------------
// A marked group's word of the head table is overwritten by a SLOT word: the key field all-ones (no live row has the key
// KEY_DEAD, so no head word looks like it) and the slot below.  GROUP_WORD_NONE is no slot word: its slot is never below a
// capacity, which stays under 2^31.
TSH_GROUP_HD uint64_t group_slot_word(uint32_t slot) { return 0xFFFFFFFF00000000ull | (uint64_t)slot; }
TSH_GROUP_HD bool group_word_is_slot(uint64_t word, uint32_t slot_cap) {
  return (uint32_t)(word >> 32) == 0xFFFFFFFFu && (uint32_t)word < slot_cap;
}
TSH_GROUP_HD uint32_t group_word_slot(uint64_t word) { return (uint32_t)word; }
// a head that marks its group: grouped, and its key at or below the band the select left (KEY_NAN: no bound)
TSH_GROUP_HD bool group_rows_marked(bool grouped_head, uint32_t head_key, uint32_t band_key) { return grouped_head && head_key <= band_key; }
// a marked group with at most m live rows sends all of them on
TSH_GROUP_HD bool group_rows_takes_all(uint32_t n_live, uint32_t m) { return n_live <= m; }
// ... a larger one the rows at or below band_of(tau_g)
TSH_GROUP_HD bool group_rows_member(uint32_t key, uint32_t tau_g_band) { return key <= tau_g_band; }
// One step of the radix select for tau_g: hist[256] counts the segment's keys that agree with the digits found so far, by
// the next digit down.  -> the digit holding the *remaining-th smallest of them (1-based), *remaining reduced to its rank
// inside that digit.  The caller guarantees 1 <= *remaining <= the histogram's total
TSH_GROUP_HD uint32_t group_rows_radix_digit(const uint32_t *hist, uint32_t *remaining) {
  uint32_t cum = 0, b = 0;
  for (; b < 255u; ++b) {
    if (cum + hist[b] >= *remaining) break;
    cum += hist[b];
  }
  *remaining -= cum;
  return b;
}
// the slots of a job: k winning groups and as many again beside them, plus a floor for small k.  More marked groups than
// that -- no bound at all, or heads tied at tau by the hundred -- and the job runs again on the exact-all route
inline int64_t group_rows_slots(int32_t k) { return 2 * (int64_t)std::max(k, 0) + 64; }

// host model of the pick: the m-th smallest key (1-based, m <= n) by the radix steps above, as the kernel takes them
inline uint32_t group_rows_mth_key(const uint32_t *keys, size_t n, uint32_t m) {
  uint32_t prefix = 0, remaining = m;
  for (int shift = 24; shift >= 0; shift -= 8) {
    uint32_t hist[256] = {0};
    const uint32_t mask = shift == 24 ? 0u : ~0u << (shift + 8);
    for (size_t i = 0; i < n; ++i)
      if ((keys[i] & mask) == prefix) ++hist[(keys[i] >> shift) & 255u];
    prefix |= group_rows_radix_digit(hist, &remaining) << shift;
  }
  return prefix;
}

// ---- the finaliser's step ---------------------------------------------------------------------------------------------
struct GroupRowsKeep {
  uint32_t hit;     // position in `hits`
  uint32_t winner;  // which winning group, in the answer's order
};
// hits in ascending (order key, id) order, the threshold applied already; a row may occur twice (neighbours then).  The
// first k distinct groups win (ungrouped rows are distinct); every later hit of a winning group is kept until that group
// has m; a candidate of any other group is cut.  keep: the kept hits in the order walked; rows[w] = rows kept for winner
// w.  -> the winners
inline size_t group_rows_cut(const Hit *hits, size_t n, size_t k, size_t m, const GroupTable &t, std::vector<GroupRowsKeep> *keep,
                             std::vector<uint32_t> *rows) {
  keep->clear();
  rows->clear();
  if (k == 0 || m == 0) return 0;
  std::unordered_map<int32_t, uint32_t> winner_of;
  winner_of.reserve(std::min(n, k) * 2 + 1);
  size_t full = 0;  // winners that hold m rows already (an ungrouped winner is full at once)
  for (size_t i = 0; i < n && !(rows->size() == k && full == k); ++i) {
    if (i > 0 && hits[i].id == hits[i - 1].id) continue;  // the second copy of a row
    const int32_t g = t.at(hits[i].id);
    uint32_t w;
    if (g < 0) {
      if (rows->size() >= k) continue;
      w = (uint32_t)rows->size();
      rows->push_back(0);
      if (m > 1) ++full;  // (never another row: full whatever m is; m == 1 is counted below)
    } else {
      auto it = winner_of.find(g);
      if (it != winner_of.end()) {
        w = it->second;
        if ((*rows)[w] >= m) continue;
      } else {
        if (rows->size() >= k) continue;
        w = (uint32_t)rows->size();
        rows->push_back(0);
        winner_of.emplace(g, w);
      }
    }
    keep->push_back(GroupRowsKeep{(uint32_t)i, w});
    if (++(*rows)[w] == m) ++full;
  }
  return rows->size();
}

// finalize_grouped's sibling: distances, threshold and order as there, then group_rows_cut.  Slot (i, j) of the answer is
// out_ids / out_dist[i * m + j]; unused slots read id -1 and distance NaN, an unused group reads group -1 and rows 0.
// out_group, out_rows: nullable.  -> the groups returned
inline int32_t finalize_grouped_rows(int metric, int dim, const float *query, int32_t k, int32_t m, double thr, const EntryList *lists, size_t n_lists,
                                     const GroupTable &t, int64_t *out_ids, double *out_dist, int32_t *out_group, int32_t *out_rows) {
  const double sqrt_mag_a = metric != TSH_METRIC_COSINE ? 0.0 : std::sqrt(query_mag_a(query, dim));
  static thread_local std::vector<Hit> hits;
  static thread_local std::vector<double> dist;
  static thread_local std::vector<GroupRowsKeep> keep;
  static thread_local std::vector<uint32_t> rows;
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
  const size_t kk = (size_t)std::max(k, 0), mm = (size_t)std::max(m, 0);
  const size_t r = group_rows_cut(hits.data(), hits.size(), kk, mm, t, &keep, &rows);
  for (size_t i = 0; i < kk * mm; ++i) {
    out_ids[i] = -1;
    out_dist[i] = std::nan("");
  }
  for (size_t i = 0; i < kk; ++i) {
    if (out_group) out_group[i] = -1;
    if (out_rows) out_rows[i] = i < r ? (int32_t)rows[i] : 0;
  }
  std::fill(rows.begin(), rows.end(), 0u);  // (now: the next free place of each winner)
  for (const GroupRowsKeep &kp : keep) {
    const Hit &h = hits[kp.hit];
    const size_t at = (size_t)kp.winner * mm + rows[kp.winner]++;
    out_ids[at] = h.id;
    out_dist[at] = dart_order_key_to_double(h.key);
    if (out_group) out_group[kp.winner] = t.at(h.id);
  }
  return (int32_t)r;
}

}  // namespace tsh
