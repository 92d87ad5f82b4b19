"""Cost of tsh_search_grouped_after and tsh_search_grouped_count against what they replace and what they add to
(profiles/search_grouped_after_ab.json): 1 M x 768 f32, L2, groups of 8 consecutive rows drawn around a common centre (a near
group contributes many near rows), k = 10 and 100, 64-query calls, us per query.  One process, one library; the legs are
interleaved -- every round times every leg once -- and the medians over the rounds are reported.  Prints one JSON line
("AB ..."); with an output path it also writes the file.
  page 1 / 2 / 10   tsh_search_grouped_after from -inf, from the last entry of page 1, from the last entry of page 9
  grouped           tsh_search_grouped: the yardstick, the parent commit's code
  caller p1/p2/p10  what a caller does without the call: tsh_search_after pages of k from where the page before stopped,
                    repeated groups (of this page and every earlier one) dropped on the host, until k new groups were seen;
                    the state of the pages before is made outside the timed region
  group count       tsh_search_grouped_count without a cursor and past page 1, against tsh_search_count
usage: python tools/ab_search_grouped_after.py [ROUNDS] [OUT.json] [ROWS]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tostore_amd import HipVectorIndex  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else None
n, d, nq, per_group = (int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000), 768, 64, 8  # (fewer rows: a rehearsal of the script, not a measurement)
rng = np.random.default_rng(2027)
n_groups = n // per_group
group_of = (np.arange(n) // per_group).astype(np.int32)
rows = np.empty((n, d), np.float32)
for a in range(0, n_groups, 5000):  # (in pieces: the noise of the whole corpus at once is another 3 GB)
    b = min(a + 5000, n_groups)
    centres = rng.standard_normal((b - a, d), dtype=np.float32)
    rows[a * per_group:b * per_group] = np.repeat(centres, per_group, axis=0) + np.float32(0.3) * rng.standard_normal(((b - a) * per_group, d), dtype=np.float32)
qs = rng.standard_normal((nq, d), dtype=np.float32)
PAGES = (1, 2, 10)


def caller_page(idx, k, state):
    """The caller's loop for ONE more page of k new groups per query.  state = (cursor distances, cursor ids, seen groups
    per query) as the pages before left it; -> (the page's rows per query, the state after it, tsh_search_after calls made)"""
    cur_d, cur_i, seen = state[0].copy(), state[1].copy(), [set(s) for s in state[2]]
    page = [[] for _ in range(nq)]
    active = np.arange(nq)
    calls = 0
    while len(active):
        ids, dist, cnt = idx.search_after(qs[active], k, (cur_d[active], cur_i[active]))
        calls += 1
        still = []
        for j, q in enumerate(active):
            for t in range(cnt[j]):
                g = int(group_of[ids[j, t]])
                if g not in seen[q]:
                    seen[q].add(g)
                    page[q].append(int(ids[j, t]))
                cur_d[q], cur_i[q] = dist[j, t], ids[j, t]
                if len(page[q]) == k:  # (the row cursor stops at the page's last row: the next page goes on from there)
                    break
            if len(page[q]) < k and cnt[j] == k:
                still.append(q)
        active = np.asarray(still, np.int64)
    return page, (cur_d, cur_i, seen), calls


def once(fn):
    t0 = time.perf_counter()
    fn()  # returns finalised results: every query has been waited for
    return (time.perf_counter() - t0) * 1e6 / nq


out = {"what": f"tools/ab_search_grouped_after.py on one MI355X: {n} x 768 f32, L2, groups of 8 consecutive rows around a common centre; us per "
               "query of 64-query calls (host clock around calls that return their results); legs interleaved, medians over the rounds",
       "rounds": rounds}
with HipVectorIndex(d, 0, capacity_rows=n) as idx:
    idx.set_batch_min_nq(0)
    idx.append(0, rows)
    del rows
    with idx.make_groups(group_of, n_groups) as h:
        legs = {}
        checks = {}
        for k in (10, 100):
            # the cursors of pages 2 and 10, and the caller's states in front of them (untimed)
            cursors = {1: (np.full(nq, -np.inf), np.zeros(nq, np.int64))}
            states = {1: (np.full(nq, -np.inf), np.zeros(nq, np.int64), [set() for _ in range(nq)])}
            cd, ci = cursors[1]
            ok = True
            for p in range(1, max(PAGES) + 1):
                ids, dist, grp, cnt = idx.search_grouped_after(qs, k, h, (cd, ci))
                page, state, _ = caller_page(idx, k, states[p])
                ok = ok and all(list(ids[q, :cnt[q]]) == page[q] for q in range(nq))
                cd, ci = dist[np.arange(nq), cnt - 1].copy(), ids[np.arange(nq), cnt - 1].copy()
                cursors[p + 1], states[p + 1] = (cd, ci), state
            checks[f"k{k}_ten_pages_equal_the_callers"] = bool(ok)
            for p in PAGES:
                legs[f"grouped_after_k{k}_page{p}"] = (lambda k=k, p=p: idx.search_grouped_after(qs, k, h, cursors[p]))
                legs[f"caller_k{k}_page{p}"] = (lambda k=k, p=p: caller_page(idx, k, states[p]))
                checks[f"caller_k{k}_page{p}_search_after_calls"] = caller_page(idx, k, states[p])[2]
            legs[f"grouped_k{k}"] = (lambda k=k: idx.search_grouped(qs, k, h))
            if k == 10:
                legs["group_count"] = lambda: idx.count_groups(qs, h)
                legs["group_count_past_page1"] = (lambda c=cursors[2]: idx.count_groups(qs, h, after=c))
                legs["row_count"] = lambda: idx.search_count(qs)
                legs["row_count_past_page1"] = (lambda c=cursors[2]: idx.search_count(qs, after=c))
                total = idx.count_groups(qs, h)
                checks["count_identity_after_page1"] = bool(np.all(idx.count_groups(qs, h, after=cursors[2]) == total - k))
                checks["groups_counted"] = int(total[0])
        for fn in legs.values():  # warm: code objects, contexts, pinned buffers
            fn()
            fn()
        s0 = idx.search_grouped_after_stats()
        us = {name: [] for name in legs}
        for _ in range(rounds):
            for name, fn in legs.items():
                us[name].append(once(fn))
        s1 = idx.search_grouped_after_stats()
        out["us_per_query"] = {name: {"median": round(float(np.median(v)), 2), "p10": round(float(np.percentile(v, 10)), 2),
                                      "p90": round(float(np.percentile(v, 90)), 2)} for name, v in us.items()}
        out["stats_of_the_timed_rounds"] = {key: s1[key] - s0[key] for key in s1}
        out["checks"] = checks
        m = {name: v["median"] for name, v in out["us_per_query"].items()}
        out["summary"] = {f"k{k}": {"page_over_grouped": {f"page{p}": round(m[f"grouped_after_k{k}_page{p}"] / m[f"grouped_k{k}"], 3) for p in PAGES},
                                    "page_over_caller": {f"page{p}": round(m[f"grouped_after_k{k}_page{p}"] / m[f"caller_k{k}_page{p}"], 3) for p in PAGES}}
                          for k in (10, 100)}
        out["summary"]["group_count_over_row_count"] = round(m["group_count"] / m["row_count"], 3)
print("AB " + json.dumps(out), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
