"""Cost of tsh_search_grouped_rows against what it builds on and what it replaces (profiles/search_grouped_rows_ab.json):
1 M x 768 f32, L2, groups of 8 consecutive rows drawn around a common centre (tools/ab_search_grouped.py's layout: a near
group contributes many near rows), k = 10 and 100, m = 1, 3 and 10, 64-query calls, us per query.  One process = one
library (TSH_LIB_PATH names another build's libtostore_hip.so, e.g. the parent commit's, which is then asked for the
baselines only); run the two alternately.  Prints one JSON line.
  1 grouped   tsh_search_grouped per query: one row per group, the baseline                               (parent commit)
  2 rows      tsh_search_grouped_rows per query at m = 1, 3, 10                                           (this commit)
  3 pages     what a caller does without the call: tsh_search_grouped, then tsh_search_after pages of k * m rows, all
              queries still short a page per call, rows of foreign groups dropped on the host, until every winning group
              has m rows or the list ends (stopped after MAX_PAGES pages: a group with fewer than m rows ends the loop only
              at the end of the list); P = pages per query.  This commit's side runs the loop once at m = 3 and checks
              that what it found is, group by group, a prefix of the entry's answer                       (parent commit)
  per pass    run this script under  rocprofv3 --kernel-trace --stats  in a run of its own (label "this-trace": rows
              searches only) and read the group_rows_* kernels' rows of tools/rocpd_summary.py's table
usage: python tools/ab_search_grouped_rows.py LABEL [CALLS_OF_64]   (LABEL starts with "parent" for the parent commit's library)
       python tools/ab_search_grouped_rows.py --merge OUT.json FILE_OF_AB_LINES ..."""
import ctypes
import json
import os
import sys
import time

import numpy as np

KS, MS = (10, 100), (1, 3, 10)
MAX_PAGES = 6


def merge(out_path, args):
    runs = []
    for f in args:
        runs += [json.loads(line[3:]) for line in open(f) if line.startswith("AB ")]
    for r in runs:
        r["lib"] = "parent commit" if r["label"].startswith("parent") else "this commit"

    def med(key, who):
        return [r[key]["median"] for r in runs if r["label"].startswith(who) and key in r]

    summary = {}
    for k in KS:
        base = med(f"grouped_k{k}_64", "parent")
        summary[f"k{k}"] = {"1_parent_grouped_us_per_query": base, "1_this_grouped_us_per_query": med(f"grouped_k{k}_64", "this")}
        for m in MS:
            rows, pages = med(f"rows_k{k}_m{m}_64", "this"), med(f"pages_k{k}_m{m}_64", "parent")
            summary[f"k{k}"][f"m{m}"] = {
                "2_rows_us_per_query": rows, "3_parent_pages_us_per_query": pages,
                "3_pages_P": [r[f"pages_k{k}_m{m}_P"] for r in runs if f"pages_k{k}_m{m}_P" in r],
                "2_over_1": round(max(rows) / min(base), 3) if rows and base else None,
                "2_below_3_worst_case": (max(rows) < min(pages)) if rows and pages else None,
                "per_search": [{key: round(v / max(r[f"rows_k{k}_m{m}_stats"]["searches"], 1), 2) for key, v in r[f"rows_k{k}_m{m}_stats"].items()}
                               for r in runs if f"rows_k{k}_m{m}_stats" in r],
                "answers_ok": [r[f"answers_ok_k{k}_m{m}"] for r in runs if f"answers_ok_k{k}_m{m}" in r],
                "rows_the_loop_found_of_the_entrys": [[r[f"rows_the_loop_found_k{k}_m{m}"], r[f"rows_the_entry_returned_k{k}_m{m}"]]
                                                      for r in runs if f"rows_the_loop_found_k{k}_m{m}" in r],
            }
    out = {"what": "tools/ab_search_grouped_rows.py on one MI355X: 1 M x 768 f32, L2, groups of 8 consecutive rows around a common centre; us "
                   "per query of 64-query calls (host clock around calls that return their results); the parent commit's library and this "
                   "commit's in alternating processes, same box",
           "runs": runs, "summary": summary}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if len(sys.argv) > 1 and sys.argv[1] == "--merge":
    merge(sys.argv[2], sys.argv[3:])
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tostore_amd import _ffi  # noqa: E402

if os.environ.get("TSH_LIB_PATH"):  # another build's library: bind what it exports
    _L = ctypes.CDLL(_ffi.LIB_PATH)
    for _name in [s for s in _ffi.SIGNATURES if not hasattr(_L, s)]:
        del _ffi.SIGNATURES[_name]
from tostore_amd import HipVectorIndex  # noqa: E402

label = sys.argv[1]
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 7
trace_only = label.endswith("trace")
has_rows = "tsh_search_grouped_rows" in _ffi.SIGNATURES
n, d, nq, per_group = 1_000_000, 768, 64, 8
rng = np.random.default_rng(2027)
n_groups = n // per_group
group_of = (np.arange(n) // per_group).astype(np.int32)
rows = np.empty((n, d), np.float32)
for a in range(0, n_groups, 5000):  # (in pieces: the noise of the whole corpus at once is another 3 GB)
    b = min(a + 5000, n_groups)
    centres = rng.standard_normal((b - a, d), dtype=np.float32)
    rows[a * per_group:b * per_group] = np.repeat(centres, per_group, axis=0) + np.float32(0.3) * rng.standard_normal(((b - a) * per_group, d), dtype=np.float32)
qs = rng.standard_normal((nq, d), dtype=np.float32)
out = {"label": label, "lib": "TSH_LIB_PATH" if os.environ.get("TSH_LIB_PATH") else "tree", "calls_of_64": calls}


def timed(fn, reps, per):
    for _ in range(2):  # warm: code objects, contexts, pinned buffers
        fn()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()  # returns finalised results: every query has been waited for
        us.append((time.perf_counter() - t0) * 1e6 / per)
    us = np.asarray(us)
    return {"median": round(float(np.median(us)), 2), "p10": round(float(np.percentile(us, 10)), 2), "p90": round(float(np.percentile(us, 90)), 2)}


def pages(idx, h, k, m):
    """The caller's loop -> (per query: the winning groups' first m row ids, in order), pages per query"""
    g_ids, g_dist, g_grp, g_cnt = idx.search_grouped(qs, k, h)
    got = [{int(g_grp[q, i]): [] for i in range(g_cnt[q])} for q in range(nq)]
    cur_d, cur_i = np.full(nq, -np.inf), np.zeros(nq, np.int64)
    n_pages = np.zeros(nq, np.int64)
    active = np.arange(nq)
    page = k * m
    # (a group with fewer than m rows is "exhausted" only at the end of the list: the loop has no bound of its own.  It is
    # stopped after MAX_PAGES here, and the queries it was stopped on are reported)
    while len(active) and n_pages.max() < MAX_PAGES:
        ids, dist, cnt = idx.search_after(qs[active], page, (cur_d[active], cur_i[active]))
        still = []
        for j, q in enumerate(active):
            n_pages[q] += 1
            for i in ids[j, :cnt[j]]:
                mine = got[q].get(int(group_of[i]))
                if mine is not None and len(mine) < m:
                    mine.append(int(i))
            cur_d[q], cur_i[q] = dist[j, cnt[j] - 1], ids[j, cnt[j] - 1]
            if cnt[j] == page and any(len(v) < m for v in got[q].values()):
                still.append(q)
        active = np.asarray(still, np.int64)
    return [list(g.values()) for g in got], n_pages, len(active)


with HipVectorIndex(d, 0, capacity_rows=n) as idx:
    idx.set_batch_min_nq(0)
    idx.append(0, rows)
    del rows
    with idx.make_groups(group_of, n_groups) as h:
        for k in KS:
            if not trace_only:
                out[f"grouped_k{k}_64"] = timed(lambda: idx.search_grouped(qs, k, h), calls, nq)
            for m in MS:
                if has_rows:
                    s0 = idx.search_grouped_rows_stats()
                    out[f"rows_k{k}_m{m}_64"] = timed(lambda: idx.search_grouped_rows(qs, k, m, h), calls, nq)
                    s1 = idx.search_grouped_rows_stats()
                    out[f"rows_k{k}_m{m}_stats"] = {key: s1[key] - s0[key] for key in s1}
                if trace_only:
                    continue
                if not has_rows or m == 3:  # (the loop is timed on the parent's side; this side checks one answer against it)
                    want, n_pages, stopped = pages(idx, h, k, m)
                    out[f"pages_k{k}_m{m}_P"] = {"mean": round(float(n_pages.mean()), 2), "min": int(n_pages.min()), "max": int(n_pages.max()),
                                                 "queries_stopped_at_max_pages": stopped}
                    if not has_rows:
                        out[f"pages_k{k}_m{m}_64"] = timed(lambda: pages(idx, h, k, m), max(calls // 2, 2), nq)
                    else:
                        r_ids, _, _, r_rows, r_cnt = idx.search_grouped_rows(qs, k, m, h)
                        # (a loop that was stopped holds a prefix of every group's rows: pages arrive in the list's order)
                        out[f"answers_ok_k{k}_m{m}"] = all(len(want[q]) == r_cnt[q] and all(list(r_ids[q, i, :len(w)]) == w and len(w) <= r_rows[q, i]
                                                                                             for i, w in enumerate(want[q])) for q in range(nq))
                        out[f"rows_the_loop_found_k{k}_m{m}"] = int(sum(len(w) for q in range(nq) for w in want[q]))
                        out[f"rows_the_entry_returned_k{k}_m{m}"] = int(r_rows.sum())
print("AB " + json.dumps(out), flush=True)
