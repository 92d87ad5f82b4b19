"""Cost of tsh_search_grouped against what it replaces and what it adds to (profiles/search_grouped_ab.json): 1 M x 768 f32,
L2, groups of 8 consecutive rows drawn around a common centre (a near group contributes many near rows), k = 10 and 100,
64-query calls, us per query.  One process = one library (TSH_LIB_PATH names another build's libtostore_hip.so, e.g. the
parent commit's, which is then asked for the baselines only); run the two alternately.  Prints one JSON line.
  1 grouped     tsh_search_grouped per query                                                           (this commit)
  2 count       tsh_search_count per query, no threshold: the same route -- an f32 scan and one pass over the keys --,
                the floor the group passes add to                                                       (parent commit)
  3 pages       what a caller does without the call: tsh_search_after pages of k, all 64 queries a page per call, until
                every query has seen k distinct groups; P = pages per query                             (parent commit)
  4 G1          group_min_kernel alone: run this script under  rocprofv3 --kernel-trace --stats  in a run of its own
                (label "this-trace": grouped searches only, both k; the kernel does not depend on k) and read the kernel's
                row of tools/rocpd_summary.py's table; --merge takes the figure as  --g1 AVG_US MIN_US  (the average is
                taken while the tail's 16 CUs share the HBM with the next query's scan, the minimum with the device idle)
  beside them   a plain tsh_search per query, routes as shipped (big shards read the int8 copy), and with the reduced
                copies off: what "a grouped search takes the f32 scan" costs
usage: python tools/ab_search_grouped.py LABEL [CALLS_OF_64]       (LABEL starts with "parent" for the parent commit's library)
       python tools/ab_search_grouped.py --merge OUT.json [--g1 AVG_US MIN_US] FILE_OF_AB_LINES ..."""
import ctypes
import json
import os
import sys
import time

import numpy as np


def merge(out_path, args):
    g1 = None
    if args and args[0] == "--g1":
        g1 = {"avg_us_beside_the_next_scan": float(args[1]), "min_us_device_idle": float(args[2])}
        args = args[3:]
    runs = []
    for f in args:
        runs += [json.loads(line[3:]) for line in open(f) if line.startswith("AB ")]
    for r in runs:
        r["lib"] = "parent commit" if r["label"].startswith("parent") else "this commit"

    def med(key, who):
        return [r[key]["median"] for r in runs if r["label"].startswith(who) and key in r]

    summary = {}
    for k in (10, 100):
        grouped, pages, count = med(f"grouped_k{k}_64", "this"), med(f"pages_k{k}_64", "parent"), med("count_64", "parent")
        p = [r[f"pages_k{k}_P"] for r in runs if r["label"].startswith("parent") and f"pages_k{k}_P" in r]
        summary[f"k{k}"] = {
            "1_grouped_us_per_query": grouped, "2_parent_count_us_per_query": count, "3_parent_pages_us_per_query": pages, "3_pages_P": p,
            "1_below_3_worst_case": (max(grouped) < min(pages)) if grouped and pages else None,
            "1_over_2": round(max(grouped) / min(count), 3) if grouped and count else None,
            "4_group_min_kernel_us": g1,
            "side_rows_per_search": [round(r[f"grouped_k{k}_stats"]["side_rows"] / max(r[f"grouped_k{k}_stats"]["searches"], 1), 2)
                                     for r in runs if f"grouped_k{k}_stats" in r],
            "plain_search_as_shipped_us_per_query": med(f"search_k{k}_64", "this"), "plain_search_f32_only_us_per_query": med(f"search_f32_k{k}_64", "this"),
            "grouped_over_plain_search_as_shipped": round(max(grouped) / min(med(f"search_k{k}_64", "this")), 2) if grouped and med(f"search_k{k}_64", "this") else None,
        }
    out = {"what": "tools/ab_search_grouped.py on one MI355X: 1 M x 768 f32, L2, groups of 8 consecutive rows around a common centre; us per "
                   "query of 64-query calls (host clock around calls that return their results); the parent commit's library and this "
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
has_grouped = "tsh_search_grouped" in _ffi.SIGNATURES
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


def pages(idx, k):
    """tsh_search_after pages of k for all queries still short of k distinct groups -> (first k group heads per query, pages per query)"""
    cur_d, cur_i = np.full(nq, -np.inf), np.zeros(nq, np.int64)
    seen = [dict() for _ in range(nq)]  # group -> its first (nearest) row, in order of appearance
    n_pages = np.zeros(nq, np.int64)
    active = np.arange(nq)
    while len(active):
        ids, dist, cnt = idx.search_after(qs[active], k, (cur_d[active], cur_i[active]))
        still = []
        for j, q in enumerate(active):
            n_pages[q] += 1
            for i in ids[j, :cnt[j]]:
                seen[q].setdefault(int(group_of[i]), int(i))
            cur_d[q], cur_i[q] = dist[j, cnt[j] - 1], ids[j, cnt[j] - 1]
            if len(seen[q]) < k and cnt[j] == k:
                still.append(q)
        active = np.asarray(still, np.int64)
    return [list(s.values())[:k] for s in seen], n_pages


with HipVectorIndex(d, 0, capacity_rows=n) as idx:
    idx.set_batch_min_nq(0)
    idx.append(0, rows)
    del rows
    for k in (10, 100):
        if has_grouped:
            with idx.make_groups(group_of, n_groups) as h:
                s0 = idx.search_grouped_stats()
                out[f"grouped_k{k}_64"] = timed(lambda: idx.search_grouped(qs, k, h), calls, nq)
                s1 = idx.search_grouped_stats()
                out[f"grouped_k{k}_stats"] = {key: s1[key] - s0[key] for key in s1}
                if trace_only:
                    continue
                g_ids = idx.search_grouped(qs, k, h)[0]
        if trace_only:
            continue
        out[f"search_k{k}_64"] = timed(lambda: idx.search(qs, k), calls, nq)
        heads, n_pages = pages(idx, k)
        out[f"pages_k{k}_P"] = {"mean": round(float(n_pages.mean()), 2), "min": int(n_pages.min()), "max": int(n_pages.max())}
        out[f"pages_k{k}_64"] = timed(lambda: pages(idx, k), max(calls // 2, 2), nq)
        if has_grouped:
            out[f"answers_ok_k{k}"] = all(list(g_ids[q]) == heads[q] for q in range(nq))
    if not trace_only:
        out["count_64"] = timed(lambda: idx.search_count(qs), calls, nq)
        idx.set_scan_f16(0)
        idx.set_scan_i8(0)
        for k in (10, 100):
            out[f"search_f32_k{k}_64"] = timed(lambda: idx.search(qs, k), calls, nq)
print("AB " + json.dumps(out), flush=True)
