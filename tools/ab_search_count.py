"""Cost of tsh_search_count against the searches it replaces, on the f32 route (profiles/search_count_ab.json): 1 M x 768
f32, L2, TSH_OPT_SCAN_F16 = 0 and TSH_OPT_SCAN_I8 = 0, us per query.  One process = one library (TSH_LIB_PATH names
another build's libtostore_hip.so, e.g. the parent commit's, which is then asked for the baselines only); run the two
alternately.  Prints one JSON line.
  gate        a lone count with T at the query's 100th neighbour, no cursor, against the PARENT's lone tsh_search(k = 100)
  unmoved     tsh_search and tsh_search_after page 100, lone, on both libraries
  reported    the count with T at the corpus' median distance (side rows per count, redo rate), 64-query calls, a keep-50 %
              handle mask, and the count of a 10 000-row list against the walk of 100 pages of k = 100
usage: python tools/ab_search_count.py LABEL [LONE_QUERIES [CALLS_OF_64]]      (one run; LABEL starts with "parent" for
                                                                               the parent commit's library)
       python tools/ab_search_count.py --merge OUT.json FILE_OF_AB_LINES ...   (the runs' lines -> the profile file)"""
import ctypes
import json
import os
import sys
import time

import numpy as np


def merge(out_path, files):
    """The committed profile: every run's line (libraries named by their label, not by a path) and a summary of the
    medians -- the worst case for the gate: the slowest count run against the fastest baseline run."""
    runs = []
    for f in files:
        runs += [json.loads(line[3:]) for line in open(f) if line.startswith("AB ")]
    for r in runs:
        r["lib"] = "parent commit" if r["label"].startswith("parent") else "this commit"

    def med(key, who):
        return [r[key]["median"] for r in runs if r["label"].startswith(who) and key in r]

    def spread(key):
        both = med(key, "parent") + med(key, "this")
        return round(max(both) / min(both) - 1, 4) if both else None

    base, gate = med("search_lone", "parent"), med("count_k100_lone", "this")
    stats = [r["count_median_stats"] for r in runs if "count_median_stats" in r]
    out = {
        "what": "tools/ab_search_count.py on one MI355X: 1 M x 768 f32, L2, TSH_OPT_SCAN_F16 = 0, TSH_OPT_SCAN_I8 = 0 (the f32 "
                "route); us per query (host clock around calls that return their results), lone queries and 64-query calls; the "
                "parent commit's library and this commit's in alternating processes, same box",
        "runs": runs,
        "summary": {
            "gate": {
                "parent_search_k100_lone_us": base, "count_T_at_100th_neighbour_lone_us": gate,
                "count_over_parent_search": round(max(gate) / min(base) - 1, 4) if base and gate else None, "allowance": 0.10,
            },
            "unmoved": {
                "search_lone_us": {"parent": base, "this": med("search_lone", "this")},
                "after_page100_lone_us": {"parent": med("after_page100_lone", "parent"), "this": med("after_page100_lone", "this")},
                "search_lone_spread_over_all_runs": spread("search_lone"), "after_page100_spread_over_all_runs": spread("after_page100_lone"),
            },
            "reported_not_gated": {
                "count_T_at_corpus_median_lone_us": med("count_median_lone", "this"),
                "side_rows_per_count_at_median": [round(s["side_rows"] / max(s["searches"], 1), 2) for s in stats],
                "redo_rate_at_median": [round(s["redone"] / max(s["searches"], 1), 4) for s in stats],
                "count_k100_64_us_per_query": med("count_k100_64", "this"), "count_median_64_us_per_query": med("count_median_64", "this"),
                "parent_search_64_us_per_query": med("search_64", "parent"),
                "count_k100_masked_handle_lone_us": med("count_masked_lone", "this"), "parent_search_masked_handle_lone_us": med("search_masked_lone", "parent"),
                "count_of_10000_row_list_lone_us": med("count_k10000_lone", "this"),
                "parent_walk_of_100_pages_us": med("walk_100_pages", "parent"), "this_walk_of_100_pages_us": med("walk_100_pages", "this"),
            },
        },
    }
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["summary"], indent=1))


if len(sys.argv) > 1 and sys.argv[1] == "--merge":
    merge(sys.argv[2], sys.argv[3:])
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tostore_amd import _ffi  # noqa: E402

if os.environ.get("TSH_LIB_PATH"):  # another build's library: bind what it exports
    _L = ctypes.CDLL(_ffi.LIB_PATH)
    for _name in [s for s in _ffi.SIGNATURES if not hasattr(_L, s)]:
        del _ffi.SIGNATURES[_name]
from tostore_amd import HipMask, HipVectorIndex  # noqa: E402

label = sys.argv[1]
lone = int(sys.argv[2]) if len(sys.argv) > 2 else 200
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 7
has_count = "tsh_search_count" in _ffi.SIGNATURES
n, d, k, nq, page = 1_000_000, 768, 100, 64, 100
rng = np.random.default_rng(2026)
rows = rng.standard_normal((n, d), dtype=np.float32)
qs = rng.standard_normal((nq, d), dtype=np.float32)
keep = np.packbits(rng.random(n) < 0.5, bitorder="little")
out = {"label": label, "lib": "TSH_LIB_PATH" if os.environ.get("TSH_LIB_PATH") else "tree", "lone_queries": lone, "calls_of_64": calls}


def timed(fn, reps, per):
    for _ in range(3):  # warm: code objects, contexts, pinned buffers
        fn()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()  # returns finalised results: every query has been waited for
        us.append((time.perf_counter() - t0) * 1e6 / per)
    us = np.asarray(us)
    return {"median": round(float(np.median(us)), 2), "p10": round(float(np.percentile(us, 10)), 2), "p90": round(float(np.percentile(us, 90)), 2)}


def walk(idx, q, pages):
    cur = (-np.inf, 0)
    for _ in range(pages):
        ids, dist, cnt = idx.search_after(q, k, cur)
        cur = (float(dist[0, -1]), int(ids[0, -1]))
    return cur


with HipVectorIndex(d, 0, capacity_rows=n) as idx:
    idx.set_batch_min_nq(0)
    idx.set_scan_f16(0)
    idx.set_scan_i8(0)
    idx.append(0, rows)
    # the corpus' median distance from the first query, from a sample of the rows (numpy: an estimate is enough)
    sample = rows[:: n // 20000].astype(np.float64)
    t_median = float(np.median(np.sqrt(((sample - qs[0].astype(np.float64)) ** 2).sum(axis=1))))
    del rows, sample
    with HipMask(idx, keep) as h:
        out["search_lone"] = timed(lambda: idx.search(qs[0], k), lone, 1)
        out["search_64"] = timed(lambda: idx.search(qs, k), calls, nq)
        out["search_masked_lone"] = timed(lambda: idx.search(qs[0], k, None, h), lone, 1)
        deep_k = k * page
        ids, dist, cnt = idx.search(qs, deep_k)
        deep = (dist[:, deep_k - k - 1].copy(), ids[:, deep_k - k - 1].copy())  # the last entry of page 99
        out["after_page100_lone"] = timed(lambda: idx.search_after(qs[0], k, (deep[0][:1], deep[1][:1])), lone, 1)
        out["walk_100_pages"] = timed(lambda: walk(idx, qs[0], page), 3, 1)
        if has_count:
            t100 = dist[:, k - 1].copy()      # the 100th neighbour's distance, per query
            t10000 = float(dist[0, deep_k - 1])
            m_dist = idx.search(qs[0], k, None, h)[1]
            out["count_k100_lone"] = timed(lambda: idx.search_count(qs[0], float(t100[0])), lone, 1)
            s0 = idx.search_count_stats()
            out["count_median_lone"] = timed(lambda: idx.search_count(qs[0], t_median), lone, 1)
            s1 = idx.search_count_stats()
            out["count_median_stats"] = {key: s1[key] - s0[key] for key in s1}
            out["count_k100_64"] = timed(lambda: idx.search_count(qs, float(t100[0])), calls, nq)
            out["count_median_64"] = timed(lambda: idx.search_count(qs, t_median), calls, nq)
            out["count_masked_lone"] = timed(lambda: idx.search_count(qs[0], float(m_dist[0, k - 1]), h), lone, 1)
            out["count_k10000_lone"] = timed(lambda: idx.search_count(qs[0], t10000), lone, 1)
            out["answers"] = {"count_k100": int(idx.search_count(qs[0], float(t100[0]))[0]), "count_masked_k100": int(idx.search_count(qs[0], float(m_dist[0, k - 1]), h)[0]),
                              "count_k10000": int(idx.search_count(qs[0], t10000)[0]), "count_median": int(idx.search_count(qs[0], t_median)[0]), "rows": n}
            out["answers_ok"] = out["answers"]["count_k100"] == k and out["answers"]["count_masked_k100"] == k and out["answers"]["count_k10000"] == deep_k
print("AB " + json.dumps(out), flush=True)
