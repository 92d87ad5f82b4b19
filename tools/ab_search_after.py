"""Cost of a page of tsh_search_after against tsh_search on the f32 route (profiles/search_after_ab.json): 1 M x 768 f32,
L2, k = 100, TSH_OPT_SCAN_F16 = 0 and TSH_OPT_SCAN_I8 = 0, lone queries and 64-query calls, us per query.  One process =
one library (TSH_LIB_PATH names another build's libtostore_hip.so, e.g. the parent commit's, which is then asked for
the baseline only); run the two alternately.  Prints one JSON line.
Behind a keep-50 % pointer mask as well (lone queries): the masked tsh_search, and page 100 of the masked list.
usage: python tools/ab_search_after.py LABEL [LONE_QUERIES [CALLS_OF_64]]      (one run; LABEL starts with "parent" for
                                                                               the parent commit's library)
       python tools/ab_search_after.py --merge OUT.json FILE_OF_AB_LINES ...   (the runs' lines -> the profile file)"""
import ctypes
import json
import os
import sys
import time
import zlib

import numpy as np



def merge(out_path, files):
    """The committed profile: every run's line (libraries named by their label, not by a path) and a summary of the
    medians -- the worst case for the ratios: the slowest page against the fastest baseline run."""
    runs = []
    for f in files:
        runs += [json.loads(line[3:]) for line in open(f) if line.startswith("AB ")]
    for r in runs:
        r["lib"] = "parent commit" if r["label"].startswith("parent") else "this commit"

    def med(key, who):
        return [r[key]["median"] for r in runs if r["label"].startswith(who) and key in r]

    base, base_m = med("search_lone", "parent"), med("search_masked_lone", "parent")
    p1, p100, p100m = med("after_page1_lone", "this"), med("after_page100_lone", "this"), med("after_masked_page100_lone", "this")
    side = [r["after_stats"] for r in runs if "after_stats" in r]
    out = {
        "what": "tools/ab_search_after.py on one MI355X: 1 M x 768 f32, L2, k = 100, TSH_OPT_SCAN_F16 = 0, TSH_OPT_SCAN_I8 = 0 "
                "(the f32 route); us per query (host clock around calls that return finalised results), lone queries and "
                "64-query calls; the parent commit's library and this commit's in alternating processes, same box",
        "runs": runs,
        "summary": {
            "parent_search_lone_us": base, "after_page1_lone_us": p1, "after_page100_lone_us": p100,
            "page1_over_baseline": round(max(p1) / min(base) - 1, 4), "page100_over_baseline": round(max(p100) / min(base) - 1, 4),
            "allowance_lone": 0.10,
            "reported_not_gated": {
                "parent_search_64_us": med("search_64", "parent"), "after_page1_64_us": med("after_page1_64", "this"),
                "after_page100_64_us": med("after_page100_64", "this"),
                "parent_search_k10000_lone_us": med("search_k10000_lone", "parent"),
                "parent_search_masked_lone_us": base_m, "after_masked_page100_lone_us": p100m,
                "masked_page100_over_masked_baseline": round(max(p100m) / min(base_m) - 1, 4) if base_m and p100m else None,
            },
            "side_rows_per_cursor_search": [round(s["side_rows"] / max(s["searches"], 1), 2) for s in side],
            "note": "page 1 starts from -inf and runs no floor pass; page 100 runs the floor pass and the side re-rank",
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
from tostore_amd import HipVectorIndex  # noqa: E402

label = sys.argv[1]
lone = int(sys.argv[2]) if len(sys.argv) > 2 else 200
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 7
has_after = "tsh_search_after" in _ffi.SIGNATURES
n, d, k, nq, page = 1_000_000, 768, 100, 64, 100
rng = np.random.default_rng(2026)
rows = rng.standard_normal((n, d), dtype=np.float32)
qs = rng.standard_normal((nq, d), dtype=np.float32)
keep = np.packbits(rng.random(n) < 0.5, bitorder="little")
out = {"label": label, "lib": "TSH_LIB_PATH" if os.environ.get("TSH_LIB_PATH") else "tree", "lone_queries": lone, "calls_of_64": calls}


def timed(fn, reps, per):
    for _ in range(3):  # warm: code objects, contexts, pinned buffers
        got = fn()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = fn()  # returns finalised results: every query has been waited for
        us.append((time.perf_counter() - t0) * 1e6 / per)
    us = np.asarray(us)
    return {"median": round(float(np.median(us)), 2), "p10": round(float(np.percentile(us, 10)), 2),
            "p90": round(float(np.percentile(us, 90)), 2), "answer_crc": zlib.crc32(got[0].tobytes() + got[1].tobytes())}


with HipVectorIndex(d, 0, capacity_rows=n) as idx:
    idx.set_batch_min_nq(0)
    idx.set_scan_f16(0)
    idx.set_scan_i8(0)
    idx.append(0, rows)
    del rows
    out["search_lone"] = timed(lambda: idx.search(qs[0], k), lone, 1)
    out["search_64"] = timed(lambda: idx.search(qs, k), calls, nq)
    deep_k = k * page
    out["search_k10000_lone"] = timed(lambda: idx.search(qs[0], deep_k), max(lone // 10, 5), 1)
    out["search_masked_lone"] = timed(lambda: idx.search(qs[0], k, None, keep), lone, 1)
    if has_after:
        m_ids, m_dist, _ = idx.search(qs[0], deep_k - k, None, keep)
        m_deep = (m_dist[:, -1].copy(), m_ids[:, -1].copy())
        out["after_masked_page100_lone"] = timed(lambda: idx.search_after(qs[0], k, m_deep, None, keep), lone, 1)
        ids, dist, cnt = idx.search(qs, deep_k - k)  # what pages 1 .. 99 hold: page 100 starts behind its last entry
        start = (np.full(nq, -np.inf), np.zeros(nq, np.int64))
        deep = (dist[:, -1].copy(), ids[:, -1].copy())
        s0 = idx.search_after_stats()
        out["after_page1_lone"] = timed(lambda: idx.search_after(qs[0], k, (start[0][:1], start[1][:1])), lone, 1)
        out["after_page100_lone"] = timed(lambda: idx.search_after(qs[0], k, (deep[0][:1], deep[1][:1])), lone, 1)
        out["after_page1_64"] = timed(lambda: idx.search_after(qs, k, start), calls, nq)
        out["after_page100_64"] = timed(lambda: idx.search_after(qs, k, deep), calls, nq)
        s1 = idx.search_after_stats()
        out["after_stats"] = {key: s1[key] - s0[key] for key in s1}
        # page 100 is what the deep tsh_search returns behind page 99
        want = idx.search(qs[0], deep_k)
        got = idx.search_after(qs[0], k, (deep[0][:1], deep[1][:1]))
        out["page100_matches_deep_search"] = bool(np.array_equal(got[0][0], want[0][0, -k:]) and np.array_equal(got[1][0], want[1][0, -k:]))
print("AB " + json.dumps(out), flush=True)
