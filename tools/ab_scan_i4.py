"""The 4-bit first pass (TSH_OPT_SCAN_I4) against the plain int8 route, in one process, the two routes alternating on the
same index (option 0 / option 2): per-query time of 64-query tsh_search calls, batched path off, f32 rows of 768, L2,
k = 100 (profiles/scan_i4_bench_ab.json).  Three parts:
  share   1 M rows whose norms are U(lo, hi) for a ladder of ranges: the share of the rows the pass leaves to the int8 scan
          (from tsh_scan_i4_stats) and both routes' times -- where the routes break even is the deny threshold
  size    the headline's corpus, U(0.5, 2), cut to 125 k, 250 k and 500 k rows: where the route starts to pay is its gate
  lone    1 M rows, U(0.5, 2), one query per call: p50 of both routes
Run it against a library that never denies the route (-DTSH_SCAN_I4_MAX_SHARE=2.0, TSH_LIB_PATH), or the forced route
is switched off after two scans of a corpus it does not pay on.  Prints one JSON line.
usage: python tools/ab_scan_i4.py [ROUNDS]"""
import json
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tostore_amd import HipVectorIndex  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N, d, k, nq, calls = 1_000_000, 768, 100, 64, 4
rng = np.random.default_rng(2026)
base = rng.standard_normal((N, d), dtype=np.float32)
base /= np.linalg.norm(base, axis=1, keepdims=True)
base *= np.float32(np.sqrt(d))  # rows of a standard normal's length, exactly
u = rng.random(N).astype(np.float32)
qs = rng.standard_normal((nq, d), dtype=np.float32)
out = {"lib": os.environ.get("TSH_LIB_PATH", "tree"), "rounds": rounds, "calls_per_round": calls}


def timed(idx, fn, calls=calls):
    """us per query of both routes, alternating; the share the 4-bit pass left; whether the answers agree."""
    us, crc, share = {0: [], 2: []}, {}, None
    for mode in (0, 2):  # warm: builds the copies, loads the code objects
        idx.set_scan_i4(mode)
        fn()
    for _ in range(rounds):
        for mode in (0, 2):
            idx.set_scan_i4(mode)
            s0 = idx.scan_i4_stats()
            t0 = time.perf_counter()
            for _ in range(calls):
                got, n_q = fn()
            us[mode].append((time.perf_counter() - t0) * 1e6 / (calls * n_q))
            s1 = idx.scan_i4_stats()
            crc[mode] = zlib.crc32(got[0].tobytes() + got[1].tobytes())
            if mode == 2:
                assert s1["scans"] - s0["scans"] == calls * n_q, (s0, s1)
                share = (s1["survivors"] - s0["survivors"]) / (s1["scans"] - s0["scans"]) / idx.size
    return {"int8_us": [round(x, 2) for x in us[0]], "i4_us": [round(x, 2) for x in us[2]],
            "int8_median": round(float(np.median(us[0])), 2), "i4_median": round(float(np.median(us[2])), 2),
            "int8_spread": round(max(us[0]) - min(us[0]), 2), "i4_spread": round(max(us[2]) - min(us[2]), 2),
            "share": round(share, 4), "same_answers": crc[0] == crc[2]}


def corpus(lo, hi, n=N):
    return base[:n] * (np.float32(lo) + np.float32(hi - lo) * u[:n])[:, None]


def index_of(rows):
    idx = HipVectorIndex(d, 0, capacity_rows=len(rows))
    idx.set_batch_min_nq(0)
    idx.append(0, rows)
    return idx


out["share"] = []
for lo, hi in ((0.5, 2.0), (0.65, 1.55), (0.75, 1.35), (0.8, 1.25), (0.85, 1.18), (0.9, 1.1)):
    with index_of(corpus(lo, hi)) as idx:
        r = timed(idx, lambda: (idx.search(qs, k), nq))
        r["norm_range"] = [lo, hi]
        out["share"].append(r)
        if (lo, hi) == (0.5, 2.0):
            lone = timed(idx, lambda: (idx.search(qs[:1], k), 1), calls=40)
            # (each entry is the mean of 40 lone queries)
            out["lone"] = lone
    print("AB_PART " + json.dumps(out["share"][-1]), flush=True)
out["size"] = []
for n in (125_000, 250_000, 500_000):
    with index_of(corpus(0.5, 2.0, n)) as idx:
        r = timed(idx, lambda: (idx.search(qs, k), nq))
        r["rows"] = n
        out["size"].append(r)
print("AB " + json.dumps(out), flush=True)
