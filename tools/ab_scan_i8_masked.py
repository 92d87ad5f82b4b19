"""Per-query time of 64-query tsh_search calls (batched path off) on 1 M x 768 f32, L2, k = 100, for a keep-50 % pointer
mask, the same mask as a handle, dense, and one tombstone (profiles/scan_i8_masked_ab.json).  One process = one library
(TSH_LIB_PATH names another build's libtostore_hip.so); prints one JSON line.
usage: python tools/ab_scan_i8_masked.py LABEL [TIMED_CALLS_PER_CASE]"""
import json
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tostore_amd import HipVectorIndex  # noqa: E402

label = sys.argv[1]
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 7
n, d, k, nq = 1_000_000, 768, 100, 64
rng = np.random.default_rng(2025)
rows = rng.standard_normal((n, d), dtype=np.float32)
rows *= rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
qs = rng.standard_normal((nq, d), dtype=np.float32)
keep = np.packbits(rng.random(n) < 0.5, bitorder="little")
out = {"label": label, "lib": os.environ.get("TSH_LIB_PATH", "tree"), "calls": calls}
with HipVectorIndex(d, 0, capacity_rows=n) as idx:
    idx.set_batch_min_nq(0)
    idx.append(0, rows)

    def run(what, mask):
        for _ in range(2):  # warm: builds the copy, loads the code objects
            got = idx.search(qs, k, None, mask)
        i0, f0 = idx.scan_i8_stats(), idx.scan_f16_stats()
        us = []
        for _ in range(calls):
            t0 = time.perf_counter()
            got = idx.search(qs, k, None, mask)  # returns finalised results: every query has been waited for
            us.append((time.perf_counter() - t0) * 1e6 / nq)
        i1, f1 = idx.scan_i8_stats(), idx.scan_f16_stats()
        out[what] = {"us_per_query": [round(x, 2) for x in us], "median": round(float(np.median(us)), 2),
                     "i8_scans": i1["scans"] - i0["scans"], "i8_redone": i1["redone"] - i0["redone"], "f16_scans": f1["scans"] - f0["scans"],
                     "answer_crc": zlib.crc32(got[0].tobytes() + got[1].tobytes())}

    run("keep50_pointer", keep)
    with idx.make_mask(keep) as h:
        run("keep50_handle", h)
    run("dense", None)
    idx.set_deleted([123_457])
    run("one_tombstone", None)
print("AB " + json.dumps(out), flush=True)
