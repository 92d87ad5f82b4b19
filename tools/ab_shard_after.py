"""Cost of a page of tsh_search_shard_after against tsh_search_shard on the f32 route (profiles/shard_after_ab.json): one
125 k x 768 f32 shard handle (one rank's share of config C2 over 8), L2, k = 100, 64-query calls into a device buffer,
TSH_OPT_SCAN_F16 = 0, TSH_OPT_SCAN_I8 = 0 and TSH_OPT_BATCH_MIN_NQ = 0 (every leg is the pipeline of single-query f32
scans), us per query.  One process = one library (TSH_LIB_PATH names another build's libtostore_hip.so, e.g. the parent
commit's, which is then asked for the baseline only); run the two alternately.  Prints one JSON line.
usage: python tools/ab_shard_after.py LABEL [CALLS_OF_64]                     (one run; LABEL starts with "parent" for
                                                                               the parent commit's library)
       python tools/ab_shard_after.py --merge OUT.json FILE_OF_AB_LINES ...   (the runs' lines -> the profile file)"""
import ctypes
import json
import os
import sys
import time
import zlib

import numpy as np


def merge(out_path, files):
    """The committed profile: every run's line and a summary of the medians -- the worst case for the ratios: the
    slowest leg of this commit against the fastest baseline run, next to each library's own run-to-run spread."""
    runs = []
    for f in files:
        runs += [json.loads(line[3:]) for line in open(f) if line.startswith("AB ")]
    for r in runs:
        r["lib"] = "parent commit" if r["label"].startswith("parent") else "this commit"

    def med(key, who):
        return [r[key]["median"] for r in runs if r["label"].startswith(who) and key in r]

    base, here = med("shard_64", "parent"), med("shard_64", "this") + med("shard_64_again", "this")
    p1, p100 = med("shard_after_page1_64", "this"), med("shard_after_page100_64", "this")
    side = [r["after_stats"] for r in runs if "after_stats" in r]
    out = {
        "what": "tools/ab_shard_after.py on one MI355X: one 125 k x 768 f32 shard handle, L2, k = 100, 64-query calls, blocks "
                "in device memory, TSH_OPT_SCAN_F16 = 0, TSH_OPT_SCAN_I8 = 0, TSH_OPT_BATCH_MIN_NQ = 0 (the f32 route, query by "
                "query); us per query (host clock around calls that return when the blocks are final); the parent commit's "
                "library and this commit's in alternating processes, same box",
        "runs": runs,
        "summary": {
            "parent_shard_64_us": base, "this_shard_64_us": here, "shard_after_page1_64_us": p1, "shard_after_page100_64_us": p100,
            "parent_run_to_run_spread": round(max(base) / min(base) - 1, 4) if base else None,
            "this_run_to_run_spread": round(max(here) / min(here) - 1, 4) if here else None,
            "this_shard_over_parent": round(max(here) / min(base) - 1, 4) if base and here else None,
            "page1_over_parent": round(max(p1) / min(base) - 1, 4) if base and p1 else None,
            "page100_over_parent": round(max(p100) / min(base) - 1, 4) if base and p100 else None,
            "allowance_page100": 0.10,
            "side_rows_per_cursor_search": [round(s["side_rows"] / max(s["searches"], 1), 2) for s in side],
            "page100_matches_deep_search": [r["page100_matches_deep_search"] for r in runs if "page100_matches_deep_search" in r],
            "note": "page 1 starts from -inf and runs no floor pass; page 100 runs the floor pass and the side append",
        },
    }
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["summary"], indent=1))


if len(sys.argv) > 1 and sys.argv[1] == "--merge":
    merge(sys.argv[2], sys.argv[3:])
    sys.exit(0)

import torch  # noqa: E402  (first: it brings its own ROCm runtime)

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tostore_amd import _ffi  # noqa: E402

if os.environ.get("TSH_LIB_PATH"):  # another build's library: bind what it exports
    _L = ctypes.CDLL(_ffi.LIB_PATH)
    for _name in [s for s in _ffi.SIGNATURES if not hasattr(_L, s)]:
        del _ffi.SIGNATURES[_name]
from tostore_amd import HipVectorIndex  # noqa: E402
from tostore_amd.sharded import merge_candidate_blocks  # noqa: E402

label = sys.argv[1]
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 15
has_after = "tsh_search_shard_after" in _ffi.SIGNATURES
n, d, k, nq, page, base = 125_000, 768, 100, 64, 100, 250_000
rng = np.random.default_rng(2026)
rows = rng.standard_normal((n, d), dtype=np.float32)
qs = rng.standard_normal((nq, d), dtype=np.float32)
out = {"label": label, "lib": "TSH_LIB_PATH" if os.environ.get("TSH_LIB_PATH") else "tree", "calls_of_64": calls}
L = _ffi.lib()
entries = L.tsh_default_block_entries(k)
bb = L.tsh_candidate_block_bytes(entries)
buf = torch.zeros(nq * bb, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
qp, bp = qs.ctypes.data_as(_ffi.p_f32), ctypes.c_void_p(buf.data_ptr())


def timed(fn, reps, per):
    for _ in range(3):  # warm: code objects, contexts, pinned buffers
        fn()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()  # returns when every block is final
        us.append((time.perf_counter() - t0) * 1e6 / per)
    us = np.asarray(us)
    return {"median": round(float(np.median(us)), 2), "p10": round(float(np.percentile(us, 10)), 2),
            "p90": round(float(np.percentile(us, 90)), 2), "blocks_crc": zlib.crc32(buf.cpu().numpy()[:8 * nq].tobytes())}


with HipVectorIndex(d, 0, capacity_rows=n, shard_device=0, row_base=base) as idx:
    idx.set_batch_min_nq(0)
    idx.set_scan_f16(0)
    idx.set_scan_i8(0)
    idx.append(base, rows)
    del rows
    out["shard_64"] = timed(lambda: _ffi.check(L.tsh_search_shard(idx._h, qp, nq, k, None, entries, bp, None)), calls, nq)
    if has_after:
        deep_k = k * page
        ids, dist, cnt = idx.search(qs, deep_k)  # pages 1 .. 100: page 100 starts behind the last entry of page 99
        start = (np.full(nq, -np.inf), np.zeros(nq, np.int64))
        deep = (np.ascontiguousarray(dist[:, deep_k - k - 1]), np.ascontiguousarray(ids[:, deep_k - k - 1]))

        def after(cur):
            _ffi.check(L.tsh_search_shard_after(idx._h, qp, nq, k, None, cur[0].ctypes.data_as(_ffi.p_f64),
                                                cur[1].ctypes.data_as(_ffi.p_i64), entries, bp, None))

        s0 = idx.search_after_stats()
        out["shard_after_page1_64"] = timed(lambda: after(start), calls, nq)
        out["shard_after_page100_64"] = timed(lambda: after(deep), calls, nq)
        s1 = idx.search_after_stats()
        out["after_stats"] = {key: s1[key] - s0[key] for key in s1}
        # the blocks of page 100, merged behind the cursor, are what the deep tsh_search returns behind page 99
        got = merge_candidate_blocks(0, d, qs, k, None, buf.cpu().numpy(), 1, entries, after=deep)
        out["page100_matches_deep_search"] = bool(np.array_equal(got[0], ids[:, -k:]) and np.array_equal(got[1], dist[:, -k:]))
        out["shard_64_again"] = timed(lambda: _ffi.check(L.tsh_search_shard(idx._h, qp, nq, k, None, entries, bp, None)), calls, nq)
print("AB " + json.dumps(out), flush=True)
