"""Cost of a grouped search across shards (profiles/shard_grouped_ab.json): two processes share one MI355X, each with a
shard handle of 500 k x 768 f32 rows (row ranges of one 1 M-row corpus), L2, k = 10 and 100, groups of 8 consecutive rows
(none spans the ranks' boundary, so today's way below is exact and comparable), 64-query calls, us per query on rank 0's
host clock around collective calls.  Legs:
  (a) sharded_grouped    tsh_search_sharded_grouped over the host transport (gloo underneath)
  (b) grouped_gather     today's way: every rank's tsh_search_grouped on its shard handle, a host all-gather of the ranks'
                         answers over the same gloo group, and the NumPy merge (order, drop repeated groups, cut to k)
  (c) sharded            tsh_search_sharded on the same shards, for scale
  (d) grouped_local      rank 0's tsh_search_grouped on its shard handle while the other rank waits: the device to itself,
                         no exchange -- the entry held against the parent commit
The short legs ((c): some 13 us per query) run five times as many calls as the long ones.
One run = one library (TSH_LIB_PATH names another build's libtostore_hip.so, e.g. the parent commit's, which is then
asked for (c) and (d) only); run the two alternately.  Rank 0 prints one JSON line.
usage: python -m torch.distributed.run --nproc-per-node 2 tools/ab_shard_grouped.py LABEL [CALLS_OF_64] [existing]
                                         (one run; LABEL starts with "parent" for the parent commit's library;
                                         "existing": legs (c) and (d) only, whatever the library has)
       python tools/ab_shard_grouped.py --merge OUT.json FILE_OF_AB_LINES ...   (the runs' lines -> the profile file)"""
import ctypes
import json
import os
import sys
import time

import numpy as np


def merge(out_path, files):
    """The committed profile: every run's line and a summary of the medians -- the worst case for the ratios (this
    commit's slowest run against the parent's fastest), next to each library's own run-to-run spread."""
    runs = []
    for f in files:
        runs += [json.loads(line[3:]) for line in open(f) if line.startswith("AB ")]
    for r in runs:
        r["lib"] = "parent commit" if r["label"].startswith("parent") else "this commit"

    def med(key, who):
        return [r[key]["median"] for r in runs if r["label"].startswith(who) and key in r]

    def spread(v):
        return round(max(v) / min(v) - 1, 4) if v else None

    def mid(v):
        return round(float(np.median(v)), 2) if v else None

    def over(here, base):
        return round(max(here) / min(base) - 1, 4) if here and base else None

    summary = {}
    for k in (10, 100):
        a, b = med("sharded_grouped_k%d" % k, "this"), med("grouped_gather_k%d" % k, "this")
        summary["k%d" % k] = {
            "a_sharded_grouped_us": a, "b_grouped_gather_numpy_us": b, "c_sharded_us": med("sharded_k%d" % k, "this"),
            "a_over_b_worst": over(a, b), "a_not_slower_than_b": bool(a and b and max(a) <= min(b)),
            "parent_sharded_us": med("sharded_k%d" % k, "parent"), "this_sharded_us": med("sharded_k%d" % k, "this"),
            "parent_sharded_spread": spread(med("sharded_k%d" % k, "parent")),
            "this_sharded_over_parent_worst": over(med("sharded_k%d" % k, "this"), med("sharded_k%d" % k, "parent")),
            "parent_grouped_local_us": med("grouped_local_k%d" % k, "parent"), "this_grouped_local_us": med("grouped_local_k%d" % k, "this"),
            "parent_grouped_local_spread": spread(med("grouped_local_k%d" % k, "parent")),
            "this_grouped_local_over_parent_worst": over(med("grouped_local_k%d" % k, "this"), med("grouped_local_k%d" % k, "parent")),
            "a_equals_b": [r["a_equals_b_k%d" % k] for r in runs if "a_equals_b_k%d" % k in r],
            "median_of_runs": {"parent_sharded": mid(med("sharded_k%d" % k, "parent")), "this_sharded": mid(med("sharded_k%d" % k, "this")),
                               "parent_grouped_local": mid(med("grouped_local_k%d" % k, "parent")),
                               "this_grouped_local": mid(med("grouped_local_k%d" % k, "this"))},
        }
    out = {
        "what": "tools/ab_shard_grouped.py on one MI355X: two processes, two shard handles of 500 k x 768 f32 (one 1 M-row corpus), "
                "L2, groups of 8 rows, 64-query calls, host transport (gloo); us per query, medians of rank 0's host clock "
                "around the collective calls; the parent commit's library and this commit's in alternating runs, same box",
        "runs": runs,
        "summary": summary,
        "timeline_phase_sums_a_k10": [r["timeline_a_k10"] for r in runs if "timeline_a_k10" in r],
        "timeline_phase_sums_a_k100": [r["timeline_a_k100"] for r in runs if "timeline_a_k100" in r],
    }
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if len(sys.argv) > 1 and sys.argv[1] == "--merge":
    merge(sys.argv[2], sys.argv[3:])
    sys.exit(0)

import torch  # noqa: E402  (first: it brings its own ROCm runtime)
import torch.distributed as dist  # noqa: E402

torch.cuda.init()
torch.cuda.set_device(0)
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tostore_amd import _ffi  # noqa: E402

if os.environ.get("TSH_LIB_PATH"):  # another build's library: bind what it exports
    _L = ctypes.CDLL(_ffi.LIB_PATH)
    for _name in [s for s in _ffi.SIGNATURES if not hasattr(_L, s)]:
        del _ffi.SIGNATURES[_name]
from tostore_amd import HipVectorIndex  # noqa: E402
from tostore_amd.sharded import CommSearcher  # noqa: E402

label = sys.argv[1]
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 9
has_new = "tsh_search_sharded_grouped" in _ffi.SIGNATURES and not (len(sys.argv) > 3 and sys.argv[3] == "existing")
per, d, nq, gsize = 500_000, 768, 64, 8
n = per * world
lo = rank * per
rows = np.random.default_rng(2026 + rank).standard_normal((per, d), dtype=np.float32)  # this rank's rows of the corpus
qs = np.random.default_rng(7).standard_normal((nq, d), dtype=np.float32)
group_of = (np.arange(n) // gsize).astype(np.int32)  # GLOBAL; per is a multiple of 8: no group spans the ranks
out = {"label": label, "lib": "TSH_LIB_PATH" if os.environ.get("TSH_LIB_PATH") else "tree", "calls_of_64": calls, "world": world}


def timed(fn, reps, only_rank0=False):
    """only_rank0: the other ranks wait at the barriers, so rank 0 has the device to itself"""
    us = []
    for i in range(2 + reps):  # (the first two warm: code objects, contexts, pinned buffers, the communicator's buffers)
        dist.barrier()
        t0 = time.perf_counter()
        if rank == 0 or not only_rank0:
            fn()
        if i >= 2:
            us.append((time.perf_counter() - t0) * 1e6 / nq)
    dist.barrier()
    us = np.asarray(us)
    return {"median": round(float(np.median(us)), 2), "p10": round(float(np.percentile(us, 10)), 2),
            "p90": round(float(np.percentile(us, 90)), 2)}


def gather_merge(idx, h, k):
    """Today's way: this rank's grouped answer, the ranks' answers gathered on the host, then ordered (distance, id),
    repeated groups dropped, cut to k -- what tests/test_gpu_search_grouped.py spells out"""
    ids, dd, grp, cnt = idx.search_grouped(qs, k, h)
    mine = np.concatenate([np.ascontiguousarray(ids).view(np.float64), dd, grp.astype(np.float64)], axis=1)  # (ids travel as their bits)
    every = np.empty((world * nq, 3 * k))  # (rank r's answers in rows [r * nq, (r + 1) * nq))
    dist.all_gather_into_tensor(torch.from_numpy(every), torch.from_numpy(np.ascontiguousarray(mine)))
    every = every.reshape(world, nq, 3 * k)
    a_ids = every[:, :, :k].view(np.int64).transpose(1, 0, 2).reshape(nq, world * k)
    a_dd = every[:, :, k:2 * k].transpose(1, 0, 2).reshape(nq, world * k)
    a_grp = every[:, :, 2 * k:].astype(np.int32).transpose(1, 0, 2).reshape(nq, world * k)
    o_ids, o_dd = np.full((nq, k), -1, np.int64), np.full((nq, k), np.nan)
    for q in range(nq):
        live = a_ids[q] >= 0
        order = np.lexsort((a_ids[q][live], a_dd[q][live]))
        seen, keep = set(), []
        for j in order:
            g = int(a_grp[q][live][j])
            if g >= 0:
                if g in seen:
                    continue
                seen.add(g)
            keep.append(j)
            if len(keep) == k:
                break
        o_ids[q, :len(keep)] = a_ids[q][live][keep]
        o_dd[q, :len(keep)] = a_dd[q][live][keep]
    return o_ids, o_dd


with HipVectorIndex(d, 0, capacity_rows=per, shard_device=0, row_base=lo) as idx:
    idx.append(lo, rows)
    del rows
    with idx.make_groups(group_of, n // gsize) as h, CommSearcher.over_torch(idx, device=0) as cs:
        for k in (10, 100):
            out["sharded_k%d" % k] = timed(lambda: cs.search(qs, k), 5 * calls)
            out["grouped_local_k%d" % k] = timed(lambda: idx.search_grouped(qs, k, h), calls, only_rank0=True)
            if has_new:
                out["grouped_gather_k%d" % k] = timed(lambda: gather_merge(idx, h, k), calls)
                cs.timeline(reset=True)
                out["sharded_grouped_k%d" % k] = timed(lambda: cs.search(qs, k, groups=h), calls)
                tl = cs.timeline()
                out["timeline_a_k%d" % k] = {key: round(float(v), 1) for key, v in tl.items() if key.endswith("_us") or key in ("calls", "groups", "retries")}
                a = cs.search(qs, k, groups=h)
                b = gather_merge(idx, h, k)
                out["a_equals_b_k%d" % k] = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)))
                out["sharded_again_k%d" % k] = timed(lambda: cs.search(qs, k), 5 * calls)
if rank == 0:
    print("AB " + json.dumps(out), flush=True)
dist.barrier()
dist.destroy_process_group()
