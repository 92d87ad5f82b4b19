"""What a tag column on the device saves over the host route (profiles/mask_tags_ab.json): one index of 1 M x 768 f32 rows,
L2, k = 100, default options, and two array-valued columns (every row's list distinct values, no NULL rows):
  acl    1 - 8 group ids per row out of 10 000
  tags   0 - 32 tags per row out of 1 000
Per column four terms: HAS ANY of 5, of 64 and of 1024 values, HAS ALL of 2.  Per term, us per call by the host clock (every
call returns when its handle is final, every search when its answer is):
  make_host    the host route: NumPy isin over the flat values, bincount of the hits by owner row (the owner array is made
               once, outside the clock), compare with the threshold, packbits, tsh_mask_create
  make_device  one tsh_mask_create_tags over the resident column
  lone_*       one query including make and destroy, for each of the two ways
The ways run alternately, round after round, in one process; the medians of the rounds' medians are printed as one "AB"
line.  A record is made of several processes' lines (--merge): per figure the median over the processes, and their lowest
and highest, which is the run-to-run spread a difference has to exceed.  No ratio is fixed in advance.
The kernel's own time comes from a kernel trace taken in a run of its own (rocprofv3 --kernel-trace --stats -- python
tools/ab_mask_tags.py trace 1 20 2); --merge puts the averages, and T1's own time term by term, into the record.
usage: python tools/ab_mask_tags.py LABEL [ROUNDS] [DEVICE_CALLS_PER_ROUND] [HOST_CALLS_PER_ROUND]
       python tools/ab_mask_tags.py --merge OUT.json FILE_OF_AB_LINES [KERNEL_STATS.csv [KERNEL_TRACE.csv]]"""
import csv
import json
import os
import sys
import time

import numpy as np

KERNELS = ("mask_tags_kernel", "mask_block_count_kernel", "mask_compact_kernel")
FIGURES = ("make_host_us", "make_device_us", "lone_host_us", "lone_device_us")


def merge(out_path, ab_file, stats_csv=None, trace_csv=None):
    runs = [json.loads(line[3:]) for line in open(ab_file) if line.startswith("AB ")]
    kernels, per_term = {}, {}
    if trace_csv:
        # T1's launches in the order they ran: the traced process makes the same number of handles for every term
        rows = [r for r in csv.DictReader(open(trace_csv)) if KERNELS[0] in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
        names = list(runs[0]["terms"])
        assert us and len(us) % len(names) == 0, (len(us), len(names))
        each = len(us) // len(names)
        for i, name in enumerate(names):
            seg = us[i * each:(i + 1) * each]
            per_term[name] = {"launches": each, "median_us": round(float(np.median(seg)), 2), "lowest_us": round(min(seg), 2),
                              "highest_us": round(max(seg), 2)}
    if stats_csv:
        for row in csv.DictReader(open(stats_csv)):
            name = row.get("Name", "")
            for kern in KERNELS:
                if kern in name:
                    kernels[kern] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2)}
    summary, not_faster = {}, []
    for name in runs[0]["terms"]:
        s = {key: runs[0]["terms"][name][key] for key in ("kept", "stored_values", "set_values", "need")}
        for fig in FIGURES:
            per = [r["terms"][name][fig] for r in runs]
            s[fig] = {"median": round(float(np.median(per)), 2), "lowest": min(per), "highest": max(per), "processes": per}
        for what in ("make", "lone"):
            h, dv = s[what + "_host_us"], s[what + "_device_us"]
            s[what + "_device_over_host"] = round(dv["median"] / h["median"], 4)
            # faster by more than the spread: the device's slowest process under the host's fastest
            if not dv["highest"] < h["lowest"]:
                not_faster.append(name + ":" + what)
        summary[name] = s
    out = {
        "what": "tools/ab_mask_tags.py on one MI355X: 1 M x 768 f32, L2, k = 100, default options; us per call by the host clock, "
                "the two ways of making a handle alternating round by round in every process, %d processes of one commit; "
                "make_host = NumPy isin + bincount by owner + compare + packbits + tsh_mask_create, make_device = one "
                "tsh_mask_create_tags; per figure the median over the processes with their lowest and highest" % len(runs),
        "processes": len(runs), "rounds": runs[0]["rounds"], "device_calls_per_round": runs[0]["device_calls"],
        "host_calls_per_round": runs[0]["host_calls"], "columns": runs[0]["columns"],
        "kernels_under_trace": kernels, "mask_tags_kernel_under_trace_by_term": per_term, "summary": summary,
        "device_not_faster_than_host_beyond_the_spread": not_faster,
    }
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"summary": {n: {k: (v["median"] if isinstance(v, dict) else v) for k, v in s.items()} for n, s in summary.items()},
                      "kernels": kernels, "mask_tags_kernel_by_term": per_term, "device_not_faster_than_host_beyond_the_spread": not_faster}, indent=1))
    return 0


if len(sys.argv) > 1 and sys.argv[1] == "--merge":
    sys.exit(merge(*sys.argv[2:6]))

import torch  # noqa: E402  (first: it brings its own ROCm runtime)

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tostore_amd import HipVectorIndex  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else "this"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
device_calls = int(sys.argv[3]) if len(sys.argv) > 3 else 60
host_calls = int(sys.argv[4]) if len(sys.argv) > 4 else 5
n, d, k, chunk = 1_000_000, 768, 100, 125_000
rng = np.random.default_rng(2033)


def column(lo, hi, universe):
    """lists of lo .. hi values of [0, universe), distinct within a row, as CSR; and the owner row of every value"""
    lens = rng.integers(lo, hi + 1, n)
    owner = np.repeat(np.arange(n), lens)
    vals = rng.integers(0, universe, len(owner)).astype(np.int64)
    order = np.lexsort((vals, owner))
    owner, vals = owner[order], vals[order]
    first = np.ones(len(vals), bool)
    first[1:] = (vals[1:] != vals[:-1]) | (owner[1:] != owner[:-1])
    owner, vals = owner[first], vals[first]
    off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=n))]).astype(np.int64)
    return off, np.ascontiguousarray(vals), owner


COLUMNS = {"acl": (1, 8, 10_000), "tags": (0, 32, 1_000)}
q = rng.standard_normal(d, dtype=np.float32)
out = {"label": label, "rounds": rounds, "device_calls": device_calls, "host_calls": host_calls, "rows": n, "dim": d, "k": k,
       "columns": {c: {"per_row": [lo, hi], "universe": u} for c, (lo, hi, u) in COLUMNS.items()}, "terms": {}}
with HipVectorIndex(d, 0, capacity_rows=n) as idx:
    for at in range(0, n, chunk):
        idx.append(at, rng.standard_normal((chunk, d), dtype=np.float32))
    for cname, (lo, hi, universe) in COLUMNS.items():
        off, vals, owner = column(lo, hi, universe)
        handle = idx.make_tags((off, vals))
        for tname, size, need in (("any5", 5, "any"), ("any64", 64, "any"), ("any1024", 1024, "any"), ("all2", 2, "all")):
            S = rng.permutation(rng.choice(universe, min(size, universe), replace=False)).astype(np.int64)
            t = len(S) if need == "all" else 1

            def host(S=S, t=t):
                c = np.bincount(owner[np.isin(vals, S)], minlength=n)
                return idx.make_mask(np.packbits(c >= t, bitorder="little"))

            def device(S=S, need=need):
                return idx.make_mask_tags(handle, S, need)

            ways = {"host": (host, host_calls), "device": (device, device_calls)}
            ref = None
            for way, (mk, _) in ways.items():  # warm: code objects, contexts; and the two ways' answers agree
                with mk() as m:
                    got = (m.kept, m.bits(), idx.search(q, k, None, m))
                if ref is None:
                    ref = got
                cnt = int(got[2][2][0])
                assert cnt == min(k, got[0]), (way, cname, tname, "kept", got[0], "count", cnt)
                assert got[0] == ref[0] and np.array_equal(got[1], ref[1]), way
                assert cnt == int(ref[2][2][0]) and np.array_equal(got[2][0][0, :cnt], ref[2][0][0, :cnt]), way
                assert np.array_equal(got[2][1][0, :cnt].view(np.uint64), ref[2][1][0, :cnt].view(np.uint64)), way
            per = {w + "_" + way: [] for w in ("make", "lone") for way in ways}
            for _ in range(rounds):
                for way, (mk, calls) in ways.items():
                    for _w in range(2):
                        with mk() as m:
                            idx.search(q, k, None, m)
                    # (the make's time is the call's alone; the lone query is the same call, its search and its destroy)
                    t_make, t_lone = [], []
                    for _c in range(calls):
                        t0 = time.perf_counter()
                        m = mk()
                        t1 = time.perf_counter()
                        idx.search(q, k, None, m)
                        m.close()
                        t2 = time.perf_counter()
                        t_make.append((t1 - t0) * 1e6)
                        t_lone.append((t2 - t0) * 1e6)
                    per["make_" + way].append(round(float(np.median(t_make)), 2))
                    per["lone_" + way].append(round(float(np.median(t_lone)), 2))
            res = {"kept": int(ref[0]), "stored_values": int(len(vals)), "set_values": int(len(S)), "need": need, "rounds_us": per}
            for key, v in per.items():
                res[key + "_us"] = round(float(np.median(v)), 2)
            out["terms"][cname + "_" + tname] = res
        handle.close()
print("AB " + json.dumps(out), flush=True)
