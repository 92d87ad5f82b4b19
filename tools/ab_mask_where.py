"""What making a WHERE mask on the device saves (profiles/mask_where_ab.json): one index of 1 M x 768 f32 rows, L2, k = 100,
default options, one int64 column (a tenant id, 100 values, uniform).  Two predicates: `tenant = 7` (about 1 % of the rows)
and `tenant BETWEEN 0 AND 49` (about 50 %).  Per predicate, us per call by the host clock (every call returns when its
handle is final, every search when its answer is):
  make_bitmap   tsh_mask_create alone, from a bitmap prepared beforehand
  make_host     the predicate on the host: the NumPy compare, packbits, then tsh_mask_create   (what a caller does today)
  make_range    tsh_mask_create_range from the resident column
  lone_*        one query including make and destroy, for each of the three ways
The ways run alternately, round after round (bitmap, host, range, bitmap, ...), and the medians of the rounds' medians are
reported with every round's own; no threshold is set, the comparison is make_host against make_range in the same run.
Under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/ab_mask_where.py trace 2 20) the kernels' own
durations say where make_range's time goes; --merge puts their averages into the record.
usage: python tools/ab_mask_where.py LABEL [ROUNDS] [CALLS_PER_ROUND]
       python tools/ab_mask_where.py --merge OUT.json FILE_OF_AB_LINES [KERNEL_STATS.csv]"""
import csv
import json
import os
import sys
import time

import numpy as np


def merge(out_path, ab_file, stats_csv=None):
    run = [json.loads(line[3:]) for line in open(ab_file) if line.startswith("AB ")][-1]
    kernels = {}
    if stats_csv:
        for row in csv.DictReader(open(stats_csv)):
            name = row.get("Name", "")
            for kern in ("mask_range_kernel", "mask_block_count_kernel", "mask_compact_kernel"):
                if kern in name:
                    kernels[kern] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2)}
    s = run["summary"]
    fold = None
    if "mask_block_count_kernel" in kernels:
        m1, make = kernels["mask_block_count_kernel"]["average_us"], s["eq_1pct"]["make_range_us"]
        nolist = s["range_50pct"]["make_range_us"]
        fold = {"m1_folded_into_the_range_kernel": False, "m1_kernel_us": m1, "make_range_1pct_us": make,
                "make_range_50pct_no_list_us": nolist,
                "why": "the two timings: M1 runs %.1f us (kernel trace) inside a make_range call of %.1f us.  Folding its popcount "
                       "into the range kernel saves at most that -- under a tenth of the call, which is already a fraction of the "
                       "host route -- and would tie the range kernel's workgroups to M2's 256-word blocks.  The whole list stage "
                       "(M1, M2, the padding, the 4-byte total, a second synchronise) is the %.1f us between the 1 %% call and "
                       "the 50 %% call, which makes no list; the rest is the range kernel, the copy of the words back to the host "
                       "and the host prefix" % (m1, make, make - nolist)}
    out = {
        "what": "tools/ab_mask_where.py on one MI355X: 1 M x 768 f32, L2, k = 100, default options, one int64 column; us per "
                "call by the host clock, the three ways of making a handle alternating round by round in one process of one "
                "commit; make_host = NumPy compare + packbits + tsh_mask_create, make_range = tsh_mask_create_range",
        "run": run, "kernels_under_trace": kernels, "m1_fold": fold, "summary": s,
    }
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"summary": s, "kernels": kernels, "m1_fold": fold}, indent=1))
    return 0


if len(sys.argv) > 1 and sys.argv[1] == "--merge":
    sys.exit(merge(*sys.argv[2:5]))

import torch  # noqa: E402  (first: it brings its own ROCm runtime)

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tostore_amd import HipVectorIndex  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else "this"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 60
n, d, k, chunk = 1_000_000, 768, 100, 125_000
rng = np.random.default_rng(2031)
tenant = rng.integers(0, 100, n).astype(np.int64)
q = rng.standard_normal(d, dtype=np.float32)
PRED = {"eq_1pct": (7, 7), "range_50pct": (0, 49)}


def us_of(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t))


out = {"label": label, "rounds": rounds, "calls_per_round": calls, "rows": n, "dim": d, "k": k}
with HipVectorIndex(d, 0, capacity_rows=n) as idx:
    for at in range(0, n, chunk):
        idx.append(at, rng.standard_normal((chunk, d), dtype=np.float32))
    attr = idx.make_attr(tenant)
    for name, (lo, hi) in PRED.items():
        ready = np.packbits((tenant >= lo) & (tenant <= hi), bitorder="little")

        def make_bitmap():
            return idx.make_mask(ready)

        def make_host():
            return idx.make_mask(np.packbits((tenant >= lo) & (tenant <= hi), bitorder="little"))

        def make_range():
            return idx.make_mask_where(attr, lo, hi)

        ways = {"bitmap": make_bitmap, "host": make_host, "range": make_range}
        ref = None
        for way, mk in ways.items():  # warm: code objects, contexts; and the three ways' answers agree
            with mk() as m:
                got = (m.kept, idx.search(q, k, None, m))
            if ref is None:
                ref = got
            assert got[0] == ref[0] and np.array_equal(got[1][0], ref[1][0]) and np.array_equal(got[1][1], ref[1][1]), way
        per = {"make_" + w: [] for w in ways}
        per.update({"lone_" + w: [] for w in ways})
        for _ in range(rounds):
            for way, mk in ways.items():
                def lone(mk=mk):
                    with mk() as m:
                        idx.search(q, k, None, m)

                for _w in range(3):
                    lone()
                # (the make's time is the call's alone: the destroy is timed apart and taken off)
                t_make = []
                for _c in range(calls):
                    t0 = time.perf_counter()
                    m = mk()
                    t_make.append((time.perf_counter() - t0) * 1e6)
                    m.close()
                per["make_" + way].append(round(float(np.median(t_make)), 2))
                per["lone_" + way].append(round(us_of(lone, calls), 2))
        res = {"kept": int(ref[0]), "rounds_us": per}
        for key, v in per.items():
            res[key + "_us"] = round(float(np.median(v)), 2)
        out[name] = res
    attr.close()
out["summary"] = {name: {key: out[name][key] for key in out[name] if key.endswith("_us") and key != "rounds_us"} | {"kept": out[name]["kept"]}
                  for name in PRED}
for name in PRED:
    s = out["summary"][name]
    s["make_range_over_make_host"] = round(s["make_range_us"] / s["make_host_us"], 3)
    s["lone_range_over_lone_host"] = round(s["lone_range_us"] / s["lone_host_us"], 3)
print("AB " + json.dumps(out), flush=True)
