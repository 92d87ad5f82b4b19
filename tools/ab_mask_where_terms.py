"""What one launch for a whole WHERE clause saves (profiles/mask_where_terms_ab.json): one index of 1 M x 768 f32 rows, L2,
k = 100, default options, three int64 columns -- a tenant id (100 values, uniform), a timestamp, a flag -- and a tenant id of
a wider domain (10 000 values).  Three predicates:
  and3     tenant = 7 AND ts BETWEEN a AND b AND NOT flag = 1
  in16     tenant IN (16 values)
  in1024   wide_tenant IN (1024 values)
Per predicate, us per call by the host clock (every call returns when its handle is final, every search when its answer is):
  make_chain   the chain of tsh_mask_create_range calls as a caller writes it today, the intermediates destroyed; for in1024
               the host route instead (NumPy isin, packbits, tsh_mask_create): nobody would chain 1024 calls
  make_one     one tsh_mask_create_where
  lone_*       one query including make and destroy, for each of the two ways
The ways run alternately, round after round (chain, one, chain, ...), and the medians of the rounds' medians are reported
with every round's own; no ratio is fixed in advance, the comparison is make_chain against make_one in the same run.
Under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/ab_mask_where_terms.py trace 2 20) the kernels' own
durations say where the time goes; --merge puts their averages into the record.
usage: python tools/ab_mask_where_terms.py LABEL [ROUNDS] [CALLS_PER_ROUND]
       python tools/ab_mask_where_terms.py --merge OUT.json FILE_OF_AB_LINES [KERNEL_STATS.csv]"""
import csv
import json
import os
import sys
import time

import numpy as np

KERNELS = ("mask_where_kernel", "mask_range_kernel", "mask_block_count_kernel", "mask_compact_kernel")


def merge(out_path, ab_file, stats_csv=None):
    run = [json.loads(line[3:]) for line in open(ab_file) if line.startswith("AB ")][-1]
    kernels = {}
    if stats_csv:
        for row in csv.DictReader(open(stats_csv)):
            name = row.get("Name", "")
            for kern in KERNELS:
                if kern in name:
                    kernels[kern] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2)}
    s = run["summary"]
    slower = [name for name in s if s[name]["make_one_over_make_chain"] > 1.0 or s[name]["lone_one_over_lone_chain"] > 1.0]
    out = {
        "what": "tools/ab_mask_where_terms.py on one MI355X: 1 M x 768 f32, L2, k = 100, default options, int64 columns; us per "
                "call by the host clock, the two ways of making a handle alternating round by round in one process of one "
                "commit; make_chain = the chain of tsh_mask_create_range calls (in1024: NumPy isin + packbits + "
                "tsh_mask_create), make_one = one tsh_mask_create_where",
        "run": run, "kernels_under_trace": kernels, "summary": s,
        "one_call_slower_than_the_chain": slower,
    }
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"summary": s, "kernels": kernels, "one_call_slower_than_the_chain": slower}, indent=1))
    return 0


if len(sys.argv) > 1 and sys.argv[1] == "--merge":
    sys.exit(merge(*sys.argv[2:5]))

import torch  # noqa: E402  (first: it brings its own ROCm runtime)

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tostore_amd import HipVectorIndex, WhereIn, WhereRange  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else "this"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 60
n, d, k, chunk = 1_000_000, 768, 100, 125_000
rng = np.random.default_rng(2032)
tenant = rng.integers(0, 100, n).astype(np.int64)
wide = rng.integers(0, 10_000, n).astype(np.int64)
ts = rng.integers(1_700_000_000, 1_700_001_000, n).astype(np.int64)
flag = rng.integers(0, 2, n).astype(np.int64)
ts_a, ts_b = 1_700_000_200, 1_700_000_700
in16 = np.sort(rng.choice(100, 16, replace=False)).astype(np.int64)
in1024 = rng.permutation(rng.choice(10_000, 1024, replace=False)).astype(np.int64)
q = rng.standard_normal(d, dtype=np.float32)


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
    a_tenant, a_wide, a_ts, a_flag = idx.make_attr(tenant), idx.make_attr(wide), idx.make_attr(ts), idx.make_attr(flag)

    def chain_and3():
        m1 = idx.make_mask_where(a_tenant, 7, 7)
        m2 = idx.make_mask_where(a_ts, ts_a, ts_b, with_mask=m1)
        m1.close()
        m3 = idx.make_mask_where(a_flag, 1, 1, negate=True, with_mask=m2)
        m2.close()
        return m3

    def one_and3():
        return idx.make_mask_clauses([[WhereRange(a_tenant, 7, 7)], [WhereRange(a_ts, ts_a, ts_b)], [WhereRange(a_flag, 1, 1, negate=True)]])

    def chain_in16():
        m = idx.make_mask_where(a_tenant, int(in16[0]), int(in16[0]))
        for v in in16[1:]:
            nxt = idx.make_mask_where(a_tenant, int(v), int(v), with_mask=m, combine="or")
            m.close()
            m = nxt
        return m

    def one_in16():
        return idx.make_mask_clauses([[WhereIn(a_tenant, in16)]])

    def host_in1024():
        return idx.make_mask(np.packbits(np.isin(wide, in1024), bitorder="little"))

    def one_in1024():
        return idx.make_mask_clauses([[WhereIn(a_wide, in1024)]])

    PRED = {"and3": {"chain": chain_and3, "one": one_and3}, "in16": {"chain": chain_in16, "one": one_in16},
            "in1024": {"chain": host_in1024, "one": one_in1024}}
    for name, ways in PRED.items():
        ref = None
        for way, mk in ways.items():  # warm: code objects, contexts; and the two ways' answers agree
            with mk() as m:
                got = (m.kept, m.bits(), idx.search(q, k, None, m))
            if ref is None:
                ref = got
            assert got[0] == ref[0] and np.array_equal(got[1], ref[1]), way
            assert np.array_equal(got[2][0], ref[2][0]) and np.array_equal(got[2][1], ref[2][1]), way
        per = {"make_" + w: [] for w in ways}
        per.update({"lone_" + w: [] for w in ways})
        for _ in range(rounds):
            for way, mk in ways.items():
                def lone(mk=mk):
                    with mk() as m:
                        idx.search(q, k, None, m)

                for _w in range(3):
                    lone()
                # (the make's time is the call's alone -- a chain's includes destroying its intermediates, as its caller
                # must --; the final handle's destroy is timed apart and taken off)
                t_make = []
                for _c in range(calls):
                    t0 = time.perf_counter()
                    m = mk()
                    t_make.append((time.perf_counter() - t0) * 1e6)
                    m.close()
                per["make_" + way].append(round(float(np.median(t_make)), 2))
                per["lone_" + way].append(round(us_of(lone, calls), 2))
        res = {"kept": int(ref[0]), "chain_is": "host route" if name == "in1024" else "%d tsh_mask_create_range calls" % (3 if name == "and3" else 16),
               "rounds_us": per}
        for key, v in per.items():
            res[key + "_us"] = round(float(np.median(v)), 2)
        out[name] = res
    for a in (a_tenant, a_wide, a_ts, a_flag):
        a.close()
out["summary"] = {name: {key: out[name][key] for key in out[name] if key.endswith("_us") and key != "rounds_us"}
                  | {"kept": out[name]["kept"], "chain_is": out[name]["chain_is"]} for name in PRED}
for name in PRED:
    s = out["summary"][name]
    s["make_one_over_make_chain"] = round(s["make_one_us"] / s["make_chain_us"], 3)
    s["lone_one_over_lone_chain"] = round(s["lone_one_us"] / s["lone_chain_us"], 3)
print("AB " + json.dumps(out), flush=True)
