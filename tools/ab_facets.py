"""What facet counts on the device cost beside the two host routes (profiles/facets_ab.json): one index of 1 M x 768 f32
rows, L2, default options (the rows only have to be there: one random block of 125 000 rows is appended eight times), and
  tenant4 / tenant64 / tenant4096   a scalar column of 4, 64 and 4096 distinct values, uniform; the keys are all of them
  one_value                         a scalar column that is one value: every lane of every wave adds to one LDS counter
  price8                            a scalar column of skewed prices; 8 edges
  acl                               the ACL-shaped tag column of tools/ab_mask_tags.py: 1 - 8 group ids per row out of
                                    10 000; the keys are 64 of them
  tags                              its tag-shaped column: 0 - 32 tags per row out of 1 000; the keys are all 1 000
each with no mask and behind a bitmap-made handle that keeps 1 % and 50 % of the rows.  Per case, us per call by the
host clock:
  device      one tsh_attr_facets / tsh_tags_facets
  host_read   host route (a): tsh_mask_read, unpackbits, the column walked with NumPy (searchsorted + bincount for a scalar
              column, isin + bincount for a tag column; the owner array is made once, outside the clock)
  host_loop   host route (b): per key one device mask maker (tsh_mask_create_range / tsh_mask_create_tags, with = the mask)
              and one tsh_search_count under it.  At most LOOP_KEYS keys are run; the figure is their cost scaled to all keys
  range_make  for scale: one tsh_mask_create_range that keeps about half the rows (no list), and its destroy
The three routes' answers are compared before anything is timed.  The routes run alternately, round after round, in one
process; the medians of the rounds' medians are printed as one "AB" line.  A record is made of several processes' lines
(--merge): per figure the median over the processes with their lowest and highest.
The kernels' own time comes from a kernel trace taken in a run of its own, device route only (rocprofv3 --kernel-trace
-- python tools/ab_facets.py trace 1 20); --merge puts each case's kernel time into the record.  A library built with
another grid cap (-DTSH_FACET_MAX_BLOCKS=n, tostore_amd/build.py) is traced the same way through TSH_LIB_PATH and merged
with --merge-cap.
usage: python tools/ab_facets.py LABEL [ROUNDS] [DEVICE_CALLS_PER_ROUND] [HOST_CALLS_PER_ROUND]
       python tools/ab_facets.py --merge OUT.json FILE_OF_AB_LINES [KERNEL_TRACE.csv]
       python tools/ab_facets.py --merge-cap OUT.json CAP KERNEL_TRACE.csv"""
import csv
import json
import os
import sys
import time

import numpy as np

KERNELS = ("attr_facets_kernel", "tags_facets_kernel")
FIGURES = ("device_us", "host_read_us", "host_loop_us")
MASKS = ("none", "keep1", "keep50")
CASES = ("tenant4", "tenant64", "tenant4096", "one_value", "price8", "acl", "tags")
LOOP_KEYS = 16


def trace_by_case(trace_csv):
    """the two kernels' launches in the order they ran: the traced process makes the same number of calls for every case"""
    rows = [r for r in csv.DictReader(open(trace_csv)) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    names = [c + "_" + m for c in CASES for m in MASKS]
    assert us and len(us) % len(names) == 0, (len(us), len(names))
    each = len(us) // len(names)
    out = {}
    for i, name in enumerate(names):
        seg = us[i * each:(i + 1) * each]
        out[name] = {"launches": each, "median_us": round(float(np.median(seg)), 2), "lowest_us": round(min(seg), 2),
                     "highest_us": round(max(seg), 2)}
    return out


def merge(out_path, ab_file, trace_csv=None):
    runs = [json.loads(line[3:]) for line in open(ab_file) if line.startswith("AB ")]
    summary = {}
    for name in runs[0]["cases"]:
        s = {key: runs[0]["cases"][name][key] for key in ("keys", "population", "loop_keys_run")}
        for fig in FIGURES:
            per = [r["cases"][name][fig] for r in runs]
            s[fig] = {"median": round(float(np.median(per)), 2), "lowest": min(per), "highest": max(per), "processes": per}
        summary[name] = s
    per = [r["range_make_us"] for r in runs]
    out = {
        "what": "tools/ab_facets.py on one MI355X: 1 M x 768 f32, L2, default options; us per call by the host clock, the "
                "routes alternating round by round in every process, %d processes of one commit; device = one tsh_attr_facets "
                "/ tsh_tags_facets, host_read = tsh_mask_read + NumPy over the column, host_loop = a device mask maker and a "
                "tsh_search_count per key (at most %d keys run, scaled to all); per figure the median over the processes with "
                "their lowest and highest" % (len(runs), LOOP_KEYS),
        "processes": len(runs), "rounds": runs[0]["rounds"], "device_calls_per_round": runs[0]["device_calls"],
        "host_calls_per_round": runs[0]["host_calls"],
        "range_make_us": {"median": round(float(np.median(per)), 2), "lowest": min(per), "highest": max(per), "processes": per},
        "kernel_under_trace_by_case": trace_by_case(trace_csv) if trace_csv else {}, "kernel_under_trace_by_grid_cap": {},
        "summary": summary,
    }
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"summary": {n: {k: (v["median"] if isinstance(v, dict) else v) for k, v in s.items()} for n, s in summary.items()},
                      "range_make_us": out["range_make_us"]["median"], "kernel": out["kernel_under_trace_by_case"]}, indent=1))
    return 0


def merge_cap(out_path, cap, trace_csv):
    out = json.load(open(out_path))
    out["kernel_under_trace_by_grid_cap"][str(int(cap))] = {n: v["median_us"] for n, v in trace_by_case(trace_csv).items()}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if len(sys.argv) > 1 and sys.argv[1] == "--merge":
    sys.exit(merge(*sys.argv[2:5]))
if len(sys.argv) > 1 and sys.argv[1] == "--merge-cap":
    sys.exit(merge_cap(*sys.argv[2:5]))

import torch  # noqa: E402  (first: it brings its own ROCm runtime)

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tostore_amd import HipVectorIndex  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else "this"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
device_calls = int(sys.argv[3]) if len(sys.argv) > 3 else 60
host_calls = int(sys.argv[4]) if len(sys.argv) > 4 else 3
trace_only = label == "trace"  # (the device route alone: the trace then holds the same launches for every case)
n, d, chunk = 1_000_000, 768, 125_000
rng = np.random.default_rng(2034)
I64_MAX = (1 << 63) - 1


def tag_column(lo, hi, universe):
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


def median_us(fn, calls):
    for _ in range(2):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return round(float(np.median(t)), 2)


q = rng.standard_normal(d, dtype=np.float32)
out = {"label": label, "rounds": rounds, "device_calls": device_calls, "host_calls": host_calls, "rows": n, "dim": d, "cases": {}}
with HipVectorIndex(d, 0, capacity_rows=n) as idx:
    block = rng.standard_normal((chunk, d), dtype=np.float32)
    for at in range(0, n, chunk):
        idx.append(at, block)
    keeps = {"none": None, "keep1": rng.random(n) < 0.01, "keep50": rng.random(n) < 0.5}
    masks = {m: (idx.make_mask(np.packbits(k, bitorder="little")) if k is not None else None) for m, k in keeps.items()}

    def read_keep(m):
        return np.ones(n, bool) if m is None else np.unpackbits(m.bits(), bitorder="little")[:n].astype(bool)

    for cname in CASES:
        kind, owner = "values", None
        if cname.startswith("tenant"):
            distinct = int(cname[6:])
            col, keys = rng.integers(0, distinct, n).astype(np.int64), rng.permutation(distinct).astype(np.int64)
        elif cname == "one_value":
            col, keys = np.full(n, 7, np.int64), np.array([7], np.int64)
        elif cname == "price8":
            col = np.minimum(rng.lognormal(3.0, 1.2, n), 1e6).astype(np.int64)
            keys, kind = np.array([0, 5, 10, 20, 50, 100, 200, 500], np.int64), "edges"
        else:
            off, col, owner = tag_column(*((1, 8, 10_000) if cname == "acl" else (0, 32, 1_000)))
            keys = rng.permutation(rng.choice(10_000, 64, replace=False) if cname == "acl" else 1_000).astype(np.int64)
        handle = idx.make_tags((off, col)) if owner is not None else idx.make_attr(col)
        order = np.argsort(keys)
        skeys = keys[order]
        loop_keys = np.arange(len(keys))[:LOOP_KEYS]
        for mname, mask in masks.items():

            def device():
                return idx.facets(handle, keys, mask, kind)

            def host_read():
                keep = read_keep(mask)
                counts = np.zeros(len(keys), np.int64)
                if owner is not None:
                    hit = keep[owner] & np.isin(col, skeys)
                    counts[order] = np.bincount(np.searchsorted(skeys, col[hit]), minlength=len(keys))
                    holders = np.bincount(owner[hit], minlength=n) > 0
                    return counts, int((keep & ~holders).sum()), 0, int(keep.sum())
                v = col[keep]
                if kind == "edges":
                    b = np.searchsorted(skeys, v, side="right") - 1
                    counts = np.bincount(b[b >= 0], minlength=len(keys)).astype(np.int64)
                    return counts, int((b < 0).sum()), 0, len(v)
                at = np.minimum(np.searchsorted(skeys, v), len(keys) - 1)
                hit = skeys[at] == v
                counts[order] = np.bincount(at[hit], minlength=len(keys))
                return counts, int((~hit).sum()), 0, len(v)

            def loop_one(j):
                if owner is not None:
                    m = idx.make_mask_tags(handle, keys[j:j + 1], "any", with_mask=mask)
                elif kind == "edges":
                    m = idx.make_mask_where(handle, int(keys[j]), int(keys[j + 1]) - 1 if j + 1 < len(keys) else I64_MAX, with_mask=mask)
                else:
                    m = idx.make_mask_where(handle, int(keys[j]), int(keys[j]), with_mask=mask)
                c = int(idx.search_count(q, None, m)[0])
                m.close()
                return c

            def host_loop():
                return [loop_one(int(j)) for j in loop_keys]

            ref = device()
            res = {"keys": int(len(keys)), "population": int(ref[3]), "loop_keys_run": int(len(loop_keys))}
            if trace_only:
                for _ in range(rounds * device_calls):
                    device()
                continue
            got = host_read()
            assert np.array_equal(ref[0], got[0]) and tuple(ref[1:]) == tuple(got[1:]), (cname, mname, "host_read", ref, got)
            assert ref[0][loop_keys].tolist() == host_loop(), (cname, mname, "host_loop")
            per = {f: [] for f in FIGURES}
            for _ in range(rounds):
                per["device_us"].append(median_us(device, device_calls))
                per["host_read_us"].append(median_us(host_read, host_calls))
                per["host_loop_us"].append(round(median_us(host_loop, host_calls) * len(keys) / len(loop_keys), 2))
            for f, v in per.items():
                res[f] = round(float(np.median(v)), 2)
            res["rounds_us"] = per
            out["cases"][cname + "_" + mname] = res
        if cname == "tenant4" and not trace_only:
            def range_make():
                idx.make_mask_where(handle, 0, 1).close()
            out["range_make_us"] = round(float(np.median([median_us(range_make, device_calls) for _ in range(rounds)])), 2)
        handle.close()
print("AB " + json.dumps(out), flush=True)
