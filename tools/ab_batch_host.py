"""The batched path's host side against another build of it (profiles/batch_host_refactor_ab.json): same decisions, same
speed.  One process = one library (TSH_LIB_PATH names another build's libtostore_hip.so, e.g. the parent commit's); run
the two alternately on one box.
  same   a fixed seeded sequence of batched calls on one shard of 150 k x 96 per metric: key kernels 0 / 1 / 2 / auto,
         9 / 64 / 130 / 1024 queries, Bernoulli and range masks by pointer and by handle, a 1 % mask (listed mode), an
         append and an overwrite between calls, the norm-grouped plane on and off.  Writes one record per call -- hashes
         of ids, distance bits and counts, tsh_counters field by field (all but the scan timer), tsh_probe_batch_row_band's
         output -- to OUT.json; --compare says where two such files differ.  Everything must be equal.
  speed  1 M x 768: 1024-query calls, cosine and L2, 64-query calls, and a 64-query call behind a 1 % mask (queries/s of
         the median call).  With TSH_TRACE_BATCH=1 in the environment the run reports the host's prep / enqueue
         microseconds of the 1024-query calls instead, read back from the library's trace lines (tracing adds event
         records to a call, so such a run's queries/s are not counted).  Prints one "AB {json}" line.
  bench  LABEL FILE: bench.py's result line in FILE as such a line (its ms per step).
usage: python tools/ab_batch_host.py same LABEL OUT.json
       python tools/ab_batch_host.py --compare A.json B.json
       python tools/ab_batch_host.py speed LABEL [CALLS]                     (LABEL starts with "parent" for the baseline)
       python tools/ab_batch_host.py bench LABEL BENCH_OUTPUT_FILE
       python tools/ab_batch_host.py --merge OUT.json FILE_OF_AB_LINES ...   (the runs' lines -> the profile file)"""
import ctypes
import hashlib
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

FIGURES = ("bench_ms_per_step", "cos_1024_qps", "l2_1024_qps", "cos_1024_prep_us", "cos_1024_enqueue_us", "l2_1024_prep_us",
           "l2_1024_enqueue_us", "cos_64_qps", "cos_64_masked_1pct_qps")


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    bad = 0
    if len(a["calls"]) != len(b["calls"]):
        print("different numbers of calls: %d against %d" % (len(a["calls"]), len(b["calls"])))
        bad += 1
    for x, y in zip(a["calls"], b["calls"]):
        for key in sorted(set(x) | set(y)):
            if x.get(key) != y.get(key):
                print("call %d (%s): %s differs: %r against %r" % (x["n"], x["what"], key, x.get(key), y.get(key)))
                bad += 1
    print("%s against %s: %d calls, %d differences" % (a["label"], b["label"], len(a["calls"]), bad))
    return bad


def merge(out_path, files):
    """The committed profile: every run's line and, per figure, both sides' medians and whether this commit's median
    lies inside the parent's own min .. max."""
    runs = []
    for f in files:
        runs += [json.loads(line[3:]) for line in open(f) if line.startswith("AB ")]
    for r in runs:
        r["lib"] = "parent commit" if r["label"].startswith("parent") else "this commit"
    summary = {}
    for key in FIGURES:
        counted = [r for r in runs if r.get(key) is not None and (key.endswith("_us") or not r.get("trace"))]
        par = [r[key] for r in counted if r["label"].startswith("parent")]
        new = [r[key] for r in counted if not r["label"].startswith("parent")]
        if par and new:
            med = float(np.median(new))
            summary[key] = {"parent_runs": par, "this_runs": new, "parent_median": float(np.median(par)), "this_median": med,
                            "parent_min": min(par), "parent_max": max(par), "this_median_inside_parent_range": min(par) <= med <= max(par)}
    out = {"what": "tools/ab_batch_host.py speed (and bench.py's default line) on one MI355X, the parent commit's library and this "
                   "commit's in alternating processes, every run counted", "runs": runs, "summary": summary}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


if len(sys.argv) > 1 and sys.argv[1] == "--compare":
    sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
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

mode, label = sys.argv[1], sys.argv[2]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def same(out_path):
    n, d, extra = 150_000, 96, 10_000
    calls = []

    def record(idx, what, qs, k, mask=None):
        rec = {"n": len(calls), "what": what}
        try:
            ids, dist, cnt = idx.search(qs, k, None, mask)
            rec.update(ids=digest(ids), dist=digest(dist.view(np.uint64)), cnt=digest(cnt), found=int(cnt.sum()))
        except Exception as e:  # noqa: BLE001 -- an error is an answer too: both libraries must give the same one
            rec["error"] = str(e)
        c = idx.counters()
        c.pop("scan_us_sum")  # a timer
        rec["counters"] = c
        try:
            a2, b2 = idx.probe_batch_row_band(qs.shape[0])
            rec["row_band"] = [digest(a2), digest(b2)]
        except Exception as e:  # noqa: BLE001
            rec["row_band"] = str(e)
        calls.append(rec)

    for metric in (0, 1, 2):
        rng = np.random.default_rng(4100 + metric)
        rows = rng.standard_normal((n + extra, d), dtype=np.float32)
        if metric != 2:
            rows *= rng.uniform(0.5, 2.0, size=(n + extra, 1)).astype(np.float32)
        qs = rng.standard_normal((1024, d), dtype=np.float32)
        bern = np.packbits(rng.random(n + extra) < 0.5, bitorder="little")
        span = np.zeros(n + extra, dtype=bool)
        span[90_000:105_000] = True
        span = np.packbits(span, bitorder="little")
        one = np.packbits(rng.random(n + extra) < 0.01, bitorder="little")
        with HipVectorIndex(d, metric, capacity_rows=n + extra) as idx:
            idx.set_batch_min_nq(2)
            idx.append(0, rows[:n])
            for grouped in ((True, False) if metric == 0 else (True,)):
                idx.set_batch_group(grouped)
                for kern in (3, 2, 1, 0):
                    idx.set_batch_kernel(kern)
                    tag = "metric %d group %d kernel %d" % (metric, grouped, kern)
                    for nq in (9, 64, 130, 1024):
                        record(idx, "%s nq %d k 10" % (tag, nq), qs[:nq], 10)
                    record(idx, "%s nq 130 k 100" % tag, qs[:130], 100)
                    with HipMask(idx, bern) as hb, HipMask(idx, span) as hs, HipMask(idx, one) as ho:
                        for name, ptr, handle in (("bernoulli", bern, hb), ("range", span, hs), ("one percent", one, ho)):
                            for nq in (9, 130):
                                record(idx, "%s nq %d %s by pointer" % (tag, nq, name), qs[:nq], 10, ptr)
                                record(idx, "%s nq %d %s by handle" % (tag, nq, name), qs[:nq], 10, handle)
                        record(idx, "%s nq 1024 one percent by handle k 100" % tag, qs, 100, ho)
            # the store grows, then rows change in place: the planes follow
            idx.set_batch_group(True)
            idx.set_batch_kernel(3)
            idx.append(n, rows[n:])
            record(idx, "metric %d after an append" % metric, qs[:64], 10)
            record(idx, "metric %d after an append, range by pointer" % metric, qs[:130], 10, span)
            idx.append(20_000, rows[n:n + 5_000] * np.float32(1.5))
            record(idx, "metric %d after an overwrite" % metric, qs[:64], 10)
            record(idx, "metric %d after an overwrite, 1024" % metric, qs, 10)
            record(idx, "metric %d after an overwrite, one percent by pointer" % metric, qs[:64], 10, one)
    with open(out_path, "w") as f:
        json.dump({"label": label, "calls": calls}, f, indent=1)
    print("%s: %d calls recorded in %s" % (label, len(calls), out_path))


def speed(calls):
    n, d, k = 1_000_000, 768, 10
    trace = os.environ.get("TSH_TRACE_BATCH") is not None
    out = {"label": label, "lib": "TSH_LIB_PATH" if os.environ.get("TSH_LIB_PATH") else "tree", "calls": calls, "trace": trace}

    def timed(fn, nq):
        """queries/s of the median call, and the medians of the library's own prep / enqueue figures when it traces"""
        for _ in range(3):
            fn()
        sys.stderr.flush()
        saved, tmp = os.dup(2), tempfile.TemporaryFile()
        if trace:
            os.dup2(tmp.fileno(), 2)  # the library writes its trace lines to stderr
        us = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            us.append((time.perf_counter() - t0) * 1e6)
        os.dup2(saved, 2)
        os.close(saved)
        tmp.seek(0)
        lines = re.findall(r"prep (\d+) us, enqueue (\d+) us", tmp.read().decode(errors="replace"))
        prep = float(np.median([int(a) for a, _ in lines])) if lines else None
        enq = float(np.median([int(b) for _, b in lines])) if lines else None
        return round(nq / float(np.median(us)) * 1e6, 1), prep, enq

    rng = np.random.default_rng(2027)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    rows *= rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    qs = rng.standard_normal((2048, d), dtype=np.float32)
    one = np.packbits(rng.random(n) < 0.01, bitorder="little")
    for name, metric in (("l2", 0), ("cos", 2)):
        with HipVectorIndex(d, metric, capacity_rows=n) as idx:
            idx.set_batch_min_nq(1)
            idx.append(0, rows)
            flip = [0]

            def call(nq, mask=None):
                flip[0] ^= 1
                return idx.search(qs[flip[0] * nq:(flip[0] + 1) * nq], k, None, mask)

            out[name + "_1024_qps"], out[name + "_1024_prep_us"], out[name + "_1024_enqueue_us"] = timed(lambda: call(1024), 1024)
            if metric == 2 and not trace:
                out["cos_64_qps"] = timed(lambda: call(64), 64)[0]
                with HipMask(idx, one) as h:
                    out["cos_64_masked_1pct_qps"] = timed(lambda: call(64, h), 64)[0]
            out[name + "_kernel"] = idx.counters()["batch_kernel_last"]
    print("AB " + json.dumps(out), flush=True)


if mode == "same":
    same(sys.argv[3])
elif mode == "bench":
    line = [ln for ln in open(sys.argv[3]) if ln.startswith("{")][-1]
    res = json.loads(line)
    print("AB " + json.dumps({"label": label, "bench_ms_per_step": res["ms_per_step"], "bench_value": res["value"],
                              "bench_batch_1024_ms_per_step": (res.get("batch_1024") or {}).get("ms_per_step")}), flush=True)
else:
    speed(int(sys.argv[3]) if len(sys.argv) > 3 else 200)
