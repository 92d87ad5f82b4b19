"""The int8 route's tail and the inline finaliser against the parent commit (profiles/i8_tail_ab.json): 1 M x 768 f32, L2,
k = 100, batched path off, host clock around calls that return their results.  One process = one library (TSH_LIB_PATH
names another build's libtostore_hip.so, e.g. the parent commit's); run the two alternately.  Prints one JSON line.
  call64       64-query calls, dense: us per call                (the end of a pipelined call: tail once, finaliser)
  call20       20-query calls, dense: us per call                (the driver's regions)
  lone         single queries, dense: p50 us                     (the whole tail every time)
  keep50_*     the same behind a keep-50 % mask handle           (the masked int8 route)
usage: python tools/ab_i8_tail.py LABEL [CALLS [LONE_QUERIES]]        (one run; LABEL starts with "parent" for the parent
                                                                      commit's library)
       python tools/ab_i8_tail.py --merge OUT.json FILE_OF_AB_LINES ...  (the runs' lines -> the profile file)"""
import json
import os
import sys
import time
import zlib

import numpy as np

CASES = ("call64", "call20", "lone", "keep50_call64", "keep50_lone")


def merge(out_path, files):
    """Per case and side the runs' medians; a case MOVED only if the gap between the two sides' medians of medians is
    larger than the larger of the two sides' (max - min)."""
    runs = []
    for f in files:
        runs += [json.loads(line[3:]) for line in open(f) if line.startswith("AB ")]
    for r in runs:
        r["lib"] = "parent commit" if r["label"].startswith("parent") else "this commit"
    summary = {}
    for case in CASES:
        side = {who: [r[case]["median_us"] for r in runs if r["label"].startswith(who) and case in r] for who in ("parent", "this")}
        if not side["parent"] or not side["this"]:
            continue
        mp, mt = float(np.median(side["parent"])), float(np.median(side["this"]))
        spread = max(max(v) - min(v) for v in side.values())
        summary[case] = {"parent_medians_us": side["parent"], "this_medians_us": side["this"], "parent_us": round(mp, 2), "this_us": round(mt, 2),
                         "gap_us": round(mp - mt, 2), "larger_spread_us": round(spread, 2),
                         "verdict": "faster" if mp - mt > spread else ("slower" if mt - mp > spread else "within spread")}
    crcs = {r["answer_crc"] for r in runs}
    out = {"what": "tools/ab_i8_tail.py on one MI355X: 1 M x 768 f32, L2, k = 100, single-query pipeline; the parent commit's library "
                   "and this commit's in alternating processes, same box; us per call (host clock)",
           "answers_identical_across_runs": len(crcs) == 1, "summary": summary, "runs": runs}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(summary, indent=1))


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tostore_amd import HipVectorIndex

    label = sys.argv[1]
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 15
    lone_n = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    n, d, k = 1_000_000, 768, 100
    rng = np.random.default_rng(2025)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    rows *= rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    qs = rng.standard_normal((256, d), dtype=np.float32)
    keep = np.packbits(rng.random(n) < 0.5, bitorder="little")
    out = {"label": label, "lib": os.environ.get("TSH_LIB_PATH", "tree"), "calls": calls, "lone_queries": lone_n}
    crc = 0
    with HipVectorIndex(d, 0, capacity_rows=n) as idx:
        idx.set_batch_min_nq(0)
        idx.append(0, rows)

        def run(what, nq, reps, mask):
            nonlocal crc
            for i in range(3):  # warm: builds the copy, loads the code objects, fills the context pool
                idx.search(qs[:nq], k, None, mask)
            i0 = idx.scan_i8_stats()
            us = []
            for i in range(reps):
                q = qs[(i * nq) % (256 - nq + 1):][:nq]
                t0 = time.perf_counter()
                got = idx.search(q, k, None, mask)
                us.append((time.perf_counter() - t0) * 1e6)
                crc = zlib.crc32(got[0].tobytes() + got[1].tobytes() + got[2].tobytes(), crc)
            i1 = idx.scan_i8_stats()
            s = sorted(us)
            out[what] = {"median_us": round(float(np.median(us)), 2), "min_us": round(s[0], 2), "p90_us": round(s[len(s) * 9 // 10], 2),
                         "i8_scans": i1["scans"] - i0["scans"], "i8_redone": i1["redone"] - i0["redone"]}

        run("call64", 64, calls, None)
        run("call20", 20, 2 * calls, None)
        run("lone", 1, lone_n, None)
        with idx.make_mask(keep) as h:
            run("keep50_call64", 64, max(calls // 2, 3), h)
            run("keep50_lone", 1, lone_n // 2, h)
    out["answer_crc"] = crc
    print("AB " + json.dumps(out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--merge":
        merge(sys.argv[2], sys.argv[3:])
    else:
        main()
