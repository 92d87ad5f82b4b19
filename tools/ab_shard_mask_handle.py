"""What a mask handle saves a sharded search per call (profiles/shard_mask_handle_ab.json): one shard handle of 1 M x 768
f32 rows, L2, k = 100, blocks into a device buffer, default options.  Per process, us per call (host clock around calls that
return when the blocks are final):
  (a) tsh_search_shard, one query per call, behind a keep-1 % POINTER mask
  (b) the same through tsh_search_shard_masked with a HANDLE of that bitmap
  (c) 64-query calls behind a keep-50 % mask, pointer and handle
  (d) tsh_search_shard, one query per call, no mask
One process = one library (TSH_LIB_PATH names another build's libtostore_hip.so, e.g. the parent commit's, which is then
asked for (a), (c) by pointer and (d) only); run the two alternately: parent, this, parent, this.  Prints one JSON line.
usage: python tools/ab_shard_mask_handle.py LABEL [LONE_CALLS] [CALLS_OF_64]         (one run; LABEL starts with "parent"
                                                                                      for the parent commit's library)
       python tools/ab_shard_mask_handle.py --merge OUT.json FILE_OF_AB_LINES ...    (the runs' lines -> the profile file;
                                                                                      exit status 1 if a gate is missed)"""
import ctypes
import json
import os
import sys
import time
import zlib

import numpy as np


def merge(out_path, files):
    """The committed profile: every run's line, the medians side by side and the gates.
    Gate 1: in every process of this commit, (b)'s median is at most (a)'s -- the handle call does a strict subset of the
    pointer call's work.  Gate 2: the pointer and the unmasked entry did not move -- this commit's (a) and (d) medians lie
    within twice the spread (max - min) of the parent's own runs around them."""
    runs = []
    for f in files:
        runs += [json.loads(line[3:]) for line in open(f) if line.startswith("AB ")]
    for r in runs:
        r["lib"] = "parent commit" if r["label"].startswith("parent") else "this commit"

    def med(key, who):
        return [r[key]["median"] for r in runs if r["label"].startswith(who) and key in r]

    gates = {"b_at_most_a_in_every_process": [r["b_handle_1pct_lone"]["median"] <= r["a_pointer_1pct_lone"]["median"]
                                              for r in runs if "b_handle_1pct_lone" in r]}
    moved = {}
    for key in ("a_pointer_1pct_lone", "d_unmasked_lone"):
        base, here = med(key, "parent"), med(key, "this")
        spread = max(base) - min(base) if base else None
        moved[key] = {"parent_us": base, "this_us": here, "parent_spread_us": None if spread is None else round(spread, 2),
                      "allowed_us": None if spread is None else [round(min(base) - 2 * spread, 2), round(max(base) + 2 * spread, 2)],
                      "within": bool(base and here and all(min(base) - 2 * spread <= x <= max(base) + 2 * spread for x in here))}
    gates["a_and_d_within_twice_the_parents_spread"] = [moved[key]["within"] for key in moved]
    a, b = med("a_pointer_1pct_lone", "this"), med("b_handle_1pct_lone", "this")
    cp, ch = med("c_pointer_50pct_64", "this"), med("c_handle_50pct_64", "this")
    out = {
        "what": "tools/ab_shard_mask_handle.py on one MI355X: one shard handle of 1 M x 768 f32, L2, k = 100, blocks in device "
                "memory, default options; us per call (host clock around calls that return when the blocks are final); the "
                "parent commit's library and this commit's in alternating processes, same box",
        "runs": runs,
        "summary": {
            "a_pointer_1pct_lone_us": a, "b_handle_1pct_lone_us": b,
            "gain_lone_us_a_minus_b": [round(x - y, 2) for x, y in zip(a, b)],
            "c_pointer_50pct_64_us_per_call": cp, "c_handle_50pct_64_us_per_call": ch,
            "gain_64_us_per_call_pointer_minus_handle": [round(x - y, 2) for x, y in zip(cp, ch)],
            "pointer_and_unmasked_against_the_parent": moved,
            "gates": gates,
            "gates_met": bool(all(all(v) and len(v) > 0 for v in gates.values())),
            "handle_blocks_equal_pointer_blocks": [r["handle_blocks_equal_pointer_blocks"] for r in runs if "handle_blocks_equal_pointer_blocks" in r],
        },
    }
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["summary"], indent=1))
    return 0 if out["summary"]["gates_met"] else 1


if len(sys.argv) > 1 and sys.argv[1] == "--merge":
    sys.exit(merge(sys.argv[2], sys.argv[3:]))

import torch  # noqa: E402  (first: it brings its own ROCm runtime)

torch.cuda.init()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tostore_amd import _ffi  # noqa: E402

if os.environ.get("TSH_LIB_PATH"):  # another build's library: bind what it exports
    _L = ctypes.CDLL(_ffi.LIB_PATH)
    for _name in [s for s in _ffi.SIGNATURES if not hasattr(_L, s)]:
        del _ffi.SIGNATURES[_name]
from tostore_amd import HipVectorIndex  # noqa: E402

label = sys.argv[1]
lone_calls = int(sys.argv[2]) if len(sys.argv) > 2 else 400
calls_64 = int(sys.argv[3]) if len(sys.argv) > 3 else 12
has_masked = "tsh_search_shard_masked" in _ffi.SIGNATURES
n, d, k, nq, base, chunk = 1_000_000, 768, 100, 64, 2_000_003, 125_000  # (a base that is no multiple of 8)
rng = np.random.default_rng(2027)
qs = rng.standard_normal((nq, d), dtype=np.float32)
bits1 = np.zeros((base + n + 7) // 8, np.uint8)
bits50 = np.zeros_like(bits1)
for bits, p in ((bits1, 0.01), (bits50, 0.5)):  # GLOBAL bitmaps: bit = global row id
    keep = np.zeros(base + n, bool)
    keep[base:] = rng.random(n) < p
    bits[:] = np.packbits(keep, bitorder="little")
out = {"label": label, "lib": "TSH_LIB_PATH" if os.environ.get("TSH_LIB_PATH") else "tree", "lone_calls": lone_calls, "calls_of_64": calls_64}
L = _ffi.lib()
entries = L.tsh_default_block_entries(k)
bb = L.tsh_candidate_block_bytes(entries)
buf = torch.zeros(nq * bb, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
qp, bp = qs.ctypes.data_as(_ffi.p_f32), ctypes.c_void_p(buf.data_ptr())


def timed(fn, reps, blocks):
    for _ in range(5):  # warm: code objects, contexts, pinned buffers
        fn()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()  # returns when every block is final
        us.append((time.perf_counter() - t0) * 1e6)
    us = np.asarray(us)
    return {"median": round(float(np.median(us)), 2), "p10": round(float(np.percentile(us, 10)), 2),
            "p90": round(float(np.percentile(us, 90)), 2), "blocks_crc": zlib.crc32(buf.cpu().numpy()[:blocks * bb].tobytes())}


def canonical(blocks):
    """the blocks' entries up to their order within a block (places are drawn with atomic adds)"""
    raw = buf.cpu().numpy()
    got = []
    for i in range(blocks):
        b = raw[i * bb:(i + 1) * bb]
        count, ent = np.frombuffer(b[:8].tobytes(), np.uint32)
        body = b[64:64 + 24 * int(min(count, ent))].reshape(-1, 24)
        got.append((int(count), sorted(bytes(x) for x in body)))
    return got


with HipVectorIndex(d, 0, capacity_rows=n, shard_device=0, row_base=base) as idx:
    for at in range(0, n, chunk):
        idx.append(base + at, rng.standard_normal((chunk, d), dtype=np.float32))
    m1, m50 = bits1.ctypes.data_as(_ffi.p_u8), bits50.ctypes.data_as(_ffi.p_u8)
    out["d_unmasked_lone"] = timed(lambda: _ffi.check(L.tsh_search_shard(idx._h, qp, 1, k, None, entries, bp, None)), lone_calls, 1)
    out["a_pointer_1pct_lone"] = timed(lambda: _ffi.check(L.tsh_search_shard(idx._h, qp, 1, k, m1, entries, bp, None)), lone_calls, 1)
    by_pointer = canonical(1)
    if has_masked:
        with idx.make_mask(bits1) as h1, idx.make_mask(bits50) as h50:
            out["b_handle_1pct_lone"] = timed(lambda: _ffi.check(L.tsh_search_shard_masked(idx._h, qp, 1, k, h1.handle(), None, None, entries, bp, None)),
                                              lone_calls, 1)
            same = canonical(1) == by_pointer
            out["a_pointer_1pct_lone_again"] = timed(lambda: _ffi.check(L.tsh_search_shard(idx._h, qp, 1, k, m1, entries, bp, None)), lone_calls, 1)
            out["c_handle_50pct_64"] = timed(lambda: _ffi.check(L.tsh_search_shard_masked(idx._h, qp, nq, k, h50.handle(), None, None, entries, bp, None)),
                                             calls_64, nq)
            by_handle = canonical(nq)
            out["c_pointer_50pct_64"] = timed(lambda: _ffi.check(L.tsh_search_shard(idx._h, qp, nq, k, m50, entries, bp, None)), calls_64, nq)
            out["handle_blocks_equal_pointer_blocks"] = bool(same and canonical(nq) == by_handle)
    else:
        out["c_pointer_50pct_64"] = timed(lambda: _ffi.check(L.tsh_search_shard(idx._h, qp, nq, k, m50, entries, bp, None)), calls_64, nq)
    out["d_unmasked_lone_again"] = timed(lambda: _ffi.check(L.tsh_search_shard(idx._h, qp, 1, k, None, entries, bp, None)), lone_calls, 1)
print("AB " + json.dumps(out), flush=True)
