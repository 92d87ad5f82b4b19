"""Worker of tests/test_gpu_comm_shard_mask_handle.py: one of W ranks sharing the test box's ONE GPU, running the library's
sharded search with a mask HANDLE per rank (tsh_search_sharded_masked) -- over the host transport (gloo underneath,
started by torch.distributed.run) or over the RCCL branch against tests/fake_rccl (TSH_RCCL_LIB; the id travels through a
file).  Every rank makes its handle from the same GLOBAL bitmap, holds the handle call to the pointer call
(tsh_search_sharded with the bitmap) and to the oracle on the whole corpus, and prints a digest of what it got: the
parent compares the ranks' digests.

argv: rows  host | rccl  [id-file]"""
import hashlib
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle  # noqa: E402

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
n, transport, d = int(sys.argv[1]), sys.argv[2], 64
if transport == "host":
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
from tostore_amd import HipVectorIndex, _ffi  # noqa: E402
from tostore_amd.sharded import CommSearcher, ShardedSearcher  # noqa: E402

if transport == "rccl":
    assert os.environ.get("TSH_RCCL_LIB"), "the rccl transport of this worker is for the stand-in library only"
    _ffi.enable_test_hooks()  # TSH_RCCL_LIB is obeyed only in a process that asked for the test hooks


def say(what, ok):
    # one write() per line: the ranks share the parent's pipe and print() would interleave words
    os.write(1, ("rank %d %s %s\n" % (rank, what, "ok" if ok else "MISMATCH")).encode())


def share_id():
    """rank 0 makes the id and publishes it (write + rename: never seen half-written); the others pick it up"""
    path = sys.argv[3]
    if rank == 0:
        uid = CommSearcher.unique_id()
        with open(path + ".tmp", "wb") as f:
            f.write(uid)
        os.rename(path + ".tmp", path)
        return uid
    t0 = time.time()
    while not os.path.exists(path):
        if time.time() - t0 > 120:
            raise RuntimeError("rank 0 never published the communicator id")
        time.sleep(0.01)
    return open(path, "rb").read()


def same_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return bool(a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def same(a, b):
    return bool(np.array_equal(a[2], b[2]) and all(
        np.array_equal(a[0][i, :a[2][i]], b[0][i, :a[2][i]]) and same_dist(a[1][i, :a[2][i]], b[1][i, :a[2][i]]) for i in range(len(a[2]))))


digest = hashlib.sha256()


def note(ids, dd, cnt):
    for i in range(len(cnt)):
        digest.update(np.ascontiguousarray(ids[i, :cnt[i]]).tobytes())
        digest.update(np.ascontiguousarray(dd[i, :cnt[i]]).tobytes())


rng = np.random.default_rng(0)  # same corpus on every rank
rows = rng.standard_normal((n, d)).astype(np.float32)
per = (n + world - 1) // world
lo, hi = min(n, rank * per), min(n, (rank + 1) * per)
rows[per + 100:per + 500] = rows[per + 50]    # a crowd wider than a block, inside rank 1's shard
nq, k, metric = 20, 10, 0
qs = rng.standard_normal((nq, d)).astype(np.float32)
few = np.packbits(rng.random(n) < 0.03, bitorder="little")
half_keep = rng.random(n) < 0.5
half_keep[per + 50:per + 500] = True  # (the crowd is kept)
half = np.packbits(half_keep, bitorder="little")


def oracle_many(queries, kk, keep):
    """(ids, dist, count) padded like the library's answer; computed on every rank from the same inputs"""
    q = np.asarray(queries, np.float32).reshape(-1, d)
    ids, dd, cnt = np.full((len(q), kk), -1, np.int64), np.full((len(q), kk), np.nan), np.zeros(len(q), np.int32)
    for i, x in enumerate(q):
        e, ed = oracle.search_exhaustive(rows, x, metric, kk, None, keep)
        cnt[i] = len(e)
        ids[i, :cnt[i]], dd[i, :cnt[i]] = e, ed
    return ids, dd, cnt


idx = HipVectorIndex(d, metric, capacity_rows=hi - lo, shard_device=0, row_base=lo)
idx.append(lo, rows[lo:hi])
idx.set_batch_min_nq(0)
cs = CommSearcher.over_torch(idx, device=0) if transport == "host" else CommSearcher(idx, world, rank, share_id(), 0)
h_few, h_half = idx.make_mask(few), idx.make_mask(half)  # this rank's handles of the GLOBAL bitmaps

# ---- 20 queries (the shrinking groups) and one query, behind a 3 % and a 50 % handle: the pointer call, the oracle
for name, bits, h in (("3 %", few, h_few), ("50 %", half, h_half)):
    got = cs.search(qs, k, row_mask=h)
    say("20 queries behind a %s handle" % name, same(got, cs.search(qs, k, row_mask=bits)) and same(got, oracle_many(qs, k, bits)))
    note(*got)
    one = cs.search(qs[5], k, row_mask=h)
    say("one query behind a %s handle" % name, same(one, cs.search(qs[5], k, row_mask=bits)) and same(one, oracle_many(qs[5], k, bits)))
    note(*one)
# ---- the cursor form: a page walk of one query to exhaustion behind the handle
e, ed = oracle.search_exhaustive(rows, qs[7], metric, n, None, half)
ids_all, dd_all, cur, pages, kk = [], [], (-math.inf, 0), 0, 64
while True:
    ids, dd, cnt = cs.search(qs[7], kk, row_mask=h_half, after=cur)
    c = int(cnt[0])
    pages += 1
    ids_all.append(ids[0, :c].copy())
    dd_all.append(dd[0, :c].copy())
    if c:
        cur = (float(dd[0, c - 1]), int(ids[0, c - 1]))
    if c < kk or pages > n:
        break
ids_all, dd_all = np.concatenate(ids_all), np.concatenate(dd_all)
say("page walk behind a handle (%d pages)" % pages, bool(np.array_equal(ids_all, e) and same_dist(dd_all, ed) and pages == len(e) // kk + 1))
digest.update(ids_all.tobytes())
digest.update(dd_all.tobytes())
at = 1000
page = cs.search(qs[7], k, row_mask=h_half, after=(float(ed[at]), int(e[at])))
say("one page: handle against pointer", same(page, cs.search(qs[7], k, row_mask=half, after=(float(ed[at]), int(e[at]))))
    and bool(np.array_equal(page[0][0], e[at + 1:at + 1 + k])))
note(*page)
# ---- a crowd of ties wider than a block: the collective's overflow retry reads the handle too (on the f32 tile scan,
# whose keys cannot tell the copies apart: the exact path would order a shard this small by id itself)
q = rows[per + 50].copy()
idx.set_exact_scan_rows(0)
t0 = cs.timeline()
got = cs.search(q, k, row_mask=h_half)
t1 = cs.timeline()
say("overflow retry behind a handle", t1["retries"] > t0["retries"] and same(got, oracle_many(q, k, half)) and same(got, cs.search(q, k, row_mask=half)))
note(*got)
idx.set_exact_scan_rows(16384)  # (the default)
# ---- the Python searchers: CommSearcher.search_many and ShardedSearcher with a HipMask
got = cs.search_many(qs, k, row_mask=h_few, group=6)
say("CommSearcher.search_many(row_mask=HipMask)", same(got, oracle_many(qs, k, few)))
note(*got)
if transport == "host":  # (the torch searcher over the same gloo group: every rank's blocks are merged)
    ss = ShardedSearcher(idx)
    a = ss.search(qs, k, row_mask=h_few)
    b = ss.search_many(qs, k, row_mask=h_half, group=6)
    c = ss.search(qs[7], k, row_mask=h_half, after=(float(ed[at]), int(e[at])))
    idx.set_exact_scan_rows(0)
    t = ss.search(q, k, row_mask=h_half)  # (the crowd: its overflow retry goes through the handle as well)
    idx.set_exact_scan_rows(16384)
    say("ShardedSearcher with a HipMask", same(a, oracle_many(qs, k, few)) and same(b, oracle_many(qs, k, half)) and same(c, page)
        and same(t, oracle_many(q, k, half)) and same(a, cs.search(qs, k, row_mask=h_few)))
    note(*a)
    note(*b)
# ---- rank 1 passes a handle made for a second, unrelated index: its own failure, the peers' TSH_E_PEER, and the
# communicator goes on
other = HipVectorIndex(d, metric, capacity_rows=64, shard_device=0, row_base=lo)
other.append(lo, rows[lo:lo + 64])
h_other = other.make_mask(few)
code = 0
try:
    cs.search(qs[:3], k, row_mask=h_other if rank == 1 else h_few)
except _ffi.TshError as err:
    code = err.code
say("a handle of another index on rank 1 (%d)" % code, code == (_ffi.TSH_E_BAD_ARG if rank == 1 else _ffi.TSH_E_PEER))
got = cs.search(qs[:3], k, row_mask=h_few)
say("the communicator goes on", same(got, oracle_many(qs[:3], k, few)))
note(*got)
h_other.close()
other.close()
os.write(1, ("rank %d digest %s\n" % (rank, digest.hexdigest())).encode())
h_few.close()
h_half.close()
cs.close()
idx.close()
if transport == "host":
    dist.barrier()
    dist.destroy_process_group()
