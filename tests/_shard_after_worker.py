"""Worker of tests/test_gpu_comm_shard_after.py: one of W ranks sharing the test box's ONE GPU, running the library's
sharded cursor search (tsh_search_sharded_after) -- over the host transport (gloo underneath, started by
torch.distributed.run) or over the RCCL branch against tests/fake_rccl (TSH_RCCL_LIB; the id travels through a file).
Every rank checks the full answer against the oracle on the whole corpus and against a single un-sharded
tsh_search_after, and prints a digest of what it got: the parent compares the ranks' digests.

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
from tostore_amd.sharded import CommSearcher  # noqa: E402

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


digest = hashlib.sha256()


def note(ids, dd, cnt):
    for i in range(len(cnt)):
        digest.update(np.ascontiguousarray(ids[i, :cnt[i]]).tobytes())
        digest.update(np.ascontiguousarray(dd[i, :cnt[i]]).tobytes())


rng = np.random.default_rng(0)  # same corpus on every rank
rows = rng.standard_normal((n, d)).astype(np.float32)
per = (n + world - 1) // world
lo, hi = min(n, rank * per), min(n, (rank + 1) * per)
rows[per - 1] = rows[per] = rows[3]           # ties across a shard boundary -> global id order
rows[per + 100:per + 500] = rows[per + 50]    # a crowd wider than a block, inside rank 1's shard
nq, k, metric = 16, 10, 0
qs = rng.standard_normal((nq, d)).astype(np.float32)
full = [oracle.search_exhaustive(rows, q, metric, n) for q in qs]  # computed once, never changed
at = [0, 1, 9, 10, 11, 99, 500, n // 2, n - 30, n - 11, n - 10, n - 2, n - 1, 37, 250, 1000]
ad = np.asarray([-math.inf] + [float(full[i][1][at[i]]) for i in range(1, nq)])
ai = np.asarray([0] + [int(full[i][0][at[i]]) for i in range(1, nq)], np.int64)


def expect(i, kk=k):
    a = 0 if i == 0 else at[i] + 1
    return full[i][0][a:a + kk], full[i][1][a:a + kk]


def check(got, kk=k):
    ids, dd, cnt = got
    ok = True
    for i in range(nq):
        e, ed = expect(i, kk)
        ok &= bool(cnt[i] == len(e) and np.array_equal(ids[i, :cnt[i]], e) and same_dist(dd[i, :cnt[i]], ed))
    return ok


idx = HipVectorIndex(d, metric, capacity_rows=hi - lo, shard_device=0, row_base=lo)
idx.append(lo, rows[lo:hi])
idx.set_batch_min_nq(0)
cs = CommSearcher.over_torch(idx, device=0) if transport == "host" else CommSearcher(idx, world, rank, share_id(), 0)

# ---- 16 queries, a cursor each: the oracle's list after each cursor, and what ONE un-sharded index answers
got = cs.search(qs, k, after=(ad, ai))
say("16 cursors against the oracle", check(got))
note(*got)
whole = HipVectorIndex(d, metric, capacity_rows=n)
whole.append(0, rows)
w_ids, w_dd, w_cnt = whole.search_after(qs, k, (ad, ai))
whole.close()
say("16 cursors against tsh_search_after", bool(np.array_equal(got[2], w_cnt) and all(
    np.array_equal(got[0][i, :w_cnt[i]], w_ids[i, :w_cnt[i]]) and same_dist(got[1][i, :w_cnt[i]], w_dd[i, :w_cnt[i]]) for i in range(nq))))
say("-inf is the cursor-less call", bool(np.array_equal(cs.search(qs[:3], k)[0], cs.search(qs[:3], k, after=(-math.inf, 5))[0])))
# ---- one (distance, id) for every query, a threshold, a mask
keep = np.packbits(rng.random(n) < 0.3, bitorder="little")
m_ids, m_dd = oracle.search_exhaustive(rows, qs[2], metric, n, None, keep)
thr = float(m_dd[60])
got = cs.search(qs[2], 100, thr, keep, after=(float(m_dd[20]), int(m_ids[20])))
e, ed = oracle.search_exhaustive(rows, qs[2], metric, n, thr, keep)
say("masked + threshold", bool(got[2][0] == len(e) - 21 and np.array_equal(got[0][0, :got[2][0]], e[21:]) and same_dist(got[1][0, :got[2][0]], ed[21:])))
note(*got)
# ---- every rank's handle asks for the matrix cores: a cursor call is never batched, and the groups are the scan
# schedule's on every rank
idx.set_batch_min_nq(1)
c0 = idx.counters()
got = cs.search(qs, k, after=(ad, ai))
c1 = idx.counters()
say("never batched", check(got) and c1["batch_launches"] == c0["batch_launches"] and c1["scan_launches"] - c0["scan_launches"] >= nq)
idx.set_batch_min_nq(0)
cs.set_group(5)
say("groups of 5", check(cs.search(qs, k, after=(ad, ai))))
cs.set_group(0)
# ---- a cursor in the middle of a crowd wider than a block: every rank retries the group with larger blocks
q = qs[4]
e, ed = full[4]
first = int(np.flatnonzero(e == per + 50)[0])
mid = first + 200
t0 = cs.timeline()
got = cs.search(q, k, after=(float(ed[mid]), int(e[mid])))
t1 = cs.timeline()
say("overflow retry behind a cursor", bool(got[2][0] == k and np.array_equal(got[0][0], e[mid + 1:mid + 1 + k]) and same_dist(got[1][0], ed[mid + 1:mid + 1 + k])
                                           and t1["retries"] > t0["retries"]))
note(*got)
# ---- a page walk of one query through the collective, to exhaustion
ids_all, dd_all, cur, pages, kk = [], [], (-math.inf, 0), 0, 64
while True:
    ids, dd, cnt = cs.search(qs[7], kk, after=cur)
    c = int(cnt[0])
    pages += 1
    ids_all.append(ids[0, :c].copy())
    dd_all.append(dd[0, :c].copy())
    if c:
        cur = (float(dd[0, c - 1]), int(ids[0, c - 1]))
    if c < kk or pages > n:
        break
ids_all, dd_all = np.concatenate(ids_all), np.concatenate(dd_all)
say("page walk (%d pages)" % pages, bool(np.array_equal(ids_all, full[7][0]) and same_dist(dd_all, full[7][1]) and pages == n // kk + 1
                                         and cs.search(qs[7], kk, after=cur)[2][0] == 0))
digest.update(ids_all.tobytes())
digest.update(dd_all.tobytes())
# ---- with the exchange asked to go out ahead: a cursor call still exchanges final blocks; same results
_ffi.check(_ffi.lib().tsh_index_set_option(None, _ffi.TSH_OPT_EXCHANGE_AHEAD, 1))
got = cs.search(qs, k, after=(ad, ai))
say("exchange ahead set: 16 cursors", check(got))
got = cs.search(q, k, after=(float(ed[mid]), int(e[mid])))
say("exchange ahead set: overflow retry", bool(got[2][0] == k and np.array_equal(got[0][0], e[mid + 1:mid + 1 + k])))
_ffi.check(_ffi.lib().tsh_index_set_option(None, _ffi.TSH_OPT_EXCHANGE_AHEAD, 0))
os.write(1, ("rank %d digest %s\n" % (rank, digest.hexdigest())).encode())
cs.close()
idx.close()
if transport == "host":
    dist.barrier()
    dist.destroy_process_group()
