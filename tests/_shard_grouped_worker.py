"""Worker of tests/test_gpu_comm_shard_grouped.py: one of W ranks sharing the test box's ONE GPU, running the library's
sharded grouped search (tsh_search_sharded_grouped) -- over the host transport (gloo underneath, started by
torch.distributed.run) or over the RCCL branch against tests/fake_rccl (TSH_RCCL_LIB; the id travels through a file).
Every rank checks the full answer against the oracle on the whole corpus (repeated groups dropped) and against a single
un-sharded tsh_search_grouped, and prints a digest of what it got -- ids, distances and groups: the parent compares the
ranks' digests.

argv: rows  host | rccl  [id-file]"""
import hashlib
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
from tostore_amd import HipMask, HipVectorIndex, _ffi  # noqa: E402
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


def first_of_each_group(eids, edist, group_of, k):
    """The specification over an oracle list: (ids, dist, groups)"""
    keep, groups, seen = [], [], set()
    for i, gid in enumerate(eids):
        if len(keep) >= k:
            break
        g = int(group_of[gid]) if gid < len(group_of) and group_of[gid] >= 0 else -1
        if g >= 0:
            if g in seen:
                continue
            seen.add(g)
        keep.append(i)
        groups.append(g)
    keep = np.asarray(keep, np.int64)
    return eids[keep], edist[keep], np.asarray(groups, np.int32)


def same_one(got, i, want):
    ids, dd, cnt, grp = got
    wi, wd, wg = want
    c = int(cnt[i])
    return bool(c == len(wi) and np.array_equal(ids[i, :c], wi) and np.array_equal(dd[i, :c].view(np.uint64), wd.view(np.uint64))
                and np.array_equal(grp[i, :c], wg) and np.all(ids[i, c:] == -1) and np.all(grp[i, c:] == -1))


digest = hashlib.sha256()


def note(ids, dd, cnt, grp):
    for i in range(len(cnt)):
        digest.update(np.ascontiguousarray(ids[i, :cnt[i]]).tobytes())
        digest.update(np.ascontiguousarray(dd[i, :cnt[i]]).tobytes())
        digest.update(np.ascontiguousarray(grp[i, :cnt[i]]).tobytes())


rng = np.random.default_rng(0)  # same corpus on every rank
rows = rng.standard_normal((n, d)).astype(np.float32)
per = (n + world - 1) // world
lo, hi = min(n, rank * per), min(n, (rank + 1) * per)
nq, k, metric, NG = 16, 10, 0, 300
qs = rng.standard_normal((nq, d)).astype(np.float32)
rows[per - 1] = rows[per] = rows[3]                      # ties across a shard boundary -> global id order
rows[per + 100:per + 500] = qs[4] + np.float32(0.01)     # 400 identical rows nearest to query 4, inside rank 1's shard ...
group_of = (np.arange(n) % NG).astype(np.int32)          # every group has rows on every rank
group_of[rng.random(n) < 0.05] = -1
group_of[per + 100:per + 500] = 7                        # ... in ONE group: 399 side rows, more than a block of 192 holds
full = [oracle.search_exhaustive(rows, q, metric, n) for q in qs]  # computed once, never changed
want = [first_of_each_group(e, ed, group_of, k) for e, ed in full]


def check(got, idxs=range(nq)):
    return all(same_one(got, j, want[i]) for j, i in enumerate(idxs))


idx = HipVectorIndex(d, metric, capacity_rows=hi - lo, shard_device=0, row_base=lo)
idx.append(lo, rows[lo:hi])
idx.set_batch_min_nq(0)
groups = idx.make_groups(group_of, NG)
cs = CommSearcher.over_torch(idx, device=0) if transport == "host" else CommSearcher(idx, world, rank, share_id(), 0)
others = [i for i in range(nq) if i != 4]  # (query 4 is the overflow retry's)

# ---- 15 queries: the oracle's list with repeated groups dropped, and what ONE un-sharded index answers
got = cs.search(qs[others], k, groups=groups)
say("15 queries against the oracle", check(got, others))
note(*got)
whole = HipVectorIndex(d, metric, capacity_rows=n)
whole.append(0, rows)
with whole.make_groups(group_of, NG) as wh:
    w_ids, w_dd, w_grp, w_cnt = whole.search_grouped(qs[others], k, wh)
whole.close()
say("15 queries against tsh_search_grouped", bool(np.array_equal(got[2], w_cnt) and np.array_equal(got[0], w_ids) and np.array_equal(got[3], w_grp)
                                                  and np.array_equal(got[1].view(np.uint64), w_dd.view(np.uint64))))
# ---- the groups really span the ranks: every group has rows on every rank, the ranks' own first-k lists repeat a group,
# and a winning group is offered by a rank that does not hold its best row
spans = all(all(((np.flatnonzero(group_of == g) >= r * per) & (np.flatnonzero(group_of == g) < (r + 1) * per)).any() for r in range(world))
            for g in range(NG))
e, ed = full[1]
k_span = 40  # (40 of 300 groups from every rank: the ranks' lists overlap for certain)
span_want = first_of_each_group(e, ed, group_of, k_span)
offers = [first_of_each_group(e[(e >= r * per) & (e < (r + 1) * per)], ed[(e >= r * per) & (e < (r + 1) * per)], group_of, k_span)[2]
          for r in range(world)]
flat = [g for o in offers for g in o.tolist() if g >= 0]
crossed = sum(any(g in offers[r].tolist() for r in range(world) if r != rid // per) for rid, g in zip(span_want[0], span_want[2]) if g >= 0)
got = cs.search(qs[1], k_span, groups=groups)
say("groups span every rank", bool(spans and len(set(flat)) < len(flat) and crossed >= 1 and same_one(got, 0, span_want)))
note(*got)
# ---- a mask by pointer and by handle, with a threshold
keep = np.packbits(rng.random(n) < 0.3, bitorder="little")
m_ids, m_dd = oracle.search_exhaustive(rows, qs[2], metric, n, None, keep)
thr = float(first_of_each_group(m_ids, m_dd, group_of, 60)[1][-1])
e, ed = oracle.search_exhaustive(rows, qs[2], metric, n, thr, keep)
m_want = first_of_each_group(e, ed, group_of, 100)
got = cs.search(qs[2], 100, thr, keep, groups=groups)
say("mask by pointer + threshold", same_one(got, 0, m_want))
note(*got)
with HipMask(idx, keep) as mh:
    got = cs.search(qs[2], 100, thr, mh, groups=groups)
say("mask by handle + threshold", same_one(got, 0, m_want))
note(*got)
# ---- 399 side rows on rank 1 do not fit its block: every rank retries the group with larger blocks
t0 = cs.timeline()
got = cs.search(qs[4], k, groups=groups)
t1 = cs.timeline()
say("overflow retry", bool(same_one(got, 0, want[4]) and t1["retries"] > t0["retries"] and got[3][0, 0] == 7))
note(*got)
# ---- 20 queries under the library's own schedule (the shrinking groups; shards this small go as one group, tsh_host_sync.h),
# every rank's handle asking for the matrix cores: never batched; then in groups of 5: four exchanges, later scans running
# while earlier groups are exchanged
q20 = [others[i % len(others)] for i in range(20)]
idx.set_batch_min_nq(1)
c0, t0 = idx.counters(), cs.timeline()
got = cs.search(qs[q20], k, groups=groups)
c1, t1 = idx.counters(), cs.timeline()
say("20 queries in shrinking groups, never batched", bool(check(got, q20) and c1["batch_launches"] == c0["batch_launches"]
                                                         and c1["scan_launches"] - c0["scan_launches"] >= 20 and t1["groups"] - t0["groups"] >= 1))
note(*got)
cs.set_group(5)
t0 = cs.timeline()
got = cs.search(qs[q20], k, groups=groups)
t1 = cs.timeline()
cs.set_group(0)
say("20 queries in groups of 5", bool(check(got, q20) and t1["groups"] - t0["groups"] == 4 and idx.counters()["batch_launches"] == c0["batch_launches"]))
note(*got)
idx.set_batch_min_nq(0)
# ---- with the exchange asked to go out ahead: a grouped call still exchanges final blocks; same results, retry included
_ffi.check(_ffi.lib().tsh_index_set_option(None, _ffi.TSH_OPT_EXCHANGE_AHEAD, 1))
t0 = cs.timeline()
got = cs.search(qs, k, groups=groups)
t1 = cs.timeline()
say("exchange ahead set and ignored", bool(check(got) and t1["retries"] > t0["retries"] and t1["pre_enqueue_us"] == t0["pre_enqueue_us"]))
note(*got)
_ffi.check(_ffi.lib().tsh_index_set_option(None, _ffi.TSH_OPT_EXCHANGE_AHEAD, 0))
# ---- the last rank passes a groups handle of another index: its own error there, TSH_E_PEER on its peers, and the next
# call succeeds everywhere
small = HipVectorIndex(d, metric, capacity_rows=64, shard_device=0, row_base=0)
small.append(0, rows[:64])
foreign = small.make_groups(group_of[:64], NG)
code = None
try:
    if rank == world - 1:
        cs.search(qs[:3], k, groups_handle=foreign.handle())
    else:
        cs.search(qs[:3], k, groups=groups)
except _ffi.TshError as err:
    code = err.code
foreign.close()
small.close()
again = cs.search(qs[:3], k, groups=groups)
say("a bad groups handle is a local failure", bool(code == (_ffi.TSH_E_BAD_ARG if rank == world - 1 else _ffi.TSH_E_PEER) and check(again, range(3))))
# ---- 80 queries as ONE group: more blocks than are merged whole, so every rank merges its slice and a second all-gather
# hands out ids and distances -- the groups of the slices other ranks merged come from this rank's own table
q80 = [others[i % len(others)] for i in range(80)]
cs.set_group(80)
got = cs.search(qs[q80], k, groups=groups)
cs.set_group(0)
say("out_group of slice owners and non-owners", check(got, q80))
note(*got)
os.write(1, ("rank %d digest %s\n" % (rank, digest.hexdigest())).encode())
groups.close()
cs.close()
idx.close()
if transport == "host":
    dist.barrier()
    dist.destroy_process_group()
