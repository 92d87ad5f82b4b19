"""Row-range sharded search, one process per GPU.

Rank g holds global rows [base_g, base_g + n_g) in its own `HipVectorIndex`
shard.  A query is scanned by every rank; each rank's fixed-size candidate
block (exact f64 sums of every row that can be in ITS top k) stays in device
memory, the blocks are all-gathered with `torch.distributed` (backend "nccl"
is RCCL over xGMI on ROCm; k'*24 B per rank per query, latency-bound), and the
host merge (`tsh_merge_candidates`: sqrt / negate / 1-cos, threshold, ordering,
top-k cut) runs on whichever ranks want the answer.  The reference has no
counterpart (it has no distributed compute at all); the
result is identical to one un-sharded index over the same rows.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np

from . import _ffi


def cursor_arrays(after, nq: int):
    """`after` -- one (distance, id) for every query, or nq of them -- as the (after_dist[nq], after_id[nq]) arrays
    the *_after entries take (tsh_search_after's cursor: GLOBAL, the same on every rank).  A pair of such arrays
    passes through."""
    if isinstance(after, tuple) and len(after) == 2 and all(isinstance(x, np.ndarray) and x.ndim == 1 for x in after):
        ad = np.ascontiguousarray(after[0], dtype=np.float64)
        ai = np.ascontiguousarray(after[1], dtype=np.int64)
        if ad.shape[0] != nq or ai.shape[0] != nq:
            raise ValueError("after: one distance and one id per query")
        return ad, ai
    a = np.asarray(after, dtype=object)
    if a.ndim == 1:
        if a.shape[0] != 2:
            raise ValueError("after must be (distance, id) or one such pair per query")
        a = np.broadcast_to(a, (nq, 2))
    if a.shape != (nq, 2):
        raise ValueError("after must be (distance, id) or one such pair per query")
    ad = np.ascontiguousarray([float(x) for x in a[:, 0]], dtype=np.float64)
    ai = np.ascontiguousarray([int(x) for x in a[:, 1]], dtype=np.int64)
    return ad, ai


def mask_forms(index, row_mask):
    """The two forms of a WHERE row set for the sharded entries: (kept alive by the caller, row_mask pointer, tsh_mask*).
    A HipMask goes to the *_masked entries (its handle; ValueError once it is closed), anything else is a GLOBAL keep
    bitmap for the pointer entries (HipVectorIndex.mask_arg)."""
    from .backend import HipMask

    if isinstance(row_mask, HipMask):
        return row_mask, None, row_mask.handle()
    keep, mp = index.mask_arg(row_mask)
    return keep, mp, None


def group_forms(index, groups, after=None):
    """A grouped call's two inputs: (tsh_groups* of the caller's HipGroups, its GLOBAL group_of array for a host merge);
    (None, None) without groups.  The handle must have been made on this rank's shard (HipVectorIndex.make_groups, from
    the same GLOBAL array on every rank); the plain grouped search takes no cursor."""
    if groups is None:
        return None, None
    if after is not None:
        raise ValueError("a grouped sharded search takes no cursor")
    return groups.handle(), groups.group_of


def _cursor_ptrs(cur):
    """(after_dist, after_id) pointers of cursor_arrays' pair; (None, None) without a cursor"""
    if cur is None:
        return None, None
    return cur[0].ctypes.data_as(_ffi.p_f64), cur[1].ctypes.data_as(_ffi.p_i64)


def merge_candidate_blocks(metric: int, dim: int, queries: np.ndarray, k: int,
                           distance_threshold: Optional[float], blocks: np.ndarray, n_blocks: int,
                           entries: int, after=None, group_of=None):
    """Host merge of `n_blocks` x nq candidate blocks (uint8 array, layout [block][query]).

    `group_of`: the GLOBAL group array of a grouped search's blocks (tsh_merge_candidates_grouped: the nearest row of
    each of the k nearest groups over all blocks); the answer is then (ids, dist, count, groups[nq,k]).  Not with `after`.

    `after`: a cursor -- one (distance, id), or one per query -- behind which the answer starts
    (tsh_merge_candidates_after); None = from the start (tsh_merge_candidates).

    Returns (ids[nq,k], dist[nq,k], count[nq]); raises _ffi.TshError(TSH_E_OVERFLOW) with
    `.needed_entries` set when a block was truncated."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    if q.ndim == 1:
        q = q[None, :]
    nq = q.shape[0]
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
    bb = _ffi.lib().tsh_candidate_block_bytes(entries)
    if blocks.size != n_blocks * nq * bb:
        raise ValueError("blocks buffer has the wrong size")
    kk = max(int(k), 0)
    ids = np.full((nq, max(kk, 1)), -1, dtype=np.int64)
    dist = np.full((nq, max(kk, 1)), np.nan, dtype=np.float64)
    cnt = np.zeros(nq, dtype=np.int32)
    need = ctypes.c_int32(entries)
    thr = math.nan if distance_threshold is None else float(distance_threshold)
    if group_of is not None:
        if after is not None:
            raise ValueError("a grouped merge takes no cursor")
        g = np.ascontiguousarray(group_of, dtype=np.int32).reshape(-1)
        grp = np.full((nq, max(kk, 1)), -1, dtype=np.int32)
        rc = _ffi.lib().tsh_merge_candidates_grouped(metric, dim, q.ctypes.data_as(_ffi.p_f32), nq, int(k), thr,
                                                     g.ctypes.data_as(_ffi.p_i32), g.shape[0],
                                                     blocks.ctypes.data_as(ctypes.c_void_p), n_blocks, entries,
                                                     ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64),
                                                     grp.ctypes.data_as(_ffi.p_i32), cnt.ctypes.data_as(_ffi.p_i32),
                                                     ctypes.byref(need))
    elif after is None:
        rc = _ffi.lib().tsh_merge_candidates(metric, dim, q.ctypes.data_as(_ffi.p_f32), nq, int(k), thr,
                                             blocks.ctypes.data_as(ctypes.c_void_p), n_blocks, entries,
                                             ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64),
                                             cnt.ctypes.data_as(_ffi.p_i32), ctypes.byref(need))
    else:
        ad, ai = cursor_arrays(after, nq)
        rc = _ffi.lib().tsh_merge_candidates_after(metric, dim, q.ctypes.data_as(_ffi.p_f32), nq, int(k), thr,
                                                   ad.ctypes.data_as(_ffi.p_f64), ai.ctypes.data_as(_ffi.p_i64),
                                                   blocks.ctypes.data_as(ctypes.c_void_p), n_blocks, entries,
                                                   ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64),
                                                   cnt.ctypes.data_as(_ffi.p_i32), ctypes.byref(need))
    if rc != _ffi.TSH_OK:
        err = _ffi.TshError(rc, _ffi.last_error())
        err.needed_entries = need.value
        raise err
    if group_of is not None:
        return ids[:, :kk], dist[:, :kk], cnt, grp[:, :kk]
    return ids[:, :kk], dist[:, :kk], cnt


class ShardedSearcher:
    """All-gather + merge around one local shard.  `group=None` = default process group."""

    def __init__(self, shard_index, group=None):
        import torch
        import torch.distributed as dist

        self._torch, self._dist = torch, dist
        self.index = shard_index
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self._bufs = {}

    def _buffers(self, nq: int, entries: int, slot: int = 0):
        """(mine, all, host) byte buffers for nq blocks per rank: views of per-(entries, slot) buffers that only
        grow, so a short last group does not allocate (pinned allocations cost about a millisecond)."""
        t = self._torch
        bb = _ffi.lib().tsh_candidate_block_bytes(entries)
        key = (entries, slot)
        cur = self._bufs.get(key)
        if cur is None or cur[0] < nq:
            cap = max(nq, 64, 0 if cur is None else cur[0])
            if len(self._bufs) > 8:
                self._bufs.clear()
            cur = (cap, t.empty(cap * bb, dtype=t.uint8, device="cuda"),
                   t.empty(self.world * cap * bb, dtype=t.uint8, device="cuda"),
                   t.empty(self.world * cap * bb, dtype=t.uint8, pin_memory=True))
            self._bufs[key] = cur
        _, mine, allb, host = cur
        return mine[: nq * bb], allb[: self.world * nq * bb], host[: self.world * nq * bb]

    def _scan(self, q: np.ndarray, k: int, mp, entries: int, slot: int, cur=None, mh=None, gh=None):
        """This rank's shard: candidate blocks for the queries of one group, left in device memory.
        cur: the queries' cursor arrays (cursor_arrays), or None.  mh: a mask handle in place of the pointer mp
        (tsh_search_shard_masked, with or without the cursor).  gh: a groups handle (tsh_search_shard_grouped, behind
        either mask form)."""
        mine, _, _ = self._buffers(q.shape[0], entries, slot)
        if gh is not None:
            _ffi.check(_ffi.lib().tsh_search_shard_grouped(self.index._h, q.ctypes.data_as(_ffi.p_f32), q.shape[0], int(k),
                                                           mp, mh, gh, entries, ctypes.c_void_p(mine.data_ptr()), None))
        elif mh is not None:
            ad, ai = _cursor_ptrs(cur)
            _ffi.check(_ffi.lib().tsh_search_shard_masked(self.index._h, q.ctypes.data_as(_ffi.p_f32), q.shape[0], int(k),
                                                          mh, ad, ai, entries, ctypes.c_void_p(mine.data_ptr()), None))
        elif cur is None:
            _ffi.check(_ffi.lib().tsh_search_shard(self.index._h, q.ctypes.data_as(_ffi.p_f32), q.shape[0], int(k), mp,
                                                   entries, ctypes.c_void_p(mine.data_ptr()), None))
        else:
            _ffi.check(_ffi.lib().tsh_search_shard_after(self.index._h, q.ctypes.data_as(_ffi.p_f32), q.shape[0], int(k),
                                                         mp, cur[0].ctypes.data_as(_ffi.p_f64),
                                                         cur[1].ctypes.data_as(_ffi.p_i64), entries,
                                                         ctypes.c_void_p(mine.data_ptr()), None))

    def _exchange_merge(self, q: np.ndarray, k: int, thr, entries: int, slot: int, mine=None, after=None, group_of=None):
        t = self._torch
        own, allb, host = self._buffers(q.shape[0], entries, slot)
        mine = own if mine is None else mine
        if self._dist.is_initialized() and self._dist.get_backend(self.group) == "gloo":
            # test setups (several ranks on one GPU): exchange through host memory
            mine_h = mine.cpu()
            self._dist.all_gather_into_tensor(host, mine_h, group=self.group)
            return merge_candidate_blocks(self.index.metric, self.index.dim, q, k, thr, host.numpy(),
                                          self.world, entries, after, group_of)
        if self._dist.is_initialized():
            self._dist.all_gather_into_tensor(allb, mine, group=self.group)
        else:
            allb = mine
        host[: allb.numel()].copy_(allb, non_blocking=True)
        t.cuda.current_stream().synchronize()
        return merge_candidate_blocks(self.index.metric, self.index.dim, q, k, thr, host[: allb.numel()].numpy(),
                                      self.world, entries, after, group_of)

    def search_many(self, queries, k: int, distance_threshold: Optional[float] = None, row_mask=None,
                    group: int = 8, after=None, groups=None):
        """A stream of independent queries, exchanged in groups: this rank's scans of ALL the queries run as one
        pipeline on a library thread (tsh_search_shard_begin: the GPU sees no group boundaries), and the calling
        thread all-gathers and merges every group as soon as its blocks are final (collectives stay on one thread,
        in one order on every rank).  Same results as search().  `after`, `row_mask`: as in search() (a HipMask:
        tsh_search_shard_begin_masked; it must stay open until this returns).  `groups`: as in search()
        (tsh_search_shard_begin_grouped): the answer is (ids, dist, count, groups)."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq, kk = q.shape[0], max(int(k), 0)
        ids = np.full((nq, kk), -1, dtype=np.int64)
        dist = np.full((nq, kk), np.nan, dtype=np.float64)
        cnt = np.zeros(nq, dtype=np.int32)
        grp = np.full((nq, kk), -1, dtype=np.int32)
        gh, group_of = group_forms(self.index, groups, after)
        L = _ffi.lib()
        entries = L.tsh_default_block_entries(int(k))
        row_mask, mp, mh = mask_forms(self.index, row_mask)  # GLOBAL mask: one bit per row id below this shard's end
        group = max(1, int(group))
        spans = [(s, min(nq, s + group)) for s in range(0, nq, group)]
        if not spans:
            return (ids, dist, cnt) if gh is None else (ids, dist, cnt, grp)
        bb = L.tsh_candidate_block_bytes(entries)
        key = ("many", entries)
        cur = self._bufs.get(key)
        if cur is None or cur[0] < nq:
            cur = (max(nq, 64), self._torch.empty(max(nq, 64) * bb, dtype=self._torch.uint8, device="cuda"))
            self._bufs[key] = cur
            self._torch.cuda.current_stream().synchronize()
        mine_all = cur[1]
        st = ctypes.c_void_p()
        cursors = None if after is None else cursor_arrays(after, nq)
        if gh is not None:
            _ffi.check(L.tsh_search_shard_begin_grouped(self.index._h, q.ctypes.data_as(_ffi.p_f32), nq, int(k), mp, mh, gh,
                                                        entries, ctypes.c_void_p(mine_all.data_ptr()), group, ctypes.byref(st)))
        elif mh is not None:
            ad, ai = _cursor_ptrs(cursors)
            _ffi.check(L.tsh_search_shard_begin_masked(self.index._h, q.ctypes.data_as(_ffi.p_f32), nq, int(k), mh, ad, ai,
                                                       entries, ctypes.c_void_p(mine_all.data_ptr()), group, ctypes.byref(st)))
        elif cursors is None:
            _ffi.check(L.tsh_search_shard_begin(self.index._h, q.ctypes.data_as(_ffi.p_f32), nq, int(k), mp, entries,
                                                ctypes.c_void_p(mine_all.data_ptr()), group, ctypes.byref(st)))
        else:
            _ffi.check(L.tsh_search_shard_begin_after(self.index._h, q.ctypes.data_as(_ffi.p_f32), nq, int(k), mp,
                                                      cursors[0].ctypes.data_as(_ffi.p_f64),
                                                      cursors[1].ctypes.data_as(_ffi.p_i64), entries,
                                                      ctypes.c_void_p(mine_all.data_ptr()), group, ctypes.byref(st)))
        try:
            for g, (lo, hi) in enumerate(spans):
                _ffi.check(L.tsh_search_shard_progress(st, hi, None))  # this group's blocks are final
                try:
                    part = None if cursors is None else (cursors[0][lo:hi], cursors[1][lo:hi])
                    got = self._exchange_merge(q[lo:hi], k, distance_threshold, entries, g % 2,
                                               mine_all[lo * bb: hi * bb], part, group_of)
                except _ffi.TshError as e:
                    if e.code != _ffi.TSH_E_OVERFLOW:
                        raise
                    _ffi.check(L.tsh_search_shard_progress(st, nq, None))  # nothing overlaps a retry
                    got = self.search(q[lo:hi], k, distance_threshold, row_mask, part, groups)  # ties: bigger blocks
                ids[lo:hi], dist[lo:hi], cnt[lo:hi] = got[:3]
                if gh is not None:
                    grp[lo:hi] = got[3]
        finally:
            rc = L.tsh_search_shard_end(st)
        _ffi.check(rc)
        return (ids, dist, cnt) if gh is None else (ids, dist, cnt, grp)

    def search(self, queries, k: int, distance_threshold: Optional[float] = None, row_mask=None, after=None, groups=None):
        """`after`: a GLOBAL cursor -- one (distance, id), or one per query; the same on every rank -- behind which
        the answer starts: the next k rows past it (tsh_search_shard_after + tsh_merge_candidates_after).  A page
        shorter than k is the last one.  `row_mask`: a GLOBAL keep bitmap, or a HipMask made for this rank's shard
        from it (tsh_search_shard_masked, on the first scan and on an overflow retry alike).  `groups`: a HipGroups made
        on this rank's shard from the GLOBAL group array, the same on every rank -- the nearest row of each of the k
        nearest groups over all ranks' rows (tsh_search_shard_grouped + tsh_merge_candidates_grouped; no cursor): the
        answer is (ids, dist, count, groups)."""
        t = self._torch
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        L = _ffi.lib()
        entries = L.tsh_default_block_entries(int(k))
        row_mask, mp, mh = mask_forms(self.index, row_mask)  # GLOBAL mask: one bit per row id below this shard's end
        cur = None if after is None else cursor_arrays(after, nq)
        gh, group_of = group_forms(self.index, groups, after)
        for _attempt in range(3):
            self._scan(q, k, mp, entries, 0, cur, mh, gh)
            try:
                return self._exchange_merge(q, k, distance_threshold, entries, 0, None, after, group_of)
            except _ffi.TshError as e:
                if e.code != _ffi.TSH_E_OVERFLOW:
                    raise
                entries = int(e.needed_entries)  # identical on every rank: all saw the same headers
        raise RuntimeError("candidate blocks kept overflowing")


class CommSearcher:
    """The same exchange through the library's OWN entry points (include/tostore_hip.h: tsh_comm_*,
    tsh_search_sharded) -- what a host without torch (one Dart process per GPU) calls.  The library pipelines the
    call itself (groups of queries: a helper thread scans group g + 1 while group g is all-gathered and merged, each
    rank merging its slice of the group's queries).

    RCCL transport: rank 0 makes the 128-byte id with `CommSearcher.unique_id()`, the host ships it to the other
    ranks over whatever channel it has, every rank constructs its searcher (collective) and then calls `search`
    with the same queries (collective).
    Host transport (`allgather=`): a callable `(send: np.ndarray[uint8], recv: np.ndarray[uint8]) -> None` that
    places every rank's bytes at recv[rank * len(send):]; `CommSearcher.over_torch(...)` builds one from a
    torch.distributed group (gloo: several ranks may share one GPU)."""

    python_groups = False  # search_many: the library forms the groups itself

    def __init__(self, shard_index, world: int, rank: int, unique_id: Optional[bytes] = None, device: int = -1,
                 allgather=None):
        self.index = shard_index
        self.world = world
        self.rank = rank
        self._c = ctypes.c_void_p()
        self._cb = None
        self.callback_error = None
        if allgather is not None:
            def _cb(_user, send, recv, nbytes):
                try:
                    src = np.ctypeslib.as_array(ctypes.cast(send, _ffi.p_u8), shape=(nbytes,))
                    dst = np.ctypeslib.as_array(ctypes.cast(recv, _ffi.p_u8), shape=(nbytes * world,))
                    allgather(src, dst)
                    return 0
                except Exception as e:  # noqa: BLE001 -- must not unwind through the C frames
                    self.callback_error = e
                    return -1
            self._cb = _ffi.ALLGATHER_FN(_cb)  # kept alive as long as the communicator
            _ffi.check(_ffi.lib().tsh_comm_create_host(world, rank, device, ctypes.cast(self._cb, ctypes.c_void_p),
                                                       None, ctypes.byref(self._c)))
            return
        if unique_id is None or len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of tsh_comm_unique_id")
        buf = ctypes.create_string_buffer(unique_id, 128)
        _ffi.check(_ffi.lib().tsh_comm_create(buf, world, rank, device, ctypes.byref(self._c)))

    @classmethod
    def over_torch(cls, shard_index, group=None, device: int = -1):
        """Host transport over a torch.distributed process group (CPU tensors: gloo)."""
        import torch
        import torch.distributed as dist

        world, rank = dist.get_world_size(group), dist.get_rank(group)

        def allgather(send, recv):
            dist.all_gather_into_tensor(torch.from_numpy(recv), torch.from_numpy(send), group=group)

        return cls(shard_index, world, rank, None, device, allgather=allgather)

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        _ffi.check(_ffi.lib().tsh_comm_unique_id(buf))
        return buf.raw

    def set_group(self, queries_per_exchange: int) -> None:
        """Queries per exchange (0 = by the size of the call).  Same value on every rank."""
        _ffi.check(_ffi.lib().tsh_comm_set_group(self._c, int(queries_per_exchange)))

    def timeline(self, reset: bool = False) -> dict:
        """Where this rank's tsh_search_sharded time went (tsh_comm_timeline, include/tostore_hip.h): sums of
        microseconds per phase since the communicator was made or last reset."""
        t = _ffi.TshCommTimeline()
        _ffi.check(_ffi.lib().tsh_comm_get_timeline(self._c, ctypes.byref(t), 1 if reset else 0))
        d = {k: getattr(t, k) for k, _ in t._fields_ if k != "reserved"}
        d["transport"] = {0: "rccl", 1: "host callback", 2: "TSH_RCCL_LIB"}.get(d["transport"], d["transport"])
        return d

    def close(self) -> None:
        if self._c:
            _ffi.lib().tsh_comm_destroy(self._c)
            self._c = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def search(self, queries, k: int, distance_threshold: Optional[float] = None, row_mask=None, shard=..., after=None,
               groups=None, groups_handle=...):
        """Collective.  `shard=None` (tests) passes a NULL handle: this rank fails locally and stays in the
        collective.  `after`: a GLOBAL cursor -- one (distance, id), or one per query; the same on every rank --
        behind which the answer starts (tsh_search_sharded_after).  `row_mask`: a GLOBAL keep bitmap, or a HipMask made
        for this rank's shard from it (tsh_search_sharded_masked, with or without `after`).  `groups`: a HipGroups made on
        this rank's shard from the GLOBAL group array, the same on every rank (tsh_search_sharded_grouped; no cursor): the
        answer is (ids, dist, count, groups).  `groups_handle` (tests) passes that pointer in the handle's place: a bad
        one is this rank's own failure inside the collective."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq, kk = q.shape[0], max(int(k), 0)
        ids = np.empty((nq, max(kk, 1)), dtype=np.int64)
        dist = np.empty((nq, max(kk, 1)), dtype=np.float64)
        cnt = np.zeros(nq, dtype=np.int32)
        thr = math.nan if distance_threshold is None else float(distance_threshold)
        row_mask, mp, mh = mask_forms(self.index, row_mask)
        h = self.index._h if shard is ... else shard
        if groups is not None or groups_handle is not ...:
            if after is not None:
                raise ValueError("a grouped sharded search takes no cursor")
            gh = groups.handle() if groups_handle is ... else groups_handle
            grp = np.full((nq, max(kk, 1)), -1, dtype=np.int32)
            _ffi.check(_ffi.lib().tsh_search_sharded_grouped(h, self._c, q.ctypes.data_as(_ffi.p_f32), nq, int(k), thr, mp, mh,
                                                             gh, ids.ctypes.data_as(_ffi.p_i64),
                                                             dist.ctypes.data_as(_ffi.p_f64), grp.ctypes.data_as(_ffi.p_i32),
                                                             cnt.ctypes.data_as(_ffi.p_i32)))
            return ids[:, :kk], dist[:, :kk], cnt, grp[:, :kk]
        if mh is not None:
            ad, ai = _cursor_ptrs(None if after is None else cursor_arrays(after, nq))
            _ffi.check(_ffi.lib().tsh_search_sharded_masked(h, self._c, q.ctypes.data_as(_ffi.p_f32), nq, int(k), thr, mh,
                                                            ad, ai, ids.ctypes.data_as(_ffi.p_i64),
                                                            dist.ctypes.data_as(_ffi.p_f64), cnt.ctypes.data_as(_ffi.p_i32)))
        elif after is None:
            _ffi.check(_ffi.lib().tsh_search_sharded(h, self._c, q.ctypes.data_as(_ffi.p_f32), nq, int(k), thr, mp,
                                                     ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64),
                                                     cnt.ctypes.data_as(_ffi.p_i32)))
        else:
            ad, ai = cursor_arrays(after, nq)
            _ffi.check(_ffi.lib().tsh_search_sharded_after(h, self._c, q.ctypes.data_as(_ffi.p_f32), nq, int(k), thr, mp,
                                                           ad.ctypes.data_as(_ffi.p_f64), ai.ctypes.data_as(_ffi.p_i64),
                                                           ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64),
                                                           cnt.ctypes.data_as(_ffi.p_i32)))
        return ids[:, :kk], dist[:, :kk], cnt

    def search_many(self, queries, k: int, distance_threshold: Optional[float] = None, row_mask=None, group: int = 0,
                    after=None, groups=None):
        """One collective call; the library forms the groups itself (same signature as
        ShardedSearcher.search_many; `group` > 0 overrides the library's choice)."""
        if group:
            self.set_group(group)
        try:
            return self.search(queries, k, distance_threshold, row_mask, after=after, groups=groups)
        finally:
            if group:
                self.set_group(0)
