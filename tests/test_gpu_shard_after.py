"""GPU: cursor search across shards (tsh_search_shard_after / tsh_search_shard_begin_after + tsh_merge_candidates_after,
include/tostore_hip.h).  Shard handles of one corpus share the test box's GPU; a page is one tsh_search_shard_after per
shard into a device buffer, then the host merge behind the same cursor.  The specification is tsh_search_after's: pages
concatenate to exactly oracle.search_exhaustive(k = n) over the WHOLE corpus -- ids equal, distances bit for bit."""
import ctypes
import math
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2
K = 7
START = (-math.inf, 0)
BOUNDS = [(0, 1000), (1000, 2531), (2531, 4099)]  # unaligned bases
GUARD = 4096  # bytes behind every shard's blocks, filled with a pattern


def _same_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def _query(rng, oracle_mod, d, metric):
    q = rng.standard_normal(d).astype(np.float32)
    return oracle_mod.normalize_f32(q) if metric == COS else q


def _cursors(after, nq):
    ad = np.ascontiguousarray(np.broadcast_to(np.asarray(after[0], dtype=np.float64).reshape(-1), (nq,)))
    ai = np.ascontiguousarray(np.broadcast_to(np.asarray(after[1], dtype=np.int64).reshape(-1), (nq,)))
    return ad, ai


class Shards:
    """Shard handles (row_base) over one corpus on device 0, and the device buffer their blocks land in:
    [shard][query] blocks, each shard's followed by a guard region."""

    def __init__(self, rows, bounds, metric):
        from tostore_amd import HipVectorIndex

        self.metric, self.d, self.bounds = metric, rows.shape[1], bounds
        self.idx = []
        for lo, hi in bounds:
            s = HipVectorIndex(self.d, metric, shard_device=0, row_base=lo)
            self.idx.append(s)
            s.append(lo, rows[lo:hi])  # shard handles take GLOBAL ids
        self._bufs = {}

    def close(self):
        for s in self.idx:
            s.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_deleted(self, ids):
        ids = np.asarray(ids, np.int64)
        for s, (lo, hi) in zip(self.idx, self.bounds):
            mine = ids[(ids >= lo) & (ids < hi)]
            if len(mine):
                s.set_deleted(mine)

    def stats(self):
        out = {}
        for s in self.idx:
            for k, v in s.search_after_stats().items():
                out[k] = out.get(k, 0) + v
        return out

    def counters(self, name):
        return sum(s.counters()[name] for s in self.idx)

    def _buffer(self, nq, entries):
        import torch

        from tostore_amd import _ffi

        bb = _ffi.lib().tsh_candidate_block_bytes(entries)
        key = (nq, entries)
        if key not in self._bufs:
            if len(self._bufs) > 4:
                self._bufs.clear()
            self._bufs[key] = torch.empty(len(self.idx) * (nq * bb + GUARD), dtype=torch.uint8, device="cuda")
        buf = self._bufs[key]
        buf.fill_(0xA5)
        torch.cuda.synchronize()
        return buf, bb

    def blocks(self, qs, k, after, mask=None, entries=None):
        """One tsh_search_shard_after per shard -> the host copy of the whole buffer (guards included), block bytes."""
        from tostore_amd import _ffi

        L = _ffi.lib()
        q = np.ascontiguousarray(qs, dtype=np.float32).reshape(-1, self.d)
        nq = q.shape[0]
        entries = L.tsh_default_block_entries(k) if entries is None else entries
        buf, bb = self._buffer(nq, entries)
        ad, ai = _cursors(after, nq)
        mp = None if mask is None else mask.ctypes.data_as(_ffi.p_u8)
        for g, s in enumerate(self.idx):
            at = buf.data_ptr() + g * (nq * bb + GUARD)
            _ffi.check(L.tsh_search_shard_after(s._h, q.ctypes.data_as(_ffi.p_f32), nq, k, mp, ad.ctypes.data_as(_ffi.p_f64),
                                                ai.ctypes.data_as(_ffi.p_i64), entries, ctypes.c_void_p(at), None))
        host = buf.cpu().numpy().reshape(len(self.idx), nq * bb + GUARD)
        assert np.all(host[:, nq * bb:] == 0xA5), "a shard search wrote past its blocks"
        return host, bb, entries

    def page(self, qs, k, after, thr=None, mask=None, entries=None):
        """A page: every shard's blocks, then the merge behind the same cursor; a truncated block is answered as every
        sharded caller answers it -- all shards again with the entry count the merge asks for."""
        from tostore_amd import _ffi
        from tostore_amd.sharded import merge_candidate_blocks

        q = np.ascontiguousarray(qs, dtype=np.float32).reshape(-1, self.d)
        nq = q.shape[0]
        for _attempt in range(3):
            host, bb, entries = self.blocks(q, k, after, mask, entries)
            try:
                return merge_candidate_blocks(self.metric, self.d, q, k, thr, np.ascontiguousarray(host[:, :nq * bb]), len(self.idx),
                                              entries, after=_cursors(after, nq))
            except _ffi.TshError as e:
                if e.code != _ffi.TSH_E_OVERFLOW:
                    raise
                assert e.needed_entries > entries
                entries = int(e.needed_entries)
        raise AssertionError("candidate blocks kept overflowing")


def _walk(sh, q, k=K, thr=None, mask=None, limit=5000):
    ids_all, dist_all, cur, pages = [], [], START, 0
    while True:
        ids, dist, cnt = sh.page(q, k, cur, thr, mask)
        c = int(cnt[0])
        assert 0 <= c <= k
        pages += 1
        assert pages <= limit, "the walk does not end"
        ids_all.append(ids[0, :c].copy())
        dist_all.append(dist[0, :c].copy())
        if c:
            cur = (float(dist[0, c - 1]), int(ids[0, c - 1]))
        if c < k:
            break
    if c:  # the one after the short page
        assert int(sh.page(q, k, cur, thr, mask)[2][0]) == 0
    return np.concatenate(ids_all), np.concatenate(dist_all), pages


def _check_walk(sh, oracle_mod, rows, q, thr=None, mask=None, keep=None, k=K):
    """keep: what the oracle is told lives (the mask and the tombstones together), as packed bits"""
    with np.errstate(all="ignore"):
        eids, edist = oracle_mod.search_exhaustive(rows, q, sh.metric, len(rows), thr, keep)
    ids, dist, pages = _walk(sh, q, k, thr, mask)
    assert np.array_equal(ids, eids), (len(ids), len(eids))
    assert _same_dist(dist, edist)
    assert pages == len(eids) // k + 1
    return eids, edist


def _decode(block, bb):
    """(count, entries, [(id, s0, s1)] of the entries written) of one block"""
    count, entries = struct.unpack_from("<II", block, 0)
    n = min(count, entries)
    return count, entries, [struct.unpack_from("<qdd", block, 64 + 24 * i) for i in range(n)]


@pytest.mark.parametrize("metric", [L2, IP, COS])
@pytest.mark.parametrize("d", [4, 128, 257])
def test_page_walk_equals_the_full_list(hip_lib, oracle_mod, metric, d):
    """Three shards at unaligned bases: dense, behind a keep-50 % mask, behind a selective mask (fewer than 1 row in 24),
    with a threshold, and after tombstoning one whole tile and every shard's last row."""
    rng = np.random.default_rng(1000 * d + metric)
    n = BOUNDS[-1][1]
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    with Shards(rows, BOUNDS, metric) as sh:
        eids, edist = _check_walk(sh, oracle_mod, rows, q)
        half = np.packbits(rng.random(n) < 0.5, bitorder="little")
        _check_walk(sh, oracle_mod, rows, q, mask=half, keep=half)
        few = np.packbits(rng.random(n) < 0.03, bitorder="little")
        _check_walk(sh, oracle_mod, rows, q, mask=few, keep=few)
        _check_walk(sh, oracle_mod, rows, q, thr=float(edist[n // 3]))
        dead = sorted(set(range(64, 128)) | {hi - 1 for _, hi in BOUNDS})
        sh.set_deleted(dead)
        alive = np.ones(n, bool)
        alive[dead] = False
        _check_walk(sh, oracle_mod, rows, q, keep=np.packbits(alive, bitorder="little"))
        both = np.packbits(alive & np.unpackbits(half, bitorder="little")[:n].astype(bool), bitorder="little")
        _check_walk(sh, oracle_mod, rows, q, mask=half, keep=both)


def test_page_walk_768(hip_lib, oracle_mod):
    rng = np.random.default_rng(768)
    n, d = 5000, 768
    rows = rng.standard_normal((n, d)).astype(np.float32)
    with Shards(rows, [(0, 1000), (1000, 2531), (2531, n)], L2) as sh:
        _check_walk(sh, oracle_mod, rows, _query(rng, oracle_mod, d, L2))


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_shards_at_tile_edges(hip_lib, oracle_mod, metric):
    """Shards of 1, 63, 64 and 65 rows, and a larger one behind them."""
    rng = np.random.default_rng(64 + metric)
    bounds = [(0, 1), (1, 64), (64, 128), (128, 193), (193, 700)]
    d = 24
    rows = rng.standard_normal((700, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    with Shards(rows, bounds, metric) as sh:
        _check_walk(sh, oracle_mod, rows, q)
        half = np.packbits(rng.random(700) < 0.5, bitorder="little")
        _check_walk(sh, oracle_mod, rows, q, mask=half, keep=half)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_selective_mask_takes_the_list_scan(hip_lib, oracle_mod, metric):
    """Shards large enough for the list scan (4096 rows and more, rows of a width it serves) behind a 2 % mask: every
    cursor search of theirs is a list scan, none takes the exact path, and the walk is exact."""
    rng = np.random.default_rng(5 + metric)
    n, d = 12_000, 100
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    bits = np.packbits(rng.random(n) < 0.02, bitorder="little")
    with Shards(rows, [(0, 5001), (5001, n)], metric) as sh:
        c0 = {k: sh.counters(k) for k in ("scan_launches", "list_scans", "exact_scans")}
        _check_walk(sh, oracle_mod, rows, q, mask=bits, keep=bits)
        c1 = {k: sh.counters(k) for k in c0}
        scans = c1["scan_launches"] - c0["scan_launches"]
        assert scans > 0 and c1["list_scans"] - c0["list_scans"] == scans and c1["exact_scans"] == c0["exact_scans"]


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_ties_across_shards(hip_lib, oracle_mod, metric):
    rng = np.random.default_rng(17 + metric)
    n, d = BOUNDS[-1][1], 40
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[1500:1600] = rows[100]  # row 100 lives in shard 0, its hundred twins in shard 1
    rows[2531] = rows[100]       # ... and one more at shard 2's first row
    q = _query(rng, oracle_mod, d, metric)
    with Shards(rows, BOUNDS, metric) as sh:
        eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n)
        first = int(np.flatnonzero(eids == 100)[0])
        crowd = [100] + list(range(1500, 1600)) + [2531]
        assert np.array_equal(eids[first:first + 102], crowd)
        # the cursor in the middle of the crowd: the page continues by id; from row 100 it crosses into shard 1; near the
        # crowd's end it crosses into shard 2 and on to the next distance
        for at in (first + 50, first, first + 97):
            ids, dist, cnt = sh.page(q, K, (float(edist[at]), int(eids[at])))
            assert cnt[0] == K and np.array_equal(ids[0], eids[at + 1:at + 1 + K]) and _same_dist(dist[0], edist[at + 1:at + 1 + K])
        _check_walk(sh, oracle_mod, rows, q)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_side_list_larger_than_its_capacity(hip_lib, oracle_mod, metric):
    """1500 identical rows inside one shard, the cursor on the 700th: the floor pass cannot decide any of them, the side
    list (1024 ids) overflows, the search is redone once with a larger one -- into the same device block."""
    rng = np.random.default_rng(3 + metric)
    d = 8
    v = rng.standard_normal(d).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    others = rng.standard_normal((2600, d)).astype(np.float32)
    rows = np.concatenate([others[:1100], np.tile(v, (1500, 1)), others[1100:]])  # the crowd: rows 1100 .. 2599, in shard 1
    bounds = [(0, 1000), (1000, 2700), (2700, len(rows))]
    eids, edist = oracle_mod.search_exhaustive(rows, q, metric, len(rows))
    first = int(np.flatnonzero(eids == 1100)[0])
    assert np.array_equal(eids[first:first + 1500], np.arange(1100, 2600))
    at = first + 699
    cur = (float(edist[at]), int(eids[at]))
    with Shards(rows, bounds, metric) as sh:
        s0 = [s.search_after_stats() for s in sh.idx]
        host, bb, entries = sh.blocks(q, 20, cur, entries=2048)  # (room for the whole crowd: this call is not retried)
        s1 = [s.search_after_stats() for s in sh.idx]
        assert [b["redone"] - a["redone"] for a, b in zip(s0, s1)] == [0, 1, 0]
        assert [b["searches"] - a["searches"] for a, b in zip(s0, s1)] == [1, 1, 1]
        assert s1[1]["side_rows"] - s0[1]["side_rows"] >= 1500
        # the redone job's block: every row of the crowd once (their exact sums: the oracle's), and the rows that follow it
        count, ent, got = _decode(host[1].tobytes(), bb)
        assert ent == 2048 and 1500 <= count <= 2048 and len(got) == count
        ids = sorted(e[0] for e in got)
        assert len(set(ids)) == len(ids) and set(range(1100, 2600)) <= set(ids) and all(1000 <= i < 2700 for i in ids)
        want = oracle_mod.exact_sums(q, rows[1100], metric)
        for e in got:
            if 1100 <= e[0] < 2600:
                assert struct.pack("<dd", *e[1:]) == struct.pack("<dd", *want)
        from tostore_amd.sharded import merge_candidate_blocks

        m_ids, m_dist, m_cnt = merge_candidate_blocks(metric, d, q, 20, None, np.ascontiguousarray(host[:, :bb]), 3, entries, after=cur)
        assert m_cnt[0] == 20 and np.array_equal(m_ids[0], eids[at + 1:at + 21]) and _same_dist(m_dist[0], edist[at + 1:at + 21])
        # ... and with default blocks, through the overflow retry: the whole list
        _check_walk(sh, oracle_mod, rows, q, k=100)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_append_at_the_blocks_edge(hip_lib, oracle_mod, metric):
    """300 identical rows in every shard, the cursor in the middle of them, blocks of 64 entries: every block reports more
    than it holds, nothing is written past entry 63 (the guard behind every block is intact), the merge asks for a retry,
    and the retry gives the exact page."""
    from tostore_amd import _ffi
    from tostore_amd.sharded import merge_candidate_blocks

    rng = np.random.default_rng(29 + metric)
    n, d = BOUNDS[-1][1], 16
    rows = rng.standard_normal((n, d)).astype(np.float32)
    for lo, _ in BOUNDS:
        rows[lo + 100:lo + 400] = rows[5]
    q = _query(rng, oracle_mod, d, metric)
    eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n)
    first = int(np.flatnonzero(eids == 5)[0])
    at = first + 450  # inside shard 1's part of the crowd
    assert 1100 <= eids[at] < 1400 and edist[at] == edist[first]
    cur = (float(edist[at]), int(eids[at]))
    with Shards(rows, BOUNDS, metric) as sh:
        host, bb, entries = sh.blocks(q, K, cur, entries=64)  # (asserts the guards)
        assert bb == 64 + 24 * 64
        for g in range(3):
            count, ent, got = _decode(host[g].tobytes(), bb)
            assert ent == 64 and count > 64 and len(got) == 64
            lo, hi = BOUNDS[g]
            assert all(lo <= e[0] < hi for e in got)
        with pytest.raises(_ffi.TshError) as e:
            merge_candidate_blocks(metric, d, q, K, None, np.ascontiguousarray(host[:, :bb]), 3, 64, after=cur)
        assert e.value.code == _ffi.TSH_E_OVERFLOW and e.value.needed_entries >= 300
        ids, dist, cnt = sh.page(q, K, cur, entries=int(e.value.needed_entries))
        assert cnt[0] == K and np.array_equal(ids[0], eids[at + 1:at + 1 + K]) and _same_dist(dist[0], edist[at + 1:at + 1 + K])


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_rows_outside_the_model_come_last(hip_lib, oracle_mod, metric):
    """One row with an infinite element and one with a NaN element, in different shards, are kept out of the scan: the
    walk returns each exactly once, last; a +inf or NaN cursor launches no scan and returns only what can follow it."""
    rng = np.random.default_rng(11 + metric)
    n, d = 1500, 32
    bounds = [(0, 500), (500, 1001), (1001, n)]
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    rows[100, 3] = -np.inf if q[3] > 0 else np.inf
    rows[1240, 5] = np.nan
    with np.errstate(all="ignore"):
        eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n)
    tail = int((~np.isfinite(edist)).sum())
    assert tail == (1 if metric == COS else 2) and not np.isfinite(edist[-tail:]).any() and not (edist == -np.inf).any()
    with Shards(rows, bounds, metric) as sh:
        assert [s.counters()["quarantined_rows"] for s in sh.idx] == [1, 0, 1]
        _check_walk(sh, oracle_mod, rows, q)
        half = np.packbits(rng.random(n) < 0.5, bitorder="little")
        _check_walk(sh, oracle_mod, rows, q, mask=half, keep=half)
        s0, scans0 = sh.stats(), sh.counters("scan_launches")
        ids, dist, cnt = sh.page(q, K, (float(edist[-tail]), int(eids[-tail])))  # a +inf or NaN cursor
        assert cnt[0] == tail - 1 and np.array_equal(ids[0, :cnt[0]], eids[n - tail + 1:]) and _same_dist(dist[0, :cnt[0]], edist[n - tail + 1:])
        ids, dist, cnt = sh.page(q, K, (math.inf, -1))  # +inf rows of any id follow it, NaN rows after them
        assert cnt[0] == tail and np.array_equal(ids[0, :tail], eids[-tail:]) and _same_dist(dist[0, :tail], edist[-tail:])
        ids, dist, cnt = sh.page(q, K, (math.nan, int(eids[-1])))
        assert cnt[0] == 0
        # ... behind a mask that keeps neither row: nothing follows +inf
        none = np.ones(n, bool)
        none[[100, 1240]] = False
        assert sh.page(q, K, (math.inf, -1), mask=np.packbits(none, bitorder="little"))[2][0] == 0
        s1 = sh.stats()
        assert s1["no_floor"] - s0["no_floor"] == 4 * 3 and s1["searches"] - s0["searches"] == 4 * 3
        assert sh.counters("scan_launches") == scans0  # no scan ran for them


def test_safe_mode(hip_lib, oracle_mod):
    """A shard with more than 1024 irregular rows is in safe mode: no floor pass runs there, its blocks are what
    tsh_search_shard makes (every row: the merge asks for larger blocks), and the merge filters by the cursor."""
    rng = np.random.default_rng(13)
    n, d = 2048, 8
    rows = rng.standard_normal((n + 500, d)).astype(np.float32)
    bad = rng.choice(n, 1100, replace=False)
    rows[bad[:550], 2] = np.inf
    rows[bad[550:], 6] = np.nan
    q = rng.standard_normal(d).astype(np.float32)
    with Shards(rows, [(0, n), (n, n + 500)], L2) as sh:
        assert [s.counters()["safe_mode"] for s in sh.idx] == [1, 0]
        s0 = [s.search_after_stats() for s in sh.idx]
        _check_walk(sh, oracle_mod, rows, q, k=100)
        s1 = [s.search_after_stats() for s in sh.idx]
        # (every search of the safe shard but those from -inf is counted as answered without a floor; it has no side rows)
        assert s1[0]["no_floor"] > s0[0]["no_floor"] and s1[0]["side_rows"] == s0[0]["side_rows"]


def _canonical(block, bb):
    """A block up to the order of its entries, whose places are drawn with atomic adds"""
    count, entries, got = _decode(block, bb)
    return count, entries, sorted(struct.pack("<qdd", *e) for e in got)


def test_progressive_form(hip_lib, oracle_mod):
    """tsh_search_shard_begin_after, 20 queries with a cursor each, taken through _progress in groups of 8: the blocks
    tsh_search_shard_after writes (entry for entry; their places within a block are drawn with atomic adds), whatever the
    handle's batch threshold says."""
    import torch

    from tostore_amd import HipVectorIndex, _ffi

    L = _ffi.lib()
    rng = np.random.default_rng(99)
    n, d, nq, k, base = 6000, 64, 20, K, 777
    rows = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((nq, d)).astype(np.float32)
    entries = L.tsh_default_block_entries(k)
    bb = L.tsh_candidate_block_bytes(entries)
    ad, ai = np.empty(nq), np.empty(nq, np.int64)
    for i in range(nq):
        eids, edist = oracle_mod.search_exhaustive(rows, qs[i], L2, n)
        at = 37 * i
        ad[i], ai[i] = (-math.inf, 0) if i == 0 else (edist[at], eids[at] + base)
    ad[nq - 1], ai[nq - 1] = math.inf, 0  # (one that launches no scan)
    with HipVectorIndex(d, L2, shard_device=0, row_base=base) as s:
        s.append(base, rows)
        s.set_batch_min_nq(4)  # a cursor call is never batched
        one = torch.full((nq * bb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        two = torch.full((nq * bb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c0 = s.counters()
        _ffi.check(L.tsh_search_shard_after(s._h, qs.ctypes.data_as(_ffi.p_f32), nq, k, None, ad.ctypes.data_as(_ffi.p_f64),
                                            ai.ctypes.data_as(_ffi.p_i64), entries, ctypes.c_void_p(one.data_ptr()), None))
        st = ctypes.c_void_p()
        _ffi.check(L.tsh_search_shard_begin_after(s._h, qs.ctypes.data_as(_ffi.p_f32), nq, k, None, ad.ctypes.data_as(_ffi.p_f64),
                                                  ai.ctypes.data_as(_ffi.p_i64), entries, ctypes.c_void_p(two.data_ptr()), 8,
                                                  ctypes.byref(st)))
        a = one.cpu().numpy()
        try:
            for want in (8, 16, 20):
                done = ctypes.c_int32(0)
                _ffi.check(L.tsh_search_shard_progress(st, want, ctypes.byref(done)))
                assert done.value >= want
                b = two.cpu().numpy()  # (host-synchronised: the leading blocks are final)
                for i in range(want):
                    assert _canonical(a[i * bb:(i + 1) * bb].tobytes(), bb) == _canonical(b[i * bb:(i + 1) * bb].tobytes(), bb), i
        finally:
            rc = L.tsh_search_shard_end(st)
        _ffi.check(rc)
        assert np.all(a[nq * bb:] == 0xA5) and np.all(two.cpu().numpy()[nq * bb:] == 0xA5)
        c1 = s.counters()
        assert c1["batch_launches"] == c0["batch_launches"] and c1["scan_launches"] - c0["scan_launches"] == 2 * (nq - 1)
        # ... and the blocks are the right ones
        from tostore_amd.sharded import merge_candidate_blocks

        ids, dist, cnt = merge_candidate_blocks(L2, d, qs, k, None, a[:nq * bb], 1, entries, after=(ad, ai))
        for i in range(nq - 1):
            eids, edist = oracle_mod.search_exhaustive(rows, qs[i], L2, n)
            lo = 0 if i == 0 else 37 * i + 1
            assert cnt[i] == k and np.array_equal(ids[i], eids[lo:lo + k] + base) and _same_dist(dist[i], edist[lo:lo + k])
        assert cnt[nq - 1] == 0


def test_the_floor_runs_on_the_device(hip_lib, oracle_mod):
    """5000 x 128 Gaussian rows, L2, three shards: about one undecided row -- the cursor's own -- per page in the shard
    that holds it (tests/test_gpu_search_after.py derives the figure); the cap of 8 per search only keeps "everything is
    ambiguous" from passing.  No search falls back to the wide-band pass."""
    rng = np.random.default_rng(23)
    n, d = 5000, 128
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    with Shards(rows, [(0, 1000), (1000, 2531), (2531, n)], L2) as sh:
        s0, f0 = sh.stats(), sh.counters("fallback_searches")
        _check_walk(sh, oracle_mod, rows, q)
        s1 = sh.stats()
        searches, side = s1["searches"] - s0["searches"], s1["side_rows"] - s0["side_rows"]
        print(f"side rows per cursor search {side / searches:.3f} over {searches} shard searches")
        assert searches == 3 * (n // K + 2) and s1["redone"] == s0["redone"] and s1["no_floor"] == s0["no_floor"]
        assert side / searches <= 8
        assert side >= n // K - 3  # (the cursor's own row is undecided, in its shard, on every page that starts from one)
        assert sh.counters("fallback_searches") == f0
