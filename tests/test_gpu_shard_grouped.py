"""GPU: grouped search across shards (tsh_search_shard_grouped / tsh_search_shard_begin_grouped +
tsh_merge_candidates_grouped, include/tostore_hip.h).  Shard handles of one corpus share the test box's GPU; a search is
one tsh_search_shard_grouped per shard into a device buffer with guard bytes behind it, then the host merge over the
union of the blocks.  The specification is tsh_search_grouped's on one un-sharded index over the same rows and the same
GLOBAL group array: oracle.search_exhaustive(k = n) with repeated groups dropped -- ids equal, distances bit for bit."""
import ctypes
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2
K = 7
BOUNDS = [(0, 1000), (1000, 2531), (2531, 4099)]  # unaligned bases
GUARD = 4096  # bytes behind every shard's blocks, filled with a pattern
LAYOUTS = ("runs7", "random", "one", "ungrouped", "own", "mix")


def _query(rng, oracle_mod, d, metric):
    q = rng.standard_normal(d).astype(np.float32)
    return oracle_mod.normalize_f32(q) if metric == COS else q


def _layout(name, n, rng):
    """-> (group_of[n] int32, n_groups): the layouts of tests/test_gpu_search_grouped.py"""
    if name == "runs7":
        return (np.arange(n) // 7).astype(np.int32), n // 7 + 1
    if name == "random":
        m = max(n // 5, 1)
        return rng.integers(0, m, n).astype(np.int32), m
    if name == "one":
        return np.full(n, 2, np.int32), 3
    if name == "ungrouped":
        return np.full(n, -1, np.int32), 1
    if name == "own":
        return np.arange(n, dtype=np.int32), n
    m = max(n // 9, 1)
    g = rng.integers(0, m, n).astype(np.int32)
    neg = rng.random(n) < 0.3
    g[neg] = -rng.integers(1, 5, int(neg.sum())).astype(np.int32)
    return g, m


def _first_of_each_group(eids, edist, group_of, k):
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


def _n_groups_in(eids, group_of):
    return len(_first_of_each_group(eids, np.zeros(len(eids)), group_of, len(eids) + 1)[0])


def _same(got, want, what, q=0):
    """got: (ids, dist, count, groups) of the merge; want: _first_of_each_group's"""
    ids, dist, cnt, grp = got
    wi, wd, wg = want
    c = int(cnt[q])
    assert c == len(wi), (what, c, len(wi))
    assert np.array_equal(ids[q, :c], wi), (what, ids[q, :c][:12], wi[:12])
    assert np.array_equal(dist[q, :c].view(np.uint64), wd.view(np.uint64)), (what, dist[q, :c][:12], wd[:12])
    assert np.array_equal(grp[q, :c], wg), (what, grp[q, :c][:12], wg[:12])
    assert np.all(ids[q, c:] == -1) and np.all(np.isnan(dist[q, c:])) and np.all(grp[q, c:] == -1), what


def _decode(block):
    """(count, entries, [(id, s0, s1)] of the entries written) of one block"""
    count, entries = struct.unpack_from("<II", block, 0)
    n = min(count, entries)
    return count, entries, [struct.unpack_from("<qdd", block, 64 + 24 * i) for i in range(n)]


def _canonical(block):
    """A block up to the order of its entries, whose places are drawn with atomic adds"""
    count, entries, got = _decode(block)
    return count, entries, sorted(struct.pack("<qdd", *e) for e in got)


class Shards:
    """Shard handles (row_base) over one corpus on device 0, every one with its own groups handle made from the GLOBAL
    array, and the device buffer their blocks land in: [shard][query] blocks, each shard's followed by a guard region."""

    def __init__(self, rows, bounds, metric, group_of, n_groups):
        from tostore_amd import HipVectorIndex

        self.metric, self.d, self.bounds = metric, rows.shape[1], bounds
        self.group_of = np.ascontiguousarray(group_of, dtype=np.int32)
        self.idx, self.groups = [], []
        for lo, hi in bounds:
            s = HipVectorIndex(self.d, metric, shard_device=0, row_base=lo)
            self.idx.append(s)
            if hi > lo:
                s.append(lo, rows[lo:hi])  # shard handles take GLOBAL ids
        self._bufs = {}
        self.set_groups(group_of, n_groups)

    def set_groups(self, group_of, n_groups):
        """Every shard's groups handle, made anew from another GLOBAL array"""
        for g in self.groups:
            g.close()
        self.group_of = np.ascontiguousarray(group_of, dtype=np.int32)
        self.groups = [s.make_groups(self.group_of, n_groups) for s in self.idx]

    def close(self):
        for g in self.groups:
            g.close()
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
        return [s.search_grouped_stats() for s in self.idx]

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

    def blocks(self, qs, k, mask=None, handles=None, entries=None):
        """One tsh_search_shard_grouped per shard -> the host copy of the whole buffer, block bytes, entries.  mask: a
        GLOBAL bitmap by pointer; handles: one HipMask per shard in its place.  The guards are checked after every call."""
        from tostore_amd import _ffi

        L = _ffi.lib()
        q = np.ascontiguousarray(qs, dtype=np.float32).reshape(-1, self.d)
        nq = q.shape[0]
        entries = L.tsh_default_block_entries(max(k, 1)) if entries is None else entries
        buf, bb = self._buffer(nq, entries)
        mp = None if mask is None else mask.ctypes.data_as(_ffi.p_u8)
        for g, s in enumerate(self.idx):
            at = buf.data_ptr() + g * (nq * bb + GUARD)
            mh = None if handles is None else handles[g].handle()
            _ffi.check(L.tsh_search_shard_grouped(s._h, q.ctypes.data_as(_ffi.p_f32), nq, k, mp, mh, self.groups[g].handle(),
                                                  entries, ctypes.c_void_p(at), None))
        host = buf.cpu().numpy().reshape(len(self.idx), nq * bb + GUARD)
        assert np.all(host[:, nq * bb:] == 0xA5), "a shard search wrote past its blocks"
        return host, bb, entries

    def search(self, qs, k, thr=None, mask=None, handles=None, entries=None, retries=None):
        """Every shard's blocks, then the grouped merge; a truncated block is answered as every sharded caller answers it
        -- all shards again with the entry count the merge asks for.  retries: a list that gets one item per retry."""
        from tostore_amd import _ffi
        from tostore_amd.sharded import merge_candidate_blocks

        q = np.ascontiguousarray(qs, dtype=np.float32).reshape(-1, self.d)
        nq = q.shape[0]
        for _attempt in range(3):
            host, bb, entries = self.blocks(q, k, mask, handles, entries)
            try:
                return merge_candidate_blocks(self.metric, self.d, q, k, thr, np.ascontiguousarray(host[:, :nq * bb]), len(self.idx),
                                              entries, group_of=self.group_of)
            except _ffi.TshError as e:
                if e.code != _ffi.TSH_E_OVERFLOW:
                    raise
                assert e.needed_entries > entries
                if retries is not None:
                    retries.append(int(e.needed_entries))
                entries = int(e.needed_entries)
        raise AssertionError("candidate blocks kept overflowing")


def _whole(rows, metric, group_of, n_groups, q, k, thr=None, mask=None):
    """tsh_search_grouped on one un-sharded index over the same rows, as (ids, dist, count, groups)"""
    from tostore_amd import HipVectorIndex

    with HipVectorIndex(rows.shape[1], metric, capacity_rows=len(rows)) as idx:
        idx.append(0, rows)
        with idx.make_groups(group_of, n_groups) as h:
            ids, dist, grp, cnt = idx.search_grouped(q, k, h, thr, mask)
    return ids, dist, cnt, grp


@pytest.mark.parametrize("metric", [L2, IP, COS])
@pytest.mark.parametrize("d", [4, 128, 257])
def test_parity_with_the_oracle_and_the_unsharded_index(hip_lib, oracle_mod, metric, d):
    """Three shards at unaligned bases x every group layout x k in {1, 7, 100, groups + 5}: shard blocks -> grouped merge
    == oracle == tsh_search_grouped on one un-sharded index."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(9000 + 10 * d + metric)
    n = BOUNDS[-1][1]
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n)
    with HipVectorIndex(d, metric, capacity_rows=n) as whole, Shards(rows, BOUNDS, metric, np.zeros(0, np.int32), 0) as sh:
        whole.append(0, rows)
        for name in LAYOUTS:
            group_of, n_groups = _layout(name, n, rng)
            sh.set_groups(group_of, n_groups)
            with whole.make_groups(group_of, n_groups) as h:
                for k in (1, K, 100, _n_groups_in(eids, group_of) + 5):
                    got = sh.search(q, k)
                    _same(got, _first_of_each_group(eids, edist, group_of, k), (name, k))
                    w_ids, w_dist, w_grp, w_cnt = whole.search_grouped(q, k, h)
                    assert np.array_equal(got[2], w_cnt) and np.array_equal(got[0], w_ids) and np.array_equal(got[3], w_grp), (name, k)
                    assert np.array_equal(got[1].view(np.uint64), w_dist.view(np.uint64)), (name, k)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_groups_that_span_every_shard(hip_lib, oracle_mod, metric):
    """group_of = row % 300: every group has rows on all three shards.  The oracle shows that the case is exercised: the
    three shards' own first-k lists, concatenated, hold a repeated group, and for a winning group the best row lies on
    another shard than some shard's own offer for that group."""
    rng = np.random.default_rng(300 + metric)
    n, d, k = BOUNDS[-1][1], 48, 20
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    group_of = (np.arange(n) % 300).astype(np.int32)
    for g in range(300):
        assert all(((np.flatnonzero(group_of == g) >= lo) & (np.flatnonzero(group_of == g) < hi)).any() for lo, hi in BOUNDS)
    eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n)
    want = _first_of_each_group(eids, edist, group_of, k)
    offers = []  # every shard's own answer: (ids, groups)
    for lo, hi in BOUNDS:
        sel = (eids >= lo) & (eids < hi)
        wi, _, wg = _first_of_each_group(eids[sel], edist[sel], group_of, k)
        offers.append((wi, wg))
    all_groups = np.concatenate([o[1] for o in offers])
    assert len(set(all_groups.tolist())) < len(all_groups), "no group is offered by two shards"
    crossed = 0
    for rid, g in zip(want[0], want[2]):
        home = [i for i, (lo, hi) in enumerate(BOUNDS) if lo <= rid < hi][0]
        crossed += any(g in o[1].tolist() for i, o in enumerate(offers) if i != home)
    assert crossed >= 1, "no winning group is offered by a shard that does not hold its best row"
    with Shards(rows, BOUNDS, metric, group_of, 300) as sh:
        for kk in (1, k, 100, 305):
            _same(sh.search(q, kk), _first_of_each_group(eids, edist, group_of, kk), ("span", kk))
        got = sh.search(q, k)
    w = _whole(rows, metric, group_of, 300, q, k)
    assert np.array_equal(got[0], w[0]) and np.array_equal(got[1].view(np.uint64), w[1].view(np.uint64)) and np.array_equal(got[3], w[3])


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_ties_across_shards(hip_lib, oracle_mod, metric):
    """Identical rows on two shards, in the same group and in different groups: the smaller id wins, and the other group
    still appears."""
    rng = np.random.default_rng(17 + metric)
    n, d = BOUNDS[-1][1], 40
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    near = (q * np.float32(0.9)).astype(np.float32) if metric != IP else (q * np.float32(9)).astype(np.float32)
    rows[[100, 1500, 2600]] = near                          # the nearest rows of all, identical, one per shard
    second = near.copy()  # the next nearest, clearly behind the three and clearly before everything else
    if metric == IP:
        second *= np.float32(0.8)
    else:
        second[0] += np.float32(0.25 * np.linalg.norm(near))
    rows[[200, 1700]] = second
    group_of = rng.integers(10, 500, n).astype(np.int32)
    group_of[[100, 2600]] = 0   # the same group on shards 0 and 2 ...
    group_of[1500] = 1          # ... and another group's identical row between them, on shard 1
    group_of[[200, 1700]] = 2   # one group, identical rows on shards 0 and 1
    eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n)
    want = _first_of_each_group(eids, edist, group_of, 10)
    assert want[0][0] == 100 and want[0][1] == 1500 and want[2][:2].tolist() == [0, 1] and edist[0] == edist[1] == edist[2]
    assert 200 in want[0].tolist() and 1700 not in want[0].tolist() and 2600 not in want[0].tolist()
    with Shards(rows, BOUNDS, metric, group_of, 500) as sh:
        for k in (1, 2, 10, 100):
            _same(sh.search(q, k), _first_of_each_group(eids, edist, group_of, k), ("ties", k))


def test_side_rows_reach_the_block(hip_lib, oracle_mod):
    """A group of 40 identical rows, nearest to the query, on shard 1: 39 of them are not the head by f32 key but as near.
    They land in the shard's device block behind the re-rank's entries (the header counts more entries than the block has
    groups), stats[1] moves; a block they do not fit in reports count > entries, and the retry is exact."""
    from tostore_amd import _ffi
    from tostore_amd.sharded import merge_candidate_blocks

    rng = np.random.default_rng(41)
    n, d, k = BOUNDS[-1][1], 32, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    rows[1100:1140] = q + np.float32(0.01)
    group_of = rng.integers(1, 400, n).astype(np.int32)
    group_of[1100:1140] = 0
    eids, edist = oracle_mod.search_exhaustive(rows, q, L2, n)
    want = _first_of_each_group(eids, edist, group_of, k)
    assert want[0][0] == 1100
    with Shards(rows, BOUNDS, L2, group_of, 400) as sh:
        s0 = sh.stats()
        host, bb, entries = sh.blocks(q, k)
        s1 = sh.stats()
        assert [b["searches"] - a["searches"] for a, b in zip(s0, s1)] == [1, 1, 1]
        assert s1[1]["side_rows"] - s0[1]["side_rows"] >= 39
        count, ent, got = _decode(host[1].tobytes())
        assert ent == entries and count <= entries and len(got) == count
        ids = [e[0] for e in got]
        assert len(set(ids)) == len(ids) and set(range(1100, 1140)) <= set(ids) and all(1000 <= i < 2531 for i in ids)
        groups_held = {int(group_of[i]) for i in ids}
        assert count > len(groups_held) and count >= len(groups_held) + 39
        sums = oracle_mod.exact_sums(q, rows[1100], L2)
        for e in got:
            if 1100 <= e[0] < 1140:
                assert struct.pack("<dd", *e[1:]) == struct.pack("<dd", *sums)
        _same(merge_candidate_blocks(L2, d, q, k, None, np.ascontiguousarray(host[:, :bb]), 3, entries, group_of=group_of), want, "default blocks")
        # blocks of 32 entries: the 39 side rows alone do not fit
        host, bb, _ = sh.blocks(q, k, entries=32)  # (asserts the guards)
        count, ent, got = _decode(host[1].tobytes())
        assert ent == 32 and count > 32 and len(got) == 32 and all(1000 <= e[0] < 2531 for e in got)
        with pytest.raises(_ffi.TshError) as e:
            merge_candidate_blocks(L2, d, q, k, None, np.ascontiguousarray(host[:, :bb]), 3, 32, group_of=group_of)
        assert e.value.code == _ffi.TSH_E_OVERFLOW and e.value.needed_entries >= 64
        retries = []
        _same(sh.search(q, k, entries=32, retries=retries), want, "through the retry")
        assert len(retries) >= 1


def test_side_list_larger_than_its_capacity(hip_lib, oracle_mod):
    """3000 identical rows in one group on shard 1, nearest to the query, n = 5000: the side list (1024 rows) overflows,
    the job is redone once with a larger one -- into the same device block, every appended row exactly once."""
    from tostore_amd.sharded import merge_candidate_blocks

    rng = np.random.default_rng(51)
    n, d, k = 5000, 32, 10
    bounds = [(0, 1000), (1000, 4531), (4531, n)]
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    same = 1000 + rng.choice(3531, 3000, replace=False)
    rows[same] = q + np.float32(0.01)
    group_of = rng.integers(1, 400, n).astype(np.int32)
    group_of[same] = 0
    eids, edist = oracle_mod.search_exhaustive(rows, q, L2, n)
    want = _first_of_each_group(eids, edist, group_of, k)
    with Shards(rows, bounds, L2, group_of, 400) as sh:
        s0 = sh.stats()
        host, bb, entries = sh.blocks(q, k, entries=4096)  # (room for the whole crowd: this call is not retried)
        s1 = sh.stats()
        assert [b["redone"] - a["redone"] for a, b in zip(s0, s1)] == [0, 1, 0]
        assert [b["searches"] - a["searches"] for a, b in zip(s0, s1)] == [1, 1, 1]
        assert s1[1]["side_rows"] - s0[1]["side_rows"] >= 2999
        count, ent, got = _decode(host[1].tobytes())
        assert ent == 4096 and 3000 <= count <= 4096 and len(got) == count
        ids = sorted(e[0] for e in got)
        assert len(set(ids)) == len(ids), "an appended row is in the block twice"
        assert set(same.tolist()) <= set(ids) and all(1000 <= i < 4531 for i in ids)
        _same(merge_candidate_blocks(L2, d, q, k, None, np.ascontiguousarray(host[:, :bb]), 3, entries, group_of=group_of), want, "after the redo")
        # ... and with default blocks, through the overflow retry
        _same(sh.search(q, k), want, "default blocks")


def test_k2_list_overflow_runs_the_wide_band_over_heads(hip_lib, oracle_mod):
    """600 groups with identical best distances at k = 100: more heads inside the band than a block holds.  The wide-band
    pass rewrites the device block; side rows and quarantined rows are appended again behind it."""
    rng = np.random.default_rng(53)
    n, d, k = 5000, 32, 100
    bounds = [(0, 1000), (1000, 2531), (2531, n)]
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    group_of = (np.arange(n) % 600).astype(np.int32)
    # every group's best on the last shard (its rows 2531 .. 4999 hold four or five rows of every group): 600 equal heads
    # there against blocks of 256 entries
    last = 2531 + rng.permutation(n - 2531)
    best = np.asarray([last[group_of[last] == g][0] for g in range(600)])
    rows[best] = q + np.float32(0.01)
    extra = np.setdiff1d(last, best)[:30]  # ... and thirty more rows like them in group 0: its side rows
    rows[extra] = q + np.float32(0.01)
    group_of[extra] = 0
    eids, edist = oracle_mod.search_exhaustive(rows, q, L2, n)
    with Shards(rows, bounds, L2, group_of, 600) as sh:
        # the wide-band pass rewrote the last shard's block (600 heads, 256 written): the side rows were appended again
        # behind it, so the header asks for room for all of them
        host, bb, entries = sh.blocks(q, k)
        count, ent, got = _decode(host[2].tobytes())
        assert ent == entries == 256 and count >= 600 + 30 and len(got) == 256
        f0 = [s.counters()["fallback_searches"] for s in sh.idx]
        retries = []
        _same(sh.search(q, k, retries=retries), _first_of_each_group(eids, edist, group_of, k), "block overflow")
        f1 = [s.counters()["fallback_searches"] for s in sh.idx]
        assert f1[2] > f0[2] and f1[:2] == f0[:2]
        assert retries and retries[0] >= 600  # (the wide band's 600 heads did not fit: the usual overflow protocol)


def test_quarantined_rows_and_safe_mode(hip_lib, oracle_mod):
    """Inner product: a quarantined row (an inf element) that is its group's best and one (1e20) that is its group's only
    row, each on another shard than the group's other rows; then a shard with more than 1024 irregular rows: safe mode,
    no device group passes there (stats[3] moves), its blocks are tsh_search_shard's and the merge does the grouping."""
    rng = np.random.default_rng(57)
    n, d = 1500, 32
    bounds = [(0, 500), (500, 1001), (1001, n)]
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    rows[100, 3] = np.inf if q[3] > 0 else -np.inf   # inner product +inf: distance -inf, the best of everything
    rows[1240, 7] = 1e20 if q[7] > 0 else -1e20      # a huge finite one
    group_of = (np.arange(n) % 200).astype(np.int32)
    group_of[300] = 101   # group 100: row 100 on shard 0, rows 500, 700, 900 on shard 1, rows 1100, 1300 on shard 2
    group_of[1240] = 250  # a group of its own
    assert [int(i) for i in np.flatnonzero(group_of == 100)] == [100, 500, 700, 900, 1100, 1300]
    with np.errstate(all="ignore"):
        eids, edist = oracle_mod.search_exhaustive(rows, q, IP, n)
    assert eids[0] == 100 and eids[1] == 1240
    with Shards(rows, bounds, IP, group_of, 251) as sh:
        assert [s.counters()["quarantined_rows"] for s in sh.idx] == [1, 0, 1]
        for k in (1, 2, 10, 100):
            _same(sh.search(q, k), _first_of_each_group(eids, edist, group_of, k), ("quarantined", k))
        got = sh.search(q, 10)
        assert got[0][0, :2].tolist() == [100, 1240] and got[3][0, :2].tolist() == [100, 250]
        # behind a mask that drops row 100, by pointer: group 100 is represented by another shard's row
        keep = np.ones(n, bool)
        keep[100] = False
        bits = np.packbits(keep, bitorder="little")
        with np.errstate(all="ignore"):
            lst = oracle_mod.search_exhaustive(rows, q, IP, n, None, bits)
        _same(sh.search(q, 250, mask=bits), _first_of_each_group(lst[0], lst[1], group_of, 250), "row 100 masked")
    n, d = 2048, 8
    rows = rng.standard_normal((n + 500, d)).astype(np.float32)
    bad = rng.choice(n, 1100, replace=False)
    rows[bad[:550], 2] = np.inf
    rows[bad[550:], 6] = np.nan
    q = rng.standard_normal(d).astype(np.float32)
    group_of = rng.integers(-1, 300, n + 500).astype(np.int32)
    with np.errstate(all="ignore"):
        eids, edist = oracle_mod.search_exhaustive(rows, q, L2, n + 500)
    with Shards(rows, [(0, n), (n, n + 500)], L2, group_of, 300) as sh:
        assert [s.counters()["safe_mode"] for s in sh.idx] == [1, 0]
        s0 = sh.stats()
        for k in (1, 10, 100):
            _same(sh.search(q, k), _first_of_each_group(eids, edist, group_of, k), ("safe mode", k))
        s1 = sh.stats()
        assert s1[0]["no_device_passes"] - s0[0]["no_device_passes"] == s1[0]["searches"] - s0[0]["searches"] >= 3
        assert s1[0]["side_rows"] == s0[0]["side_rows"]
        assert s1[1]["no_device_passes"] == s0[1]["no_device_passes"] and s1[1]["searches"] - s0[1]["searches"] >= 3


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_masks_and_tombstones(hip_lib, oracle_mod, metric):
    """A dense keep-50 % mask and "nothing kept", by pointer and by handle, over three shards; then tombstones set after
    the groups handles were made: a whole tile, every shard's last row and the nearest group's head."""
    from tostore_amd import HipMask

    rng = np.random.default_rng(80 + metric)
    n, d = BOUNDS[-1][1], 64
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    group_of = (np.arange(n) % 300).astype(np.int32)
    full = oracle_mod.search_exhaustive(rows, q, metric, n)
    with Shards(rows, BOUNDS, metric, group_of, 300) as sh:
        for kept in (rng.random(n) < 0.5, np.zeros(n, bool)):
            bits = np.packbits(kept, bitorder="little")
            lst = oracle_mod.search_exhaustive(rows, q, metric, n, None, bits)
            handles = [HipMask(s, bits) for s in sh.idx]
            try:
                for k in (1, K, 100):
                    want = _first_of_each_group(lst[0], lst[1], group_of, k)
                    _same(sh.search(q, k, mask=bits), want, ("pointer mask", int(kept.sum()), k))
                    _same(sh.search(q, k, handles=handles), want, ("mask handle", int(kept.sum()), k))
            finally:
                for h in handles:
                    h.close()
        dead = sorted(set(range(64, 128)) | {hi - 1 for _, hi in BOUNDS} | {int(full[0][0])})
        sh.set_deleted(dead)
        alive = np.ones(n, bool)
        alive[dead] = False
        lst = oracle_mod.search_exhaustive(rows, q, metric, n, None, np.packbits(alive, bitorder="little"))
        for k in (1, K, 100, 305):
            _same(sh.search(q, k), _first_of_each_group(lst[0], lst[1], group_of, k), ("tombstones", k))
        half = rng.random(n) < 0.5
        bits = np.packbits(half, bitorder="little")
        lst = oracle_mod.search_exhaustive(rows, q, metric, n, None, np.packbits(alive & half, bitorder="little"))
        _same(sh.search(q, 100, mask=bits), _first_of_each_group(lst[0], lst[1], group_of, 100), "tombstones and a mask")


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_selective_mask_takes_the_list_scan(hip_lib, oracle_mod, metric):
    """One shard of 4608 rows (and a small one behind it) behind a 2 % mask, by pointer and by handle: the big shard's
    grouped searches are list scans, none takes the exact path, and the merged answer is exact."""
    from tostore_amd import HipMask

    rng = np.random.default_rng(5 + metric)
    n, d = 5200, 100
    bounds = [(0, 4608), (4608, n)]
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    group_of = (np.arange(n) // 3 % 700).astype(np.int32)
    bits = np.packbits(rng.random(n) < 0.02, bitorder="little")
    lst = oracle_mod.search_exhaustive(rows, q, metric, n, None, bits)
    with Shards(rows, bounds, metric, group_of, 700) as sh:
        big = sh.idx[0]
        handles = [HipMask(s, bits) for s in sh.idx]
        try:
            for form in ({"mask": bits}, {"handles": handles}):
                c0 = big.counters()
                for k in (1, K, 100):
                    _same(sh.search(q, k, **form), _first_of_each_group(lst[0], lst[1], group_of, k), (sorted(form), k))
                c1 = big.counters()
                scans = c1["scan_launches"] - c0["scan_launches"]
                assert scans >= 3 and c1["list_scans"] - c0["list_scans"] == scans and c1["exact_scans"] == c0["exact_scans"]
        finally:
            for h in handles:
                h.close()


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_shards_at_tile_edges(hip_lib, oracle_mod, metric):
    """Shards of 1, 63, 64, 65 and 129 rows, an empty one in the middle, and a larger one behind them."""
    rng = np.random.default_rng(64 + metric)
    bounds = [(0, 1), (1, 64), (64, 128), (128, 128), (128, 193), (193, 322), (322, 700)]
    n, d = 700, 24
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n)
    half = np.packbits(rng.random(n) < 0.5, bitorder="little")
    lst = oracle_mod.search_exhaustive(rows, q, metric, n, None, half)
    with Shards(rows, bounds, metric, np.zeros(0, np.int32), 0) as sh:
        for name in ("runs7", "random", "mix"):
            group_of, n_groups = _layout(name, n, rng)
            sh.set_groups(group_of, n_groups)
            for k in (1, K, 100, _n_groups_in(eids, group_of) + 5):
                _same(sh.search(q, k), _first_of_each_group(eids, edist, group_of, k), (name, k))
            _same(sh.search(q, K, mask=half), _first_of_each_group(lst[0], lst[1], group_of, K), (name, "masked"))
            # the empty shard's blocks: valid, empty
            host, bb, entries = sh.blocks(q, K)
            count, ent, got = _decode(host[3].tobytes())
            assert count == 0 and ent == entries and got == []


def test_progressive_form(hip_lib, oracle_mod):
    """tsh_search_shard_begin_grouped over 9 queries with step 1 and 4, taken through _progress: whenever _progress(want)
    returns, the leading blocks are final -- entry for entry the blocks tsh_search_shard_grouped writes (places within a
    block are drawn with atomic adds), side rows included."""
    import torch

    from tostore_amd import HipVectorIndex, _ffi
    from tostore_amd.sharded import merge_candidate_blocks

    L = _ffi.lib()
    rng = np.random.default_rng(99)
    n, d, nq, k, base = 6000, 64, 9, K, 777
    rows = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((nq, d)).astype(np.float32)
    for i in range(nq):  # forty identical rows in one group beside every query: side rows in every block
        rows[600 * i + 5:600 * i + 45] = qs[i] + np.float32(0.01)
    group_of = np.concatenate([np.full(base, -1), np.arange(n) // 50]).astype(np.int32)  # GLOBAL ids: the shard starts at 777
    entries = L.tsh_default_block_entries(k)
    bb = L.tsh_candidate_block_bytes(entries)
    with HipVectorIndex(d, L2, shard_device=0, row_base=base) as s:
        s.append(base, rows)
        with s.make_groups(group_of, n // 50 + 1) as h:
            one = torch.full((nq * bb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            _ffi.check(L.tsh_search_shard_grouped(s._h, qs.ctypes.data_as(_ffi.p_f32), nq, k, None, None, h.handle(), entries,
                                                  ctypes.c_void_p(one.data_ptr()), None))
            a = one.cpu().numpy()
            assert np.all(a[nq * bb:] == 0xA5)
            for i in range(nq):
                count, _, got = _decode(a[i * bb:(i + 1) * bb].tobytes())
                assert count <= entries and set(range(base + 600 * i + 5, base + 600 * i + 45)) <= {e[0] for e in got}, i
            for step, wants in ((1, (1, 2, 5, 9)), (4, (4, 8, 9))):
                two = torch.full((nq * bb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                s0 = s.search_grouped_stats()
                st = ctypes.c_void_p()
                _ffi.check(L.tsh_search_shard_begin_grouped(s._h, qs.ctypes.data_as(_ffi.p_f32), nq, k, None, None, h.handle(), entries,
                                                            ctypes.c_void_p(two.data_ptr()), step, ctypes.byref(st)))
                try:
                    for want in wants:
                        done = ctypes.c_int32(0)
                        _ffi.check(L.tsh_search_shard_progress(st, want, ctypes.byref(done)))
                        assert done.value >= want
                        b = two.cpu().numpy()  # (host-synchronised: the leading blocks are final)
                        for i in range(want):
                            assert _canonical(a[i * bb:(i + 1) * bb].tobytes()) == _canonical(b[i * bb:(i + 1) * bb].tobytes()), (step, want, i)
                finally:
                    rc = L.tsh_search_shard_end(st)
                _ffi.check(rc)
                assert np.all(two.cpu().numpy()[nq * bb:] == 0xA5)
                assert s.search_grouped_stats()["searches"] - s0["searches"] == nq
            # ... and the blocks are the right ones
            got = merge_candidate_blocks(L2, d, qs, k, None, a[:nq * bb], 1, entries, group_of=group_of)
            for i in range(nq):
                eids, edist = oracle_mod.search_exhaustive(rows, qs[i], L2, n)
                _same(got, _first_of_each_group(eids + base, edist, group_of, k), ("progressive", i), q=i)


def test_never_batched(hip_lib, oracle_mod):
    """64 queries in one call, whatever TSH_OPT_BATCH_MIN_NQ says (1: by estimated cost; 2: from two queries on): the
    batched-call counters do not move, every query is its own scan."""
    from tostore_amd import HipVectorIndex, _ffi
    from tostore_amd.sharded import merge_candidate_blocks

    import torch

    L = _ffi.lib()
    rng = np.random.default_rng(67)
    n, d, nq, k = 5000, 128, 64, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((nq, d)).astype(np.float32)
    group_of = (np.arange(n) // 7).astype(np.int32)
    entries = L.tsh_default_block_entries(k)
    bb = L.tsh_candidate_block_bytes(entries)
    with HipVectorIndex(d, L2, shard_device=0, row_base=0) as s:
        s.append(0, rows)
        with s.make_groups(group_of, n // 7 + 1) as h:
            buf = torch.full((nq * bb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            for min_nq in (1, 2):
                s.set_batch_min_nq(min_nq)
                c0, s0 = s.counters(), s.search_grouped_stats()
                _ffi.check(L.tsh_search_shard_grouped(s._h, qs.ctypes.data_as(_ffi.p_f32), nq, k, None, None, h.handle(), entries,
                                                      ctypes.c_void_p(buf.data_ptr()), None))
                st = ctypes.c_void_p()
                _ffi.check(L.tsh_search_shard_begin_grouped(s._h, qs.ctypes.data_as(_ffi.p_f32), nq, k, None, None, h.handle(), entries,
                                                            ctypes.c_void_p(buf.data_ptr()), 16, ctypes.byref(st)))
                _ffi.check(L.tsh_search_shard_progress(st, nq, None))
                _ffi.check(L.tsh_search_shard_end(st))
                c1 = s.counters()
                assert c1["batch_launches"] == c0["batch_launches"] and c1["exact_scans"] == c0["exact_scans"], min_nq
                assert c1["scan_launches"] - c0["scan_launches"] == 2 * nq and c1["searches"] - c0["searches"] == 2 * nq
                assert s.search_grouped_stats()["searches"] - s0["searches"] == 2 * nq
            host = buf.cpu().numpy()
            assert np.all(host[nq * bb:] == 0xA5)
            got = merge_candidate_blocks(L2, d, qs, k, None, host[:nq * bb], 1, entries, group_of=group_of)
            for i in (0, 31, 63):
                eids, edist = oracle_mod.search_exhaustive(rows, qs[i], L2, n)
                _same(got, _first_of_each_group(eids, edist, group_of, k), ("64 queries", i), q=i)


def test_errors_and_trivial_cases(hip_lib, oracle_mod):
    """Both mask forms, NULL groups, handles of another index, an orphaned groups handle: TSH_E_BAD_ARG, nothing written.
    k <= 0 and an empty shard: valid empty blocks that merge to count 0."""
    import torch

    from tostore_amd import HipMask, HipVectorIndex, _ffi
    from tostore_amd.sharded import merge_candidate_blocks

    L = _ffi.lib()
    rng = np.random.default_rng(71)
    n, d, k = 500, 16, 5
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((1, d)).astype(np.float32)
    qp = q.ctypes.data_as(_ffi.p_f32)
    group_of = (np.arange(n) // 4).astype(np.int32)
    bits = np.packbits(np.ones(n, bool), bitorder="little")
    mp = bits.ctypes.data_as(_ffi.p_u8)
    entries = L.tsh_default_block_entries(k)
    bb = L.tsh_candidate_block_bytes(entries)
    buf = torch.full((bb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    at = ctypes.c_void_p(buf.data_ptr())

    def both(idx_h, maskp, maskh, gh, kk=k):
        st = ctypes.c_void_p(1)
        rc1 = L.tsh_search_shard_grouped(idx_h, qp, 1, kk, maskp, maskh, gh, entries, at, None)
        rc2 = L.tsh_search_shard_begin_grouped(idx_h, qp, 1, kk, maskp, maskh, gh, entries, at, 0, ctypes.byref(st))
        if rc2 == 0:
            rc2 = L.tsh_search_shard_progress(st, 1, None)
            rc_end = L.tsh_search_shard_end(st)
            rc2 = rc2 or rc_end
        else:
            assert not st.value  # (a failed begin leaves no handle behind)
        return rc1, rc2

    with HipVectorIndex(d, L2, shard_device=0, row_base=0) as s, HipVectorIndex(d, L2, shard_device=0, row_base=0) as other:
        s.append(0, rows)
        other.append(0, rows)
        with s.make_groups(group_of, n) as h, other.make_groups(group_of, n) as h_other, HipMask(s, bits) as mh, \
                HipMask(other, bits) as mh_other:
            bad = (_ffi.TSH_E_BAD_ARG, _ffi.TSH_E_BAD_ARG)
            assert both(s._h, mp, mh.handle(), h.handle()) == bad and "at most one" in _ffi.last_error()
            assert both(s._h, None, None, None) == bad and "groups is NULL" in _ffi.last_error()
            assert both(s._h, None, None, h_other.handle()) == bad and "another index" in _ffi.last_error()
            assert both(s._h, None, mh_other.handle(), h.handle()) == bad and "another index" in _ffi.last_error()
            assert np.all(buf.cpu().numpy() == 0xA5), "a refused call wrote to the blocks"
            # a good call, by both mask forms
            assert both(s._h, mp, None, h.handle()) == (0, 0) and both(s._h, None, mh.handle(), h.handle()) == (0, 0)
            host = buf.cpu().numpy()
            eids, edist = oracle_mod.search_exhaustive(rows, q[0], L2, n)
            _same(merge_candidate_blocks(L2, d, q, k, None, host[:bb], 1, entries, group_of=group_of),
                  _first_of_each_group(eids, edist, group_of, k), "a good call")
            # k <= 0: a valid empty block that merges to nothing
            for kk in (0, -3):
                buf.fill_(0xA5)
                torch.cuda.synchronize()
                assert both(s._h, None, None, h.handle(), kk) == (0, 0)
                host = buf.cpu().numpy()
                count, ent, got = _decode(host[:bb].tobytes())
                assert count == 0 and ent == entries and np.all(host[bb:] == 0xA5)
                ids, dist, cnt, grp = merge_candidate_blocks(L2, d, q, kk, None, host[:bb], 1, entries, group_of=group_of)
                assert cnt[0] == 0
                ids, dist, cnt, grp = merge_candidate_blocks(L2, d, q, k, None, host[:bb], 1, entries, group_of=group_of)
                assert cnt[0] == 0 and np.all(ids == -1) and np.all(grp == -1)
        # an orphaned groups handle: its index is destroyed first
        orphan_idx = HipVectorIndex(d, L2, shard_device=0, row_base=0)
        orphan_idx.append(0, rows)
        orphan = orphan_idx.make_groups(group_of, n)
        orphan_idx._live_masks().discard(orphan)
        raw = orphan.handle()
        orphan_idx.close()
        assert both(s._h, None, None, raw) == (_ffi.TSH_E_BAD_ARG, _ffi.TSH_E_BAD_ARG) and "destroyed" in _ffi.last_error()
        orphan.close()  # frees only the handle
    # an empty shard
    with HipVectorIndex(d, L2, shard_device=0, row_base=300) as empty:
        with empty.make_groups(group_of, n) as h:
            buf.fill_(0xA5)
            torch.cuda.synchronize()
            assert both(empty._h, None, None, h.handle()) == (0, 0)
            host = buf.cpu().numpy()
            count, ent, got = _decode(host[:bb].tobytes())
            assert count == 0 and ent == entries and np.all(host[bb:] == 0xA5)
            assert merge_candidate_blocks(L2, d, q, k, None, host[:bb], 1, entries, group_of=group_of)[2][0] == 0
