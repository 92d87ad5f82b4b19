"""GPU: count the rows a search would return (tsh_search_count, include/tostore_hip.h).  The specification is one
sentence -- out_count[q] is the number of entries in the list tsh_search_after would return with k = infinity -- and the
oracle is search_exhaustive(k = n) with all_distances: the list's length past the cursor, an integer, compared with ==,
under masks, tombstones, gaps, thresholds at and one ulp beside a row's distance, ties, quarantined rows, safe mode,
several shards and shard handles."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2


def _query(rng, oracle_mod, d, metric):
    q = rng.standard_normal(d).astype(np.float32)
    return oracle_mod.normalize_f32(q) if metric == COS else q


def _order_key(d):
    """double.compareTo as an integer order (-0.0 below +0.0, every NaN the one largest key)"""
    d = np.atleast_1d(np.asarray(d, np.float64))
    b = d.view(np.uint64)
    key = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    return np.where(np.isnan(d), np.uint64(0xFFFFFFFFFFFFFFFF), key)


def _past(eids, edist, cursor):
    """How many entries of an oracle list follow the cursor strictly in (compareTo(distance), id) order"""
    if cursor is None or cursor[0] == -math.inf:
        return len(eids)
    ck, keys = _order_key(cursor[0])[0], _order_key(edist)
    return int(np.count_nonzero((keys > ck) | ((keys == ck) & (eids > cursor[1]))))


def _thresholds(dist):
    """From the rows' own distances: minimum, maximum and median (the dense part, where the side list is busiest), each one
    ulp below and above; and None, +inf, -inf, 0.0, -0.0"""
    fin = np.sort(dist[np.isfinite(dist)])
    out = [None, math.inf, -math.inf, 0.0, -0.0]
    for v in (fin[0], fin[-1], fin[len(fin) // 2]):
        out += [float(v), float(np.nextafter(v, -np.inf)), float(np.nextafter(v, np.inf))]
    return out


def _cursors(eids, edist, base=0):
    """-inf; a row's own (d, id); (d, id - 1); (d, 2^62); a distance between two rows -- around the middle of the list the
    oracle gives without a threshold (an empty list: cursors that name no row).  'No cursor' is the callers' own call."""
    if len(eids) == 0:
        return [(-math.inf, 0), (0.5, 0), (0.5, -1), (0.5, 2**62), (0.25, 0)]
    m = len(eids) // 2
    d, i = float(edist[m]), int(eids[m]) + base
    nxt = float(edist[min(m + 1, len(eids) - 1)])
    return [(-math.inf, 7), (d, i), (d, i - 1), (d, 2**62), (d + (nxt - d) / 2, 0)]


def _check(idx, oracle_mod, rows, q, metric, mask=None, keep=None, base=0, thresholds=None, dist=None):
    """Every threshold x every cursor, the five cursors in one call (one scan each), 'no cursor' in a call of its own.
    keep: what the oracle is told lives (the mask, the tombstones and the gaps together), as packed bits."""
    n = len(rows)
    with np.errstate(all="ignore"):
        dist = oracle_mod.all_distances(q, rows, metric) if dist is None else dist
        cursors = _cursors(*oracle_mod.search_exhaustive(rows, q, metric, n, None, keep), base=base)
    a_dist = np.asarray([c[0] for c in cursors], np.float64)
    a_id = np.asarray([c[1] for c in cursors], np.int64)
    qs = np.tile(q, (len(cursors), 1))
    for thr in _thresholds(dist) if thresholds is None else thresholds:
        with np.errstate(all="ignore"):
            eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n, thr, keep)
        eids = eids + base
        got = idx.search_count(q, thr, mask)
        assert got.dtype == np.int64 and got.shape == (1,)
        assert int(got[0]) == len(eids), (n, thr, "no cursor", int(got[0]), len(eids))
        got = idx.search_count(qs, thr, mask, (a_dist, a_id))
        want = [_past(eids, edist, c) for c in cursors]
        assert got.tolist() == want, (n, thr, cursors, got.tolist(), want)


@pytest.mark.parametrize("metric", [L2, IP, COS])
@pytest.mark.parametrize("d", [4, 128, 257])
def test_count_equals_the_list_length(hip_lib, oracle_mod, metric, d):
    """Every shape dense, behind a keep-50 % mask as a pointer and as a handle, behind 'nothing kept', with a keep-1 % mask
    at n = 5000 (the list scan) in both forms, with tombstones (one whole tile and the last row) and with a gap of
    absent ids."""
    from tostore_amd import HipMask, HipVectorIndex

    rng = np.random.default_rng(1000 * d + metric)
    for n in (1, 63, 64, 65, 4097, 5000):
        rows = rng.standard_normal((n, d)).astype(np.float32)
        q = _query(rng, oracle_mod, d, metric)
        dist = oracle_mod.all_distances(q, rows, metric)
        with HipVectorIndex(d, metric, capacity_rows=n) as idx:
            idx.append(0, rows)
            _check(idx, oracle_mod, rows, q, metric, dist=dist)
            kept = rng.random(n) < 0.5
            if n == 1:
                kept[:] = True
            masks = [kept, np.zeros(n, bool)]
            if n == 5000:
                masks.append(rng.random(n) < 0.01)
            for m in masks:
                bits = np.packbits(m, bitorder="little")
                c0 = idx.counters()
                _check(idx, oracle_mod, rows, q, metric, mask=bits, keep=bits, dist=dist)
                with HipMask(idx, bits) as h:
                    _check(idx, oracle_mod, rows, q, metric, mask=h, keep=bits, dist=dist)
                if n == 5000 and d == 257 and 0 < m.sum() < 100:  # (rows of 257 floats: a width the list scan serves)
                    assert idx.counters()["list_scans"] > c0["list_scans"]
            # tombstones: one whole tile and the last row
            t = 1 if n >= 129 else 0
            dead = sorted(set(range(64 * t, min(64 * t + 64, n))) | {n - 1})
            idx.set_deleted(np.asarray(dead, np.int64))
            alive = np.ones(n, bool)
            alive[dead] = False
            _check(idx, oracle_mod, rows, q, metric, keep=np.packbits(alive, bitorder="little"), dist=dist)
        if n >= 65:  # a gap of absent ids: rows [0, a) and [b, n), nothing in between (a, b inside tiles)
            a, b = n // 3 + 1, n // 3 + 1 + min(n // 4, 64 + 30)
            present = np.ones(n, bool)
            present[a:b] = False
            with HipVectorIndex(d, metric, capacity_rows=n) as idx:
                idx.append(0, rows[:a])
                idx.append(b, rows[b:])
                assert idx.size == n
                _check(idx, oracle_mod, rows, q, metric, keep=np.packbits(present, bitorder="little"), dist=dist)


def test_count_768(hip_lib, oracle_mod):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(768)
    n, d = 5000, 768
    rows = rng.standard_normal((n, d)).astype(np.float32)
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        _check(idx, oracle_mod, rows, _query(rng, oracle_mod, d, L2), L2)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_pages_and_counts_agree(hip_lib, oracle_mod, metric):
    """Walk pages of k = 7: after every page, count(after = its last entry) is the total minus the rows consumed so far, and
    0 after the short page -- with and without a threshold, dense and behind a handle."""
    from tostore_amd import HipMask, HipVectorIndex

    rng = np.random.default_rng(41 + metric)
    n, d, k = 300, 24, 7
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    dist = oracle_mod.all_distances(q, rows, metric)
    bits = np.packbits(rng.random(n) < 0.5, bitorder="little")
    with HipVectorIndex(d, metric, capacity_rows=n) as idx, HipVectorIndex(d, metric, capacity_rows=n) as other:
        idx.append(0, rows)
        other.append(0, rows)
        with HipMask(idx, bits) as h:
            for thr, mask, keep in ((None, None, None), (float(np.sort(dist)[200]), None, None), (None, h, bits), (float(np.sort(dist)[200]), bits, bits)):
                eids, _ = oracle_mod.search_exhaustive(rows, q, metric, n, thr, keep)
                total = int(idx.search_count(q, thr, mask)[0])
                assert total == len(eids)
                assert int(idx.search_count(q, thr, mask, (-math.inf, 0))[0]) == total
                cur, used = (-math.inf, 0), 0
                while True:
                    ids, dd, cnt = idx.search_after(q, k, cur, thr, mask)
                    c = int(cnt[0])
                    used += c
                    if c:
                        cur = (float(dd[0, c - 1]), int(ids[0, c - 1]))
                    assert int(idx.search_count(q, thr, mask, cur)[0]) == total - used
                    if c < k:
                        break
                assert used == total and int(idx.search_count(q, thr, mask, cur)[0]) == 0
        # count(threshold = none, cursor = (d_i, id_i)) is n_live minus the rank of row i
        eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n)
        at = np.arange(0, n, 13)
        got = idx.search_count(np.tile(q, (len(at), 1)), None, None, (edist[at].copy(), eids[at].copy()))
        assert got.tolist() == (n - 1 - at).tolist()
        # errors: both masks, one NULL cursor array, a mask of another index
        from tostore_amd import _ffi

        L = _ffi.lib()
        out = np.full(1, 99, np.int64)
        a_dist, a_id = np.zeros(1), np.zeros(1, np.int64)
        qp, op = q.ctypes.data_as(_ffi.p_f32), out.ctypes.data_as(_ffi.p_i64)
        with HipMask(idx, bits) as h, HipMask(other, bits) as foreign:
            assert L.tsh_search_count(idx._h, qp, 1, math.nan, bits.ctypes.data_as(_ffi.p_u8), h.handle(), None, None, op) == _ffi.TSH_E_BAD_ARG
            assert L.tsh_search_count(idx._h, qp, 1, math.nan, None, None, a_dist.ctypes.data_as(_ffi.p_f64), None, op) == _ffi.TSH_E_BAD_ARG
            assert L.tsh_search_count(idx._h, qp, 1, math.nan, None, None, None, a_id.ctypes.data_as(_ffi.p_i64), op) == _ffi.TSH_E_BAD_ARG
            assert L.tsh_search_count(idx._h, qp, 1, math.nan, None, foreign.handle(), None, None, op) == _ffi.TSH_E_BAD_ARG
            assert out[0] == 99
            assert L.tsh_search_count(idx._h, qp, 1, math.nan, None, h.handle(), None, None, op) == _ffi.TSH_OK
            assert out[0] == len(oracle_mod.search_exhaustive(rows, q, metric, n, None, bits)[0])
        with pytest.raises(ValueError):
            idx.search_count(q, None, h)  # a closed HipMask
    # an empty index: counts of 0
    with HipVectorIndex(d, metric, capacity_rows=16) as idx:
        assert idx.search_count(np.tile(q, (3, 1))).tolist() == [0, 0, 0]
        assert idx.search_count(q, 1.0, None, (0.5, 3)).tolist() == [0]


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_ties(hip_lib, oracle_mod, metric):
    """1500 identical rows among others, more than the side list holds, the threshold at their distance and a cursor id in
    their middle: exact, and redone exactly once per such search (each on a handle of its own: the context that was given a
    larger side list keeps it, so a second such search on the same handle need not be redone)."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(3)
    d = 8
    v = rng.standard_normal(d).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    others = rng.standard_normal((700, d)).astype(np.float32)
    rows = np.concatenate([others[:300], np.tile(v, (1500, 1)), others[300:]])
    n = len(rows)
    dist = oracle_mod.all_distances(q, rows, metric)
    tie = float(dist[300])
    assert len(set(dist[300:1800].view(np.uint64).tolist())) == 1
    cases = ((tie, None), (tie, (tie, 1000)), (None, (tie, 1000)), (float(np.nextafter(tie, -np.inf)), (tie, 1000)),
             (float(np.nextafter(tie, np.inf)), (float(np.nextafter(tie, -np.inf)), 5)))
    for thr, cursor in cases:  # (an index each: a context keeps the larger side list a redo gave it)
        eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n, thr)
        with HipVectorIndex(d, metric, capacity_rows=n) as idx:
            idx.append(0, rows)
            s0 = idx.search_count_stats()
            got = int(idx.search_count(q, thr, None, cursor)[0])
            s1 = idx.search_count_stats()
            assert got == _past(eids, edist, cursor), (thr, cursor)
            assert s1["redone"] - s0["redone"] == 1 and s1["searches"] - s0["searches"] == 1, (thr, cursor, s0, s1)
            assert s1["side_rows"] - s0["side_rows"] >= 1500
            # ... and again on the same handle: exact, with or without another redo
            assert int(idx.search_count(q, thr, None, cursor)[0]) == got
            assert idx.search_count_stats()["redone"] - s1["redone"] <= 1
    with HipVectorIndex(d, metric, capacity_rows=n) as idx:
        idx.append(0, rows)
        # off the crowd: nothing is redone
        s0 = idx.search_count_stats()
        thr = float(np.sort(dist)[100]) if dist[300] > np.sort(dist)[100] else float(np.sort(dist)[-100])
        assert int(idx.search_count(q, thr)[0]) == len(oracle_mod.search_exhaustive(rows, q, metric, n, thr)[0])
        assert idx.search_count_stats()["redone"] == s0["redone"]


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_rows_outside_the_model(hip_lib, oracle_mod, metric):
    """Rows with a NaN, an infinite and a 1e20 element are quarantined and counted by their exact distances: a NaN distance
    passes every threshold, as the oracle has it; a +inf or NaN cursor and a threshold below everything run no scan."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(11 + metric)
    n, d = 500, 32
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    rows[100, 3] = -np.inf if q[3] > 0 else np.inf
    rows[40, 5] = np.nan
    rows[333, 7] = 1e20
    with np.errstate(all="ignore"):
        dist = oracle_mod.all_distances(q, rows, metric)
    with HipVectorIndex(d, metric, capacity_rows=n) as idx:
        idx.append(0, rows)
        assert idx.counters()["quarantined_rows"] == 3 and not idx.counters()["safe_mode"]
        _check(idx, oracle_mod, rows, q, metric, dist=dist)
        bits = np.packbits(rng.random(n) < 0.5, bitorder="little")
        _check(idx, oracle_mod, rows, q, metric, mask=bits, keep=bits, dist=dist)
        with np.errstate(all="ignore"):
            eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n)
        s0, c0 = idx.search_count_stats(), idx.counters()
        for cursor in ((math.inf, -1), (math.nan, int(eids[-1])), (math.nan, -1)):
            assert int(idx.search_count(q, None, None, cursor)[0]) == _past(eids, edist, cursor)
        with np.errstate(all="ignore"):
            assert int(idx.search_count(q, -math.inf)[0]) == len(oracle_mod.search_exhaustive(rows, q, metric, n, -math.inf)[0])
        s1 = idx.search_count_stats()
        assert s1["no_window"] - s0["no_window"] == 4 and s1["searches"] - s0["searches"] == 4
        assert idx.counters()["scan_launches"] == c0["scan_launches"]  # no scan ran for them


def test_safe_mode(hip_lib, oracle_mod):
    """More than 1024 irregular rows: the shard is in safe mode, no window pass runs, every row is decided by its exact
    distance."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(13)
    n, d = 2048, 8
    rows = rng.standard_normal((n, d)).astype(np.float32)
    bad = rng.choice(n, 1100, replace=False)
    rows[bad[:550], 2] = np.inf
    rows[bad[550:], 6] = np.nan
    q = rng.standard_normal(d).astype(np.float32)
    with np.errstate(all="ignore"):
        dist = oracle_mod.all_distances(q, rows, L2)
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        assert idx.counters()["safe_mode"]
        s0 = idx.search_count_stats()
        _check(idx, oracle_mod, rows, q, L2, dist=dist)
        bits = np.packbits(rng.random(n) < 0.5, bitorder="little")
        _check(idx, oracle_mod, rows, q, L2, mask=bits, keep=bits, dist=dist)
        s1 = idx.search_count_stats()
        assert s1["no_window"] - s0["no_window"] == s1["searches"] - s0["searches"] > 0 and s1["side_rows"] == s0["side_rows"]


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_many_queries_and_launch_counters(hip_lib, oracle_mod, metric):
    """A 9-query call equals nine 1-query calls and never takes the batched path; scan_launches grows by one per counted
    query; a tsh_search and a tsh_search_after behind a count still equal the oracle (the count words are left clean)."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(19 + metric)
    n, d, k = 5000, 128, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    qs = np.stack([_query(rng, oracle_mod, d, metric) for _ in range(9)])
    dist = oracle_mod.all_distances(qs[0], rows, metric)
    thr = float(np.sort(dist)[n // 2])
    with HipVectorIndex(d, metric, capacity_rows=n) as idx:
        idx.append(0, rows)
        idx.set_batch_min_nq(2)  # (the batched path would take a 9-query tsh_search)
        c0 = idx.counters()
        many = idx.search_count(qs, thr)
        c1 = idx.counters()
        assert c1["batch_launches"] == c0["batch_launches"]
        assert c1["scan_launches"] - c0["scan_launches"] == 9 and c1["searches"] - c0["searches"] == 9
        ones = [int(idx.search_count(qs[i], thr)[0]) for i in range(9)]
        want = [len(oracle_mod.search_exhaustive(rows, qs[i], metric, n, thr)[0]) for i in range(9)]
        assert many.tolist() == ones == want
        c2 = idx.counters()
        assert c2["scan_launches"] - c1["scan_launches"] == 9 and c2["exact_scans"] == c0["exact_scans"]
        for i in range(3):  # count, search, count, cursor search: on the same handle
            eids, edist = oracle_mod.search_exhaustive(rows, qs[i], metric, 2 * k)
            assert int(idx.search_count(qs[i], thr)[0]) == want[i]
            ids, dd, cnt = idx.search(qs[i], k)
            assert cnt[0] == k and np.array_equal(ids[0], eids[:k]) and np.array_equal(dd[0].view(np.uint64), edist[:k].view(np.uint64))
            assert int(idx.search_count(qs[i], thr, None, (float(edist[k - 1]), int(eids[k - 1])))[0]) == want[i] - k
            ids, dd, cnt = idx.search_after(qs[i], k, (float(edist[k - 1]), int(eids[k - 1])))
            assert cnt[0] == k and np.array_equal(ids[0], eids[k:]) and np.array_equal(dd[0].view(np.uint64), edist[k:].view(np.uint64))


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_several_shards_and_shard_handles(hip_lib, oracle_mod, metric, monkeypatch):
    """A handle over three shards sums its shards' counts; two shard handles with an unaligned row_base count their own rows
    under a GLOBAL mask and a GLOBAL cursor, and their counts add up to the whole index's."""
    from tostore_amd import HipMask, HipVectorIndex, _ffi

    rng = np.random.default_rng(17 + metric)
    n, d = 3000, 40
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[1500:1600] = rows[100]  # ties across shards
    q = _query(rng, oracle_mod, d, metric)
    dist = oracle_mod.all_distances(q, rows, metric)
    thresholds = [None, float(dist[100]), float(np.nextafter(dist[100], -np.inf)), float(np.sort(dist)[n // 2]), -math.inf]
    bits = np.packbits(rng.random(n) < 0.5, bitorder="little")
    monkeypatch.setenv("TSH_SHARDS_SHARE_DEVICES", "1")
    _ffi.enable_test_hooks()
    try:
        with HipVectorIndex(d, metric, capacity_rows=n, n_devices=3) as idx:
            idx.append(0, rows)
            _check(idx, oracle_mod, rows, q, metric, thresholds=thresholds, dist=dist)
            _check(idx, oracle_mod, rows, q, metric, mask=bits, keep=bits, thresholds=thresholds, dist=dist)
            with HipMask(idx, bits) as h:
                _check(idx, oracle_mod, rows, q, metric, mask=h, keep=bits, thresholds=thresholds, dist=dist)
            dead = rng.choice(n, 200, replace=False)
            idx.set_deleted(dead)
            alive = np.ones(n, bool)
            alive[dead] = False
            _check(idx, oracle_mod, rows, q, metric, keep=np.packbits(alive, bitorder="little"), thresholds=thresholds, dist=dist)
    finally:
        _ffi.enable_test_hooks(False)
    # two shard handles: rows [0, cut) and [cut, n) of one index, cut inside a tile and inside a mask byte
    cut = 1237
    with HipVectorIndex(d, metric, capacity_rows=cut, shard_device=0, row_base=0) as lo, \
            HipVectorIndex(d, metric, capacity_rows=n - cut, shard_device=0, row_base=cut) as hi:
        lo.append(0, rows[:cut])
        hi.append(cut, rows[cut:])
        cursors = _cursors(*oracle_mod.search_exhaustive(rows, q, metric, n, None, bits))
        cursors[1] = (float(dist[100]), 1550)  # (inside the crowd of ties that spans both shards)
        a_dist = np.asarray([c[0] for c in cursors], np.float64)
        a_id = np.asarray([c[1] for c in cursors], np.int64)
        qs = np.tile(q, (len(cursors), 1))
        with HipMask(lo, bits) as h_lo, HipMask(hi, bits) as h_hi:
            for thr in thresholds:
                for m_lo, m_hi, keep in ((None, None, None), (bits, bits, bits), (h_lo, h_hi, bits)):
                    eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n, thr, keep)
                    assert int(lo.search_count(q, thr, m_lo)[0] + hi.search_count(q, thr, m_hi)[0]) == len(eids)
                    got = lo.search_count(qs, thr, m_lo, (a_dist, a_id)) + hi.search_count(qs, thr, m_hi, (a_dist, a_id))
                    assert got.tolist() == [_past(eids, edist, c) for c in cursors], (thr, cursors)
                    own = lo.search_count(qs, thr, m_lo, (a_dist, a_id))  # ... and each covers its own rows only
                    assert own.tolist() == [_past(eids[eids < cut], edist[eids < cut], c) for c in cursors]


def test_the_window_runs_on_the_device(hip_lib, oracle_mod):
    """5000 x 128 Gaussian rows, L2: the window's two bands are each about 1.4e-6 wide relative to the distance against
    roughly 25 000 rows per unit of relative distance at the median -- well under one row per band.  The cap of 8 side rows
    per count only keeps "everything is ambiguous" from passing; no count is redone or answered without the window."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(23)
    n, d = 5000, 128
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    dist = oracle_mod.all_distances(q, rows, L2)
    eids, edist = oracle_mod.search_exhaustive(rows, q, L2, n)
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        s0, c0 = idx.search_count_stats(), idx.counters()
        at = np.arange(5, n, 50)
        for i in at:
            thr, cur = float(edist[min(i + 1000, n - 1)]), (float(edist[i]), int(eids[i]))
            assert int(idx.search_count(q, thr, None, cur)[0]) == min(1000, n - 1 - i)
        s1, c1 = idx.search_count_stats(), idx.counters()
        searches = s1["searches"] - s0["searches"]
        side = s1["side_rows"] - s0["side_rows"]
        print(f"side rows per count {side / searches:.3f}")
        assert searches == len(at) and s1["redone"] == s0["redone"] and s1["no_window"] == s0["no_window"]
        assert 2 <= side / searches <= 8  # (the cursor's own row and the threshold's are undecided on every count)
        assert c1["candidates_total"] == c0["candidates_total"] and c1["fallback_searches"] == c0["fallback_searches"]
