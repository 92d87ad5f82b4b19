"""GPU: search after a cursor (tsh_search_after / tsh_search_submit_after, include/tostore_hip.h).  The specification is
one sentence -- successive pages, each started from the last entry of the page before, concatenate to exactly the
list tsh_search would return with k = infinity -- and the oracle is search_exhaustive(k = n): ids and distances bit
for bit, under masks, tombstones, thresholds, ties, quarantined rows, safe mode, several shards and tickets."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2
K = 7
START = (-math.inf, 0)


def _same_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def _query(rng, oracle_mod, d, metric):
    q = rng.standard_normal(d).astype(np.float32)
    return oracle_mod.normalize_f32(q) if metric == COS else q


def _walk(idx, q, k=K, thr=None, mask=None, start=START, limit=5000):
    """Pages from `start` to exhaustion -> (ids, distances, pages).  The last page is short (or empty), and a page asked
    for after a short one is empty."""
    ids_all, dist_all, cur, pages = [], [], start, 0
    while True:
        ids, dist, cnt = idx.search_after(q, k, cur, thr, mask)
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
        assert int(idx.search_after(q, k, cur, thr, mask)[2][0]) == 0
    return np.concatenate(ids_all), np.concatenate(dist_all), pages


def _check_walk(idx, oracle_mod, rows, q, metric, thr=None, mask=None, keep=None, base=0, k=K):
    """keep: what the oracle is told lives (the mask and the tombstones together), as packed bits"""
    eids, edist = oracle_mod.search_exhaustive(rows, q, metric, len(rows), thr, keep)
    ids, dist, pages = _walk(idx, q, k, thr, mask)
    assert np.array_equal(ids, eids + base), (len(ids), len(eids))
    assert _same_dist(dist, edist)
    assert pages == len(eids) // k + 1
    return eids, edist


@pytest.mark.parametrize("metric", [L2, IP, COS])
@pytest.mark.parametrize("d", [4, 128, 257])
def test_page_walk_equals_the_full_list(hip_lib, oracle_mod, metric, d):
    """Every shape dense, behind a keep-50 % mask as a pointer and as a handle, and with tombstones."""
    from tostore_amd import HipMask, HipVectorIndex

    rng = np.random.default_rng(100 * d + metric)
    for n in (1, 63, 64, 65, 4097, 5000):
        rows = rng.standard_normal((n, d)).astype(np.float32)
        q = _query(rng, oracle_mod, d, metric)
        with HipVectorIndex(d, metric, capacity_rows=n) as idx:
            idx.append(0, rows)
            _check_walk(idx, oracle_mod, rows, q, metric)
            kept = rng.random(n) < 0.5
            if n == 1:
                kept[:] = True  # (the one row kept; "nothing kept" is n = 63's turn)
            if n == 63:
                kept[:] = False
            bits = np.packbits(kept, bitorder="little")
            _check_walk(idx, oracle_mod, rows, q, metric, mask=bits, keep=bits)
            with HipMask(idx, bits) as h:
                _check_walk(idx, oracle_mod, rows, q, metric, mask=h, keep=bits)
            # tombstones: one whole tile and the last row
            t = 1 if n >= 129 else 0
            dead = sorted(set(range(64 * t, min(64 * t + 64, n))) | {n - 1})
            idx.set_deleted(np.asarray(dead, np.int64))
            alive = np.ones(n, bool)
            alive[dead] = False
            _check_walk(idx, oracle_mod, rows, q, metric, keep=np.packbits(alive, bitorder="little"))


def test_page_walk_768(hip_lib, oracle_mod):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(768)
    n, d = 5000, 768
    rows = rng.standard_normal((n, d)).astype(np.float32)
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        _check_walk(idx, oracle_mod, rows, _query(rng, oracle_mod, d, L2), L2)


@pytest.mark.parametrize("form", ["pointer", "handle"])
@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_page_walk_behind_a_mask(hip_lib, oracle_mod, metric, form):
    """A keep-50 % mask in both forms, with tombstones on top, at a shape with a partial last tile and at one with few rows."""
    from tostore_amd import HipMask, HipVectorIndex

    rng = np.random.default_rng(31 + metric)
    for n, d in ((65, 4), (5000, 128), (4097, 257)):
        rows = rng.standard_normal((n, d)).astype(np.float32)
        q = _query(rng, oracle_mod, d, metric)
        kept = rng.random(n) < 0.5
        bits = np.packbits(kept, bitorder="little")
        with HipVectorIndex(d, metric, capacity_rows=n) as idx:
            idx.append(0, rows)
            mask = HipMask(idx, bits) if form == "handle" else bits
            _check_walk(idx, oracle_mod, rows, q, metric, mask=mask, keep=bits)
            dead = rng.choice(n, n // 10, replace=False)
            idx.set_deleted(dead)
            alive = kept.copy()
            alive[dead] = False
            _check_walk(idx, oracle_mod, rows, q, metric, mask=mask, keep=np.packbits(alive, bitorder="little"))


@pytest.mark.parametrize("form", ["pointer", "handle"])
@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_selective_mask_takes_the_list_scan(hip_lib, oracle_mod, metric, form):
    from tostore_amd import HipMask, HipVectorIndex

    rng = np.random.default_rng(5 + metric)
    n = 40_000
    for d, listed in ((100, True), (128, False)):  # (rows of 128 floats: a width the list scan does not serve -- tiles)
        rows = rng.standard_normal((n, d)).astype(np.float32)
        q = _query(rng, oracle_mod, d, metric)
        kept = rng.random(n) < 0.02
        bits = np.packbits(kept, bitorder="little")
        with HipVectorIndex(d, metric, capacity_rows=n) as idx:
            idx.append(0, rows)
            mask = HipMask(idx, bits) if form == "handle" else bits
            c0 = idx.counters()
            eids, _ = _check_walk(idx, oracle_mod, rows, q, metric, mask=mask, keep=bits)
            c1 = idx.counters()
            scans = c1["scan_launches"] - c0["scan_launches"]
            assert scans >= len(eids) // K + 1 and c1["searches"] - c0["searches"] == scans
            assert c1["list_scans"] - c0["list_scans"] == (scans if listed else 0)
            assert c1["exact_scans"] == c0["exact_scans"]


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_cursor_edges(hip_lib, oracle_mod, metric):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(77 + metric)
    n, d, k = 1000, 64, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n)
    with HipVectorIndex(d, metric, capacity_rows=n) as idx:
        idx.append(0, rows)
        # -inf, whatever the id: tsh_search, bit for bit -- several queries in one call as well
        qs = np.stack([q, _query(rng, oracle_mod, d, metric), _query(rng, oracle_mod, d, metric)])
        s_ids, s_dist, s_cnt = idx.search(qs, k)
        for any_id in (0, -5, 2**40):
            a_ids, a_dist, a_cnt = idx.search_after(qs, k, (-math.inf, any_id))
            assert np.array_equal(a_cnt, s_cnt) and np.array_equal(a_ids, s_ids)
            assert np.array_equal(a_dist.view(np.uint64), s_dist.view(np.uint64))
        # a cursor per query
        a_ids, a_dist, a_cnt = idx.search_after(qs, k, (s_dist[:, k - 1].copy(), s_ids[:, k - 1].copy()))
        for i in range(3):
            e, ed = oracle_mod.search_exhaustive(rows, qs[i], metric, 2 * k)
            assert a_cnt[i] == k and np.array_equal(a_ids[i], e[k:]) and _same_dist(a_dist[i], ed[k:])
        # past the last row
        ids, dist, cnt = idx.search_after(q, k, (float(edist[-1]), int(eids[-1])))
        assert cnt[0] == 0
        ids, dist, cnt = idx.search_after(q, k, (float(edist[-1]), n + 5))
        assert cnt[0] == 0
        # between two rows, on no row: by distance, and by an id that names no row at a row's distance
        mid = (float(edist[499]) + float(edist[500])) / 2
        assert edist[499] < mid < edist[500]
        ids, dist, cnt = idx.search_after(q, k, (mid, 0))
        assert cnt[0] == k and np.array_equal(ids[0], eids[500:510]) and _same_dist(dist[0], edist[500:510])
        ids, dist, cnt = idx.search_after(q, k, (float(edist[500]), int(eids[500]) - 1 if eids[500] else -1))
        assert np.array_equal(ids[0], eids[500:510])
        ids, dist, cnt = idx.search_after(q, k, (float(edist[500]), 2**40))
        assert np.array_equal(ids[0], eids[501:511])
        # k larger than what remains
        ids, dist, cnt = idx.search_after(q, 50, (float(edist[-4]), int(eids[-4])))
        assert cnt[0] == 3 and np.array_equal(ids[0, :3], eids[-3:]) and np.all(ids[0, 3:] == -1)
        # a threshold that cuts inside a page
        thr = float(edist[503])
        ids, dist, cnt = idx.search_after(q, k, (float(edist[499]), int(eids[499])), thr)
        assert cnt[0] == 4 and np.array_equal(ids[0, :4], eids[500:504])
        # the cursor on a tombstoned row's (distance, id)
        gone = int(eids[500])
        idx.set_deleted(np.asarray([gone], np.int64))
        ids, dist, cnt = idx.search_after(q, k, (float(edist[500]), gone))
        assert np.array_equal(ids[0], eids[501:511]) and _same_dist(dist[0], edist[501:511])
        ids, dist, cnt = idx.search_after(q, k, (float(edist[499]), int(eids[499])))
        assert np.array_equal(ids[0], eids[501:511])
        # k <= 0 and nq = 0: OK with counts 0 -- through the index ...
        ids, dist, cnt = idx.search_after(q, 0, START)
        assert cnt[0] == 0 and ids.shape == (1, 0)
        ids, dist, cnt = idx.search_after(np.zeros((0, d), np.float32), k, START)
        assert ids.shape == (0, k) and dist.shape == (0, k) and cnt.shape == (0,)
        ids, dist, cnt = idx.search_after(np.zeros((0, d), np.float32), k, (np.zeros(0), np.zeros(0, np.int64)))
        assert ids.shape == (0, k) and cnt.shape == (0,)
        # ... and through the raw entry, with a real cursor: k = -1, k = 0 answer OK and count 0, nq = 0 touches nothing
        from tostore_amd import _ffi

        L = _ffi.lib()
        a_dist, a_id = np.asarray([float(edist[10])]), np.asarray([int(eids[10])], np.int64)
        for kk, nq in ((-1, 1), (0, 1), (k, 0)):
            r_ids, r_dist, r_cnt = np.full(k, 77, np.int64), np.full(k, 7.0), np.full(1, 99, np.int32)
            rc = L.tsh_search_after(idx._h, q.ctypes.data_as(_ffi.p_f32), nq, kk, math.nan, None, None,
                                    a_dist.ctypes.data_as(_ffi.p_f64), a_id.ctypes.data_as(_ffi.p_i64),
                                    r_ids.ctypes.data_as(_ffi.p_i64), r_dist.ctypes.data_as(_ffi.p_f64), r_cnt.ctypes.data_as(_ffi.p_i32))
            assert rc == _ffi.TSH_OK, (kk, nq, _ffi.last_error())
            assert r_cnt[0] == (99 if nq == 0 else 0) and np.all(r_ids == 77) and np.all(r_dist == 7.0)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_ties(hip_lib, oracle_mod, metric):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(3)
    d = 8
    v = rng.standard_normal(d).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    # 300 identical rows over five tiles, the cursor on the 150th
    rows = np.tile(v, (300, 1))
    dist = oracle_mod.all_distances(q, rows, metric)
    assert len(set(dist.view(np.uint64).tolist())) == 1
    with HipVectorIndex(d, metric, capacity_rows=300) as idx:
        idx.append(0, rows)
        ids, dd, cnt = idx.search_after(q, K, (float(dist[0]), 149))
        assert cnt[0] == K and np.array_equal(ids[0], np.arange(150, 150 + K)) and _same_dist(dd[0], dist[:K])
        _check_walk(idx, oracle_mod, rows, q, metric)
    # 1500 identical rows among others, more than the side list holds: one redo with a larger list, and exact
    others = rng.standard_normal((700, d)).astype(np.float32)
    rows = np.concatenate([others[:300], np.tile(v, (1500, 1)), others[300:]])
    eids, edist = oracle_mod.search_exhaustive(rows, q, metric, len(rows))
    first = int(np.flatnonzero(eids == 300)[0])  # where the crowd starts in the list
    assert np.array_equal(eids[first:first + 1500], np.arange(300, 1800))
    with HipVectorIndex(d, metric, capacity_rows=len(rows)) as idx:
        idx.append(0, rows)
        s0 = idx.search_after_stats()
        ids, dd, cnt = idx.search_after(q, 20, (float(edist[first + 700]), int(eids[first + 700])))
        s1 = idx.search_after_stats()
        assert cnt[0] == 20 and np.array_equal(ids[0], eids[first + 701:first + 721]) and _same_dist(dd[0], edist[first + 701:first + 721])
        assert s1["redone"] - s0["redone"] == 1 and s1["searches"] - s0["searches"] == 1
        assert s1["side_rows"] - s0["side_rows"] >= 1500
        _check_walk(idx, oracle_mod, rows, q, metric, k=100)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_rows_outside_the_model_come_last(hip_lib, oracle_mod, metric):
    """One row with an infinite element (placed so that its distance is +inf or NaN, never -inf) and one with a NaN element
    are quarantined: the walk returns each exactly once, the non-finite distances last, in compareTo order; a +inf or NaN
    cursor continues.  (Cosine gives the NaN row the distance 1 -- its denominator is not positive -- so one row is last.)"""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(11 + metric)
    n, d = 500, 32
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    rows[100, 3] = -np.inf if q[3] > 0 else np.inf
    rows[40, 5] = np.nan
    with np.errstate(all="ignore"):
        eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n)
    tail = int((~np.isfinite(edist)).sum())
    assert tail == (1 if metric == COS else 2) and not np.isfinite(edist[-tail:]).any() and not (edist == -np.inf).any()
    assert set(eids[-tail:].tolist()) <= {40, 100}
    with HipVectorIndex(d, metric, capacity_rows=n) as idx:
        idx.append(0, rows)
        assert idx.counters()["quarantined_rows"] == 2 and not idx.counters()["safe_mode"]
        ids, dist, _ = _walk(idx, q)
        assert np.array_equal(ids, eids) and _same_dist(dist, edist)
        s0 = idx.search_after_stats()
        c0 = idx.counters()
        ids, dist, cnt = idx.search_after(q, K, (float(edist[-tail]), int(eids[-tail])))  # a +inf or NaN cursor
        assert cnt[0] == tail - 1 and np.array_equal(ids[0, :cnt[0]], eids[n - tail + 1:]) and _same_dist(dist[0, :cnt[0]], edist[n - tail + 1:])
        ids, dist, cnt = idx.search_after(q, K, (math.inf, -1))  # +inf rows of any id follow it, NaN rows after them
        assert cnt[0] == tail and np.array_equal(ids[0, :tail], eids[-tail:]) and _same_dist(dist[0, :tail], edist[-tail:])
        ids, dist, cnt = idx.search_after(q, K, (math.nan, int(eids[-1])))
        assert cnt[0] == 0
        s1 = idx.search_after_stats()
        assert s1["no_floor"] - s0["no_floor"] == 3 and s1["searches"] - s0["searches"] == 3
        assert idx.counters()["scan_launches"] == c0["scan_launches"]  # no scan ran for them


def test_safe_mode(hip_lib, oracle_mod):
    """More than 1024 irregular rows: the shard is in safe mode, no floor pass runs, the finaliser filters."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(13)
    n, d = 2048, 8
    rows = rng.standard_normal((n, d)).astype(np.float32)
    bad = rng.choice(n, 1100, replace=False)
    rows[bad[:550], 2] = np.inf
    rows[bad[550:], 6] = np.nan
    q = rng.standard_normal(d).astype(np.float32)
    with np.errstate(all="ignore"):
        eids, edist = oracle_mod.search_exhaustive(rows, q, L2, n)
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        assert idx.counters()["safe_mode"]
        s0 = idx.search_after_stats()
        ids, dist, pages = _walk(idx, q, k=100)
        s1 = idx.search_after_stats()
        assert np.array_equal(ids, eids) and _same_dist(dist, edist)
        # (every page but the first, which starts from -inf, is counted as answered without a floor)
        assert s1["no_floor"] - s0["no_floor"] == s1["searches"] - s0["searches"] - 1 and s1["side_rows"] == s0["side_rows"]


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_several_shards_and_shard_handles(hip_lib, oracle_mod, metric, monkeypatch):
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(17 + metric)
    n, d = 3000, 40
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[1500:1600] = rows[100]  # ties across shards
    q = _query(rng, oracle_mod, d, metric)
    monkeypatch.setenv("TSH_SHARDS_SHARE_DEVICES", "1")
    _ffi.enable_test_hooks()
    try:
        with HipVectorIndex(d, metric, capacity_rows=n, n_devices=3) as idx:
            idx.append(0, rows)
            dead = rng.choice(n, 200, replace=False)
            idx.set_deleted(dead)
            alive = np.ones(n, bool)
            alive[dead] = False
            _check_walk(idx, oracle_mod, rows, q, metric, keep=np.packbits(alive, bitorder="little"))
            bits = np.packbits(rng.random(n) < 0.5, bitorder="little")
            both = np.packbits(alive & np.unpackbits(bits, bitorder="little")[:n].astype(bool), bitorder="little")
            _check_walk(idx, oracle_mod, rows, q, metric, mask=bits, keep=both)
    finally:
        _ffi.enable_test_hooks(False)
    base = 1000
    with HipVectorIndex(d, metric, capacity_rows=n, shard_device=0, row_base=base) as idx:
        idx.append(base, rows)
        _check_walk(idx, oracle_mod, rows, q, metric, base=base)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_tickets(hip_lib, oracle_mod, metric):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(19 + metric)
    n, d, k = 5000, 128, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n)
    bits = np.packbits(rng.random(n) < 0.5, bitorder="little")
    with HipVectorIndex(d, metric, capacity_rows=n) as idx:
        idx.append(0, rows)
        at = [0, 9, 2500, n - 4]
        cursors = [START] + [(float(edist[i]), int(eids[i])) for i in at[1:]]
        sync = [idx.search_after(q, k, c) for c in cursors]
        tickets = [idx.submit(q, k, after=c) for c in cursors]
        for i in (2, 0, 3, 1):
            t_ids, t_dist = idx.wait(tickets[i])
            ids, dist, cnt = sync[i]
            assert np.array_equal(t_ids, ids[0, :cnt[0]]) and _same_dist(t_dist, dist[0, :cnt[0]])
            lo = 0 if i == 0 else at[i] + 1
            assert np.array_equal(t_ids, eids[lo:lo + k])
        # ... behind a mask, with a threshold at the wait
        mids, mdist = oracle_mod.search_exhaustive(rows, q, metric, n, None, bits)
        t = idx.submit(q, k, bits, after=(float(mdist[99]), int(mids[99])))
        t_ids, t_dist = idx.wait(t, float(mdist[104]))
        assert np.array_equal(t_ids, mids[100:105]) and _same_dist(t_dist, mdist[100:105])


def test_the_floor_runs_on_the_device(hip_lib, oracle_mod):
    """5000 x 128 Gaussian rows, L2: the floor's interval is about 1.4e-6 wide relative to the distance, against roughly
    25 000 rows per unit of relative distance -- about one row, the cursor's own, per page.  The cap of 8 only keeps
    "everything is ambiguous" from passing.  And the select behind the floor sees no more candidates than tsh_search's."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(23)
    n, d = 5000, 128
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        c0 = idx.counters()
        for _ in range(8):
            idx.search(q, K)
        c1 = idx.counters()
        per_search = (c1["candidates_total"] - c0["candidates_total"]) / 8
        s0 = idx.search_after_stats()
        _check_walk(idx, oracle_mod, rows, q, L2)
        s1, c2 = idx.search_after_stats(), idx.counters()
        searches = s1["searches"] - s0["searches"]
        side = s1["side_rows"] - s0["side_rows"]
        per_page = (c2["candidates_total"] - c1["candidates_total"]) / searches
        print(f"side rows per cursor search {side / searches:.3f}; candidates per page {per_page:.2f}, per tsh_search {per_search:.2f}")
        assert searches == n // K + 2 and s1["redone"] == s0["redone"] and s1["no_floor"] == s0["no_floor"]
        assert side / searches <= 8
        assert side >= searches - 3  # (the cursor's own row is undecided on every page that starts from one)
        assert per_page <= 2 * per_search
        assert c2["fallback_searches"] == c1["fallback_searches"]
