"""GPU: the coarse int8 first pass behind tombstones, gaps, quarantined rows and dense caller masks
(TSH_OPT_SCAN_I8_MASKED, scan_i8_kernel<MASKED> + tsh_scan_i8.hip.h).

One tombstone, one gap of absent ids, one quarantined row or a WHERE mask too dense for the list scan used to take a big
shard's single-query scans off the int8 copy for good.  The masked kernel loads the live rows' bytes only, dead tiles
never count towards the threshold, a dead tile's stale keys never survive, and a query whose survivor list overflows is
redone BEHIND THE SAME MASK.  Every index here forces the route on small shapes (option value 2), switches the exact path
and the batched path off, and is held to the oracle with a keep mask: ids, counts and distance bits.  Unless a test says
otherwise every search must also have run over the int8 copy (scan_i8_stats) with nothing redone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2, IP, COS = 0, 1, 2
N = 20_037  # 313 whole tiles and one of 5 rows
TILE = 64


def _open(d, metric, rows, capacity=None, mode=2, dense_mode=1, first=0, **kw):
    from tostore_amd import HipVectorIndex

    idx = HipVectorIndex(d, metric, capacity_rows=capacity or len(rows), **kw)
    idx.set_scan_i8(dense_mode)
    idx.set_scan_i8_masked(mode)
    idx.set_exact_scan_rows(0)
    idx.set_batch_min_nq(0)
    if len(rows):
        idx.append(first, rows)
    return idx


def _same(got, ref, what="", base=0):
    assert np.array_equal(got[2], ref[2]), "counts differ from the oracle's " + what
    ref_ids = np.where(ref[0] >= 0, ref[0] + base, ref[0])
    assert np.array_equal(got[0], ref_ids), "ids differ from the oracle's " + what
    assert np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), "distance bits differ from the oracle's " + what


def _corpus(rng, n, d, metric, nq=8, oracle_mod=None):
    rows = rng.standard_normal((n, d), dtype=np.float32)
    if metric != COS:
        rows *= rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    if metric == COS:
        qs = np.stack([oracle_mod.normalize_f32(q) for q in qs])
    return rows, qs


def _bits(keep):
    return np.packbits(np.asarray(keep, bool), bitorder="little")


def _search_i8(idx, qs, k, ref, mask=None, what="", base=0):
    """One call of len(qs) single-query searches: the oracle's answer, every scan over the int8 copy, none redone."""
    s0 = idx.scan_i8_stats()
    _same(idx.search(qs, k, None, mask), ref, what, base)
    s1 = idx.scan_i8_stats()
    assert s1["scans"] - s0["scans"] == len(qs), (what, s0, s1)
    assert s1["redone"] == s0["redone"], (what, s0, s1)


def _tickets_i8(idx, qs, k, ref, mask=None, what=""):
    s0 = idx.scan_i8_stats()
    tickets = [idx.submit(q, k, mask) for q in qs]
    for i, t in enumerate(tickets):
        ids, dist = idx.wait(t)
        assert np.array_equal(ids, ref[0][i, :ref[2][i]]), (what, i)
        assert np.array_equal(dist.view(np.uint64), ref[1][i, :ref[2][i]].view(np.uint64)), (what, i)
    s1 = idx.scan_i8_stats()
    assert s1["scans"] - s0["scans"] == len(qs), (what, s0, s1)
    assert s1["redone"] == s0["redone"], (what, s0, s1)


def _edge_tombstones(rng, n, nearest):
    """live[] after: the queries' nearest rows, a random 5 %, one whole tile, all but one row of another, tiles left
    with 9 and with 57 live rows (a short last batch of one row each, an odd number of batches), every row of the last,
    partial tile."""
    live = rng.random(n) >= 0.05
    live[7 * TILE:8 * TILE] = False
    for tile, cnt in ((11, 1), (20, 9), (21, 57), (150, 9), (151, 57)):
        if (tile + 1) * TILE > n:
            continue
        live[tile * TILE:(tile + 1) * TILE] = False
        cand = np.setdiff1d(np.arange(tile * TILE, (tile + 1) * TILE), nearest)  # (the survivors are not the nearest rows)
        live[rng.choice(cand, cnt, replace=False)] = True
    live[nearest] = False
    live[(n // TILE) * TILE:] = False
    assert live[11 * TILE:12 * TILE].sum() == 1 and live[20 * TILE:21 * TILE].sum() == 9 and live[21 * TILE:22 * TILE].sum() == 57
    return live


@pytest.mark.parametrize("metric", [L2, IP, COS])
@pytest.mark.parametrize("d", [768, 1000, 1536, 2048])  # 2048: the widest int8 row, eight chunks
def test_tombstones_at_tile_edges(hip_lib, oracle_mod, d, metric):
    rng = np.random.default_rng(1000 * d + metric)
    rows, qs = _corpus(rng, N, d, metric, oracle_mod=oracle_mod)
    nearest = oracle_mod.search_heap_many_mt(rows, qs, metric, 1)[0][:, 0]
    live = _edge_tombstones(rng, N, nearest)
    keep = _bits(live)
    with _open(d, metric, rows) as idx:
        idx.set_deleted(np.nonzero(~live)[0])
        for k in (10, 100):
            ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, keep)
            assert not np.isin(ref[0], nearest).any()
            _search_i8(idx, qs, k, ref, None, "k=%d" % k)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_caller_masks(hip_lib, oracle_mod, metric):
    d, k = 768, 30
    rng = np.random.default_rng(300 + metric)
    rows, qs = _corpus(rng, N, d, metric, oracle_mod=oracle_mod)
    span = np.zeros(N, bool)
    span[1000 + 17:9000 + 45] = True  # one range that starts and ends inside a tile
    masks = {"keep 70 %": rng.random(N) < 0.7, "keep 10 %": rng.random(N) < 0.1, "one range": span}
    with _open(d, metric, rows) as idx:
        def every_form(keep, ref, what):
            _search_i8(idx, qs, k, ref, _bits(keep), what + ", pointer")
            _tickets_i8(idx, qs, k, ref, _bits(keep), what + ", pointer, tickets")
            with idx.make_mask(_bits(keep)) as h:
                _search_i8(idx, qs, k, ref, h, what + ", handle")
                _search_i8(idx, qs[:1], k, [r[:1] for r in ref], h, what + ", handle, a lone query")
                _tickets_i8(idx, qs, k, ref, h, what + ", handle, tickets")

        for what, keep in masks.items():
            every_form(keep, oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(keep)), what)
        # ... combined with tombstones: the nearest kept rows of every query, under every mask, die
        dead_all = np.zeros(N, bool)
        for keep in masks.values():
            dead = np.unique(oracle_mod.search_heap_many_mt(rows, qs, metric, 3, None, _bits(keep & ~dead_all))[0])
            idx.set_deleted(dead)
            dead_all[dead] = True
        for what, keep in masks.items():
            ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(keep & ~dead_all))
            every_form(keep, ref, what + " and tombstones")
        _search_i8(idx, qs, k, oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(~dead_all)), None, "tombstones alone")


def test_k_around_the_number_of_live_tiles(hip_lib, oracle_mod):
    """4 000 rows are 63 tiles; 23 whole tiles are deleted, 40 stay alive.  The threshold is the k-th smallest minimum of
    the LIVE tiles: k = 39 and 40 have one, k = 41 and 100 have none (every live row survives).  At most 4 000 rows
    survive, the list holds 4 096: nothing may be redone."""
    d, metric, n = 768, L2, 4000
    rng = np.random.default_rng(5)
    rows, qs = _corpus(rng, n, d, metric, nq=4)
    dead_tiles = np.sort(rng.choice(63, 23, replace=False))
    live = np.ones(n, bool)
    for t in dead_tiles:
        live[t * TILE:(t + 1) * TILE] = False
    assert sum(live[t * TILE:(t + 1) * TILE].any() for t in range(63)) == 40
    with _open(d, metric, rows) as idx:
        idx.set_deleted(np.nonzero(~live)[0])
        for k in (39, 40, 41, 100):
            ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(live))
            _search_i8(idx, qs, k, ref, None, "k=%d" % k)


@pytest.mark.parametrize("metric", [L2, COS])
def test_fewer_live_rows_than_k(hip_lib, oracle_mod, metric):
    """All but 5 rows deleted and k = 10: 5 entries; every row deleted: none.  tsh_search and the ticket form."""
    d, k = 768, 10
    rng = np.random.default_rng(61 + metric)
    rows, qs = _corpus(rng, N, d, metric, nq=4, oracle_mod=oracle_mod)
    live = np.zeros(N, bool)
    live[[3, 64 * 100 + 63, 64 * 101, 12_345, N - 1]] = True
    with _open(d, metric, rows) as idx:
        idx.set_deleted(np.nonzero(~live)[0])
        ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(live))
        assert np.all(ref[2] == 5)
        _search_i8(idx, qs, k, ref, None, "5 live rows")
        _tickets_i8(idx, qs, k, ref, None, "5 live rows, tickets")
        idx.set_deleted(np.nonzero(live)[0])
        ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(np.zeros(N, bool)))
        assert np.all(ref[2] == 0)
        _search_i8(idx, qs, k, ref, None, "no live row")
        _tickets_i8(idx, qs, k, ref, None, "no live row, tickets")


@pytest.mark.parametrize("metric", [L2, COS])
def test_not_all_live_without_deletes(hip_lib, oracle_mod, metric):
    d, k = 768, 25
    rng = np.random.default_rng(41 + metric)
    rows, qs = _corpus(rng, N, d, metric, nq=4, oracle_mod=oracle_mod)
    # a gap of absent ids: rows [0, a) and [b, N), nothing in between (a, b inside tiles)
    a, b = 6_000 + 21, 6_000 + 21 + 3 * TILE + 30
    present = np.ones(N, bool)
    present[a:b] = False
    ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(present))
    with _open(d, metric, rows[:a], capacity=N) as idx:
        idx.append(b, rows[b:])
        assert idx.size == N
        _search_i8(idx, qs, k, ref, None, "a gap of absent ids")
    # one quarantined row (an inf element): answered on the side where it belongs in the answer, the rest scans int8
    bad = rows.copy()
    bad[4_321, 5] = np.inf
    with _open(d, metric, bad) as idx:
        assert idx.counters()["quarantined_rows"] == 1
        _search_i8(idx, qs, k, oracle_mod.search_heap_many_mt(bad, qs, metric, k), None, "a quarantined row")
    # a shard handle of global ids under a global mask
    base = 1003
    keep = rng.random(N) < 0.6
    gmask = _bits(np.concatenate([rng.random(base) < 0.5, keep]))
    with _open(d, metric, rows, first=base, shard_device=0, row_base=base) as idx:
        _search_i8(idx, qs, k, oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(keep)), gmask, "a shard handle", base=base)


@pytest.mark.parametrize("form", ["pointer", "handle", "ticket"])
@pytest.mark.parametrize("metric", [L2, COS])
def test_redo_keeps_the_mask(hip_lib, oracle_mod, metric, form):
    """10 000 identical rows are the query's nearest and every second one, the lowest ids among them, is masked out: the
    5 000 kept twins overflow the survivor list (4 096), and the redo must look through the same mask.  A second such query
    in a row denies the route: a third does not scan the int8 copy."""
    d, k = 768, 100
    rng = np.random.default_rng(77 + metric)
    rows, qs = _corpus(rng, N, d, metric, nq=3, oracle_mod=oracle_mod)
    twin = (qs[0] + 0.05 * rng.standard_normal(d)).astype(np.float32)
    qs[1] = twin + 0.01 * rng.standard_normal(d).astype(np.float32)
    qs[2] = twin - 0.01 * rng.standard_normal(d).astype(np.float32)
    if metric == COS:
        qs = np.stack([oracle_mod.normalize_f32(q) for q in qs])
    where = np.sort(rng.choice(N, 10_000, replace=False))
    rows[where] = twin
    keep = np.ones(N, bool)
    keep[where[0::2]] = False
    mask = _bits(keep)
    ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, mask)
    assert np.array_equal(ref[0][0], where[1::2][:k])  # ties: the lowest KEPT ids first
    with _open(d, metric, rows) as idx:
        def one(i, m):
            if form == "ticket":
                ids, dist = idx.wait(idx.submit(qs[i], k, m))
                return ids[None, :], dist[None, :], np.array([len(ids)])
            return idx.search(qs[i:i + 1], k, None, m)

        def three(m):
            for i, (scans, redone) in enumerate(((1, 1), (2, 2), (2, 2))):  # (the third: denied, no int8 scan)
                got = one(i, m)
                st = idx.scan_i8_stats()
                assert not np.isin(got[0], where[0::2]).any(), "a masked-out row came back from the redo of query %d" % i
                _same(got, tuple(x[i:i + 1] for x in ref), "%s, query %d" % (form, i))
                assert st["scans"] == scans and st["redone"] == redone, (i, st)

        if form == "handle":
            with idx.make_mask(mask) as h:
                three(h)
        else:
            three(mask)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_band_under_masks(hip_lib, metric):
    """Rows at quantisation midpoints (test_gpu_scan_i8.py::test_band_probe_on_midpoint_rows) in a tombstoned shard:
    lower <= exact <= upper for every live row, both NaN for every dead one."""
    d, n = 768, 4096 + 29
    rng = np.random.default_rng(9000 + metric)
    q = rng.standard_normal(d).astype(np.float32)
    s0 = np.ldexp(1.0, -rng.integers(0, 12, size=n))[:, None]
    c = 2.0 * rng.integers(-63, 63, size=(n, d))
    rows = (c + np.where(q > 0, 0.5, -0.5)[None, :]) * s0
    rows[np.arange(n), np.arange(n) % d] = 127.0 * s0[:, 0]  # pins every row's scale to its s0
    rows = rows.astype(np.float32)
    r64, q64 = rows.astype(np.float64), q.astype(np.float64)
    dot, nrm2 = r64 @ q64, np.einsum("ij,ij->i", r64, r64)
    exact = nrm2 - 2.0 * dot if metric == L2 else (-dot if metric == IP else -dot / np.sqrt(nrm2))
    live = _edge_tombstones(rng, n, np.array([0, 63, 64]))
    with _open(d, metric, rows) as idx:
        idx.set_deleted(np.nonzero(~live)[0])
        lo, up = idx.probe_scan_i8_keys(q)
    lo, up = lo.astype(np.float64), up.astype(np.float64)
    assert np.all(np.isnan(lo[~live])) and np.all(np.isnan(up[~live])), "a dead row has a key"
    assert np.all(np.isfinite(lo[live])) and np.all(np.isfinite(up[live]))
    w = (up[live] - lo[live]) / 2
    ratio = np.abs((lo[live] + up[live]) / 2 - exact[live]) / w
    print("metric %d: max |key - exact| / w on live midpoint rows: %.4f" % (metric, ratio.max()))
    assert np.all(lo[live] <= exact[live]) and np.all(exact[live] <= up[live]), float(ratio.max())


def test_option_semantics(hip_lib, oracle_mod):
    d, k, metric = 768, 30, L2
    rng = np.random.default_rng(5)
    rows, qs = _corpus(rng, N, d, metric, nq=4)
    keep = rng.random(N) < 0.7
    mask = _bits(keep)
    ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, mask)
    with _open(d, metric, rows) as idx:
        _search_i8(idx, qs, k, ref, mask, "value 2")
        base = idx.scan_i8_stats()["scans"]
        cases = (("value 0", 1, 0, 1), ("value 1 on 61 MB of rows", 1, 1, 1), ("TSH_OPT_SCAN_I8 = 0 with value 2", 0, 2, 1),
                 ("TSH_OPT_SCAN_I8 = 2 with value 1", 2, 1, 1), ("value 1 with TSH_OPT_SCAN_F16_MASKED = 2", 1, 1, 2))
        for what, dense_mode, mode, f16_masked in cases:
            idx.set_scan_i8(dense_mode)
            idx.set_scan_i8_masked(mode)
            idx.set_scan_f16_masked(f16_masked)
            _same(idx.search(qs, k, None, mask), ref, what)
            assert idx.scan_i8_stats()["scans"] == base, what
        # a tombstoned small shard under TSH_OPT_SCAN_I8 = 2 and value 1 scans fp16 where that is forced, never int8
        idx.set_scan_i8(2)
        idx.set_scan_i8_masked(1)
        idx.set_scan_f16_masked(2)
        idx.set_deleted([7])
        live = np.ones(N, bool)
        live[7] = False
        f0 = idx.scan_f16_stats()["scans"]
        _same(idx.search(qs, k), oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(live)), "one tombstone")
        assert idx.scan_i8_stats()["scans"] == base and idx.scan_f16_stats()["scans"] - f0 == len(qs)
        # value 3 is refused and leaves the setting alone
        idx.set_scan_f16_masked(1)
        idx.set_scan_i8_masked(2)
        with pytest.raises(Exception):
            idx.set_scan_i8_masked(3)
        _search_i8(idx, qs, k, oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(keep & live)), mask, "value 2 after a refused 3")


def test_big_shard_launch_shapes(hip_lib, oracle_mod):
    """From 6144 tiles on a masked scan is launched in the dense scans' shape when it keeps most rows and as a grid of
    four-wave workgroups striding over the tiles when it does not: both, and the tombstone-only case, at the smallest
    such shard (d = 256: 403 MB of rows) -- forced (value 2) and by the automatic rule (value 1: above 256 MiB)."""
    d, k, metric = 256, 20, L2
    n = 6144 * TILE + 37
    rng = np.random.default_rng(17)
    rows, qs = _corpus(rng, n, d, metric, nq=4)
    with _open(d, metric, rows) as idx:
        for what, frac in (("keep 70 %", 0.7), ("keep 10 %", 0.1)):
            keep = rng.random(n) < frac
            keep[5 * TILE:9 * TILE] = False
            ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(keep))
            for mode in (2, 1):
                idx.set_scan_i8_masked(mode)
                _search_i8(idx, qs, k, ref, _bits(keep), "%s, value %d" % (what, mode))
        dead = np.unique(oracle_mod.search_heap_many_mt(rows, qs, metric, 2)[0])
        idx.set_deleted(dead)
        live = ~np.isin(np.arange(n), dead)
        ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(live))
        for mode in (2, 1):
            idx.set_scan_i8_masked(mode)
            _search_i8(idx, qs, k, ref, None, "tombstones, value %d" % mode)
