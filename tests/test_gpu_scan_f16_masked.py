"""GPU: tile scans that are NOT dense over the fp16 copy of the rows (TSH_OPT_SCAN_F16_MASKED, scan_f16_kernel<MASKED>).

Tombstones, quarantined rows, gaps of absent ids and caller masks too dense for the list scan used to send a shard's
single-query scans back to the f32 kernel at twice the HBM bytes.  The masked fp16 kernel loads the live rows' halves
only; its keys carry the same per-row band, the f64 re-rank decides, and a query whose candidate list overflows is redone
through the f32 scan BEHIND THE SAME MASK.  Every index here forces the route on small shapes (option value 2), switches
the exact path and the batched path off, and is held to the oracle: ids, counts and distance bits.  Unless a test says
otherwise every search must also have run over the fp16 copy (scan_f16_stats) with nothing redone."""
import numpy as np
import pytest

from test_gpu_bands import _exact_keys, _patterned

pytestmark = pytest.mark.gpu
L2, IP, COS = 0, 1, 2
N = 20_037  # 313 whole tiles and one of 5 rows
TILE = 64


def _open(d, metric, rows, capacity=None, mode=2, dense_mode=1, first=0, **kw):
    from tostore_amd import HipVectorIndex

    idx = HipVectorIndex(d, metric, capacity_rows=capacity or len(rows), **kw)
    idx.set_scan_f16(dense_mode)
    idx.set_scan_f16_masked(mode)
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


def _search_f16(idx, qs, k, ref, mask=None, what="", redone=0, base=0):
    """One call of len(qs) single-query searches: the oracle's answer, every scan over the fp16 copy."""
    s0 = idx.scan_f16_stats()
    _same(idx.search(qs, k, None, mask), ref, what, base)
    s1 = idx.scan_f16_stats()
    assert s1["scans"] - s0["scans"] == len(qs), (what, s0, s1)
    assert s1["redone"] - s0["redone"] == redone, (what, s0, s1)


def _tickets_f16(idx, qs, k, ref, mask=None, what="", redone=0):
    s0 = idx.scan_f16_stats()
    tickets = [idx.submit(q, k, mask) for q in qs]
    for i, t in enumerate(tickets):
        ids, dist = idx.wait(t)
        assert np.array_equal(ids, ref[0][i, :ref[2][i]]), (what, i)
        assert np.array_equal(dist.view(np.uint64), ref[1][i, :ref[2][i]].view(np.uint64)), (what, i)
    s1 = idx.scan_f16_stats()
    assert s1["scans"] - s0["scans"] == len(qs), (what, s0, s1)
    assert s1["redone"] - s0["redone"] == redone, (what, s0, s1)


def _edge_tombstones(rng, n, nearest):
    """live[] after: the queries' nearest rows, a random 5 %, one whole tile, all but one row of another, tiles left
    with 9 and with 57 live rows (a short last batch of one row each), every row of the last, partial tile."""
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
@pytest.mark.parametrize("d", [768, 1000, 1536])
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
            _search_f16(idx, qs, k, ref, None, "k=%d" % k)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_caller_masks(hip_lib, oracle_mod, metric):
    d, k = 768, 30
    rng = np.random.default_rng(300 + metric)
    rows, qs = _corpus(rng, N, d, metric, oracle_mod=oracle_mod)
    span = np.zeros(N, bool)
    span[1000 + 17:9000 + 45] = True  # one range that starts and ends inside a tile
    masks = {"keep 70 %": rng.random(N) < 0.7, "keep 10 %": rng.random(N) < 0.1, "one range": span}
    with _open(d, metric, rows) as idx:
        for what, keep in masks.items():
            ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(keep))
            _search_f16(idx, qs, k, ref, _bits(keep), what + ", pointer")
            with idx.make_mask(_bits(keep)) as h:
                _search_f16(idx, qs, k, ref, h, what + ", handle")
                _search_f16(idx, qs[:1], k, [r[:1] for r in ref], h, what + ", handle, a lone query")
                if what != "keep 70 %":
                    _tickets_f16(idx, qs, k, ref, h, what + ", handle, tickets")
            if what != "one range":
                _tickets_f16(idx, qs, k, ref, _bits(keep), what + ", pointer, tickets")
        # ... combined with tombstones: the nearest kept rows of every query die
        keep = masks["keep 70 %"]
        dead = np.unique(oracle_mod.search_heap_many_mt(rows, qs, metric, 3, None, _bits(keep))[0])
        idx.set_deleted(dead)
        both = keep.copy()
        both[dead] = False
        ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(both))
        _search_f16(idx, qs, k, ref, _bits(keep), "mask and tombstones, pointer")
        with idx.make_mask(_bits(keep)) as h:
            _search_f16(idx, qs, k, ref, h, "mask and tombstones, handle")
            _tickets_f16(idx, qs, k, ref, h, "mask and tombstones, handle, tickets")
        _tickets_f16(idx, qs, k, ref, _bits(keep), "mask and tombstones, pointer, tickets")
        _search_f16(idx, qs, k, oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(~np.isin(np.arange(N), dead))), None,
                    "tombstones alone")


def test_big_shard_launch_shapes(hip_lib, oracle_mod):
    """From 6144 tiles on a masked scan is launched in the dense scans' shape when it keeps most rows and as a grid of
    four-wave workgroups striding over the tiles when it does not: both, and the tombstone-only case, at the smallest
    such shard (d = 256: 403 MB of rows)."""
    d, k, metric = 256, 20, L2
    n = 6144 * TILE + 37
    rng = np.random.default_rng(17)
    rows, qs = _corpus(rng, n, d, metric, nq=4)
    with _open(d, metric, rows) as idx:
        for what, frac in (("keep 70 %", 0.7), ("keep 10 %", 0.1)):
            keep = rng.random(n) < frac
            keep[5 * TILE:9 * TILE] = False
            ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(keep))
            _search_f16(idx, qs, k, ref, _bits(keep), what)
        dead = np.unique(oracle_mod.search_heap_many_mt(rows, qs, metric, 2)[0])
        idx.set_deleted(dead)
        live = ~np.isin(np.arange(n), dead)
        _search_f16(idx, qs, k, oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(live)), None, "tombstones")


@pytest.mark.parametrize("metric", [L2, COS])
def test_row_with_a_wholly_empty_chunk(hip_lib, oracle_mod, metric):
    """d = 2120 is 530 groups of four elements: nine chunks per row, scanned by the kernels for ten (the widths come from
    a short list), so lanes 0-17 of chunk 8 hold data and chunk 9 none at all.  The f32 scan, the fp16 scan dense, and the
    fp16 scan with tombstones on both sides of a tile edge."""
    d, k = 2120, 10
    n = 64 * TILE + 37
    rng = np.random.default_rng(2120 + metric)
    rows, qs = _corpus(rng, n, d, metric, nq=4, oracle_mod=oracle_mod)
    ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k)
    with _open(d, metric, rows, mode=0, dense_mode=0) as idx:
        _same(idx.search(qs, k), ref, "f32")
        assert idx.scan_f16_stats()["scans"] == 0
    with _open(d, metric, rows, dense_mode=2) as idx:
        _search_f16(idx, qs, k, ref, None, "fp16, dense")
        dead = np.union1d(np.unique(ref[0][:, :2]), np.arange(3 * TILE - 2, 3 * TILE + 2))
        idx.set_deleted(dead)
        live = ~np.isin(np.arange(n), dead)
        _search_f16(idx, qs, k, oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(live)), None, "fp16, tombstones")


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
        _search_f16(idx, qs, k, ref, None, "a gap of absent ids")
    # one quarantined row (an inf element): re-ranked on the side, the rest scans fp16
    bad = rows.copy()
    bad[4_321, 5] = np.inf
    with _open(d, metric, bad) as idx:
        assert idx.counters()["quarantined_rows"] == 1
        _search_f16(idx, qs, k, oracle_mod.search_heap_many_mt(bad, qs, metric, k), None, "a quarantined row")
    # a shard handle of global ids under a global mask
    base = 1003
    keep = rng.random(N) < 0.6
    gmask = _bits(np.concatenate([rng.random(base) < 0.5, keep]))
    with _open(d, metric, rows, first=base, shard_device=0, row_base=base) as idx:
        _search_f16(idx, qs, k, oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(keep)), gmask, "a shard handle", base=base)


def test_copy_stays_current(hip_lib, oracle_mod):
    d, k, metric = 768, 20, L2
    rng = np.random.default_rng(53)
    n0 = 12_000
    rows, qs = _corpus(rng, N, d, metric, nq=4)
    with _open(d, metric, rows[:n0], capacity=N) as idx:
        dead = np.unique(oracle_mod.search_heap_many_mt(rows[:n0], qs, metric, 2)[0])
        idx.set_deleted(dead)
        live = ~np.isin(np.arange(N), dead)
        _search_f16(idx, qs, k, oracle_mod.search_heap_many_mt(rows[:n0], qs, metric, k, None, _bits(live[:n0])), None, "at first")
        assert idx.scan_f16_stats()["rows_converted"] == n0
        idx.append(n0, rows[n0:])  # past the watermark
        _search_f16(idx, qs, k, oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, _bits(live)), None, "after an append")
        assert idx.scan_f16_stats()["rows_converted"] == N  # the appended rows only


@pytest.mark.parametrize("form", ["pointer", "handle", "ticket"])
@pytest.mark.parametrize("metric", [L2, COS])
def test_redo_keeps_the_mask(hip_lib, oracle_mod, metric, form):
    """2 000 identical rows nearest the query overflow the fp16 candidate list; the f32 redo must look through the same
    mask: every second twin, the lowest ids among them, is masked out and must not come back."""
    d, k = 768, 100
    rng = np.random.default_rng(77 + metric)
    rows, qs = _corpus(rng, N, d, metric, nq=1, oracle_mod=oracle_mod)
    twin = (qs[0] + 0.05 * rng.standard_normal(d)).astype(np.float32)
    where = np.sort(rng.choice(N, 2000, replace=False))
    rows[where] = twin
    keep = np.ones(N, bool)
    keep[where[0::2]] = False
    mask = _bits(keep)
    ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, mask)
    assert np.array_equal(ref[0][0], where[1::2][:k])  # ties: the lowest KEPT ids first
    with _open(d, metric, rows) as idx:
        if form == "pointer":
            got = idx.search(qs, k, None, mask)
        elif form == "handle":
            with idx.make_mask(mask) as h:
                got = idx.search(qs, k, None, h)
        else:
            ids, dist = idx.wait(idx.submit(qs[0], k, mask))
            got = (ids[None, :], dist[None, :], np.array([len(ids)]))
        st = idx.scan_f16_stats()
    assert not np.isin(got[0], where[0::2]).any(), "a masked-out row came back from the f32 redo"
    _same(got, ref, form)
    assert st["scans"] == 1 and st["redone"] == 1, st


@pytest.mark.parametrize("metric", [L2, IP])
def test_band_under_masks(hip_lib, metric):
    """|stored key - w - exact| <= w for every live row of a tombstoned shard of rows at fp16 rounding midpoints; the
    key of every dead row is NaN."""
    d, n = 768, 4096 + 29
    rng = np.random.default_rng(9100 + metric)
    q = _patterned(rng, d, 2, up=False)
    base = np.stack([_patterned(rng, d, 2, up=bool(i & 1)) for i in range(n)])
    rows = base * np.ldexp(1.0, -rng.integers(0, 5, size=n)).astype(np.float32)[:, None]
    live = _edge_tombstones(rng, n, np.array([0, 63, 64]))
    qn2 = float(q.astype(np.float64) @ q.astype(np.float64))
    exact = _exact_keys(rows, q, metric) - (qn2 if metric == L2 else 0.0)
    with _open(d, metric, rows) as idx:
        idx.set_deleted(np.nonzero(~live)[0])
        up, w = idx.probe_scan_f16_keys(q)
    up, w = up.astype(np.float64), w.astype(np.float64)
    assert np.all(np.isnan(up[~live])), "a dead row has a key"
    assert np.all(np.isfinite(up[live])) and np.all(np.isfinite(w)) and np.all(w > 0)
    ratio = np.abs(up[live] - w[live] - exact[live]) / w[live]
    print("max |key - exact| / w on live patterned rows: %.4f" % ratio.max())
    assert ratio.max() <= 1.0, "a key is further from its exact value than its row's band: %.4f" % ratio.max()


def test_option_semantics(hip_lib, oracle_mod):
    d, k, metric = 768, 30, L2
    rng = np.random.default_rng(5)
    rows, qs = _corpus(rng, N, d, metric, nq=4)
    keep = rng.random(N) < 0.7
    mask = _bits(keep)
    ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, mask)
    with _open(d, metric, rows, dense_mode=2) as idx:
        _search_f16(idx, qs, k, ref, mask, "value 2")
        base = idx.scan_f16_stats()["scans"]
        for what, dense_mode, mode in (("value 0", 2, 0), ("value 1 on 61 MB of rows", 2, 1), ("TSH_OPT_SCAN_F16 = 0 with value 2", 0, 2)):
            idx.set_scan_f16(dense_mode)
            idx.set_scan_f16_masked(mode)
            _same(idx.search(qs, k, None, mask), ref, what)
            assert idx.scan_f16_stats()["scans"] == base, what
        idx.set_scan_f16(1)  # the dense route's own gate does not hold the masked one back, nor does its value 2 force it
        idx.set_scan_f16_masked(2)
        _search_f16(idx, qs, k, ref, mask, "value 2 under TSH_OPT_SCAN_F16 = 1")
        with pytest.raises(Exception):
            idx.set_scan_f16_masked(3)
