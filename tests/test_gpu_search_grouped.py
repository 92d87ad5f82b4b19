"""GPU: the nearest row of each of the k nearest groups (tsh_search_grouped, include/tostore_hip.h).  The oracle is
search_exhaustive(rows, q, metric, n, thr, keep) -- the list L a plain search would return with k = infinity -- and then,
in Python, the first entry of each group, cut to k.  Ids are compared with ==, distances as uint64 views, groups with ==."""
import math
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2
LAYOUTS = ("runs7", "random", "one", "ungrouped", "own", "mix")


def _query(rng, oracle_mod, d, metric):
    q = rng.standard_normal(d).astype(np.float32)
    return oracle_mod.normalize_f32(q) if metric == COS else q


def _layout(name, n, rng):
    """-> (group_of[n] int32, n_groups)"""
    if name == "runs7":  # runs of 7 consecutive rows: they straddle wave and tile edges
        return (np.arange(n) // 7).astype(np.int32), n // 7 + 1
    if name == "random":  # equal ids that are not adjacent inside a wave
        m = max(n // 5, 1)
        return rng.integers(0, m, n).astype(np.int32), m
    if name == "one":
        return np.full(n, 2, np.int32), 3
    if name == "ungrouped":
        return np.full(n, -1, np.int32), 1
    if name == "own":
        return np.arange(n, dtype=np.int32), n
    m = max(n // 9, 1)  # a mix with negatives
    g = rng.integers(0, m, n).astype(np.int32)
    neg = rng.random(n) < 0.3
    g[neg] = -rng.integers(1, 5, int(neg.sum())).astype(np.int32)
    return g, m


def _first_of_each_group(eids, edist, group_of, k, base=0):
    """The specification over an oracle list: (ids, dist, groups), ids global"""
    keep, groups, seen = [], [], set()
    for i, gid in enumerate(eids + base):
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
    return eids[keep] + base, edist[keep], np.asarray(groups, np.int32)


def _n_groups_in(eids, group_of, base=0):
    return len(_first_of_each_group(eids, np.zeros(len(eids)), group_of, len(eids) + 1, base)[0])


def _same(got, want, what):
    ids, dist, grp, cnt = got
    wi, wd, wg = want
    assert cnt[0] == len(wi), (what, int(cnt[0]), len(wi))
    c = int(cnt[0])
    assert np.array_equal(ids[0, :c], wi), (what, ids[0, :c][:12], wi[:12])
    assert np.array_equal(dist[0, :c].view(np.uint64), wd.view(np.uint64)), (what, dist[0, :c][:12], wd[:12])
    assert np.array_equal(grp[0, :c], wg), (what, grp[0, :c][:12], wg[:12])
    assert np.all(ids[0, c:] == -1) and np.all(np.isnan(dist[0, c:])) and np.all(grp[0, c:] == -1), what


def _check(idx, h, group_of, lst, q, ks, thr=None, mask=None, base=0, what=""):
    eids, edist = lst
    for k in ks:
        _same(idx.search_grouped(q, k, h, thr, mask), _first_of_each_group(eids, edist, group_of, k, base), (what, k, thr))


@pytest.mark.parametrize("metric", [L2, IP, COS])
@pytest.mark.parametrize("d", [4, 128, 257])
def test_grouped_equals_first_of_each_group(hip_lib, oracle_mod, metric, d):
    """Every shape x every layout x k in {1, 10, 100, groups + 5}, dense; "ungrouped" and "own group" held to tsh_search
    itself as well; then, for two layouts, behind a keep-50 % mask as pointer and as handle, "nothing kept", a keep-1 % mask
    at n = 5000 (the list scan), tombstones (a whole tile, the last row and the nearest group's head) and a gap of ids."""
    from tostore_amd import HipMask, HipVectorIndex

    rng = np.random.default_rng(7000 + 10 * d + metric)
    for n in (1, 63, 64, 65, 4097, 5000):
        rows = rng.standard_normal((n, d)).astype(np.float32)
        q = _query(rng, oracle_mod, d, metric)
        full = oracle_mod.search_exhaustive(rows, q, metric, n)
        with HipVectorIndex(d, metric, capacity_rows=n) as idx:
            idx.append(0, rows)
            for name in LAYOUTS:
                group_of, n_groups = _layout(name, n, rng)
                ks = (1, 10, 100, _n_groups_in(full[0], group_of) + 5)
                with idx.make_groups(group_of, n_groups) as h:
                    _check(idx, h, group_of, full, q, ks, what=(n, name))
                    if name in ("ungrouped", "own"):
                        for k in ks:
                            ids, dist, cnt = idx.search(q, k)
                            gi, gd, _, gc = idx.search_grouped(q, k, h)
                            assert gc[0] == cnt[0] and np.array_equal(gi, ids) and np.array_equal(gd.view(np.uint64), dist.view(np.uint64))
                    if name == "one":
                        gi, gd, gg, gc = idx.search_grouped(q, 10, h)
                        assert gc[0] == 1 and gi[0, 0] == full[0][0] and gg[0, 0] == 2
            for name in ("runs7", "mix"):
                group_of, n_groups = _layout(name, n, rng)
                with idx.make_groups(group_of, n_groups) as h:
                    kept = rng.random(n) < 0.5
                    if n == 1:
                        kept[:] = True
                    masks = [kept, np.zeros(n, bool)]
                    if n == 5000:
                        masks.append(rng.random(n) < 0.01)
                    for m in masks:
                        bits = np.packbits(m, bitorder="little")
                        lst = oracle_mod.search_exhaustive(rows, q, metric, n, None, bits)
                        c0 = idx.counters()
                        _check(idx, h, group_of, lst, q, (10, 100), mask=bits, what=(n, name, "pointer mask", int(m.sum())))
                        with HipMask(idx, bits) as mh:
                            _check(idx, h, group_of, lst, q, (10, 100), mask=mh, what=(n, name, "mask handle", int(m.sum())))
                        if n == 5000 and d == 257 and 0 < m.sum() < 100:  # (rows of 257 floats: a width the list scan serves)
                            assert idx.counters()["list_scans"] > c0["list_scans"]
            # tombstones: one whole tile, the last row and the head of the nearest group -- the group stays, represented by
            # its next row
            group_of, n_groups = _layout("runs7", n, rng)
            with idx.make_groups(group_of, n_groups) as h:
                t = 1 if n >= 129 else 0
                dead = sorted(set(range(64 * t, min(64 * t + 64, n))) | {n - 1, int(full[0][0])})
                idx.set_deleted(np.asarray(dead, np.int64))
                alive = np.ones(n, bool)
                alive[dead] = False
                lst = oracle_mod.search_exhaustive(rows, q, metric, n, None, np.packbits(alive, bitorder="little"))
                _check(idx, h, group_of, lst, q, (1, 10, 100), what=(n, "tombstones"))
                g0 = group_of[full[0][0]]
                if alive[group_of == g0].any() and not (64 * t <= full[0][0] < 64 * t + 64):
                    assert g0 in idx.search_grouped(q, n, h)[2][0]
        if n >= 65:  # a gap of absent ids
            a, b = n // 3 + 1, n // 3 + 1 + min(n // 4, 64 + 30)
            present = np.ones(n, bool)
            present[a:b] = False
            with HipVectorIndex(d, metric, capacity_rows=n) as idx:
                idx.append(0, rows[:a])
                idx.append(b, rows[b:])
                lst = oracle_mod.search_exhaustive(rows, q, metric, n, None, np.packbits(present, bitorder="little"))
                for name in ("runs7", "random"):
                    group_of, n_groups = _layout(name, n, rng)
                    with idx.make_groups(group_of, n_groups) as h:
                        _check(idx, h, group_of, lst, q, (10, 100), what=(n, name, "gap"))


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_thresholds(hip_lib, oracle_mod, metric):
    """Thresholds at and one ulp beside the k-th group's distance, and beside everything."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(31 + metric)
    n, d, k = 5000, 128, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    full = oracle_mod.search_exhaustive(rows, q, metric, n)
    with HipVectorIndex(d, metric, capacity_rows=n) as idx:
        idx.append(0, rows)
        for name in ("runs7", "random"):
            group_of, n_groups = _layout(name, n, rng)
            dk = float(_first_of_each_group(*full, group_of, k)[1][-1])
            with idx.make_groups(group_of, n_groups) as h:
                for thr in (dk, float(np.nextafter(dk, -np.inf)), float(np.nextafter(dk, np.inf)), math.inf, -math.inf, float(full[1][0])):
                    lst = oracle_mod.search_exhaustive(rows, q, metric, n, thr)
                    _check(idx, h, group_of, lst, q, (1, k, 100), thr=thr, what=(name, thr))


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_ties(hip_lib, oracle_mod, metric):
    """Rows of small integers at d = 4: exact ties inside groups and across groups, the id decides the head."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(41 + metric)
    d = 4
    for n in (65, 700, 5000):
        rows = rng.integers(-2, 3, (n, d)).astype(np.float32)
        q = rng.integers(-2, 3, d).astype(np.float32)
        if metric == COS:
            q = oracle_mod.normalize_f32(q + np.float32(0.25))
        with np.errstate(all="ignore"):
            full = oracle_mod.search_exhaustive(rows, q, metric, n)
        if n >= 700:  # (more rows than the 625 there can be: ties for certain)
            assert len(np.unique(full[1])) < len(full[1])
        with HipVectorIndex(d, metric, capacity_rows=n) as idx:
            idx.append(0, rows)
            for name in ("runs7", "random", "mix", "own"):
                group_of, n_groups = _layout(name, n, rng)
                with idx.make_groups(group_of, n_groups) as h:
                    _check(idx, h, group_of, full, q, (1, 10, 100, _n_groups_in(full[0], group_of) + 5), what=(n, name, "ties"))


def test_side_list_overflow_is_redone(hip_lib, oracle_mod):
    """One group of 3000 identical rows among 5000, nearest to the query: 2999 rows that are not the head but as near by
    key.  The side list (1024 rows) overflows, the job is redone with a larger one, stats [2] moves."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(51)
    n, d, k = 5000, 32, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    same = rng.choice(n, 3000, replace=False)
    rows[same] = q + np.float32(0.01)
    group_of = rng.integers(1, 400, n).astype(np.int32)
    group_of[same] = 0
    full = oracle_mod.search_exhaustive(rows, q, L2, n)
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        with idx.make_groups(group_of, 400) as h:
            s0 = idx.search_grouped_stats()
            _check(idx, h, group_of, full, q, (k,), what="side overflow")
            s1 = idx.search_grouped_stats()
            assert s1["redone"] - s0["redone"] == 1 and s1["side_rows"] - s0["side_rows"] >= 2999
            _check(idx, h, group_of, full, q, (k,), what="side overflow, again")  # (the context kept the larger list)
            assert idx.search_grouped_stats()["redone"] == s1["redone"]


def test_candidate_block_overflow_runs_the_wide_band_over_heads(hip_lib, oracle_mod):
    """600 groups with identical best distances at k = 100: more heads inside the band than the block holds."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(53)
    n, d, k = 5000, 32, 100
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    group_of = (np.arange(n) % 600).astype(np.int32)
    best = rng.permutation(n)[:1200]
    best = np.asarray([best[group_of[best] == g][0] for g in range(600) if (group_of[best] == g).any()])
    rows[best] = q + np.float32(0.01)
    full = oracle_mod.search_exhaustive(rows, q, L2, n)
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        with idx.make_groups(group_of, 600) as h:
            c0 = idx.counters()
            _check(idx, h, group_of, full, q, (k,), what="block overflow")
            assert idx.counters()["fallback_searches"] > c0["fallback_searches"]


def test_rows_outside_the_model_and_safe_mode(hip_lib, oracle_mod):
    """A quarantined row (an inf / 1e20 element) that is its group's best under inner product; then more than 1024 irregular
    rows: safe mode, no device group passes, stats [3] moves."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(57)
    n, d = 500, 32
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    rows[100, 3] = np.inf if q[3] > 0 else -np.inf  # inner product +inf: distance -inf, the best of everything
    rows[333, 7] = 1e20 if q[7] > 0 else -1e20      # a huge finite one: the best of its group
    group_of = (np.arange(n) // 7).astype(np.int32)
    with np.errstate(all="ignore"):
        full = oracle_mod.search_exhaustive(rows, q, IP, n)
    assert full[0][0] == 100 and full[0][1] == 333
    with HipVectorIndex(d, IP, capacity_rows=n) as idx:
        idx.append(0, rows)
        assert idx.counters()["quarantined_rows"] == 2 and not idx.counters()["safe_mode"]
        with idx.make_groups(group_of, n) as h:
            _check(idx, h, group_of, full, q, (1, 2, 10, 100), what="quarantined")
            ids = idx.search_grouped(q, 10, h)[0][0]
            assert ids[0] == 100 and ids[1] == 333
    n, d = 2048, 8
    rows = rng.standard_normal((n, d)).astype(np.float32)
    bad = rng.choice(n, 1100, replace=False)
    rows[bad[:550], 2] = np.inf
    rows[bad[550:], 6] = np.nan
    q = rng.standard_normal(d).astype(np.float32)
    group_of = rng.integers(-1, 300, n).astype(np.int32)
    with np.errstate(all="ignore"):
        full = oracle_mod.search_exhaustive(rows, q, L2, n)
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        assert idx.counters()["safe_mode"]
        with idx.make_groups(group_of, 300) as h:
            s0 = idx.search_grouped_stats()
            _check(idx, h, group_of, full, q, (1, 10, 100), what="safe mode")
            s1 = idx.search_grouped_stats()
            assert s1["no_device_passes"] - s0["no_device_passes"] == s1["searches"] - s0["searches"] == 3
            assert s1["side_rows"] == s0["side_rows"]


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_several_devices_and_shard_handles(hip_lib, oracle_mod, metric, monkeypatch):
    """A handle over two devices that share a GPU, groups spanning the shards; a shard handle whose row_base is not a
    multiple of 64 answers for its own rows, and the ranks' answers merge to the whole index's."""
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(61 + metric)
    n, d = 3000, 40
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[1500:1600] = rows[100]  # ties across shards
    q = _query(rng, oracle_mod, d, metric)
    group_of = rng.integers(0, 500, n).astype(np.int32)  # every group has rows on both shards
    group_of[rng.random(n) < 0.1] = -1
    full = oracle_mod.search_exhaustive(rows, q, metric, n)
    bits = np.packbits(rng.random(n) < 0.5, bitorder="little")
    masked = oracle_mod.search_exhaustive(rows, q, metric, n, None, bits)
    monkeypatch.setenv("TSH_SHARDS_SHARE_DEVICES", "1")
    _ffi.enable_test_hooks()
    try:
        with HipVectorIndex(d, metric, capacity_rows=n, n_devices=2) as idx:
            idx.append(0, rows)
            with idx.make_groups(group_of, 500) as h:
                _check(idx, h, group_of, full, q, (1, 10, 100, 520), what="two devices")
                _check(idx, h, group_of, masked, q, (10, 100), mask=bits, what="two devices, masked")
    finally:
        _ffi.enable_test_hooks(False)
    cut = 1237
    with HipVectorIndex(d, metric, capacity_rows=cut, shard_device=0, row_base=0) as lo, \
            HipVectorIndex(d, metric, capacity_rows=n - cut, shard_device=0, row_base=cut) as hi:
        lo.append(0, rows[:cut])
        hi.append(cut, rows[cut:])
        with lo.make_groups(group_of, 500) as h_lo, hi.make_groups(group_of, 500) as h_hi:
            for k in (1, 10, 100):
                for lst, m in ((full, None), (masked, bits)):
                    parts = []
                    for idx, h, sel in ((lo, h_lo, lst[0] < cut), (hi, h_hi, lst[0] >= cut)):
                        got = idx.search_grouped(q, k, h, None, m)
                        _same(got, _first_of_each_group(lst[0][sel], lst[1][sel], group_of, k), ("shard handle", k))
                        c = int(got[3][0])
                        parts.append((got[0][0, :c], got[1][0, :c]))
                    # the ranks' answers: concatenated, ordered, repeated groups dropped, cut to k
                    ids = np.concatenate([p[0] for p in parts])
                    dist = np.concatenate([p[1] for p in parts])
                    pos = {int(i): r for r, i in enumerate(lst[0])}  # (the oracle's order IS (compareTo(distance), id))
                    order = sorted(range(len(ids)), key=lambda i: pos[int(ids[i])])
                    merged = _first_of_each_group(ids[order], dist[order], group_of, k)
                    want = _first_of_each_group(lst[0], lst[1], group_of, k)
                    assert np.array_equal(merged[0], want[0]) and np.array_equal(merged[1].view(np.uint64), want[1].view(np.uint64))


def test_many_queries_threads_and_launch_counters(hip_lib, oracle_mod):
    """Eight queries in one call equal eight calls and never take the batched path; four threads share one groups handle;
    a plain search and a count behind grouped searches still equal the oracle (the side list's words are left clean)."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(67)
    n, d, k = 5000, 128, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((8, d)).astype(np.float32)
    group_of = (np.arange(n) // 7).astype(np.int32)
    want = [_first_of_each_group(*oracle_mod.search_exhaustive(rows, qs[i], L2, n), group_of, k) for i in range(8)]
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        idx.set_batch_min_nq(2)  # (the batched path would take an 8-query tsh_search)
        with idx.make_groups(group_of, n // 7 + 1) as h:
            c0, s0 = idx.counters(), idx.search_grouped_stats()
            ids, dist, grp, cnt = idx.search_grouped(qs, k, h)
            c1 = idx.counters()
            assert c1["batch_launches"] == c0["batch_launches"] and c1["exact_scans"] == c0["exact_scans"]
            assert c1["scan_launches"] - c0["scan_launches"] == 8 and c1["searches"] - c0["searches"] == 8
            assert idx.search_grouped_stats()["searches"] - s0["searches"] == 8
            for i in range(8):
                _same((ids[i:i + 1], dist[i:i + 1], grp[i:i + 1], cnt[i:i + 1]), want[i], ("one call", i))
                _same(idx.search_grouped(qs[i], k, h), want[i], ("eight calls", i))
            errors = []

            def worker(t):
                try:
                    for r in range(6):
                        i = (t * 2 + r) % 8
                        _same(idx.search_grouped(qs[i], k, h), want[i], ("thread", t, i))
                except Exception as e:  # noqa: BLE001
                    errors.append(e)

            threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            assert not errors, errors
            eids, edist = oracle_mod.search_exhaustive(rows, qs[0], L2, k)
            i2, d2, c2 = idx.search(qs[0], k)
            assert c2[0] == k and np.array_equal(i2[0], eids) and np.array_equal(d2[0].view(np.uint64), edist.view(np.uint64))
            thr = float(edist[-1])
            assert int(idx.search_count(qs[0], thr)[0]) == k


def test_groups_set_after_an_append_and_a_handle_that_outlives_its_index(hip_lib, oracle_mod):
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(71)
    n, d, k = 1000, 16, 10
    rows = rng.standard_normal((2 * n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    group_of = np.concatenate([(np.arange(n) // 7), (np.arange(n) // 3)]).astype(np.int32)
    idx = HipVectorIndex(d, L2)
    idx.append(0, rows[:n])
    h = idx.make_groups(group_of[:n], n)
    _check(idx, h, group_of[:n], oracle_mod.search_exhaustive(rows[:n], q, L2, n), q, (k, 100), what="before the append")
    idx.append(n, rows[n:])
    full = oracle_mod.search_exhaustive(rows, q, L2, 2 * n)
    _check(idx, h, group_of[:n], full, q, (k, 100), what="appended rows are ungrouped until they are set")
    h.set(n, group_of[n:])
    _check(idx, h, group_of, full, q, (k, 100), what="after set")
    over = group_of.copy()
    over[:50] = 5  # overwrite: the first fifty rows become one group
    h.set(0, over[:50])
    _check(idx, h, over, full, q, (k, 100), what="after an overwrite")
    with pytest.raises(_ffi.TshError, match="n_groups"):
        h.set(0, np.array([n], np.int32))
    # the Python index closes its groups with itself: the raw handle is kept alive past the index here
    idx._live_masks().discard(h)
    raw = h.handle()
    idx.close()
    g = np.zeros(4, np.int32)
    assert _ffi.lib().tsh_groups_set(raw, 0, 4, g.ctypes.data_as(_ffi.p_i32)) == _ffi.TSH_E_BAD_ARG
    assert "destroyed" in _ffi.last_error()
    with HipVectorIndex(d, L2) as other:
        other.append(0, rows[:n])
        with pytest.raises(_ffi.TshError, match="another index"):
            other.search_grouped(q, k, h)
    h.close()  # frees only the handle


def test_trivial_cases_and_the_manager(hip_lib, oracle_mod):
    from tostore_amd import HipVectorIndex, VectorIndexManager

    with HipVectorIndex(4, L2) as idx:
        with idx.make_groups(np.zeros(0, np.int32), 0) as h:
            ids, dist, grp, cnt = idx.search_grouped(np.zeros(4, np.float32), 5, h)
            assert cnt[0] == 0 and np.all(ids == -1)  # an empty index
        idx.append(0, np.eye(4, dtype=np.float32))
        with idx.make_groups([0, 0, 1, 1], 2) as h:
            assert idx.search_grouped(np.zeros(4, np.float32), 0, h)[3][0] == 0  # k <= 0
    m = VectorIndexManager(4, L2)
    try:
        vecs = [[1, 0, 0, 0], [0.9, 0, 0, 0], [0, 1, 0, 0], [0, 0.5, 0, 0], [0, 0, 1, 0]]
        m.insert_batch(["a1", "a2", "b1", "b2", "c1"], vecs)
        with m.index.make_groups([0, 0, 1, 1, -1], 2) as h:
            res = m.vectorSearch([1, 0.6, 0, 0], topK=3, group_by=h)
            assert [r.primaryKey for r in res] == ["a1", "b2", "c1"]
            plain = m.vectorSearch([1, 0.6, 0, 0], topK=5)
            firsts = {}
            for r in plain:
                firsts.setdefault(r.primaryKey[0], r.primaryKey)
            assert [r.primaryKey for r in res] == list(firsts.values())[:3]
            with pytest.raises(ValueError):
                m.vectorSearch([1, 0, 0, 0], topK=3, group_by=h, after=(0.0, 0))
    finally:
        m.close()
