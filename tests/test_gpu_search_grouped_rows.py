"""GPU: the m nearest rows of each of the k nearest groups (tsh_search_grouped_rows, include/tostore_hip.h).  The oracle
is search_exhaustive(rows, q, metric, n, thr, keep) -- the list L a plain search would return with k = infinity -- cut in
Python exactly as the specification reads: the winning groups are the groups of the first k entries of "L without entries
whose group occurred earlier"; of each, the first m entries of L that belong to it.  Ids are compared with ==, distances as
uint64 views, groups, rows and counts with ==, unused slots included."""
import math
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2
LAYOUTS = ("runs7", "random", "one", "ungrouped", "own", "mix")
MS = (1, 2, 3, 64)


def _query(rng, oracle_mod, d, metric):
    q = rng.standard_normal(d).astype(np.float32)
    return oracle_mod.normalize_f32(q) if metric == COS else q


def _layout(name, n, rng):
    """-> (group_of[n] int32, n_groups)"""
    if name == "runs7":  # runs of 7 consecutive rows: they straddle wave, tile and workgroup edges
        return (np.arange(n) // 7).astype(np.int32), n // 7 + 1
    if name == "random":  # equal ids that are not adjacent inside a wave, groups scattered across tiles
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


def _spec(lst, group_of, k, m, base=0):
    """The specification over an oracle list -> (ids[k, m], dist[k, m], group[k], rows[k], count), ids global"""
    eids, edist = lst
    gids = np.asarray(eids, np.int64) + base
    table = np.asarray(group_of, np.int64)
    g = np.full(len(gids), -1, np.int64)
    inside = gids < len(table)
    g[inside] = np.maximum(table[gids[inside]], -1)
    # G: L without entries whose group occurred earlier; its first k entries name the winners
    grouped = np.flatnonzero(g >= 0)
    _, first = np.unique(g[grouped], return_index=True)
    in_G = np.sort(np.concatenate([np.flatnonzero(g < 0), grouped[first]]))[:k]
    ids = np.full((k, m), -1, np.int64)
    dist = np.full((k, m), np.nan)
    grp = np.full(k, -1, np.int32)
    rows = np.zeros(k, np.int32)
    for w, p in enumerate(in_G):
        mine = np.flatnonzero(g == g[p])[:m] if g[p] >= 0 else np.asarray([p])  # the first m entries of L of that group
        ids[w, :len(mine)] = gids[mine]
        dist[w, :len(mine)] = edist[mine]
        grp[w] = g[p]
        rows[w] = len(mine)
    return ids, dist, grp, rows, len(in_G)


def _n_groups_in(lst, group_of, base=0):
    return _spec(lst, group_of, len(lst[0]) + 1, 1, base)[4]


def _same(got, want, what, q=0):
    ids, dist, grp, rows, cnt = got
    wi, wd, wg, wr, wc = want
    assert cnt[q] == wc, (what, int(cnt[q]), wc)
    assert np.array_equal(grp[q], wg), (what, grp[q][:12], wg[:12])
    assert np.array_equal(rows[q], wr), (what, rows[q][:12], wr[:12])
    assert np.array_equal(ids[q], wi), (what, ids[q][:4], wi[:4])
    assert np.array_equal(dist[q].view(np.uint64), wd.view(np.uint64)), (what, dist[q][:4], wd[:4])  # (one NaN: the unused slots' own)


def _check(idx, h, group_of, lst, q, ks, ms=MS, thr=None, mask=None, base=0, what=""):
    for k in ks:
        for m in ms:
            _same(idx.search_grouped_rows(q, k, m, h, thr, mask), _spec(lst, group_of, k, m, base), (what, k, m, thr))


def test_the_unused_slots_nan_is_the_oracle_sides_nan():
    """_same compares distances as bits: the NaN the library writes into unused slots must be numpy's default NaN."""
    assert np.array([math.nan]).view(np.uint64)[0] == np.full(1, np.nan).view(np.uint64)[0] == 0x7FF8000000000000


@pytest.mark.parametrize("metric", [L2, IP, COS])
@pytest.mark.parametrize("d", [1, 128])
def test_rows_of_groups_equal_the_specification(hip_lib, oracle_mod, metric, d):
    """Rows at the tile (64) and workgroup (256) edges x every layout x k in {1, 10, groups + 5} x m in {1, 2, 3, 64},
    and the identities: m = 1 is search_grouped bit for bit, one group is search cut to m, ungrouped rows and rows that
    are their own group are search with one row per group."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(9000 + 10 * d + metric)
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        rows = rng.standard_normal((n, d)).astype(np.float32)
        q = _query(rng, oracle_mod, d, metric)
        full = oracle_mod.search_exhaustive(rows, q, metric, n)
        with HipVectorIndex(d, metric, capacity_rows=n) as idx:
            idx.append(0, rows)
            for name in LAYOUTS:
                group_of, n_groups = _layout(name, n, rng)
                ks = (1, 10, _n_groups_in(full, group_of) + 5)
                with idx.make_groups(group_of, n_groups) as h:
                    _check(idx, h, group_of, full, q, ks, what=(n, name))
                    for k in ks:
                        gi, gd, gg, gc = idx.search_grouped(q, k, h)
                        ri, rd, rg, rr, rc = idx.search_grouped_rows(q, k, 1, h)
                        assert np.array_equal(rc, gc) and np.array_equal(ri[:, :, 0], gi) and np.array_equal(rg, gg)
                        assert np.array_equal(rd[:, :, 0].view(np.uint64), gd.view(np.uint64))
                        assert np.array_equal(rr[0], (np.arange(k) < gc[0]).astype(np.int32))
                    if name == "one":
                        for m in MS:
                            ids, dist, cnt = idx.search(q, m)
                            ri, rd, rg, rr, rc = idx.search_grouped_rows(q, 10, m, h)
                            assert rc[0] == 1 and rr[0, 0] == cnt[0] and rg[0, 0] == 2
                            c = int(cnt[0])
                            assert np.array_equal(ri[0, 0, :c], ids[0, :c]) and np.array_equal(rd[0, 0, :c].view(np.uint64), dist[0, :c].view(np.uint64))
                    if name in ("ungrouped", "own"):
                        for k in ks:
                            ids, dist, cnt = idx.search(q, k)
                            ri, rd, rg, rr, rc = idx.search_grouped_rows(q, k, 3, h)
                            assert rc[0] == cnt[0] and np.array_equal(ri[:, :, 0], ids) and np.array_equal(rd[:, :, 0].view(np.uint64), dist.view(np.uint64))
                            assert np.all(ri[:, :, 1:] == -1) and np.all(rr[0, :cnt[0]] == 1)


def test_rows_of_768_floats(hip_lib, oracle_mod):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(9768)
    n, d = 1000, 768
    rows = rng.standard_normal((n, d)).astype(np.float32)
    for metric in (L2, IP, COS):
        q = _query(rng, oracle_mod, d, metric)
        full = oracle_mod.search_exhaustive(rows, q, metric, n)
        with HipVectorIndex(d, metric, capacity_rows=n) as idx:
            idx.append(0, rows)
            for name in ("runs7", "random", "mix"):
                group_of, n_groups = _layout(name, n, rng)
                with idx.make_groups(group_of, n_groups) as h:
                    _check(idx, h, group_of, full, q, (1, 10, _n_groups_in(full, group_of) + 5), what=(768, metric, name))


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_thresholds_that_cut_inside_a_winning_group(hip_lib, oracle_mod, metric):
    """Thresholds at and one ulp beside the distance of a winning group's second and last returned row, and beside
    everything: the group keeps the rows at or below the threshold, and stays a winner through its first row alone."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(131 + metric)
    n, d, k, m = 1000, 128, 10, 3
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    full = oracle_mod.search_exhaustive(rows, q, metric, n)
    with HipVectorIndex(d, metric, capacity_rows=n) as idx:
        idx.append(0, rows)
        for name in ("runs7", "random"):
            group_of, n_groups = _layout(name, n, rng)
            free = _spec(full, group_of, k, m)
            full_groups = np.flatnonzero(free[3] == m)  # winners that hold m rows: the thresholds cut inside them
            assert len(full_groups) >= 2
            a, b = int(full_groups[0]), int(full_groups[-1])
            cuts = [float(free[1][a, 1]), float(free[1][a, 2]), float(free[1][b, 1]), float(free[1][k - 1, 0])]
            with idx.make_groups(group_of, n_groups) as h:
                for c in cuts:
                    for thr in (c, float(np.nextafter(c, -np.inf)), float(np.nextafter(c, np.inf))):
                        lst = oracle_mod.search_exhaustive(rows, q, metric, n, thr)
                        _check(idx, h, group_of, lst, q, (1, k, 200), ms=(1, m, 64), thr=thr, what=(name, thr))
                for thr in (math.inf, -math.inf, float(full[1][0])):
                    lst = oracle_mod.search_exhaustive(rows, q, metric, n, thr)
                    _check(idx, h, group_of, lst, q, (k,), ms=(m,), thr=thr, what=(name, thr))


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_masks_and_tombstones(hip_lib, oracle_mod, metric):
    """A keep-50 % mask as pointer and as handle, "nothing kept", a keep-1 % mask that takes the list scan (its positions
    map through the list); tombstones over a whole tile, on the nearest group's head, and on all but one row of the nearest
    group, which then returns fewer than m rows; a gap of absent ids."""
    from tostore_amd import HipMask, HipVectorIndex

    rng = np.random.default_rng(171 + metric)
    n, d = 5000, 257  # (4096 rows and more, rows of 257 floats: where the list scan serves)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    full = oracle_mod.search_exhaustive(rows, q, metric, n)
    with HipVectorIndex(d, metric, capacity_rows=n) as idx:
        idx.append(0, rows)
        for name in ("runs7", "mix"):
            group_of, n_groups = _layout(name, n, rng)
            with idx.make_groups(group_of, n_groups) as h:
                for kept in (rng.random(n) < 0.5, np.zeros(n, bool), rng.random(n) < 0.01):
                    bits = np.packbits(kept, bitorder="little")
                    lst = oracle_mod.search_exhaustive(rows, q, metric, n, None, bits)
                    c0 = idx.counters()
                    _check(idx, h, group_of, lst, q, (10, 100), ms=(2, 64), mask=bits, what=(name, "pointer mask", int(kept.sum())))
                    with HipMask(idx, bits) as mh:
                        _check(idx, h, group_of, lst, q, (10, 100), ms=(2, 64), mask=mh, what=(name, "mask handle", int(kept.sum())))
                    if 0 < kept.sum() < 100:
                        assert idx.counters()["list_scans"] > c0["list_scans"]
        group_of, n_groups = _layout("runs7", n, rng)
        with idx.make_groups(group_of, n_groups) as h:
            head = int(full[0][0])
            g0 = group_of[head]
            second = -1
            for cand in _spec(full, group_of, 10, 1)[0][1:, 0]:  # a winner whose rows the tombstones below do not touch otherwise
                members = np.flatnonzero(group_of == group_of[cand])
                if members.min() >= 128 and members.max() < n - 1:
                    second = int(cand)
                    break
            assert second >= 0
            others = [int(i) for i in np.flatnonzero(group_of == group_of[second]) if i != second]
            dead = sorted(set(range(64, 128)) | {n - 1, head} | set(others))
            idx.set_deleted(np.asarray(dead, np.int64))
            alive = np.ones(n, bool)
            alive[dead] = False
            lst = oracle_mod.search_exhaustive(rows, q, metric, n, None, np.packbits(alive, bitorder="little"))
            _check(idx, h, group_of, lst, q, (1, 10, 100), what="tombstones")
            got = idx.search_grouped_rows(q, 10, 3, h)
            w = list(got[2][0]).index(group_of[second])
            assert got[3][0, w] == 1  # the group whose other rows are gone gives the one it has
            if not 64 <= head < 128 and alive[group_of == g0].any():
                every = idx.search_grouped_rows(q, _n_groups_in(lst, group_of) + 5, 3, h)
                w = list(every[2][0]).index(g0)  # the group whose head is gone stays, through its other rows
                assert head not in every[0][0] and every[3][0, w] == min(3, int(alive[group_of == g0].sum()))
    a, b = n // 3 + 1, n // 3 + 95  # a gap of absent ids
    present = np.ones(n, bool)
    present[a:b] = False
    with HipVectorIndex(d, metric, capacity_rows=n) as idx:
        idx.append(0, rows[:a])
        idx.append(b, rows[b:])
        lst = oracle_mod.search_exhaustive(rows, q, metric, n, None, np.packbits(present, bitorder="little"))
        group_of, n_groups = _layout("random", n, rng)
        with idx.make_groups(group_of, n_groups) as h:
            _check(idx, h, group_of, lst, q, (10, 100), ms=(3,), what="gap")


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_ties(hip_lib, oracle_mod, metric):
    """Rows of small integers at d = 4: exact ties inside groups and across groups, the id decides."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(141 + metric)
    d = 4
    for n in (65, 700):
        rows = rng.integers(-2, 3, (n, d)).astype(np.float32)
        q = rng.integers(-2, 3, d).astype(np.float32)
        if metric == COS:
            q = oracle_mod.normalize_f32(q + np.float32(0.25))
        with np.errstate(all="ignore"):
            full = oracle_mod.search_exhaustive(rows, q, metric, n)
        with HipVectorIndex(d, metric, capacity_rows=n) as idx:
            idx.append(0, rows)
            for name in ("runs7", "random", "mix"):
                group_of, n_groups = _layout(name, n, rng)
                with idx.make_groups(group_of, n_groups) as h:
                    _check(idx, h, group_of, full, q, (1, 10, _n_groups_in(full, group_of) + 5), what=(n, name, "ties"))


def test_duplicates_overflow_the_side_list_and_are_redone_once(hip_lib, oracle_mod):
    """One group of 3000 identical rows among 5000, nearest to the query: its second-smallest key is every one's key, so all
    3000 are members.  The side list (2048 rows at k = 10, m = 2) overflows, the job is redone once with a larger one,
    stats "redone" moves by one and not again on the next job."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(151)
    n, d, k, m = 5000, 32, 10, 2
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
            s0, g0 = idx.search_grouped_rows_stats(), idx.search_grouped_stats()
            _check(idx, h, group_of, full, q, (k,), ms=(m,), what="side overflow")
            s1 = idx.search_grouped_rows_stats()
            assert s1["redone"] - s0["redone"] == 1 and s1["member_rows"] - s0["member_rows"] >= 3000 and s1["exact_all"] == s0["exact_all"]
            assert s1["searches"] - s0["searches"] == 1 and s1["marked_groups"] - s0["marked_groups"] >= k
            _check(idx, h, group_of, full, q, (k,), ms=(m,), what="side overflow, again")  # (the context kept the larger list)
            assert idx.search_grouped_rows_stats()["redone"] == s1["redone"]
            assert idx.search_grouped_stats() == g0  # these jobs move none of the grouped searches' counters
            want = _spec(full, group_of, k, 1)
            gi, gd, gg, gc = idx.search_grouped(q, k, h)  # a plain grouped job right behind
            assert gc[0] == want[4] and np.array_equal(gi[0], want[0][:, 0]) and idx.search_grouped_stats()["redone"] == g0["redone"]


def test_a_group_larger_than_the_member_segments_is_redone_once(hip_lib, oracle_mod):
    """One group holding all of 9000 rows: more members than the segment space of a fresh context (8192 rows).  The job is
    redone once with room for the count the first run left; the answer is search cut to m."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(153)
    n, d = 9000, 8
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    group_of = np.zeros(n, np.int32)
    full = oracle_mod.search_exhaustive(rows, q, L2, n)
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        with idx.make_groups(group_of, 1) as h:
            s0 = idx.search_grouped_rows_stats()
            _check(idx, h, group_of, full, q, (3,), ms=(3,), what="segment overflow")
            s1 = idx.search_grouped_rows_stats()
            assert s1["redone"] - s0["redone"] == 1 and s1["exact_all"] == s0["exact_all"] and s1["marked_groups"] - s0["marked_groups"] == 1
            _check(idx, h, group_of, full, q, (3,), ms=(64,), what="segment overflow, again")
            assert idx.search_grouped_rows_stats()["redone"] == s1["redone"]


def test_heads_tied_at_tau_overflow_the_slots_and_take_the_exact_all_route(hip_lib, oracle_mod):
    """600 identical rows in 200 groups, nearest to the query, k = 5, m = 2: every head ties at tau, 200 marked groups
    against 74 slots.  The job runs again on the exact-all route, counted, and the answer is right."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(155)
    n, d, k, m = 1000, 32, 5, 2
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    rows[:600] = q + np.float32(0.01)
    group_of = np.concatenate([rng.permutation(600) % 200, 200 + np.arange(400) // 3]).astype(np.int32)
    full = oracle_mod.search_exhaustive(rows, q, L2, n)
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        with idx.make_groups(group_of, 400) as h:
            s0 = idx.search_grouped_rows_stats()
            _check(idx, h, group_of, full, q, (k,), ms=(m,), what="slot overflow")
            s1 = idx.search_grouped_rows_stats()
            assert s1["exact_all"] - s0["exact_all"] == 1 and s1["redone"] - s0["redone"] == 1 and s1["searches"] - s0["searches"] == 1
            assert s1["marked_groups"] - s0["marked_groups"] >= 200
            # k = 150: 364 slots hold all of the 334 groups whatever the select's bound, the device passes answer
            _check(idx, h, group_of, full, q, (150,), ms=(m,), what="slots suffice")
            s2 = idx.search_grouped_rows_stats()
            assert s2["exact_all"] == s1["exact_all"] and s2["redone"] == s1["redone"]


def test_candidate_block_overflow_runs_the_wide_band_over_heads(hip_lib, oracle_mod):
    """600 groups with identical best distances at k = 100: more heads inside the band than the block holds; 600 marked
    groups against 264 slots on top."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(157)
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
            _check(idx, h, group_of, full, q, (k,), ms=(3,), what="block overflow")
            assert idx.counters()["fallback_searches"] > c0["fallback_searches"]
            _check(idx, h, group_of, full, q, (400,), ms=(3,), what="block overflow, slots suffice")


def test_rows_outside_the_model_and_safe_mode(hip_lib, oracle_mod):
    """A quarantined row (an inf / 1e20 element) inside a winning group, and as a group's only good row: the exact-all
    route, "exact_all" moves with every job.  Then more than 1024 irregular rows: safe mode, the same route."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(159)
    n, d = 500, 32
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    group_of = (np.arange(n) // 7).astype(np.int32)
    near = np.flatnonzero(group_of == group_of[100])
    rows[near] = q * np.float32(3.0) + rng.standard_normal((len(near), d)).astype(np.float32) * np.float32(0.01)  # a winning group ...
    rows[100, 3] = np.inf if q[3] > 0 else -np.inf  # ... with a row of inner product +inf: distance -inf, the best of everything
    rows[333, 7] = 1e20 if q[7] > 0 else -1e20      # a huge finite one: its group's only good row
    with np.errstate(all="ignore"):
        full = oracle_mod.search_exhaustive(rows, q, IP, n)
    assert full[0][0] == 100 and full[0][1] == 333
    with HipVectorIndex(d, IP, capacity_rows=n) as idx:
        idx.append(0, rows)
        assert idx.counters()["quarantined_rows"] == 2 and not idx.counters()["safe_mode"]
        with idx.make_groups(group_of, n) as h:
            s0 = idx.search_grouped_rows_stats()
            _check(idx, h, group_of, full, q, (1, 2, 10, 100), ms=(1, 3, 64), what="quarantined")
            s1 = idx.search_grouped_rows_stats()
            assert s1["exact_all"] - s0["exact_all"] == s1["searches"] - s0["searches"] == 12 and s1["member_rows"] == s0["member_rows"]
            got = idx.search_grouped_rows(q, 2, 3, h)
            assert got[0][0, 0, 0] == 100 and got[3][0, 0] == 3 and got[0][0, 1, 0] == 333
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
            s0, g0 = idx.search_grouped_rows_stats(), idx.search_grouped_stats()
            _check(idx, h, group_of, full, q, (1, 10, 100), ms=(2,), what="safe mode")
            s1 = idx.search_grouped_rows_stats()
            assert s1["exact_all"] - s0["exact_all"] == s1["searches"] - s0["searches"] == 3 and s1["redone"] == s0["redone"]
            assert idx.search_grouped_stats() == g0


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_several_devices_and_shard_handles(hip_lib, oracle_mod, metric, monkeypatch):
    """A handle over two devices that share a GPU.  Groups spanning the cut: the exact-all route, counted, answers exact.
    The same handle with every group closed inside a shard (runs of 7, the cut at a multiple of 7): the device passes,
    "exact_all" does not move.  A shard handle whose row_base is not a multiple of 64 answers for its own rows with global
    ids."""
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(161 + metric)
    n, d = 2688, 40  # two shards of 1344 = 7 * 192 rows
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[1500:1600] = rows[100]  # ties across shards
    q = _query(rng, oracle_mod, d, metric)
    spanning = rng.integers(0, 500, n).astype(np.int32)  # every group has rows on both shards
    spanning[rng.random(n) < 0.1] = -1
    closed = (np.arange(n) // 7).astype(np.int32)
    full = oracle_mod.search_exhaustive(rows, q, metric, n)
    bits = np.packbits(rng.random(n) < 0.5, bitorder="little")
    masked = oracle_mod.search_exhaustive(rows, q, metric, n, None, bits)
    monkeypatch.setenv("TSH_SHARDS_SHARE_DEVICES", "1")
    _ffi.enable_test_hooks()
    try:
        with HipVectorIndex(d, metric, capacity_rows=n, n_devices=2) as idx:
            idx.append(0, rows)
            with idx.make_groups(spanning, 500) as h:
                s0 = idx.search_grouped_rows_stats()
                _check(idx, h, spanning, full, q, (1, 10, 520), ms=(2, 64), what="two devices, spanning")
                _check(idx, h, spanning, masked, q, (10,), ms=(3,), mask=bits, what="two devices, spanning, masked")
                s1 = idx.search_grouped_rows_stats()
                assert s1["searches"] - s0["searches"] == 14 and s1["exact_all"] - s0["exact_all"] == 14  # (a job per shard)
                h.set(0, closed)  # the same handle, every group inside a shard now
                _check(idx, h, closed, full, q, (1, 10, 400), ms=(2, 64), what="two devices, closed")
                _check(idx, h, closed, masked, q, (10,), ms=(3,), mask=bits, what="two devices, closed, masked")
                s2 = idx.search_grouped_rows_stats()
                assert s2["exact_all"] == s1["exact_all"] and s2["searches"] - s1["searches"] == 14 and s2["member_rows"] > s1["member_rows"]
    finally:
        _ffi.enable_test_hooks(False)
    cut = 1237
    with HipVectorIndex(d, metric, capacity_rows=n - cut, shard_device=0, row_base=cut) as hi:
        hi.append(cut, rows[cut:])
        with hi.make_groups(spanning, 500) as h_hi:
            for lst, mk in ((full, None), (masked, bits)):
                sel = lst[0] >= cut
                own = (lst[0][sel], lst[1][sel])
                _check(hi, h_hi, spanning, own, q, (1, 10, 100), ms=(1, 3), mask=mk, what="shard handle")
            assert hi.search_grouped_rows(q, 10, 1, h_hi)[0][0].min() >= cut  # global ids


def test_many_queries_threads_and_what_a_rows_job_leaves_behind(hip_lib, oracle_mod):
    """Eight queries in one call equal eight calls and never take the batched path; four threads share one groups handle; a
    plain search, a count, a grouped search and a grouped cursor page right behind a rows job still equal the oracle (the
    side list, the head table and the heads are left clean); search_grouped launches what it launched before."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(167)
    n, d, k, m = 5000, 128, 10, 3
    rows = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((8, d)).astype(np.float32)
    group_of = (np.arange(n) // 7).astype(np.int32)
    lists = [oracle_mod.search_exhaustive(rows, qs[i], L2, n) for i in range(8)]
    want = [_spec(lists[i], group_of, k, m) for i in range(8)]
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        idx.set_batch_min_nq(2)  # (the batched path would take an 8-query tsh_search)
        with idx.make_groups(group_of, n // 7 + 1) as h:
            c0, s0 = idx.counters(), idx.search_grouped_rows_stats()
            got = idx.search_grouped_rows(qs, k, m, h)
            c1 = idx.counters()
            assert c1["batch_launches"] == c0["batch_launches"] and c1["exact_scans"] == c0["exact_scans"]
            assert c1["scan_launches"] - c0["scan_launches"] == 8 and c1["searches"] - c0["searches"] == 8
            s1 = idx.search_grouped_rows_stats()
            assert s1["searches"] - s0["searches"] == 8 and s1["redone"] == s0["redone"] and s1["exact_all"] == s0["exact_all"]
            assert s1["marked_groups"] - s0["marked_groups"] >= 8 * k and s1["member_rows"] - s0["member_rows"] >= 8 * k * m
            for i in range(8):
                _same(got, want[i], ("one call", i), q=i)
                _same(idx.search_grouped_rows(qs[i], k, m, h), want[i], ("eight calls", i))
            errors = []

            def worker(t):
                try:
                    for r in range(6):
                        i = (t * 2 + r) % 8
                        _same(idx.search_grouped_rows(qs[i], k, m, h), want[i], ("thread", t, i))
                except Exception as e:  # noqa: BLE001
                    errors.append(e)

            threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            assert not errors, errors
            # right behind a rows job, on the contexts it used: the other entries against the oracle
            for i in range(4):
                _same(idx.search_grouped_rows(qs[i], k, m, h), want[i], ("before the others", i))
                eids, edist = lists[i][0][:k], lists[i][1][:k]
                i2, d2, c2 = idx.search(qs[i], k)
                assert c2[0] == k and np.array_equal(i2[0], eids) and np.array_equal(d2[0].view(np.uint64), edist.view(np.uint64))
                _same(idx.search_grouped_rows(qs[i], k, m, h), want[i], ("between the others", i))
                assert int(idx.search_count(qs[i], float(edist[-1]))[0]) == k
                _same(idx.search_grouped_rows(qs[i], k, m, h), want[i], ("between the others", i))
                w1 = _spec(lists[i], group_of, 2 * k, 1)
                gi, gd, gg, gc = idx.search_grouped(qs[i], k, h)
                assert gc[0] == k and np.array_equal(gi[0], w1[0][:k, 0]) and np.array_equal(gd[0].view(np.uint64), w1[1][:k, 0].view(np.uint64))
                _same(idx.search_grouped_rows(qs[i], k, m, h), want[i], ("between the others", i))
                ai, ad, ag, ac = idx.search_grouped_after(qs[i], k, h, (float(gd[0, k - 1]), int(gi[0, k - 1])))
                assert ac[0] == k and np.array_equal(ai[0], w1[0][k:, 0]) and np.array_equal(ad[0].view(np.uint64), w1[1][k:, 0].view(np.uint64))
                assert int(idx.count_groups(qs[i], h)[0]) == _n_groups_in(lists[i], group_of)
            # search_grouped launches what it launched before this entry existed, and moves none of its counters
            c0, s0, g0 = idx.counters(), idx.search_grouped_rows_stats(), idx.search_grouped_stats()
            idx.search_grouped(qs, k, h)
            c1, g1 = idx.counters(), idx.search_grouped_stats()
            assert c1["scan_launches"] - c0["scan_launches"] == 8 and c1["searches"] - c0["searches"] == 8
            assert c1["batch_launches"] == c0["batch_launches"] and c1["fallback_searches"] == c0["fallback_searches"]
            assert g1["searches"] - g0["searches"] == 8 and g1["redone"] == g0["redone"] and g1["no_device_passes"] == g0["no_device_passes"]
            assert idx.search_grouped_rows_stats() == s0


def test_groups_set_after_an_append_and_a_handle_that_outlives_its_index(hip_lib, oracle_mod):
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(173)
    n, d, k = 1000, 16, 10
    rows = rng.standard_normal((2 * n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    group_of = np.concatenate([(np.arange(n) // 7), (np.arange(n) // 3)]).astype(np.int32)
    idx = HipVectorIndex(d, L2)
    idx.append(0, rows[:n])
    h = idx.make_groups(group_of[:n], n)
    _check(idx, h, group_of[:n], oracle_mod.search_exhaustive(rows[:n], q, L2, n), q, (k, 100), ms=(2, 64), what="before the append")
    idx.append(n, rows[n:])
    full = oracle_mod.search_exhaustive(rows, q, L2, 2 * n)
    _check(idx, h, group_of[:n], full, q, (k, 100), ms=(2, 64), what="appended rows are ungrouped until they are set")
    h.set(n, group_of[n:])
    _check(idx, h, group_of, full, q, (k, 100), ms=(2, 64), what="after set")
    over = group_of.copy()
    over[:50] = 5  # overwrite: the first fifty rows become one group
    h.set(0, over[:50])
    _check(idx, h, over, full, q, (k, 100), ms=(2, 64), what="after an overwrite")
    # the Python index closes its groups with itself: the raw handle is kept alive past the index here
    idx._live_masks().discard(h)
    idx.close()
    with HipVectorIndex(d, L2) as other:
        other.append(0, rows[:n])
        with pytest.raises(_ffi.TshError, match="another index"):
            other.search_grouped_rows(q, k, 2, h)
    h.close()  # frees only the handle
    with HipVectorIndex(d, L2) as idx2:
        idx2.append(0, rows[:n])
        h2 = idx2.make_groups(group_of[:n], n)
        h2.close()
        with pytest.raises(Exception):  # a closed HipGroups raises, as the other grouped entries have it
            idx2.search_grouped_rows(q, k, 2, h2)
        with idx2.make_groups(group_of[:n], n) as h3:
            mk = idx2.make_mask(np.packbits(np.ones(n, bool), bitorder="little"))
            mk.close()
            with pytest.raises(Exception):
                idx2.search_grouped_rows(q, k, 2, h3, row_mask=mk)


def test_trivial_cases_and_the_manager(hip_lib, oracle_mod):
    from tostore_amd import HipVectorIndex, VectorIndexManager, _ffi

    with HipVectorIndex(4, L2) as idx:
        with idx.make_groups(np.zeros(0, np.int32), 0) as h:
            ids, dist, grp, rows, cnt = idx.search_grouped_rows(np.zeros(4, np.float32), 5, 2, h)
            assert cnt[0] == 0 and np.all(ids == -1) and ids.shape == (1, 5, 2) and np.all(rows == 0) and np.all(grp == -1)  # an empty index
            assert idx.search_grouped_rows(np.zeros(4, np.float32), 5, 0, h)[4][0] == 0  # ... whatever rows_per_group says below 1
        idx.append(0, np.eye(4, dtype=np.float32))
        with idx.make_groups([0, 0, 1, 1], 2) as h:
            assert idx.search_grouped_rows(np.zeros(4, np.float32), 0, 2, h)[4][0] == 0  # k <= 0
            assert idx.search_grouped_rows(np.zeros(4, np.float32), 0, 0, h)[4][0] == 0  # k <= 0 and rows_per_group <= 0
            for m in (0, -3, 65):
                with pytest.raises(_ffi.TshError, match="rows_per_group"):
                    idx.search_grouped_rows(np.zeros(4, np.float32), 2, m, h)
            ids, dist, grp, rows, cnt = idx.search_grouped_rows(np.array([1, 0.5, 0, 0], np.float32), 2, 64, h)
            assert cnt[0] == 2 and list(grp[0]) == [0, 1] and list(rows[0]) == [2, 2] and list(ids[0, 0, :2]) == [0, 1] and list(ids[0, 1, :2]) == [2, 3]
    m = VectorIndexManager(4, L2)
    try:
        vecs = [[1, 0, 0, 0], [0.9, 0, 0, 0], [0, 1, 0, 0], [0, 0.5, 0, 0], [0, 0, 1, 0], [0.8, 0, 0, 0]]
        m.insert_batch(["a1", "a2", "b1", "b2", "c1", "a3"], vecs)
        with m.index.make_groups([0, 0, 1, 1, -1, 0], 2) as h:
            res = m.vectorSearchGroups([1, 0.6, 0, 0], h, topK=3, groupSize=2)
            assert [(g, [r.primaryKey for r in rs]) for g, rs in res] == [(0, ["a1", "a2"]), (1, ["b2", "b1"]), (-1, ["c1"])]
            plain = m.vectorSearch([1, 0.6, 0, 0], topK=6)
            by_doc = {}
            for r in plain:
                by_doc.setdefault(r.primaryKey[0], []).append(r.primaryKey)
            assert [[r.primaryKey for r in rs] for _, rs in res] == [v[:2] for v in by_doc.values()]
            assert [g for g, _ in m.vectorSearchGroups([1, 0.6, 0, 0], h)] == [0, 1, -1]  # topK = 10, groupSize = 3
            assert [r.primaryKey for r in m.vectorSearchGroups([1, 0.6, 0, 0], h)[0][1]] == ["a1", "a2", "a3"]
            assert [r.primaryKey for r in m.vectorSearch([1, 0.6, 0, 0], topK=3, group_by=h)] == ["a1", "b2", "c1"]  # unchanged
            only_a = m.vectorSearchGroups([1, 0.6, 0, 0], h, pk_of=lambda node: {0: "a1", 5: "a3"}.get(node))
            assert [(g, [r.primaryKey for r in rs]) for g, rs in only_a] == [(0, ["a1", "a3"])]
    finally:
        m.close()
