"""GPU: grouped search behind a cursor and the count of groups (tsh_search_grouped_after, tsh_search_grouped_count,
include/tostore_hip.h).  The oracle is search_exhaustive(rows, q, metric, n, thr, keep) -- the list L a plain search would
return with k = infinity -- and then, in Python, G: the first entry of each group; a page is the first k entries of G past
the cursor, a count their number.  Ids are compared with ==, distances as uint64 views, groups with ==."""
import math
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2
LAYOUTS = ("runs7", "random", "one", "ungrouped", "own", "mix")
START = (-math.inf, 0)


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


def _G(lst, group_of, base=0):
    """The specification over an oracle list (local ids + base = global ids): G as (ids, dist, groups), ids global"""
    eids, edist = lst
    keep, groups, seen = [], [], set()
    for i, gid in enumerate(eids + base):
        g = int(group_of[gid]) if gid < len(group_of) and group_of[gid] >= 0 else -1
        if g >= 0:
            if g in seen:
                continue
            seen.add(g)
        keep.append(i)
        groups.append(g)
    keep = np.asarray(keep, np.int64)
    return eids[keep] + base, edist[keep], np.asarray(groups, np.int32)


def _okey(d):
    """Dart double.compareTo as an integer order: -0.0 just below +0.0, every NaN the one largest key"""
    d = np.atleast_1d(np.asarray(d, np.float64))
    b = d.view(np.uint64)
    key = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
    return np.where(np.isnan(d), np.uint64(0xFFFFFFFFFFFFFFFF), key)


def _past(G, cursor):
    """The entries of G that follow the cursor strictly"""
    ids, dist, grp = G
    if cursor[0] == -math.inf:
        return G
    ck = _okey(cursor[0])[0]
    k = _okey(dist)
    sel = (k > ck) | ((k == ck) & (ids > cursor[1]))
    return ids[sel], dist[sel], grp[sel]


def _same(got, want, what):
    ids, dist, grp, cnt = got
    wi, wd, wg = want
    assert cnt[0] == len(wi), (what, int(cnt[0]), len(wi))
    c = int(cnt[0])
    assert np.array_equal(ids[0, :c], wi), (what, ids[0, :c][:12], wi[:12])
    assert np.array_equal(dist[0, :c].view(np.uint64), wd.view(np.uint64)), (what, dist[0, :c][:12], wd[:12])
    assert np.array_equal(grp[0, :c], wg), (what, grp[0, :c][:12], wg[:12])
    assert np.all(ids[0, c:] == -1) and np.all(np.isnan(dist[0, c:])) and np.all(grp[0, c:] == -1), what


def _page(idx, h, q, G, k, cursor, thr=None, mask=None, what=""):
    """One page and the count past the same cursor, against G"""
    want = _past(G, cursor)
    _same(idx.search_grouped_after(q, k, h, cursor, thr, mask), tuple(a[:k] for a in want), (what, k, cursor))
    assert int(idx.count_groups(q, h, thr, mask, after=cursor)[0]) == len(want[0]), (what, "count", cursor)


def _walk(idx, h, q, G, k, thr=None, mask=None, start=0, max_pages=None, what=""):
    """Pages of k from G's entry `start` on (the cursor: the entry before it) until a short page or max_pages: they
    concatenate to G; after every page, count(after = its last entry) == count(no cursor) - entries of G so far."""
    total = int(idx.count_groups(q, h, thr, mask)[0])
    assert total == len(G[0]), (what, "count without a cursor", total, len(G[0]))
    cursor = START if start == 0 else (float(G[1][start - 1]), int(G[0][start - 1]))
    pos, pages = start, 0
    while max_pages is None or pages < max_pages:
        got = idx.search_grouped_after(q, k, h, cursor, thr, mask)
        _same(got, tuple(a[pos:pos + k] for a in G), (what, "page", pages, "k", k, "from", pos))
        c = int(got[3][0])
        pos += c
        pages += 1
        if c:
            cursor = (float(got[1][0, c - 1]), int(got[0][0, c - 1]))
            left = int(idx.count_groups(q, h, thr, mask, after=cursor)[0])
            assert left == total - pos, (what, "count after", pos, "entries", left, total)
        if c < k:
            assert pos == len(G[0]), (what, "a short page before the end", pos, len(G[0]))
            return
    assert max_pages is not None


def _walks(idx, h, q, G, thr=None, mask=None, what=""):
    """k in {1, 7, 100}: whole walks where they are short, else the first pages, pages from the middle and the tail"""
    n = len(G[0])
    for a, b in zip(idx.search_grouped_after(q, 10, h, START, thr, mask), idx.search_grouped(q, 10, h, thr, mask)):
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), (what, "-inf")
    for k, pages in ((1, 8), (7, 10), (100, None)):
        if pages is None or n <= k * pages:
            _walk(idx, h, q, G, k, thr, mask, what=what)
        else:
            _walk(idx, h, q, G, k, thr, mask, max_pages=pages, what=what)
            _walk(idx, h, q, G, k, thr, mask, start=n // 2, max_pages=pages, what=what)
            _walk(idx, h, q, G, k, thr, mask, start=n - k * 2 - 1, what=what)


@pytest.mark.parametrize("metric", [L2, IP, COS])
@pytest.mark.parametrize("d", [4, 128, 257])
def test_pages_walk_to_G(hip_lib, oracle_mod, metric, d):
    """Every shape x every layout, dense: pages of k in {1, 7, 100} concatenate to G, a cursor of -inf equals search_grouped
    bit for bit, the count identity holds after every page, "one group" counts 1 or 0.  Then, for two layouts, behind a
    keep-50 % mask as pointer and as handle, "nothing kept", a keep-1 % mask at n = 5000 (the list scan), tombstones (a whole
    tile, the last row and the nearest group's head), a gap of ids and a threshold inside the list."""
    from tostore_amd import HipMask, HipVectorIndex

    rng = np.random.default_rng(9000 + 10 * d + metric)
    for n in (1, 63, 64, 65, 4097, 5000):
        rows = rng.standard_normal((n, d)).astype(np.float32)
        q = _query(rng, oracle_mod, d, metric)
        full = oracle_mod.search_exhaustive(rows, q, metric, n)
        with HipVectorIndex(d, metric, capacity_rows=n) as idx:
            idx.append(0, rows)
            for name in LAYOUTS:
                group_of, n_groups = _layout(name, n, rng)
                G = _G(full, group_of)
                with idx.make_groups(group_of, n_groups) as h:
                    _walks(idx, h, q, G, what=(n, name))
                    if name == "one":
                        assert int(idx.count_groups(q, h)[0]) == 1
                        assert int(idx.count_groups(q, h, after=(float(full[1][0]), int(full[0][0])))[0]) == 0
                        # the group's best is consumed: its other rows do not come back
                        assert idx.search_grouped_after(q, 5, h, (float(full[1][0]), int(full[0][0])))[3][0] == 0
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
                        G = _G(oracle_mod.search_exhaustive(rows, q, metric, n, None, bits), group_of)
                        c0 = idx.counters()
                        _walks(idx, h, q, G, mask=bits, what=(n, name, "pointer mask", int(m.sum())))
                        with HipMask(idx, bits) as mh:
                            _walks(idx, h, q, G, mask=mh, what=(n, name, "mask handle", int(m.sum())))
                        if n == 5000 and d == 257 and 0 < m.sum() < 100:  # (rows of 257 floats: a width the list scan serves)
                            assert idx.counters()["list_scans"] > c0["list_scans"]
                    if n >= 65:  # a threshold inside the list
                        thr = float(full[1][n // 3])
                        G = _G(oracle_mod.search_exhaustive(rows, q, metric, n, thr), group_of)
                        _walks(idx, h, q, G, thr=thr, what=(n, name, "threshold"))
            group_of, n_groups = _layout("runs7", n, rng)
            with idx.make_groups(group_of, n_groups) as h:
                t = 1 if n >= 129 else 0
                dead = sorted(set(range(64 * t, min(64 * t + 64, n))) | {n - 1, int(full[0][0])})
                idx.set_deleted(np.asarray(dead, np.int64))
                alive = np.ones(n, bool)
                alive[dead] = False
                G = _G(oracle_mod.search_exhaustive(rows, q, metric, n, None, np.packbits(alive, bitorder="little")), group_of)
                _walks(idx, h, q, G, what=(n, "tombstones"))
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
                        _walks(idx, h, q, _G(lst, group_of), what=(n, name, "gap"))


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_a_consumed_group_does_not_come_back(hip_lib, oracle_mod, metric):
    """Layout "random": the cursor is set just past a group's best row (on it, and one ulp beyond it) while that group still
    has rows beyond the cursor.  The group is consumed: none of its rows may appear on the page or in the count.  This test
    fails on "floor, then group" -- flooring the rows at the cursor first makes the best of the group's remaining rows its
    head, and the group comes back."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(101 + metric)
    n, d = 5000, 128
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    group_of, n_groups = _layout("random", n, rng)
    full = oracle_mod.search_exhaustive(rows, q, metric, n)
    G = _G(full, group_of)
    with HipVectorIndex(d, metric, capacity_rows=n) as idx:
        idx.append(0, rows)
        with idx.make_groups(group_of, n_groups) as h:
            sizes = np.bincount(group_of, minlength=n_groups)
            open_ = [e for e in range(len(G[0])) if sizes[G[2][e]] > 1]  # (entries whose group has rows beyond its best)
            assert len(open_) > 100
            for e in (open_[0], open_[1], open_[5], open_[40], open_[len(open_) // 2], open_[-1]):
                g = int(G[2][e])
                for cursor in ((float(G[1][e]), int(G[0][e])), (float(np.nextafter(G[1][e], np.inf)), -1)):
                    for k in (1, 10, 2000):
                        got = idx.search_grouped_after(q, k, h, cursor)
                        assert g not in got[2][0, :int(got[3][0])], ("the consumed group came back", e, k)
                        _page(idx, h, q, G, k, cursor, what=("consumed", e))


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_cursor_shapes(hip_lib, oracle_mod, metric):
    """A cursor on a non-head row of a group, midway between two entries, before every row, beyond every row (an empty
    page), +inf and NaN (no scan), and -- L2 -- a cursor of -0.0 and +0.0 over rows at distance 0."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(111 + metric)
    n, d = 4097, 40
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = _query(rng, oracle_mod, d, metric)
    if metric == L2:
        rows[[5, 70, 3000]] = q  # distance +0.0
    full = oracle_mod.search_exhaustive(rows, q, metric, n)
    with HipVectorIndex(d, metric, capacity_rows=n) as idx:
        idx.append(0, rows)
        for name in ("runs7", "random", "mix"):
            group_of, n_groups = _layout(name, n, rng)
            G = _G(full, group_of)
            heads = set(int(i) for i in G[0])
            non_heads = [i for i in range(len(full[0])) if int(full[0][i]) not in heads]
            with idx.make_groups(group_of, n_groups) as h:
                cursors = [(float(full[1][i]), int(full[0][i])) for i in (non_heads[:3] + non_heads[len(non_heads) // 2:][:3] + non_heads[-2:])]
                cursors += [((float(G[1][i]) + float(G[1][i + 1])) / 2, 0) for i in (0, 7, len(G[0]) // 2, len(G[0]) - 2)]
                cursors += [(float(np.nextafter(full[1][0], -np.inf)), n + 5), (float(full[1][-1]), int(full[0][-1])),
                            (float(np.nextafter(full[1][-1], np.inf)), 0), (math.inf, 0), (math.nan, 0), (-0.0, 0), (0.0, 6), (0.0, -1)]
                for cursor in cursors:
                    for k in (1, 10, 100):
                        _page(idx, h, q, G, k, cursor, what=(name, "cursor shapes"))
                assert idx.search_grouped_after(q, 10, h, (float(np.nextafter(full[1][-1], np.inf)), 0))[3][0] == 0


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_ties(hip_lib, oracle_mod, metric):
    """Rows of small integers at d = 4: rows duplicated across groups and within one group, the id decides."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(121 + metric)
    d = 4
    for n in (65, 700, 5000):
        rows = rng.integers(-2, 3, (n, d)).astype(np.float32)
        q = rng.integers(-2, 3, d).astype(np.float32)
        if metric == COS:
            q = oracle_mod.normalize_f32(q + np.float32(0.25))
        with np.errstate(all="ignore"):
            full = oracle_mod.search_exhaustive(rows, q, metric, n)
        with HipVectorIndex(d, metric, capacity_rows=n) as idx:
            idx.append(0, rows)
            for name in ("runs7", "random", "mix", "own"):
                group_of, n_groups = _layout(name, n, rng)
                with idx.make_groups(group_of, n_groups) as h:
                    _walks(idx, h, q, _G(full, group_of), what=(n, name, "ties"))


def test_side_list_overflow_is_redone(hip_lib, oracle_mod):
    """3000 rows equal to the cursor's row, each the head of its own group (or ungrouped): every one of them is undecided
    by key.  The side list (1024 rows) overflows, the job is redone with a larger one, stats "redone" moves -- for the page
    and for the count."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(131)
    n, d, k = 5000, 32, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    same = np.sort(rng.choice(n, 3000, replace=False))
    rows[same] = q + np.float32(0.01)
    group_of = np.arange(n, dtype=np.int32)
    group_of[same[::3]] = -1
    group_of[same[1500]] = group_of[same[10]]  # (and two of them in one group: the later one never appears)
    full = oracle_mod.search_exhaustive(rows, q, L2, n)
    G = _G(full, group_of)
    cursor = (float(full[1][0]), int(same[1400]))
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        with idx.make_groups(group_of, n) as h:
            s0 = idx.search_grouped_after_stats()
            want = _past(G, cursor)
            assert int(same[1500]) not in want[0]
            _same(idx.search_grouped_after(q, k, h, cursor), tuple(a[:k] for a in want), "side overflow")
            s1 = idx.search_grouped_after_stats()
            assert s1["redone"] - s0["redone"] == 1 and s1["side_rows"] - s0["side_rows"] >= 3000 and s1["searches"] - s0["searches"] == 1
            _same(idx.search_grouped_after(q, k, h, cursor), tuple(a[:k] for a in want), "side overflow, again")  # (the context kept the larger list)
            assert idx.search_grouped_after_stats()["redone"] == s1["redone"]
        with HipVectorIndex(d, L2, capacity_rows=n) as other:  # a fresh context: the count overflows too
            other.append(0, rows)
            with other.make_groups(group_of, n) as h2:
                s0 = other.search_grouped_after_stats()
                assert int(other.count_groups(q, h2, after=cursor)[0]) == len(want[0])
                s1 = other.search_grouped_after_stats()
                assert s1["redone"] - s0["redone"] == 1 and s1["counts"] - s0["counts"] == 1
        # the older entries' counters did not move
        assert idx.search_grouped_stats()["searches"] == 0 and idx.search_after_stats()["searches"] == 0 and idx.search_count_stats()["searches"] == 0


def test_candidate_block_overflow_runs_the_wide_band_over_floored_heads(hip_lib, oracle_mod):
    """600 groups with identical best distances at k = 100, a cursor in their middle: more heads past the cursor inside the
    band than the block holds."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(133)
    n, d, k = 5000, 32, 100
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    group_of = (np.arange(n) % 600).astype(np.int32)
    rows[:600] = q + np.float32(0.01)
    rows[600:1200] = q + np.float32(0.0100001)  # a hair farther: the heads past the cursor
    full = oracle_mod.search_exhaustive(rows, q, L2, n)
    G = _G(full, group_of)
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        with idx.make_groups(group_of, 600) as h:
            c0 = idx.counters()
            _page(idx, h, q, G, k, (float(G[1][0]) * 0.5, 0), what="block overflow")  # (well before the 600 heads: all past the cursor)
            assert idx.counters()["fallback_searches"] > c0["fallback_searches"]
            _page(idx, h, q, G, k, (float(G[1][300]), int(G[0][300])), what="block overflow, a cursor among the ties")


def test_rows_outside_the_model_and_safe_mode(hip_lib, oracle_mod):
    """The exact-all route by a quarantined row: one inf-element row that is its group's best under inner product (and a huge
    finite one) -- answers are exact and stats "exact_all" moves with every job.  Then more than 1024 irregular rows: safe
    mode."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(137)
    n, d = 500, 32
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    rows[100, 3] = np.inf if q[3] > 0 else -np.inf  # inner product +inf: distance -inf, the best of everything
    rows[333, 7] = 1e20 if q[7] > 0 else -1e20      # a huge finite one: the best of its group
    group_of = (np.arange(n) // 7).astype(np.int32)
    with np.errstate(all="ignore"):
        full = oracle_mod.search_exhaustive(rows, q, IP, n)
    assert full[0][0] == 100 and full[0][1] == 333
    G = _G(full, group_of)
    with HipVectorIndex(d, IP, capacity_rows=n) as idx:
        idx.append(0, rows)
        assert idx.counters()["quarantined_rows"] == 2 and not idx.counters()["safe_mode"]
        with idx.make_groups(group_of, n) as h:
            s0 = idx.search_grouped_after_stats()
            # (row 100's distance is -inf, and a cursor of -inf is "from the start": pages start there or past row 333)
            for k in (1, 2, 10, 100):
                _page(idx, h, q, G, k, START, what="quarantined")
            _walk(idx, h, q, G, 7, start=2, what="quarantined")
            _walk(idx, h, q, G, 1, start=2, max_pages=8, what="quarantined")
            # past the quarantined best of group 14: rows 98 .. 104 stay away
            got = idx.search_grouped_after(q, 100, h, (float(full[1][1]), 333))
            assert 14 not in got[2][0] and 47 not in got[2][0] and got[3][0] == len(G[0]) - 2
            _page(idx, h, q, G, 10, (math.inf, 0), what="quarantined, +inf")
            s1 = idx.search_grouped_after_stats()
            jobs = s1["searches"] - s0["searches"] + s1["counts"] - s0["counts"]
            assert jobs > 0 and s1["exact_all"] - s0["exact_all"] == jobs and s1["side_rows"] == s0["side_rows"]
            idx.set_deleted(np.asarray([100, 333], np.int64))  # no live quarantined row: the device passes again
            alive = np.ones(n, bool)
            alive[[100, 333]] = False
            with np.errstate(all="ignore"):
                G2 = _G(oracle_mod.search_exhaustive(rows, q, IP, n, None, np.packbits(alive, bitorder="little")), group_of)
            _walk(idx, h, q, G2, 7, what="quarantined rows deleted")
            assert idx.search_grouped_after_stats()["exact_all"] == s1["exact_all"]
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
            _walks(idx, h, q, _G(full, group_of), what="safe mode")


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_several_devices_and_shard_handles(hip_lib, oracle_mod, metric, monkeypatch):
    """A handle over two devices that share a GPU.  Groups spanning the shards: the exact-all route, answers exact, stats
    "exact_all" moves.  The same handle with every group closed inside a shard (runs of 7, the cut at a multiple of 7): the
    device passes, "exact_all" does not move.  A shard handle whose row_base is not a multiple of 64 answers for its own
    rows."""
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(141 + metric)
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
                s0 = idx.search_grouped_after_stats()
                _walk(idx, h, q, _G(full, spanning), 7, max_pages=6, what="two devices, spanning")
                _walk(idx, h, q, _G(full, spanning), 100, what="two devices, spanning")
                _walk(idx, h, q, _G(masked, spanning), 100, mask=bits, what="two devices, spanning, masked")
                s1 = idx.search_grouped_after_stats()
                jobs = s1["searches"] - s0["searches"] + s1["counts"] - s0["counts"]
                assert jobs > 0 and s1["exact_all"] - s0["exact_all"] == jobs
                h.set(0, closed)  # the same handle, every group inside a shard now
                _walk(idx, h, q, _G(full, closed), 7, max_pages=6, what="two devices, closed")
                _walk(idx, h, q, _G(full, closed), 7, start=190, max_pages=6, what="two devices, closed, across the cut")
                _walk(idx, h, q, _G(full, closed), 100, what="two devices, closed")
                _walk(idx, h, q, _G(masked, closed), 100, mask=bits, what="two devices, closed, masked")
                s2 = idx.search_grouped_after_stats()
                assert s2["exact_all"] == s1["exact_all"] and s2["searches"] > s1["searches"]
    finally:
        _ffi.enable_test_hooks(False)
    cut = 1237
    with HipVectorIndex(d, metric, capacity_rows=n - cut, shard_device=0, row_base=cut) as hi:
        hi.append(cut, rows[cut:])
        with hi.make_groups(spanning, 500) as h_hi:
            for lst, m in ((full, None), (masked, bits)):
                sel = lst[0] >= cut
                G = _G((lst[0][sel], lst[1][sel]), spanning)
                _walk(hi, h_hi, q, G, 7, mask=m, max_pages=6, what="shard handle")
                _walk(hi, h_hi, q, G, 100, mask=m, what="shard handle")


def test_many_queries_and_threads(hip_lib, oracle_mod):
    """Eight queries with eight cursors in one call equal eight calls and never take the batched path; eight threads page
    concurrently over one groups handle; a plain search and a count behind them still equal the oracle."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(151)
    n, d, k = 5000, 128, 7
    rows = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((8, d)).astype(np.float32)
    group_of, n_groups = _layout("random", n, rng)
    Gs = [_G(oracle_mod.search_exhaustive(rows, qs[i], L2, n), group_of) for i in range(8)]
    with HipVectorIndex(d, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        idx.set_batch_min_nq(2)  # (the batched path would take an 8-query tsh_search)
        with idx.make_groups(group_of, n_groups) as h:
            a_dist = np.asarray([-math.inf] + [float(Gs[i][1][i * 3]) for i in range(1, 8)])
            a_id = np.asarray([0] + [int(Gs[i][0][i * 3]) for i in range(1, 8)], np.int64)
            c0 = idx.counters()
            ids, dist, grp, cnt = idx.search_grouped_after(qs, k, h, (a_dist, a_id))
            counts = idx.count_groups(qs, h, after=(a_dist, a_id))
            c1 = idx.counters()
            assert c1["batch_launches"] == c0["batch_launches"] and c1["exact_scans"] == c0["exact_scans"]
            assert c1["scan_launches"] - c0["scan_launches"] == 16
            for i in range(8):
                want = _past(Gs[i], (a_dist[i], a_id[i]))
                _same((ids[i:i + 1], dist[i:i + 1], grp[i:i + 1], cnt[i:i + 1]), tuple(a[:k] for a in want), ("one call", i))
                assert int(counts[i]) == len(want[0])
            errors = []

            def worker(t):
                try:
                    _walk(idx, h, qs[t], Gs[t], k, start=t * 5, max_pages=8, what=("thread", t))
                except Exception as e:  # noqa: BLE001
                    errors.append(e)

            threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            assert not errors, errors
            eids, edist = oracle_mod.search_exhaustive(rows, qs[0], L2, 10)
            i2, d2, c2 = idx.search(qs[0], 10)
            assert c2[0] == 10 and np.array_equal(i2[0], eids) and np.array_equal(d2[0].view(np.uint64), edist.view(np.uint64))
            assert int(idx.search_count(qs[0], float(edist[-1]))[0]) == 10


def test_trivial_cases_errors_and_the_manager(hip_lib, oracle_mod):
    from tostore_amd import HipMask, HipVectorIndex, VectorIndexManager, _ffi

    with HipVectorIndex(4, L2) as idx:
        with idx.make_groups(np.zeros(0, np.int32), 0) as h:
            ids, dist, grp, cnt = idx.search_grouped_after(np.zeros(4, np.float32), 5, h, START)
            assert cnt[0] == 0 and np.all(ids == -1)  # an empty index
            assert int(idx.count_groups(np.zeros(4, np.float32), h)[0]) == 0
        idx.append(0, np.eye(4, dtype=np.float32))
        h = idx.make_groups([0, 0, 1, 1], 2)
        assert idx.search_grouped_after(np.zeros(4, np.float32), 0, h, START)[3][0] == 0  # k <= 0
        q = np.zeros(4, np.float32)
        cnt = np.zeros(1, np.int64)
        one = np.zeros(1, np.float64)
        # exactly one cursor array
        rc = _ffi.lib().tsh_search_grouped_count(idx._h, q.ctypes.data_as(_ffi.p_f32), 1, math.nan, None, None, h.handle(),
                                                 one.ctypes.data_as(_ffi.p_f64), None, cnt.ctypes.data_as(_ffi.p_i64))
        assert rc == _ffi.TSH_E_BAD_ARG
        m = HipMask(idx, np.packbits(np.ones(4, bool), bitorder="little"))
        m.close()
        with pytest.raises(ValueError):
            idx.search_grouped_after(q, 2, h, START, row_mask=m)
        with pytest.raises(ValueError):
            idx.count_groups(q, h, row_mask=m)
        h.close()
        with pytest.raises(ValueError):
            idx.search_grouped_after(q, 2, h, START)
        with pytest.raises(ValueError):
            idx.count_groups(q, h)
    m = VectorIndexManager(4, L2)
    try:
        vecs = [[1, 0, 0, 0], [0.9, 0, 0, 0], [0, 1, 0, 0], [0, 0.5, 0, 0], [0, 0, 1, 0]]
        m.insert_batch(["a1", "a2", "b1", "b2", "c1"], vecs)
        with m.index.make_groups([0, 0, 1, 1, -1], 2) as h:
            assert m.countGroups([1, 0.6, 0, 0], h) == 3
            page, cursor, keys = None, START, []
            while page is None or len(page) == 2:
                page = m.vectorSearchGroupedAfter([1, 0.6, 0, 0], h, cursor, topK=2)
                keys += [r.primaryKey for r in page]
                if page:
                    cursor = (page[-1].distance, page[-1].nodeId)
                    assert m.countGroups([1, 0.6, 0, 0], h, after=cursor) == 3 - len(keys)
            assert keys == ["a1", "b2", "c1"]
    finally:
        m.close()
