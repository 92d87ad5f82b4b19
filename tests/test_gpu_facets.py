"""GPU: facet counts on the device (tsh_attr_facets, tsh_tags_facets; F1 attr_facets_kernel and F2 tags_facets_kernel of
tostore_amd/csrc/tsh_facet.hip.h, their host side tsh_facet_plan.h).  NumPy on the host is the specification
(_attr_spec, _tags_spec over the population _P) and the answer is exact.  The population is held to the entries that
exist: the total is tsh_search_count's answer without a threshold, and a key's count is that count under the mask a
range or tag term makes of the key.  The sizes are the smallest at which these kernels can still go wrong: a wave's word
of 64 rows, its passes of 64 values, the grid's cap (a second grid-stride word per wave), the part cache's list threshold
at 4096 rows, QUARANTINE_MAX + 1 irregular rows.  d = 8 throughout: the rows only have to be there."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2 = 0
D = 8
NULL, I64_MIN, I64_MAX = -(1 << 63), -(1 << 63), (1 << 63) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tostore_amd", "csrc")


def _wrap_rows():
    """grid cap x waves per workgroup x 64 rows + 65, from the kernels' own constants: the grid is at its cap there and a
    wave takes a second grid-stride word"""
    facet, where = open(os.path.join(CSRC, "tsh_facet.hip.h")).read(), open(os.path.join(CSRC, "tsh_where.hip.h")).read()
    cap = int(re.search(r"^#define TSH_FACET_MAX_BLOCKS (\d+)", facet, re.M).group(1))
    assert re.search(r"constexpr int FACET_MAX_BLOCKS = TSH_FACET_MAX_BLOCKS;", facet)
    assert re.search(r"constexpr int FACET_BLOCK = WHERE_BLOCK;", facet) and re.search(r"constexpr int FACET_WAVES = FACET_BLOCK / 64;", facet)
    block = int(re.search(r"constexpr int WHERE_BLOCK = (\d+);", where).group(1))
    return cap * (block // 64) * 64 + 65


WRAP = _wrap_rows()


# ---- the specification ------------------------------------------------------------------------------------------------------------
def _bits(keep, n_bytes=None):
    b = np.packbits(np.asarray(keep, bool), bitorder="little")
    if n_bytes is not None:
        b = np.concatenate([b, np.zeros(n_bytes - len(b), np.uint8)])
    return b


def _P(live, keep=None):
    """the rows a search could return: present and not tombstoned (`live`, one flag per row id below the index's size),
    and kept by the mask if one is given (rows beyond its bitmap are not kept)"""
    p = np.asarray(live, bool).copy()
    if keep is not None:
        k = np.zeros(len(p), bool)
        m = min(len(p), len(keep))
        k[:m] = np.asarray(keep, bool)[:m]
        p &= k
    return p


def _v(vals, n):
    """the column's value of rows 0 .. n - 1: rows beyond the column read as NULL"""
    v = np.full(n, NULL, np.int64)
    m = min(n, len(vals))
    v[:m] = np.asarray(vals, np.int64)[:m]
    return v


def _attr_spec(vals, P, keys, kind="values"):
    keys = np.asarray(keys, np.int64).reshape(-1)
    vp = _v(vals, len(P))[P]
    nn = vp[vp != NULL]
    if kind == "values":
        u, c = np.unique(nn, return_counts=True)
        at = np.searchsorted(u, keys)
        hit = (at < len(u)) & (keys != NULL)
        hit[hit] = u[at[hit]] == keys[hit]
        counts = np.zeros(len(keys), np.int64)
        counts[hit] = c[at[hit]]
        other = len(nn) - int(np.isin(nn, keys[keys != NULL]).sum())
    else:
        b = np.searchsorted(keys, nn, side="right") - 1  # the last edge <= v
        counts = np.bincount(b[b >= 0], minlength=len(keys)).astype(np.int64)
        other = int((b < 0).sum())
    return counts, other, len(vp) - len(nn), len(vp)


def _tags_spec(col, P, keys):
    off, vals = col
    n = len(P)
    keys = np.asarray(keys, np.int64).reshape(-1)
    m = min(n, len(off) - 1)
    owner = np.repeat(np.arange(len(off) - 1), np.diff(off))
    owner, vals = owner[owner < m], vals[:off[m]]
    is_null = np.ones(n, bool)  # (rows beyond the column)
    is_null[:m] = np.bincount(owner[vals == NULL], minlength=m) > 0
    ok = P & ~is_null
    S = np.unique(keys[keys != NULL])
    sel = ok[owner] & np.isin(vals, S)
    pairs = np.unique(np.stack([owner[sel], vals[sel]]), axis=1) if sel.any() else np.zeros((2, 0), np.int64)  # a row is a set
    per_key = np.bincount(np.searchsorted(S, pairs[1]), minlength=len(S)) if len(S) else np.zeros(0, np.int64)
    counts = np.zeros(len(keys), np.int64)
    real = keys != NULL
    counts[real] = per_key[np.searchsorted(S, keys[real])]
    holders = np.zeros(n, bool)
    holders[pairs[0]] = True
    return counts, int((ok & ~holders).sum()), int((P & is_null).sum()), int(P.sum())


def _eq(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, "counts", np.flatnonzero(got[0] != want[0])[:8], got[0][:8], want[0][:8])
    assert tuple(got[1:]) == tuple(want[1:]), (what, "other, null, total", got[1:], want[1:])


def _attr_ok(idx, attr, vals, live, keys, kind="values", mask=None, keep=None, what=""):
    got = idx.facets(attr, keys, mask, kind)
    assert got[0].dtype == np.int64 and got[0].shape == (len(keys),)
    _eq(got, _attr_spec(vals, _P(live, keep), keys, kind), what)
    return got


def _tags_ok(idx, tags, col, live, keys, mask=None, keep=None, what=""):
    got = idx.facets(tags, keys, mask)
    _eq(got, _tags_spec(col, _P(live, keep), keys), what)
    return got


def _count(idx, mask=None):
    """tsh_search_count without a threshold: |P| by the entry that exists"""
    return int(idx.search_count(np.ones(D, np.float32), None, mask)[0])


def _random_attr(rng, n, universe=12, p_null=0.1):
    v = rng.integers(0, universe, n).astype(np.int64)
    v[rng.random(n) < p_null] = NULL
    return v


def _random_tags(rng, n, universe=40, max_len=8, p_null=0.08, p_empty=0.15):
    lens = rng.integers(1, max_len + 1, n)
    lens[rng.random(n) < p_empty] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    vals = rng.integers(0, universe, off[-1]).astype(np.int64)
    for r in np.flatnonzero((rng.random(n) < p_null) & (lens > 0)):
        vals[off[r] + (0, lens[r] - 1, lens[r] // 2)[r % 3]] = NULL
    return off, vals


def _csr(lists):
    lens = np.array([len(r) for r in lists], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    vals = np.concatenate([np.asarray(r, np.int64).reshape(-1) for r in lists]) if len(lists) else np.zeros(0, np.int64)
    return off, vals.astype(np.int64)


def _ones(n):
    return np.ones((n, D), np.float32)


# ---- 1. rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 4095, 4096, 4097, WRAP])
def test_rows_are_numpys(hip_lib, n):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(n)
    cap = n + 479
    live = np.ones(n, bool)
    vals = _random_attr(rng, n + 70)  # 70 entries longer than the index: they must not be counted
    vals[rng.integers(0, n, 3)] = I64_MAX
    vals[rng.integers(0, n, 3)] = I64_MIN + 1
    short = vals[:n - (n + 2) // 3]  # ... and a column that ends inside the index
    col = _random_tags(rng, n + 70)
    tshort = (col[0][:n - (n + 2) // 3 + 1], col[1])
    keys = np.array([7, 3, NULL, 3, I64_MAX, 11, 100, I64_MIN + 1], np.int64)  # unsorted, repeated, a NULL, one in no row
    edges = np.array([I64_MIN + 1, 2, 3, 9, I64_MAX], np.int64)
    with HipVectorIndex(D, L2, capacity_rows=cap) as idx:
        idx.append(0, _ones(n))
        assert _count(idx) == n
        with idx.make_attr(vals) as attr, idx.make_attr(short) as ashort, idx.make_tags(col) as tags, idx.make_tags(tshort) as tsh:
            # a capacity-sized bitmap with every bit past the last row set -- none is counted; a selective one; a range-made one
            w = rng.random(n) < 0.4
            full = np.ones(cap, bool)
            full[:n] = w
            few = rng.random(n) < 0.01
            few[n // 2] = True
            with idx.make_mask(_bits(full)) as mw, idx.make_mask(_bits(few)) as mfew, idx.make_mask_where(attr, 2, 8) as mr:
                in_range = (_v(vals, n) != NULL) & (_v(vals, n) >= 2) & (_v(vals, n) <= 8)
                for mask, keep in ((None, None), (mw, w), (mfew, few), (mr, in_range)):
                    got = _attr_ok(idx, attr, vals, live, keys, "values", mask, keep)
                    assert got[3] == _count(idx, mask)
                    _attr_ok(idx, attr, vals, live, edges, "edges", mask, keep)
                    _attr_ok(idx, ashort, short, live, keys, "values", mask, keep)
                    _attr_ok(idx, ashort, short, live, edges[1:], "edges", mask, keep)
                    _attr_ok(idx, attr, vals, live, [], "values", mask, keep)
                    got = _tags_ok(idx, tags, col, live, [3, 17, NULL, 3, 39, 1000], mask, keep)
                    assert got[3] == _count(idx, mask)
                    _tags_ok(idx, tsh, tshort, live, [1, 2, 3], mask, keep)
                    _tags_ok(idx, tags, col, live, [], mask, keep)


# ---- 2. keys ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [0, 1, 2, 3, 4095, 4096])
def test_keys_are_numpys(hip_lib, size):
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(100 + size)
    n = 20_011
    live = np.ones(n, bool)
    vals = rng.integers(-3000, 3000, n).astype(np.int64)
    vals[rng.random(n) < 0.05] = NULL
    vals[:4] = (I64_MAX, I64_MIN + 1, I64_MAX, I64_MIN + 1)
    col = _random_tags(rng, n, universe=6000)
    col[1][col[0][5]:col[0][5] + 1] = I64_MAX  # (row 5's first value, if it has one)
    pool = np.concatenate([[I64_MAX, I64_MIN + 1], rng.permutation(np.arange(-3200, 3200))]).astype(np.int64)
    keys = pool[:size].copy()
    rng.shuffle(keys)
    noisy = np.concatenate([keys, keys[:3], [NULL, NULL]]) if size else np.array([NULL], np.int64)  # repeats and NULLs do not count to the limit
    rng.shuffle(noisy)
    keep = rng.random(n) < 0.5
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, _ones(n))
        with idx.make_attr(vals) as attr, idx.make_tags(col) as tags, idx.make_mask(_bits(keep)) as mk:
            for mask, kp in ((None, None), (mk, keep)):
                for ks in (keys, noisy):
                    got = _attr_ok(idx, attr, vals, live, ks, "values", mask, kp)
                    # the counts of the distinct keys + other + null = total
                    real = ks != NULL
                    _, first = np.unique(ks[real], return_index=True)
                    assert int(got[0][real][first].sum()) + got[1] + got[2] == got[3]
                    _tags_ok(idx, tags, col, live, ks, mask, kp)
                e = np.sort(keys)
                got = _attr_ok(idx, attr, vals, live, e, "edges", mask, kp)
                assert int(got[0].sum()) + got[1] + got[2] == got[3]
            if size == 4096:  # one more distinct key is refused, whatever else the keys hold
                over = np.concatenate([keys, [3201]]).astype(np.int64)
                for column, kind in ((attr, "values"), (attr, "edges"), (tags, "values")):
                    with pytest.raises(_ffi.TshError, match="TSH_FACET_MAX_KEYS"):
                        idx.facets(column, np.sort(over), None, kind)


def test_edges(hip_lib):
    from tostore_amd import HipVectorIndex, _ffi

    n = 1_000
    vals = np.arange(n, dtype=np.int64) - 100  # -100 .. 899
    vals[::97] = NULL
    vals[1], vals[2], vals[3] = I64_MAX, I64_MAX - 1, I64_MIN + 1
    live = np.ones(n, bool)
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, _ones(n))
        with idx.make_attr(vals) as attr:
            for e in ([0], [500], [I64_MAX], [I64_MIN + 1], [0, 1, 2, 3], [-100, 0, 10, 899], [-1000, 5000], [10, 20, I64_MAX],
                      [I64_MIN + 1, I64_MIN + 2, I64_MAX - 1, I64_MAX]):
                got = _attr_ok(idx, attr, vals, live, e, "edges", what=e)
                assert int(got[0].sum()) + got[1] + got[2] == got[3] == n
            # values equal to edges open their bucket; values below the first edge are other; the last bucket is open
            got = idx.facets(attr, [10, 20, I64_MAX], None, "edges")
            nn = vals[vals != NULL]
            assert got[0].tolist() == [int(((nn >= 10) & (nn < 20)).sum()), int(((nn >= 20) & (nn < I64_MAX)).sum()), 1]
            assert got[1] == int((nn < 10).sum())
            for bad in ([1, 1], [2, 1], [NULL, 3], [0, 5, 5]):
                with pytest.raises(_ffi.TshError):
                    idx.facets(attr, bad, None, "edges")


# ---- 3. one hot counter, and none ---------------------------------------------------------------------------------------------
def test_one_value_and_all_distinct_at_the_wrap_shape(hip_lib):
    from tostore_amd import HipVectorIndex

    n = WRAP
    rng = np.random.default_rng(3)
    live = np.ones(n, bool)
    one = np.full(n, 42, np.int64)
    distinct = rng.permutation(n).astype(np.int64)
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, _ones(n))
        with idx.make_attr(one) as a1, idx.make_attr(distinct) as a2:
            got = _attr_ok(idx, a1, one, live, [42, 41])
            assert got[0].tolist() == [n, 0] and got[1:] == (0, 0, n)
            assert _attr_ok(idx, a1, one, live, [0, 42, 43], "edges")[0].tolist() == [0, n, 0]
            assert _attr_ok(idx, a1, one, live, [7])[1] == n  # every row "other": one counter again
            keys = rng.choice(n, 4096, replace=False).astype(np.int64)
            got = _attr_ok(idx, a2, distinct, live, keys)
            assert (got[0] == 1).all() and got[1] == n - 4096
            got = _attr_ok(idx, a2, distinct, live, np.sort(keys), "edges")
            assert int(got[0].sum()) + got[1] == n
            # two runs agree bit for bit
            again = idx.facets(a2, keys)
            assert np.array_equal(again[0], _attr_ok(idx, a2, distinct, live, keys)[0])
        # a key every row holds, in a tag column
        lists = [[5, i % 7 + 10] for i in range(n)]
        col = _csr(lists)
        with idx.make_tags(col) as tags:
            got = _tags_ok(idx, tags, col, live, [5, 10, 99])
            assert got[0][0] == n and got[1] == 0


# ---- 4. masks -----------------------------------------------------------------------------------------------------------------
def test_masks(hip_lib):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(4)
    n, more = 9_001, 777
    vals = _random_attr(rng, n + more)
    col = _random_tags(rng, n + more)
    keys = [1, 5, 9, 11]
    with HipVectorIndex(D, L2, capacity_rows=n + more) as idx:
        idx.append(0, _ones(n))
        live = np.ones(n, bool)
        with idx.make_attr(vals) as attr, idx.make_tags(col) as tags:
            dense = rng.random(n) < 0.7
            sel = np.zeros(n, bool)
            sel[rng.choice(n, 37, replace=False)] = True  # selective: the part keeps a list beside its words
            short = rng.random(n // 3) < 0.5  # shorter than the index: the rows beyond it are not kept
            none = np.zeros(n, bool)
            masks = [(idx.make_mask(_bits(k)), k) for k in (dense, sel, short, none)]
            rkeep = (_v(vals, n) != NULL) & (_v(vals, n) <= 6)
            masks.append((idx.make_mask_where(attr, I64_MIN + 1, 6), rkeep))
            for m, k in masks:
                got = _attr_ok(idx, attr, vals, live, keys, "values", m, k)
                assert got[3] == _count(idx, m) == int(_P(live, k).sum())
                _attr_ok(idx, attr, vals, live, [2, 6], "edges", m, k)
                _tags_ok(idx, tags, col, live, [3, 17, 22], m, k)
            # the masks were made before this append: their parts are rebuilt for the grown shard and keep no new row
            idx.append(n, _ones(more))
            live = np.ones(n + more, bool)
            for m, k in masks:
                got = _attr_ok(idx, attr, vals, live, keys, "values", m, k)
                assert got[3] == _count(idx, m) == int(_P(live, k).sum())
                _tags_ok(idx, tags, col, live, [3, 17, 22], m, k)
            assert _attr_ok(idx, attr, vals, live, keys)[3] == n + more
            for m, _ in masks:
                m.close()


# ---- 5. the population --------------------------------------------------------------------------------------------------------
def test_population(hip_lib):
    """tombstones, a gap left by an append, overwritten rows, quarantined rows kept by the mask and not, a column shorter
    than the index, and a _set seen by the next call"""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(5)
    a, gap, b = 3_000, 130, 1_500
    n = a + gap + b
    vals = _random_attr(rng, n - 400)  # shorter than the index
    col = _random_tags(rng, n - 400)
    lists = [col[1][col[0][i]:col[0][i + 1]].tolist() for i in range(n - 400)]
    keys, tkeys = [0, 3, 7, 11, 50], [3, 17, 22, 50]
    with HipVectorIndex(D, L2, capacity_rows=n + 64) as idx:
        idx.append(0, _ones(a))
        idx.append(a + gap, _ones(b))  # rows a .. a + gap - 1 were never written
        live = np.ones(n, bool)
        live[a:a + gap] = False
        assert idx.size == n and _count(idx) == a + b
        attr, tags = idx.make_attr(vals), idx.make_tags(col)
        keep = rng.random(n) < 0.5
        mk = idx.make_mask(_bits(keep))

        def check(what):
            for m, k in ((None, None), (mk, keep)):
                got = _attr_ok(idx, attr, vals, live, keys, "values", m, k, what)
                assert got[3] == _count(idx, m), what
                _attr_ok(idx, attr, vals, live, [1, 4, 8], "edges", m, k, what)
                got = _tags_ok(idx, tags, _csr(lists), live, tkeys, m, k, what)
                assert got[3] == _count(idx, m), what

        check("gap")
        dead = rng.choice(np.flatnonzero(live), 500, replace=False)
        idx.set_deleted(dead)
        live[dead] = False
        check("tombstones")
        idx.append(100, _ones(200))  # overwritten rows are rows again, tombstoned or not
        live[100:300] = True
        check("overwritten")
        # quarantined rows: a non-finite element.  Rows 10 .. 15 (half kept by the mask, half not), a word's last lane, the last row
        bad = _ones(1)
        bad[0, 3] = np.inf
        q_ids = [10, 11, 12, 13, 14, 15, 63, 64, n - 1]
        keep[10:13], keep[13:16] = True, False
        mk.close()
        mk = idx.make_mask(_bits(keep))
        for r in q_ids:
            idx.append(r, bad)
            live[r] = True
        c = idx.counters()
        assert c["quarantined_rows"] == len(q_ids) and not c["safe_mode"]
        check("quarantined")
        idx.set_deleted([11, 14])  # a tombstoned quarantined row leaves P
        live[[11, 14]] = False
        check("quarantined and tombstoned")
        # _set is seen by the next call: an overwrite inside, then an extension past the old end over a gap of NULL rows
        vals = np.concatenate([vals, np.full(100, NULL), np.full(150, 50)]).astype(np.int64)
        vals[5:25] = 50
        attr.set(5, vals[5:25])
        attr.set(n - 300, vals[n - 300:n - 150])
        new_mid = [[50], [], [3, 17, 22], [NULL, 3]] * 5
        lists[5:25] = new_mid
        tags.set(5, new_mid)
        lists += [[NULL]] * 100 + [[50, 3]] * 150
        tags.set(n - 300, [[50, 3]] * 150)
        check("set")
        new_live = int(live[n - 300:n - 150].sum())  # (the rows the extension gave the value 50, tombstones taken off)
        assert new_live > 100 and idx.facets(attr, [50])[0][0] >= new_live and idx.facets(tags, [50])[0][0] >= new_live
        for h in (mk, attr, tags):
            h.close()


def test_a_shard_in_safe_mode(hip_lib):
    """QUARANTINE_MAX + 1 = 1 025 irregular rows: the shard leaves the quarantine route.  The first 1 024 are on the host's
    list with their live bits clear, the rest keep their live bits; P is the same rows either way"""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(6)
    n, n_bad = 3_001, 1_025
    rows = _ones(n)
    bad = rng.choice(n, n_bad, replace=False)
    rows[bad, 2] = np.nan
    vals = _random_attr(rng, n)
    col = _random_tags(rng, n)
    live = np.ones(n, bool)
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, rows)
        assert idx.counters()["safe_mode"]
        keep = rng.random(n) < 0.5
        with idx.make_attr(vals) as attr, idx.make_tags(col) as tags, idx.make_mask(_bits(keep)) as mk:
            for m, k in ((None, None), (mk, keep)):
                got = _attr_ok(idx, attr, vals, live, [0, 3, 7, 11])
                assert got[3] == _count(idx) == n
                got = _attr_ok(idx, attr, vals, live, [0, 3, 7, 11], "values", m, k)
                assert got[3] == _count(idx, m)
                _tags_ok(idx, tags, col, live, [3, 17, 22], m, k)
            dead = np.concatenate([bad[:40], np.setdiff1d(np.arange(n), bad)[:40]])
            idx.set_deleted(dead)
            live[dead] = False
            got = _attr_ok(idx, attr, vals, live, [0, 3, 7, 11], "values", mk, keep)
            assert got[3] == _count(idx, mk)
            _tags_ok(idx, tags, col, live, [3, 17, 22])


# ---- 6. tag spans -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [1, 63])
def test_tag_spans(hip_lib, tail):
    """a word whose span ends `tail` values into a pass of 64; empty sets; NULL rows; a row whose list crosses a pass; a
    key held by every non-NULL row"""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(tail)
    n = 64 * 3 + 17
    lists = [[1000] + rng.choice(50, int(rng.integers(0, 4)), replace=False).tolist() for _ in range(n)]
    lists[3] = []
    lists[4] = [NULL]
    lists[5] = [7, NULL, 1000]
    lists[70] = [1000] + list(range(100, 100 + 150))  # crosses two pass edges
    lists[127] = []
    lists[128] = [1000] + list(range(200, 200 + 64))
    # word 0's span: a multiple of 64 plus `tail`
    lists[9] = []
    span0 = sum(len(set(r)) if NULL not in r else 0 for r in lists[:64])
    lists[9] = [1000] + list(range(300, 300 + ((tail - span0 - 1) % 64 or 64)))
    assert sum(len(set(r)) if NULL not in r else 0 for r in lists[:64]) % 64 == tail
    col = _csr(lists)
    live = np.ones(n, bool)
    keep = rng.random(n) < 0.6
    keep[[3, 4, 70]] = True
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, _ones(n))
        with idx.make_tags(col) as tags, idx.make_mask(_bits(keep)) as mk:
            for m, k in ((None, None), (mk, keep)):
                got = _tags_ok(idx, tags, col, live, [1000, 7, 249, 101, 263, 300, 12, NULL, 7], m, k)
                P = _P(live, k)
                assert got[0][0] == int(P.sum()) - got[2] - int(P[[3, 127]].sum())  # every non-NULL, non-empty row holds 1000
                got = _tags_ok(idx, tags, col, live, [12], m, k)
                assert got[1] >= int(P[[3, 127]].sum())  # empty sets are "other"
                _tags_ok(idx, tags, col, live, list(range(0, 50)) + list(range(100, 250)), m, k)
            idx.set_deleted([70, 3])
            live[[70, 3]] = False
            _tags_ok(idx, tags, col, live, [1000, 101, 12])


# ---- 7. cross-checks against the entries that exist ---------------------------------------------------------------------------
def test_counts_are_search_counts_under_the_keys_masks(hip_lib):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(7)
    n = 6_007
    rows = rng.standard_normal((n, D)).astype(np.float32)
    rows[[5, 700], 1] = np.inf  # two quarantined rows
    vals = _random_attr(rng, n - 50)
    col = _random_tags(rng, n - 50)
    q = rng.standard_normal(D).astype(np.float32)
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, rows)
        idx.set_deleted(rng.choice(n, 300, replace=False))
        keep = rng.random(n) < 0.5
        with idx.make_attr(vals) as attr, idx.make_tags(col) as tags, idx.make_mask(_bits(keep)) as mk:
            for mask in (None, mk):
                keys = np.array([0, 3, 7, 11, 99], np.int64)
                counts, other, null, total = idx.facets(attr, keys, mask)
                assert total == int(idx.search_count(q, None, mask)[0])
                for j, key in enumerate(keys):
                    with idx.make_mask_where(attr, int(key), int(key), with_mask=mask) as mj:
                        assert counts[j] == int(idx.search_count(q, None, mj)[0]), key
                with idx.make_mask_where(attr, I64_MIN + 1, I64_MAX, with_mask=mask) as mnn:
                    assert total - null == int(idx.search_count(q, None, mnn)[0])
                assert int(counts.sum()) + other + null == total
                tkeys = np.array([3, 17, 22, 999], np.int64)
                counts, other, null, total = idx.facets(tags, tkeys, mask)
                assert total == int(idx.search_count(q, None, mask)[0])
                for j, key in enumerate(tkeys):
                    with idx.make_mask_tags(tags, [int(key)], "any", with_mask=mask) as mj:
                        assert counts[j] == int(idx.search_count(q, None, mj)[0]), key
                with idx.make_mask_tags(tags, tkeys, "any", True, with_mask=mask) as mo:  # non-NULL rows that hold none
                    assert other == int(idx.search_count(q, None, mo)[0])


# ---- 8. shard handles and several devices -------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,n", [(12_353, 5_005), (12_837, 4_999)])
def test_shard_handle_counts_its_own_rows_by_global_id(hip_lib, base, n):
    from tostore_amd import HipVectorIndex

    assert base % 64 in (1, 37) and n % 64 != 0
    rng = np.random.default_rng(base)
    total = base + n + 203
    rows = _ones(n)
    rows[17, 0] = np.inf  # a quarantined row: the host reads the column at row_base + 17
    for length in (total, base + n - 70, base + 17):  # by GLOBAL row id: past the shard, ending inside it, barely reaching it
        vals = _random_attr(rng, length)
        col = _random_tags(rng, length)
        live = np.zeros(base + n, bool)
        live[base:] = True
        keep = rng.random(total) < 0.5
        with HipVectorIndex(D, L2, capacity_rows=n, shard_device=0, row_base=base) as idx:
            idx.append(base, rows)
            with idx.make_attr(vals) as attr, idx.make_tags(col) as tags, idx.make_mask(_bits(keep)) as mk:
                for m, k in ((None, None), (mk, keep)):
                    got = _attr_ok(idx, attr, vals, live, [0, 3, 7, 11], "values", m, k)
                    assert got[3] == _count(idx, m)
                    _attr_ok(idx, attr, vals, live, [2, 5], "edges", m, k)
                    _tags_ok(idx, tags, col, live, [3, 17, 22], m, k)


def test_in_process_shards(hip_lib):
    """n_devices = 3 in one process (sharing the one GPU), as tests/test_gpu_mask_tags.py makes one: the library sums its
    shards; the second shard ends inside a word and the third is empty, or all three hold rows"""
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(77)
    os.environ["TSH_SHARDS_SHARE_DEVICES"] = "1"
    _ffi.enable_test_hooks()
    try:
        for cap, n in ((70_000, 30_001), (70_001, 50_003)):
            rows = _ones(n)
            rows[[3, 25_000, n - 1], 0] = np.inf
            live = np.ones(n, bool)
            for length in (n - 77, n + 30):
                vals, col = _random_attr(rng, length), _random_tags(rng, length)
                keep = rng.random(n) < 0.5
                with HipVectorIndex(D, L2, capacity_rows=cap, n_devices=3) as idx:
                    idx.append(0, rows)
                    with idx.make_attr(vals) as attr, idx.make_tags(col) as tags, idx.make_mask(_bits(keep)) as mk:
                        for m, k in ((None, None), (mk, keep)):
                            got = _attr_ok(idx, attr, vals, live, [0, 3, 7, 11], "values", m, k)
                            assert got[3] == _count(idx, m)
                            _attr_ok(idx, attr, vals, live, [2, 5], "edges", m, k)
                            _tags_ok(idx, tags, col, live, [3, 17, 22], m, k)
    finally:
        _ffi.enable_test_hooks(False)
        del os.environ["TSH_SHARDS_SHARE_DEVICES"]


# ---- 9. lifetime and errors ---------------------------------------------------------------------------------------------------
def test_orphans_foreign_handles_and_an_empty_index(hip_lib):
    from tostore_amd import _ffi

    L = _ffi.lib()
    rows = np.random.default_rng(7).standard_normal((100, D)).astype(np.float32)
    vals = (np.arange(100) % 5).astype(np.int64)
    off, tv = _csr([[i % 5, 10 + i % 3] for i in range(100)])
    pa, po, pt = (x.ctypes.data_as(_ffi.p_i64) for x in (vals, off, tv))
    keys = np.array([2, 1, 1], np.int64)
    pk = keys.ctypes.data_as(_ffi.p_i64)
    SENT = -77

    def index(fill=True):
        h = ctypes.c_void_p()
        _ffi.check(L.tsh_index_create(D, L2, 0, 1, ctypes.byref(h)))
        if fill:
            _ffi.check(L.tsh_index_append(h, 0, 100, rows.ctypes.data_as(_ffi.p_f32)))
        return h

    def facets(idx, attr=None, tags=None, mask=None):
        counts, rest = np.full(3, SENT, np.int64), np.full(3, SENT, np.int64)
        pc, pr = counts.ctypes.data_as(_ffi.p_i64), rest.ctypes.data_as(_ffi.p_i64)
        rc = L.tsh_attr_facets(idx, attr, mask, 0, pk, 3, pc, pr) if attr else L.tsh_tags_facets(idx, tags, mask, pk, 3, pc, pr)
        return rc, counts.tolist(), rest.tolist()

    untouched = ([SENT] * 3, [SENT] * 3)
    a, b, e = index(), index(), index(False)
    attr_a, attr_b, tags_a, tags_b, mask_a, mask_b, attr_e, tags_e = (ctypes.c_void_p() for _ in range(8))
    ones = np.full(13, 0xFF, np.uint8)
    for idx, attr, tags, mask in ((a, attr_a, tags_a, mask_a), (b, attr_b, tags_b, mask_b)):
        _ffi.check(L.tsh_attr_create(idx, pa, 100, ctypes.byref(attr)))
        _ffi.check(L.tsh_tags_create(idx, po, 100, pt, ctypes.byref(tags)))
        _ffi.check(L.tsh_mask_create(idx, ones.ctypes.data_as(_ffi.p_u8), 13, ctypes.byref(mask)))
    assert facets(a, attr=attr_a, mask=mask_a) == (0, [20, 20, 20], [60, 0, 100])
    assert facets(a, tags=tags_a, mask=mask_a) == (0, [20, 20, 20], [60, 0, 100])
    # a column of another index; a mask of another index
    for kw in (dict(attr=attr_b), dict(tags=tags_b), dict(attr=attr_a, mask=mask_b), dict(tags=tags_a, mask=mask_b)):
        rc, counts, rest = facets(a, **kw)
        assert rc == _ffi.TSH_E_BAD_ARG and "another index" in _ffi.last_error() and (counts, rest) == untouched, kw
    # an empty index gives zeros
    _ffi.check(L.tsh_attr_create(e, pa, 100, ctypes.byref(attr_e)))
    _ffi.check(L.tsh_tags_create(e, po, 100, pt, ctypes.byref(tags_e)))
    assert facets(e, attr=attr_e) == (0, [0, 0, 0], [0, 0, 0]) and facets(e, tags=tags_e) == (0, [0, 0, 0], [0, 0, 0])
    # index a goes first: its handles are orphaned, not dangling
    _ffi.check(L.tsh_index_destroy(a))
    for kw in (dict(attr=attr_a), dict(tags=tags_a), dict(attr=attr_b, mask=mask_a), dict(tags=tags_b, mask=mask_a)):
        rc, counts, rest = facets(b, **kw)
        assert rc == _ffi.TSH_E_BAD_ARG and (counts, rest) == untouched, kw
    assert facets(b, attr=attr_b, mask=mask_b)[0] == 0
    for h, destroy in ((attr_a, L.tsh_attr_destroy), (tags_a, L.tsh_tags_destroy), (mask_a, L.tsh_mask_destroy), (attr_b, L.tsh_attr_destroy),
                       (attr_e, L.tsh_attr_destroy), (tags_e, L.tsh_tags_destroy)):
        assert destroy(h) == _ffi.TSH_OK
    assert L.tsh_index_destroy(b) == _ffi.TSH_OK and L.tsh_index_destroy(e) == _ffi.TSH_OK
    assert L.tsh_tags_destroy(tags_b) == _ffi.TSH_OK and L.tsh_mask_destroy(mask_b) == _ffi.TSH_OK


# ---- 10. threads --------------------------------------------------------------------------------------------------------------
def test_calls_share_the_handles_beside_a_setter_and_searches(hip_lib):
    """Six threads count facets of one attribute and one tag handle while a seventh overwrites both columns, alternating
    between two known columns, and an eighth searches: every answer is NumPy's for one of the two columns whole, never a
    mixture, and the last call sees the last _set."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(10)
    n = 20_001
    live = np.ones(n, bool)
    va, vb = _random_attr(rng, n), _random_attr(rng, n, universe=6)
    ca, cb = _random_tags(rng, n, max_len=8), _random_tags(rng, n, max_len=5)
    keep = rng.random(n) < 0.5
    keys, tkeys = [0, 3, 5, 11], [3, 17, 22]
    P = _P(live, keep)
    a_answers = [_attr_spec(v, P, keys) for v in (va, vb)]
    t_answers = [_tags_spec(c, P, tkeys) for c in (ca, cb)]
    assert not np.array_equal(a_answers[0][0], a_answers[1][0]) and not np.array_equal(t_answers[0][0], t_answers[1][0])
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, rng.standard_normal((n, D)).astype(np.float32))
        attr, tags, mk = idx.make_attr(va), idx.make_tags(ca), idx.make_mask(_bits(keep))
        start, stop = threading.Barrier(8), threading.Event()
        got, errors, sets = [[] for _ in range(6)], [], [0]

        def counter(which):
            try:
                start.wait(30)
                while not stop.is_set():
                    got[which].append(("a", idx.facets(attr, keys, mk)) if which % 2 else ("t", idx.facets(tags, tkeys, mk)))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        def setter():
            try:
                start.wait(30)
                for _ in range(24):
                    sets[0] += 1
                    attr.set(0, (vb, va)[sets[0] % 2])
                    tags.set(0, (cb, ca)[sets[0] % 2])
            except Exception as e:  # noqa: BLE001
                errors.append(e)
            finally:
                stop.set()

        def searcher():
            try:
                start.wait(30)
                q = np.ones(D, np.float32)
                while not stop.is_set():
                    assert idx.search(q, 10, None, mk)[2][0] == 10
                    assert int(idx.search_count(q, None, mk)[0]) == int(P.sum())
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=counter, args=(i,)) for i in range(6)] + [threading.Thread(target=setter), threading.Thread(target=searcher)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        assert not any(t.is_alive() for t in threads), "a thread is still waiting: deadlock"
        assert not errors, errors
        assert sets[0] == 24 and all(len(g) >= 1 for g in got)
        for g in got:
            for kind, ans in g:
                want = a_answers if kind == "a" else t_answers
                assert any(np.array_equal(ans[0], w[0]) and tuple(ans[1:]) == tuple(w[1:]) for w in want), "an answer mixes the two columns"
        _attr_ok(idx, attr, (vb, va)[sets[0] % 2], live, keys, "values", mk, keep)
        _tags_ok(idx, tags, (cb, ca)[sets[0] % 2], live, tkeys, mk, keep)
        for h in (mk, attr, tags):
            h.close()


# ---- 11. fuzz -----------------------------------------------------------------------------------------------------------------
def test_sequence_fuzz(hip_lib):
    """A seeded sequence of appends (extending, overwriting, leaving gaps, now and then a non-finite row), deletes, _sets
    and facet calls on one index, the model beside it."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(2025)
    calls = 0
    for round_ in range(4):
        cap = 6_000
        live = np.zeros(0, bool)
        vals = np.zeros(0, np.int64)
        lists = []
        universe = int(rng.choice([8, 40, 3000]))
        with HipVectorIndex(D, L2, capacity_rows=cap) as idx:
            idx.append(0, _ones(70))
            live = np.ones(70, bool)
            attr, tags = idx.make_attr(vals), idx.make_tags(_csr(lists))
            masks = []
            for step in range(40):
                op = int(rng.integers(0, 10))
                n = len(live)
                if op <= 1 and n < cap - 700:  # append: extend (sometimes over a gap) or overwrite
                    cnt = int(rng.integers(1, 500))
                    first = int(rng.choice([n, n, n + int(rng.integers(1, 130)), int(rng.integers(0, n))]))
                    rows = _ones(cnt)
                    if rng.random() < 0.3:
                        rows[int(rng.integers(0, cnt)), 0] = np.inf
                    idx.append(first, rows)
                    if first + cnt > n:
                        live = np.concatenate([live, np.zeros(first + cnt - n, bool)])
                    live[first:first + cnt] = True
                elif op == 2:
                    dead = rng.choice(n, int(rng.integers(1, 60)), replace=False)
                    dead = dead[live[dead]]
                    if len(dead):
                        idx.set_deleted(dead)
                        live[dead] = False
                elif op == 3:
                    first, cnt = int(rng.integers(0, n + 40)), int(rng.integers(1, 400))
                    new = _random_attr(rng, cnt, universe)
                    if first + cnt > len(vals):
                        vals = np.concatenate([vals, np.full(first + cnt - len(vals), NULL, np.int64)])
                    vals[first:first + cnt] = new
                    attr.set(first, new)
                elif op == 4:
                    first, cnt = int(rng.integers(0, n + 40)), int(rng.integers(1, 400))
                    c = _random_tags(rng, cnt, universe)
                    new = [c[1][c[0][i]:c[0][i + 1]].tolist() for i in range(cnt)]
                    if first > len(lists):
                        lists += [[NULL]] * (first - len(lists))
                    lists[first:first + cnt] = new
                    tags.set(first, new)
                elif op == 5 and len(masks) < 4:
                    keep = rng.random(int(rng.integers(1, n + 1))) < rng.random()  # (often shorter than the index)
                    masks.append((idx.make_mask(_bits(keep)), keep))
                else:
                    m, k = masks[int(rng.integers(0, len(masks)))] if masks and rng.random() < 0.6 else (None, None)
                    size = int(rng.choice([0, 1, 3, 20, 700]))
                    ks = rng.integers(-2, universe + 2, size).astype(np.int64)
                    if size and rng.random() < 0.3:
                        ks[0] = NULL
                    got = _attr_ok(idx, attr, vals, live, ks, "values", m, k, (round_, step))
                    assert got[3] == _count(idx, m), (round_, step)
                    e = np.unique(ks[ks != NULL])
                    _attr_ok(idx, attr, vals, live, e, "edges", m, k, (round_, step))
                    _tags_ok(idx, tags, _csr(lists), live, ks, m, k, (round_, step))
                    calls += 1
            for m, _ in masks:
                m.close()
            attr.close()
            tags.close()
    assert calls >= 40
