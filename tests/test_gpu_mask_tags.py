"""GPU: a HAS ANY / HAS ALL term over a tag column made into a mask handle on the device (tsh_tags_create / _set / _destroy,
tsh_mask_create_tags; T1 mask_tags_kernel of tostore_amd/csrc/tsh_tags.hip.h, its host side tsh_tags_plan.h).  NumPy on
the host is the specification (_spec) and the answer is exact: the handle's bitmap is NumPy's byte for byte through
tsh_mask_read, its kept count NumPy's popcount, no bit at or past the last row; and a search with the handle is bit for
bit -- ids, distances, route -- the search with a tsh_mask_create handle made from NumPy's bitmap.  The sizes are the
smallest at which this kernel can still go wrong: a wave's word of 64 rows, its passes of 64 values, the grid's cap (a
second grid-stride word per wave), mask_finish_part's list threshold at 4096 rows.  d = 8 throughout: the rows only have
to be there."""
import ctypes
import os
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2, IP, COS = 0, 1, 2
D = 8
NULL, I64_MIN, I64_MAX = -(1 << 63), -(1 << 63), (1 << 63) - 1
ROUTE = ("exact_scans", "list_scans", "batch_launches", "fallback_searches")


# ---- the column as a caller holds it: CSR (offsets, values) ------------------------------------------------------------------
def _csr(lists):
    lens = np.array([len(r) for r in lists], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    vals = np.concatenate([np.asarray(r, np.int64).reshape(-1) for r in lists]) if len(lists) else np.zeros(0, np.int64)
    return off, vals.astype(np.int64)


def _lists(col):
    off, vals = col
    return [vals[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _spec(col, n, S, need="any", negate=False):
    """The specification.  Row i < n of the column (offsets, values): NULL if beyond the column or if its list holds NULL;
    c_i = distinct values of its list that are in S (S without duplicates and NULL); kept iff not NULL and
    (c_i >= t) != negate, t = |S| for "all", 1 for "any", else the count given."""
    off, vals = col
    m = min(n, len(off) - 1)
    S = np.unique(np.asarray([s for s in S if s != NULL], np.int64))
    t = len(S) if need == "all" else (1 if need == "any" else int(need))
    owner = np.repeat(np.arange(len(off) - 1), np.diff(off))
    owner, vals = owner[owner < m], vals[:off[m]]
    is_null = np.bincount(owner[vals == NULL], minlength=m) > 0
    order = np.lexsort((vals, owner))
    o, v = owner[order], vals[order]
    first = np.ones(len(v), bool)
    first[1:] = (v[1:] != v[:-1]) | (o[1:] != o[:-1])  # (a value the caller gave a row twice counts once)
    c = np.bincount(o[first & np.isin(v, S)], minlength=m)
    keep = np.zeros(n, bool)
    keep[:m] = ~is_null & ((c >= t) != negate)
    return keep


def _bits(keep, n_bytes=None):
    b = np.packbits(np.asarray(keep, bool), bitorder="little")
    if n_bytes is not None:
        b = np.concatenate([b, np.zeros(n_bytes - len(b), np.uint8)])
    return b


def _holds(m, keep, n_rows_end, slack=9):
    """the handle's bitmap is `keep` (bit i = GLOBAL row id i) byte for byte, zero past it; kept is its popcount"""
    nb = (n_rows_end + 7) // 8 + slack
    got = m.bits(nb)
    assert got.dtype == np.uint8 and got.shape == (nb,)
    assert np.array_equal(got, _bits(keep, nb)), np.flatnonzero(np.unpackbits(got ^ _bits(keep, nb), bitorder="little"))[:8]
    assert m.kept == int(np.count_nonzero(keep))
    short = m.bits()  # by default one bit per row id the index holds
    assert short.shape == ((m.index.size + 7) // 8,) and np.array_equal(short, got[:len(short)])


def _check(idx, tags, col, n, S, need="any", negate=False, end=None, with_mask=None, with_keep=None, combine="and", slack=9):
    want = _spec(col, n, S, need, negate)
    if with_keep is not None:
        want = (want | with_keep) if combine == "or" else (want & with_keep)
    with idx.make_mask_tags(tags, np.asarray(S, np.int64), need, negate, with_mask=with_mask, combine=combine) as m:
        _holds(m, want, n if end is None else end, slack)
    return want


def _random_column(rng, n, universe=40, max_len=8, p_null=0.08, p_empty=0.15):
    """mostly short lists over a small universe (so that sets of a few values match many rows), duplicates inside a list,
    some rows NULL (the NULL first, last or alone in the list), some empty"""
    lens = rng.integers(1, max_len + 1, n)
    lens[rng.random(n) < p_empty] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    vals = rng.integers(0, universe, off[-1]).astype(np.int64)
    for r in np.flatnonzero((rng.random(n) < p_null) & (lens > 0)):
        vals[off[r] + (0, lens[r] - 1, lens[r] // 2)[r % 3]] = NULL
    return off, vals


def _queries(rng, nq, metric=L2):
    q = rng.standard_normal((nq, D)).astype(np.float32)
    return q / np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32) if metric == COS else q


def _same(a, b, what=""):
    assert np.array_equal(a[2], b[2]), ("counts", what)
    for i, c in enumerate(a[2]):
        assert np.array_equal(a[0][i, :c], b[0][i, :c]), ("ids", what, i)
        assert np.array_equal(a[1][i, :c].view(np.uint64), b[1][i, :c].view(np.uint64)), ("distance bits", what, i)


def _pair(idx, qs, k, mb, mr):
    """the bitmap-made and the tags-made handle of one row set: the same answer by the same route -> that route"""
    c0 = idx.counters()
    a = idx.search(qs, k, None, mb)
    c1 = idx.counters()
    b = idx.search(qs, k, None, mr)
    c2 = idx.counters()
    _same(a, b)
    ra = {c: c1[c] - c0[c] for c in ROUTE}
    rb = {c: c2[c] - c1[c] for c in ROUTE}
    assert ra == rb, ("the bitmap handle and the tags handle took different routes", ra, rb)
    if ra["batch_launches"]:
        assert c1["batch_kernel_last"] == c2["batch_kernel_last"]
    assert ra["fallback_searches"] == 0
    return ra


# ---- 1. rows ------------------------------------------------------------------------------------------------------------------
# 4096 is where mask_finish_part starts listing; 524 353 = 2048 workgroups x 4 words x 64 rows + 65: the grid is at its cap
# there and a wave takes a second grid-stride word, 8192 words after its first
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 4095, 4096, 4097, 524_353])
def test_rows_are_numpys(hip_lib, n):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(n)
    cap = n + 479
    rows = np.zeros((n, D), np.float32)
    rows[:, 0] = 1
    X = 777_777  # in no list but the planted ones
    off, vals = _random_column(rng, n + 70)  # 70 rows longer than the index: they must not be read into the result
    planted = {}
    if n == 524_353:
        # lane 7 matches in word w and not in word w + 8192, lane 9 the other way round, for w = 0 and 1: a counter that
        # is not zeroed between a wave's words shows as a kept row that holds nothing of the set
        for w in (0, 1):
            for lane, first in ((7, True), (9, False)):
                for word, match in ((w, first), (w + 8192, not first)):
                    r = word * 64 + lane
                    if r < n:
                        planted[r] = match
        lens = np.diff(off)
        for r in planted:
            lens[r] = 1
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        vals = rng.integers(0, 40, off[-1]).astype(np.int64)
        vals[rng.random(len(vals)) < 0.01] = NULL
        for r, match in planted.items():
            vals[off[r]] = X if match else 41
        assert len(planted) >= 6
    col = (off, vals)
    short = (off[:n - (n + 2) // 3 + 1], vals)  # ... and a column that ends inside the index
    with HipVectorIndex(D, L2, capacity_rows=cap) as idx:
        idx.append(0, rows)
        with idx.make_tags(col) as tags, idx.make_tags(short) as tshort:
            if planted:
                for negate in (False, True):
                    want = _check(idx, tags, col, n, [X], "any", negate)
                    for r, match in planted.items():
                        assert want[r] == (match != negate)
            terms = [([3], "any", False), ([3, 17, 22, 39], "any", True), ([3, 17], "all", False), ([5, 6, 7, 8, 9, 10], 2, True)]
            if not planted:  # (at the large size NumPy's side is what takes the time: the four above, each way once)
                terms += [(S, need, not negate) for S, need, negate in terms] + [([], "all", False), ([], "all", True), ([], "any", False),
                                                                                  ([], "any", True)]
            for S, need, negate in terms:
                _check(idx, tags, col, n, S, need, negate)
            _check(idx, tshort, short, n, [1, 2, 3], "any")
            _check(idx, tshort, short, n, [1, 2, 3], "any", True)
            # `with` under AND and OR: a capacity-sized bitmap with every bit past the last row set -- none comes through
            w = rng.random(n) < 0.3
            full = np.ones(cap, bool)
            full[:n] = w
            with idx.make_mask(_bits(full)) as mw:
                _check(idx, tags, col, n, [3, 17, 22], "any", False, end=cap, with_mask=mw, with_keep=w, combine="and", slack=70)
                _check(idx, tshort, short, n, [4], "any", True, end=cap, with_mask=mw, with_keep=w, combine="or", slack=70)
                if not planted:
                    _check(idx, tags, col, n, [3, 17, 22], "any", False, end=cap, with_mask=mw, with_keep=w, combine="or", slack=70)
                    _check(idx, tshort, short, n, [4], "any", True, end=cap, with_mask=mw, with_keep=w, combine="and", slack=70)


# ---- 2. spans -----------------------------------------------------------------------------------------------------------------
def _distinct(rng, k, lo=0, hi=10_000):
    return rng.choice(hi - lo, k, replace=False).astype(np.int64) + lo


@pytest.mark.parametrize("tail", [1, 63])
def test_spans_are_numpys(hip_lib, tail):
    """Words built one by one: every row an empty set; every row NULL; one row of 5000 values alone; lists of 63, 64, 65 and
    128 values that begin and end on the edges of the word's 64-value passes; spans of 0, 1, 64 and 65 values; and a ragged
    last word under a column that goes on past the index."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(tail)
    lists = []
    lists += [[] for _ in range(64)]                                   # word 0: all empty (a span of 0 values)
    lists += [[NULL] if r % 2 else [4, NULL, 9] for r in range(64)]    # word 1: all NULL
    w2 = [[] for _ in range(64)]
    w2[17] = _distinct(rng, 5000)                                      # word 2: 5000 values, 79 passes, one owner
    lists += w2
    w3 = [[] for _ in range(64)]                                       # word 3: 64 | 128 | 63 + 1 | 65 + 63 = 6 passes exactly
    for r, k in zip((0, 1, 5, 6, 40, 63), (64, 128, 63, 1, 65, 63)):
        w3[r] = _distinct(rng, k)
    lists += w3
    w4 = [[] for _ in range(64)]
    w4[63] = [7]                                                       # word 4: a span of 1 value, owned by the last lane
    lists += w4
    lists += [[int(v)] for v in rng.integers(0, 12, 64)]              # word 5: a span of 64 values, one per row
    w6 = [[int(v)] for v in rng.integers(0, 12, 64)]
    w6[31] = [3, 7]                                                    # word 6: a span of 65 values
    lists += w6
    lists += [list(_distinct(rng, int(k), 0, 12)) for k in rng.integers(0, 5, tail)]  # the ragged last word ...
    n = len(lists)
    assert n == 7 * 64 + tail
    lists += [[3, 7, 5000 + j] for j in range(100)]                    # ... and rows beyond the index that would match
    col = _csr(lists)
    rows = np.ones((n, D), np.float32)
    big, edge = np.asarray(lists[2 * 64 + 17]), np.asarray(lists[3 * 64 + 1])
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, rows)
        with idx.make_tags(col) as tags:
            sets = [([3, 7], "any"), ([3, 7], "all"), ([7], "any"), (list(big[::7]), 700), (list(big[::7]), 800), (list(big[:4096]), "all"),
                    (list(big[:4096]), 4096), (list(edge), "all"), (list(edge) + [10_001], "all"), (list(edge[:64]), 64),
                    (list(np.asarray(lists[3 * 64 + 40])[[0, 63, 64]]), 3), (list(np.asarray(lists[3 * 64 + 63])[[0, 62]]) + [7], 2),
                    (list(range(12)), 1), ([], "all"), ([], "any")]
            for S, need in sets:
                for negate in (False, True):
                    want = _check(idx, tags, col, n, S, need, negate)
                    assert not want[64:128].any()          # NULL rows are kept by no term
                    assert not want[n:].any()
            want = _spec(col, n, list(big[::7]), 700)
            assert want[2 * 64 + 17] and want.sum() == 1   # 715 of the 5000 are in the set
            assert _spec(col, n, list(edge), "all")[3 * 64 + 1] and _spec(col, n, [], "all")[:64].all()


# ---- 3. counters --------------------------------------------------------------------------------------------------------------
def test_counters_are_wide_enough_and_count_sets(hip_lib):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(3)
    n = 200
    S300, S4096 = _distinct(rng, 300, 0, 100_000), _distinct(rng, 4096, 200_000, 300_000)
    lists = [list(_distinct(rng, int(k), 0, 100_000)) for k in rng.integers(0, 6, n)]
    lists[70] = list(rng.permutation(S300))                            # all 300, and not a value more
    lists[71] = list(rng.permutation(np.concatenate([S300[:256], [100_001]])))
    lists[72] = list(rng.permutation(np.concatenate([S300[:255], S300[:255]])))  # 255 of them, each given twice
    lists[130] = list(rng.permutation(S4096))
    lists[131] = list(S4096[:4095])
    lists[5] = [42, 42, 42, 42, 42]                                    # one value five times: a set of one
    lists[6] = [42, 43, 42]
    col = _csr(lists)
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, np.ones((n, D), np.float32))
        with idx.make_tags(col) as tags:
            for need, rows_kept in ((255, {70, 71, 72}), (256, {70, 71}), (257, {70}), (300, {70}), ("all", {70}), (301, set())):
                want = _check(idx, tags, col, n, S300, need)
                assert set(np.flatnonzero(want)) == rows_kept, need
                _check(idx, tags, col, n, S300, need, True)
            assert set(np.flatnonzero(_check(idx, tags, col, n, S4096, "all"))) == {130}
            assert set(np.flatnonzero(_check(idx, tags, col, n, S4096, 4095))) == {130, 131}
            _check(idx, tags, col, n, S4096, "all", True)
            want = _check(idx, tags, col, n, [42, 43, 44], 2)
            assert not want[5] and want[6]
            assert _check(idx, tags, col, n, [42], 1)[5]


# ---- 4. sets ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [0, 1, 2, 3, 4095, 4096])
def test_sets_are_numpys(hip_lib, size):
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(100 + size)
    n = 4_097
    members = _distinct(rng, size, 0, 1 << 20) * 3 - (1 << 20)  # multiples of 3: their neighbours are no members
    if size >= 2:
        members[0], members[1] = I64_MIN + 1, I64_MAX
    pool = np.concatenate([[I64_MIN + 1, I64_MIN + 2, I64_MAX, I64_MAX - 1, 0, -1, 1], members, members[2:] - 1, members[2:] + 1,
                           rng.integers(-(1 << 21), 1 << 21, 64)]).astype(np.int64)
    lens = rng.integers(0, 7, n)
    lens[10] = 3
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    vals = pool[rng.integers(0, len(pool), off[-1])]
    vals[rng.random(len(vals)) < 0.02] = NULL
    vals[off[10]:off[11]] = I64_MAX, 5, I64_MIN + 1  # (both ends of the value range in one row, whatever the draw)
    col = (off, vals)
    # as a caller hands it over: any order, some values twice, NULLs among them
    given = rng.permutation(np.concatenate([members, members[: size // 3], [NULL, NULL]]))
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, np.ones((n, D), np.float32))
        with idx.make_tags(col) as tags:
            for need in ("any", "all", 2):
                for negate in (False, True):
                    assert np.array_equal(_check(idx, tags, col, n, given, need, negate), _spec(col, n, members, need, negate))
            if size >= 2:
                ends = _spec(col, n, [I64_MIN + 1, I64_MAX], "all")
                assert ends.any() and np.array_equal(_check(idx, tags, col, n, [I64_MAX, NULL, I64_MIN + 1], "all"), ends)
            if size == 0:
                _check(idx, tags, col, n, [], "any")  # (a NULL pointer with n_set == 0)
            if size == 4096:  # one distinct value more is refused, and nothing is made
                with pytest.raises(_ffi.TshError) as e:
                    idx.make_mask_tags(tags, np.concatenate([given, [12_345_678]]))
                assert e.value.code == _ffi.TSH_E_BAD_ARG and "TSH_TAGS_MAX_SET_VALUES" in str(e.value)


# ---- 5. the semantics table ---------------------------------------------------------------------------------------------------
def test_semantics_table(hip_lib):
    """need x negate x with on one column of 4097 rows with NULL rows, empty rows and rows beyond the column; `with` made
    from a bitmap, from a range, from a clause and from another tags call"""
    from tostore_amd import HipVectorIndex, WhereIn

    rng = np.random.default_rng(5)
    n, have = 4_097, 3_900
    col = _random_column(rng, have, universe=12, max_len=6)
    attr_col = rng.integers(0, 10, n).astype(np.int64)
    S = [2, 5, 7]
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, np.ones((n, D), np.float32))
        wb = rng.random(n) < 0.4
        with idx.make_tags(col) as tags, idx.make_attr(attr_col) as attr, idx.make_mask(_bits(wb)) as m_bitmap, \
                idx.make_mask_where(attr, 2, 6) as m_range, idx.make_mask_clauses([[WhereIn(attr, [1, 3, 8])]]) as m_where, \
                idx.make_mask_tags(tags, [1, 11], "any", True) as m_tags:
            withs = [(None, None), (m_bitmap, wb), (m_range, (attr_col >= 2) & (attr_col <= 6)), (m_where, np.isin(attr_col, [1, 3, 8])),
                     (m_tags, _spec(col, n, [1, 11], "any", True))]
            null = ~_spec(col, n, [], "all")
            assert null[have:].all() and null[:have].any() and not null[:have].all()
            empty = np.zeros(n, bool)
            empty[:have] = (np.diff(col[0]) == 0)
            assert empty.any()
            for need in ("all", 1, 2, len(S), len(S) + 1):
                for negate in (False, True):
                    for wm, wk in withs:
                        for combine in (("and",) if wm is None else ("and", "or")):
                            want = _check(idx, tags, col, n, S, need, negate, with_mask=wm, with_keep=wk, combine=combine)
                            if wm is None:
                                assert not (want & null).any()  # a NULL row is kept by no term, negated or not
                                if need == len(S) + 1:          # more than |S|: none; negated: every non-NULL row
                                    assert np.array_equal(want, ~null if negate else np.zeros(n, bool))
                                    assert not negate or (want & empty).any()
            # HAS ALL of nothing keeps every non-NULL row, HAS ANY of nothing none
            assert np.array_equal(_check(idx, tags, col, n, [], "all"), ~null)
            assert not _check(idx, tags, col, n, [NULL], "any").any()


def test_composes_with_a_scalar_clause(hip_lib):
    """tenant = 7 AND acl HAS ANY (...): tsh_mask_create_where, then tsh_mask_create_tags with that handle under AND"""
    from tostore_amd import HipVectorIndex, WhereRange

    rng = np.random.default_rng(55)
    n = 20_001
    tenant = rng.integers(5, 9, n).astype(np.int64)
    tenant[rng.random(n) < 0.1] = NULL
    acl = _random_column(rng, n, universe=200, max_len=8)
    groups = rng.choice(200, 25, replace=False)
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, rng.standard_normal((n, D)).astype(np.float32))
        with idx.make_attr(tenant) as a, idx.make_tags(acl) as t, idx.make_mask_clauses([[WhereRange(a, 7, 7)]]) as mw:
            want = _check(idx, t, acl, n, groups, "any", with_mask=mw, with_keep=tenant == 7)
            assert want.any() and np.array_equal(want, (tenant == 7) & _spec(acl, n, groups))
            with idx.make_mask_tags(t, groups, with_mask=mw) as mr, idx.make_mask(_bits(want)) as mb:
                _pair(idx, _queries(rng, 3), 20, mb, mr)


# ---- 6. search parity and routes ----------------------------------------------------------------------------------------------
def _scan_paths(idx):
    yield "exact"
    idx.set_exact_select(False)
    yield "exact_select"
    idx.set_exact_select(True)
    idx.set_exact_scan_rows(0)
    yield "prefilter"
    idx.set_exact_scan_rows(16384)


def _tickets(idx, qs, k, mb, mr, after=None):
    ra = [idx.wait(t) for t in [idx.submit(q, k, mb, after) for q in qs]]
    rb = [idx.wait(t) for t in [idx.submit(q, k, mr, after) for q in qs]]
    for (ia, da), (ib, db) in zip(ra, rb):
        assert np.array_equal(ia, ib) and np.array_equal(da.view(np.uint64), db.view(np.uint64))


def _every_route(idx, rng, metric, mb, mr, k=100):
    """nq = 1 on every scan path, a multi-query call below the batch threshold, tickets, a cursor, the batched kernels"""
    qs = _queries(rng, 4, metric)
    routes = {}
    idx.set_batch_min_nq(0)
    for path in _scan_paths(idx):
        routes[path] = _pair(idx, qs[:1], k, mb, mr)
    idx.set_batch_min_nq(16)  # (four queries: below the threshold, one by one)
    assert _pair(idx, qs, k, mb, mr)["batch_launches"] == 0
    _tickets(idx, qs[:2], k, mb, mr)
    first = idx.search(qs, k, None, mb)
    c = int(first[2].min())
    cur = (first[1][:, c // 2].copy(), first[0][:, c // 2].copy())
    c0 = idx.counters()["fallback_searches"]
    _same(idx.search_after(qs, k, cur, None, mb), idx.search_after(qs, k, cur, None, mr), "search_after")
    _tickets(idx, qs[:1], k, mb, mr, after=(float(cur[0][0]), int(cur[1][0])))
    assert idx.counters()["fallback_searches"] == c0
    idx.set_batch_min_nq(2)
    for kern in (2, 1, 0):
        idx.set_batch_kernel(kern)
        assert _pair(idx, qs, k, mb, mr)["batch_launches"] >= 1, kern
    idx.set_batch_kernel(3)
    idx.set_batch_min_nq(0)
    return routes


# the kept counts on the limits, on both sides of each: 16 384 rows for the exact path and the batched listed mode, 16 385
# past both; one kept row in 24 for the list scan and the listed mode (341 * 24 <= 8191 < 342 * 24)
@pytest.mark.parametrize("n,metric,kept", [(393_217, L2, 16_384), (393_217, L2, 16_385), (8_191, COS, 341), (8_191, IP, 342)])
def test_search_parity_on_every_route(hip_lib, n, metric, kept):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(n + kept)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    if metric == COS:
        rows /= np.linalg.norm(rows, axis=1, keepdims=True).astype(np.float32)
    # acl HAS ANY (5000, 5001, 5002) with exactly `kept` rows: the picked rows hold one or two of the three among their tags
    off, vals = _random_column(rng, n, universe=1000, max_len=6, p_empty=0.0, p_null=0.0)
    pick = np.concatenate([rng.choice(n - 1, kept - 1, replace=False), [n - 1]])  # (the last row: its word's tail is ragged)
    others = np.setdiff1d(np.arange(n), pick)
    vals[off[others[rng.random(len(others)) < 0.05]]] = NULL  # one of the other rows in twenty has no value
    vals[off[pick]] = 5000 + (pick % 3)
    two = pick[(off[pick + 1] - off[pick]) >= 2][::2]
    vals[off[two] + 1] = 5000 + ((two + 1) % 3)
    col, S = (off, vals), [5002, 5000, 5001]
    keep = _spec(col, n, S)
    assert int(keep.sum()) == kept and keep[n - 1]
    q_in, q_out = int(pick[0]), int(np.flatnonzero(~keep)[5])  # one quarantined row inside the predicate, one outside it
    rows[q_in, 3] = np.inf
    rows[q_out, 0] = np.inf
    with HipVectorIndex(D, metric) as idx:
        idx.append(0, rows)
        assert idx.counters()["quarantined_rows"] == 2
        with idx.make_tags(col) as tags:
            with idx.make_mask(_bits(keep)) as mb, idx.make_mask_tags(tags, S) as mr:
                _holds(mr, keep, n)
                routes = _every_route(idx, rng, metric, mb, mr)
                print("routes", n, kept, routes["exact"])
            inv = _spec(col, n, S, "any", True)  # the complement of the non-NULL rows: dense
            with idx.make_mask(_bits(inv)) as mb, idx.make_mask_tags(tags, S, negate=True) as mr:
                _holds(mr, inv, n)
                print("routes, dense", n, kept, _every_route(idx, rng, metric, mb, mr)["exact"])


# ---- 7. shard handles and several devices -------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,n", [(12_353, 5_005), (12_837, 4_999)])
def test_shard_handle_reads_the_column_by_global_id(hip_lib, base, n):
    """row_base is no multiple of 8 or 64: the shard's value span starts in the middle of the column's array, and its
    offsets are rebased to it"""
    from tostore_amd import HipVectorIndex

    assert base % 64 in (1, 37) and n % 64 != 0
    rng = np.random.default_rng(base)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    total = base + n + 203
    for length in (total, base + n - 70, base + 17):  # by GLOBAL row id: past the shard, ending inside it, barely reaching it
        off, vals = _random_column(rng, length)
        with HipVectorIndex(D, L2, capacity_rows=n, shard_device=0, row_base=base) as idx:
            idx.append(base, rows)
            with idx.make_tags((off, vals)) as tags:
                for S, need, negate in (([3, 17, 22], "any", False), ([3, 17], "all", False), ([4], "any", True), ([], "all", False)):
                    g = _spec((off, vals), total, S, need, negate)
                    g[:base] = False
                    g[base + n:] = False
                    with idx.make_mask_tags(tags, S, need, negate) as mr, idx.make_mask(_bits(g)) as mb:
                        _holds(mr, g, total)  # global bits: zero outside [base, base + n)
                        _pair(idx, _queries(rng, 3), 40, mb, mr)
                        if g.any():
                            assert (idx.search(_queries(rng, 1), 5, None, mr)[0][0, :1] >= base).all()


def test_in_process_shards(hip_lib):
    """n_devices = 3 in one process (sharing the one GPU): capacity 70 000 puts the shards at 0, 23 360, 46 720; 30 001 rows
    end the second shard inside a word and leave the third empty, 50 003 rows fill two shards and end the third after 3283.
    Every shard's value span starts where its neighbour's ends."""
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(77)
    os.environ["TSH_SHARDS_SHARE_DEVICES"] = "1"
    _ffi.enable_test_hooks()
    try:
        for cap, n in ((70_000, 30_001), (70_001, 50_003)):
            rows = rng.standard_normal((n, D)).astype(np.float32)
            for length in (n - 77, n + 30):
                col = _random_column(rng, length)
                with HipVectorIndex(D, L2, capacity_rows=cap, n_devices=3) as idx:
                    idx.append(0, rows)
                    with idx.make_tags(col) as tags:
                        for S, need, negate in (([3, 17, 22], "any", False), ([9, 10, 11, 12], 2, True)):
                            keep = _spec(col, n, S, need, negate)
                            with idx.make_mask_tags(tags, S, need, negate) as mr, idx.make_mask(_bits(keep)) as mb:
                                _holds(mr, keep, cap)
                                qs = _queries(rng, 3)
                                idx.set_batch_min_nq(0)
                                _pair(idx, qs[:1], 50, mb, mr)
                                _pair(idx, qs, 50, mb, mr)
                                idx.set_batch_min_nq(2)
                                assert _pair(idx, qs, 50, mb, mr)["batch_launches"] >= 1
                                idx.set_batch_min_nq(0)
    finally:
        _ffi.enable_test_hooks(False)
        del os.environ["TSH_SHARDS_SHARE_DEVICES"]


# ---- 8. snapshots, tsh_tags_set, appends, tombstones --------------------------------------------------------------------------
def test_a_handle_is_a_snapshot_and_set_is_seen_by_the_next(hip_lib):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(8)
    n, more = 5_001, 700
    rows = rng.standard_normal((n + more, D)).astype(np.float32)
    col = _random_column(rng, n)
    lists = [list(r) for r in _lists(col)]
    S = [3, 17, 22]
    qs = _queries(rng, 3)
    with HipVectorIndex(D, L2, capacity_rows=n + more) as idx:
        idx.append(0, rows[:n])
        tags = idx.make_tags(col)
        old_keep = _spec(col, n, S)
        with idx.make_mask_tags(tags, S) as old:
            before = idx.search(qs, 30, None, old)
            # an overwrite inside that changes the lists' lengths: rows 100 .. 1099 become [3], [], [1, 2, 3, 4, 5], ...
            new_mid = [[3], [], [1, 2, 3, 4, 5], [NULL, 3]] * 250
            tags.set(100, new_mid)
            lists[100:1100] = new_mid
            _holds(old, old_keep, n)
            _same(idx.search(qs, 30, None, old), before, "after tsh_tags_set")
            now = _csr(lists)
            new_keep = _check(idx, tags, now, n, S)
            assert not np.array_equal(new_keep, old_keep)
            _check(idx, tags, now, n, [1, 2, 3, 4, 5], "all")
            # an extension over a gap: rows n + 100 .. n + 199 all match, rows n .. n + 99 become NULL rows (not yet in the index)
            tags.set(n + 100, [[17, 3]] * 100)
            lists += [[NULL]] * 100 + [[17, 3]] * 100
            now = _csr(lists)
            _check(idx, tags, now, n, S)
            # the index grows: the old handle keeps no new row, though the column would let a hundred of them through
            idx.append(n, rows[n:])
            assert old.kept == int(old_keep.sum())
            grown = np.concatenate([old_keep, np.zeros(more, bool)])
            _holds(old, grown, n + more)
            with idx.make_mask(_bits(old_keep)) as mb:
                _pair(idx, qs, 30, mb, old)
                idx.set_batch_min_nq(2)
                _pair(idx, qs, 30, mb, old)
                idx.set_batch_min_nq(0)
            want = _check(idx, tags, now, n + more, S)
            assert want[n + 100:n + 200].all() and not want[n:n + 100].any() and not want[n + 200:].any()
            _check(idx, tags, now, n + more, S, "any", True)
            # tombstones: the rows stay in kept, and never come back from a search
            with idx.make_mask_tags(tags, S) as cur:
                hit = idx.search(qs[:1], 10, None, cur)[0][0]
                idx.set_deleted(hit[:5])
                assert cur.kept == int(want.sum())
                after = idx.search(qs[:1], 10, None, cur)[0][0]
                assert not set(hit[:5]) & set(after) and set(hit[5:]) <= set(after)
                with idx.make_mask(_bits(want)) as mb:
                    _pair(idx, qs, 30, mb, cur)
            # ... and the old handle outlives the column it was made from
            tags.close()
            _holds(old, grown, n + more)
            with pytest.raises(ValueError):
                idx.make_mask_tags(tags, S)


# ---- 9. lifetime and errors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tags_first", [False, True])
def test_orphans_and_foreign_handles(hip_lib, tags_first):
    from tostore_amd import _ffi

    L = _ffi.lib()
    rows = np.random.default_rng(7).standard_normal((100, D)).astype(np.float32)
    off, vals = _csr([[i % 5, 10 + i % 3] for i in range(100)])
    po, pv = off.ctypes.data_as(_ffi.p_i64), vals.ctypes.data_as(_ffi.p_i64)
    S = np.array([2, 1, 1], np.int64)
    ps = S.ctypes.data_as(_ffi.p_i64)

    def index():
        h = ctypes.c_void_p()
        _ffi.check(L.tsh_index_create(D, L2, 0, 1, ctypes.byref(h)))
        _ffi.check(L.tsh_index_append(h, 0, 100, rows.ctypes.data_as(_ffi.p_f32)))
        return h

    def make(idx, tags, with_, out, combine=0):
        return L.tsh_mask_create_tags(idx, tags, ps, 3, _ffi.TSH_TAGS_ANY, 0, with_, combine, ctypes.byref(out))

    a, b = index(), index()
    tags_a, tags_b, mask_a, mask_b, out = (ctypes.c_void_p() for _ in range(5))
    _ffi.check(L.tsh_tags_create(a, po, 100, pv, ctypes.byref(tags_a)))
    _ffi.check(L.tsh_tags_create(b, po, 100, pv, ctypes.byref(tags_b)))
    _ffi.check(make(a, tags_a, None, mask_a))
    _ffi.check(make(b, tags_b, None, mask_b))
    assert L.tsh_mask_kept(mask_a) == 40 and L.tsh_mask_kept(mask_b) == 40
    for tags, with_ in ((tags_b, None), (tags_a, mask_b)):  # a column of another index; a with of another index
        out.value = 0x20
        assert make(a, tags, with_, out, 1) == _ffi.TSH_E_BAD_ARG
        assert "another index" in _ffi.last_error() and not out.value
    # index a goes first: its column and mask are orphaned, not dangling
    _ffi.check(L.tsh_index_destroy(a))
    out.value = 0x20
    assert make(b, tags_a, None, out) == _ffi.TSH_E_BAD_ARG and not out.value
    out.value = 0x20
    assert make(b, tags_b, mask_a, out) == _ffi.TSH_E_BAD_ARG and not out.value
    assert L.tsh_tags_set(tags_a, 0, 100, po, pv) == _ffi.TSH_E_BAD_ARG and "destroyed" in _ffi.last_error()
    assert L.tsh_tags_destroy(tags_a) == _ffi.TSH_OK and L.tsh_mask_destroy(mask_a) == _ffi.TSH_OK
    # index b: the column before the index, or after it
    if tags_first:
        assert L.tsh_tags_destroy(tags_b) == _ffi.TSH_OK
        assert L.tsh_mask_kept(mask_b) == 40  # (a mask outlives its column)
        assert L.tsh_mask_destroy(mask_b) == _ffi.TSH_OK
        assert L.tsh_index_destroy(b) == _ffi.TSH_OK
    else:
        assert L.tsh_index_destroy(b) == _ffi.TSH_OK
        assert L.tsh_mask_destroy(mask_b) == _ffi.TSH_OK
        assert L.tsh_tags_destroy(tags_b) == _ffi.TSH_OK


# ---- 10. threads --------------------------------------------------------------------------------------------------------------
def test_makers_share_a_handle_under_a_setter(hip_lib):
    """Eight threads make masks from one tag handle while a ninth overwrites the whole column, alternating between two known
    columns of different list lengths: every mask made is NumPy's answer for one of the two columns whole, never a mixture."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(10)
    n = 20_001
    col_a, col_b = _random_column(rng, n, max_len=8), _random_column(rng, n, max_len=5)
    S = [3, 17, 22]
    keeps = [_spec(c, n, S) for c in (col_a, col_b)]
    answers = [(_bits(k), int(k.sum())) for k in keeps]
    assert not np.array_equal(keeps[0], keeps[1])
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, rng.standard_normal((n, D)).astype(np.float32))
        tags = idx.make_tags(col_a)
        start, stop = threading.Barrier(9), threading.Event()
        got, errors, sets = [[] for _ in range(8)], [], [0]

        def maker(which):
            try:
                start.wait(30)
                while not stop.is_set():
                    with idx.make_mask_tags(tags, S) as m:
                        got[which].append((m.bits(), m.kept))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        def setter():
            try:
                start.wait(30)
                deadline = time.monotonic() + 1.5
                while time.monotonic() < deadline:
                    sets[0] += 1
                    tags.set(0, (col_b, col_a)[sets[0] % 2])
            except Exception as e:  # noqa: BLE001
                errors.append(e)
            finally:
                stop.set()

        threads = [threading.Thread(target=maker, args=(i,)) for i in range(8)] + [threading.Thread(target=setter)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        assert not any(t.is_alive() for t in threads), "a thread is still waiting: deadlock"
        assert not errors, errors
        assert sets[0] >= 2 and all(len(g) >= 1 for g in got)
        for g in got:
            for bits, kept in g:
                assert any(np.array_equal(bits, b) and kept == k for b, k in answers), "a mask mixes the two columns"
        last = (col_b, col_a)[sets[0] % 2]
        _check(idx, tags, last, n, S)
        tags.close()


# ---- 11. fuzz -----------------------------------------------------------------------------------------------------------------
def test_fuzz(hip_lib):
    """200 random cases in one process: rows <= 5000, list lengths heavy-tailed (mostly 0 - 8, now and then 100 - 1000),
    random set, need, negate and with."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(2024)
    cases = 0
    for _ in range(20):
        n = int(rng.integers(1, 5001))
        with HipVectorIndex(D, L2) as idx:
            idx.append(0, np.ones((n, D), np.float32))
            for _ in range(2):
                length = int(rng.choice([n, n, max(n - int(rng.integers(0, 200)), 0), n + int(rng.integers(1, 200))]))
                universe = int(rng.choice([20, 300, 5000]))
                lens = rng.integers(0, 9, length)
                longs = rng.random(length) < 0.004
                lens[longs] = rng.integers(100, 1001, int(longs.sum()))
                off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                vals = rng.integers(0, universe, off[-1]).astype(np.int64)
                vals[rng.random(len(vals)) < 0.003] = NULL
                col = (off, vals)
                wk = rng.random(n) < rng.random()
                with idx.make_tags(col) as tags, idx.make_mask(_bits(wk)) as mw:
                    for _ in range(5):
                        size = int(rng.choice([0, 1, 2, 5, 64, 700]))
                        S = rng.integers(0, universe, size).astype(np.int64)
                        if size and rng.random() < 0.3:
                            S[0] = NULL
                        need = ["any", "all", int(rng.integers(1, 6)), int(rng.integers(1, 200))][int(rng.integers(0, 4))]
                        negate = bool(rng.random() < 0.4)
                        mode = int(rng.integers(0, 3))
                        if mode == 0:
                            _check(idx, tags, col, n, S, need, negate)
                        else:
                            _check(idx, tags, col, n, S, need, negate, with_mask=mw, with_keep=wk, combine=("and", "or")[mode - 1])
                        cases += 1
    assert cases == 200
