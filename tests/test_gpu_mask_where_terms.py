"""GPU: a whole WHERE clause made into a mask handle in one launch (tsh_mask_create_where; W2 mask_where_kernel of
tostore_amd/csrc/tsh_where.hip.h, planned by tsh_where_plan.h).  NumPy on the host is the specification and the answer is
exact: the handle's bitmap is NumPy's byte for byte through tsh_mask_read, its kept count NumPy's popcount, no bit at or
past the last row; a one-term call and a chain of tsh_mask_create_range calls give the same bits; and a search with the
handle is bit for bit -- ids, distances, route -- the search with a tsh_mask_create handle made from NumPy's bitmap.
d = 8 throughout: the rows only have to be there."""
import ctypes
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2, IP, COS = 0, 1, 2
D = 8
NULL, I64_MIN, I64_MAX = -(1 << 63), -(1 << 63), (1 << 63) - 1
ROUTE = ("exact_scans", "list_scans", "batch_launches", "fallback_searches")
# equality, an inner range, lo > hi, everything but NULL's own value, everything
TERMS = [(3, 3), (2, 6), (6, 2), (I64_MIN + 1, I64_MAX), (I64_MIN, I64_MAX)]


def _bits(keep, n_bytes=None):
    b = np.packbits(np.asarray(keep, bool), bitorder="little")
    if n_bytes is not None:
        b = np.concatenate([b, np.zeros(n_bytes - len(b), np.uint8)])
    return b


def _column(rng, n):
    """small integers with many duplicates, one entry in ten NULL, the two ends of the value range sprinkled in"""
    v = rng.integers(0, 10, n).astype(np.int64)
    v[rng.random(n) < 0.1] = NULL
    v[rng.random(n) < 0.03] = I64_MIN + 1
    v[rng.random(n) < 0.03] = I64_MAX
    return v


def _v(col, n):
    """the column as n rows see it: rows past it read as NULL"""
    v = np.full(n, NULL, np.int64)
    m = min(n, len(col))
    v[:m] = col[:m]
    return v


# a term of the specification: ("r", column number, lo, hi, negate) or ("s", column number, values, negate)
def R(ci, lo, hi, negate=False):
    return ("r", ci, lo, hi, negate)


def S(ci, values, negate=False):
    return ("s", ci, list(values), negate)


def _keep(cols, n, clauses):
    """the specification: a term keeps row i < n iff it has a value and hit != negate; a clause is the OR of its terms,
    the result the AND of the clauses"""
    res = np.ones(n, bool)
    for clause in clauses:
        c = np.zeros(n, bool)
        for t in clause:
            v = _v(cols[t[1]], n)
            if t[0] == "r":
                hit = (v >= np.int64(t[2])) & (v <= np.int64(t[3]))
            else:
                hit = np.isin(v, np.array([x for x in t[2] if x != NULL], np.int64))
            c |= (v != NULL) & (hit != bool(t[-1]))
        res &= c
    return res


def _terms(attrs, clauses):
    from tostore_amd import WhereIn, WhereRange

    return [[WhereRange(attrs[t[1]], t[2], t[3], t[4]) if t[0] == "r" else WhereIn(attrs[t[1]], np.array(t[2], np.int64), t[3])
             for t in clause] for clause in clauses]


def _holds(m, keep, n_rows_end, slack=9):
    """the handle's bitmap is `keep` (bit i = GLOBAL row id i) byte for byte, zero past it; kept is its popcount"""
    nb = (n_rows_end + 7) // 8 + slack
    got = m.bits(nb)
    assert got.dtype == np.uint8 and got.shape == (nb,)
    assert np.array_equal(got, _bits(keep, nb)), np.flatnonzero(got != _bits(keep, nb))[:8]
    assert m.kept == int(np.count_nonzero(keep))
    short = m.bits()  # by default one bit per row id the index holds
    assert short.shape == ((m.index.size + 7) // 8,) and np.array_equal(short, got[:len(short)])


def _check(idx, attrs, cols, n, clauses, end=None, with_mask=None, with_keep=None, combine="and", slack=9):
    want = _keep(cols, n, clauses)
    if with_keep is not None:
        want = (want | with_keep) if combine == "or" else (want & with_keep)
    with idx.make_mask_clauses(_terms(attrs, clauses), with_mask=with_mask, combine=combine) as m:
        _holds(m, want, n if end is None else end, slack)
    return want


def _queries(rng, nq, metric=L2):
    q = rng.standard_normal((nq, D)).astype(np.float32)
    return q / np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32) if metric == COS else q


def _same(a, b, what=""):
    assert np.array_equal(a[2], b[2]), ("counts", what)
    for i, c in enumerate(a[2]):
        assert np.array_equal(a[0][i, :c], b[0][i, :c]), ("ids", what, i)
        assert np.array_equal(a[1][i, :c].view(np.uint64), b[1][i, :c].view(np.uint64)), ("distance bits", what, i)


def _pair(idx, qs, k, mb, mr):
    """the bitmap-made and the clause-made handle of one row set: the same answer by the same route -> that route"""
    c0 = idx.counters()
    a = idx.search(qs, k, None, mb)
    c1 = idx.counters()
    b = idx.search(qs, k, None, mr)
    c2 = idx.counters()
    _same(a, b)
    ra = {c: c1[c] - c0[c] for c in ROUTE}
    rb = {c: c2[c] - c1[c] for c in ROUTE}
    assert ra == rb, ("the bitmap handle and the clause handle took different routes", ra, rb)
    if ra["batch_launches"]:
        assert c1["batch_kernel_last"] == c2["batch_kernel_last"]
    assert ra["fallback_searches"] == 0
    return ra


def _tickets(idx, qs, k, mb, mr):
    ta = [idx.submit(q, k, mb) for q in qs]
    ra = [idx.wait(t) for t in ta]
    tb = [idx.submit(q, k, mr) for q in qs]
    rb = [idx.wait(t) for t in tb]
    for (ia, da), (ib, db) in zip(ra, rb):
        assert np.array_equal(ia, ib) and np.array_equal(da.view(np.uint64), db.view(np.uint64))


def _scan_paths(idx):
    yield "exact"
    idx.set_exact_select(False)
    yield "exact_select"
    idx.set_exact_select(True)
    idx.set_exact_scan_rows(0)
    yield "prefilter"
    idx.set_exact_scan_rows(16384)


def _every_route(idx, rng, metric, mb, mr, ks=(1, 100)):
    """nq = 1 on every scan path, a multi-query call below the batch threshold, tickets, the batched kernels 0 / 1 / 2"""
    qs = _queries(rng, 4, metric)
    routes = {}
    idx.set_batch_min_nq(0)
    for k in ks:
        for path in _scan_paths(idx):
            routes[(k, path)] = _pair(idx, qs[:1], k, mb, mr)
        idx.set_batch_min_nq(16)  # (four queries: below the threshold, one by one)
        assert _pair(idx, qs, k, mb, mr)["batch_launches"] == 0
        _tickets(idx, qs[:2], k, mb, mr)
        idx.set_batch_min_nq(2)
        for kern in (2, 1, 0):
            idx.set_batch_kernel(kern)
            assert _pair(idx, qs, k, mb, mr)["batch_launches"] >= 1, kern
        idx.set_batch_kernel(3)
        idx.set_batch_min_nq(0)
    return routes


def _other_entries(idx, rng, metric, n, keep, mb, mr):
    """cursor, count and grouped searches take the clause handle as they take the bitmap handle"""
    qs = _queries(rng, 3, metric)
    k = int(min(20, keep.sum()))
    first = idx.search(qs, k, None, mb)
    cur = (first[1][:, k - 1].copy(), first[0][:, k - 1].copy())
    _same(idx.search_after(qs, k, cur, None, mb), idx.search_after(qs, k, cur, None, mr), "search_after")
    thr = float(first[1][0, k // 2])
    ca, cb = idx.search_count(qs, thr, mb), idx.search_count(qs, thr, mr)
    assert np.array_equal(ca, cb) and (ca <= keep.sum()).all()
    assert metric != L2 or ca[0] >= k // 2 + 1  # (the first query's own eleventh distance: at least eleven rows count)
    assert np.array_equal(idx.search_count(qs, None, mr), np.full(3, keep.sum()))
    with idx.make_groups(np.arange(n, dtype=np.int32) // 7, n // 7 + 1) as g:
        ga, gb = idx.search_grouped(qs, k, g, None, mb), idx.search_grouped(qs, k, g, None, mr)
        _same((ga[0], ga[1], ga[3]), (gb[0], gb[1], gb[3]), "search_grouped")
        assert np.array_equal(ga[2], gb[2])


# ---- 1. rows and clauses --------------------------------------------------------------------------------------------------
# 524 353 = 2048 workgroups x 4 words x 64 rows + 65: the grid is at its cap there and the grid-stride loop takes a second
# pass, whose last word is ragged
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4097, 20_001, 524_353])
def test_clauses_are_numpys(hip_lib, n):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(n)
    cap = n + 479
    rows = rng.standard_normal((n, D)).astype(np.float32)
    # eight columns; the first shorter than the index, the second as long, the third longer
    lens = [n - (n + 2) // 3, n, n + 70] + [n] * 5
    cols = [_column(rng, n + 70)[:ln] for ln in lens]
    cols[4] = rng.integers(1_700_000_000, 1_700_001_000, max(n - 500, n // 2)).astype(np.int64)  # a timestamp, the tail without
    cols[5] = _column(rng, n + 9) % 2  # a flag ...
    cols[5][rng.random(n + 9) < 0.1] = NULL  # ... that one row in ten lacks
    a, b = 1_700_000_200, 1_700_000_700
    with HipVectorIndex(D, L2, capacity_rows=cap) as idx:
        idx.append(0, rows)
        attrs = [idx.make_attr(c) for c in cols]
        # one range term: tsh_mask_create_range's handle bit for bit, over the short, the exact and the long column
        for ci in (0, 1, 2):
            for lo, hi in TERMS:
                for negate in (False, True):
                    with idx.make_mask_where(attrs[ci], lo, hi, negate) as m1, \
                            idx.make_mask_clauses(_terms(attrs, [[R(ci, lo, hi, negate)]])) as m2:
                        nb = (cap + 7) // 8 + 70
                        assert np.array_equal(m1.bits(nb), m2.bits(nb)) and m1.kept == m2.kept
                        _holds(m2, _keep(cols, n, [[R(ci, lo, hi, negate)]]), n)
        # tenant IN (3, 7) AND ts BETWEEN a AND b AND NOT flag = 1: three columns, the chain's final handle
        where = [[R(0, 3, 3), R(0, 7, 7)], [R(4, a, b)], [R(5, 1, 1, True)]]
        with idx.make_mask_where(attrs[0], 3, 3) as c1, idx.make_mask_where(attrs[0], 7, 7, with_mask=c1, combine="or") as c2, \
                idx.make_mask_where(attrs[4], a, b, with_mask=c2) as c3, \
                idx.make_mask_where(attrs[5], 1, 1, negate=True, with_mask=c3, combine="and") as c4, \
                idx.make_mask_clauses(_terms(attrs, where)) as m:
            nb = (cap + 7) // 8 + 70
            assert np.array_equal(c4.bits(nb), m.bits(nb)) and c4.kept == m.kept
            _holds(m, _keep(cols, n, where), n)
        # ... and the same with the IN-list as a set
        _check(idx, attrs, cols, n, [[S(0, [7, 3])], [R(4, a, b)], [R(5, 1, 1, True)]])
        # 32 terms in one OR clause over one column: windows, points, the ends, a few negated
        ors = [R(1, int(lo), int(lo) + int(w), bool(ng)) for lo, w, ng in zip(rng.integers(-2, 11, 29), rng.integers(-1, 2, 29),
                                                                                rng.random(29) < 0.1)]
        ors += [R(1, I64_MAX, I64_MAX), R(1, I64_MIN, I64_MIN + 1), R(1, 4, 4)]
        assert len(ors) == 32
        _check(idx, attrs, cols, n, [ors])
        _check(idx, attrs, cols, n, [[R(1, v, v) for v in (0, 2, 4, 6, 8)] * 6 + [R(1, 9, 9), R(1, I64_MAX, I64_MAX)]])
        # 32 one-term AND clauses over eight columns: wide windows and negated points, so that rows survive
        ands = []
        for t in range(32):
            ci = t % 8
            if ci in (4, 5):
                ands.append([R(ci, 0, I64_MAX)] if t % 3 else [R(ci, 1, 1, True)])
            else:
                ands.append([R(ci, int(rng.integers(-3, 2)), I64_MAX)] if t % 2 else [R(ci, int(rng.integers(0, 10)), int(rng.integers(0, 10)), True)])
        want = _check(idx, attrs, cols, n, ands)
        assert n < 4095 or want.any()
        # negated terms, NULL rows present in every column: a NULL row is kept by no term
        _check(idx, attrs, cols, n, [[R(0, 3, 3, True)]])
        _check(idx, attrs, cols, n, [[R(0, 3, 3, True), S(1, [2, 5], True)], [S(2, [1, 2, 3, I64_MAX], True), R(5, 0, 0)]])
        # the empty range and the empty set, plain and negated; alone, or-ed and and-ed with a real term
        for empty in (R(2, 6, 2), S(2, []), S(2, [NULL, NULL])):
            full = (empty[0],) + empty[1:-1] + (True,)
            assert not _check(idx, attrs, cols, n, [[empty]]).any()
            assert np.array_equal(_check(idx, attrs, cols, n, [[full]]), _v(cols[2], n) != NULL)
            _check(idx, attrs, cols, n, [[empty, R(1, 2, 6)], [full]])
            assert not _check(idx, attrs, cols, n, [[R(1, 2, 6)], [empty]]).any()
        # an IN term and a range term over the same column in one clause, and in two
        _check(idx, attrs, cols, n, [[S(1, [1, 8, I64_MIN + 1]), R(1, 3, 5)]])
        _check(idx, attrs, cols, n, [[S(1, [1, 4, 8, I64_MIN + 1])], [R(1, 3, 9, True)]])
        # `with` under AND and OR: a handle made by a clause, and one made from a capacity-sized bitmap with every bit
        # past the last row set -- none comes through
        w = rng.random(n) < 0.3
        full = np.ones(cap, bool)
        full[:n] = w
        with idx.make_mask(_bits(full)) as mw, idx.make_mask_clauses(_terms(attrs, [[S(3, [1, 2, 3])]])) as mc:
            assert mw.kept == int(w.sum())
            wc = _keep(cols, n, [[S(3, [1, 2, 3])]])
            for combine in ("or", "and"):
                _check(idx, attrs, cols, n, where, end=cap, with_mask=mw, with_keep=w, combine=combine, slack=70)
                _check(idx, attrs, cols, n, [ors], end=cap, with_mask=mc, with_keep=wc, combine=combine, slack=70)
            # NULL under OR: a row without a value is kept by `with` alone, negated term or not
            want = _check(idx, attrs, cols, n, [[R(0, 3, 3, True)]], end=cap, with_mask=mw, with_keep=w, combine="or")
            assert n < 4095 or (want & (_v(cols[0], n) == NULL)).any()
        for at in attrs:
            at.close()


# ---- 2. sets ----------------------------------------------------------------------------------------------------------------
def _set_and_column(rng, size, n):
    """`size` distinct members with both ends of the value range among them (from two members on), and a column that
    holds members, the values just below and just above members, values between them, the ends and NULLs"""
    members = rng.choice(1 << 20, size, replace=False).astype(np.int64) * 3 - (1 << 20)  # multiples of 3: neighbours are no members
    if size >= 2:
        members[0], members[1] = I64_MIN + 1, I64_MAX
    pool = [np.array([I64_MIN + 1, I64_MIN + 2, I64_MAX, I64_MAX - 1, 0, -1, 1], np.int64)]
    if size:
        inner = members[2:] if size > 2 else members[:0]
        pool += [members, inner - 1, inner + 1, inner + 3]
    pool.append(rng.integers(-(1 << 21), 1 << 21, 64).astype(np.int64))
    pool = np.concatenate(pool)
    col = pool[rng.integers(0, len(pool), n)]
    col[rng.random(n) < 0.1] = NULL
    col[:4] = I64_MIN + 1, I64_MAX, I64_MIN + 2, I64_MAX - 1  # (the ends and their neighbours, whatever the draw)
    if size > 2:
        col[4:7] = members[2], members[2] - 1, members[2] + 1
    # as a caller hands it over: any order, some values twice, a NULL among them
    given = np.concatenate([members, members[: size // 3], [NULL]]) if size else np.array([NULL], np.int64)
    return members, rng.permutation(given), col


@pytest.mark.parametrize("size", [0, 1, 2, 63, 64, 65, 4095, 4096])
def test_sets_are_numpys(hip_lib, size):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(100 + size)
    n = 4_097
    rows = rng.standard_normal((n, D)).astype(np.float32)
    members, given, col = _set_and_column(rng, size, n)
    cols = [col, _column(rng, n)]
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, rows)
        attrs = [idx.make_attr(c) for c in cols]
        for negate in (False, True):
            want = _check(idx, attrs, cols, n, [[S(0, given, negate)]])
            v = _v(col, n)
            assert np.array_equal(want, (v != NULL) & (np.isin(v, members) != negate))
            if size >= 2:  # the ends of the value range are members, and rows hold them
                assert (want[v == I64_MAX] != negate).all() and (v == I64_MAX).any() and (v == I64_MIN + 1).any()
        if size:
            assert _keep(cols, n, [[S(0, given)]]).any()
        # the set beside a range term over another column, and as one clause of two
        _check(idx, attrs, cols, n, [[S(0, given), R(1, 3, 3)], [R(1, 0, 9)]])
        if size == 0:
            # without members the NULL alone, or nothing at all (a NULL pointer with n_set == 0)
            _check(idx, attrs, cols, n, [[S(0, [], True)]])
        for at in attrs:
            at.close()


@pytest.mark.parametrize("sizes", [(4000, 96), (2000, 2000, 96), (1, 4095), (64, 0, 65)])
def test_sets_share_the_budget(hip_lib, sizes):
    """two and three IN terms in one call: every term but the first finds its values at a nonzero offset of the staged array"""
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(sum(sizes))
    n = 4_097
    rows = rng.standard_normal((n, D)).astype(np.float32)
    made = [_set_and_column(rng, s, n) for s in sizes]
    cols = [m[2] for m in made]
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, rows)
        attrs = [idx.make_attr(c) for c in cols]
        terms = [S(i, m[1], bool(i % 2)) for i, m in enumerate(made)]
        _check(idx, attrs, cols, n, [terms])                 # one OR clause
        _check(idx, attrs, cols, n, [[t] for t in terms])    # one clause each
        # every set over the FIRST column too: the offsets differ, the column is loaded once
        _check(idx, attrs, cols, n, [[S(0, m[1]) for m in made], [R(0, I64_MIN + 1, I64_MAX)]])
        if sum(sizes) == _ffi.TSH_WHERE_MAX_SET_VALUES:  # one value more anywhere is refused, and nothing is made
            extra = _terms(attrs, [[t] for t in terms] + [[S(0, [12345678])]])
            with pytest.raises(_ffi.TshError) as e:
                idx.make_mask_clauses(extra)
            assert e.value.code == _ffi.TSH_E_BAD_ARG and "TSH_WHERE_MAX_SET_VALUES" in str(e.value)
        for at in attrs:
            at.close()


# ---- 3. search parity and routes -------------------------------------------------------------------------------------------
# the kept counts on the limits, on both sides of each: 16 384 rows for the exact path and the batched listed mode, 16 385
# past both; one kept row in 24 for the list scan and the listed mode (341 * 24 <= 8191 < 342 * 24)
@pytest.mark.parametrize("n,metric,kept", [(393_217, L2, 16_384), (393_217, L2, 16_385), (8_191, COS, 341), (8_191, IP, 342)])
def test_search_parity_on_every_route(hip_lib, n, metric, kept):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(n + kept)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    if metric == COS:
        rows /= np.linalg.norm(rows, axis=1, keepdims=True).astype(np.float32)
    # tenant IN (7, 11) AND ts >= 5 AND NOT flag = 1, with exactly `kept` rows: the picked rows pass all three
    tenant = _column(rng, n)
    tenant[tenant == 7] = 8
    ts = rng.integers(0, 10, n).astype(np.int64)
    flag = rng.integers(0, 2, n).astype(np.int64)
    pick = np.concatenate([rng.choice(n - 1, kept - 1, replace=False), [n - 1]])  # (the last row: its word's tail is ragged)
    tenant[pick[::2]], tenant[pick[1::2]] = 7, 11
    other = np.ones(n, bool)
    other[pick] = False
    ts[other & (rng.random(n) < 0.5)] = 2      # half of the others fail on ts ...
    tenant[other & (ts >= 5) & (flag == 0)] = 4  # ... and whoever still passes ts and flag is of another tenant
    ts[pick], flag[pick] = 6, 0
    cols = [tenant, ts, flag]
    where = [[S(0, [11, 7])], [R(1, 5, I64_MAX)], [R(2, 1, 1, True)]]
    keep = _keep(cols, n, where)
    assert int(keep.sum()) == kept and keep[n - 1]
    # one quarantined row (an inf element) inside the predicate, one outside it
    q_in, q_out = int(pick[0]), int(np.flatnonzero(~keep)[5])
    rows[q_in, 3] = np.inf
    rows[q_out, 0] = np.inf
    with HipVectorIndex(D, metric) as idx:
        idx.append(0, rows)
        assert idx.counters()["quarantined_rows"] == 2
        attrs = [idx.make_attr(c) for c in cols]
        with idx.make_mask(_bits(keep)) as mb, idx.make_mask_clauses(_terms(attrs, where)) as mr:
            _holds(mr, keep, n)
            routes = _every_route(idx, rng, metric, mb, mr)
            print("routes", n, kept, routes[(100, "exact")])
            _other_entries(idx, rng, metric, n, keep, mb, mr)
        # the complement of the first clause, dense
        dense = [[S(0, [11, 7], True)]]
        inv = _keep(cols, n, dense)
        with idx.make_mask(_bits(inv)) as mb, idx.make_mask_clauses(_terms(attrs, dense)) as mr:
            _holds(mr, inv, n)
            _every_route(idx, rng, metric, mb, mr, ks=(100,))
        for at in attrs:
            at.close()


# ---- 4. shard handles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,n", [(12_353, 5_005), (12_837, 4_999)])
def test_shard_handle_reads_three_columns_by_global_id(hip_lib, base, n):
    from tostore_amd import HipVectorIndex

    assert base % 64 in (1, 37) and n % 64 != 0
    rng = np.random.default_rng(base)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    total = base + n + 203
    # by GLOBAL row id, the neighbours' values on both sides; one column ends inside the shard, one before its end
    cols = [_column(rng, total), _column(rng, base + n - 70), _column(rng, total + 5)]
    with HipVectorIndex(D, L2, capacity_rows=n, shard_device=0, row_base=base) as idx:
        idx.append(base, rows)
        attrs = [idx.make_attr(c) for c in cols]
        for where in ([[R(0, 2, 4)], [S(1, [1, 3, 5, 7, I64_MAX]), R(2, 0, 0)], [R(2, 9, 9, True)]],
                      [[S(0, [3])]], [[R(0, 3, 3, True), S(1, [], True)]]):
            g = np.zeros(total, bool)
            g[base:base + n] = _keep([c[base:] for c in cols], n, where)
            with idx.make_mask_clauses(_terms(attrs, where)) as mr, idx.make_mask(_bits(g)) as mb:
                _holds(mr, g, total)  # global bits: zero outside [base, base + n)
                got = _pair(idx, _queries(rng, 3), 40, mb, mr)
                assert got["fallback_searches"] == 0
                assert (idx.search(_queries(rng, 1), 5, None, mr)[0][0, :1] >= base).all()
        for at in attrs:
            at.close()


# ---- 5. several devices -------------------------------------------------------------------------------------------------
def test_in_process_shards(hip_lib):
    """n_devices = 3 in one process (sharing the one GPU): capacity 70 000 puts the shards at 0, 23 360, 46 720.  What the
    rows leave ragged is every shard's END: 30 001 rows end the second shard inside a word and a byte and leave the third
    empty; 50 003 rows fill two shards and end the third after 3283.  One column is 77 rows short of the index."""
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(55)
    os.environ["TSH_SHARDS_SHARE_DEVICES"] = "1"
    _ffi.enable_test_hooks()
    try:
        for cap, n in ((70_000, 30_001), (70_001, 50_003)):
            rows = rng.standard_normal((n, D)).astype(np.float32)
            cols = [_column(rng, n - 77), _column(rng, n), _column(rng, n + 30)]
            with HipVectorIndex(D, L2, capacity_rows=cap, n_devices=3) as idx:
                idx.append(0, rows)
                attrs = [idx.make_attr(c) for c in cols]
                for where in ([[S(0, [3, 4, I64_MAX]), R(1, 3, 3)], [R(2, 2, 6, True)]], [[S(1, range(0, 10, 2), True)]]):
                    keep = _keep(cols, n, where)
                    with idx.make_mask_clauses(_terms(attrs, where)) as mr, idx.make_mask(_bits(keep)) as mb:
                        _holds(mr, keep, cap)
                        qs = _queries(rng, 3)
                        idx.set_batch_min_nq(0)
                        _pair(idx, qs[:1], 50, mb, mr)
                        _pair(idx, qs, 50, mb, mr)
                        idx.set_batch_min_nq(2)
                        assert _pair(idx, qs, 50, mb, mr)["batch_launches"] >= 1
                        idx.set_batch_min_nq(0)
                for at in attrs:
                    at.close()
    finally:
        _ffi.enable_test_hooks(False)
        del os.environ["TSH_SHARDS_SHARE_DEVICES"]


# ---- 6. snapshot --------------------------------------------------------------------------------------------------------
def test_a_handle_is_a_snapshot(hip_lib):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(6)
    n, more = 5_001, 700
    rows = rng.standard_normal((n + more, D)).astype(np.float32)
    cols = [_column(rng, n), _column(rng, n)]
    where = [[S(0, [3, 9])], [R(1, 1, 8)]]
    qs = _queries(rng, 3)
    with HipVectorIndex(D, L2, capacity_rows=n + more) as idx:
        idx.append(0, rows[:n])
        attrs = [idx.make_attr(c) for c in cols]
        old_keep = _keep(cols, n, where)
        with idx.make_mask_clauses(_terms(attrs, where)) as old:
            before = idx.search(qs, 30, None, old)
            # one column changes under the handle: every 3 becomes a 5, every 4 a 3 -- and the rows to come are all 3
            new0 = cols[0].copy()
            new0[cols[0] == 3] = 5
            new0[cols[0] == 4] = 3
            attrs[0].set(0, new0)
            attrs[0].set(n, np.full(more, 3, np.int64))
            attrs[1].set(n, np.full(more, 2, np.int64))
            _holds(old, old_keep, n)
            _same(idx.search(qs, 30, None, old), before, "after tsh_attr_set")
            _check(idx, attrs, [new0, cols[1]], n, where)  # (the columns are longer than the index now: 700 values wait)
            # the index grows: no new row is kept, though the columns would let every one of them through
            idx.append(n, rows[n:])
            assert old.kept == int(old_keep.sum())
            grown = np.concatenate([old_keep, np.zeros(more, bool)])
            _holds(old, grown, n + more)
            with idx.make_mask(_bits(old_keep)) as mb:
                _pair(idx, qs, 30, mb, old)
                idx.set_batch_min_nq(2)
                _pair(idx, qs, 30, mb, old)
                idx.set_batch_min_nq(0)
            now = [np.concatenate([new0, np.full(more, 3, np.int64)]), np.concatenate([cols[1], np.full(more, 2, np.int64)])]
            assert _check(idx, attrs, now, n + more, where)[n:].all()
            # ... and the handle outlives the columns it was made from
            for at in attrs:
                at.close()
            _holds(old, grown, n + more)
            _same(idx.search(qs, 30, None, old), idx.search(qs, 30, None, _bits(grown)), "after tsh_attr_destroy")
            with pytest.raises(ValueError):
                idx.make_mask_clauses(_terms(attrs, where))


# ---- 7. lifetime and errors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attr_first", [False, True])
def test_orphans_and_foreign_handles(hip_lib, attr_first):
    from tostore_amd import _ffi

    L = _ffi.lib()
    rows = np.random.default_rng(7).standard_normal((100, D)).astype(np.float32)
    col = np.arange(100, dtype=np.int64) % 5
    p64 = col.ctypes.data_as(_ffi.p_i64)
    members = np.array([2, 1, 1], np.int64)

    def index():
        h = ctypes.c_void_p()
        _ffi.check(L.tsh_index_create(D, L2, 0, 1, ctypes.byref(h)))
        _ffi.check(L.tsh_index_append(h, 0, 100, rows.ctypes.data_as(_ffi.p_f32)))
        return h

    def where(idx, attr_handles, with_, out, combine=0):
        """attr IN (1, 2) of the first handle, and-ed with 0 <= attr <= 4 of each of the others"""
        arr = (_ffi.TshWhereTerm * len(attr_handles))()
        for i, h in enumerate(attr_handles):
            arr[i].attr, arr[i].clause = h, i
            if i == 0:
                arr[i].kind, arr[i].set, arr[i].n_set = _ffi.TSH_TERM_IN, members.ctypes.data_as(_ffi.p_i64), 3
            else:
                arr[i].kind, arr[i].lo, arr[i].hi = _ffi.TSH_TERM_RANGE, 0, 4
        return L.tsh_mask_create_where(idx, ctypes.cast(arr, _ffi.p_void), len(attr_handles), with_, combine, ctypes.byref(out))

    a, b = index(), index()
    attr_a, attr_a2, attr_b, mask_a, mask_b, out = (ctypes.c_void_p() for _ in range(6))
    _ffi.check(L.tsh_attr_create(a, p64, 100, ctypes.byref(attr_a)))
    _ffi.check(L.tsh_attr_create(a, p64, 100, ctypes.byref(attr_a2)))
    _ffi.check(L.tsh_attr_create(b, p64, 100, ctypes.byref(attr_b)))
    _ffi.check(where(a, [attr_a, attr_a2], None, mask_a))
    _ffi.check(where(b, [attr_b], None, mask_b))
    assert L.tsh_mask_kept(mask_a) == 40 and L.tsh_mask_kept(mask_b) == 40
    # an attr of another index, first or second of the terms; a with of another index
    for attrs, with_ in (([attr_b], None), ([attr_a, attr_b], None), ([attr_a], mask_b)):
        out.value = 0x20
        assert where(a, attrs, with_, out, 1) == _ffi.TSH_E_BAD_ARG
        assert "another index" in _ffi.last_error() and not out.value
    # index a goes first: its attrs and mask are orphaned, not dangling
    buf = np.full(16, 0xAB, np.uint8)
    _ffi.check(L.tsh_mask_read(mask_a, buf.ctypes.data_as(_ffi.p_u8), 16))
    assert np.array_equal(buf, _bits((col == 1) | (col == 2), 16))
    _ffi.check(L.tsh_index_destroy(a))
    out.value = 0x20
    assert where(b, [attr_a], None, out) == _ffi.TSH_E_BAD_ARG and not out.value
    out.value = 0x20
    assert where(b, [attr_b, attr_a2], None, out) == _ffi.TSH_E_BAD_ARG and not out.value
    out.value = 0x20
    assert where(b, [attr_b], mask_a, out) == _ffi.TSH_E_BAD_ARG and not out.value
    buf[:] = 0xAB
    assert L.tsh_mask_read(mask_a, buf.ctypes.data_as(_ffi.p_u8), 16) == _ffi.TSH_E_BAD_ARG and (buf == 0xAB).all()
    assert L.tsh_attr_destroy(attr_a) == _ffi.TSH_OK and L.tsh_attr_destroy(attr_a2) == _ffi.TSH_OK
    assert L.tsh_mask_destroy(mask_a) == _ffi.TSH_OK
    # index b: the attr before the index, or after it
    if attr_first:
        assert L.tsh_attr_destroy(attr_b) == _ffi.TSH_OK
        assert L.tsh_mask_kept(mask_b) == 40  # (a mask outlives its column)
        assert L.tsh_mask_destroy(mask_b) == _ffi.TSH_OK
        assert L.tsh_index_destroy(b) == _ffi.TSH_OK
    else:
        assert L.tsh_index_destroy(b) == _ffi.TSH_OK
        assert L.tsh_mask_destroy(mask_b) == _ffi.TSH_OK
        assert L.tsh_attr_destroy(attr_b) == _ffi.TSH_OK


# ---- 8. threads -----------------------------------------------------------------------------------------------------------
def test_opposite_orders_do_not_deadlock_against_a_set(hip_lib):
    """Two threads make clauses that name the same two attribute handles in opposite orders while a third overwrites one
    of the columns: nobody waits for ever, and every handle made holds the column as it was before the set or as it was
    after it -- never a mixture."""
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(8)
    n, rounds = 20_001, 25
    rows = rng.standard_normal((n, D)).astype(np.float32)
    col_a, col_b = _column(rng, n), _column(rng, n)
    new_a = (col_a + 1) % 10
    new_a[col_a == NULL] = 3  # (the rows without a value get one)
    orders = ([[R(0, 3, 3)], [S(1, [2, 4, 6])]], [[S(1, [2, 4, 6])], [R(0, 3, 3)]])
    old, new = _keep([col_a, col_b], n, orders[0]), _keep([new_a, col_b], n, orders[0])
    assert old.any() and new.any() and not np.array_equal(old, new)
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, rows)
        attrs = [idx.make_attr(col_a), idx.make_attr(col_b)]
        start = threading.Barrier(3)
        got, errors = [[], []], []

        def maker(which):
            try:
                start.wait(30)
                for _ in range(rounds):
                    with idx.make_mask_clauses(_terms(attrs, orders[which])) as m:
                        got[which].append((m.bits(), m.kept))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        def setter():
            try:
                start.wait(30)
                attrs[0].set(0, new_a)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=maker, args=(0,)), threading.Thread(target=maker, args=(1,)), threading.Thread(target=setter)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        assert not any(t.is_alive() for t in threads), "a thread is still waiting: deadlock"
        assert not errors, errors
        olds, news = (_bits(old), int(old.sum())), (_bits(new), int(new.sum()))
        for which in (0, 1):
            assert len(got[which]) == rounds
            seen_new = False
            for bits, kept in got[which]:
                is_old = np.array_equal(bits, olds[0]) and kept == olds[1]
                is_new = np.array_equal(bits, news[0]) and kept == news[1]
                assert is_old or is_new, "a handle mixes the column before and after tsh_attr_set"
                assert not (seen_new and is_old), "the old column came back after the new one was seen"
                seen_new = seen_new or is_new
        _check(idx, attrs, [new_a, col_b], n, orders[0])
        for at in attrs:
            at.close()
