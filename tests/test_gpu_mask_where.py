"""GPU: WHERE range terms made into mask handles on the device (tsh_attr_create, tsh_mask_create_range, tsh_mask_read;
tostore_amd/csrc/tsh_where.hip.h).  NumPy on the host is the specification and the answer is exact: the handle's bitmap is
NumPy's byte for byte, its kept count NumPy's popcount, no bit at or past the last row; and a search with the handle is
bit for bit -- ids, distances, route -- the search with a tsh_mask_create handle made from NumPy's bitmap (which
tests/test_gpu_mask_edges.py and its neighbours hold to the oracle).  d = 32 throughout."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2, IP, COS = 0, 1, 2
D = 32
NULL, I64_MIN, I64_MAX = -(1 << 63), -(1 << 63), (1 << 63) - 1
ROUTE = ("exact_scans", "list_scans", "batch_launches", "fallback_searches")
# equality, an inner range, lo > hi, everything but NULL's own value, everything: each plain and negated
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


def _term(col, n, lo, hi, negate=False):
    """the specification: row i < n is kept iff it has a value and (lo <= v <= hi) != negate; rows past the column: NULL"""
    v = np.full(n, NULL, np.int64)
    m = min(n, len(col))
    v[:m] = col[:m]
    return (v != NULL) & (((v >= np.int64(lo)) & (v <= np.int64(hi))) != bool(negate))


def _holds(m, keep, n_rows_end, slack=9):
    """the handle's bitmap is `keep` (bit i = GLOBAL row id i) byte for byte, zero past it; kept is its popcount"""
    nb = (n_rows_end + 7) // 8 + slack
    got = m.bits(nb)
    assert got.dtype == np.uint8 and got.shape == (nb,)
    assert np.array_equal(got, _bits(keep, nb)), np.flatnonzero(got != _bits(keep, nb))[:8]
    assert m.kept == int(np.count_nonzero(keep))
    short = m.bits()  # by default one bit per row id the index holds
    assert short.shape == ((m.index.size + 7) // 8,) and np.array_equal(short, got[:len(short)])


def _queries(rng, nq, metric=L2):
    q = rng.standard_normal((nq, D)).astype(np.float32)
    return q / np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32) if metric == COS else q


def _same(a, b, what=""):
    assert np.array_equal(a[2], b[2]), ("counts", what)
    for i, c in enumerate(a[2]):
        assert np.array_equal(a[0][i, :c], b[0][i, :c]), ("ids", what, i)
        assert np.array_equal(a[1][i, :c].view(np.uint64), b[1][i, :c].view(np.uint64)), ("distance bits", what, i)


def _pair(idx, qs, k, mb, mr):
    """the bitmap-made and the range-made handle of one row set: the same answer by the same route -> that route"""
    c0 = idx.counters()
    a = idx.search(qs, k, None, mb)
    c1 = idx.counters()
    b = idx.search(qs, k, None, mr)
    c2 = idx.counters()
    _same(a, b)
    ra = {c: c1[c] - c0[c] for c in ROUTE}
    rb = {c: c2[c] - c1[c] for c in ROUTE}
    assert ra == rb, ("the bitmap handle and the range handle took different routes", ra, rb)
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


# ---- 1. bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4097, 16_385, 20_001])
def test_bits_are_numpys(hip_lib, n):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(n)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, rows)
        for col_len in (n - (n + 2) // 3, n, n + 70):  # shorter than, equal to and longer than the index
            col = _column(rng, n + 70)[:col_len]
            with idx.make_attr(col) as attr:
                for lo, hi in TERMS:
                    for negate in (False, True):
                        with idx.make_mask_where(attr, lo, hi, negate) as m:
                            _holds(m, _term(col, n, lo, hi, negate), n)
        # NULL is kept by no term, whatever its bounds: a column of NULLs only
        with idx.make_attr(np.full(n, NULL, np.int64)) as attr:
            for negate in (False, True):
                with idx.make_mask_where(attr, I64_MIN, I64_MAX, negate) as m:
                    _holds(m, np.zeros(n, bool), n)


# ---- 2. search parity and routes ----------------------------------------------------------------------------------------
# the kept counts on the limits, on both sides of each: 16 384 rows for the exact path and the batched listed mode
# (16 384 * 24 = 393 216 < 393 217 rows: one in 24 holds there too, and 16 385 is past both); one kept row in 24 for the
# list scan and the listed mode (341 * 24 <= 8191 < 342 * 24)
@pytest.mark.parametrize("n,metric,kept", [(393_217, L2, 16_384), (393_217, L2, 16_385), (8_191, COS, 341), (8_191, IP, 342)])
def test_search_parity_on_every_route(hip_lib, n, metric, kept):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(n + kept)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    if metric == COS:
        rows /= np.linalg.norm(rows, axis=1, keepdims=True).astype(np.float32)
    col = _column(rng, n)
    col[col == 7] = 8
    pick = rng.choice(n - 1, kept - 1, replace=False)
    col[pick] = 7
    col[n - 1] = 7  # (the last row: its word's tail is the ballot of lanes past the rows)
    # one quarantined row (an inf element) inside the predicate, one outside it
    q_in = int(pick[0])
    q_out = int(np.flatnonzero((col >= 0) & (col <= 9) & (col != 7))[5])
    rows[q_in, 3] = np.inf
    rows[q_out, 0] = np.inf
    keep = _term(col, n, 7, 7)
    assert int(keep.sum()) == kept and keep[q_in] and not keep[q_out]
    with HipVectorIndex(D, metric) as idx:
        idx.append(0, rows)
        assert idx.counters()["quarantined_rows"] == 2
        with idx.make_attr(col) as attr, idx.make_mask(_bits(keep)) as mb, idx.make_mask_where(attr, 7, 7) as mr:
            _holds(mr, keep, n)
            routes = _every_route(idx, rng, metric, mb, mr)
            if kept == 16_384:  # a lone query reads the kept rows' list by their exact sums; one row more closes that route
                assert routes[(100, "exact")]["exact_scans"] == 1
            if kept == 16_385:
                assert routes[(100, "exact")]["exact_scans"] == 0
        # the complement, dense: NOT (tenant = 7) keeps the other rows that have a value
        with idx.make_attr(col) as attr, idx.make_mask_where(attr, 7, 7, negate=True) as mr:
            inv = _term(col, n, 7, 7, True)
            assert inv[q_out] and not inv[q_in]
            _holds(mr, inv, n)
            with idx.make_mask(_bits(inv)) as mb:
                _every_route(idx, rng, metric, mb, mr, ks=(100,))


# ---- 3. chains ----------------------------------------------------------------------------------------------------------
def test_chains_are_numpys(hip_lib):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(3)
    n, cap = 20_001, 20_480
    rows = rng.standard_normal((n, D)).astype(np.float32)
    tenant, flag = _column(rng, n), _column(rng, n + 9) % 2
    flag[rng.random(n + 9) < 0.1] = NULL
    ts = rng.integers(1_700_000_000, 1_700_001_000, n - 500).astype(np.int64)  # (the last 500 rows have no timestamp)
    a, b = 1_700_000_200, 1_700_000_700
    with HipVectorIndex(D, L2, capacity_rows=cap) as idx:
        idx.append(0, rows)
        with idx.make_attr(tenant) as at, idx.make_attr(ts) as ats, idx.make_attr(flag) as af:
            # tenant IN (3, 7) AND ts BETWEEN a AND b AND NOT flag = 1
            k1 = _term(tenant, n, 3, 3)
            k2 = k1 | _term(tenant, n, 7, 7)
            k3 = k2 & _term(ts, n, a, b)
            k4 = k3 & _term(flag, n, 1, 1, True)
            with idx.make_mask_where(at, 3, 3) as m1, idx.make_mask_where(at, 7, 7, with_mask=m1, combine="or") as m2, \
                    idx.make_mask_where(ats, a, b, with_mask=m2) as m3, \
                    idx.make_mask_where(af, 1, 1, negate=True, with_mask=m3, combine="and") as m4:
                for m, kp in ((m1, k1), (m2, k2), (m3, k3), (m4, k4)):
                    _holds(m, kp, n)
                assert 0 < k4.sum() < k3.sum() < k2.sum()
                with idx.make_mask(_bits(k4)) as mb:
                    _every_route(idx, rng, L2, mb, m4, ks=(100,))
                # an intermediate may go first: every step's handle stands alone
                m2.close()
                m1.close()
                _holds(m4, k4, n)
            # a `with` made from a capacity-sized bitmap, every bit past the last row set: none comes through under OR
            w = rng.random(n) < 0.3
            full = np.ones(cap, bool)
            full[:n] = w
            with idx.make_mask(_bits(full)) as mw:
                assert mw.kept == int(w.sum())
                for combine, want in (("or", k1 | w), ("and", k1 & w)):
                    with idx.make_mask_where(at, 3, 3, with_mask=mw, combine=combine) as m:
                        _holds(m, want, cap, slack=70)
                        with idx.make_mask(_bits(want)) as mb:
                            _pair(idx, _queries(rng, 3), 50, mb, m)
                # NULL under OR: a row without a tenant is kept by `with` alone, negated term or not
                with idx.make_mask_where(at, 3, 3, negate=True, with_mask=mw, combine="or") as m:
                    want = _term(tenant, n, 3, 3, True) | w
                    assert (want & (tenant == NULL)).any()
                    _holds(m, want, cap)


# ---- 4. shard handles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,n", [(12_353, 5_005), (12_837, 4_999)])
def test_shard_handle_reads_the_column_by_global_id(hip_lib, base, n):
    import torch

    from tostore_amd import HipVectorIndex, _ffi
    from tostore_amd.sharded import merge_candidate_blocks

    assert base % 64 in (1, 37) and n % 64 != 0
    rng = np.random.default_rng(base)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    total = base + n + 203
    col = _column(rng, total)  # by GLOBAL row id: the neighbours' values on both sides
    L = _ffi.lib()
    with HipVectorIndex(D, L2, capacity_rows=n, shard_device=0, row_base=base) as idx:
        idx.append(base, rows)
        for lo, hi, negate in ((2, 4, False), (3, 3, False), (3, 3, True)):
            g = np.zeros(total, bool)
            g[base:base + n] = _term(col[base:], n, lo, hi, negate)
            with idx.make_attr(col) as attr, idx.make_mask_where(attr, lo, hi, negate) as mr, idx.make_mask(_bits(g)) as mb:
                _holds(mr, g, total)  # global bits: zero outside [base, base + n)
                k, qs = 40, _queries(rng, 3)
                _pair(idx, qs, k, mb, mr)
                entries = L.tsh_default_block_entries(k)
                bb = L.tsh_candidate_block_bytes(entries)
                merged = []
                for m in (mb, mr):
                    buf = torch.zeros(len(qs) * bb, dtype=torch.uint8, device="cuda")
                    _ffi.check(L.tsh_search_shard_masked(idx._h, qs.ctypes.data_as(_ffi.p_f32), len(qs), k, m.handle(), None, None,
                                                         entries, ctypes.c_void_p(buf.data_ptr()), None))
                    torch.cuda.synchronize()
                    merged.append(merge_candidate_blocks(L2, D, qs, k, None, buf.cpu().numpy(), 1, entries))
                _same(merged[0], merged[1], "tsh_search_shard_masked")
                assert (merged[1][0][:, 0] >= base).all()


# ---- 5. several devices -------------------------------------------------------------------------------------------------
def test_in_process_shards(hip_lib):
    """n_devices = 3 in one process (sharing the one GPU): capacity 70 000 puts the shards at 0, 23 360, 46 720 (the
    library places in-process shards at multiples of 64 rows; a base inside a word is test 4's).  What the rows leave
    ragged is every shard's END: 30 001 rows end the second shard inside a word and a byte (6641 rows) and leave the
    third empty; 50 003 rows fill two shards and end the third after 3283.  The column is 77 rows short of the index."""
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(55)
    os.environ["TSH_SHARDS_SHARE_DEVICES"] = "1"
    _ffi.enable_test_hooks()
    try:
        for cap, n in ((70_000, 30_001), (70_001, 50_003)):
            rows = rng.standard_normal((n, D)).astype(np.float32)
            col = _column(rng, n - 77)
            with HipVectorIndex(D, L2, capacity_rows=cap, n_devices=3) as idx:
                idx.append(0, rows)
                with idx.make_attr(col) as attr:
                    for lo, hi, negate in ((3, 3, False), (2, 6, True)):
                        keep = _term(col, n, lo, hi, negate)
                        with idx.make_mask_where(attr, lo, hi, negate) as mr, idx.make_mask(_bits(keep)) as mb:
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


# ---- 6. snapshot --------------------------------------------------------------------------------------------------------
def test_a_handle_is_a_snapshot(hip_lib):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(6)
    n, more = 5_001, 700
    rows = rng.standard_normal((n + more, D)).astype(np.float32)
    col = _column(rng, n)
    qs = _queries(rng, 3)
    with HipVectorIndex(D, L2, capacity_rows=n + more) as idx:
        idx.append(0, rows[:n])
        attr = idx.make_attr(col)
        old_keep = _term(col, n, 3, 3)
        with idx.make_mask_where(attr, 3, 3) as old:
            before = idx.search(qs, 30, None, old)
            # the column changes under the handle: every 3 becomes a 5, every 4 a 3 -- and the rows to come are all 3
            new_col = col.copy()
            new_col[col == 3] = 5
            new_col[col == 4] = 3
            attr.set(0, new_col)
            attr.set(n, np.full(more, 3, np.int64))
            _holds(old, old_keep, n)
            _same(idx.search(qs, 30, None, old), before, "after tsh_attr_set")
            with idx.make_mask_where(attr, 3, 3) as new:
                _holds(new, _term(new_col, n, 3, 3), n)  # (the column is longer than the index now: 700 values wait)
            # the index grows: no new row is kept, though the column says 3 for each of them
            idx.append(n, rows[n:])
            assert old.kept == int(old_keep.sum())
            grown = np.concatenate([old_keep, np.zeros(more, bool)])
            _holds(old, grown, n + more)
            with idx.make_mask(_bits(old_keep)) as mb:
                _pair(idx, qs, 30, mb, old)
                idx.set_batch_min_nq(2)
                _pair(idx, qs, 30, mb, old)
                idx.set_batch_min_nq(0)
            with idx.make_mask_where(attr, 3, 3) as new:
                _holds(new, np.concatenate([_term(new_col, n, 3, 3), np.ones(more, bool)]), n + more)
            # ... and the handle outlives the column it was made from
            attr.close()
            _holds(old, grown, n + more)
            _same(idx.search(qs, 30, None, old), idx.search(qs, 30, None, _bits(grown)), "after tsh_attr_destroy")
            try:
                idx.make_mask_where(attr, 3, 3)
                raise AssertionError("a closed HipAttr was passed on")
            except ValueError:
                pass


# ---- 7. lifetime and errors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attr_first", [False, True])
def test_orphans_and_foreign_handles(hip_lib, attr_first):
    from tostore_amd import _ffi

    L = _ffi.lib()
    rows = np.random.default_rng(7).standard_normal((100, D)).astype(np.float32)
    col = np.arange(100, dtype=np.int64) % 5
    p64 = col.ctypes.data_as(_ffi.p_i64)

    def index():
        h = ctypes.c_void_p()
        _ffi.check(L.tsh_index_create(D, L2, 0, 1, ctypes.byref(h)))
        _ffi.check(L.tsh_index_append(h, 0, 100, rows.ctypes.data_as(_ffi.p_f32)))
        return h

    a, b = index(), index()
    attr_a, attr_b, mask_a, mask_b, out = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    _ffi.check(L.tsh_attr_create(a, p64, 100, ctypes.byref(attr_a)))
    _ffi.check(L.tsh_attr_create(b, p64, 100, ctypes.byref(attr_b)))
    _ffi.check(L.tsh_mask_create_range(a, attr_a, 1, 2, 0, None, 0, ctypes.byref(mask_a)))
    _ffi.check(L.tsh_mask_create_range(b, attr_b, 1, 2, 0, None, 0, ctypes.byref(mask_b)))
    assert L.tsh_mask_kept(mask_a) == 40
    # an attr, or a with, of another index
    for attr, with_ in ((attr_b, None), (attr_a, mask_b)):
        out.value = 0x20
        assert L.tsh_mask_create_range(a, attr, 1, 2, 0, with_, 1, ctypes.byref(out)) == _ffi.TSH_E_BAD_ARG
        assert "another index" in _ffi.last_error() and not out.value
    # index a goes first: its attr and mask are orphaned, not dangling
    buf = np.full(16, 0xAB, np.uint8)
    _ffi.check(L.tsh_mask_read(mask_a, buf.ctypes.data_as(_ffi.p_u8), 16))
    assert np.array_equal(buf, _bits(_term(col, 100, 1, 2), 16))
    _ffi.check(L.tsh_index_destroy(a))
    out.value = 0x20
    assert L.tsh_mask_create_range(b, attr_a, 1, 2, 0, None, 0, ctypes.byref(out)) == _ffi.TSH_E_BAD_ARG and not out.value
    out.value = 0x20
    assert L.tsh_mask_create_range(b, attr_b, 1, 2, 0, mask_a, 0, ctypes.byref(out)) == _ffi.TSH_E_BAD_ARG and not out.value
    assert L.tsh_attr_set(attr_a, 0, 100, p64) == _ffi.TSH_E_BAD_ARG and "destroyed" in _ffi.last_error()
    buf[:] = 0xAB
    assert L.tsh_mask_read(mask_a, buf.ctypes.data_as(_ffi.p_u8), 16) == _ffi.TSH_E_BAD_ARG and (buf == 0xAB).all()
    assert L.tsh_attr_destroy(attr_a) == _ffi.TSH_OK and L.tsh_mask_destroy(mask_a) == _ffi.TSH_OK
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


# ---- 8. the other entries that take a handle ------------------------------------------------------------------------------
def test_cursor_count_and_grouped_take_the_handle(hip_lib):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(8)
    n = 6_007
    rows = rng.standard_normal((n, D)).astype(np.float32)
    col = _column(rng, n)
    keep = _term(col, n, 2, 6)
    qs = _queries(rng, 3)
    with HipVectorIndex(D, L2) as idx:
        idx.append(0, rows)
        with idx.make_attr(col) as attr, idx.make_mask_where(attr, 2, 6) as mr, idx.make_mask(_bits(keep)) as mb:
            first = idx.search(qs, 20, None, mb)
            cur = (first[1][:, 19].copy(), first[0][:, 19].copy())
            _same(idx.search_after(qs, 20, cur, None, mb), idx.search_after(qs, 20, cur, None, mr), "search_after")
            thr = float(first[1][0, 10])  # (the first query's eleventh distance: at least eleven rows count for it)
            ca, cb = idx.search_count(qs, thr, mb), idx.search_count(qs, thr, mr)
            assert np.array_equal(ca, cb) and ca[0] >= 11 and (ca <= keep.sum()).all()
            assert np.array_equal(idx.search_count(qs, None, mr), np.full(3, keep.sum()))
            with idx.make_groups(np.arange(n, dtype=np.int32) // 7, n // 7 + 1) as g:
                ga, gb = idx.search_grouped(qs, 20, g, None, mb), idx.search_grouped(qs, 20, g, None, mr)
                _same((ga[0], ga[1], ga[3]), (gb[0], gb[1], gb[3]), "search_grouped")
                assert np.array_equal(ga[2], gb[2])
