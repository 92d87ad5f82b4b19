"""GPU: one row set made into a mask handle four ways -- tsh_mask_create from NumPy's bitmap, tsh_mask_create_range,
tsh_mask_create_where with one range term, tsh_mask_create_tags over a tag column that holds the same values -- must be
one row set: the same bitmap byte for byte (NumPy's), the same kept count, the same search, alone and combined with
another handle, before and after an append, whichever of the handle and its index is destroyed first.  The three device
makers share their host side (tsh_lib.hip make_device_mask, mask_device_part); this holds them to each other.

Two indexes, d = 32, L2: (a) three in-process shards on the one device, 50 003 rows of capacity 70 001 (shards of 23 360,
23 360 and 3 283 rows: the last one ends inside a word and a byte and is too short for a list); (b) one shard handle at
row base 12 347 -- inside a byte and a word -- with 4 097 rows, just over the 4 096 from which a part gets a list.  The
column holds 0..99, is 77 rows shorter than the index and NULL at a few rows; `col == 3` keeps about 1 % (the list
route), `col < 50` about half (the dense route)."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2, D = 0, 32
NULL = -(1 << 63)
MORE = 700
PREDICATES = {"eq3": (3, 3), "lt50": (0, 49)}  # inclusive ranges over the column's 0..99


def _bits(keep, n_bytes):
    b = np.packbits(np.asarray(keep, bool), bitorder="little")
    return np.concatenate([b, np.zeros(n_bytes - len(b), np.uint8)])


def _case(which):
    """(base, n, capacity, index arguments, the column by GLOBAL row id, the rows of the shards by local row)"""
    if which == "in_process_shards":
        base, n, cap, kw, shards = 0, 50_003, 70_001, dict(n_devices=3), [(0, 23_360), (23_360, 46_720), (46_720, 50_003)]
    else:
        base, n, cap, kw, shards = 12_347, 4_097, 4_097 + MORE, dict(shard_device=0, row_base=12_347), [(12_347, 12_347 + 4_097)]
    rng = np.random.default_rng(2024 + base)
    col = rng.integers(0, 100, base + n - 77).astype(np.int64)
    col[rng.choice(len(col), 41, replace=False)] = NULL
    col[base + 5] = col[base + n - 78] = NULL  # (a few inside the index's rows whatever the base)
    return base, n, cap, kw, col, shards, rng


def _keep(col, base, n, pred):
    """the specification, by GLOBAL row id: rows [base, base + n) that have a value inside the predicate's range"""
    lo, hi = PREDICATES[pred]
    v = np.full(base + n, NULL, np.int64)
    v[:len(col)] = col
    keep = (v != NULL) & (v >= lo) & (v <= hi)
    keep[:base] = False
    return keep


def _check_case_table(col, base, n, shards):
    """the NumPy side alone, before anything is made: `col == 3` keeps 0.2 % .. 3 % of every shard's rows, `col < 50` more
    than a third, and no shard is empty"""
    for lo, hi in shards:
        assert hi > lo
        few = _keep(col, base, n, "eq3")[lo:hi].mean()
        many = _keep(col, base, n, "lt50")[lo:hi].mean()
        assert 0.002 <= few <= 0.03 and many > 1 / 3, (lo, hi, few, many)


def _search(idx, qs, m):
    ids, dist, cnt = idx.search(qs, 20, None, m)
    return ids.copy(), dist.copy().view(np.uint64), cnt.copy()


def _one_row_set(idx, qs, handles, keep, end):
    """every handle holds `keep` (GLOBAL bits, zero to `end` and past it), keeps as many rows, and searches alike"""
    nb = (end + 7) // 8 + 9
    want = _bits(keep, nb)
    first = None
    for name, m in handles.items():
        got = m.bits(nb)
        assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:8])
        assert m.kept == int(np.count_nonzero(keep)), name
        res = _search(idx, qs, m)
        if first is None:
            first = res
        for a, b in zip(first, res):
            assert np.array_equal(a, b), name


@pytest.mark.parametrize("which", ["in_process_shards", "shard_handle"])
def test_four_makers_one_row_set(hip_lib, which):
    from tostore_amd import HipVectorIndex, WhereRange, _ffi

    base, n, cap, kw, col, shards, rng = _case(which)
    _check_case_table(col, base, n, shards)
    rows = rng.standard_normal((n + MORE, D)).astype(np.float32)
    qs = rng.standard_normal((3, D)).astype(np.float32)
    L = _ffi.lib()
    shared = which == "in_process_shards"
    if shared:
        os.environ["TSH_SHARDS_SHARE_DEVICES"] = "1"
        _ffi.enable_test_hooks()
    idx = None
    try:
        idx = HipVectorIndex(D, L2, capacity_rows=cap, **kw)
        idx.append(base, rows[:n])
        idx.set_batch_min_nq(0)
        attr = idx.make_attr(col)
        tags = idx.make_tags((np.arange(len(col) + 1, dtype=np.int64), col))  # row i: the one value col[i]; NULL stays NULL
        even = np.zeros(base + n, bool)
        even[base:len(col)] = (col[base:] != NULL) & (col[base:] % 2 == 0)
        m_even = idx.make_mask(_bits(even, (base + n + 7) // 8))
        made = {}
        for pred, (lo, hi) in PREDICATES.items():
            keep = _keep(col, base, n, pred)
            values = np.arange(lo, hi + 1, dtype=np.int64)
            makers = {
                "range": lambda w=None, c="and": idx.make_mask_where(attr, lo, hi, False, w, c),
                "where": lambda w=None, c="and": idx.make_mask_clauses([[WhereRange(attr, lo, hi)]], w, c),
                "tags": lambda w=None, c="and": idx.make_mask_tags(tags, values, "any", False, w, c),
            }
            handles = {"bitmap": idx.make_mask(_bits(keep, (base + n + 7) // 8))}
            handles.update({name: make() for name, make in makers.items()})
            _one_row_set(idx, qs, handles, keep, base + n)
            for combine, both in (("and", keep & even), ("or", keep | even)):
                for name, make in makers.items():
                    with make(m_even, combine) as m:
                        nb = (base + n + 7) // 8 + 9
                        assert np.array_equal(m.bits(nb), _bits(both, nb)), (pred, name, combine)
                        assert m.kept == int(np.count_nonzero(both)), (pred, name, combine)
            made[pred] = (handles, keep)
        # the index grows: every handle is a snapshot, rebuilt from its own bitmap -- none keeps a new row
        idx.append(base + n, rows[n:])
        for pred, (handles, keep) in made.items():
            _one_row_set(idx, qs, handles, np.concatenate([keep, np.zeros(MORE, bool)]), base + n + MORE)
        # one predicate's handles go before the index, the other's after it
        m_even.close()
        attr.close()
        tags.close()
        for m in made["eq3"][0].values():
            assert L.tsh_mask_destroy(m._h) == _ffi.TSH_OK
            m._h = ctypes.c_void_p()
        assert L.tsh_index_destroy(idx._h) == _ffi.TSH_OK
        idx._h = ctypes.c_void_p()
        for m in made["lt50"][0].values():
            assert L.tsh_mask_destroy(m._h) == _ffi.TSH_OK
            m._h = ctypes.c_void_p()
    finally:
        if idx is not None:
            idx.close()
        if shared:
            _ffi.enable_test_hooks(False)
            del os.environ["TSH_SHARDS_SHARE_DEVICES"]
