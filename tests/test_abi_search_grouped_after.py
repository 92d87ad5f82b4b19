"""CPU: the grouped cursor search's and the group count's entries of the C ABI (tsh_search_grouped_after,
tsh_search_grouped_count, tsh_search_grouped_after_stats) exist with their ctypes prototypes, validate their arguments
before any device work, refuse to compute without a device instead of falling back, and are named by the header's additive
list, the Python index, the host mirror and the Dart bridge with matching arity.  (Calls that need an index run on the
GPU: tests/test_gpu_search_grouped_after.py; the rules are held to the specification by
tests/test_host_group_after_rule.py.)"""
import ctypes
import inspect
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tsh_search_grouped_after", "tsh_search_grouped_count", "tsh_search_grouped_after_stats")
ARITY = {"tsh_search_grouped_after": 14, "tsh_search_grouped_count": 10, "tsh_search_grouped_after_stats": 2}


def _p(a, t):
    return a.ctypes.data_as(t)


def test_symbols_and_prototypes():
    from tostore_amd import _ffi

    L = _ffi.lib()
    for name in NAMES:
        assert name in _ffi.SIGNATURES, name
        fn = getattr(L, name)  # the shared library exports it
        restype, argtypes = _ffi.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
        assert len(argtypes) == ARITY[name]
    # tsh_search_grouped's arguments with the two cursor arrays behind the groups handle
    g = list(_ffi.SIGNATURES["tsh_search_grouped"][1])
    assert _ffi.SIGNATURES["tsh_search_grouped_after"][1] == g[:8] + [_ffi.p_f64, _ffi.p_i64] + g[8:]
    # tsh_search_count's arguments with the groups handle behind the mask
    c = list(_ffi.SIGNATURES["tsh_search_count"][1])
    assert _ffi.SIGNATURES["tsh_search_grouped_count"][1] == c[:6] + [_ffi.p_void] + c[6:]


def test_argument_validation_comes_first():
    """Nothing here has an index or a device behind it: every call is refused on its arguments alone."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    q = np.zeros((1, 4), np.float32)
    ids, dist, grp, cnt = np.full(3, 77, np.int64), np.zeros(3), np.zeros(3, np.int32), np.full(1, 99, np.int32)
    n64 = np.full(1, 99, np.int64)
    a_dist, a_id = np.zeros(1, np.float64), np.zeros(1, np.int64)
    fake = ctypes.c_void_p(0x10)  # never dereferenced: the checks below come before any use of a handle
    some_mask = np.ones(8, np.uint8)

    def page(row_mask, mask, groups, ad, ai):
        return L.tsh_search_grouped_after(None, _p(q, _ffi.p_f32), 1, 3, math.nan, row_mask, mask, groups, ad, ai, _p(ids, _ffi.p_i64),
                                          _p(dist, _ffi.p_f64), _p(grp, _ffi.p_i32), _p(cnt, _ffi.p_i32))

    def count(row_mask, mask, groups, ad, ai):
        return L.tsh_search_grouped_count(None, _p(q, _ffi.p_f32), 1, math.nan, row_mask, mask, groups, ad, ai, _p(n64, _ffi.p_i64))

    pd, pi = _p(a_dist, _ffi.p_f64), _p(a_id, _ffi.p_i64)
    assert page(None, None, None, pd, pi) == _ffi.TSH_E_BAD_ARG and "groups is NULL" in _ffi.last_error()
    assert page(_p(some_mask, _ffi.p_u8), fake, fake, pd, pi) == _ffi.TSH_E_BAD_ARG and "both" in _ffi.last_error()
    for ad, ai in ((None, None), (pd, None), (None, pi)):  # a page needs its cursor
        assert page(None, None, fake, ad, ai) == _ffi.TSH_E_BAD_ARG and "after_dist / after_id is NULL" in _ffi.last_error()
    assert count(None, None, None, pd, pi) == _ffi.TSH_E_BAD_ARG and "groups is NULL" in _ffi.last_error()
    assert count(_p(some_mask, _ffi.p_u8), fake, fake, None, None) == _ffi.TSH_E_BAD_ARG and "both" in _ffi.last_error()
    for ad, ai in ((pd, None), (None, pi)):  # a count takes both arrays or neither
        assert count(None, None, fake, ad, ai) == _ffi.TSH_E_BAD_ARG and "both or neither" in _ffi.last_error()
    assert cnt[0] == 99 and ids[0] == 77 and n64[0] == 99
    stats = (ctypes.c_int64 * 5)()
    assert L.tsh_search_grouped_after_stats(None, stats) == _ffi.TSH_E_BAD_ARG


def test_no_device_is_an_error_not_a_fallback():
    """Without a device no index exists: valid arguments on "no index" say so."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    q = np.zeros((1, 4), np.float32)
    ids, dist, grp, cnt = np.full(3, 77, np.int64), np.zeros(3), np.zeros(3, np.int32), np.full(1, 99, np.int32)
    n64 = np.full(1, 99, np.int64)
    a_dist, a_id = np.zeros(1, np.float64), np.zeros(1, np.int64)
    want = _ffi.TSH_E_NO_DEVICE if L.tsh_device_count() <= 0 else _ffi.TSH_E_BAD_ARG
    fake = ctypes.c_void_p(0x10)  # never dereferenced: "no index" is answered first
    rc = L.tsh_search_grouped_after(None, _p(q, _ffi.p_f32), 1, 3, math.nan, None, None, fake, _p(a_dist, _ffi.p_f64), _p(a_id, _ffi.p_i64),
                                    _p(ids, _ffi.p_i64), _p(dist, _ffi.p_f64), _p(grp, _ffi.p_i32), _p(cnt, _ffi.p_i32))
    assert rc == want
    for ad, ai in ((None, None), (_p(a_dist, _ffi.p_f64), _p(a_id, _ffi.p_i64))):
        assert L.tsh_search_grouped_count(None, _p(q, _ffi.p_f32), 1, math.nan, None, None, fake, ad, ai, _p(n64, _ffi.p_i64)) == want
    if want == _ffi.TSH_E_NO_DEVICE:
        assert "no HIP device" in _ffi.last_error()
    assert cnt[0] == 99 and ids[0] == 77 and n64[0] == 99  # nothing was answered


def test_a_handle_of_another_index_is_refused():
    """Needs two indexes, so a device: where there is none, creating an index is itself refused (not a fallback)."""
    from tostore_amd import HipVectorIndex, _ffi

    if _ffi.lib().tsh_device_count() <= 0:
        h = ctypes.c_void_p()
        assert _ffi.lib().tsh_index_create(4, 0, 0, 1, ctypes.byref(h)) == _ffi.TSH_E_NO_DEVICE
        return
    rows = np.eye(4, dtype=np.float32)
    with HipVectorIndex(4, 0) as a, HipVectorIndex(4, 0) as b:
        a.append(0, rows)
        b.append(0, rows)
        with a.make_groups([0, 0, 1, 1], 2) as ga, b.make_mask(np.array([0xFF], np.uint8)) as mb:
            for call in (lambda: b.search_grouped_after(rows[0], 2, ga, (-math.inf, 0)), lambda: b.count_groups(rows[0], ga),
                         lambda: a.search_grouped_after(rows[0], 2, ga, (-math.inf, 0), row_mask=mb), lambda: a.count_groups(rows[0], ga, row_mask=mb)):
                try:
                    call()
                    raise AssertionError("a handle of another index was accepted")
                except RuntimeError as e:
                    assert "another index" in str(e)


def test_bindings_name_the_entries():
    from tostore_amd import HipVectorIndex, VectorIndexManager

    assert list(inspect.signature(HipVectorIndex.search_grouped_after).parameters) == ["self", "queries", "k", "groups", "after", "distance_threshold",
                                                                                       "row_mask"]
    assert list(inspect.signature(HipVectorIndex.count_groups).parameters) == ["self", "queries", "groups", "distance_threshold", "row_mask", "after"]
    assert callable(getattr(HipVectorIndex, "search_grouped_after_stats", None))
    assert callable(getattr(VectorIndexManager, "vectorSearchGroupedAfter", None)) and callable(getattr(VectorIndexManager, "countGroups", None))
    with open(os.path.join(ROOT, "include", "tostore_hip.h")) as f:
        header = f.read()
    assert re.search(r"Additive since[^/]*tsh_search_grouped_after, tsh_search_grouped_count,\s*\*\s*tsh_search_grouped_after_stats\. \*/", header)
    assert re.search(r"#define TSH_ABI_VERSION 5\b", header)
    with open(os.path.join(ROOT, "tostore_amd", "dart", "tostore_hip_bridge.dart")) as f:
        dart = f.read()
    for name in NAMES:
        # the C declaration's arity ...
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == ARITY[name], name
        # ... and the Dart typedef the symbol is looked up with
        m = re.search(r"lookupFunction<(\w+),\s*(\w+)>\(\s*'%s'\)" % name, dart)
        assert m, name
        for td in m.groups():
            t = re.search(r"typedef %s = \w+ Function\(([^;]*)\);" % td, dart)
            assert t, td
            assert len(re.sub(r"<[^<>]*(<[^<>]*>)?[^<>]*>", "", t.group(1)).split(",")) == ARITY[name], td
    assert re.search(r"\bsearchGroupedAfter\(", dart) and re.search(r"\bcountGroups\(", dart) and re.search(r"\bsearchGroupedAfterStats\(", dart)
    assert re.search(r"searchGroupedAfter with a disposed HipRowGroups", dart) and re.search(r"countGroups with a disposed HipRowGroups", dart)
    assert re.search(r"searchGroupedAfter with a disposed HipRowMask", dart) and re.search(r"countGroups with a disposed HipRowMask", dart)
