"""CPU: the grouped-search entries of the C ABI (tsh_groups_create / _set / _destroy, tsh_search_grouped,
tsh_search_grouped_stats) exist with their ctypes prototypes, validate their arguments before any device work, refuse to
compute without a device instead of falling back, and are named by the header's additive list, the Python index and the
Dart bridge with matching arity.  (Calls that need an index run on the GPU: tests/test_gpu_search_grouped.py; the rules
are held to the specification by tests/test_host_group_rule.py.)"""
import ctypes
import inspect
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tsh_groups_create", "tsh_groups_set", "tsh_groups_destroy", "tsh_search_grouped", "tsh_search_grouped_stats")
ARITY = {"tsh_groups_create": 5, "tsh_groups_set": 4, "tsh_groups_destroy": 1, "tsh_search_grouped": 12, "tsh_search_grouped_stats": 2}


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
    assert _ffi.SIGNATURES["tsh_search_grouped"][1] == [_ffi.p_void, _ffi.p_f32, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, _ffi.p_u8,
                                                        _ffi.p_void, _ffi.p_void, _ffi.p_i64, _ffi.p_f64, _ffi.p_i32, _ffi.p_i32]
    # (the address of the handle to fill travels as void *, as the header declares it)
    assert _ffi.SIGNATURES["tsh_groups_create"][1] == [_ffi.p_void, _ffi.p_i32, ctypes.c_int64, ctypes.c_int32, _ffi.p_void]


def test_argument_validation_comes_first():
    """Nothing here has an index or a device behind it: every call is refused on its arguments alone."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    q = np.zeros((1, 4), np.float32)
    ids, dist, grp, cnt = np.full(3, 77, np.int64), np.zeros(3), np.zeros(3, np.int32), np.full(1, 99, np.int32)
    fake = ctypes.c_void_p(0x10)  # never dereferenced: the checks below come before any use of a handle
    some_mask = np.ones(8, np.uint8)

    def grouped(row_mask, mask, groups):
        return L.tsh_search_grouped(None, _p(q, _ffi.p_f32), 1, 3, math.nan, row_mask, mask, groups, _p(ids, _ffi.p_i64), _p(dist, _ffi.p_f64),
                                    _p(grp, _ffi.p_i32), _p(cnt, _ffi.p_i32))

    assert grouped(None, None, None) == _ffi.TSH_E_BAD_ARG and "groups is NULL" in _ffi.last_error()
    assert grouped(_p(some_mask, _ffi.p_u8), fake, fake) == _ffi.TSH_E_BAD_ARG and "both" in _ffi.last_error()
    assert cnt[0] == 99 and ids[0] == 77

    out = ctypes.c_void_p(0x20)
    g = np.array([0, 1, -1, 2], np.int32)
    assert L.tsh_groups_create(None, _p(g, _ffi.p_i32), 4, (1 << 26) + 1, ctypes.byref(out)) == _ffi.TSH_E_BAD_ARG
    assert "n_groups" in _ffi.last_error() and not out.value  # (*out is cleared on every failure)
    assert L.tsh_groups_create(None, _p(g, _ffi.p_i32), 4, -1, ctypes.byref(out)) == _ffi.TSH_E_BAD_ARG
    assert L.tsh_groups_create(None, _p(g, _ffi.p_i32), 4, 2, ctypes.byref(out)) == _ffi.TSH_E_BAD_ARG  # the id 2 is not below 2
    assert "group_of[3]" in _ffi.last_error()
    assert L.tsh_groups_create(None, None, 4, 8, ctypes.byref(out)) == _ffi.TSH_E_BAD_ARG
    assert L.tsh_groups_create(None, _p(g, _ffi.p_i32), -1, 8, ctypes.byref(out)) == _ffi.TSH_E_BAD_ARG
    assert L.tsh_groups_create(None, _p(g, _ffi.p_i32), 4, 8, None) == _ffi.TSH_E_BAD_ARG
    assert L.tsh_groups_set(None, 0, 4, _p(g, _ffi.p_i32)) == _ffi.TSH_E_BAD_ARG
    assert L.tsh_groups_destroy(None) == _ffi.TSH_OK
    stats = (ctypes.c_int64 * 4)()
    assert L.tsh_search_grouped_stats(None, stats) == _ffi.TSH_E_BAD_ARG


def test_no_device_is_an_error_not_a_fallback():
    """Without a device no index exists: valid arguments on "no index" say so."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    q = np.zeros((1, 4), np.float32)
    ids, dist, grp, cnt = np.full(3, 77, np.int64), np.zeros(3), np.zeros(3, np.int32), np.full(1, 99, np.int32)
    want = _ffi.TSH_E_NO_DEVICE if L.tsh_device_count() <= 0 else _ffi.TSH_E_BAD_ARG
    fake = ctypes.c_void_p(0x10)  # never dereferenced: "no index" is answered first
    rc = L.tsh_search_grouped(None, _p(q, _ffi.p_f32), 1, 3, math.nan, None, None, fake, _p(ids, _ffi.p_i64), _p(dist, _ffi.p_f64),
                              _p(grp, _ffi.p_i32), _p(cnt, _ffi.p_i32))
    assert rc == want
    out = ctypes.c_void_p()
    g = np.array([0, 1, -1, 2], np.int32)
    assert L.tsh_groups_create(None, _p(g, _ffi.p_i32), 4, 8, ctypes.byref(out)) == want and not out.value
    if want == _ffi.TSH_E_NO_DEVICE:
        assert "no HIP device" in _ffi.last_error()
    assert cnt[0] == 99 and ids[0] == 77  # nothing was answered


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
            try:
                b.search_grouped(rows[0], 2, ga)
                raise AssertionError("a groups handle of another index was accepted")
            except RuntimeError as e:
                assert "another index" in str(e)
            try:
                a.search_grouped(rows[0], 2, ga, row_mask=mb)
                raise AssertionError("a mask handle of another index was accepted")
            except RuntimeError as e:
                assert "another index" in str(e)


def test_bindings_name_the_entries():
    from tostore_amd import HipGroups, HipVectorIndex, VectorIndexManager

    assert list(inspect.signature(HipVectorIndex.search_grouped).parameters) == ["self", "queries", "k", "groups", "distance_threshold", "row_mask"]
    assert list(inspect.signature(HipVectorIndex.make_groups).parameters) == ["self", "group_of", "n_groups"]
    assert callable(getattr(HipVectorIndex, "search_grouped_stats", None))
    assert callable(getattr(HipGroups, "set", None)) and hasattr(HipGroups, "__enter__") and hasattr(HipGroups, "close")
    assert "group_by" in inspect.signature(VectorIndexManager.vectorSearch).parameters
    with open(os.path.join(ROOT, "include", "tostore_hip.h")) as f:
        header = f.read()
    assert re.search(r"Additive since.*tsh_search_count, tsh_search_count_stats;\s*\*\s*tsh_groups_create, tsh_groups_set, tsh_groups_destroy, "
                     r"tsh_search_grouped, tsh_search_grouped_stats\. \*/", header, flags=re.S)
    assert re.search(r"#define TSH_ABI_VERSION 5\b", header)
    with open(os.path.join(ROOT, "tostore_amd", "dart", "tostore_hip_bridge.dart")) as f:
        dart = f.read()
    for name in NAMES:
        # the C declaration's arity ...
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == ARITY[name], name
        # ... and the Dart typedef the symbol is looked up with
        m = re.search(r"lookupFunction<(\w+), (\w+)>\('%s'\)" % name, dart)
        assert m, name
        for td in m.groups():
            t = re.search(r"typedef %s = \w+ Function\(([^;]*)\);" % td, dart)
            assert t, td
            assert len(re.sub(r"<[^<>]*(<[^<>]*>)?[^<>]*>", "", t.group(1)).split(",")) == ARITY[name], td
    assert re.search(r"\bclass HipRowGroups\b", dart) and re.search(r"\bsearchGrouped\(", dart) and re.search(r"\bsearchGroupedStats\(", dart)
    assert re.search(r"searchGrouped with a disposed HipRowGroups", dart)
