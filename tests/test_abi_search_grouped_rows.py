"""CPU: the rows-per-group entries of the C ABI (tsh_search_grouped_rows, tsh_search_grouped_rows_stats) exist with their
ctypes prototypes, validate their arguments before any device work and leave the output buffers alone when they refuse,
refuse to compute without a device instead of falling back, and are named by the header's additive list, the Python index,
the manager and the Dart bridge with matching arity.  (Calls that need an index run on the GPU:
tests/test_gpu_search_grouped_rows.py; the rules are held to the specification by tests/test_host_group_rows_rule.py.)"""
import ctypes
import inspect
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tsh_search_grouped_rows", "tsh_search_grouped_rows_stats")
ARITY = {"tsh_search_grouped_rows": 14, "tsh_search_grouped_rows_stats": 2}


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
    # tsh_search_grouped's arguments with rows_per_group behind k and out_rows behind out_group
    g = list(_ffi.SIGNATURES["tsh_search_grouped"][1])
    assert _ffi.SIGNATURES["tsh_search_grouped_rows"][1] == g[:4] + [ctypes.c_int32] + g[4:11] + [_ffi.p_i32] + g[11:]
    assert _ffi.SIGNATURES["tsh_search_grouped_rows_stats"][1] == [_ffi.p_void, _ffi.p_i64]


def _buffers():
    return np.full(6, 77, np.int64), np.full(6, 5.5), np.full(3, 42, np.int32), np.full(3, 43, np.int32), np.full(1, 99, np.int32)


def test_argument_validation_comes_first():
    """Nothing here has an index or a device behind it: every call is refused on its arguments alone, and what it was
    given to fill stays as it was."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    q = np.zeros((1, 4), np.float32)
    ids, dist, grp, rows, cnt = _buffers()
    fake = ctypes.c_void_p(0x10)  # never dereferenced: the checks below come before any use of a handle
    some_mask = np.ones(8, np.uint8)

    def call(m, row_mask, mask, groups, k=3):
        return L.tsh_search_grouped_rows(None, _p(q, _ffi.p_f32), 1, k, m, math.nan, row_mask, mask, groups, _p(ids, _ffi.p_i64), _p(dist, _ffi.p_f64),
                                         _p(grp, _ffi.p_i32), _p(rows, _ffi.p_i32), _p(cnt, _ffi.p_i32))

    assert call(2, None, None, None) == _ffi.TSH_E_BAD_ARG and "groups is NULL" in _ffi.last_error()
    assert call(2, _p(some_mask, _ffi.p_u8), fake, fake) == _ffi.TSH_E_BAD_ARG and "both" in _ffi.last_error()
    for m in (0, -1, 65, 1 << 20):
        assert call(m, None, None, fake) == _ffi.TSH_E_BAD_ARG, m
        assert "rows_per_group" in _ffi.last_error() and "[1, 64]" in _ffi.last_error()
    assert call(65, None, None, fake, k=0) == _ffi.TSH_E_BAD_ARG  # (above the range there is no trivial case)
    want = _buffers()
    for got, w in zip((ids, dist, grp, rows, cnt), want):
        assert np.array_equal(got, w)
    stats = (ctypes.c_int64 * 5)()
    assert L.tsh_search_grouped_rows_stats(None, stats) == _ffi.TSH_E_BAD_ARG


def test_no_device_is_an_error_not_a_fallback():
    """Without a device no index exists: valid arguments on "no index" say so."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    q = np.zeros((1, 4), np.float32)
    ids, dist, grp, rows, cnt = _buffers()
    want = _ffi.TSH_E_NO_DEVICE if L.tsh_device_count() <= 0 else _ffi.TSH_E_BAD_ARG
    fake = ctypes.c_void_p(0x10)  # never dereferenced: "no index" is answered first
    for m in (1, 2, 64):
        rc = L.tsh_search_grouped_rows(None, _p(q, _ffi.p_f32), 1, 3, m, math.nan, None, None, fake, _p(ids, _ffi.p_i64), _p(dist, _ffi.p_f64),
                                       _p(grp, _ffi.p_i32), _p(rows, _ffi.p_i32), _p(cnt, _ffi.p_i32))
        assert rc == want
        if want == _ffi.TSH_E_NO_DEVICE:
            assert "no HIP device" in _ffi.last_error()
    assert cnt[0] == 99 and ids[0] == 77 and rows[0] == 43  # nothing was answered


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
                b.search_grouped_rows(rows[0], 2, 2, ga)
                raise AssertionError("a groups handle of another index was accepted")
            except RuntimeError as e:
                assert "another index" in str(e)
            try:
                a.search_grouped_rows(rows[0], 2, 2, ga, row_mask=mb)
                raise AssertionError("a mask handle of another index was accepted")
            except RuntimeError as e:
                assert "another index" in str(e)


def test_bindings_name_the_entries():
    from tostore_amd import HipVectorIndex, VectorIndexManager

    assert list(inspect.signature(HipVectorIndex.search_grouped_rows).parameters) == ["self", "queries", "k", "rows_per_group", "groups",
                                                                                      "distance_threshold", "row_mask"]
    assert callable(getattr(HipVectorIndex, "search_grouped_rows_stats", None))
    assert list(inspect.signature(VectorIndexManager.vectorSearchGroups).parameters) == ["self", "queryVector", "group_by", "topK", "groupSize",
                                                                                         "distanceThreshold", "rowMask", "pk_of"]
    sig = inspect.signature(VectorIndexManager.vectorSearchGroups)
    assert sig.parameters["topK"].default == 10 and sig.parameters["groupSize"].default == 3
    with open(os.path.join(ROOT, "include", "tostore_hip.h")) as f:
        header = f.read()
    assert re.search(r"Additive since[^/]*tsh_search_grouped_rows, tsh_search_grouped_rows_stats\. \*/", header)
    assert re.search(r"#define TSH_ABI_VERSION 5\b", header)  # additive: the number does not move
    for word in ("EXACT-ALL", "Out of scope", "quarantined", "span"):
        assert word in header[header.index("grouped search, several rows per group"):], word
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
    assert re.search(r"\bsearchGroupedRows\(", dart) and re.search(r"\bsearchGroupedRowsStats\(", dart)
    assert re.search(r"searchGroupedRows with a disposed HipRowGroups", dart)
    # the rule header is host-only: no HIP in it, and the kernels take its functions as they stand
    with open(os.path.join(ROOT, "tostore_amd", "csrc", "tsh_group_rows_rule.h")) as f:
        rule = f.read()
    assert "hip_runtime" not in rule and "group_rows_cut" in rule and "TSH_GROUP_HD" in rule
