"""CPU: the count entries of the C ABI (tsh_search_count / tsh_search_count_stats) validate their arguments before anything
else, refuse to compute without a device instead of falling back, and are bound by the ctypes table, the Python index
and the Dart bridge.  (Calls that need an index run on the GPU: tests/test_gpu_search_count.py; the window and the exact
predicate are held to the specification by tests/test_host_count_window.py.)"""
import ctypes
import inspect
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_argument_validation_comes_first():
    from tostore_amd import _ffi

    L = _ffi.lib()
    q, a_dist, a_id, cnt = np.zeros((1, 4), np.float32), np.zeros(1), np.zeros(1, np.int64), np.full(1, 99, np.int64)
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    some_mask = np.ones(8, np.uint8)
    fake_handle = ctypes.c_void_p(0x10)  # never dereferenced: both forms of a mask at once are refused first
    rc = L.tsh_search_count(None, p(q, _ffi.p_f32), 1, math.nan, p(some_mask, _ffi.p_u8), fake_handle, None, None, p(cnt, _ffi.p_i64))
    assert rc == _ffi.TSH_E_BAD_ARG and "both" in _ffi.last_error()
    for ad, ai in ((None, p(a_id, _ffi.p_i64)), (p(a_dist, _ffi.p_f64), None)):  # exactly one NULL cursor array
        rc = L.tsh_search_count(None, p(q, _ffi.p_f32), 1, math.nan, None, None, ad, ai, p(cnt, _ffi.p_i64))
        assert rc == _ffi.TSH_E_BAD_ARG and "after_" in _ffi.last_error()
    out = (ctypes.c_int64 * 4)()
    assert L.tsh_search_count_stats(None, out) == _ffi.TSH_E_BAD_ARG
    assert cnt[0] == 99


def test_no_device_is_an_error_not_a_fallback():
    """Without a device no index exists: a count on "no index" says so, with or without a cursor."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    q, a_dist, a_id, cnt = np.zeros((1, 4), np.float32), np.zeros(1), np.zeros(1, np.int64), np.full(1, 99, np.int64)
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    want = _ffi.TSH_E_NO_DEVICE if L.tsh_device_count() <= 0 else _ffi.TSH_E_BAD_ARG
    assert L.tsh_search_count(None, p(q, _ffi.p_f32), 1, 1.0, None, None, None, None, p(cnt, _ffi.p_i64)) == want
    assert L.tsh_search_count(None, p(q, _ffi.p_f32), 1, 1.0, None, None, p(a_dist, _ffi.p_f64), p(a_id, _ffi.p_i64), p(cnt, _ffi.p_i64)) == want
    if want == _ffi.TSH_E_NO_DEVICE:
        assert "no HIP device" in _ffi.last_error()
    assert cnt[0] == 99  # nothing was answered


def test_bindings_name_the_entries():
    from tostore_amd import HipVectorIndex, _ffi

    for name in ("tsh_search_count", "tsh_search_count_stats"):
        assert name in _ffi.SIGNATURES
    assert list(inspect.signature(HipVectorIndex.search_count).parameters) == ["self", "queries", "distance_threshold", "row_mask", "after"]
    assert callable(getattr(HipVectorIndex, "search_count_stats", None))
    with open(os.path.join(ROOT, "tostore_amd", "dart", "tostore_hip_bridge.dart")) as f:
        dart = f.read()
    for name in ("tsh_search_count", "tsh_search_count_stats"):
        assert re.search(r"'%s'" % name, dart), name
    assert re.search(r"\bsearchCount\(", dart) and re.search(r"\bsearchCountStats\(", dart)
    with open(os.path.join(ROOT, "include", "tostore_hip.h")) as f:
        header = f.read()
    assert re.search(r"Additive since.*tsh_search_count, tsh_search_count_stats", header, flags=re.S)
    assert re.search(r"#define TSH_ABI_VERSION 5\b", header)
