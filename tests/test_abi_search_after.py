"""CPU: the cursor entries of the C ABI (tsh_search_after / tsh_search_submit_after / tsh_search_after_stats) validate
their arguments before anything else, refuse to compute without a device instead of falling back, and are bound by
the ctypes table, the Python index and the Dart bridge.  (Calls that need an index -- nq = 0, k <= 0 -> OK with
counts 0 -- run on the GPU: tests/test_gpu_search_after.py; the finaliser's cursor filter is held to the compareTo
order by tests/test_host_after_band.py.)"""
import ctypes
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(nq=1, k=3, d=4):
    q = np.zeros((nq, d), np.float32)
    a_dist = np.full(nq, -math.inf, np.float64)
    a_id = np.zeros(nq, np.int64)
    ids = np.zeros((nq, k), np.int64)
    dist = np.zeros((nq, k), np.float64)
    cnt = np.full(nq, 99, np.int32)
    return q, a_dist, a_id, ids, dist, cnt


def test_argument_validation_comes_first():
    from tostore_amd import _ffi

    L = _ffi.lib()
    q, a_dist, a_id, ids, dist, cnt = _args()
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    some_mask = np.ones(8, np.uint8)
    fake_handle = ctypes.c_void_p(0x10)  # never dereferenced: both forms of a mask at once are refused first
    rc = L.tsh_search_after(None, p(q, _ffi.p_f32), 1, 3, math.nan, p(some_mask, _ffi.p_u8), fake_handle, p(a_dist, _ffi.p_f64),
                            p(a_id, _ffi.p_i64), p(ids, _ffi.p_i64), p(dist, _ffi.p_f64), p(cnt, _ffi.p_i32))
    assert rc == _ffi.TSH_E_BAD_ARG and "both" in _ffi.last_error()
    for ad, ai in ((None, p(a_id, _ffi.p_i64)), (p(a_dist, _ffi.p_f64), None), (None, None)):
        rc = L.tsh_search_after(None, p(q, _ffi.p_f32), 1, 3, math.nan, None, None, ad, ai, p(ids, _ffi.p_i64),
                                p(dist, _ffi.p_f64), p(cnt, _ffi.p_i32))
        assert rc == _ffi.TSH_E_BAD_ARG and "after_" in _ffi.last_error()
    t = ctypes.c_int32(5)
    rc = L.tsh_search_submit_after(None, p(q, _ffi.p_f32), 3, p(some_mask, _ffi.p_u8), fake_handle, 0.0, 0, ctypes.byref(t))
    assert rc == _ffi.TSH_E_BAD_ARG
    out = (ctypes.c_int64 * 4)()
    assert L.tsh_search_after_stats(None, out) == _ffi.TSH_E_BAD_ARG


def test_no_device_is_an_error_not_a_fallback():
    """Without a device no index exists: a cursor search on "no index" says so, as every compute entry does."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    q, a_dist, a_id, ids, dist, cnt = _args()
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    want = _ffi.TSH_E_NO_DEVICE if L.tsh_device_count() <= 0 else _ffi.TSH_E_BAD_ARG
    rc = L.tsh_search_after(None, p(q, _ffi.p_f32), 1, 3, math.nan, None, None, p(a_dist, _ffi.p_f64), p(a_id, _ffi.p_i64),
                            p(ids, _ffi.p_i64), p(dist, _ffi.p_f64), p(cnt, _ffi.p_i32))
    assert rc == want
    t = ctypes.c_int32(5)
    assert L.tsh_search_submit_after(None, p(q, _ffi.p_f32), 3, None, None, 0.0, 0, ctypes.byref(t)) == want
    if want == _ffi.TSH_E_NO_DEVICE:
        assert "no HIP device" in _ffi.last_error()
    assert cnt[0] == 99 and not ids.any()  # nothing was answered


def test_bindings_name_the_entries():
    from tostore_amd import HipVectorBackend, HipVectorIndex, VectorIndexManager, _ffi
    import inspect

    for name in ("tsh_search_after", "tsh_search_submit_after", "tsh_search_after_stats"):
        assert name in _ffi.SIGNATURES
    assert callable(getattr(HipVectorIndex, "search_after", None)) and callable(getattr(HipVectorIndex, "search_after_stats", None))
    assert "after" in inspect.signature(HipVectorIndex.submit).parameters
    assert "after" in inspect.signature(HipVectorBackend.search).parameters
    assert "after" in inspect.signature(VectorIndexManager.vectorSearch).parameters
    with open(os.path.join(ROOT, "tostore_amd", "dart", "tostore_hip_bridge.dart")) as f:
        dart = f.read()
    for name in ("tsh_search_after", "tsh_search_submit_after", "tsh_search_after_stats"):
        assert re.search(r"'%s'" % name, dart), name
    assert re.search(r"\bsearchAfter\(", dart) and re.search(r"\bsearchAfterAsync\(", dart)
    with open(os.path.join(ROOT, "include", "tostore_hip.h")) as f:
        assert re.search(r"Additive since.*tsh_search_after, tsh_search_submit_after, tsh_search_after_stats", f.read(), flags=re.S)
