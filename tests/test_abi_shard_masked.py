"""CPU: the sharded entries that take a mask HANDLE and an optional cursor (tsh_search_shard_masked,
tsh_search_shard_begin_masked, tsh_search_sharded_masked; include/tostore_hip.h).  Every layer carries the three names,
half a cursor is refused before anything else is looked at, and without a device they refuse to compute."""
import ctypes
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tsh_search_shard_masked", "tsh_search_shard_begin_masked", "tsh_search_sharded_masked")
DART_METHODS = ("searchShardMasked", "shardStreamBeginMasked", "searchShardedMasked")


def test_every_layer_carries_the_three_entries():
    import inspect

    from tostore_amd import _ffi, sharded

    bridge = open(os.path.join(ROOT, "tostore_amd", "dart", "tostore_hip_bridge.dart")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header = open(os.path.join(ROOT, "include", "tostore_hip.h")).read()
    src = inspect.getsource(sharded)
    for name in NAMES:
        assert name in _ffi.SIGNATURES and hasattr(_ffi.lib(), name), name
        assert name + "(" in header and "'%s'" % name in bridge and "`%s`" % name in integration, name
        assert "." + name + "(" in src, name + " is not called by sharded.py"
    since = header[header.index("Additive since"):header.index("/* status codes */")]
    for name in NAMES:
        assert name in since, name + " is not listed as additive"
    assert "#define TSH_ABI_VERSION 5" in header and _ffi.ABI_VERSION == 5
    for method in DART_METHODS:
        assert method + "(" in bridge and method in integration, method


def test_half_a_cursor_is_refused_and_no_device_is_said():
    """Exactly one NULL cursor array is TSH_E_BAD_ARG on all three, with after_dist in the text, whatever else is
    passed; a failed _begin_masked leaves *out NULL.  Both arrays or neither are valid: without a device the entries
    then answer TSH_E_NO_DEVICE."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    q = np.zeros(4, np.float32)
    qp = q.ctypes.data_as(_ffi.p_f32)
    ad, ai = np.zeros(1), np.zeros(1, np.int64)
    adp, aip = ad.ctypes.data_as(_ffi.p_f64), ai.ctypes.data_as(_ffi.p_i64)
    ids, dist, cnt = np.zeros(3, np.int64), np.zeros(3), np.zeros(1, np.int32)
    idp, dp, cp = ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64), cnt.ctypes.data_as(_ffi.p_i32)
    blk = np.zeros(64 + 24 * 8, np.uint8)
    bp = blk.ctypes.data_as(ctypes.c_void_p)
    for a, b in ((None, aip), (adp, None)):
        assert L.tsh_search_shard_masked(None, qp, 1, 3, None, a, b, 8, bp, None) == _ffi.TSH_E_BAD_ARG
        assert "after_dist" in _ffi.last_error()
        st = ctypes.c_void_p(1)
        assert L.tsh_search_shard_begin_masked(None, qp, 1, 3, None, a, b, 8, bp, 0, ctypes.byref(st)) == _ffi.TSH_E_BAD_ARG
        assert "after_dist" in _ffi.last_error()
        assert not st.value  # (a failed begin leaves no handle behind)
        assert L.tsh_search_sharded_masked(None, None, qp, 1, 3, math.nan, None, a, b, idp, dp, cp) == _ffi.TSH_E_BAD_ARG
        assert "after_dist" in _ffi.last_error()
    if L.tsh_device_count() > 0:
        return
    for a, b in ((None, None), (adp, aip)):
        assert L.tsh_search_shard_masked(None, qp, 1, 3, None, a, b, 8, bp, None) == _ffi.TSH_E_NO_DEVICE
        st = ctypes.c_void_p(1)
        assert L.tsh_search_shard_begin_masked(None, qp, 1, 3, None, a, b, 8, bp, 0, ctypes.byref(st)) == _ffi.TSH_E_NO_DEVICE
        assert not st.value
        assert L.tsh_search_sharded_masked(None, None, qp, 1, 3, math.nan, None, a, b, idp, dp, cp) == _ffi.TSH_E_NO_DEVICE
        assert "no HIP device" in _ffi.last_error()


def test_python_searchers_take_a_mask_handle():
    """ShardedSearcher and CommSearcher route a HipMask to the *_masked entries and refuse a closed one as
    HipMask.handle() does (ValueError), before any library call."""
    import inspect

    from tostore_amd import backend, sharded

    src = inspect.getsource(sharded.mask_forms)
    assert "HipMask" in src and ".handle()" in src
    for fn in (sharded.ShardedSearcher.search, sharded.ShardedSearcher.search_many, sharded.CommSearcher.search):
        assert "mask_forms(" in inspect.getsource(fn), fn

    class _Index:  # (what mask_forms asks of an index for the pointer form)
        def mask_arg(self, m):
            return m, "ptr"

    closed = backend.HipMask.__new__(backend.HipMask)
    closed._h = ctypes.c_void_p()
    with pytest.raises(ValueError):
        sharded.mask_forms(_Index(), closed)
    opened = backend.HipMask.__new__(backend.HipMask)
    opened._h = ctypes.c_void_p(16)
    assert sharded.mask_forms(_Index(), opened) == (opened, None, opened._h)
    opened._h = ctypes.c_void_p()  # (nothing for __del__ to destroy)
    arr = np.zeros(2, np.uint8)
    assert sharded.mask_forms(_Index(), arr) == (arr, "ptr", None)
    assert sharded.mask_forms(_Index(), None) == (None, "ptr", None)


def test_header_is_strict_c99(tmp_path):
    """The header with the three declarations compiles as strict C99 and a C program that names them links."""
    import shutil
    import subprocess

    from tostore_amd import build

    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    so = build.build_library()
    src = tmp_path / "abi_masked.c"
    src.write_text(
        '#include "tostore_hip.h"\n#include <stdio.h>\n'
        "int main(void) {\n  float q[4] = {0}; double ad[1] = {0}; int64_t id[1]; double d[1]; int32_t c[1];\n"
        "  char blk[64 + 24 * 8]; tsh_shard_stream *st = 0;\n"
        "  int a = tsh_search_shard_masked(0, q, 1, 1, 0, ad, 0, 8, blk, 0);\n"
        "  int b = tsh_search_shard_begin_masked(0, q, 1, 1, 0, ad, 0, 8, blk, 0, &st);\n"
        "  int e = tsh_search_sharded_masked(0, 0, q, 1, 1, 0.0, 0, ad, 0, id, d, c);\n"
        '  printf("%d %d %d %d\\n", a, b, e, st == 0);\n  return 0;\n}\n')
    exe = tmp_path / "abi_masked"
    libdir = os.path.dirname(so)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), "-L", libdir, "-ltostore_hip", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["-1", "-1", "-1", "1"]
