"""CPU: the attribute-column entries of the C ABI (tsh_attr_create / _set / _destroy, tsh_mask_create_range,
tsh_mask_read) exist with their ctypes prototypes, validate their arguments before any device work, and are named by the
header's additive list, the Python index and the Dart bridge with matching arity; f64_order_key orders doubles as
double.compareTo does.  (Calls that need an index run on the GPU: tests/test_gpu_mask_where.py.)"""
import ctypes
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tsh_attr_create", "tsh_attr_set", "tsh_attr_destroy", "tsh_mask_create_range", "tsh_mask_read")
ARITY = {"tsh_attr_create": 4, "tsh_attr_set": 4, "tsh_attr_destroy": 1, "tsh_mask_create_range": 8, "tsh_mask_read": 3}
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


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
    # (the attribute handle, and the address of the one to fill, travel as void *, as the header declares them)
    assert _ffi.SIGNATURES["tsh_attr_create"][1] == [_ffi.p_void, _ffi.p_i64, ctypes.c_int64, _ffi.p_void]
    assert _ffi.SIGNATURES["tsh_attr_set"][1] == [_ffi.p_void, ctypes.c_int64, ctypes.c_int64, _ffi.p_i64]
    assert _ffi.SIGNATURES["tsh_mask_create_range"][1] == [_ffi.p_void, _ffi.p_void, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                                           _ffi.p_void, ctypes.c_int32, ctypes.POINTER(_ffi.p_void)]
    assert _ffi.SIGNATURES["tsh_mask_read"] == (ctypes.c_int32, [_ffi.p_void, _ffi.p_u8, ctypes.c_int64])
    assert _ffi.TSH_ATTR_NULL == I64_MIN and (_ffi.TSH_MASK_AND, _ffi.TSH_MASK_OR) == (0, 1)


def test_argument_validation_comes_first():
    """Nothing here has an index or a device behind it: every call is refused on its arguments alone."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    fake = ctypes.c_void_p(0x10)  # never dereferenced: the checks below come before any use of a handle
    v = np.array([1, 2, I64_MIN, 4], np.int64)

    def make(idx, attr, with_, combine, out):
        return L.tsh_mask_create_range(idx, attr, 0, 9, 0, with_, combine, out)

    # tsh_mask_create_range: a NULL idx, attr or out; a combine that is neither AND nor OR, with and without `with`
    for idx, attr, with_, combine, word in ((None, fake, None, 0, "index is NULL"), (fake, None, None, 0, "attr is NULL"),
                                            (None, None, None, 1, "index is NULL"),
                                            (fake, fake, None, 2, "combine"), (fake, fake, None, -1, "combine"),
                                            (fake, fake, fake, 7, "combine"), (None, None, None, 2, "combine")):
        out = ctypes.c_void_p(0x20)
        assert make(idx, attr, with_, combine, ctypes.byref(out)) == _ffi.TSH_E_BAD_ARG, word
        assert word in _ffi.last_error(), (word, _ffi.last_error())
        assert not out.value, word  # (*out is cleared on every failure)
    assert make(fake, fake, None, 0, None) == _ffi.TSH_E_BAD_ARG and "out is NULL" in _ffi.last_error()

    # tsh_mask_read: n_bytes < 0, a NULL buffer with bytes to write, a NULL handle; the buffer is not touched
    buf = np.full(4, 0xAB, np.uint8)
    assert L.tsh_mask_read(fake, _p(buf, _ffi.p_u8), -1) == _ffi.TSH_E_BAD_ARG and "n_bytes" in _ffi.last_error()
    assert L.tsh_mask_read(fake, None, 4) == _ffi.TSH_E_BAD_ARG and "out_bits" in _ffi.last_error()
    assert L.tsh_mask_read(None, _p(buf, _ffi.p_u8), 4) == _ffi.TSH_E_BAD_ARG and "mask is NULL" in _ffi.last_error()
    assert L.tsh_mask_read(None, None, 0) == _ffi.TSH_E_BAD_ARG
    assert (buf == 0xAB).all()

    # the attribute handle's own entries
    out = ctypes.c_void_p(0x20)
    assert L.tsh_attr_create(None, None, 4, ctypes.byref(out)) == _ffi.TSH_E_BAD_ARG and not out.value
    out = ctypes.c_void_p(0x20)
    assert L.tsh_attr_create(None, _p(v, _ffi.p_i64), -1, ctypes.byref(out)) == _ffi.TSH_E_BAD_ARG and not out.value
    assert L.tsh_attr_create(None, _p(v, _ffi.p_i64), 4, None) == _ffi.TSH_E_BAD_ARG
    out = ctypes.c_void_p(0x20)
    want = _ffi.TSH_E_NO_DEVICE if L.tsh_device_count() <= 0 else _ffi.TSH_E_BAD_ARG  # (no index: no fallback either)
    assert L.tsh_attr_create(None, _p(v, _ffi.p_i64), 4, ctypes.byref(out)) == want and not out.value
    assert L.tsh_attr_set(None, 0, 4, _p(v, _ffi.p_i64)) == _ffi.TSH_E_BAD_ARG
    assert L.tsh_attr_set(fake, -1, 4, _p(v, _ffi.p_i64)) == _ffi.TSH_E_BAD_ARG
    assert L.tsh_attr_set(fake, 0, -4, _p(v, _ffi.p_i64)) == _ffi.TSH_E_BAD_ARG
    assert L.tsh_attr_set(fake, 0, 4, None) == _ffi.TSH_E_BAD_ARG
    assert L.tsh_attr_destroy(None) == _ffi.TSH_OK


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
        with a.make_attr([1, 2, 3, 4]) as aa, b.make_attr([1, 2, 3, 4]) as ab, b.make_mask(np.array([0xFF], np.uint8)) as mb:
            for attr, with_mask in ((ab, None), (aa, mb)):
                try:
                    a.make_mask_where(attr, 0, 9, with_mask=with_mask)
                    raise AssertionError("a handle of another index was accepted")
                except RuntimeError as e:
                    assert "another index" in str(e)


def test_closed_handles_raise_before_the_library_is_called():
    """A closed HipAttr, or a closed with_mask, is a ValueError: never NULL, which would read as "no handle"."""
    from tostore_amd import HipAttr, HipMask, HipVectorIndex

    idx = HipVectorIndex.__new__(HipVectorIndex)
    idx._h = ctypes.c_void_p()
    attr, mask = HipAttr.__new__(HipAttr), HipMask.__new__(HipMask)
    attr._h = mask._h = ctypes.c_void_p()  # (as close() leaves them)
    live = HipAttr.__new__(HipAttr)
    live._h = ctypes.c_void_p(0x10)
    try:
        for a, w in ((attr, None), (live, mask)):
            try:
                HipVectorIndex.make_mask_where(idx, a, 0, 1, with_mask=w)
                raise AssertionError("a closed handle was passed on")
            except ValueError as e:
                assert "closed" in str(e)
        try:
            HipVectorIndex.make_mask_where(idx, live, 0, 1, combine="xor")
            raise AssertionError("combine='xor' was accepted")
        except ValueError:
            pass
    finally:
        live._h = attr._h  # (nothing to destroy)


def test_f64_order_key_is_double_compare_to():
    from tostore_amd import ATTR_NULL, f64_order_key

    rng = np.random.default_rng(7)
    rnd = np.concatenate([rng.standard_normal(500) * 10.0 ** rng.integers(-300, 300, 500),
                          rng.integers(I64_MIN, I64_MAX, 500, dtype=np.int64).view(np.float64)])
    rnd = rnd[np.isfinite(rnd)]
    tiny = np.float64(5e-324)
    special = np.array([-np.inf, -1.7976931348623157e308, -2.2250738585072014e-308, -2.225073858507201e-308, -tiny, -0.0, 0.0, tiny,
                        2.225073858507201e-308, 2.2250738585072014e-308, 1.7976931348623157e308, np.inf])
    finite = np.unique(np.concatenate([rnd, special]))  # ascending by <, -0.0 and 0.0 folded into one
    zero = int(np.flatnonzero(finite == 0.0)[0])
    vals = np.concatenate([finite[:zero], [-0.0, 0.0], finite[zero + 1:]])  # ... and told apart again: compareTo does
    assert np.signbit(vals[zero]) and not np.signbit(vals[zero + 1])
    keys = f64_order_key(vals)
    assert keys.dtype == np.int64 and (np.diff(keys.astype(object)) > 0).all()  # strictly ascending, as the values
    # NaNs of both signs and any payload: one key, past +inf (compareTo: NaN equals NaN and follows everything)
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF],
                    np.uint64).view(np.float64)
    assert np.isnan(nans).all()
    nk = f64_order_key(nans)
    assert (nk == nk[0]).all() and nk[0] > keys[-1]
    # equal values, equal keys; the argument is not written to
    again = vals.copy()
    assert np.array_equal(f64_order_key(again), keys) and np.array_equal(again.view(np.int64), vals.view(np.int64))
    # no key is the NULL: its bit pattern would be a negative NaN's, and every NaN was made the positive quiet one
    assert ATTR_NULL == I64_MIN and not (keys == ATTR_NULL).any() and not (nk == ATTR_NULL).any()
    every = np.concatenate([vals, nans])
    order = np.argsort(f64_order_key(every), kind="stable")
    assert np.array_equal(order[:len(vals)], np.arange(len(vals)))


def test_bindings_name_the_entries():
    from tostore_amd import HipAttr, HipMask, HipVectorIndex

    assert list(inspect.signature(HipVectorIndex.make_attr).parameters) == ["self", "values"]
    assert list(inspect.signature(HipVectorIndex.make_mask_where).parameters) == ["self", "attr", "lo", "hi", "negate", "with_mask", "combine"]
    sig = inspect.signature(HipVectorIndex.make_mask_where).parameters
    assert sig["negate"].default is False and sig["with_mask"].default is None and sig["combine"].default == "and"
    assert callable(getattr(HipAttr, "set", None)) and hasattr(HipAttr, "__enter__") and hasattr(HipAttr, "close")
    assert callable(getattr(HipMask, "bits", None))
    with open(os.path.join(ROOT, "include", "tostore_hip.h")) as f:
        header = f.read()
    assert re.search(r"Additive since, same version, continued: tsh_attr_create, tsh_attr_set, tsh_attr_destroy, tsh_mask_create_range,\s*\*\s*"
                     r"tsh_mask_read\. \*/", header)
    assert re.search(r"#define TSH_ABI_VERSION 5\b", header)
    assert re.search(r"#define TSH_ATTR_NULL INT64_MIN\b", header) and re.search(r"#define TSH_MASK_AND 0\b", header)
    assert re.search(r"#define TSH_MASK_OR 1\b", header)
    with open(os.path.join(ROOT, "tostore_amd", "backend.py")) as f:
        backend = f.read()
    with open(os.path.join(ROOT, "tostore_amd", "dart", "tostore_hip_bridge.dart")) as f:
        dart = f.read()
    for name in NAMES:
        assert name in backend, name
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
    assert re.search(r"\bclass HipRowAttr\b", dart) and re.search(r"\bstatic HipRowMask\? where\(", dart) and re.search(r"\breadBits\(", dart)
    # a disposed handle is refused before the library sees it, as a disposed HipRowMask is by the searches
    assert re.search(r"createMaskWhere with a disposed HipRowAttr", dart) and re.search(r"createMaskWhere with a disposed HipRowMask", dart)
