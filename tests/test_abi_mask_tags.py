"""CPU: the tag-column entries of the C ABI (tsh_tags_create / _set / _destroy, tsh_mask_create_tags; include/tostore_hip.h)
exist with ctypes prototypes equal to the header's parameter lists; the constants agree in the header, Python and Dart; a
strict C99 file that calls the four entries compiles against the header; every argument the header lists as TSH_E_BAD_ARG
and that needs no index is refused on the arguments alone, with *out cleared and no handle dereferenced; closed Python
handles raise before the library is called; the bindings and documents name the entries.
(Calls that need an index run on the GPU: tests/test_gpu_mask_tags.py.)"""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tostore_hip.h")
BRIDGE = os.path.join(ROOT, "tostore_amd", "dart", "tostore_hip_bridge.dart")
I64_MIN = -(1 << 63)
PARAMS = {
    "tsh_tags_create": ["tsh_index *idx", "const int64_t *offsets", "int64_t n", "const int64_t *values", "void *out"],
    "tsh_tags_set": ["void *tags", "int64_t first_row_id", "int64_t n", "const int64_t *offsets", "const int64_t *values"],
    "tsh_tags_destroy": ["void *tags"],
    "tsh_mask_create_tags": ["tsh_index *idx", "void *tags", "const int64_t *set", "int64_t n_set", "int32_t need", "int32_t negate",
                             "tsh_mask *with", "int32_t combine", "tsh_mask **out"],
}
CONSTANTS = {"TSH_TAGS_ALL": 0, "TSH_TAGS_ANY": 1, "TSH_TAGS_MAX_SET_VALUES": 4096}
DART_CONSTANTS = {"tagsAll": "TSH_TAGS_ALL", "tagsAny": "TSH_TAGS_ANY", "tagsMaxSetValues": "TSH_TAGS_MAX_SET_VALUES"}


def _strip(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_symbols_and_prototypes():
    from tostore_amd import _ffi

    L = _ffi.lib()
    header = _strip(open(HEADER).read())
    c2ctypes = {"tsh_index *": _ffi.p_void, "void *": _ffi.p_void, "tsh_mask *": _ffi.p_void, "tsh_mask **": ctypes.POINTER(_ffi.p_void),
                "const int64_t *": _ffi.p_i64, "int64_t ": ctypes.c_int64, "int32_t ": ctypes.c_int32}
    for name, params in PARAMS.items():
        fn = getattr(L, name)  # the shared library exports it
        restype, argtypes = _ffi.SIGNATURES[name]
        assert fn.restype is restype is ctypes.c_int32 and list(fn.argtypes) == list(argtypes)
        m = re.search(r"\bint32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        got = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert got == params, name
        assert list(argtypes) == [c2ctypes[re.match(r"(.*?)\w+$", p).group(1)] for p in params], name
    assert re.search(r"\btypedef struct tsh_tags tsh_tags;", header)


def test_constants_agree():
    from tostore_amd import _ffi

    header, dart = open(HEADER).read(), open(BRIDGE).read()
    for name, val in CONSTANTS.items():
        m = re.search(r"^#define %s (\d+)\b" % name, header, re.M)
        assert m and int(m.group(1)) == val, name
        assert getattr(_ffi, name) == val, name
    for dname, cname in DART_CONSTANTS.items():
        m = re.search(r"static const int %s = (\d+);" % dname, dart)
        assert m and int(m.group(1)) == CONSTANTS[cname], dname
    assert re.search(r"#define TSH_ABI_VERSION 5\b", header) and _ffi.ABI_VERSION == 5
    assert _ffi.TSH_TAGS_MAX_SET_VALUES == _ffi.TSH_WHERE_MAX_SET_VALUES  # (both are what 32 KB of LDS hold)
    plan = open(os.path.join(ROOT, "tostore_amd", "csrc", "tsh_tags_plan.h")).read()
    assert re.search(r"constexpr int TAGS_MAX_SET_VALUES = 4096;", plan) and re.search(r"constexpr int32_t TAGS_NEED_ALL = 0;", plan)


def test_a_c99_caller_compiles(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "caller.c"
    src.write_text('''#include "tostore_hip.h"
#include <stddef.h>
int use(tsh_index *idx, tsh_mask *with) {
  const int64_t offsets[3] = {0, 2, 3}, values[3] = {5, 7, TSH_ATTR_NULL}, set[2] = {7, 9};
  tsh_tags *tags = NULL;
  tsh_mask *mask = NULL;
  int32_t rc = tsh_tags_create(idx, offsets, 2, values, &tags);
  if (rc != TSH_OK) return rc;
  rc = tsh_tags_set(tags, 2, 2, offsets, values);
  if (rc == TSH_OK) rc = tsh_mask_create_tags(idx, tags, set, 2, TSH_TAGS_ANY, 0, with, TSH_MASK_AND, &mask);
  if (rc == TSH_OK) rc = tsh_mask_create_tags(idx, tags, set, 2, TSH_TAGS_ALL, 1, NULL, TSH_MASK_OR, &mask);
  if (rc == TSH_OK) rc = tsh_mask_create_tags(idx, tags, NULL, 0, 3, 0, NULL, TSH_MASK_AND, &mask);
  tsh_mask_destroy(mask);
  tsh_tags_destroy(tags);
  return rc + (int)(sizeof(int[TSH_TAGS_MAX_SET_VALUES == 4096 ? 1 : -1]) - sizeof(int));
}
''')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "caller.o")], check=True)


def test_argument_validation_comes_first():
    """Nothing here has an index or a device behind it: every call is refused on its arguments alone, and no handle is
    dereferenced (the fake ones would fault)."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    fake = ctypes.c_void_p(0x10)
    vals = np.arange(5000, dtype=np.int64)
    pv = vals.ctypes.data_as(_ffi.p_i64)

    def offsets(*o):
        a = np.array(o, np.int64)
        return a, a.ctypes.data_as(_ffi.p_i64)

    _, ok = offsets(0, 2, 4)
    csr_errors = [
        ("n < 0", dict(n=-1)),
        ("offsets is NULL", dict(off=None)),
        ("offsets[0]", dict(off=offsets(1, 2, 4)[1])),
        ("never decrease", dict(off=offsets(0, 3, 2)[1])),
        ("never decrease", dict(off=offsets(0, -1, 4)[1])),
        ("values is NULL", dict(values=None)),
    ]
    # tsh_tags_create: the CSR is judged before the index is looked at (a fake one, or none)
    for word, kw in csr_errors:
        for idx in (fake, None):
            out = ctypes.c_void_p(0x20)
            rc = L.tsh_tags_create(idx, kw.get("off", ok), kw.get("n", 2), kw.get("values", pv), ctypes.byref(out))
            assert rc == _ffi.TSH_E_BAD_ARG and word in _ffi.last_error() and not out.value, word
    assert L.tsh_tags_create(fake, ok, 2, pv, None) == _ffi.TSH_E_BAD_ARG and "out is NULL" in _ffi.last_error()
    out = ctypes.c_void_p(0x20)
    want = _ffi.TSH_E_NO_DEVICE if L.tsh_device_count() <= 0 else _ffi.TSH_E_BAD_ARG  # (no index: as tsh_attr_create answers)
    assert L.tsh_tags_create(None, ok, 2, pv, ctypes.byref(out)) == want and not out.value
    # tsh_tags_set: the same, before the handle is looked at
    for word, kw in csr_errors:
        rc = L.tsh_tags_set(fake, 0, kw.get("n", 2), kw.get("off", ok), kw.get("values", pv))
        assert rc == _ffi.TSH_E_BAD_ARG and word in _ffi.last_error(), word
    assert L.tsh_tags_set(None, 0, 2, ok, pv) == _ffi.TSH_E_BAD_ARG and "tags is NULL" in _ffi.last_error()
    assert L.tsh_tags_set(fake, -1, 2, ok, pv) == _ffi.TSH_E_BAD_ARG and "first_row_id" in _ffi.last_error()
    assert L.tsh_tags_destroy(None) == _ffi.TSH_OK

    def make(idx=fake, tags=fake, set_=pv, n_set=3, need=1, negate=0, with_=None, combine=0, null_out=False):
        out = ctypes.c_void_p(0x20)
        rc = L.tsh_mask_create_tags(idx, tags, set_, n_set, need, negate, with_, combine, None if null_out else ctypes.byref(out))
        return rc, out.value, _ffi.last_error()

    nulls = np.concatenate([vals[:4096], [I64_MIN, 17, 17]])  # 4096 distinct values, a NULL and duplicates: within the limit ...
    cases = [
        ("index is NULL", dict(idx=None)),
        ("tags is NULL", dict(tags=None)),
        ("need < 0", dict(need=-1)),
        ("need < 0", dict(need=-(1 << 31))),
        ("n_set < 0", dict(n_set=-1)),
        ("set is NULL", dict(set_=None, n_set=2)),
        ("TSH_TAGS_MAX_SET_VALUES", dict(n_set=4097)),
        ("TSH_TAGS_MAX_SET_VALUES", dict(n_set=5000, need=0)),
        ("combine", dict(combine=2)),
        ("combine", dict(combine=-1)),
        ("combine", dict(combine=7, with_=fake)),
        ("combine", dict(idx=None, combine=2)),
    ]
    for word, kw in cases:
        rc, out, err = make(**kw)
        assert rc == _ffi.TSH_E_BAD_ARG, (word, rc)
        assert word in err, (word, err)
        assert not out, word  # (*out is cleared on every failure)
    rc, _, err = make(null_out=True)
    assert rc == _ffi.TSH_E_BAD_ARG and "out is NULL" in err
    # ... so the limit is not what refuses this one: with no index it gets as far as "index is NULL"
    rc, out, err = make(idx=None, set_=nulls.ctypes.data_as(_ffi.p_i64), n_set=len(nulls))
    assert rc == _ffi.TSH_E_BAD_ARG and "index is NULL" in err and not out


def test_closed_handles_raise_before_the_library_is_called():
    """A closed HipTags, or a closed with_mask, is a ValueError: never NULL, which would read as "no handle"."""
    from tostore_amd import HipMask, HipTags, HipVectorIndex

    idx = HipVectorIndex.__new__(HipVectorIndex)
    idx._h = ctypes.c_void_p()
    closed, mask = HipTags.__new__(HipTags), HipMask.__new__(HipMask)
    closed._h = mask._h = ctypes.c_void_p()  # (as close() leaves them)
    live = HipTags.__new__(HipTags)
    live._h = ctypes.c_void_p(0x10)
    try:
        with pytest.raises(ValueError, match="closed"):
            HipVectorIndex.make_mask_tags(idx, closed, [1, 2])
        with pytest.raises(ValueError, match="closed"):
            HipVectorIndex.make_mask_tags(idx, live, [1, 2], "all", True, with_mask=mask)
        with pytest.raises(ValueError, match="closed"):
            closed.set(0, [[1], [2, 3]])
        with pytest.raises(ValueError):
            HipVectorIndex.make_mask_tags(idx, live, [1], combine="xor")
        for need in ("some", 0, -1, 1.5, True):
            with pytest.raises(ValueError):
                HipVectorIndex.make_mask_tags(idx, live, [1], need=need)
    finally:
        live._h = closed._h  # (nothing to destroy)


def test_csr_of_lists_and_pairs():
    from tostore_amd.backend import _tags_csr

    off, vals = _tags_csr([[3, 1], (), np.array([7]), range(2)])
    assert off.dtype == vals.dtype == np.int64 and off.tolist() == [0, 2, 2, 3, 5] and vals.tolist() == [3, 1, 7, 0, 1]
    off, vals = _tags_csr([])
    assert off.tolist() == [0] and vals.shape == (0,)
    off, vals = _tags_csr(([0, 1, 3], np.array([9, 8, 7], np.int32)))
    assert off.dtype == vals.dtype == np.int64 and off.tolist() == [0, 1, 3] and vals.tolist() == [9, 8, 7]


def test_bindings_and_documents_name_the_entries():
    from tostore_amd import HipTags, HipVectorIndex

    sig = inspect.signature(HipVectorIndex.make_mask_tags).parameters
    assert list(sig) == ["self", "tags", "values", "need", "negate", "with_mask", "combine"]
    assert sig["need"].default == "any" and sig["negate"].default is False and sig["with_mask"].default is None and sig["combine"].default == "and"
    assert list(inspect.signature(HipVectorIndex.make_tags).parameters) == ["self", "lists"]
    for member in ("close", "set", "handle", "__enter__", "__exit__"):
        assert callable(getattr(HipTags, member)), member
    header, dart = open(HEADER).read(), open(BRIDGE).read()
    backend = open(os.path.join(ROOT, "tostore_amd", "backend.py")).read()
    assert re.search(r"Additive since, same version, continued: tsh_tags_create, tsh_tags_set, tsh_tags_destroy, tsh_mask_create_tags\b", header)
    arity = {"tsh_tags_create": 5, "tsh_tags_set": 5, "tsh_tags_destroy": 1, "tsh_mask_create_tags": 9}
    for name, n_args in arity.items():
        assert name in backend, name
        m = re.search(r"lookupFunction<(\w+), (\w+)>\('%s'\)" % name, dart)
        assert m, name
        for td in m.groups():
            t = re.search(r"typedef %s = \w+ Function\(([^;]*)\);" % td, dart)
            assert t and len(re.sub(r"<[^<>]*(<[^<>]*>)?[^<>]*>", "", t.group(1)).split(",")) == n_args, td
    assert re.search(r"\bfinal class HipTagColumn\b", dart) and re.search(r"\bstatic HipRowMask\? hasTags\(", dart)
    # a disposed handle is refused before the library sees it
    assert "createMaskTags with a disposed HipTagColumn" in dart and "createMaskTags with a disposed HipRowMask" in dart
    assert re.search(r"bool set\(int firstNodeId, List<List<int>> lists\) \{\s*if \(_tags == nullptr\) return false;", dart)
    # the header's "Not here" list of the attribute columns no longer names what these entries do
    assert "string or multi-valued attributes" not in header
    for doc, word in (("DESIGN.md", "## Addendum: tag columns"), ("INTEGRATION.md", "tsh_mask_create_tags"), ("README.md", "tag column")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
    build = open(os.path.join(ROOT, "tostore_amd", "build.py")).read()
    assert '"tsh_tags.hip.h"' in build and '"tsh_tags_plan.h"' in build
