"""CPU: the facet entries of the C ABI (tsh_attr_facets, tsh_tags_facets; include/tostore_hip.h) exist with ctypes
prototypes equal to the header's parameter lists; the constants agree in the header, Python, Dart and the host plan; a
strict C99 file that calls both entries compiles against the header; every argument the header lists as TSH_E_BAD_ARG and
that needs no index is refused on the arguments alone, with the outputs untouched and no handle dereferenced; closed
Python handles raise before the library is called; the bindings and documents name the entries.
(Calls that need an index run on the GPU: tests/test_gpu_facets.py.)"""
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
    "tsh_attr_facets": ["tsh_index *idx", "void *attr", "tsh_mask *mask", "int32_t kind", "const int64_t *keys", "int64_t n_keys",
                        "int64_t *out_counts", "int64_t *out_rest"],
    "tsh_tags_facets": ["tsh_index *idx", "void *tags", "tsh_mask *mask", "const int64_t *keys", "int64_t n_keys", "int64_t *out_counts",
                        "int64_t *out_rest"],
}
CONSTANTS = {"TSH_FACET_VALUES": 0, "TSH_FACET_EDGES": 1, "TSH_FACET_MAX_KEYS": 4096}
DART_CONSTANTS = {"facetValues": "TSH_FACET_VALUES", "facetEdges": "TSH_FACET_EDGES", "facetMaxKeys": "TSH_FACET_MAX_KEYS"}
PLAN_CONSTANTS = {"FACET_VALUES": "TSH_FACET_VALUES", "FACET_EDGES": "TSH_FACET_EDGES", "FACET_MAX_KEYS": "TSH_FACET_MAX_KEYS"}


def _strip(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_symbols_and_prototypes():
    from tostore_amd import _ffi

    L = _ffi.lib()
    header = _strip(open(HEADER).read())
    c2ctypes = {"tsh_index *": _ffi.p_void, "void *": _ffi.p_void, "tsh_mask *": _ffi.p_void, "const int64_t *": _ffi.p_i64,
                "int64_t *": _ffi.p_i64, "int64_t ": ctypes.c_int64, "int32_t ": ctypes.c_int32}
    for name, params in PARAMS.items():
        fn = getattr(L, name)  # the shared library exports it
        restype, argtypes = _ffi.SIGNATURES[name]
        assert fn.restype is restype is ctypes.c_int32 and list(fn.argtypes) == list(argtypes)
        m = re.search(r"\bint32_t\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name
        got = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert got == params, name
        assert list(argtypes) == [c2ctypes[re.match(r"(.*?)\w+$", p).group(1)] for p in params], name


def test_constants_agree():
    from tostore_amd import _ffi

    header, dart = open(HEADER).read(), open(BRIDGE).read()
    plan = open(os.path.join(ROOT, "tostore_amd", "csrc", "tsh_facet_plan.h")).read()
    for name, val in CONSTANTS.items():
        m = re.search(r"^#define %s\s+(\d+)\b" % name, header, re.M)
        assert m and int(m.group(1)) == val, name
        assert getattr(_ffi, name) == val, name
    for dname, cname in DART_CONSTANTS.items():
        m = re.search(r"static const int %s = (\d+);" % dname, dart)
        assert m and int(m.group(1)) == CONSTANTS[cname], dname
    for pname, cname in PLAN_CONSTANTS.items():
        m = re.search(r"constexpr int(?:32_t)? %s = (\d+);" % pname, plan)
        assert m and int(m.group(1)) == CONSTANTS[cname], pname
    assert re.search(r"constexpr int64_t FACET_NULL = INT64_MIN;", plan) and _ffi.TSH_ATTR_NULL == I64_MIN
    assert re.search(r"#define TSH_ABI_VERSION 5\b", header) and _ffi.ABI_VERSION == 5
    # what 48 KB of LDS hold: the keys and a 32-bit counter each, as the set of a tag or IN term is what 32 KB hold
    assert _ffi.TSH_FACET_MAX_KEYS == _ffi.TSH_TAGS_MAX_SET_VALUES == _ffi.TSH_WHERE_MAX_SET_VALUES


def test_a_c99_caller_compiles(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "caller.c"
    src.write_text('''#include "tostore_hip.h"
#include <stddef.h>
int use(tsh_index *idx, tsh_attr *attr, tsh_tags *tags, tsh_mask *mask) {
  const int64_t keys[3] = {7, TSH_ATTR_NULL, 7}, edges[2] = {0, 10};
  int64_t counts[3], rest[3];
  int32_t rc = tsh_attr_facets(idx, attr, mask, TSH_FACET_VALUES, keys, 3, counts, rest);
  if (rc == TSH_OK) rc = tsh_attr_facets(idx, attr, NULL, TSH_FACET_EDGES, edges, 2, counts, rest);
  if (rc == TSH_OK) rc = tsh_attr_facets(idx, attr, NULL, TSH_FACET_VALUES, NULL, 0, NULL, rest);
  if (rc == TSH_OK) rc = tsh_tags_facets(idx, tags, mask, keys, 3, counts, rest);
  if (rc == TSH_OK) rc = tsh_tags_facets(idx, tags, NULL, NULL, 0, NULL, rest);
  return rc + (int)(sizeof(int[TSH_FACET_MAX_KEYS == 4096 ? 1 : -1]) - sizeof(int));
}
''')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "caller.o")], check=True)


def test_argument_validation_comes_first():
    """Nothing here has an index or a device behind it: every call is refused on its arguments alone, no handle is
    dereferenced (the fake ones would fault) and neither output array is written."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    fake = ctypes.c_void_p(0x10)
    vals = np.arange(5000, dtype=np.int64)
    pv = vals.ctypes.data_as(_ffi.p_i64)
    SENT = -77

    def arr(*a):
        a = np.array(a, np.int64)
        return a, a.ctypes.data_as(_ffi.p_i64)

    def call(entry, idx=fake, col=fake, mask=None, kind=0, keys=pv, n_keys=3, counts=True, rest=True):
        oc, orr = np.full(5000, SENT, np.int64), np.full(3, SENT, np.int64)
        pc = oc.ctypes.data_as(_ffi.p_i64) if counts else None
        pr = orr.ctypes.data_as(_ffi.p_i64) if rest else None
        if entry == "attr":
            rc = L.tsh_attr_facets(idx, col, mask, kind, keys, n_keys, pc, pr)
        else:
            rc = L.tsh_tags_facets(idx, col, mask, keys, n_keys, pc, pr)
        assert (oc == SENT).all() and (orr == SENT).all(), "an output was written"
        return rc, _ffi.last_error()

    # 4096 distinct values, a NULL and duplicates: within the limit ...
    nulls = np.concatenate([vals[:4096], [I64_MIN, 17, 17]])
    both = [
        ("index is NULL", dict(idx=None)),
        ("is NULL", dict(col=None)),
        ("out_rest is NULL", dict(rest=False)),
        ("out_rest is NULL", dict(rest=False, idx=None, col=None)),
        ("n_keys < 0", dict(n_keys=-1)),
        ("keys is NULL", dict(keys=None, n_keys=2)),
        ("out_counts is NULL", dict(counts=False)),
        ("TSH_FACET_MAX_KEYS", dict(n_keys=4097)),
        ("TSH_FACET_MAX_KEYS", dict(n_keys=5000)),
    ]
    for entry in ("attr", "tags"):
        for word, kw in both:
            rc, err = call(entry, **kw)
            assert rc == _ffi.TSH_E_BAD_ARG, (entry, word, rc)
            assert word in err, (entry, word, err)
        # ... so the limit is not what refuses this one: with no index it gets as far as "index is NULL"
        rc, err = call(entry, idx=None, keys=nulls.ctypes.data_as(_ffi.p_i64), n_keys=len(nulls))
        assert rc == _ffi.TSH_E_BAD_ARG and "index is NULL" in err
    assert "attr is NULL" in call("attr", col=None)[1] and "tags is NULL" in call("tags", col=None)[1]
    # the attribute entry's kind and its edge rules
    for kind in (2, -1, 1 << 30):
        rc, err = call("attr", kind=kind)
        assert rc == _ffi.TSH_E_BAD_ARG and "kind" in err, kind
    edge_errors = [
        ("ascend", arr(1, 1)), ("ascend", arr(2, 1)), ("ascend", arr(0, 5, 5, 9)), ("ascend", arr(3, I64_MIN)),
        ("TSH_ATTR_NULL", arr(I64_MIN, 4)), ("TSH_ATTR_NULL", arr(I64_MIN)),
    ]
    for word, (a, pa) in edge_errors:
        rc, err = call("attr", kind=_ffi.TSH_FACET_EDGES, keys=pa, n_keys=len(a))
        assert rc == _ffi.TSH_E_BAD_ARG and word in err, (word, err)
    rc, err = call("attr", kind=_ffi.TSH_FACET_EDGES, n_keys=4097)  # (ascending, but too many)
    assert rc == _ffi.TSH_E_BAD_ARG and "TSH_FACET_MAX_KEYS" in err
    # the same unsorted keys are fine as VALUES: without an index they get as far as "index is NULL"
    a, pa = arr(2, 1, 1, I64_MIN)
    rc, err = call("attr", idx=None, keys=pa, n_keys=4)
    assert rc == _ffi.TSH_E_BAD_ARG and "index is NULL" in err
    # n_keys == 0 needs neither array
    rc, err = call("attr", idx=None, keys=None, n_keys=0, counts=False)
    assert rc == _ffi.TSH_E_BAD_ARG and "index is NULL" in err


def test_closed_handles_raise_before_the_library_is_called():
    """A closed HipAttr / HipTags, or a closed row_mask, is a ValueError: never NULL, which would read as "no filter"."""
    from tostore_amd import HipAttr, HipMask, HipTags, HipVectorIndex

    idx = HipVectorIndex.__new__(HipVectorIndex)
    idx._h = ctypes.c_void_p()
    mask = HipMask.__new__(HipMask)
    mask._h = ctypes.c_void_p()  # (as close() leaves it)
    made = [mask]
    try:
        for cls in (HipAttr, HipTags):
            closed, live = cls.__new__(cls), cls.__new__(cls)
            closed._h, live._h = ctypes.c_void_p(), ctypes.c_void_p(0x10)
            made += [closed, live]
            with pytest.raises(ValueError, match="closed"):
                HipVectorIndex.facets(idx, closed, [1, 2])
            with pytest.raises(ValueError, match="closed"):
                HipVectorIndex.facets(idx, live, [1, 2], row_mask=mask)
            with pytest.raises(ValueError):
                HipVectorIndex.facets(idx, live, [1, 2], kind="ranges")
            with pytest.raises(TypeError):
                HipVectorIndex.facets(idx, live, [1, 2], row_mask=np.ones(4, np.uint8))
        with pytest.raises(ValueError):
            HipVectorIndex.facets(idx, made[-1], [1, 2], kind="edges")  # (a tag column counts by value)
        with pytest.raises(TypeError):
            HipVectorIndex.facets(idx, mask, [1, 2])
    finally:
        for h in made:
            h._h = ctypes.c_void_p()  # (nothing to destroy)


def test_bindings_and_documents_name_the_entries():
    from tostore_amd import HipVectorIndex

    sig = inspect.signature(HipVectorIndex.facets).parameters
    assert list(sig) == ["self", "column", "keys", "row_mask", "kind"]
    assert sig["row_mask"].default is None and sig["kind"].default == "values"
    header, dart = open(HEADER).read(), open(BRIDGE).read()
    backend = open(os.path.join(ROOT, "tostore_amd", "backend.py")).read()
    assert re.search(r"Additive since, same version, continued: tsh_attr_facets, tsh_tags_facets\b", header)
    arity = {"tsh_attr_facets": 8, "tsh_tags_facets": 7}
    for name, n_args in arity.items():
        assert name in backend, name
        m = re.search(r"lookupFunction<(\w+), (\w+)>\('%s'\)" % name, dart)
        assert m, name
        for td in m.groups():
            t = re.search(r"typedef %s = \w+ Function\(([^;]*)\);" % td, dart)
            assert t and len(re.sub(r"<[^<>]*(<[^<>]*>)?[^<>]*>", "", t.group(1)).split(",")) == n_args, td
    assert re.search(r"\bfinal class HipFacetCounts\b", dart)
    # both classes have the method, and a disposed column or mask is refused before the library sees it
    for cls, field, word in (("HipRowAttr", "_attr", "facets with a disposed HipRowAttr"), ("HipTagColumn", "_tags", "facets with a disposed HipTagColumn")):
        body = dart[dart.index("final class %s " % cls):]
        body = body[:body.index("\n}\n")]
        m = re.search(r"HipFacetCounts\? facets\(HipVectorBackend backend, Int64List keys, \{[^}]*\}\) \{(.*?)\n  \}", body, flags=re.S)
        assert m, cls
        assert re.search(r"if \(%s == nullptr\) \{\s*Logger\.warn\('%s'[^;]*;\s*return null;" % (field, word), m.group(1)), cls
        assert re.search(r"if \(mask != null && mask\._mask == nullptr\) \{\s*Logger\.warn\('facets with a disposed HipRowMask'[^;]*;\s*return null;",
                         m.group(1)), cls
    for doc, word in (("DESIGN.md", "## Addendum: facet counts"), ("INTEGRATION.md", "tsh_attr_facets"), ("INTEGRATION.md", "tsh_tags_facets"),
                      ("README.md", "facet counts")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)
    build = open(os.path.join(ROOT, "tostore_amd", "build.py")).read()
    assert '"tsh_facet.hip.h"' in build and '"tsh_facet_plan.h"' in build
