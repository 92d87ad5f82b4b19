"""CPU: the whole-clause entry of the C ABI (tsh_mask_create_where, tsh_where_term; include/tostore_hip.h) exists with
its ctypes prototype; the ctypes and Dart mirrors of the term record lay it out as a C99 compile of the header does; the
constants agree in the header, Python and Dart; every argument the header lists as TSH_E_BAD_ARG is refused before any
device work, with *out cleared; closed Python handles raise before the library is called; the bindings name the entry.
(Calls that need an index run on the GPU: tests/test_gpu_mask_where_terms.py.)"""
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
FIELDS = ("attr", "lo", "hi", "set", "n_set", "kind", "negate", "clause", "reserved")
CONSTANTS = {"TSH_TERM_RANGE": 0, "TSH_TERM_IN": 1, "TSH_WHERE_MAX_TERMS": 32, "TSH_WHERE_MAX_COLUMNS": 8,
             "TSH_WHERE_MAX_SET_VALUES": 4096}
DART_CONSTANTS = {"termRange": "TSH_TERM_RANGE", "termIn": "TSH_TERM_IN", "whereMaxTerms": "TSH_WHERE_MAX_TERMS",
                  "whereMaxColumns": "TSH_WHERE_MAX_COLUMNS", "whereMaxSetValues": "TSH_WHERE_MAX_SET_VALUES"}


def _strip(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_symbol_and_prototype():
    from tostore_amd import _ffi

    L = _ffi.lib()
    fn = L.tsh_mask_create_where  # the shared library exports it
    restype, argtypes = _ffi.SIGNATURES["tsh_mask_create_where"]
    assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert (restype, argtypes) == (ctypes.c_int32, [_ffi.p_void, _ffi.p_void, ctypes.c_int32, _ffi.p_void, ctypes.c_int32,
                                                    ctypes.POINTER(_ffi.p_void)])
    m = re.search(r"\bint32_t\s+tsh_mask_create_where\s*\(([^)]*)\)\s*;", _strip(open(HEADER).read()))
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["tsh_index *idx", "const void *terms", "int32_t n_terms", "tsh_mask *with", "int32_t combine", "tsh_mask **out"]


def test_term_record_layout_is_the_c_compilers(tmp_path):
    from tostore_amd import _ffi

    T = _ffi.TshWhereTerm
    assert tuple(f for f, _ in T._fields_) == FIELDS
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    src.write_text('#include "tostore_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n'
                   '  printf("%d", (int)sizeof(tsh_where_term));\n'
                   + "".join('  printf(" %%d %%d", (int)offsetof(tsh_where_term, %s), (int)sizeof(((tsh_where_term *)0)->%s));\n' % (f, f)
                             for f in FIELDS)
                   + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert nums[0] == ctypes.sizeof(T) == 56
    for i, f in enumerate(FIELDS):
        assert (nums[1 + 2 * i], nums[2 + 2 * i]) == (getattr(T, f).offset, getattr(T, f).size), f
    # the Dart struct: the same fields in the same order with the same widths
    body = re.search(r"final\s+class\s+TshWhereTerm\s+extends\s+Struct\s*\{(.*?)\n\}", _strip(open(BRIDGE).read()), flags=re.S).group(1)
    dart = re.findall(r"(?:@(\w+)\(\)\s*)?external\s+([\w<>]+)\s+(\w+)\s*;", body)
    snake = lambda s: re.sub(r"([A-Z])", lambda m: "_" + m.group(1).lower(), s)  # noqa: E731
    assert [snake(name) for _, _, name in dart] == list(FIELDS)
    width = {"Int32": 4, "Int64": 8}
    for (ann, dtype, name), f in zip(dart, FIELDS):
        if dtype.startswith("Pointer<"):
            assert not ann and getattr(T, f).size == ctypes.sizeof(ctypes.c_void_p), name
            assert dtype == {"attr": "Pointer<Void>", "set": "Pointer<Int64>"}[f]
        else:
            assert dtype == "int" and width[ann] == getattr(T, f).size, name


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


def test_argument_validation_comes_first():
    """Nothing here has an index or a device behind it: every call is refused on its arguments alone, and no handle is
    dereferenced (the fake ones would fault)."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    fake = ctypes.c_void_p(0x10)
    vals = np.arange(5000, dtype=np.int64)
    pv = vals.ctypes.data_as(_ffi.p_i64)

    def term(attr=0x10, lo=0, hi=9, set_=None, n_set=0, kind=0, negate=0, clause=0, reserved=0):
        return (attr, lo, hi, set_, n_set, kind, negate, clause, reserved)

    def call(terms, idx=fake, with_=None, combine=0, n_terms=None, null_terms=False, null_out=False):
        arr = (_ffi.TshWhereTerm * max(len(terms), 1))()
        for rec, t in zip(arr, terms):
            rec.attr, rec.lo, rec.hi, rec.set, rec.n_set, rec.kind, rec.negate, rec.clause, rec.reserved = t
        out = ctypes.c_void_p(0x20)
        rc = L.tsh_mask_create_where(idx, None if null_terms else ctypes.cast(arr, _ffi.p_void),
                                     len(terms) if n_terms is None else n_terms, with_, combine,
                                     None if null_out else ctypes.byref(out))
        return rc, out.value, _ffi.last_error()

    one = [term()]
    cases = [
        ("index is NULL", dict(terms=one, idx=None)),
        ("terms is NULL", dict(terms=one, null_terms=True)),
        ("n_terms", dict(terms=one, n_terms=0)),
        ("n_terms", dict(terms=one, n_terms=-3)),
        ("n_terms", dict(terms=[term()] * 33)),
        ("attr is NULL", dict(terms=[term(attr=None)])),
        ("attr is NULL", dict(terms=[term(), term(attr=None, kind=1)])),
        ("combine", dict(terms=one, combine=2)),
        ("combine", dict(terms=one, combine=-1)),
        ("combine", dict(terms=one, combine=7, with_=fake)),
        ("combine", dict(terms=one, idx=None, combine=2)),
        ("kind", dict(terms=[term(kind=2)])),
        ("kind", dict(terms=[term(), term(kind=-1)])),
        ("reserved", dict(terms=[term(reserved=1)])),
        ("reserved", dict(terms=[term(), term(), term(reserved=-1)])),
        ("n_set < 0", dict(terms=[term(kind=1, set_=pv, n_set=-1)])),
        ("set is NULL", dict(terms=[term(kind=1, set_=None, n_set=3)])),
        ("TSH_WHERE_MAX_COLUMNS", dict(terms=[term(attr=0x10 * (i + 1), clause=i) for i in range(9)])),
        ("TSH_WHERE_MAX_SET_VALUES", dict(terms=[term(kind=1, set_=pv, n_set=4097)])),
        ("TSH_WHERE_MAX_SET_VALUES", dict(terms=[term(kind=1, set_=pv, n_set=4096), term(kind=1, set_=pv, n_set=1, clause=1)])),
        ("clause", dict(terms=[term(), term(), term(clause=2)])),
        ("clause", dict(terms=[term(clause=1)])),
        ("clause", dict(terms=[term(), term(clause=1), term(clause=0)])),
    ]
    for word, kw in cases:
        rc, out, err = call(**kw)
        assert rc == _ffi.TSH_E_BAD_ARG, (word, rc)
        assert word in err, (word, err)
        assert not out, word  # (*out is cleared on every failure)
    rc, _, err = call(one, null_out=True)
    assert rc == _ffi.TSH_E_BAD_ARG and "out is NULL" in err


def test_closed_handles_raise_before_the_library_is_called():
    """A closed HipAttr in any term, or a closed with_mask, is a ValueError: never NULL, which would read as "no handle"."""
    from tostore_amd import HipAttr, HipMask, HipVectorIndex, WhereIn, WhereRange

    idx = HipVectorIndex.__new__(HipVectorIndex)
    idx._h = ctypes.c_void_p()
    closed, mask = HipAttr.__new__(HipAttr), HipMask.__new__(HipMask)
    closed._h = mask._h = ctypes.c_void_p()  # (as close() leaves them)
    live = HipAttr.__new__(HipAttr)
    live._h = ctypes.c_void_p(0x10)
    try:
        for clauses, w in (([[WhereRange(closed, 0, 1)]], None), ([[WhereRange(live, 0, 1)], [WhereIn(closed, [1, 2], negate=True)]], None),
                           ([[WhereRange(live, 0, 1), WhereIn(live, [])]], mask)):
            with pytest.raises(ValueError, match="closed"):
                HipVectorIndex.make_mask_clauses(idx, clauses, with_mask=w)
        with pytest.raises(ValueError):
            HipVectorIndex.make_mask_clauses(idx, [[WhereRange(live, 0, 1)]], combine="xor")
        with pytest.raises(ValueError):
            HipVectorIndex.make_mask_clauses(idx, [[WhereRange(live, 0, 1)], []])
        with pytest.raises(TypeError):
            HipVectorIndex.make_mask_clauses(idx, [[(live, 0, 1)]])
    finally:
        live._h = closed._h  # (nothing to destroy)


def test_bindings_name_the_entry():
    from tostore_amd import HipVectorIndex, WhereIn, WhereRange

    sig = inspect.signature(HipVectorIndex.make_mask_clauses).parameters
    assert list(sig) == ["self", "clauses", "with_mask", "combine"]
    assert sig["with_mask"].default is None and sig["combine"].default == "and"
    assert list(inspect.signature(WhereRange).parameters) == ["attr", "lo", "hi", "negate"]
    assert list(inspect.signature(WhereIn).parameters) == ["attr", "values", "negate"]
    assert inspect.signature(WhereRange).parameters["negate"].default is False
    assert inspect.signature(WhereIn).parameters["negate"].default is False
    header, dart = open(HEADER).read(), open(BRIDGE).read()
    backend = open(os.path.join(ROOT, "tostore_amd", "backend.py")).read()
    assert re.search(r"Additive since, same version, continued: tsh_mask_create_where\b", header)
    assert "tsh_mask_create_where" in backend
    m = re.search(r"lookupFunction<(\w+), (\w+)>\('tsh_mask_create_where'\)", dart)
    assert m
    for td in m.groups():
        t = re.search(r"typedef %s = \w+ Function\(([^;]*)\);" % td, dart)
        assert t and len(re.sub(r"<[^<>]*(<[^<>]*>)?[^<>]*>", "", t.group(1)).split(",")) == 6, td
    assert re.search(r"\bfinal class TshWhereTerm extends Struct\b", dart) and re.search(r"\bstatic HipRowMask\? whereClauses\(", dart)
    # a disposed handle is refused before the library sees it
    assert "createMaskWhereClauses with a disposed HipRowAttr" in dart and "createMaskWhereClauses with a disposed HipRowMask" in dart
    # the header's "Not here" list no longer names what this entry does
    assert "several terms in one launch" not in header
