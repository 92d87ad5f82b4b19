"""CPU: TSH_OPT_SCAN_I8_MASKED has one number, 13, in the header, the ctypes table and the Dart bridge; the Python
index has its setter; option id 11 stays unassigned (the suite pins it as an unknown id)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_defines():
    with open(os.path.join(ROOT, "include", "tostore_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return {name: int(value) for name, value in re.findall(r"^#define\s+(TSH_OPT_[A-Z0-9_]+)\s+(\d+)\s*$", text, flags=re.M)}


def test_header_defines_the_option_as_13():
    opts = _header_defines()
    assert opts.get("TSH_OPT_SCAN_I8_MASKED") == 13, opts
    assert len(set(opts.values())) == len(opts), "two options share a number"


def test_option_11_is_still_undefined():
    assert 11 not in _header_defines().values()


def test_ctypes_table_and_dart_bridge_carry_the_same_number():
    from tostore_amd import _ffi

    assert _ffi.TSH_OPT_SCAN_I8_MASKED == _header_defines()["TSH_OPT_SCAN_I8_MASKED"] == 13
    with open(os.path.join(ROOT, "tostore_amd", "dart", "tostore_hip_bridge.dart")) as f:
        dart = f.read()
    assert re.search(r"\b13 = TSH_OPT_SCAN_I8_MASKED\b", dart), "the bridge's option list does not name the option"
    m = re.search(r"static const int optScanI8Masked = (\d+);", dart)
    assert m and int(m.group(1)) == 13


def test_the_index_has_the_setter():
    from tostore_amd import HipVectorIndex

    assert callable(getattr(HipVectorIndex, "set_scan_i8_masked", None))
