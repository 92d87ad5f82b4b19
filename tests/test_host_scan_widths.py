"""CPU: row width -> tile-scan instantiation (tostore_amd/csrc/tsh_scan_widths.h) and the width list of the GPU sweep
(tests/golden/scan_width_sweep.json, run by tests/test_gpu_scan_widths.py) -- tests/cpp/scan_widths_test.cpp, compiled
here with g++ (the header has no HIP in it): pick_nch, the fp16 and int8 families' predicates at their edges, and that
the list's widths reach every (family, chunk count, kind of row) any width can reach.  The list itself is held to the
rule it was written by, and taking any one width out of it must be noticed."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST = os.path.join(ROOT, "tests", "golden", "scan_width_sweep.json")
NCHS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("scan_widths") / "scan_widths_test"
    src = os.path.join(ROOT, "tests", "cpp", "scan_widths_test.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(out), src], check=True)
    return str(out)


def _run(exe, path):
    return subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)


def test_scan_widths_cpp(exe):
    p = _run(exe, LIST)
    print(p.stdout)
    assert p.returncode == 0 and "scan widths ok" in p.stdout, p.stdout + p.stderr


def test_the_list_is_the_rule():
    """Per chunk count: the full width, a row ending 72 elements (fp16-eligible) and 101 elements (three pad elements)
    into its last chunk and, from ten chunks on, one that leaves a chunk empty; the four packed-row widths."""
    widths = json.load(open(LIST))
    assert all(type(w) is int for w in widths) and widths == sorted(set(widths))
    want = {30, 32, 64, 128}
    for n in NCHS:
        want |= {256 * n, 256 * (n - 1) + 72, 256 * (n - 1) + 101}
        if n >= 10:
            want.add(256 * (n - 2) + 72)
    assert set(widths) == want and len(widths) == 44


def test_a_dropped_width_is_noticed(exe, tmp_path):
    """Without any one of its widths the list no longer reaches every instantiation (or every chunk count with pad
    elements) -- but for d = 32, 72 and 3912, whose instantiations d = 30, 101 and 3941 reach as well: those three are
    held by test_the_list_is_the_rule alone."""
    widths = json.load(open(LIST))
    unnoticed = []
    for w in widths:
        path = tmp_path / ("without_%d.json" % w)
        path.write_text(json.dumps([x for x in widths if x != w]))
        p = _run(exe, path)
        if p.returncode == 0:
            unnoticed.append(w)
        else:
            assert "MISS" in p.stdout, p.stdout + p.stderr
    assert unnoticed == [32, 72, 3912]
