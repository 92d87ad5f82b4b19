"""CPU: the window of a count (tostore_amd/csrc/tsh_count_band.h) against a software model of the scan's key at both ends
of its claimed error bound, and the finaliser's exact predicate against the specification written a second time --
tests/cpp/count_window_test.cpp, compiled here with g++ (the header has no HIP in it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_count_window_cpp(tmp_path):
    exe = tmp_path / "count_window_test"
    src = os.path.join(ROOT, "tests", "cpp", "count_window_test.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "window ok" in p.stdout, p.stdout + p.stderr
