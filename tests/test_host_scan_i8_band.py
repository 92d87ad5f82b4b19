"""CPU: the coarse int8 scan's error band (tostore_amd/csrc/tsh_scan_i8_band.h) against a software model of the kernel's
arithmetic -- tests/cpp/scan_i8_band_test.cpp, compiled here with g++ (the header has no HIP in it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_i8_band_cpp(tmp_path):
    exe = tmp_path / "scan_i8_band_test"
    src = os.path.join(ROOT, "tests", "cpp", "scan_i8_band_test.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "band ok" in p.stdout, p.stdout + p.stderr
