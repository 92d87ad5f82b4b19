"""CPU: the 4-bit first pass's error band (tostore_amd/csrc/tsh_scan_i4_band.h) against a software model of the kernel's
arithmetic -- tests/cpp/scan_i4_band_test.cpp, compiled here with g++ (the header has no HIP in it), once plainly and
once as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_scan_i4_band_cpp(tmp_path, flags):
    exe = tmp_path / "scan_i4_band_test"
    src = os.path.join(ROOT, "tests", "cpp", "scan_i4_band_test.cpp")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", str(exe), src], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and "band ok" in p.stdout, p.stdout + p.stderr
