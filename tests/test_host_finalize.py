"""CPU: the finaliser (tostore_amd/csrc/tsh_finalize.h: finalize_query, count_entries, Cursors) against a plain
filter-sort-cut reference over seeded candidate lists -- tests/cpp/finalize_test.cpp, compiled here with g++ (the header
has no HIP in it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_finalize_cpp(tmp_path):
    exe = tmp_path / "finalize_test"
    src = os.path.join(ROOT, "tests", "cpp", "finalize_test.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "finalize ok" in p.stdout, p.stdout + p.stderr
