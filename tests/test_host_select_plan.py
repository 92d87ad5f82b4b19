"""CPU: the K2 select's plan (tostore_amd/csrc/tsh_select_plan.h) -- tests/cpp/select_plan_test.cpp, compiled here with
g++ (the header has no HIP in it): which of the three instantiations of select_kernel a search takes, and every path
predicate of select_tau / select_body on both sides of its edge (tiles 64/65, 512/513, 16384/16385; k 128/129, 256/257,
512/513, 1024/1025; M < k, M == k, 64 M == k, 64 M < k).  tests/test_abi.py holds tsh_default_block_entries, which
answers from the same header, on the library's side."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_select_plan_cpp(tmp_path):
    out = tmp_path / "select_plan_test"
    src = os.path.join(ROOT, "tests", "cpp", "select_plan_test.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(out), src], check=True)
    p = subprocess.run([str(out)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "select plan ok" in p.stdout, p.stdout + p.stderr
