"""CPU: the decisions of a batched (matrix-core) call (tostore_amd/csrc/tsh_batch_plan.h): the sample's size and window,
the estimate's order statistic against a long-double binomial tail, the key kernel's choice and scale, listed mode, the
tail's chunks, the cost model's stated decisions, the bands' rounding and the queries' norms --
tests/cpp/batch_plan_test.cpp, compiled here with g++ (the header has no HIP in it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_plan_cpp(tmp_path):
    exe = tmp_path / "batch_plan_test"
    src = os.path.join(ROOT, "tests", "cpp", "batch_plan_test.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "batch plan ok" in p.stdout, p.stdout + p.stderr
