"""CPU: the host side of a facet count (tostore_amd/csrc/tsh_facet_plan.h: the caller's keys normalised to the sorted set
the kernels stage, the edge rules, the bucket rule both kernels include, the one-word models of the two kernels, the
quarantined rows' share, the sum over shards and the scatter to the caller's order) -- tests/cpp/facet_plan_test.cpp, a
program of its own built here with g++ under the address and undefined-behaviour sanitizers (the header has no HIP in
it) and run; nothing of it is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facet_plan_cpp(tmp_path):
    exe = tmp_path / "facet_plan_test"
    src = os.path.join(ROOT, "tests", "cpp", "facet_plan_test.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), src], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "facet plan ok" in p.stdout, p.stdout + p.stderr
