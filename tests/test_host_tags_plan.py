"""CPU: the host side of a tag column and its HAS ANY / HAS ALL term (tostore_amd/csrc/tsh_tags_plan.h: the caller's CSR
normalised to sorted, deduplicated rows with NULL flags; tsh_tags_set's splice; the rebased 32-bit offsets and valid words
a shard's part uploads; the query set and its threshold; the one-row model of the kernel) --
tests/cpp/tags_plan_test.cpp, a program of its own built here with g++ under the address and undefined-behaviour
sanitizers (the header has no HIP in it) and run; nothing of it is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tags_plan_cpp(tmp_path):
    exe = tmp_path / "tags_plan_test"
    src = os.path.join(ROOT, "tests", "cpp", "tags_plan_test.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), src], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "tags plan ok" in p.stdout, p.stdout + p.stderr
