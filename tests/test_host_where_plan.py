"""CPU: the host plan of a WHERE clause (tostore_amd/csrc/tsh_where_plan.h: the table of distinct columns, the IN terms'
values sorted and deduped into one array, the 32-byte term records with their clause flags) --
tests/cpp/where_plan_test.cpp, a program of its own built here with g++ under the address and undefined-behaviour
sanitizers (the header has no HIP in it) and run; nothing of it is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_where_plan_cpp(tmp_path):
    exe = tmp_path / "where_plan_test"
    src = os.path.join(ROOT, "tests", "cpp", "where_plan_test.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), src], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "where plan ok" in p.stdout, p.stdout + p.stderr
