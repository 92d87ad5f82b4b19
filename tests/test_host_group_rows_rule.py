"""CPU: the rules of a grouped search with several rows per group (tostore_amd/csrc/tsh_group_rows_rule.h) -- the marked
groups and their slot words, the radix select for a group's m-th key, the member predicate and the finaliser's step --
against a software model of the scan's key at both ends of its claimed error bound and a brute-force answer, the
finaliser's step against the specification written a second time, and the counter-example of a group spanning two shards:
tests/cpp/group_rows_rule_test.cpp, compiled here with g++ (the header has no HIP in it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_rows_rule_cpp(tmp_path):
    exe = tmp_path / "group_rows_rule_test"
    src = os.path.join(ROOT, "tests", "cpp", "group_rows_rule_test.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "group rows rule ok" in p.stdout, p.stdout + p.stderr
