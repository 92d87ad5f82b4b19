"""CPU: the rules of a grouped cursor search and of a group count (tostore_amd/csrc/tsh_group_after_rule.h) -- the head
classes against the cursor's floor keys and the count's window, the side predicate and the two finaliser steps -- against a
software model of the scan's key at both ends of its claimed error bound and a brute-force "G after the cursor": pages for
k in {1, 10, all}, counts, no consumed group from the "certainly before" case, pages concatenating to G:
tests/cpp/group_after_rule_test.cpp, compiled here with g++ (the header has no HIP in it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_after_rule_cpp(tmp_path):
    exe = tmp_path / "group_after_rule_test"
    src = os.path.join(ROOT, "tests", "cpp", "group_after_rule_test.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "group after rule ok" in p.stdout, p.stdout + p.stderr
