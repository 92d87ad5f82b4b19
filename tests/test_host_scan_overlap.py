"""CPU: which single-query scans alternate between the two scan streams (tostore_amd/csrc/tsh_scan_overlap.h): the
decisions for the shapes the rule was made for, the small-shard edge, the drain share at the first big-shard tile count
and monotonicity -- tests/cpp/scan_overlap_rule_test.cpp, compiled here with g++ (the header has no HIP in it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_overlap_rule_cpp(tmp_path):
    exe = tmp_path / "scan_overlap_rule_test"
    src = os.path.join(ROOT, "tests", "cpp", "scan_overlap_rule_test.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), src], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "overlap rule ok" in p.stdout, p.stdout + p.stderr
