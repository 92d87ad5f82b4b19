"""CPU: the tile order of the batched key passes (tostore_amd/csrc/tsh_batch_tiles.h: which query tile and row tile
workgroup slot b scores) -- tests/cpp/batch_tiles_test.cpp, compiled here with g++ (the header has no HIP in it).  For
q_tiles 1-8 and n_tiles 1-300: the map is a bijection; in full rounds q_tiles consecutive workgroups of an XCD share a
row tile; a persistent grid that is a multiple of 8 q_tiles keeps every workgroup on its query tile, and three query
tiles on a grid of 256 do not (what tests/test_gpu_batch_shapes.py::test_persistent_loop_changes_query_tile relies on)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_tiles_cpp(tmp_path):
    exe = tmp_path / "batch_tiles_test"
    src = os.path.join(ROOT, "tests", "cpp", "batch_tiles_test.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), src], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0 and "batch tiles ok" in p.stdout, p.stdout + p.stderr
