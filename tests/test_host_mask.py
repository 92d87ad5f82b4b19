"""A caller's WHERE bitmap sliced to one shard's rows, on the CPU (tostore_amd/csrc/tsh_host_sync.h slice_mask,
mask_kept_rows, popcount_words, list_mask_bits): every row base 0..71 plus 12 347, 23 360 and 2^20 + 3, every shard
length 1..200 plus 4095..4097 and 65 535..65 537, the shard's range zero, all ones or random with every bit around it
set -- a bitmap sized for capacity, or the global one each rank is handed.  The slice must hold the range's bits and no
other: its words bit for bit, their popcount, their list and the unsliced count all equal what NumPy's unpackbits of
the range says."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slice_mask_at_byte_tile_and_shard_edges(tmp_path):
    exe = tmp_path / "host_mask_test"
    src = os.path.join(ROOT, "tests", "cpp", "host_mask_test.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", str(exe), src], check=True)
    rnd = np.random.default_rng(907).integers(0, 256, 65537 // 8 + 16, dtype=np.uint8)
    (tmp_path / "rnd.bin").write_bytes(rnd.tobytes())
    out = tmp_path / "cases.bin"
    r = subprocess.run([str(exe), str(tmp_path / "rnd.bin"), str(out)], capture_output=True, text=True, timeout=300)
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr)
    assert r.returncode == 0, r.stderr
    bases = list(range(72)) + [12_347, 23_360, (1 << 20) + 3]
    lens = list(range(1, 201)) + [4095, 4096, 4097, 65_535, 65_536, 65_537]
    assert r.stdout.split() == ["ok", str(len(bases) * len(lens) * 4), "cases"]
    rbits = np.unpackbits(rnd, bitorder="little")

    want = {}  # (rows, kind) -> (words as bytes, popcount, count, sum of ids, weighted sum): the range's bits, nothing past

    def expected(rows, kind):
        if (rows, kind) not in want:
            bits = np.zeros(rows, np.uint8) if kind == 0 else np.ones(rows, np.uint8) if kind == 1 else rbits[:rows]
            n_words = (rows + 63) // 64 + 1
            packed = np.zeros(n_words * 8, np.uint8)
            p = np.packbits(bits, bitorder="little")
            packed[:p.size] = p
            ids = np.flatnonzero(bits).astype(np.uint64)
            w = np.arange(1, ids.size + 1, dtype=np.uint64)
            want[(rows, kind)] = (packed.tobytes(), int(bits.sum()), ids.size, int(ids.sum(dtype=np.uint64)),
                                  int((ids * w).sum(dtype=np.uint64)))
        return want[(rows, kind)]

    data = out.read_bytes()
    pos, bad = 0, []
    for base in bases:
        for rows in lens:
            for kind in range(4):
                rec = np.frombuffer(data, np.int64, 8, pos)
                n_words = (rows + 63) // 64 + 1
                words = data[pos + 64:pos + 64 + 8 * n_words]
                pos += 64 + 8 * n_words
                assert (int(rec[0]), int(rec[1]), int(rec[2])) == (base, rows, kind)
                wb, pop, cnt, s, ws = expected(rows, kind)
                got = (words == wb, int(rec[3]) == pop, int(rec[4]) == pop, int(rec[5]) == cnt,
                       int(rec[6]) & (2**64 - 1) == s, int(rec[7]) & (2**64 - 1) == ws)
                if not all(got):
                    bad.append((base, rows, kind, int(rec[3]), pop, int(rec[4]),
                                [n for n, ok in zip(("words", "popcount", "kept", "listed", "ids", "order"), got) if not ok]))
    assert pos == len(data)
    assert not bad, "%d of %d cases wrong, e.g. (row_base, rows, kind, popcount, want, kept, what): %s" % (
        len(bad), len(bases) * len(lens) * 4, bad[:8])
