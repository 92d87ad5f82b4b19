"""Worker of tests/test_gpu_scan_f16.py: the fp16 copy of the rows (30.8 MB here) cannot be allocated
(TSH_TEST_FAIL_ALLOC_OVER = 16 MB, obeyed only after the test hooks were asked for -- hence a process of its own): the
searches must answer from the f32 scan, bit-exact, without asking for the copy again, and the handle must stay usable."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle  # noqa: E402
from tostore_amd import HipVectorIndex, _ffi  # noqa: E402

oracle.build()
_ffi.enable_test_hooks()
rng = np.random.default_rng(3)
n, d, k = 20_037, 768, 30
rows = (rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, size=(n, 1))).astype(np.float32)
qs = rng.standard_normal((6, d)).astype(np.float32)
ok = True
with HipVectorIndex(d, 0, capacity_rows=n + 64) as idx:
    idx.set_scan_f16(2)
    idx.set_exact_scan_rows(0)
    idx.set_batch_min_nq(0)
    idx.append(0, rows[:n - 10])
    for upto in (n - 10, n):
        if upto == n:
            idx.append(n - 10, rows[n - 10:])
        ids, dist, cnt = idx.search(qs, k)
        ref = oracle.search_heap_many_mt(rows[:upto], qs, 0, k)
        ok &= bool(np.array_equal(cnt, ref[2]) and np.array_equal(ids, ref[0])
                   and np.array_equal(dist.view(np.uint64), ref[1].view(np.uint64)))
    st = idx.scan_f16_stats()
    ok &= st["scans"] == 0 and st["copy_bytes"] == 0 and st["rows_converted"] == 0
    print(st)
print("degraded ok" if ok else "MISMATCH")
sys.exit(0 if ok else 1)
