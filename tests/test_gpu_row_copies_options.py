"""GPU: the two reduced-precision copies of the rows side by side, and every option's accepted range.

A shard can hold an int8 copy of its rows (dense, all-live scans: TSH_OPT_SCAN_I8) and an fp16 copy (TSH_OPT_SCAN_F16,
TSH_OPT_SCAN_F16_MASKED) at the same time.  Both follow the row store: a reallocation releases them together and takes
their bytes off the shard's account, and the next scan rebuilds only the copy it reads.  Answers are those of a twin index
that never builds a copy.  tsh_index_set_option accepts exactly the documented range of every option and leaves the
setting alone when it refuses a value."""
import numpy as np
import pytest

from tostore_amd import _ffi

pytestmark = pytest.mark.gpu
L2 = 0


def _same(got, ref, what):
    assert np.array_equal(got[2], ref[2]), "counts differ from the twin's " + what
    assert np.array_equal(got[0], ref[0]), "ids differ from the twin's " + what
    assert np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), "distance bits differ from the twin's " + what


def test_both_copies_resident_then_released_together(hip_lib):
    from tostore_amd import HipVectorIndex

    d, n0, cap, n1, k = 256, 130, 192, 300, 5  # d = 256: the narrowest row the fp16 scan takes
    rng = np.random.default_rng(2024)
    rows = rng.standard_normal((n1, d)).astype(np.float32)
    rows *= rng.uniform(0.5, 2.0, size=(n1, 1)).astype(np.float32)
    qs = rng.standard_normal((4, d)).astype(np.float32)
    bytes16, bytes8 = cap * d * 2, cap * d + cap * 4

    def make(f16, i8):
        idx = HipVectorIndex(d, L2, capacity_rows=cap)
        idx.set_scan_f16(f16)
        idx.set_scan_f16_masked(2)
        idx.set_scan_i8(i8)
        idx.set_exact_scan_rows(0)  # tile scans: a shard this small would otherwise answer from its exact sums
        idx.set_batch_min_nq(0)
        idx.append(0, rows[:n0])
        return idx

    with make(2, 2) as idx, make(0, 0) as twin:
        def search(i, what):
            _same(idx.search(qs[i:i + 1], k), twin.search(qs[i:i + 1], k), what)
            return idx.scan_f16_stats(), idx.scan_i8_stats()

        f0, i0 = idx.scan_f16_stats(), idx.scan_i8_stats()
        assert f0["copy_bytes"] == 0 and i0["copy_bytes"] == 0
        # a dense search builds the int8 copy
        f1, i1 = search(0, "dense")
        assert i1["scans"] - i0["scans"] == 1 and i1["redone"] == 0, (i0, i1)
        assert i1["copy_bytes"] == bytes8 and i1["rows_converted"] == n0, i1
        assert f1["scans"] == 0 and f1["copy_bytes"] == 0, f1
        # a tombstone: the scan is masked now, and the fp16 copy is built beside the int8 copy
        for x in (idx, twin):
            x.set_deleted([7])
        f2, i2 = search(1, "one tombstone")
        assert f2["scans"] - f1["scans"] == 1 and f2["redone"] == 0, (f1, f2)
        assert f2["copy_bytes"] == bytes16 and f2["rows_converted"] == n0, f2
        assert i2["copy_bytes"] == bytes8 and i2["scans"] == i1["scans"] and i2["rows_converted"] == n0, i2
        # an append past the capacity: both copies are released with the old row store, and their bytes with them
        b0, t0 = idx.counters()["bytes_resident"], twin.counters()["bytes_resident"]
        for x in (idx, twin):
            x.append(n0, rows[n0:n1])
        b1, t1 = idx.counters()["bytes_resident"], twin.counters()["bytes_resident"]
        f3, i3 = idx.scan_f16_stats(), idx.scan_i8_stats()
        assert f3["copy_bytes"] == 0 and i3["copy_bytes"] == 0, (f3, i3)
        assert t1 > t0, "the append did not grow the row store"
        assert b1 - b0 == (t1 - t0) - bytes16 - bytes8, (b0, b1, t0, t1)
        # the next search rebuilds the fp16 copy only, from row 0
        f4, i4 = search(2, "after the append")
        assert f4["scans"] - f3["scans"] == 1 and f4["redone"] == 0, (f3, f4)
        assert f4["rows_converted"] - f3["rows_converted"] == n1 and f4["copy_bytes"] > bytes16, (f3, f4)
        assert i4 == i3, (i3, i4)
        assert idx.counters()["bytes_resident"] - b1 >= f4["copy_bytes"]
        _same(idx.search(qs, k), twin.search(qs, k), "all queries at the end")


# option -> (lowest, highest) documented value (include/tostore_hip.h)
RANGES = {
    _ffi.TSH_OPT_BATCH_MIN_NQ: (0, 1 << 20),
    _ffi.TSH_OPT_BATCH_KERNEL: (0, 3),
    _ffi.TSH_OPT_EXACT_SCAN_ROWS: (0, 16384),
    _ffi.TSH_OPT_EXACT_SELECT: (0, 1),
    _ffi.TSH_OPT_BATCH_HUB: (0, 1),
    _ffi.TSH_OPT_BATCH_GROUP: (0, 1),
    _ffi.TSH_OPT_SCAN_F16: (0, 2),
    _ffi.TSH_OPT_SCAN_F16_MASKED: (0, 2),
    _ffi.TSH_OPT_SCAN_I8: (0, 2),
}


def test_every_options_edges(hip_lib):
    """The lowest and the highest documented value are taken, one below and one above are refused and change nothing:
    where a search's counters show the setting in force -- the exact path's, the int8 and the fp16 routes', the batched
    key kernel -- they show the last accepted value, with the highest and with the lowest in force."""
    from tostore_amd import HipVectorIndex

    L = hip_lib
    n = 64
    rng = np.random.default_rng(5)

    def corpus(d, rows=n):
        return rng.standard_normal((rows, d)).astype(np.float32), rng.standard_normal((8, d)).astype(np.float32)

    def set_opt(idx, opt, value):
        return L.tsh_index_set_option(idx._h, opt, value)

    def refused(idx, opt, lo, hi):
        for bad in (lo - 1, hi + 1):
            assert set_opt(idx, opt, bad) == _ffi.TSH_E_BAD_ARG, (opt, bad)
            assert _ffi.last_error(), (opt, bad)

    rows, qs = corpus(8)
    with HipVectorIndex(8, L2, capacity_rows=n) as idx:
        idx.append(0, rows)
        for opt, (lo, hi) in RANGES.items():
            for value in (hi, lo):
                assert set_opt(idx, opt, value) == _ffi.TSH_OK, (opt, value)
            refused(idx, opt, lo, hi)
        assert set_opt(idx, 11, 0) == _ffi.TSH_E_BAD_ARG and set_opt(idx, 0, 0) == _ffi.TSH_E_BAD_ARG  # unknown ids
        assert set_opt(idx, 999, 1) == _ffi.TSH_E_BAD_ARG
        for h in (idx._h, None):
            assert L.tsh_index_set_option(h, _ffi.TSH_OPT_TEST_HOOKS, _ffi.TSH_TEST_HOOKS_MAGIC + 1) == _ffi.TSH_E_BAD_ARG
            assert L.tsh_index_set_option(h, _ffi.TSH_OPT_EXCHANGE_AHEAD, 2) == _ffi.TSH_E_BAD_ARG
        assert L.tsh_index_set_option(None, _ffi.TSH_OPT_SCAN_I8, 1) == _ffi.TSH_E_BAD_ARG  # a per-shard option without an index

    def in_force(d, opt, observe, setup=(), rows=n):
        """observe(idx) -> what one search shows of the setting; the same with the highest and with the lowest in force,
        each followed by the two refused values"""
        data, qs = corpus(d, rows)
        lo, hi = RANGES[opt]
        seen = []
        with HipVectorIndex(d, L2, capacity_rows=rows) as idx:
            idx.set_batch_min_nq(0)
            for o, v in setup:
                assert set_opt(idx, o, v) == _ffi.TSH_OK
            idx.append(0, data)
            for value in (hi, lo):
                assert set_opt(idx, opt, value) == _ffi.TSH_OK
                refused(idx, opt, lo, hi)
                seen.append(observe(idx, qs))
        return seen

    def delta(stat):
        def observe(idx, qs):
            before = stat(idx)
            idx.search(qs[:1], 5)
            return stat(idx) - before
        return observe

    def masked_f16_scans(idx, qs):
        keep = np.ones(n, bool)
        keep[3] = False  # 63 of 64 rows kept: a tile scan behind the mask, not a list
        before = idx.scan_f16_stats()["scans"]
        idx.search(qs[:1], 5, None, np.packbits(keep, bitorder="little"))
        return idx.scan_f16_stats()["scans"] - before

    def batch_kernel(idx, qs):
        idx.set_batch_min_nq(2)
        idx.search(qs, 5)
        return idx.counters()["batch_kernel_last"]

    no_exact = ((_ffi.TSH_OPT_EXACT_SCAN_ROWS, 0),)
    assert in_force(8, _ffi.TSH_OPT_EXACT_SCAN_ROWS, delta(lambda i: i.counters()["exact_scans"])) == [1, 0]
    assert in_force(256, _ffi.TSH_OPT_SCAN_I8, delta(lambda i: i.scan_i8_stats()["scans"])) == [1, 0]
    assert in_force(256, _ffi.TSH_OPT_SCAN_F16, delta(lambda i: i.scan_f16_stats()["scans"]),
                    no_exact + ((_ffi.TSH_OPT_SCAN_I8, 0),)) == [1, 0]
    assert in_force(256, _ffi.TSH_OPT_SCAN_F16_MASKED, masked_f16_scans, no_exact + ((_ffi.TSH_OPT_SCAN_F16, 2),)) == [1, 0]
    auto, mfma = in_force(64, _ffi.TSH_OPT_BATCH_KERNEL, batch_kernel, rows=4096)  # (the smallest shard that batches)
    assert auto in (1, 2) and mfma == 0, (auto, mfma)  # 3 = auto: bf16x3 or fp16 keys by the corpus; 0 = f32 MFMA
