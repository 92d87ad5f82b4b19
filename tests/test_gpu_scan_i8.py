"""GPU: the coarse int8 first pass of single-query scans (TSH_OPT_SCAN_I8, scan_i8_kernel + tsh_scan_i8.hip.h).

Dense, all-live scans read an int8 copy of the rows -- a quarter of the f32 bytes -- whose keys carry a proven per-row
band (tostore_amd/csrc/tsh_scan_i8_band.h); the rows whose lower side is at or below the k-th smallest tile minimum of
upper sides go through the exact scan + select, so answers must stay the oracle's bit for bit.  Every index here
forces the route on small shapes (option 2), switches the batched path off, and is held to the oracle: ids, counts
and distance bits.  A parity case also asserts that the route RAN and that nothing was redone through the f32 scan."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, IP, COS = 0, 1, 2
N = 20_037  # not a multiple of 64: 314 tiles, the last one ragged
RATIOS = []


def _open(d, metric, rows, capacity=None, mode=2, pick=True):
    from tostore_amd import HipVectorIndex

    idx = HipVectorIndex(d, metric, capacity_rows=capacity or len(rows))
    idx.set_scan_i8(mode)
    idx.set_batch_min_nq(0)
    idx.set_exact_select(pick)
    if len(rows):
        idx.append(0, rows)
    return idx


def _same(got, ref, what=""):
    assert np.array_equal(got[2], ref[2]), "counts differ from the oracle's " + what
    assert np.array_equal(got[0], ref[0]), "ids differ from the oracle's " + what
    assert np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), "distance bits differ from the oracle's " + what


def _corpus(rng, n, d, metric, nq=4):
    rows = rng.standard_normal((n, d)).astype(np.float32)
    if metric != COS:
        rows *= rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    qs = rng.standard_normal((nq, d)).astype(np.float32)
    return rows, qs


def _ran(idx, s0, n, what=""):
    s1 = idx.scan_i8_stats()
    assert s1["scans"] - s0["scans"] == n and s1["redone"] == s0["redone"], (what, s0, s1)
    return s1


@pytest.mark.parametrize("n,d,metric,ks", [
    (N, 768, L2, (100, 1)),  # k = 1: the wide pick behind the exact scan
    (N, 768, IP, (100,)),
    (N, 768, COS, (100,)),
    (40_000, 100, L2, (10,)),  # a one-chunk row that ends inside its chunk
    (N, 1000, L2, (100,)),     # a part-filled last chunk
])
def test_parity(hip_lib, oracle_mod, n, d, metric, ks):
    rng = np.random.default_rng(100 * d + metric)
    rows, qs = _corpus(rng, n, d, metric)
    if metric == COS:
        qs = np.stack([oracle_mod.normalize_f32(q) for q in qs])
    with _open(d, metric, rows) as idx:
        for k in ks:
            ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k)
            s0 = idx.scan_i8_stats()
            _same(idx.search(qs, k), ref, "k=%d" % k)
            s1 = _ran(idx, s0, len(qs), "k=%d" % k)
            if k == ks[0] and d == 768 and metric == L2:  # the ticket entry takes the same route
                tickets = [idx.submit(q, k) for q in qs]
                for i, t in enumerate(tickets):
                    ids, dist = idx.wait(t)
                    assert np.array_equal(ids, ref[0][i, :ref[2][i]]), i
                    assert np.array_equal(dist.view(np.uint64), ref[1][i, :ref[2][i]].view(np.uint64)), i
                s1 = _ran(idx, s1, len(qs), "tickets")
        assert s1["rows_converted"] == n and s1["copy_bytes"] >= n * d
        assert idx.scan_f16_stats()["copy_bytes"] == 0  # no fp16 copy for a shard whose scans all take this route
    if d == 768 and metric == L2:  # E2 where the wide pick ran (k = 1)
        with _open(d, metric, rows, pick=False) as idx:
            _same(idx.search(qs, 1), oracle_mod.search_heap_many_mt(rows, qs, metric, 1), "k=1, E2")
            _ran(idx, {"scans": 0, "redone": 0}, len(qs))


def test_copy_stays_current_and_option_0(hip_lib, oracle_mod):
    """An append past the watermark, an overwrite, a row with an inf element; then option 0."""
    d, k, metric = 768, 20, L2
    rng = np.random.default_rng(31)
    rows, qs = _corpus(rng, 17_000, d, metric)
    n0, n1 = 12_000, 17_000
    with _open(d, metric, rows[:n0], capacity=18_048) as idx:
        def check(n, what, fresh, ran=True):
            s0 = idx.scan_i8_stats()
            _same(idx.search(qs, k), oracle_mod.search_heap_many_mt(rows[:n], qs, metric, k), what)
            s1 = idx.scan_i8_stats()
            assert s1["scans"] - s0["scans"] == (len(qs) if ran else 0) and s1["redone"] == 0, (what, s0, s1)
            assert s1["rows_converted"] - s0["rows_converted"] == fresh, (what, s0, s1)

        check(n0, "at first", n0)
        idx.append(n0, rows[n0:n1])
        check(n1, "after an append", n1 - n0)  # only the rows past the watermark
        r = 4321
        rows[r] = (qs[1] + 0.01 * rng.standard_normal(d)).astype(np.float32)  # a stored row becomes a query's nearest
        idx.append(r, rows[r:r + 1])
        check(n1, "after an overwrite", n1)  # rebuilt
        idx.set_scan_i8(0)
        check(n1, "option 0", 0, ran=False)
        idx.set_scan_i8(2)
        rows[77, 5] = np.inf  # quarantined: the shard is no longer all-live, its scans take another route
        idx.append(77, rows[77:78])
        check(n1, "with a quarantined row", 0, ran=False)


def test_overflow_is_redone_and_denied(hip_lib, oracle_mod):
    """8 192 copies of one row, the query's nearest: every copy survives, the list (4 096) overflows.  The answer is the
    oracle's through the f32 redo, once per query; after two in a row the third query does not take the route."""
    d, k, metric = 768, 100, L2
    rng = np.random.default_rng(77)
    rows, qs = _corpus(rng, N, d, metric, nq=3)
    twin = (qs[0] + 0.05 * rng.standard_normal(d)).astype(np.float32)
    qs[1] = twin + 0.01 * rng.standard_normal(d).astype(np.float32)
    qs[2] = twin - 0.01 * rng.standard_normal(d).astype(np.float32)
    where = np.sort(rng.choice(N, 8192, replace=False))
    rows[where] = twin
    ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k)
    assert np.array_equal(ref[0][0], where[:k])  # ties: the lowest ids first
    with _open(d, metric, rows) as idx:
        for i in range(3):
            got = idx.search(qs[i:i + 1], k)
            _same(got, tuple(x[i:i + 1] for x in ref), "query %d" % i)
            st = idx.scan_i8_stats()
            assert st["scans"] == min(i + 1, 2) and st["redone"] == min(i + 1, 2), (i, st)


def test_k_around_the_number_of_tiles(hip_lib, oracle_mod):
    """4 000 rows are 63 tiles: k = 62, 63 (a bound from nearly every tile), 64 and 100 (fewer live tiles than k: no bound,
    every row survives).  All of them fit the list of 4 096, so nothing is redone -- at 20 037 rows k = 315 would leave
    every row a survivor and go through the f32 redo, which proves nothing about this route."""
    d, metric = 768, L2
    rng = np.random.default_rng(5)
    rows, qs = _corpus(rng, 4000, d, metric)
    with _open(d, metric, rows) as idx:
        for k in (62, 63, 64, 100):
            s0 = idx.scan_i8_stats()
            _same(idx.search(qs, k), oracle_mod.search_heap_many_mt(rows, qs, metric, k), "k=%d" % k)
            _ran(idx, s0, len(qs), "k=%d" % k)


def test_big_shard_launch_shape(hip_lib, oracle_mod):
    """From 6144 tiles on the scan is launched in the dense scans' shape -- several waves per workgroup, a workgroup per
    two or four tiles -- where every shard above runs one-wave workgroups: the smallest such shard (d = 256: 403 MB of
    rows), its last tile ragged."""
    d, k, metric = 256, 20, L2
    n = 6144 * 64 + 37
    rng = np.random.default_rng(17)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    rows *= rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    qs = rng.standard_normal((4, d), dtype=np.float32)
    ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k)
    with _open(d, metric, rows) as idx:
        s0 = idx.scan_i8_stats()
        _same(idx.search(qs, k), ref)
        _ran(idx, s0, len(qs))


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_band_probe_on_midpoint_rows(hip_lib, metric):
    """Rows whose elements sit at quantisation midpoints (codes +/- 1/2), every error of the sign of its q_j: every exact
    key (f64) lies inside [lower, upper]."""
    d, n = 768, 4096
    rng = np.random.default_rng(9000 + metric)
    q = rng.standard_normal(d).astype(np.float32)
    s0 = np.ldexp(1.0, -rng.integers(0, 12, size=n))[:, None]
    c = 2.0 * rng.integers(-63, 63, size=(n, d))
    rows = (c + np.where(q > 0, 0.5, -0.5)[None, :]) * s0
    rows[np.arange(n), np.arange(n) % d] = 127.0 * s0[:, 0]  # pins every row's scale to its s0
    rows = rows.astype(np.float32)
    r64, q64 = rows.astype(np.float64), q.astype(np.float64)
    dot, nrm2 = r64 @ q64, np.einsum("ij,ij->i", r64, r64)
    exact = nrm2 - 2.0 * dot if metric == L2 else (-dot if metric == IP else -dot / np.sqrt(nrm2))
    with _open(d, metric, rows) as idx:
        lo, up = idx.probe_scan_i8_keys(q)
    lo, up = lo.astype(np.float64), up.astype(np.float64)
    w = (up - lo) / 2
    ratio = np.abs((lo + up) / 2 - exact) / w
    print("metric %d: max |key - exact| / w on midpoint rows: %.4f" % (metric, ratio.max()))
    RATIOS.append({"metric": ["l2", "ip", "cosine"][metric], "dim": d, "max_abs_err_over_w_midpoints": float(ratio.max())})
    assert np.all(np.isfinite(lo)) and np.all(lo <= exact) and np.all(exact <= up), float(ratio.max())


def test_zz_write_band_ratios():
    if RATIOS:
        with open(os.path.join(ROOT, "profiles", "scan_i8_band_ratios.json"), "w") as f:
            json.dump(RATIOS, f, indent=1)
            f.write("\n")
