"""GPU: the single-query scan over the fp16 copy of the rows (TSH_OPT_SCAN_F16, scan_f16_kernel).

Big shards' dense scans read a resident fp16 copy -- half the HBM bytes per query -- whose keys carry a per-row band
w_i = alpha |v_i| + beta (tostore_amd/csrc/tsh_scan_f16_band.h); the f64 re-rank decides, so answers must stay the
oracle's bit for bit.  Every index here forces the route on small shapes (option 2), switches the exact path and the
batched path off, and is held to the oracle: ids, counts and distance bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_bands import _candidates, _exact_keys, _nudge_to, _patterned

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, IP, COS = 0, 1, 2
N = 20_037  # not a multiple of 64
RATIOS = []


def _open(d, metric, rows, capacity=None, mode=2):
    from tostore_amd import HipVectorIndex

    idx = HipVectorIndex(d, metric, capacity_rows=capacity or len(rows))
    idx.set_scan_f16(mode)
    idx.set_exact_scan_rows(0)
    idx.set_batch_min_nq(0)
    if len(rows):
        idx.append(0, rows)
    return idx


def _same(got, ref, what=""):
    assert np.array_equal(got[2], ref[2]), "counts differ from the oracle's " + what
    assert np.array_equal(got[0], ref[0]), "ids differ from the oracle's " + what
    assert np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), "distance bits differ from the oracle's " + what


def _corpus(rng, n, d, metric, nq=8):
    rows = rng.standard_normal((n, d)).astype(np.float32)
    if metric != COS:
        rows *= rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    qs = rng.standard_normal((nq, d)).astype(np.float32)
    return rows, qs


@pytest.mark.parametrize("metric", [L2, IP, COS])
@pytest.mark.parametrize("d", [768, 1000, 1024, 1536])
def test_parity(hip_lib, oracle_mod, d, metric):
    rng = np.random.default_rng(100 * d + metric)
    rows, qs = _corpus(rng, N, d, metric)
    if metric == COS:
        qs = np.stack([oracle_mod.normalize_f32(q) for q in qs])
    ref100 = oracle_mod.search_heap_many_mt(rows, qs, metric, 100)
    ref10 = oracle_mod.search_heap_many_mt(rows, qs, metric, 10)
    with _open(d, metric, rows) as idx:
        for k, ref in ((10, ref10), (100, ref100)):
            s0 = idx.scan_f16_stats()
            _same(idx.search(qs, k), ref, "k=%d" % k)
            s1 = idx.scan_f16_stats()
            assert s1["scans"] - s0["scans"] == len(qs) and s1["redone"] == 0, (s0, s1)
            if d == 768 and metric == L2 and k == 10:  # the ticket entry takes the same route
                tickets = [idx.submit(q, k) for q in qs]
                for i, t in enumerate(tickets):
                    ids, dist = idx.wait(t)
                    assert np.array_equal(ids, ref[0][i, :ref[2][i]]), i
                    assert np.array_equal(dist.view(np.uint64), ref[1][i, :ref[2][i]].view(np.uint64)), i
                s2 = idx.scan_f16_stats()
                assert s2["scans"] - s1["scans"] == len(qs) and s2["redone"] == 0, (s1, s2)
        assert s1["rows_converted"] == N and s1["copy_bytes"] >= N * d * 2


@pytest.mark.parametrize("metric", [L2, COS])
def test_ineligible_width_stays_on_f32(hip_lib, oracle_mod, metric):
    rng = np.random.default_rng(7 + metric)
    rows, qs = _corpus(rng, N, 200, metric)
    with _open(200, metric, rows) as idx:
        _same(idx.search(qs, 100), oracle_mod.search_heap_many_mt(rows, qs, metric, 100))
        assert idx.scan_f16_stats()["scans"] == 0 and idx.scan_f16_stats()["copy_bytes"] == 0


@pytest.mark.parametrize("metric", [L2, IP])
def test_copy_stays_current(hip_lib, oracle_mod, metric):
    """Appends past the watermark, overwrites, a reallocation and a change of the scale: every search afterwards reads
    a copy that matches the rows."""
    d, k = 768, 20
    rng = np.random.default_rng(31 + metric)
    rows, qs = _corpus(rng, 12_000 + 5_000 + 9_000 + 1, d, metric, nq=4)
    n0, n1, n2 = 12_000, 17_000, 26_000
    with _open(d, metric, rows[:n0], capacity=18_048) as idx:
        def check(n, what, fresh):
            s0 = idx.scan_f16_stats()
            _same(idx.search(qs, k), oracle_mod.search_heap_many_mt(rows[:n], qs, metric, k), what)
            s1 = idx.scan_f16_stats()
            assert s1["scans"] - s0["scans"] == len(qs) and s1["redone"] == s0["redone"], (what, s0, s1)
            assert s1["rows_converted"] - s0["rows_converted"] == fresh, (what, s0, s1)

        check(n0, "at first", n0)
        idx.append(n0, rows[n0:n1])
        check(n1, "after an append", n1 - n0)  # only the rows past the watermark
        # 50 stored rows become the queries' new nearest neighbours
        where = rng.choice(n1, 50, replace=False)
        for i, r in enumerate(where):
            v = qs[i % len(qs)] * (1.0 if metric == L2 else 3.0) + 0.01 * rng.standard_normal(d)
            rows[r] = v.astype(np.float32)
            idx.append(int(r), rows[r:r + 1])
        check(n1, "after overwrites", n1)  # rebuilt
        idx.append(n1, rows[n1:n2])  # past the capacity: the row store reallocates
        check(n2, "after a reallocation", n2)
        rows[n2] = rows[0]
        rows[n2, 5] = 3.0e5  # the largest element by far: another power-of-two scale
        idx.append(n2, rows[n2:n2 + 1])
        check(n2 + 1, "after a change of the scale", n2 + 1)


def test_outside_the_route(hip_lib, oracle_mod):
    d, k, metric = 768, 30, L2
    rng = np.random.default_rng(5)
    rows, qs = _corpus(rng, N, d, metric, nq=4)
    with _open(d, metric, rows) as idx:
        _same(idx.search(qs, k), oracle_mod.search_heap_many_mt(rows, qs, metric, k))
        base = idx.scan_f16_stats()["scans"]
        assert base == len(qs)
        mask = np.packbits(rng.random(N) < 0.7, bitorder="little")
        _same(idx.search(qs, k, None, mask), oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, mask), "behind a mask")
        assert idx.scan_f16_stats()["scans"] == base
        idx.set_scan_f16(0)
        _same(idx.search(qs, k), oracle_mod.search_heap_many_mt(rows, qs, metric, k), "option 0")
        assert idx.scan_f16_stats()["scans"] == base
        idx.set_scan_f16(1)  # auto: 61 MB of rows are far below the size gate
        _same(idx.search(qs, k), oracle_mod.search_heap_many_mt(rows, qs, metric, k), "option 1")
        assert idx.scan_f16_stats()["scans"] == base
        idx.set_scan_f16(2)
        idx.set_deleted([int(oracle_mod.search_heap_many_mt(rows, qs[:1], metric, 1)[0][0, 0])])
        dead = np.ones(N, bool)
        dead[int(oracle_mod.search_heap_many_mt(rows, qs[:1], metric, 1)[0][0, 0])] = False
        live_mask = np.packbits(dead, bitorder="little")
        _same(idx.search(qs, k), oracle_mod.search_heap_many_mt(rows, qs, metric, k, None, live_mask), "after a tombstone")
        assert idx.scan_f16_stats()["scans"] == base


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("d", [768, 1536])
def test_band_held_row_by_row(hip_lib, oracle_mod, d, metric):
    """(1) Rows whose operands sit at fp16 rounding midpoints -/+ 1 ulp, all products of one sign, norms a factor 16
    apart (and a tail of rows deep in fp16's subnormal steps): |stored key - w - exact| <= w for every row.
    (2) A 40 960-row corpus whose true top k and 2 k outsiders sit inside the claimed band with their approximate order
    inverted: the oracle's answer, nothing redone."""
    K = 50
    rng = np.random.default_rng(9000 + 10 * metric + d)
    q = _patterned(rng, d, 2, up=False)
    base = np.stack([_patterned(rng, d, 2, up=bool(i & 1)) for i in range(4096)])
    expo = np.where(rng.random(len(base)) < 0.8, rng.integers(0, 5, size=len(base)), rng.integers(5, 27, size=len(base)))
    rows = base * np.ldexp(1.0, -expo).astype(np.float32)[:, None]
    qn2 = float(q.astype(np.float64) @ q.astype(np.float64))

    def exact_of(r):  # what the fp16 kernel's key stands for: the L2 key leaves the common |q|^2 out
        e = _exact_keys(r, q, metric)
        return e - qn2 if metric == L2 else e

    with _open(d, metric, rows) as idx:
        up, w = idx.probe_scan_f16_keys(q)
    up, w = up.astype(np.float64), w.astype(np.float64)
    ratio = np.abs(up - w - exact_of(rows)) / w
    print("max |key - exact| / w on patterned rows: %.4f" % ratio.max())
    assert np.all(np.isfinite(up)) and ratio.max() <= 1.0, "a key is further from its exact value than its row's band: %.4f" % ratio.max()
    nrm = np.sqrt(np.einsum("ij,ij->i", rows.astype(np.float64), rows.astype(np.float64)))
    assert w[nrm < nrm.max() / 8].max() < 0.2 * w.max(), "short rows do not carry a narrower band"

    # ---- (2) the worst cases around a boundary (the construction of test_gpu_bands.py, fp16 patterns) -------------
    qc, cand, kb = _candidates(rng, d, metric, 2, float(np.median(w)), None)
    qcn2 = float(qc.astype(np.float64) @ qc.astype(np.float64))
    with _open(d, metric, cand) as idx:
        up0, w0 = idx.probe_scan_f16_keys(qc)
    ex0 = _exact_keys(cand, qc, metric)
    k0 = up0.astype(np.float64) - w0 + (qcn2 if metric == L2 else 0.0)  # on _exact_keys' scale
    emax = float(np.max(np.abs(k0 - ex0)))
    wmed = float(np.median(w0))
    spread = min(1.9 * wmed, max(1.5 * emax, 1e-3 * wmed))
    cand = _nudge_to(cand, qc, metric, 2, kb + rng.uniform(-1.0, 1.0, size=len(cand)) * spread, rng)
    exact = _exact_keys(cand, qc, metric)
    with _open(d, metric, cand) as idx:
        up1, w1 = idx.probe_scan_f16_keys(qc)
    keys = up1.astype(np.float64) - w1 + (qcn2 if metric == L2 else 0.0)
    ratio2 = np.abs(keys - exact) / w1
    print("max |key - exact| / w around the boundary: %.4f" % ratio2.max())
    assert ratio2.max() <= 1.0
    RATIOS.append({"metric": ["l2", "ip"][metric], "dim": d, "max_abs_err_over_w_patterned": float(ratio.max()),
                   "max_abs_err_over_w_boundary": float(ratio2.max())})
    better = np.nonzero((exact < kb) & (exact > kb - spread))[0]
    worse = np.nonzero((exact > kb) & (exact < kb + spread))[0]
    assert len(better) >= 4 * K and len(worse) >= 4 * K
    g = better[np.argsort(-keys[better])[:K]]
    b = worse[np.argsort(keys[worse])[:2 * K]]
    n_total = 40960
    filler = np.stack([_patterned(rng, d, 2, up=bool(i & 1)) for i in range(1024)])
    rows2 = np.tile(filler, (n_total // 1024, 1))[:n_total] * rng.choice([-1.0, 1.0], size=(n_total, d)).astype(np.float32)
    pos = rng.choice(n_total, len(g) + len(b), replace=False)
    pos_g, pos_b = pos[:len(g)], pos[len(g):]
    rows2[pos_g] = cand[g]
    rows2[pos_b] = cand[b]
    assert set(np.argsort(_exact_keys(rows2, qc, metric), kind="stable")[:K].tolist()) == set(pos_g.tolist())
    with _open(d, metric, rows2) as idx:
        c0 = idx.counters()
        upa, wa = idx.probe_scan_f16_keys(qc)
        ka = upa.astype(np.float64) - wa
        inverted = int(np.sum(ka[pos_b] < np.max(ka[pos_g])))
        got = idx.search(qc[None, :], K)
        st, c1 = idx.scan_f16_stats(), idx.counters()
    _same(got, oracle_mod.search_heap_many_mt(rows2, qc[None, :], metric, K))
    assert set(got[0][0].tolist()) == set(pos_g.tolist())
    assert st["scans"] == 1 and st["redone"] == 0 and c1["fallback_searches"] == c0["fallback_searches"]
    assert inverted > 0 or ratio2.max() < 0.02, "the construction did not invert any approximate ranking"


def test_zz_write_band_ratios():
    if RATIOS:
        out = os.path.join(ROOT, "profiles", "scan_f16_band_ratios.json")
        with open(out, "w") as f:
            json.dump(RATIOS, f, indent=1)
            f.write("\n")


@pytest.mark.parametrize("metric", [L2, COS])
def test_crowded_neighbours_are_redone_in_f32(hip_lib, oracle_mod, metric):
    d, k = 768, 100
    rng = np.random.default_rng(77 + metric)
    rows, qs = _corpus(rng, N, d, metric, nq=1)
    if metric == COS:
        qs = np.stack([oracle_mod.normalize_f32(q) for q in qs])
    twin = (qs[0] + 0.05 * rng.standard_normal(d)).astype(np.float32)
    where = np.sort(rng.choice(N, 2000, replace=False))
    rows[where] = twin  # 2 000 identical rows, the query's nearest
    ref = oracle_mod.search_heap_many_mt(rows, qs, metric, k)
    assert np.array_equal(ref[0][0], where[:k])  # ties: the lowest ids first
    with _open(d, metric, rows, mode=0) as idx:  # the f32 path on the same input
        _same(idx.search(qs, k), ref, "f32")
        f32_fallbacks = idx.counters()["fallback_searches"]
    with _open(d, metric, rows) as idx:
        _same(idx.search(qs, k), ref, "fp16")
        st, c = idx.scan_f16_stats(), idx.counters()
    assert st["scans"] == 1 and st["redone"] == 1, st
    assert c["fallback_searches"] == f32_fallbacks, (c, f32_fallbacks)


def test_pipelined_call_equals_single_queries(hip_lib, oracle_mod):
    d, k, metric = 768, 20, IP
    rng = np.random.default_rng(64)
    rows, qs = _corpus(rng, N, d, metric, nq=64)
    with _open(d, metric, rows) as idx:
        many = idx.search(qs, k)
        one = [idx.search(q[None, :], k) for q in qs]
        assert idx.scan_f16_stats() == {"scans": 128, "redone": 0, "rows_converted": N, "copy_bytes": idx.scan_f16_stats()["copy_bytes"]}
    for i in range(3):
        assert np.array_equal(many[i].view(np.uint64) if i == 1 else many[i], np.concatenate([o[i].view(np.uint64) if i == 1 else o[i] for o in one]))
    _same(many, oracle_mod.search_heap_many_mt(rows, qs, metric, k))


def test_copy_that_does_not_fit_degrades_to_f32(hip_lib):
    """With the copy's allocation made to fail (the batched path's hook, in a process of its own) searches are exact on
    the f32 scan and the handle stays usable."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_scan_f16_degrade_worker.py")], cwd=ROOT,
                       env=dict(os.environ, TSH_TEST_FAIL_ALLOC_OVER=str(16 << 20)), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert "degraded ok" in p.stdout, p.stdout
