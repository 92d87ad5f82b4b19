"""GPU: the 4-bit first pass in front of the coarse int8 scan (TSH_OPT_SCAN_I4, tostore_amd/csrc/tsh_scan_i4.hip.h).

A dense L2 scan first reads a plane of the int8 copy's high nibbles and bounds every row's key; the int8 scan then reads
only the rows that bound could not rule out, and the exact path answers as ever -- so answers must stay the oracle's bit
for bit, and the same as with the pass switched off.  Every index here forces the route on small shapes (option 2) and
switches the batched path off.  The survivors the device reports are held to the NumPy model (tests/scan_i4_model.py)."""
import json
import os

import numpy as np
import pytest

import scan_i4_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, IP, COS = 0, 1, 2
N = 20_037  # not a multiple of 64: 314 tiles, the last one ragged
RATIOS = []


def _open(d, metric, rows, capacity=None, i4=2, i8=2):
    from tostore_amd import HipVectorIndex

    idx = HipVectorIndex(d, metric, capacity_rows=capacity or len(rows))
    idx.set_scan_i8(i8)
    idx.set_scan_i8_masked(i8)
    idx.set_scan_i4(i4)
    idx.set_batch_min_nq(0)
    if len(rows):
        idx.append(0, rows)
    return idx


def _same(got, ref, what=""):
    assert np.array_equal(got[2], ref[2]), "counts differ " + what
    assert np.array_equal(got[0], ref[0]), "ids differ " + what
    assert np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), "distance bits differ " + what


def _one_by_one(idx, qs, k):
    """Query by query, so that each scan's survivors can be read from the stats."""
    outs, kept = [], []
    for q in qs:
        s0 = idx.scan_i4_stats()
        outs.append(idx.search(q[None, :], k))
        s1 = idx.scan_i4_stats()
        kept.append((s1["scans"] - s0["scans"], s1["survivors"] - s0["survivors"]))
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(3)), kept


@pytest.mark.parametrize("n,d,ks", [
    (N, 768, (100, 10, 1)),
    (40_000, 100, (10,)),   # a row that ends inside its only group of 32
    (N, 1000, (100,)),      # a part-filled last group
    (8_200, 2048, (100,)),  # the int8 family's widest row; the query no longer rides in the argument segment
])
def test_parity_and_survivors(hip_lib, oracle_mod, n, d, ks):
    rng = np.random.default_rng(100 * d)
    rows, qs = M.spread_corpus(rng, n, d)
    model = M.Shard(rows)
    with _open(d, L2, rows) as idx, _open(d, L2, rows, i4=0) as off:
        for k in ks:
            ref = oracle_mod.search_heap_many_mt(rows, qs, L2, k)
            i8_0 = idx.scan_i8_stats()
            got, kept = _one_by_one(idx, qs, k)
            _same(got, ref, "(oracle) k=%d" % k)
            _same(got, off.search(qs, k), "(option 0) k=%d" % k)
            i8_1 = idx.scan_i8_stats()
            assert i8_1["scans"] - i8_0["scans"] == len(qs) and i8_1["redone"] == i8_0["redone"], (i8_0, i8_1)
            for q, (ran, total) in zip(qs, kept):
                lo, hi = model.survivors(q, k)
                print("n=%d d=%d k=%d: device %d survivors, model %d..%d" % (n, d, k, total, lo, hi))
                assert ran == 1 and lo <= total <= hi, (k, ran, total, lo, hi)
        st = idx.scan_i4_stats()
        assert st["rows_converted"] == n and st["copy_bytes"] >= n * d // 2 and st["denials"] == 0, st
        assert off.scan_i4_stats()["scans"] == 0 and off.scan_i4_stats()["copy_bytes"] == 0


@pytest.mark.parametrize("d", [768, 1000])
def test_band_probe(hip_lib, d):
    """Every row's f64 key lies inside [lower, upper]: a spread corpus, and rows whose every element sits 8 codes off its
    nibble's midpoint with the sign of q_j (the L1 side's worst case)."""
    rng = np.random.default_rng(9400 + d)
    n = 4096
    rows, qs = M.spread_corpus(rng, n, d, nq=1)
    q = qs[0]
    s0 = np.ldexp(1.0, -rng.integers(0, 12, size=n // 2))[:, None]
    nib = rng.integers(1, 15, size=(n // 2, d))
    adv = ((16 * nib + 8 - 128) + np.where(q > 0, 7.49, -7.49)[None, :]) * s0
    adv[np.arange(n // 2), np.arange(n // 2) % d] = 127.0 * s0[:, 0]  # pins every row's scale to its s0
    rows[: n // 2] = adv.astype(np.float32)
    exact = M.Shard(rows).exact_keys(q)
    with _open(d, L2, rows) as idx:
        lo, up = idx.probe_scan_i4_keys(q)
    lo, up = lo.astype(np.float64), up.astype(np.float64)
    ratio = np.abs((lo + up) / 2 - exact) / ((up - lo) / 2)
    print("d=%d: max |key - exact| / w: adversarial rows %.4f, spread rows %.4f" % (d, ratio[: n // 2].max(), ratio[n // 2:].max()))
    RATIOS.append({"dim": d, "max_abs_err_over_w_adversarial": float(ratio[: n // 2].max()),
                   "max_abs_err_over_w_spread": float(ratio[n // 2:].max())})
    assert np.all(np.isfinite(lo)) and np.all(lo <= exact) and np.all(exact <= up), float(ratio.max())
    # the rows' errors are 7.49 of the L1 side's 8.5 codes an element: 0.88 -- a slack band fails too
    assert ratio[: n // 2].max() >= 0.85


def test_fewer_tiles_than_k(hip_lib, oracle_mod):
    """4 100 rows are 65 tiles: k = 100 has fewer live tiles than k (no bound: every row survives A, and B's list of 4 096
    overflows into the f32 redo); k = 64 and 65 bound from nearly every tile; 3 000 rows with k = 100 fit B's list, and
    the survivors' total is every row."""
    d = 768
    rng = np.random.default_rng(5)
    rows, qs = M.spread_corpus(rng, 4_100, d)
    with _open(d, L2, rows) as idx:
        for k in (64, 65, 100):
            _same(idx.search(qs, k), oracle_mod.search_heap_many_mt(rows, qs, L2, k), "k=%d" % k)
    with _open(d, L2, rows[:3_000]) as idx:
        got, kept = _one_by_one(idx, qs, 100)
        _same(got, oracle_mod.search_heap_many_mt(rows[:3_000], qs, L2, 100))
        # (every row survived A twice in a row: the deny rule then keeps the next scans on the plain int8 route)
        assert kept == [(1, 3_000), (1, 3_000), (0, 0), (0, 0)] and idx.scan_i4_stats()["denials"] == 1, kept
    with _open(d, L2, rows[:50]) as idx:  # k larger than the rows
        _same(idx.search(qs, 100), oracle_mod.search_heap_many_mt(rows[:50], qs, L2, 100))


def test_overflow_is_redone(hip_lib, oracle_mod):
    """8 192 copies of one row, the query's nearest: every copy survives A and B, B's list (4 096) overflows and the query
    is redone through the f32 scan, counted by the int8 route."""
    d, k = 768, 100
    rng = np.random.default_rng(77)
    rows, qs = M.spread_corpus(rng, N, d, nq=1)
    twin = (qs[0] + 0.05 * rng.standard_normal(d)).astype(np.float32)
    where = np.sort(rng.choice(N, 8192, replace=False))
    rows[where] = twin
    ref = oracle_mod.search_heap_many_mt(rows, qs, L2, k)
    with _open(d, L2, rows) as idx:
        _same(idx.search(qs, k), ref)
        assert idx.scan_i4_stats()["scans"] == 1 and idx.scan_i8_stats()["redone"] == 1


def test_copy_stays_current(hip_lib, oracle_mod):
    """An append past the watermark, an overwrite and a row with an inf element: the plane follows the int8 copy."""
    d, k = 768, 20
    rng = np.random.default_rng(31)
    rows, qs = M.spread_corpus(rng, 17_000, d)
    n0, n1 = 12_000, 17_000
    with _open(d, L2, rows[:n0], capacity=18_048) as idx:
        def check(n, what, fresh, ran=True):
            s0 = idx.scan_i4_stats()
            _same(idx.search(qs, k), oracle_mod.search_heap_many_mt(rows[:n], qs, L2, k), what)
            s1 = idx.scan_i4_stats()
            assert s1["scans"] - s0["scans"] == (len(qs) if ran else 0), (what, s0, s1)
            assert s1["rows_converted"] - s0["rows_converted"] == fresh, (what, s0, s1)

        check(n0, "at first", n0)
        idx.append(n0, rows[n0:n1])
        check(n1, "after an append", n1 - n0)
        r = 4321
        rows[r] = (qs[1] + 0.01 * rng.standard_normal(d)).astype(np.float32)
        idx.append(r, rows[r:r + 1])
        check(n1, "after an overwrite", n1)
        rows[77, 5] = np.inf  # quarantined: the shard is no longer dense
        idx.append(77, rows[77:78])
        check(n1, "with a quarantined row", 0, ran=False)


def test_unit_rows_are_denied(hip_lib, oracle_mod):
    """Unit-norm rows: A prunes nothing (the model says so: test_host_scan_i4_model.py).  Two scans, then the route is
    denied and the next scans take the plain int8 route; answers equal throughout."""
    d, k = 768, 100
    rng = np.random.default_rng(100 * d)
    rows, qs = M.unit_corpus(rng, N, d)
    ref = oracle_mod.search_heap_many_mt(rows, qs, L2, k)
    with _open(d, L2, rows) as idx:
        got, kept = _one_by_one(idx, qs, k)
        _same(got, ref)
        st = idx.scan_i4_stats()
        assert [r for r, _ in kept] == [1, 1, 0, 0] and st["denials"] == 1 and st["denied_left"] == 254, (kept, st)
        assert all(t > M.MAX_SHARE * N for _, t in kept[:2]), kept
        assert idx.scan_i8_stats()["scans"] == 4 and idx.scan_i8_stats()["redone"] == 0


def test_unit_rows_are_denied_once_by_a_pipelined_call(hip_lib, oracle_mod):
    """The same corpus, eight queries in ONE call: several scans are in flight when the second one over the share is seen.
    The scans that finish after the denial fell count as scans and nothing else -- one denial of 256, not a doubled one --
    and the next call's four queries each use one of them up."""
    d, k = 768, 100
    rng = np.random.default_rng(100 * d)
    rows, _ = M.unit_corpus(rng, N, d)
    qs = rng.standard_normal((12, d)).astype(np.float32)
    ref = oracle_mod.search_heap_many_mt(rows, qs, L2, k)
    with _open(d, L2, rows) as idx:
        _same(idx.search(qs[:8], k), tuple(x[:8] for x in ref))
        st = idx.scan_i4_stats()
        assert 2 <= st["scans"] <= 8 and st["denials"] == 1 and st["denied_left"] == 256 - (8 - st["scans"]), st
        _same(idx.search(qs[8:], k), tuple(x[8:] for x in ref))
        s2 = idx.scan_i4_stats()
        assert s2["scans"] == st["scans"] and s2["denials"] == 1 and s2["denied_left"] == st["denied_left"] - 4, (st, s2)


def test_route_not_taken(hip_lib, oracle_mod):
    """Inner product, cosine, a caller's mask and a tombstone: the 4-bit pass does not run and its stats stay put."""
    d, k = 768, 10
    rng = np.random.default_rng(8)
    rows, qs = M.spread_corpus(rng, N, d)
    for metric in (IP, COS):
        with _open(d, metric, rows) as idx:
            q = np.stack([oracle_mod.normalize_f32(x) for x in qs]) if metric == COS else qs
            _same(idx.search(q, k), oracle_mod.search_heap_many_mt(rows, q, metric, k))
            assert idx.scan_i4_stats() == {"scans": 0, "survivors": 0, "rows_converted": 0, "copy_bytes": 0, "denials": 0, "denied_left": 0}
            assert idx.scan_i8_stats()["scans"] == len(qs)
    with _open(d, L2, rows) as idx:
        keep = rng.random(N) < 0.7
        got = idx.search(qs, k, row_mask=np.packbits(keep, bitorder="little"))
        sub = np.flatnonzero(keep)
        ref = oracle_mod.search_heap_many_mt(rows[sub], qs, L2, k)
        assert np.array_equal(got[0], sub[ref[0]]) and np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64))
        assert idx.scan_i4_stats()["scans"] == 0
        idx.set_deleted([5])
        live = np.delete(np.arange(N), 5)
        ref = oracle_mod.search_heap_many_mt(rows[live], qs, L2, k)
        got = idx.search(qs, k)
        assert np.array_equal(got[0], live[ref[0]]) and np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64))
        assert idx.scan_i4_stats()["scans"] == 0 and idx.scan_i4_stats()["copy_bytes"] == 0


def test_zz_write_band_ratios():
    """Appends this run's worst ratios to the record."""
    if not RATIOS:
        return
    path = os.path.join(ROOT, "profiles", "scan_i4_band_ratios.json")
    try:
        with open(path) as f:
            record = json.load(f)
    except (OSError, ValueError):
        record = []
    record.append({"worst": max(max(r["max_abs_err_over_w_adversarial"], r["max_abs_err_over_w_spread"]) for r in RATIOS), "cases": RATIOS})
    with open(path, "w") as f:
        json.dump(record[-20:], f, indent=1)
        f.write("\n")
