"""GPU: every width of the f32, fp16 and int8 tile scans against the oracle and against f64 keys.

The single-query tile scan is one skeleton (tsh_scan_tile.inc.h) instantiated per row store, chunk count (NCH = 1-8,
10, 12, 14, 16; fp16 up to 14, int8 up to 8), FULL or ragged rows, dense or MASKED, and metric.  The width list --
tests/golden/scan_width_sweep.json, which tests/test_host_scan_widths.py holds to the set of instantiations the
dispatch can reach -- has per chunk count the full width, a row that ends 72 elements into its last chunk (fp16-eligible),
one that ends 101 elements into it (ld rounds up: three pad elements inside the row), from ten chunks on a row that
leaves a whole chunk of its kernel empty, and the four packed-row widths (d = 30, 32, 64, 128: the f32 packed kernel,
and the int8 tile scan on 8 / 16 / 32 lanes).  Each width is one test; inside it, per metric and for a dense and a
tombstoned shard, every family that serves the width is held to

  (a) the oracle: counts, ids and distance bits of 4 queries at k = 10, the route's own counter advancing by the
      number of queries, nothing redone, no wide-band fallback;
  (b) its key probe against f64 keys of the same operation, on EVERY live row: the f32 key within the claimed bound
      (as tests/test_gpu_bands.py forms it), |stored - w - exact| <= w for fp16, lower <= exact <= upper for int8;
      dead rows are NaN (fp16, int8);
  (c) the same probes on adversarial rows of the same shape: operands at fp16 rounding midpoints / plain f32 patterns
      for the fp16 and f32 scans, rows at int8 quantisation midpoints for the int8 scan.

The corpus is 16 tiles and one of 37 rows, capacity = rows, so the last tile is ragged and the copies end at the last
tile.  The tombstones leave tiles with 0, 1, 7, 8, 9, 15, 16, 17, 33, 63 and 64 live rows and a partly deleted last
tile -- the edges of the 8-row batches and of the masked pipeline's two groups per batch -- and kill every query's
nearest row.

"Nothing redone" is a property of the inputs, not of the code under test:
  int8   the survivor list holds I8_LIST_CAP = 4096 rows and the shard has 1061: it cannot overflow.
  fp16   the candidate block of k = 10 holds tsh_default_block_entries(10) = 192 entries.  The select emits a row when
         its lower side is at or below the k-th smallest tile minimum of upper sides plus the uniform 2 w_max: with
         every key within w <= w_max of its exact value, only rows whose EXACT key is at or below the tenth smallest
         exact tile minimum + 4 w_max can be emitted.  That count is taken here on the CPU from f64 keys, with w_max from
         tsh_scan_f16_band.h itself (compiled by g++: tests/cpp/scan_f16_band_lib.cpp), and asserted to stay below half
         the block for every width, metric and query before the search runs.  (So that the tombstoned shard has ten
         tiles with a low minimum, the tiles left with 15 or more live rows keep each query's best row of the tile.)

The worst |key - exact| / w per family, width, metric and dense / masked goes to profiles/scan_width_sweep.json: the
assertion is soundness (ratio <= 1), the file is the record of tightness.

Out of scope here: the big-shard launch shapes (6144 tiles and more: several waves per workgroup, more than one tile
per wave) -- they need 400 MB indexes and are covered at d = 256 by the test_big_shard_launch_shape(s) tests; every
shard here runs one-wave workgroups, one tile per wave.  scan_list_kernel is test_selective_masks_every_width's; the
batched path's key kernels have a sweep of their own, tests/test_gpu_batch_shapes.py."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from test_gpu_bands import _exact_keys, _patterned

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, IP, COS = 0, 1, 2
METRIC_NAMES = ("l2", "ip", "cosine")
SCAN = -1
TILE = 64
N = 16 * TILE + 37
NQ, K = 4, 10
NCHS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16)
LIVE_COUNTS = (64, 63, 33, 17, 16, 15, 9, 8, 7, 1, 0)  # per tile, beside a partly deleted last tile
WIDTHS = json.load(open(os.path.join(ROOT, "tests", "golden", "scan_width_sweep.json")))
RESULTS = {}


def _nch(d):
    need = ((d + 3) // 4 + 63) // 64
    return min(o for o in NCHS if o >= need)


def _families(d):
    fam = ["f32"]
    if d >= 256 and d % 8 == 0 and _nch(d) <= 14:
        fam.append("fp16")
    if _nch(d) <= 8:
        fam.append("int8")
    return fam


def _bits(keep):
    return np.packbits(np.asarray(keep, bool), bitorder="little")


@pytest.fixture(scope="module")
def f16_band(tmp_path_factory):
    """(metric, q, rows) -> w_max of tsh_scan_f16_band.h for the shard's norm bounds, by the header itself."""
    so = tmp_path_factory.mktemp("scan_f16_band") / "libscan_f16_band.so"
    src = os.path.join(ROOT, "tests", "cpp", "scan_f16_band_lib.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), src], check=True)
    lib = ctypes.CDLL(str(so))
    fp = ctypes.POINTER(ctypes.c_float)
    lib.scan_f16_band_of.restype = ctypes.c_int
    lib.scan_f16_band_of.argtypes = [ctypes.c_int, ctypes.c_int, fp, ctypes.c_float, ctypes.c_float, ctypes.c_float, fp]

    def w_max(metric, q, rows):
        nrm = np.sqrt(np.einsum("ij,ij->i", rows.astype(np.float64), rows.astype(np.float64)))
        mx = np.nextafter(np.float32(nrm.max()), np.float32(np.inf))  # (bounds, as the ingest pass keeps them: outwards)
        mn = np.nextafter(np.float32(nrm.min()), np.float32(0))
        q = np.ascontiguousarray(q, np.float32)
        out = (ctypes.c_float * 3)()
        ok = lib.scan_f16_band_of(metric, q.shape[0], q.ctypes.data_as(fp), float(mx), float(mn), float(np.abs(rows).max()), out)
        assert ok == 1
        return float(out[2])

    return w_max


def _gaussian(rng, d, metric, normalize):
    rows = rng.standard_normal((N, d), dtype=np.float32)
    if metric != COS:
        rows *= rng.uniform(0.5, 2.0, size=(N, 1)).astype(np.float32)
    qs = rng.standard_normal((NQ, d), dtype=np.float32)
    if metric == COS:
        qs = np.stack([normalize(q) for q in qs])
    return rows, qs


def _tombstones(rng, exact):
    """live[] over the N rows.  exact: f64 keys [NQ, N].  Every query's nearest row dies; eleven tiles are left with
    LIVE_COUNTS live rows, none of them a nearest row, and from 15 live rows on each query's best other row of the tile
    among them (module docstring: the fp16 candidate count); the other whole tiles lose the nearest rows and a few
    more; the last, partial tile loses about half of its rows."""
    nearest = np.unique(np.argmin(exact, axis=1))
    live = np.ones(N, bool)
    n_near = np.array([np.sum(nearest // TILE == t) for t in range(N // TILE)])
    order = sorted(range(N // TILE), key=lambda t: (n_near[t], rng.random()))  # the 64-row tile holds no nearest row
    counts = dict(zip(order, LIVE_COUNTS))
    for t in range(N // TILE):
        ids = np.arange(t * TILE, (t + 1) * TILE)
        cand = np.setdiff1d(ids, nearest)
        if t not in counts:
            live[rng.choice(cand, 3, replace=False)] = False
            continue
        live[ids] = False
        keep = []
        if counts[t] >= 15:
            masked = np.where(np.isin(ids, nearest)[None, :], np.inf, exact[:, ids])
            keep = list(np.unique(ids[np.argmin(masked, axis=1)]))
        rest = np.setdiff1d(cand, keep)
        keep += list(rng.choice(rest, counts[t] - len(keep), replace=False))
        live[keep] = True
    tail = np.setdiff1d(np.arange((N // TILE) * TILE, N), nearest)
    live[rng.choice(tail, len(tail) // 2, replace=False)] = False
    live[nearest] = False
    per_tile = [int(live[t * TILE:(t + 1) * TILE].sum()) for t in range(N // TILE)]
    assert set(LIVE_COUNTS) <= set(per_tile), per_tile
    assert 0 < live[(N // TILE) * TILE:].sum() < N % TILE
    assert sum(c > 0 for c in per_tile) + 1 >= K  # live tiles: a threshold exists
    return live


def _f16_candidates(exact, live, w_max):
    """Per query, the rows the fp16 select can emit at most: live rows whose exact key is at or below the K-th smallest
    exact minimum of the live tiles + 4 w_max (module docstring)."""
    out = []
    for e in exact:
        e = np.where(live, e, np.inf)
        mins = np.sort([e[t * TILE:(t + 1) * TILE].min() for t in range((N + TILE - 1) // TILE)])
        assert np.isfinite(mins[K - 1])
        out.append(int(np.sum(e <= mins[K - 1] + 4.0 * w_max * 1.001)))  # (1.001: the select's own f32 roundings)
    return out


def _reduced(exact, q, metric):
    """The reduced scans' L2 key leaves the common |q|^2 out."""
    q64 = q.astype(np.float64)
    return exact - (q64 @ q64 if metric == L2 else 0.0)


def _set_route(idx, family):
    idx.set_scan_f16(2 if family == "fp16" else 0)
    idx.set_scan_f16_masked(2 if family == "fp16" else 0)
    idx.set_scan_i8(2 if family == "int8" else 0)
    idx.set_scan_i8_masked(2 if family == "int8" else 0)


def _open(d, metric, rows):
    from tostore_amd import HipVectorIndex

    idx = HipVectorIndex(d, metric, capacity_rows=len(rows))
    idx.set_batch_min_nq(0)
    idx.set_exact_scan_rows(0)
    idx.append(0, rows)
    return idx


def _check(fails, cond, msg):
    """Every miss of a width is reported, not the first alone: test_width asserts on the list at its end."""
    if not cond:
        fails.append(msg)
    return bool(cond)


def _probe_ratio(idx, family, q, metric, exact, live, what, fails):
    """Check (b) for one query: the worst |key - exact| / w over the live rows, held to <= 1.  exact: the f64 keys of
    _exact_keys (|q|^2 included for L2)."""
    dead = ~live
    if family == "f32":
        keys, eps_rel, delta_abs = idx.probe_scan_keys(q)
        mid = keys.astype(np.float64)
        w = (eps_rel / 3.0) * np.abs(exact) + delta_abs if metric == L2 else np.full(N, delta_abs / 2.0 / 1.0001)
        ex = exact
    elif family == "fp16":
        up, w = idx.probe_scan_f16_keys(q)
        up, w = up.astype(np.float64), w.astype(np.float64)
        _check(fails, np.all(np.isnan(up[dead])), what + ": a dead row has a key")
        _check(fails, np.all(np.isfinite(w[live])) and np.all(w[live] > 0), what + ": a band that is not positive and finite")
        mid = up - w
        ex = _reduced(exact, q, metric)
    else:
        lo, up = idx.probe_scan_i8_keys(q)
        lo, up = lo.astype(np.float64), up.astype(np.float64)
        _check(fails, np.all(np.isnan(lo[dead])) and np.all(np.isnan(up[dead])), what + ": a dead row has a key")
        mid, w = (lo + up) / 2, (up - lo) / 2
        ex = _reduced(exact, q, metric)
        if np.all(np.isfinite(lo[live])) and np.all(np.isfinite(up[live])):  # the claim itself, not its rounded midpoint
            _check(fails, np.all(lo[live] <= ex[live]) and np.all(ex[live] <= up[live]), what + ": an exact key outside [lower, upper]")
    if not _check(fails, np.all(np.isfinite(mid[live])), what + ": a live row's key is not finite"):
        return float("inf")
    worst = float(np.max(np.abs(mid[live] - ex[live]) / w[live]))
    print("%s: max |key - exact| / w = %.4f" % (what, worst))
    if family != "int8":  # (int8: held above, side by side -- the midpoint of two f32 sides rounds)
        _check(fails, worst <= 1.0, "%s: a key is further from its exact value than its bound: %.4f" % (what, worst))
    return worst


def _parity(got, ref, what, fails):
    """counts, ids and distance bits of a search are the oracle's"""
    _check(fails, np.array_equal(got[2], ref[2]), what + ": counts differ from the oracle's")
    _check(fails, np.array_equal(got[0], ref[0]), what + ": ids differ from the oracle's")
    _check(fails, np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), what + ": distance bits differ from the oracle's")


def _search(idx, family, qs, ref, what, fails):
    """Check (a)."""
    f0, i0, c0 = idx.scan_f16_stats(), idx.scan_i8_stats(), idx.counters()
    got = idx.search(qs, K)
    f1, i1, c1 = idx.scan_f16_stats(), idx.scan_i8_stats(), idx.counters()
    _parity(got, ref, what, fails)
    _check(fails, f1["scans"] - f0["scans"] == (len(qs) if family == "fp16" else 0), "%s: fp16 scans %s -> %s" % (what, f0, f1))
    _check(fails, i1["scans"] - i0["scans"] == (len(qs) if family == "int8" else 0), "%s: int8 scans %s -> %s" % (what, i0, i1))
    _check(fails, f1["redone"] == f0["redone"] and i1["redone"] == i0["redone"], "%s: a query was redone: %s -> %s, %s -> %s" % (what, f0, f1, i0, i1))
    _check(fails, c1["fallback_searches"] == c0["fallback_searches"], what + ": a query took the wide-band fallback")


def _record(family, d, metric, key, ratio):
    e = RESULTS.setdefault((family, d, metric), {"family": family, "dim": d, "nch": _nch(d), "metric": METRIC_NAMES[metric]})
    e[key] = round(max(ratio, e.get(key, 0.0)), 4)


def _adversarial(rng, d, normalize):
    """Check (c)'s corpora, shared by the metrics: name -> (families probed, rows, query).  fp16 / f32: positive operands
    just below / above fp16's rounding midpoints (every rounding of a row errs one way), norms over a factor 16; f32:
    plain f32 patterns; int8: codes +/- 1/2 with every error of the sign of its q_j, one element at 127 s0 pinning the
    row's scale."""
    out = {}
    scale = np.ldexp(1.0, -rng.integers(0, 5, size=N)).astype(np.float32)[:, None]
    up = (np.arange(N) & 1).astype(bool)[:, None]
    out["fp16 midpoints"] = (("fp16", "f32"), np.where(up, _patterned(rng, (N, d), 2, True), _patterned(rng, (N, d), 2, False)) * scale,
                             _patterned(rng, d, 2, up=False))
    out["f32 patterns"] = (("f32",), _patterned(rng, (N, d), SCAN, False) * scale, _patterned(rng, d, SCAN, up=False))
    q = rng.standard_normal(d).astype(np.float32)
    s0 = np.ldexp(1.0, -rng.integers(0, 12, size=N))[:, None]
    rows = (2.0 * rng.integers(-63, 63, size=(N, d)) + np.where(q > 0, 0.5, -0.5)[None, :]) * s0
    rows[np.arange(N), np.arange(N) % d] = 127.0 * s0[:, 0]
    assert np.array_equal(rows.astype(np.float32).astype(np.float64), rows)
    out["int8 midpoints"] = (("int8",), rows.astype(np.float32), q)
    return out


@pytest.mark.parametrize("d", WIDTHS)
def test_width(hip_lib, oracle_mod, f16_band, d):
    rng = np.random.default_rng(7000 + d)
    families = _families(d)
    fails = []
    adversarial = _adversarial(rng, d, oracle_mod.normalize_f32)
    for metric in (L2, IP, COS):
        name = "d=%d %s" % (d, METRIC_NAMES[metric])
        rows, qs = _gaussian(rng, d, metric, oracle_mod.normalize_f32)
        exact = np.stack([_exact_keys(rows, q, metric) for q in qs])
        live = _tombstones(rng, exact)
        all_live = np.ones(N, bool)
        assert not live[np.argmin(exact, axis=1)].any()
        ref = {False: oracle_mod.search_heap_many_mt(rows, qs, metric, K),
               True: oracle_mod.search_heap_many_mt(rows, qs, metric, K, None, _bits(live))}
        assert not np.isin(ref[True][0], np.argmin(exact, axis=1)).any()
        if "fp16" in families:  # nothing can be redone: a property of these inputs
            cap = hip_lib.tsh_default_block_entries(K)
            assert cap == 192
            for masked, lv in ((False, all_live), (True, live)):
                for i, q in enumerate(qs):
                    n_cand = _f16_candidates(exact[i:i + 1], lv, f16_band(metric, q, rows))[0]
                    print("%s query %d%s: at most %d fp16 candidates" % (name, i, ", tombstoned" if masked else "", n_cand))
                    assert n_cand < cap // 2, (name, i, masked, n_cand)
        with _open(d, metric, rows) as idx:
            for masked, lv in ((False, all_live), (True, live)):
                if masked:
                    idx.set_deleted(np.nonzero(~live)[0])
                for family in families:
                    what = "%s %s%s" % (name, family, ", tombstoned" if masked else "")
                    _set_route(idx, family)
                    _search(idx, family, qs, ref[masked], what, fails)
                    worst = max(_probe_ratio(idx, family, q, metric, exact[i], lv, what, fails) for i, q in enumerate(qs))
                    _record(family, d, metric, "masked" if masked else "dense", worst)
        for corpus, (fams, arows, aq) in adversarial.items():
            fams = [f for f in fams if f in families]
            if not fams:
                continue
            aq = oracle_mod.normalize_f32(aq) if metric == COS else aq
            aexact = _exact_keys(arows, aq, metric)
            alive = _tombstones(rng, np.stack([aexact]))
            with _open(d, metric, arows) as idx:
                for masked, lv in ((False, all_live), (True, alive)):
                    if masked:
                        idx.set_deleted(np.nonzero(~alive)[0])
                    for family in fams:
                        what = "%s %s on %s%s" % (name, family, corpus, ", tombstoned" if masked else "")
                        _set_route(idx, family)
                        worst = _probe_ratio(idx, family, aq, metric, aexact, lv, what, fails)
                        _record(family, d, metric, ("masked" if masked else "dense") + "_adversarial", worst)
    assert not fails, "%d checks missed:\n%s" % (len(fails), "\n".join(fails))


def test_zz_write_width_sweep():
    """(runs last in this file) the measured ratios of a whole sweep, for profiles/scan_width_sweep.json"""
    if {d for (_, d, _) in RESULTS} != set(WIDTHS):
        return  # (a part of the sweep ran: the record of the whole one stays)
    out = [RESULTS[key] for key in sorted(RESULTS, key=lambda x: (("f32", "fp16", "int8").index(x[0]), x[1], x[2]))]
    assert max(max(v for v in e.values() if isinstance(v, float)) for e in out) <= 1.0
    with open(os.path.join(ROOT, "profiles", "scan_width_sweep.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in out) + "\n]\n")
