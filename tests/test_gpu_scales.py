"""GPU: the scan and key kernels against the oracle and against f64 keys far from unit magnitude.

Every band of a ranking kernel has terms that scale with the data and terms that do not (the fp16 scan's sub = 2^(-14 -
v_exp) and under, the int8 scan's scale floor, the f32 scan's d 7.9e-31 / d 7.5e-37, the batched planes' 2^v_exp / 2^q_exp
and dot_scale, the +-55 guards, the 1e15 and 2^-50 quarantine lines); the host arithmetic of those bands is swept over
wide ranges by tests/cpp/*_band_test.cpp, the device kernels were only ever run on elements of order 1.  Here the corpora
of tests/scale_inputs.py -- rows times 2^er, queries times 2^eq, er = eq from -118 to 46, five mismatched pairs, and
`mixed`, norms 2^30 apart inside one shard -- go through every family; what may be demanded of each case is worked out on
the CPU (scale_inputs.facts, asserted by tests/test_host_scale_inputs.py).  Cosine queries are unit vectors, as the ABI
requires (_normalizeFloat32): queries that are not are outside the contract and not tested.

test_scale[case-d], per metric, on a dense shard and a tombstoned one (every query's nearest row dead), per family of the
width (f32, fp16, int8, forced with mode 2):
  (a) parity, always: counts, ids and distance bits are the oracle's run on the scaled inputs -- at the refused and
      swamped scales, on the all-quarantined cosine shard (safe mode) and with subnormal keys too;
  (b) the route, where the table says "demanded": the family's scans advance by the number of queries, nothing is redone,
      no wide-band fallback (test_gpu_scan_widths._search as it stands); "refused" (fp16): the scans counter does not
      move and the probe refuses as well; "free": only (a), the counters are recorded;
  (c) wherever the route ran, its keys against f64 keys of the scaled f32 inputs on every live row, in absolute terms
      (test_gpu_scan_widths._probe_ratio as it stands: f32 within its bound, |stored - w - exact| <= w for fp16, lower <=
      exact <= upper for int8, dead rows NaN, every live key and band finite, the band positive).  The reduced scans' L2
      key is handed over as |v|^2 - 2 q.v summed in f64 (scale_inputs.reduced_keys), under the metric argument of a key
      that leaves nothing out: |q - v|^2 - |q|^2 cancels to nothing in f64 when the query is 2^40 above the rows.
test_scale_batched[case] (d = 768, a shard of 4096 + 256 + 37 rows: smaller shards are not batched), per metric and key
kernel (f32 MFMA, bf16x3, fp16; set_batch_min_nq(2)), dense and tombstoned (every query's nearest row dead, and rows at
the edges of 64-, 128- and 256-row units): search() equals the oracle bit for bit; the queries answered alone -- the
single-query launches the call made -- are exactly the ones the plan drops wherever the CPU count of candidates says
no list can overflow, and at least those elsewhere; the kernel that ran is
the one tsh_batch_plan.h predicts (a forced fp16 turns into bf16x3 where f16_scale_exp refuses the rows' scale); the
queries the plan keeps have all their probe_batch_keys keys within the claimed bound (test_gpu_batch_shapes._probe: per
row 2 |key - exact| <= alpha2 |v| + beta2 for fp16 keys of L2 / inner product, the uniform d2 otherwise); the queries the
batch drops as bad -- the query-side scale guard included -- are answered alone and are part of the parity check.
test_mixed_query_magnitudes_in_one_batch: four queries at 2^0 and four at 2^-12 of them in one call: the fp16 kernel
drops the small ones (top_q / 256) and they are redone alone; all eight equal the oracle.
test_downstream[er] (-38, 0, 46; the f32 route): the second page of search_after from the first page's last (distance,
id), and search_count under the oracle's 40th distance, against the oracle's full ordered list.

The worst ratio per (family or kernel, case, metric, dense / masked) and the route actually taken go to
profiles/scale_sweep.json: the assertion is soundness (ratio <= 1), the file is the record of tightness.  No tolerance
is chosen here: every comparison is bit equality with the oracle or the library's own claimed bound."""
import json
import os

import numpy as np
import pytest

import scale_inputs as si
from scale_inputs import COS, IP, K, L2, METRIC_NAMES, N
from test_gpu_batch_shapes import KERNEL_NAMES
from test_gpu_batch_shapes import _open as _open_batch
from test_gpu_batch_shapes import _probe as _probe_batch
from test_gpu_scan_widths import _bits, _check, _families, _open, _parity, _probe_ratio, _search, _set_route

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULTS = {}
RAN = set()


def _oracle(oracle_mod, rows, qs, metric, live=None):
    return oracle_mod.search_heap_many_mt(rows, qs, metric, K, None, None if live is None else _bits(live))


def _taken(f0, f1, i0, i1, c0, c1):
    """the route a call of searches took, from the counters it moved"""
    parts = [name + " x%d" % (b[key] - a[key]) for name, a, b, key in (("fp16", f0, f1, "scans"), ("int8", i0, i1, "scans"),
             ("fp16 redone", f0, f1, "redone"), ("int8 redone", i0, i1, "redone"), ("wide-band fallback", c0, c1, "fallback_searches"),
             ("exact scan", c0, c1, "exact_scans")) if b[key] != a[key]]
    return ", ".join(parts) if parts else "f32"


def _searched(idx, family, route, qs, ref, what, fails):
    """(a) always; (b) where the table demands or refuses.  Returns the route taken."""
    f0, i0, c0 = idx.scan_f16_stats(), idx.scan_i8_stats(), idx.counters()
    if route == "demanded":
        _search(idx, family, qs, ref, what, fails)
    else:
        _parity(idx.search(qs, K), ref, what, fails)
    f1, i1, c1 = idx.scan_f16_stats(), idx.scan_i8_stats(), idx.counters()
    if route == "refused" and family == "fp16":
        _check(fails, f1["scans"] == f0["scans"], "%s: the fp16 scan ran where the header refuses: %s -> %s" % (what, f0, f1))
    taken = _taken(f0, f1, i0, i1, c0, c1)
    print("%s: table says %s, took %s" % (what, route, taken))
    return taken


def _probed(idx, family, expect, q, metric, exact, reduced, live, what, fails):
    """(c) for one query: the worst ratio, None where the route does not run (and must not: `expect`)"""
    from tostore_amd._ffi import TshError

    try:
        if family == "f32":
            return _probe_ratio(idx, family, q, metric, exact, live, what, fails)
        if family == "int8":  # (the band positive: _probe_ratio divides by it)
            lo, up = idx.probe_scan_i8_keys(q)
            _check(fails, np.all(up[live] > lo[live]), what + ": a band that is not positive")
        return _probe_ratio(idx, family, q, IP if metric == L2 else metric, reduced, live, what, fails)
    except TshError as e:
        _check(fails, not expect, "%s: the probe refused a query inside the model: %s" % (what, e))
        return None


def _record(kind, name, d, case, metric, **kw):
    e = RESULTS.setdefault((kind, name, d, case, metric), {"kind": kind, "name": name, "dim": d, "case": case, "metric": METRIC_NAMES[metric]})
    for key, v in kw.items():
        if isinstance(v, float):
            v = round(max(v, e.get(key) or 0.0), 4)
        e[key] = v


@pytest.mark.parametrize("d", si.WIDTHS)
@pytest.mark.parametrize("case", si.CASES)
def test_scale(hip_lib, oracle_mod, case, d):
    fails = []
    for metric in (L2, IP, COS):
        if metric == COS and not si.cosine_runs(case):
            continue
        f = si.facts(d, case, metric)
        name = "d=%d %s %s" % (d, case, METRIC_NAMES[metric])
        all_live = np.ones(N, bool)
        ref = {False: _oracle(oracle_mod, f.rows, f.qs, metric), True: _oracle(oracle_mod, f.rows, f.qs, metric, f.live)}
        with _open(d, metric, f.rows) as idx:
            c = idx.counters()
            _check(fails, bool(c["safe_mode"]) == f.safe and c["quarantined_rows"] == min(f.n_irregular, si.QUARANTINE_MAX),
                   "%s: safe mode %d, %d rows quarantined; the rules give %s, %d" % (name, c["safe_mode"], c["quarantined_rows"], f.safe, f.n_irregular))
            for masked, lv in ((False, all_live), (True, f.live)):
                if masked:
                    idx.set_deleted(np.nonzero(~f.live)[0])
                tag = "masked" if masked else "dense"
                for family in _families(d):
                    what = "%s %s%s" % (name, family, ", tombstoned" if masked else "")
                    route = f.routes[masked][family]
                    _set_route(idx, family)
                    taken = _searched(idx, family, route, f.qs, ref[masked], what, fails)
                    ratios = []
                    for i, q in enumerate(f.qs):
                        expect = not f.safe and (family == "f32" or (family == "int8" and f.i8_ok[i]) or
                                                 (family == "fp16" and f.f16_exp_ok and f.f16_ok[i]))
                        r = _probed(idx, family, expect, q, metric, f.exact[i], f.reduced[i], lv, what, fails)
                        _check(fails, expect or r is None, what + ": the probe ran where the header (or safe mode) refuses")
                        _check(fails, not expect or r is not None, what + ": no keys to hold to their bound")
                        if r is not None:
                            ratios.append(r)
                    _record("scan", family, d, case, metric, **{"table_" + tag: route, "taken_" + tag: taken,
                                                                 tag: float(max(ratios)) if ratios else None})
    RAN.add(("scan", case, d))
    assert not fails, "%d checks missed:\n%s" % (len(fails), "\n".join(fails))


def _batched(idx, kernel, f, qs, bad, quiet, live, ref, what, fails):
    """search() of one batched call against the oracle; the kernel the plan predicts; the queries answered alone (the
    single-query launches: exactly the ones the plan drops where `quiet` -- the CPU count says no list can overflow --,
    at least those otherwise); then the kept queries' keys on the live rows.  Returns (what ran, as observed; worst ratio)."""
    c0 = idx.counters()
    got = idx.search(qs, K)
    c1 = idx.counters()
    _parity(got, ref, what, fails)
    kern, n_bad = f.kern[kernel], int(bad.sum())
    moved = {key: c1[key] - c0[key] for key in ("batch_launches", "scan_launches", "fallback_searches", "batch_scan_fallbacks", "exact_scans")}
    alone = moved["scan_launches"]
    took = "safe mode: %d single-query launches" % alone if f.safe else \
        "%s, %d of %d queries answered alone (%d dropped by the plan)" % (KERNEL_NAMES[c1["batch_kernel_last"]], alone, len(qs), n_bad)
    print("%s: %s; counters moved %s" % (what, took, moved))
    if f.safe:
        _check(fails, moved["batch_launches"] == 0 and alone == len(qs), what + ": a batched call in safe mode, or a query not answered alone")
        return took, None
    _check(fails, moved["batch_launches"] > 0 and c1["batch_kernel_last"] == kern,
           "%s: the plan says %s, %s ran (%d launches)" % (what, KERNEL_NAMES[kern], KERNEL_NAMES[c1["batch_kernel_last"]], moved["batch_launches"]))
    _check(fails, alone == n_bad if quiet else n_bad <= alone <= len(qs),
           "%s: %d queries answered alone, the plan drops %d%s" % (what, alone, n_bad, " and no list can overflow" if quiet else ""))
    if bad.all():
        return took, None
    exact = si.bsi.exact_keys_many(f.rows, qs[~bad], f.metric)
    nrm = np.sqrt(np.einsum("ij,ij->i", f.rows.astype(np.float64), f.rows.astype(np.float64)))
    return took, _probe_batch(idx, kern, f.metric, qs[~bad], exact, nrm, live, what, fails)


def _batched_both(oracle_mod, f, kernel, qs, bad, quiet, case, what, fails):
    """a dense pass and a tombstoned one (every query's nearest row dead) of one index"""
    ref = {False: _oracle(oracle_mod, f.rows, qs, f.metric), True: _oracle(oracle_mod, f.rows, qs, f.metric, f.live)}
    with _open_batch(768, f.metric, f.rows, kernel) as idx:
        for masked, live in ((False, np.ones(len(f.rows), bool)), (True, f.live)):
            if masked:
                idx.set_deleted(np.nonzero(~f.live)[0])
            tag = "masked" if masked else "dense"
            took, worst = _batched(idx, kernel, f, qs, bad, quiet[masked], live, ref[masked], what + (", tombstoned" if masked else ""), fails)
            _record("batch", KERNEL_NAMES[kernel], 768, case, f.metric, **{"taken_" + tag: took, tag: worst})


@pytest.mark.parametrize("case", si.CASES)
def test_scale_batched(hip_lib, oracle_mod, case):
    fails = []
    for metric in (L2, IP, COS):
        if metric == COS and not si.cosine_runs(case):
            continue
        f = si.batch_facts(case, metric)
        assert not f.live[np.argmin(f.exact, axis=1)].any()
        for kernel in (0, 1, 2):
            quiet = {m: f.candidates[kernel, m] < f.half_cap for m in (False, True)}
            _batched_both(oracle_mod, f, kernel, f.qs, f.bad[kernel], quiet, case, "batched %s %s %s" % (case, METRIC_NAMES[metric], KERNEL_NAMES[kernel]), fails)
    RAN.add(("batch", case, 768))
    assert not fails, "%d checks missed:\n%s" % (len(fails), "\n".join(fails))


@pytest.mark.parametrize("metric", [L2, IP])
def test_mixed_query_magnitudes_in_one_batch(hip_lib, oracle_mod, metric):
    f = si.batch_facts("0,0", metric)
    qs = f.qs.copy()
    qs[4:] = si._times(qs[4:], -12)
    fails = []
    for kernel in (0, 1, 2):
        bad = si.batch_bad(metric, f.stats, f.kern[kernel], qs)
        assert bad.tolist() == ([False] * 4 + [True] * 4 if kernel == 2 else [False] * 8)
        exact = si.bsi.exact_keys_many(f.rows, qs[~bad], metric)
        quiet = {m: si.batch_candidates(si.libs(), f, f.kern[kernel], qs[~bad], exact, lv, float(np.abs(exact).max())) < f.half_cap
                 for m, lv in ((False, np.ones(len(f.rows), bool)), (True, f.live))}
        assert quiet[False] and quiet[True]  # the small queries are the ONLY ones that may be answered alone
        _batched_both(oracle_mod, f, kernel, qs, bad, quiet, "queries 2^0 and 2^-12", "mixed query magnitudes %s %s" % (METRIC_NAMES[metric], KERNEL_NAMES[kernel]), fails)
    assert not fails, "%d checks missed:\n%s" % (len(fails), "\n".join(fails))


@pytest.mark.parametrize("er", si.DOWNSTREAM)
def test_downstream(hip_lib, oracle_mod, er):
    """(e) behind the keys, on the f32 route: the second page of a cursor search and a count, against the oracle's full list"""
    d, case = 768, "%d,%d" % (er, er)
    for metric in (L2, IP, COS):
        f = si.facts(d, case, metric)
        with _open(d, metric, f.rows) as idx:
            _set_route(idx, "f32")
            for i, q in enumerate(f.qs):
                eids, edist = oracle_mod.search_exhaustive(f.rows, q, metric, N)
                assert len(eids) == N
                ids, dist, cnt = idx.search(q, K)
                assert cnt[0] == K and np.array_equal(ids[0], eids[:K]) and np.array_equal(dist[0].view(np.uint64), edist[:K].view(np.uint64))
                ids, dist, cnt = idx.search_after(q, K, (float(dist[0][K - 1]), int(ids[0][K - 1])))
                assert cnt[0] == K and np.array_equal(ids[0], eids[K:2 * K]), (case, metric, i, "the second page's ids")
                assert np.array_equal(dist[0].view(np.uint64), edist[K:2 * K].view(np.uint64)), (case, metric, i, "the second page's distances")
                thr = float(edist[39])
                want = len(oracle_mod.search_exhaustive(f.rows, q, metric, N, thr)[0])
                assert want == int(np.sum(edist <= thr)) >= 40
                assert int(idx.search_count(q, thr)[0]) == want, (case, metric, i, "the count")


def test_zz_write_scale_sweep():
    """(runs last in this file) the measured ratios and the routes taken of a whole sweep, for profiles/scale_sweep.json"""
    whole = {("scan", case, d) for case in si.CASES for d in si.WIDTHS} | {("batch", case, 768) for case in si.CASES}
    if not whole <= RAN:
        return  # (a part of the sweep ran: the record of the whole one stays)
    out = [RESULTS[key] for key in sorted(RESULTS, key=lambda x: (x[0], x[2], x[1], str(x[3]), x[4]))]
    assert max(v for e in out for key, v in e.items() if key in ("dense", "masked") and v is not None) <= 1.0
    with open(os.path.join(ROOT, "profiles", "scale_sweep.json"), "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(e) for e in out) + "\n]\n")
