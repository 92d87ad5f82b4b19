"""CPU: the inputs of tests/test_gpu_scales.py (tests/scale_inputs.py) are what that file says they are, and the routes
that sweep demands are the inputs' to demand.  Needs g++ and numpy only.

  1. Scale invariance of the oracle.  Powers of two move no bit of an f64 sum in this range, so for a case (er, eq) the
     oracle's run on the scaled inputs is pinned by its run at (0, 0): inner product -- the same ids, distances
     ldexp(d0, er + eq); L2 with er = eq -- the same ids, distances ldexp(d0, er); cosine -- the same ids AND the same
     distance bits (dot and both norms scale exactly, the quotient is the same f64 division).  L2 with er != eq is
     another ranking altogether (|v|^2 - 2 q.v weighs its two terms differently): there the oracle's ids are held to
     an f64 ranking made here in numpy wherever that ranking is decided by more than f64's own resolution.
  2. Quarantine: no case has an irregular L2 / inner-product row (the largest element of 2^46 times the corpus is below
     1e15); cosine rows' norms, 2^4.8 at d = 768 and 2^2.5 at d = 32, are above 2^-50 down to er = -45 and ALL below it
     from er = -60 down -- 1061 > QUARANTINE_MAX irregular rows: safe mode.  (No case leaves a shard partly quarantined.)
  3. The routes (scale_inputs module docstring): at d = 768 the fp16 scan is demanded for every metric, dense and
     tombstoned, in every case from 2^-38 to 2^46 and in every mismatched case but L2 at (0, 40) and (-40, 40), below;
     at 2^-45 the header still says ok (L2, inner product) but its absolute terms swallow the keys -- every live row is
     a candidate: free; from 2^-60 down the header refuses.  The int8 band is ok for every query of every case, and its survivors cannot overflow the list.
     The f32 scan is demanded in the same cases with two exceptions that the arithmetic here shows: L2 with queries 2^40
     above the rows -- (0, 40) and (-40, 40) -- where every key is |q|^2 to within 2^-38, far inside the RELATIVE band
     3 eps of any tau: every row is a candidate at any scale of that shape, the wide-band fallback is the design.
     The same two cases leave the fp16 scan's demanded set: the oracle itself resolves |q - v|^2 no better than
     (d + 4) 2^-52 |q|^2 -- 2^47 where the keys |v|^2 - 2 q.v of ALL rows lie within 2^49 (0, 40) resp. 2^11 (-40, 40) of
     each other -- its distances are ties broken by id, and a band that is to bound the oracle's order (tsh_scan_f16_band.h,
     tsh_scan_i8_band.h: the term this sweep added) makes every row a candidate.  The int8 list takes all 1061.
  4. The batched path: a shard of 1061 rows is not batched and one of 4096 is (shard_takes_batch); which kernel a forced fp16 runs as (bf16x3 where f16_scale_exp refuses the rows' scale: L2 / inner
     product from 2^-60 down; cosine planes hold unit rows: always fp16) and which queries the batch drops (all of
     them where the queries' own scale is outside the guard: eq = -45 and -60).
"""
import numpy as np
import pytest

import scale_inputs as si
from scale_inputs import COS, IP, K, L2, N
from test_gpu_scan_widths import _bits

LOW = ("-118,-118", "-100,-100", "-60,-60")


def _oracle(oracle_mod, rows, qs, metric, live=None):
    return oracle_mod.search_heap_many_mt(rows, qs, metric, K, None, None if live is None else _bits(live))


def test_the_case_list():
    assert len(si.CASES) == 15 and len(set(si.CASES)) == 15 and set(si.CLEAN) < set(si.CASES) and len(si.CLEAN) == 10
    assert [c for c in si.CASES if si.cosine_runs(c)] == ["%d,%d" % (e, e) for e in si.SAME] + ["40,-40", "-40,40", "mixed"]
    assert N == 16 * 64 + 37


@pytest.mark.parametrize("d", si.WIDTHS)
def test_scaling_is_exact_and_inside_the_model(d):
    for metric in (L2, IP, COS):
        rows, qs, j = si.base(d, metric)
        assert rows.shape == (N, d) and qs.shape == (si.NQ, d) and j.min() == 0 and j.max() == 30
        for case in si.CASES:
            r, q = si.scaled(case, metric, (rows, qs, j))  # (asserts exactness)
            assert np.abs(r).max() < si.BIG_ABS and np.abs(q).max() < si.BIG_ABS and np.all(np.abs(r).max(axis=1) > 0)
        top = float(np.abs(si.scaled("46,46", metric, (rows, qs, j))[0]).max())
        print("d=%d %s: max |element| at 2^46 = %.3g" % (d, si.METRIC_NAMES[metric], top))
        nrm = np.linalg.norm(si.scaled("mixed", metric, (rows, qs, j))[0].astype(np.float64), axis=1)
        assert nrm.max() / nrm.min() > 2.0 ** 29


@pytest.mark.parametrize("d", si.WIDTHS)
def test_the_oracle_is_scale_invariant(oracle_mod, d):
    for metric in (L2, IP, COS):
        f0 = si.facts(d, "0,0", metric)
        ids0, dist0, cnt0 = _oracle(oracle_mod, f0.rows, f0.qs, metric)
        assert np.all(cnt0 == K)
        for case in si.CASES:
            if case == "mixed" or (metric == COS and not si.cosine_runs(case)):
                continue
            er, eq = si.exps(case)
            f = si.facts(d, case, metric)
            ids, dist, cnt = _oracle(oracle_mod, f.rows, f.qs, metric)
            assert np.all(cnt == K)
            if metric == L2 and er != eq:
                # not invariant: held to an f64 ranking of |v|^2 - 2 q.v where its gaps are above the oracle's own
                # resolution (it sums |q - v|^2: 2^-50 |q - v|^2 covers d roundings of 2^-53 each)
                for i in range(si.NQ):
                    order = np.argsort(f.reduced[i], kind="stable")
                    gaps = np.diff(f.reduced[i][order][:K + 1])
                    if gaps.min() > 2.0 ** -50 * f.exact[i].max():
                        assert np.array_equal(ids[i], order[:K]), (case, i)
                continue
            assert np.array_equal(ids, ids0), (si.METRIC_NAMES[metric], case)
            want = dist0 if metric == COS else np.ldexp(dist0, er if metric == L2 else er + eq)
            assert np.array_equal(dist.view(np.uint64), want.view(np.uint64)), (si.METRIC_NAMES[metric], case)


@pytest.mark.parametrize("d", si.WIDTHS)
def test_quarantine_expectations(d):
    assert N > si.QUARANTINE_MAX
    for case in si.CASES:
        for metric in (L2, IP, COS):
            f = si.facts(d, case, metric)
            tiny = metric == COS and case in LOW
            assert f.n_irregular == (N if tiny else 0) and f.safe == tiny, (case, metric, f.n_irregular)


@pytest.mark.parametrize("d", si.WIDTHS)
def test_routes_that_may_be_demanded(d):
    demanded = 0
    for case in si.CASES:
        for metric in (L2, IP, COS):
            if metric == COS and not si.cosine_runs(case):
                continue
            f = si.facts(d, case, metric)
            name = "d=%d %s %s" % (d, case, si.METRIC_NAMES[metric])
            for masked in (False, True):
                print("%s%s: %s; candidates f32 %s fp16 %s, int8 survivors %s" % (name, ", tombstoned" if masked else "", f.routes[masked],
                      f.f32_candidates[masked], f.f16_candidates.get(masked), f.i8_survivors.get(masked)))
                demanded += sum(v == "demanded" for v in f.routes[masked].values())
                n_live = int(f.live.sum()) if masked else N
                # int8: ok everywhere, and the list cannot overflow; the route is the shard's to refuse in safe mode
                assert all(f.i8_ok), name
                assert all(s is not None and s <= N < si.I8_LIST_CAP for s in f.i8_survivors[masked]), name
                assert f.routes[masked]["int8"] == ("refused" if f.safe else "demanded"), name
                swamped_l2 = metric == L2 and case in ("0,40", "-40,40")
                if d == 768:
                    fp16 = f.routes[masked]["fp16"]
                    if case in si.CLEAN and not swamped_l2:
                        assert fp16 == "demanded" and max(f.f16_candidates[masked]) < 40, name
                    if swamped_l2:  # the oracle's own rounding of |q - v|^2, (d + 4) 2^-52 |q|^2, is in the band: every row
                        qn2 = f.qs.astype(np.float64) ** 2
                        w_max = [si.libs().f16(metric, q, f.stats)[3] for q in f.qs]
                        assert fp16 == "free" and all(f.f16_ok) and min(f.f16_candidates[masked]) == n_live, name
                        assert np.all(np.array(w_max) >= (d + 4) * 2.0 ** -52 * qn2.sum(axis=1)), name
                    if case in LOW:
                        assert fp16 == "refused" and not f.f16_exp_ok and f.v_exp > 55, name
                    if case == "-45,-45" and metric == COS:  # 2^-45 x 2^3: the scale is just outside the guard
                        assert fp16 == "refused" and f.v_exp == 56, name
                    if case == "-45,-45" and metric != COS:  # inside the guard and ok, but the absolute terms swallow the keys
                        assert fp16 == "free" and f.v_exp == 55 and all(f.f16_ok) and min(f.f16_candidates[masked]) == n_live, name
                else:
                    assert "fp16" not in f.routes[masked]
                if case in si.CLEAN and not swamped_l2:
                    assert f.routes[masked]["f32"] == "demanded" and max(f.f32_candidates[masked]) < 40, name
                if swamped_l2:  # every key is |q|^2 to within far less than the relative band of ANY tau: why it is free
                    eps_rel = si.f32_band(L2, d, f.qs[0], f.stats[0])[0]
                    assert np.all(f.exact.max(axis=1) / f.exact.min(axis=1) - 1.0 < 1e-3 * eps_rel) and f.routes[masked]["f32"] == "free", name
                if case in LOW and metric != COS:  # keys far below delta_abs (d 2^-100 resp. d 7.5e-37)
                    assert f.routes[masked]["f32"] == "free" and min(f.f32_candidates[masked]) == n_live, name
    print("d=%d: %d (case, metric, dense / tombstoned, family) routes demanded" % (d, demanded))
    assert demanded >= (180 if d == 768 else 120)  # what the sweep demands is not nothing


@pytest.mark.parametrize("d", si.WIDTHS)
def test_the_4bit_routes_that_may_be_demanded(d):
    """scale_inputs.i4_facts (L2, dense), for tests/test_gpu_scales_i4.py: tsh_scan_i4_band.h says ok for every query of
    every case -- its refusal lines (a largest scale below 2^-126 or above 1e30, a widest band of 1e37) lie outside these
    corpora: 2^-118 times the largest element over 127 is still 1.2e-37 -- so no case is refused.  Demanded: wherever the
    model's survivors stay a tenth of the rows below the share.  Free, with (nearly) every row a survivor: keys of 2^-200
    and less, far below the band's underflow terms (2^-118, 2^-100); L2 with queries 2^40 above the rows, where the
    oracle's own (d + 4) 2^-52 |q|^2 is in the band ((-40, 40), and (0, 40) at d = 768: at d = 32 that term is 2^38 beside
    keys 2^42 apart); norms 2^30 apart at d = 768, where a_v max|v| of the longest rows swallows the short rows' keys."""
    import scan_i4_model as M

    share = int(M.MAX_SHARE * N)
    free = {"-118,-118", "-100,-100", "-40,40"} | ({"0,40", "mixed"} if d == 768 else set())
    for case in si.CASES:
        g = si.i4_facts(d, case)
        print("d=%d %s: %s, the model's survivors at most %s" % (d, case, g.route, g.survivors))
        assert all(g.i4_ok) and all(g.i8_ok) and not g.safe, case
        if case in free:
            assert g.route == "free" and min(g.survivors) >= 0.9 * N, case
        else:
            assert g.route == "demanded" and K <= min(g.survivors) and max(g.survivors) <= share - 0.10 * N, case
    assert share == 339


def test_the_f32_band_is_the_designs():
    """spot values of the formulas at d = 768: nch = 3"""
    q = np.zeros(768, np.float32)
    q[0] = 2.0
    assert si._nch(768) == 3
    assert si.f32_band(L2, 768, q, 5.0) == (float(np.float32(3 * 20 * 2.0 ** -23)), float(np.float32(768 * 7.9e-31)))
    want = 2.0 * (18 * 2.0 ** -23 * 2.0 * (1 + 1e-6) * 5.0 * (1 + 1e-6) + 768 * 7.5e-37) * 1.0001
    assert si.f32_band(IP, 768, q, 5.0) == (0.0, float(np.float32(want)))
    want = 2.0 * (2.0 * (1 + 1e-6) * (18 * 2.0 ** -23 + 2.0 ** -21) + 768 * 7.5e-37) * 1.0001
    assert si.f32_band(COS, 768, q, 5.0) == (0.0, float(np.float32(want)))


def test_the_batched_corpus_is_the_smallest_that_is_batched():
    """shard_takes_batch itself: the 1061-row corpus of the scans is never batched, 4096 rows is the line"""
    lb = si.libs()
    for metric in (L2, IP, COS):
        assert not lb.batch_takes(metric, 768, N, 2, si.NQ_BATCH, K) and not lb.batch_takes(metric, 768, 4095, 2, si.NQ_BATCH, K)
        assert lb.batch_takes(metric, 768, 4096, 2, si.NQ_BATCH, K) and lb.batch_takes(metric, 768, si.N_BATCH, 2, si.NQ_BATCH, K)


def test_the_batched_plan_at_every_scale():
    for case in si.CASES:
        for metric in (L2, IP, COS):
            if metric == COS and not si.cosine_runs(case):
                continue
            f = si.batch_facts(case, metric)
            assert f.rows.shape == (si.N_BATCH, 768) and f.qs.shape == (si.NQ_BATCH, 768)
            assert f.safe == (metric == COS and case in LOW) and f.n_irregular == (si.N_BATCH if f.safe else 0)
            assert f.kern[0] == 0 and f.kern[1] == 1
            assert f.kern[2] == (1 if metric != COS and case in LOW else 2), (case, metric)
            assert not f.bad[0].any() and not f.bad[1].any()
            all_dropped = metric != COS and case in ("-45,-45", "46,-60")  # the queries' own scale: 2^-45 x 2^2 is outside
            assert f.bad[2].all() if all_dropped else not f.bad[2].any(), (case, metric)
            # the tombstones kill every query's nearest row; which lists cannot overflow: everywhere from 2^-45 up but
            # L2 with queries 2^40 above the rows and -- by this count, an upper bound -- L2 rows of mixed norms on bf16x3 / fp16
            # keys; below 2^-60 the absolute term d 7.5e-37 swallows every L2 / inner-product key
            assert not f.live[np.argmin(f.exact, axis=1)].any() and 70 <= (~f.live).sum() <= 80
            swamped = metric != COS and case in LOW or metric == L2 and case in ("0,40", "-40,40")
            for kernel in (0, 1, 2):
                for masked in (False, True):
                    n = f.candidates[kernel, masked]
                    if swamped:
                        assert n >= f.half_cap, (case, metric, kernel, n)
                    elif not (case == "mixed" and metric == L2 and kernel != 0):
                        assert n < 64 < f.half_cap == 2048, (case, metric, kernel, n)
