"""Inputs of tests/test_gpu_scales.py -- the scan and key kernels far from unit magnitude -- and the properties that
sweep rests on, checkable without a GPU (tests/test_host_scale_inputs.py asserts every one of them).

One base corpus per width (d = 768: the f32, fp16 and int8 tile scans and the three batched key kernels; d = 32: the
packed f32 scan and the int8 scan on 8 lanes), made as test_gpu_scan_widths._gaussian makes it: 16 tiles and one of 37
rows, capacity = rows, 4 queries, k = 10, L2 / inner-product rows times U(0.5, 2) per row, cosine queries normalised
(the ABI requires it: cosine queries that are not unit vectors are outside the contract and are not tested).  Every
element is then rounded to a multiple of 2^-31 -- nothing for an element of 2^-8 and more, at most 2^-32 for a smaller
one -- so that 2^-118 times the corpus is still exact in f32 (the smallest subnormal step is 2^-149).

A case is (er, eq): rows times 2^er and, for L2 and inner product, queries times 2^eq, both exact in f32 (asserted).
Cosine takes each distinct er once, with its unit queries.  `mixed`: row i times its own 2^-j_i, j_i drawn from 0..30 --
norms 2^30 apart inside one shard.  The batched path needs a shard of 4096 rows (shard_takes_batch), so its cases run on
a second base corpus of the same make, 4096 + 256 + 37 rows (a ragged last tile for either tile shape) and 8 queries.

What facts() works out per case, width and metric, from f64 keys and from the headers themselves (g++: tests/cpp/
scan_f16_band_lib.cpp, scan_i8_band_lib.cpp, batch_plan_lib.cpp), never from the library under test:
  quarantine   a row with an element above 1e15 (or not finite), for cosine a row whose norm is below 2^-50: up to
               QUARANTINE_MAX = 1024 rows are quarantined, more put the shard in safe mode
  fp16         "refused": scan_f16_exp says no, or scan_f16_band(...).ok is false for every query (or safe mode);
               "demanded": ok for every query and _f16_candidates (test_gpu_scan_widths) below 96 = half of
               tsh_default_block_entries(10) for every query -- the scan must run and nothing may be redone; else "free"
  int8         "demanded": scan_i8_band(...).ok for every query; the survivors -- rows whose exact key - 2 w_i is at or
               below the k-th smallest tile minimum + 2 max w -- are 1061 at most, under I8_LIST_CAP = 4096: the list
               cannot overflow at any scale; else "free" (safe mode: "refused")
  f32          the band recomputed here from DESIGN.md section 4 / compute_band (L2: eps_rel = 3 (4 nch + 8) 2^-23,
               delta_abs = d 7.9e-31; inner product: 2 ((4 nch + 6) 2^-23 |q| max|v| + d 7.5e-37) 1.0001; cosine:
               2 (|q| ((4 nch + 6) 2^-23 + 2^-21) + d 7.5e-37) 1.0001); "demanded" -- no wide-band fallback -- when the
               rows whose exact key less its own error is inside the band of the k-th smallest exact tile minimum (what
               the select takes for tau) plus its error stay below 96; else "free"
  4-bit        i4_facts() (L2, dense; tests/test_gpu_scales_i4.py): "demanded" where the int8 band and tsh_scan_i4_band.h
               (tests/cpp/scan_i4_band_lib.cpp) are ok for every query and the survivors of the NumPy model
               (scan_i4_model.py) stay at or below SCAN_I4_MAX_SHARE of the rows; "refused" where the 4-bit band's ok is
               false for every query; else "free"
  batched      batch_facts(): the kernel a forced option runs as and the queries the call drops (tsh_batch_plan.h), the
               tombstones of the second pass (every query's nearest row dead), and the most rows a query can have on
               its candidate list (batch_candidates) -- below half of cand_cap nothing but the dropped queries may be
               answered alone
"""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

import batch_shape_inputs as bsi
from test_gpu_bands import _exact_keys
from test_gpu_scan_widths import COS, IP, K, L2, METRIC_NAMES, N, NQ, TILE, _f16_candidates, _families, _gaussian, _nch, _tombstones

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (768, 32)
SAME = (-118, -100, -60, -45, -38, -20, 0, 20, 46)
MISMATCHED = ((0, 40), (0, -40), (40, -40), (-40, 40), (46, -60))
CASES = tuple("%d,%d" % (e, e) for e in SAME) + tuple("%d,%d" % c for c in MISMATCHED) + ("mixed",)
CLEAN = tuple("%d,%d" % (e, e) for e in SAME if -38 <= e <= 46) + tuple("%d,%d" % c for c in MISMATCHED)  # must be demanded
DOWNSTREAM = (-38, 0, 46)
BIG_ABS = 1.0e15
TINY_NORM = 2.0 ** -50
QUARANTINE_MAX = 1024
I8_LIST_CAP = 4096
HALF_BLOCK = 96  # half of tsh_default_block_entries(10) = 192
SEED = 20261020
N_BATCH = 4096 + 256 + 37
NQ_BATCH = 8
GRID = 2.0 ** 31


def exps(case):
    """(er, eq) of a case; None for `mixed`"""
    return None if case == "mixed" else tuple(int(v) for v in case.split(","))


def cosine_runs(case):
    """cosine takes each distinct er once: in the first case of CASES that has it (`mixed` is its own)"""
    if case == "mixed":
        return True
    er = exps(case)[0]
    return next(c for c in CASES if c != "mixed" and exps(c)[0] == er) == case


def _on_grid(a):
    out = (np.round(a.astype(np.float64) * GRID) / GRID).astype(np.float32)
    assert np.all(np.abs(out.astype(np.float64) - a) <= 2.0 ** -32) and np.array_equal(out[np.abs(a) >= 2.0 ** -8], a[np.abs(a) >= 2.0 ** -8])
    return out


@functools.lru_cache(maxsize=None)
def base(d, metric):
    """(rows [N, d], queries [NQ, d], j [N]: the exponents of `mixed`) of one width and metric"""
    import oracle

    oracle.build()
    rng = np.random.default_rng(SEED + 10 * d + metric)
    rows, qs = _gaussian(rng, d, metric, oracle.normalize_f32)
    rows = _on_grid(rows)
    if metric != COS:
        qs = _on_grid(qs)
    return rows, qs, rng.integers(0, 31, size=N)


@functools.lru_cache(maxsize=None)
def base_batch(metric):
    """the batched path's base corpus at d = 768: (rows [N_BATCH, 768], queries [NQ_BATCH, 768], j [N_BATCH])"""
    import oracle

    oracle.build()
    rng = np.random.default_rng(SEED + 7 + metric)
    rows = rng.standard_normal((N_BATCH, 768), dtype=np.float32)
    if metric != COS:
        rows *= rng.uniform(0.5, 2.0, size=(N_BATCH, 1)).astype(np.float32)
    qs = rng.standard_normal((NQ_BATCH, 768), dtype=np.float32)
    if metric == COS:
        qs = np.stack([oracle.normalize_f32(q) for q in qs])
    else:
        qs = _on_grid(qs)
    return _on_grid(rows), qs, rng.integers(0, 31, size=N_BATCH)


def _times(a, e):
    """a * 2^e, exact in f32 (asserted)"""
    want = np.ldexp(a.astype(np.float64), e)
    out = want.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), want) and np.all(np.isfinite(out)), "2^%s times the corpus is not exact in f32" % (e,)
    return out


def scaled(case, metric, b):
    """(rows, queries) of a case from a base (rows, queries, j)"""
    rows, qs, j = b
    if case == "mixed":
        return _times(rows, -j[:, None]), qs
    er, eq = exps(case)
    rows = _times(rows, er)
    if er == 46:
        assert np.abs(rows).max() < BIG_ABS
    return rows, (qs if metric == COS else _times(qs, eq))


class Libs:
    """tsh_scan_f16_band.h, tsh_scan_i8_band.h and tsh_batch_plan.h by g++"""

    def __init__(self, workdir):
        self.plan = bsi.PlanLib(workdir)
        fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
        c_int, c_f = ctypes.c_int, ctypes.c_float
        libs = {}
        for name in ("scan_f16_band", "scan_i8_band"):
            so = os.path.join(str(workdir), "lib%s_scales.so" % name)
            src = os.path.join(ROOT, "tests", "cpp", name + "_lib.cpp")
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
            libs[name] = ctypes.CDLL(so)
        self.f16_lib, self.i8_lib = libs["scan_f16_band"], libs["scan_i8_band"]
        self.f16_lib.scan_f16_band_of.restype = c_int
        self.f16_lib.scan_f16_band_of.argtypes = [c_int, c_int, fp, c_f, c_f, c_f, fp]
        self.f16_lib.scan_f16_exp_of.restype = c_int
        self.f16_lib.scan_f16_exp_of.argtypes = [c_f, ip]
        self.i8_lib.scan_i8_band_of.restype = c_int
        self.i8_lib.scan_i8_band_of.argtypes = [c_int, c_int, fp, c_f, c_f, c_f, fp]
        self.i8_lib.scan_i8_scale_of.restype = c_f
        self.i8_lib.scan_i8_scale_of.argtypes = [c_f]
        self.plan.lib.batch_f16_scale_exp_of.restype = c_int
        self.plan.lib.batch_f16_scale_exp_of.argtypes = [c_f, ip]

    def f16_exp(self, max_abs):
        e = ctypes.c_int(0)
        return bool(self.f16_lib.scan_f16_exp_of(float(max_abs), ctypes.byref(e))), e.value

    def f16(self, metric, q, stats):
        """(ok, alpha, beta, w_max)"""
        q = np.ascontiguousarray(q, np.float32)
        out = (ctypes.c_float * 3)()
        ok = self.f16_lib.scan_f16_band_of(metric, len(q), q.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), stats[0], stats[1], stats[2], out)
        return bool(ok), float(out[0]), float(out[1]), float(out[2])

    def i8(self, metric, q, stats):
        """(ok, a_s, a_v, beta)"""
        q = np.ascontiguousarray(q, np.float32)
        out = (ctypes.c_float * 4)()
        ok = self.i8_lib.scan_i8_band_of(metric, len(q), q.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), stats[0], stats[1], stats[2], out)
        return bool(ok), float(out[0]), float(out[1]), float(out[2])

    def i8_scales(self, row_max):
        return np.array([self.i8_lib.scan_i8_scale_of(float(v)) for v in row_max], np.float64)

    def batch_exp(self, top):
        e = ctypes.c_int(0)
        return bool(self.plan.lib.batch_f16_scale_exp_of(float(top), ctypes.byref(e))), e.value

    def batch_kernel(self, metric, d, n_rows, stats, kernel, nq, k):
        """the key kernel plan_batch runs when `kernel` is forced on a shard of these statistics"""
        out = (ctypes.c_int64 * len(self.plan.FIELDS))()
        self.plan.lib.batch_plan_of(metric, d, n_rows, stats[0], stats[1], stats[2], kernel, 1, nq, k, -1, out)
        return int(out[self.plan.FIELDS.index("kern")])

    def batch_takes(self, metric, d, n_rows, batch_min_nq, nq, k):
        """shard_takes_batch: does a call of nq queries on a shard of n_rows rows go to the matrix cores?"""
        fn = self.plan.lib.batch_takes_of
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        return bool(fn(metric, d, n_rows, batch_min_nq, nq, k))

    def batch_band_ok(self, metric, d, n_rows, stats, kernel, q):
        out = (ctypes.c_float * 3)()
        q64 = q.astype(np.float64)
        return self.plan.lib.batch_band_of(metric, d, n_rows, stats[0], stats[1], stats[2], kernel, float(q64 @ q64), out) == 1


@functools.lru_cache(maxsize=1)
def libs():
    workdir = tempfile.mkdtemp(prefix="scale_inputs_")
    atexit.register(shutil.rmtree, workdir, True)
    return Libs(workdir)


def quarantine(rows, metric):
    """(rows the documented rules quarantine, safe mode): the rules, not the kernel's arithmetic -- no row of any case
    lies within 1 % of either line (asserted), so that the two cannot differ"""
    r64 = rows.astype(np.float64)
    amax = np.abs(r64).max(axis=1)
    nrm = np.sqrt(np.einsum("ij,ij->i", r64, r64))
    assert not np.any((amax > 0.99 * BIG_ABS) & (amax < 1.01 * BIG_ABS)) and not np.any((nrm > 0.99 * TINY_NORM) & (nrm < 1.01 * TINY_NORM))
    irregular = ~np.isfinite(amax) | (amax > BIG_ABS)
    if metric == COS:
        irregular |= (nrm > 0) & (nrm < TINY_NORM)
    n = int(irregular.sum())
    return irregular, n > QUARANTINE_MAX


def reduced_keys(rows, q, metric):
    """f64 keys of the operation the fp16 and int8 scans approximate: L2 leaves the common |q|^2 out.  Summed as
    |v|^2 - 2 q.v and not as |q - v|^2 - |q|^2: with queries 2^40 and more above the rows the second form cancels to
    nothing in f64, while the first is good to 2^-50 (|v|^2 + |q| |v|) -- nothing beside a band of 2^-11 |q| |v|."""
    if metric != L2:
        return _exact_keys(rows, q, metric)
    r64, q64 = rows.astype(np.float64), q.astype(np.float64)
    return np.einsum("ij,ij->i", r64, r64) - 2.0 * (r64 @ q64)


def f32_band(metric, d, q, max_norm):
    """(eps_rel, delta_abs) of compute_band, from the formulas of DESIGN.md section 4"""
    u2, nch = 2.0 ** -23, _nch(d)
    q64 = q.astype(np.float64)
    qn = np.sqrt(q64 @ q64) * (1.0 + 1e-6)
    if metric == L2:
        return float(np.float32(3.0 * (4.0 * nch + 8.0) * u2)), float(np.float32(d * 7.9e-31))
    gam = (4.0 * nch + 6.0) * u2
    delta = gam * qn * max_norm * (1.0 + 1e-6) if metric == IP else qn * (gam + 2.0 ** -21)
    return 0.0, float(np.float32(2.0 * (delta + d * 7.5e-37) * 1.0001))


def _tile_kth(e):
    mins = np.sort([e[t * TILE:(t + 1) * TILE].min() for t in range((len(e) + TILE - 1) // TILE)])
    assert np.isfinite(mins[K - 1])
    return mins[K - 1]


def f32_candidates(metric, exact, live, eps_rel, delta_abs):
    """Rows the f32 select can emit at most, for one query: tau, the k-th smallest tile minimum of the keys, is at most
    the k-th smallest exact tile minimum plus its error; the band is tau + |tau| eps_rel + delta_abs; a row's key is at
    least its exact key less its own error.  (1.001: the select's own roundings.)"""
    e = np.where(live, exact, np.inf)
    err = (eps_rel / 3.0) * np.abs(e) + delta_abs if metric == L2 else np.full(len(e), delta_abs / 2.0)
    kth = _tile_kth(e)
    tau = kth + ((eps_rel / 3.0) * abs(kth) + delta_abs if metric == L2 else delta_abs / 2.0)
    band = tau + abs(tau) * eps_rel + delta_abs
    with np.errstate(invalid="ignore"):
        return int(np.sum(np.where(live, e - err, np.inf) <= band + 1e-3 * abs(band)))


def i8_survivors(metric, reduced, live, w):
    """the int8 pass's survivors at most, for one query: exact key - 2 w_i at or below the k-th smallest tile minimum of
    the exact keys + 2 max w"""
    e = np.where(live, reduced, np.inf)
    return int(np.sum(e - 2.0 * w <= _tile_kth(e) + 2.0 * w[live].max()))


class Facts:
    pass


@functools.lru_cache(maxsize=None)
def facts(d, case, metric):
    """Everything the sweep rests on for one case, width and metric (module docstring)."""
    lb = libs()
    f = Facts()
    f.d, f.case, f.metric = d, case, metric
    f.rows, f.qs = scaled(case, metric, base(d, metric))
    f.exact = np.stack([_exact_keys(f.rows, q, metric) for q in f.qs])
    f.reduced = np.stack([reduced_keys(f.rows, q, metric) for q in f.qs])
    irregular, f.safe = quarantine(f.rows, metric)
    f.n_irregular = int(irregular.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        ranked = np.where(np.isfinite(f.exact), f.exact, np.inf)  # (a zero cosine norm: none in these corpora)
    f.live = _tombstones(np.random.default_rng(SEED + 1000 * d + 10 * metric + CASES.index(case)), ranked)
    f.stats = bsi.PlanLib.norms(f.rows)
    f.f16_exp_ok, f.v_exp = lb.f16_exp(f.stats[2])
    r64 = f.rows.astype(np.float64)
    nrm = np.sqrt(np.einsum("ij,ij->i", r64, r64))
    scales = lb.i8_scales(np.abs(f.rows).max(axis=1))
    families = _families(d)
    f.routes, f.f16_candidates, f.f32_candidates, f.i8_survivors = {}, {}, {}, {}
    f.f16_ok = [lb.f16(metric, q, f.stats)[0] for q in f.qs] if "fp16" in families else []
    f.i8_ok = [lb.i8(metric, q, f.stats)[0] for q in f.qs]
    for masked, live in ((False, np.ones(N, bool)), (True, f.live)):
        routes = {}
        # f32
        cand = []
        for i, q in enumerate(f.qs):
            eps_rel, delta_abs = f32_band(metric, d, q, f.stats[0])
            cand.append(f32_candidates(metric, f.exact[i], live, eps_rel, delta_abs))
        f.f32_candidates[masked] = cand
        routes["f32"] = "demanded" if not f.safe and max(cand) < HALF_BLOCK else "free"
        # fp16
        if "fp16" in families:
            cand = []
            for i, q in enumerate(f.qs):
                ok, _, _, w_max = lb.f16(metric, q, f.stats)
                cand.append(_f16_candidates(f.reduced[i:i + 1], live, w_max)[0] if ok else None)
            f.f16_candidates[masked] = cand
            if f.safe or not any(f.f16_ok):
                routes["fp16"] = "refused"
            elif all(f.f16_ok) and max(cand) < HALF_BLOCK:
                routes["fp16"] = "demanded"
            else:
                routes["fp16"] = "free"
        # int8
        if "int8" in families:
            surv = []
            for i, q in enumerate(f.qs):
                ok, a_s, a_v, beta = lb.i8(metric, q, f.stats)
                if not ok:
                    surv.append(None)
                    continue
                w = a_s * scales / nrm + beta if metric == COS else a_s * scales + a_v * nrm + beta
                surv.append(i8_survivors(metric, f.reduced[i], live, w * 1.001))
            f.i8_survivors[masked] = surv
            routes["int8"] = "refused" if f.safe else ("demanded" if all(f.i8_ok) else "free")
        f.routes[masked] = routes
    return f


@functools.lru_cache(maxsize=None)
def i4_facts(d, case):
    """The 4-bit first pass in front of the int8 scan (L2, dense: the only shape it takes) for one case and width, on the
    rows, queries and reduced keys of facts(d, case, L2).  ok per query from tsh_scan_i4_band.h itself (tests/cpp/
    scan_i4_band_lib.cpp), the survivors from the NumPy model (scan_i4_model.Shard.survivors: at most).  The route:
      "demanded"  the int8 band and the 4-bit band are ok for every query and the model's survivors stay at or below
                  SCAN_I4_MAX_SHARE of the rows for every query -- no scan can be denied: each query runs one 4-bit and
                  one int8 scan;
      "refused"   the 4-bit band's ok is false for every query: the pass never runs and its probe refuses;
      "free"      otherwise (a band as wide as the keys keeps every row, and the deny rule may act)."""
    import scan_i4_inputs as si4
    import scan_i4_model as M

    f = facts(d, case, L2)
    g = Facts()
    g.d, g.case, g.rows, g.qs, g.reduced, g.i8_ok, g.safe = d, case, f.rows, f.qs, f.reduced, f.i8_ok, f.safe
    g.i4_ok = [si4.header_band(q, f.stats[0], f.stats[2])[0] for q in f.qs]
    sh = M.Shard(f.rows)
    with np.errstate(all="ignore"):
        g.survivors = [sh.survivors(q, K)[1] if ok else None for q, ok in zip(f.qs, g.i4_ok)]
    if f.safe or not any(g.i4_ok):
        g.route = "refused"
    elif all(g.i4_ok) and all(g.i8_ok) and max(g.survivors) <= int(M.MAX_SHARE * N):
        g.route = "demanded"
    else:
        g.route = "free"
    return g


@functools.lru_cache(maxsize=None)
def batch_facts(case, metric):
    """The batched path's case: rows, queries, and per forced kernel what tsh_batch_plan.h says of it -- the kernel that
    runs (a forced fp16 turns into bf16x3 where f16_scale_exp refuses the rows' scale) and the queries the batch drops
    as `bad` (no band: batch_delta2; fp16: the batch's largest query element outside the guard of f16_scale_exp -- every
    query --, or a query whose largest element is below 1 / 256 of the batch's)."""
    lb = libs()
    f = Facts()
    f.case, f.metric = case, metric
    f.rows, f.qs = scaled(case, metric, base_batch(metric))
    irregular, f.safe = quarantine(f.rows, metric)
    f.n_irregular = int(irregular.sum())
    f.stats = bsi.PlanLib.norms(f.rows)
    f.exact = bsi.exact_keys_many(f.rows, f.qs, metric)
    f.live = batch_tombstones(f.exact)
    f.kern, f.bad, f.candidates = {}, {}, {}
    cap = lb.plan.plan(metric, 768, N_BATCH, 0, NQ_BATCH, K)["cand_cap"]
    f.half_cap = cap // 2
    key_max = float(np.abs(f.exact).max())
    for kernel in (0, 1, 2):
        kern = f.kern[kernel] = lb.batch_kernel(metric, 768, N_BATCH, f.stats, kernel, NQ_BATCH, K)
        bad = f.bad[kernel] = batch_bad(metric, f.stats, kern, f.qs)
        for masked, live in ((False, np.ones(N_BATCH, bool)), (True, f.live)):
            f.candidates[kernel, masked] = batch_candidates(lb, f, kern, f.qs[~bad], f.exact[~bad], live, key_max)
    return f


def batch_tombstones(exact):
    """live[] over the batched corpus: every query's nearest row dies, and with them rows at the edges of 64-, 128- and
    256-row units, the shard's last row and one whole 64-row run (as test_gpu_batch_shapes._dense_dead)"""
    live = np.ones(exact.shape[1], bool)
    live[[5 * 64, 5 * 64 + 63, 9 * 128, 9 * 128 + 127, 7 * 256, 7 * 256 + 255, exact.shape[1] - 1] + list(range(40 * 64, 41 * 64))] = False
    live[np.argmin(exact, axis=1)] = False
    return live


def batch_candidates(lb, f, kern, qs, exact, live, key_max):
    """The most rows any of these queries can have on its candidate list: the shard is its own sample (16384 rows at
    most), so the threshold is the K-th smallest key, and with every key within D of its exact value (D: batch_delta2 at
    the longest row, batch_shape_inputs.PlanLib.bound) only live rows within 4 D of the K-th smallest exact key can
    be listed.  Below half of cand_cap no list can overflow: nothing but the dropped queries is answered alone."""
    worst = 0
    for q, e in zip(qs, exact):
        D = lb.plan.bound(f.metric, 768, N_BATCH, f.stats, kern, q, key_max)
        e = np.where(live, e, np.inf)
        worst = max(worst, int(np.sum(e <= np.sort(e)[K - 1] + 4.0 * D)))
    return worst


def batch_bad(metric, stats, kern, qs):
    """the queries of one call that batch_prepare_queries drops, by tsh_batch_plan.h: no band (batch_delta2); fp16 keys: a
    query whose largest element is below 1 / 256 of the batch's, or every query where the batch's largest element is
    outside the guard of f16_scale_exp"""
    lb = libs()
    qmax = np.abs(qs).max(axis=1)
    bad = np.array([not lb.batch_band_ok(metric, qs.shape[1], N_BATCH, stats, kern, q) for q in qs])
    if kern == 2:
        top = np.float32(qmax[~bad].max()) if (~bad).any() else np.float32(0)
        bad |= ~(qmax >= top * np.float32(0.00390625))
        if top > 0 and not lb.batch_exp(top)[0]:
            bad[:] = True
    return bad
