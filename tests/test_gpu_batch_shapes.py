"""GPU: the batched (matrix-core) key kernels -- f32 MFMA, bf16x3, fp16 "ping-pong" (tsh_batch.hip.h, tsh_batch_f16pp.hip.h)
-- against f64 keys at every tile, chunk and lane edge, dense and filtered, on both workgroup tiles.

(a) test_dense_keys_every_pair[d]: the dense instantiations.  WIDTHS has, per chunk count nk = ceil(d / 32) in 1, 2, 3,
    4, 5, 6, 8, 9, the full width 32 nk, one element in the last chunk (32 (nk - 1) + 1) and 32 (nk - 1) + 19 (odd: ld
    pads) -- every branch shape of the bf16x3 K loop (1, 2, 3, 4, 5 and more chunks, either parity of the remainder) and
    fp16 ring turns of one, two and three.  The shard has 4096 + 256 + 37 rows, capacity = rows: a ragged last tile for
    either tile width and n_tiles % 8 != 0.  Per metric and kernel the probe's keys of ALL nq x rows pairs (nq = 100: the
    128-query tile of every kernel, 28 of its rows padding -- bf16x3 and fp16 take the 256 tile for every batch of more
    than 128; nq = 130: two query tiles, 128 + 2 for the f32 kernel, 130 + 126 rows of padding for the others; nq = 257:
    one query in the second tile, three tiles for the f32 kernel) are held to the bound the host claims: |key - exact| <= d2[q] / 2 / 1.0001, and for fp16 keys of
    L2 / inner product 2 |key - exact| <= alpha2[q] |v| + beta2[q]; on Gaussian rows (norms over [0.5, 2] for L2 / IP), on
    rows whose operands sit at the rounding midpoints of the kernel's format (test_gpu_bands._patterned), with the plane
    in row order instead of norm-grouped, and with tombstones at the edges of 64-, 128- and 256-row units, on the shard's
    last row and on a whole 64-row run: dead rows are NaN, every live key is finite and within its bound.  The worst
    |key - exact| / bound per (kernel, width, metric, tile) goes to profiles/batch_shape_sweep.json.
(b) test_planted_neighbours_at_every_edge: the filtered instantiations.  batch_shape_inputs.planted_edges plants every
    query's k = 8 nearest rows at tile, wave-column and lane-half edges, at both ends of the sample, in the ragged tile;
    its check() proves on the CPU that each is a certain survivor and that no list can overflow.  Counts, ids and
    distance bits must be the oracle's and NOTHING may be redone: a row dropped at an edge cannot hide behind a scan.
(c) test_epilogue_crowds: the fp16 epilogue's rare branches by construction (batch_shape_inputs.epilogue_crowds): two
    survivors of a lane in one block, three in three blocks, a hit list flushed in the walk and on the straight path, a
    dead row inside a crowd, a crowd on the shard's last rows -- on the 256-query tile (257 queries) and the 128-query one.
(d) test_persistent_loop_changes_query_tile: 600 queries (three query tiles) and more filtered tiles than CUs: workgroups
    take a second tile of another query tile, and rows planted in exactly those tiles must come back -- rows that the
    thresholds of the workgroup's FIRST query tile, or |v|^2 of its first tile's rows, would drop; the dense counterpart holds all 600 x rows keys of such a launch to their bound.
"""
import json
import os

import numpy as np
import pytest

import batch_shape_inputs as bsi
from batch_shape_inputs import COS, IP, L2, METRIC_NAMES, K
from test_gpu_bands import _exact_keys, _patterned

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_NAMES = ("f32 MFMA", "bf16x3", "fp16")
NKS = (1, 2, 3, 4, 5, 6, 8, 9)
WIDTHS = tuple(sorted({w for nk in NKS for w in (32 * nk, 32 * (nk - 1) + 1, 32 * (nk - 1) + 19)}))
N_DENSE = 4096 + 256 + 37
NQS = (100, 130, 257)
QUIET = ("scan_launches", "fallback_searches", "batch_scan_fallbacks", "batch_plane_fallbacks", "exact_redone")
RESULTS = {}


@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    return bsi.PlanLib(tmp_path_factory.mktemp("batch_plan"))


def test_the_width_list_is_the_rule():
    assert len(WIDTHS) == 24 and {(d + 31) // 32 for d in WIDTHS} == set(NKS)
    assert {(-(-d // 32) + 3) // 4 for d in WIDTHS} == {1, 2, 3}  # fp16 ring turns


def _check(fails, cond, msg):
    if not cond:
        fails.append(msg)
    return bool(cond)


def _open(d, metric, rows, kernel, group=True):
    from tostore_amd import HipVectorIndex

    idx = HipVectorIndex(d, metric, capacity_rows=len(rows))
    idx.append(0, rows)
    idx.set_batch_kernel(kernel)
    idx.set_batch_min_nq(2)
    if not group:
        idx.set_batch_group(False)
    return idx


def _tile(kernel, nq):
    return 256 if kernel != 0 and nq > 128 else 128


def _probe(idx, kernel, metric, qs, exact, nrm, live, what, fails):
    """All nq x rows keys of one probe call against their bounds: the worst |key - exact| / bound (inf on a miss that
    leaves no ratio)."""
    nq = len(qs)
    keys, d2 = idx.probe_batch_keys(qs, K)
    _check(fails, idx.counters()["batch_kernel_last"] == kernel, what + ": another key kernel ran")
    keys = keys.astype(np.float64)
    if kernel == 2 and metric != COS:
        a2, b2 = idx.probe_batch_row_band(nq)
        bound = (a2.astype(np.float64)[:, None] * nrm[None, :] + b2.astype(np.float64)[:, None]) / 2.0
    else:
        bound = np.broadcast_to((d2.astype(np.float64) / 2.0 / 1.0001)[:, None], keys.shape)
    _check(fails, np.all(np.isnan(keys[:, ~live])), what + ": a dead row has a key")
    if not _check(fails, np.all(np.isfinite(keys[:, live])), what + ": a live row's key is not finite"):
        return float("inf")
    ratio = np.abs(keys[:, live] - exact[:nq][:, live]) / bound[:, live]
    worst = float(ratio.max())
    print("%s: max |key - exact| / bound = %.4f" % (what, worst))
    if worst > 1.0:
        q, r = np.unravel_index(np.argmax(ratio), ratio.shape)
        _check(fails, False, "%s: a key is further from its exact value than its bound: %.4f (query %d, row %d)"
               % (what, worst, q, np.nonzero(live)[0][r]))
    return worst


def _record(kernel, d, metric, nq, key, ratio):
    tile = _tile(kernel, nq)
    e = RESULTS.setdefault((kernel, d, metric, tile), {"kernel": KERNEL_NAMES[kernel], "dim": d, "chunks": (d + 31) // 32,
                                                       "metric": METRIC_NAMES[metric], "tile": tile})
    e[key] = round(max(ratio, e.get(key, 0.0)), 4)


def _dense_corpora(rng, d, metric, normalize):
    """name -> (kernels probed, rows, queries)"""
    nq = max(NQS)
    rows = rng.standard_normal((N_DENSE, d), dtype=np.float32)
    if metric != COS:
        rows *= rng.uniform(0.5, 2.0, size=(N_DENSE, 1)).astype(np.float32)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    # inside the error model: the fp16 kernel scales a batch by its largest element, and a query whose own largest
    # element is 2^8 below that is answered alone, not by the key kernel (one or two of 257 Gaussian queries at d = 1)
    qmax = np.abs(qs).max(axis=1)
    small = qmax < qmax.max() / 64
    qs[small] *= (qmax.max() / 64 / qmax[small])[:, None]
    out = {"gaussian": ((0, 1, 2), rows, qs)}
    scale = np.ldexp(1.0, -rng.integers(0, 5, size=N_DENSE)).astype(np.float32)[:, None]  # norms over a factor 16
    up = (np.arange(N_DENSE) & 1).astype(bool)[:, None]
    for kernel in (0, 1, 2):
        prows = np.where(up, _patterned(rng, (N_DENSE, d), kernel, True), _patterned(rng, (N_DENSE, d), kernel, False)) * scale
        out["patterned %s" % KERNEL_NAMES[kernel]] = ((kernel,), prows.astype(np.float32), _patterned(rng, (nq, d), kernel, False))
    if metric == COS:
        out = {name: (ks, r, np.stack([normalize(q) for q in q_])) for name, (ks, r, q_) in out.items()}
    return out


def _dense_dead():
    dead = [5 * 64, 5 * 64 + 63, 9 * 128, 9 * 128 + 127, 7 * 256, 7 * 256 + 255, N_DENSE - 1] + list(range(40 * 64, 41 * 64))
    live = np.ones(N_DENSE, bool)
    live[dead] = False
    return live


@pytest.mark.parametrize("d", WIDTHS)
def test_dense_keys_every_pair(hip_lib, oracle_mod, d):
    rng = np.random.default_rng(9000 + d)
    fails = []
    all_live, tomb = np.ones(N_DENSE, bool), _dense_dead()
    for metric in (L2, IP, COS):
        for corpus, (kernels, rows, qs) in _dense_corpora(rng, d, metric, oracle_mod.normalize_f32).items():
            assert np.abs(qs).max(axis=1).min() >= np.abs(qs).max() / 128
            exact = bsi.exact_keys_many(rows, qs, metric)
            for q in (0, 129, 256):  # (the many-query form of the reference is the one-query form)
                one = _exact_keys(rows, qs[q], metric)
                assert np.allclose(exact[q], one, rtol=0, atol=1e-11 * (1.0 + np.abs(one).max()))
            nrm = np.sqrt(np.einsum("ij,ij->i", rows.astype(np.float64), rows.astype(np.float64)))
            for kernel in kernels:
                name = "d=%d %s %s, %s rows" % (d, METRIC_NAMES[metric], KERNEL_NAMES[kernel], corpus)
                with _open(d, metric, rows, kernel) as idx:
                    for nq in NQS:
                        worst = _probe(idx, kernel, metric, qs[:nq], exact, nrm, all_live, "%s, nq=%d" % (name, nq), fails)
                        _record(kernel, d, metric, nq, "dense" if corpus == "gaussian" else "dense_patterned", worst)
                    if corpus != "gaussian":
                        continue
                    idx.set_deleted(np.nonzero(~tomb)[0])
                    for nq in NQS:
                        worst = _probe(idx, kernel, metric, qs[:nq], exact, nrm, tomb, "%s, nq=%d, tombstoned" % (name, nq), fails)
                        _record(kernel, d, metric, nq, "tombstoned", worst)
                if corpus == "gaussian" and kernel == 2 and metric != COS:  # the plane in row order: no perm to undo
                    with _open(d, metric, rows, kernel, group=False) as idx:
                        worst = _probe(idx, kernel, metric, qs[:130], exact, nrm, all_live, name + ", nq=130, plane in row order", fails)
                        _record(kernel, d, metric, 130, "row_order", worst)
    assert not fails, "%d checks missed:\n%s" % (len(fails), "\n".join(fails))


def test_zz_write_batch_shape_sweep():
    """(runs last in this file) the measured ratios of a whole sweep, for profiles/batch_shape_sweep.json"""
    if {d for (_, d, _, _) in RESULTS} != set(WIDTHS):
        return  # (a part of the sweep ran: the record of the whole one stays)
    out = [RESULTS[key] for key in sorted(RESULTS)]
    assert max(max(v for v in e.values() if isinstance(v, float)) for e in out) <= 1.0
    with open(os.path.join(ROOT, "profiles", "batch_shape_sweep.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in out) + "\n]\n")


# ---- the filtered instantiations -----------------------------------------------------------------------------------
def _search_is_the_oracles(idx, kernel, c, ref, what, fails):
    """counts, ids and distance bits of one batched search are the oracle's, by the kernel asked for, nothing redone"""
    c0 = idx.counters()
    got = idx.search(c.qs, c.k, row_mask=None if c.keep is None else bsi.bits(c.keep))
    c1 = idx.counters()
    _check(fails, c1["batch_launches"] > c0["batch_launches"] and c1["batch_kernel_last"] == kernel, what + ": not batched by this kernel")
    _check(fails, np.array_equal(got[2], ref[2]), what + ": counts differ from the oracle's")
    if not _check(fails, np.array_equal(got[0], ref[0]), what + ": ids differ from the oracle's"):
        bad = np.nonzero(np.any(got[0] != ref[0], axis=1))[0]
        missing = sorted(set(ref[0][bad].ravel().tolist()) - set(got[0][bad].ravel().tolist()))
        fails.append("   queries %s; rows missing: %s" % (bad[:16].tolist(), missing[:32]))
    _check(fails, np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), what + ": distance bits differ from the oracle's")
    for name in QUIET:
        _check(fails, c1[name] == c0[name], "%s: %s moved: %d -> %d" % (what, name, c0[name], c1[name]))


def _oracle(oracle_mod, c):
    present = c.present
    mask = None if present.all() else bsi.bits(present)
    ref = oracle_mod.search_heap_many_mt(c.rows, c.qs, c.metric, c.k, None, mask)
    for queries, positions in c.groups:  # (the construction: the planted rows are the answer)
        own = set(np.asarray(positions)[present[np.asarray(positions)]].tolist())
        for q in queries:
            got = set(ref[0][q][:min(len(own), c.k)].tolist())
            assert got <= own, (q, got - own)
    return ref


def _run(idx, c):
    if not c.live.all():
        idx.set_deleted(np.nonzero(~c.live)[0])
    return idx


@pytest.mark.parametrize("metric", [L2, IP, COS])
@pytest.mark.parametrize("case", ["d=40", "d=160", "d=264", "d=40 row order", "d=40 tombstoned", "d=40 masked"])
def test_planted_neighbours_at_every_edge(hip_lib, oracle_mod, plan_lib, case, metric):
    d = int(case.split()[0][2:])
    variant = case.split()[-1] if case.split()[-1] in ("tombstoned", "masked") else "plain"
    kernels = (2,) if case.endswith("row order") else (0, 1, 2)
    fails = []
    for nq in NQS:
        rng = np.random.default_rng(100 * d + 10 * metric + nq)
        c, windows = bsi.planted_edges(rng, plan_lib, metric, d, nq, oracle_mod.normalize_f32, variant)
        for s0, n_sample in set(windows.values()):
            bsi.check(plan_lib, c, n_sample, s0)
        ref = _oracle(oracle_mod, c)
        for kernel in kernels:
            what = "%s %s %s nq=%d" % (case, METRIC_NAMES[metric], KERNEL_NAMES[kernel], nq)
            with _open(d, metric, c.rows, kernel, group=not case.endswith("row order")) as idx:
                _search_is_the_oracles(_run(idx, c), kernel, c, ref, what, fails)
    assert not fails, "%d checks missed:\n%s" % (len(fails), "\n".join(fails))


@pytest.mark.parametrize("nq", bsi.CROWD_NQS)
@pytest.mark.parametrize("flush", [None, "walk", "fast"])
@pytest.mark.parametrize("metric", [L2, COS])
def test_epilogue_crowds(hip_lib, oracle_mod, plan_lib, metric, flush, nq):
    rng = np.random.default_rng(300 + metric)
    c, n_sample = bsi.epilogue_crowds(rng, plan_lib, metric, oracle_mod.normalize_f32, flush, nq)
    bsi.check(plan_lib, c, n_sample)
    ref = _oracle(oracle_mod, c)
    fails = []
    with _open(c.d, metric, c.rows, 2, group=False) as idx:
        _search_is_the_oracles(_run(idx, c), 2, c, ref, "crowds %s flush=%s nq=%d" % (METRIC_NAMES[metric], flush, nq), fails)
    assert not fails, "%d checks missed:\n%s" % (len(fails), "\n".join(fails))


def _cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("metric", [L2, COS])
def test_persistent_loop_changes_query_tile(hip_lib, oracle_mod, plan_lib, metric):
    cus = _cus()
    print("compute units: %d" % cus)
    rng = np.random.default_rng(400 + metric)
    c, n_sample, second = bsi.persistent(rng, plan_lib, metric, cus, oracle_mod.normalize_f32)
    plan = plan_lib.plan(metric, c.d, len(c.rows), 2, len(c.qs), c.k, group=False)
    tiles = plan["nq_pad"] // plan["tile"] * -(-(len(c.rows) - n_sample) // plan["tile_n"])
    assert plan["nq_pad"] // plan["tile"] == 3 and tiles > cus and tiles % cus != 0
    assert any(changed for _, _, _, changed in second)
    bsi.check(plan_lib, c, n_sample)
    ref = _oracle(oracle_mod, c)
    fails = []
    with _open(c.d, metric, c.rows, 2, group=False) as idx:
        _search_is_the_oracles(idx, 2, c, ref, "persistent %s, %d CUs, %d tiles" % (METRIC_NAMES[metric], cus, tiles), fails)
    assert not fails, "%d checks missed:\n%s" % (len(fails), "\n".join(fails))


@pytest.mark.parametrize("metric", [L2, COS])
def test_persistent_loop_dense_keys(hip_lib, oracle_mod, plan_lib, metric):
    """the dense counterpart: 600 queries on a shard whose dense launch has 3 x ceil(rows / 256) tiles, more than CUs and
    no multiple of them -- every (query, row) key within its bound, as in test_dense_keys_every_pair"""
    cus = _cus()
    d, nq = 64, bsi.PERSISTENT_NQ
    n = (cus // 3 + 3) * 256 + 37
    tiles = 3 * -(-n // 256)
    assert tiles > cus and tiles % cus != 0 and nq * n <= 1 << 28
    assert plan_lib.plan(metric, d, n, 2, nq, K, group=False)["tile"] == 256
    rng = np.random.default_rng(500 + metric)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    if metric != COS:
        rows *= rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    if metric == COS:
        qs = np.stack([oracle_mod.normalize_f32(q) for q in qs])
    exact = bsi.exact_keys_many(rows, qs, metric)
    nrm = np.sqrt(np.einsum("ij,ij->i", rows.astype(np.float64), rows.astype(np.float64)))
    fails = []
    with _open(d, metric, rows, 2, group=False) as idx:
        _probe(idx, 2, metric, qs, exact, nrm, np.ones(n, bool), "persistent dense %s, %d CUs, %d tiles" % (METRIC_NAMES[metric], cus, tiles), fails)
    assert not fails, "\n".join(fails)
