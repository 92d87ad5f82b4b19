"""GPU: the 4-bit first pass (scan_i4_kernel<4>, rows4_convert_kernel: tostore_amd/csrc/tsh_scan_i4.hip.h) held to its
NumPy model at every row shape, and through growth, an overwrite and odd rows in sequence.

The kernel works in groups of 32 elements, four groups to a register buffer, two buffers, loads past the last group
clamped to it; a row that ends inside a group takes tail >> 2 of its eight quads.  The width list --
tests/golden/scan_i4_width_sweep.json, held to its rule by tests/test_host_scan_i4_widths.py -- reaches every tail length
under every ngf mod 4, rows shorter than one group, one and two full trips of the buffer, pad elements inside ld, both
sides of the edge where the query stops riding in the argument segment, and the int8 family's widest rows.  Each width
is one test (L2, dense, the route forced, 16 tiles and one of 37 rows, capacity = rows; the corpus of
scan_i4_inputs.corpus: Gaussian rows with a zero row, a row of one element, a row of +-max and a row of 2^-100):

  (a) search: 4 queries one by one at k = 10 -- counts, ids and distance bits are the oracle's and those of an index with
      the pass switched off; per query the 4-bit scans and the int8 scans advance by 1, nothing is redone, no wide-band
      fallback; the survivors reported lie within the model's (at least, at most).  That every scan runs is a property of
      the inputs: where the model's upper survivor count is at most 0.32 N = 339 rows for every query, one index serves
      all four; where it is not (narrow rows: the band is as wide as the keys) a fresh index serves each pair of queries
      -- the deny rule cannot act before the third scan.
  (b) dense probes: the same 4 queries through probe_scan_i4_keys on every row -- every side finite, up > lo,
      lo <= exact <= up, and two-sided against the model (scan_i4_inputs.check_sides): the key within the model's margin,
      the band within 1e-6 w + 2^-23 max(|lo|, |up|).
  (c) position probes: one-hot queries e_j at j = 0..7, 28..31, the first and last element of the last full group, every
      element of the tail group and d - 1, held to (b)'s checks.  With |q|_1 = 1 one nibble step of element j is hundreds
      to thousands of margins on every row of ordinary magnitude (test_host_scan_i4_widths.py): the plane is read back
      element by element.  The library takes one-hot queries; were one refused, e_j + 2^-12 g (g Gaussian) stands in, its
      nibble step asserted on the CPU to stay above 10 margins.
  (d) adversarial rows: test_band_probe's rows at this width (7.49 codes off every nibble's midpoint with the sign of q_j,
      one element pinning the scale): the band is sound, and from d = 32 on the worst |key - exact| / w is at least 0.85
      (below, the pinned element dominates the row).

Every miss of a width is collected and asserted at its end.  The worst ratios per width and check go to
profiles/scan_i4_width_sweep.json when the whole list ran.

test_growth_and_odd_rows: one index at d = 100 through open at capacity 1024, 1000 rows, a search, 600 more (growth past
the capacity: rho lives at cap x groups x 16 inside the copy), an overwrite in the last tile, a zero row and a plain append, with
parity, (b) against a fresh model and the rows converted after each step.

Carried out once on scratch builds, neither of them kept: a library whose kernel skips the part-filled last group, and one
that reads it against the query elements four places down, both at d = 1000 (ngf = 31, a tail of two quads).
run_width(1000) on the unchanged library: no miss.  The group skipped: all four dense probes miss (b) -- the keys of 1053
of 1061 rows off the model's by up to 65 margins --, the position probes e_992 .. e_999, the tail's eight elements, miss
(c) with the exact keys of nearly every row outside [lower, upper], and three queries' survivors leave the model's
count by one row; the searches' answers stay right.  The group read four places down: all four dense probes miss (b), by
up to 139 margins, and e_991 .. e_999 miss (c).  test_gpu_scan_i4.test_band_probe passed on both: at d = 1000 its worst
|key - exact| / w went from 0.8794 to 0.9785 and 0.9793, still inside the band."""
import json
import os

import numpy as np
import pytest

import scan_i4_inputs as si4
import scan_i4_model as M
from scan_i4_inputs import K, N
from test_gpu_scan_i4 import L2, _open

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULTS = {}


def _check(fails, cond, msg):
    if not cond:
        fails.append(msg)
    return bool(cond)


def _parity(got, ref, what, fails):
    _check(fails, np.array_equal(got[2], ref[2]), what + ": counts differ")
    _check(fails, np.array_equal(got[0], ref[0]), what + ": ids differ")
    _check(fails, np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), what + ": distance bits differ")


def _worse(a, b):
    return {key: max(a.get(key, 0.0), b[key]) for key in b}


def _searches(d, rows, qs, sh, oracle_mod, fails):
    """Check (a).  Returns the survivors the device reported, per query."""
    name = "d=%d search" % d
    ref = oracle_mod.search_heap_many_mt(rows, qs, L2, K)
    most = [sh.survivors(q, K)[1] for q in qs]
    groups = [range(len(qs))] if max(most) <= si4.SHARE_ROWS else [range(0, 2), range(2, 4)]
    print("%s: the model's upper survivor counts %s of %d rows: %d index(es)" % (name, most, N, len(groups)))
    with _open(d, L2, rows, i4=0) as off:
        got_off = off.search(qs, K)
        _check(fails, off.scan_i4_stats()["scans"] == 0, name + ": the pass ran with option 0")
    _parity(got_off, ref, name + " (option 0 against the oracle)", fails)
    kept = []
    for group in groups:
        with _open(d, L2, rows) as idx:
            for i in group:
                what = "%s query %d" % (name, i)
                a0, b0, c0 = idx.scan_i4_stats(), idx.scan_i8_stats(), idx.counters()
                got = idx.search(qs[i][None, :], K)
                a1, b1, c1 = idx.scan_i4_stats(), idx.scan_i8_stats(), idx.counters()
                _parity(got, tuple(x[i:i + 1] for x in ref), what + " (oracle)", fails)
                _parity(got, tuple(x[i:i + 1] for x in got_off), what + " (option 0)", fails)
                _check(fails, a1["scans"] - a0["scans"] == 1, "%s: 4-bit scans %s -> %s" % (what, a0, a1))
                _check(fails, b1["scans"] - b0["scans"] == 1, "%s: int8 scans %s -> %s" % (what, b0, b1))
                _check(fails, b1["redone"] == b0["redone"], "%s: redone %s -> %s" % (what, b0, b1))
                _check(fails, c1["fallback_searches"] == c0["fallback_searches"], what + ": a wide-band fallback")
                least, upper = sh.survivors(qs[i], K)
                total = a1["survivors"] - a0["survivors"]
                kept.append(total)
                _check(fails, least <= total <= upper, "%s: %d survivors, the model says %d..%d" % (what, total, least, upper))
    return kept


def _probe(idx, sh, q, what, fails, j=None):
    """(b) / (c) for one query; j: the element a one-hot query reads back"""
    from tostore_amd._ffi import TshError

    try:
        lo, up = idx.probe_scan_i4_keys(q)
    except TshError as e:
        if j is None:
            fails.append("%s: the probe refused: %s" % (what, e))
            return None
        q = si4.near_one_hot(sh.dim, j)
        assert si4.nibble_step_in_margins(sh, q, j) > 10.0
        what += " (e_j + 2^-12 g)"
        lo, up = idx.probe_scan_i4_keys(q)
    return si4.check_sides(lo, up, sh, q, what, fails)


def run_width(d, oracle_mod, fails):
    """Everything test_width holds one width to; returns the width's record."""
    rows, qs = si4.corpus(d)
    sh = si4.shard(d)
    ld, ngf, t = si4.shape(d)
    rec = {"dim": d, "ngf": ngf, "t": t}
    rec["survivors"] = _searches(d, rows, qs, sh, oracle_mod, fails)
    dense, position = {}, {}
    with _open(d, L2, rows) as idx:
        for i, q in enumerate(qs):
            r = _probe(idx, sh, q, "d=%d dense probe %d" % (d, i), fails)
            dense = _worse(dense, r) if r else dense
        for j in si4.positions(d):
            r = _probe(idx, sh, si4.one_hot(d, j), "d=%d position probe e_%d" % (d, j), fails, j)
            position = _worse(position, r) if r else position
    rec.update({"dense_" + key: round(v, 4) for key, v in dense.items()})
    rec.update({"position_" + key: round(v, 4) for key, v in position.items()})
    arows, aq, n_adv = si4.band_probe_rows(d)
    exact = M.Shard(arows).exact_keys(aq)
    with _open(d, L2, arows) as idx:
        lo, up = (x.astype(np.float64) for x in idx.probe_scan_i4_keys(aq))
    what = "d=%d adversarial rows" % d
    if _check(fails, np.all(np.isfinite(lo)) and np.all(np.isfinite(up)) and np.all(up > lo), what + ": a side is not finite, or no band"):
        ratio = np.abs((lo + up) / 2 - exact) / ((up - lo) / 2)
        rec["adversarial"], rec["adversarial_spread_rows"] = round(float(ratio[:n_adv].max()), 4), round(float(ratio[n_adv:].max()), 4)
        _check(fails, np.all(lo <= exact) and np.all(exact <= up), "%s: an exact key outside [lower, upper]: %.4f" % (what, ratio.max()))
        if d >= 32:
            _check(fails, ratio[:n_adv].max() >= 0.85, "%s: the worst ratio is %.4f: a slack band" % (what, ratio[:n_adv].max()))
    print("d=%d: %s" % (d, rec))
    return rec


@pytest.mark.parametrize("d", si4.WIDTHS)
def test_width(hip_lib, oracle_mod, d):
    fails = []
    RESULTS[d] = run_width(d, oracle_mod, fails)
    assert not fails, "%d checks missed:\n%s" % (len(fails), "\n".join(fails))


def test_growth_and_odd_rows(hip_lib, oracle_mod):
    """One index, d = 100 (three full groups and a tail of one quad), in this order: open at capacity 1024; 1000 rows; a
    search; 600 more -- past the capacity: the row store and with it the copies are made anew; an overwrite in the last
    tile (1600 rows are 25 full tiles: the ragged last tile is the zero row's); a zero row; 30 rows more.  After each step
    parity with the oracle, check (b) against a fresh model of the rows as they stand, and rows_converted advancing by
    what row_copy_ensure's watermark says: everything after a growth or an overwrite, only the new rows after a plain
    append.  The row store grows to exactly the rows it is asked for, so the zero row is a second growth (the capacity is
    read from the plane's bytes: groups x 16 + 4 a row) and the 30 rows behind it are the plain append.
    (The conversion is counted over the search and the probes together: whichever comes first converts.)"""
    d = 100
    per_row = 4 * 16 + 4  # four groups of 16 bytes and rho
    rng = np.random.default_rng(4100)
    rows, qs = M.spread_corpus(rng, 1631, d)
    rows[1600] = 0.0
    fails = []
    plain = []
    with _open(d, L2, rows[:0], capacity=1024) as idx:
        def step(n, what, new_rows=None):
            """new_rows: rows appended behind the last one (None: an overwrite)"""
            s0 = idx.scan_i4_stats()
            fits = new_rows is not None and s0["copy_bytes"] > 0 and n <= s0["copy_bytes"] // per_row
            fresh = new_rows if fits else n
            plain.append(fits)
            got = idx.search(qs, K)
            _parity(got, oracle_mod.search_heap_many_mt(rows[:n], qs, L2, K), what, fails)
            sh = M.Shard(rows[:n])
            for i, q in enumerate(qs):
                _probe(idx, sh, q, "%s, probe %d" % (what, i), fails)
            s1 = idx.scan_i4_stats()
            print("%s: %s -> %s" % (what, s0, s1))
            _check(fails, s1["rows_converted"] - s0["rows_converted"] == fresh, "%s: %d rows converted, the rule says %d" % (what, s1["rows_converted"] - s0["rows_converted"], fresh))
            _check(fails, s1["scans"] > s0["scans"], what + ": no 4-bit scan ran")

        idx.append(0, rows[:1000])
        step(1000, "1000 rows", 1000)
        idx.append(1000, rows[1000:1600])
        step(1600, "600 more, past the capacity", 600)
        r = 1590
        rows[r] = (qs[1] + 0.01 * rng.standard_normal(d)).astype(np.float32)
        idx.append(r, rows[r:r + 1])
        step(1600, "an overwrite in the last tile")
        idx.append(1600, rows[1600:1601])
        step(1601, "a zero row in a tile of its own", 1)
        idx.append(1601, rows[1601:1631])
        step(1631, "30 rows more, inside the capacity", 30)
    _check(fails, plain == [False, False, False, False, True], "which appends fit the capacity: %s" % plain)
    assert not fails, "%d checks missed:\n%s" % (len(fails), "\n".join(fails))


def test_zz_write_width_sweep():
    """(runs last in this file) the ratios of a whole sweep, for profiles/scan_i4_width_sweep.json"""
    if set(RESULTS) != set(si4.WIDTHS):
        return  # (a part of the sweep ran: the record of the whole one stays)
    with open(os.path.join(ROOT, "profiles", "scan_i4_width_sweep.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(RESULTS[d]) for d in sorted(RESULTS)) + "\n]\n")
