"""GPU: the 4-bit first pass (TSH_OPT_SCAN_I4) far from unit magnitude -- the cases of tests/scale_inputs.py (rows times
2^er, queries times 2^eq, er = eq from -118 to 46, five mismatched pairs, and `mixed`) at d = 768 and d = 32, L2, dense,
the route forced as tests/test_gpu_scan_i4.py forces it.  scan_i4_band has refusal lines of its own and absolute terms
(the scale floor 2^-126, rho flushed, the underflow term) that a corpus of order 1 never meets.

test_scale_i4[case-d]:
  parity   always: counts, ids and distance bits are the oracle's on the scaled inputs;
  route    what scale_inputs.i4_facts works out on the CPU (asserted by tests/test_host_scale_inputs.py, never taken from
           the library): "demanded" -- query by query, the 4-bit scans and the int8 scans each advance by 1, nothing is
           redone, no wide-band fallback; "refused" -- the 4-bit stats do not move and the probe refuses; "free" -- parity
           alone, the counters are recorded;
  probe    for every query the header takes (ok): every side finite, the band positive, lower <= reduced key <= upper on
           every row, the key |v|^2 - 2 q.v summed in f64 (scale_inputs.reduced_keys); a query the header refuses must be
           refused by the probe.
The worst |key - exact| / w per case and width and the route taken go to profiles/scan_i4_scale_sweep.json."""
import json
import os

import numpy as np
import pytest

import scale_inputs as si
from scale_inputs import K, L2
from test_gpu_scan_i4 import _open

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULTS = {}


def _check(fails, cond, msg):
    if not cond:
        fails.append(msg)
    return bool(cond)


@pytest.mark.parametrize("d", si.WIDTHS)
@pytest.mark.parametrize("case", si.CASES)
def test_scale_i4(hip_lib, oracle_mod, case, d):
    from tostore_amd._ffi import TshError

    g = si.i4_facts(d, case)
    name = "d=%d %s" % (d, case)
    fails = []
    ref = oracle_mod.search_heap_many_mt(g.rows, g.qs, L2, K)
    rec = {"dim": d, "case": case, "table": g.route}
    with _open(d, L2, g.rows) as idx:
        first = idx.scan_i4_stats()
        for i, q in enumerate(g.qs):
            what = "%s query %d" % (name, i)
            a0, b0, c0 = idx.scan_i4_stats(), idx.scan_i8_stats(), idx.counters()
            got = idx.search(q[None, :], K)
            a1, b1, c1 = idx.scan_i4_stats(), idx.scan_i8_stats(), idx.counters()
            _check(fails, np.array_equal(got[2], ref[2][i:i + 1]), what + ": counts differ from the oracle's")
            _check(fails, np.array_equal(got[0], ref[0][i:i + 1]), what + ": ids differ from the oracle's")
            _check(fails, np.array_equal(got[1].view(np.uint64), ref[1][i:i + 1].view(np.uint64)), what + ": distance bits differ from the oracle's")
            if g.route == "demanded":
                _check(fails, a1["scans"] - a0["scans"] == 1, "%s: 4-bit scans %s -> %s" % (what, a0, a1))
                _check(fails, b1["scans"] - b0["scans"] == 1, "%s: int8 scans %s -> %s" % (what, b0, b1))
                _check(fails, b1["redone"] == b0["redone"], "%s: redone %s -> %s" % (what, b0, b1))
                _check(fails, c1["fallback_searches"] == c0["fallback_searches"], what + ": a wide-band fallback")
            if g.route == "refused":
                _check(fails, (a1["scans"], a1["survivors"], a1["rows_converted"]) == (a0["scans"], a0["survivors"], a0["rows_converted"]),
                       "%s: the 4-bit pass moved where the header refuses: %s -> %s" % (what, a0, a1))
        last = idx.scan_i4_stats()
        rec["taken"] = "4-bit x%d, %d survivors, %d denials" % (last["scans"] - first["scans"], last["survivors"] - first["survivors"], last["denials"])
        print("%s: table says %s (the model's survivors at most %s), took %s" % (name, g.route, g.survivors, rec["taken"]))
        worst = None
        for i, (q, ok) in enumerate(zip(g.qs, g.i4_ok)):
            what = "%s probe %d" % (name, i)
            try:
                lo, up = (x.astype(np.float64) for x in idx.probe_scan_i4_keys(q))
            except TshError as e:
                _check(fails, not ok, "%s: the probe refused a query inside the model: %s" % (what, e))
                continue
            if not _check(fails, ok, what + ": the probe ran where the header refuses"):
                continue
            if not _check(fails, np.all(np.isfinite(lo)) and np.all(np.isfinite(up)), what + ": a side is not finite"):
                continue
            _check(fails, np.all(up > lo), what + ": a band that is not positive")
            _check(fails, np.all(lo <= g.reduced[i]) and np.all(g.reduced[i] <= up), what + ": a reduced key outside [lower, upper]")
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst or 0.0, float(np.max(np.abs((lo + up) / 2 - g.reduced[i]) / ((up - lo) / 2))))
        rec["ratio"] = None if worst is None else round(worst, 4)
    RESULTS[(d, case)] = rec
    assert not fails, "%d checks missed:\n%s" % (len(fails), "\n".join(fails))


def test_zz_write_scale_sweep_i4():
    """(runs last in this file) the routes taken and the ratios of a whole sweep, for profiles/scan_i4_scale_sweep.json"""
    if set(RESULTS) != {(d, case) for d in si.WIDTHS for case in si.CASES}:
        return  # (a part of the sweep ran: the record of the whole one stays)
    with open(os.path.join(ROOT, "profiles", "scan_i4_scale_sweep.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(RESULTS[key]) for key in sorted(RESULTS, key=lambda x: (x[0], si.CASES.index(x[1])))) + "\n]\n")
