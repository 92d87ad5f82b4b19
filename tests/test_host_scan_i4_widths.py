"""CPU: what the 4-bit pass's width sweep (tests/test_gpu_scan_i4_widths.py) rests on.  Needs g++ and numpy only.

  1. The width list (tests/golden/scan_i4_width_sweep.json) is exactly the rule's (scan_i4_inputs.rule) and every member
     is a width the int8 family serves -- scan_i8_supported(pick_nch(ld / 4)) of tsh_scan_widths.h itself; the shapes it
     reaches: every tail length t = 1..7 under every ngf mod 4 with ngf < 4 (every prefetch clamped), ngf = 0, one and two
     full trips of the four-group buffer with and without a tail, pad elements inside ld, both sides of the inline-query
     edge (ld <= 960) with a tail, and the int8 family's widest rows.
  2. scan_i4_model.band equals tsh_scan_i4_band.h (tests/cpp/scan_i4_band_lib.cpp) bit for bit on the sweep's queries:
     the four Gaussian queries of every width, one-hot queries at the first and last element and the near-one-hot stand-in.
  3. A NumPy emulation of scan_i4_kernel's f32 chain order and epilogue (scan_i4_inputs.emulate) passes the sweep's
     checks (b) against the model at d = 1, 3, 4, 28, 30, 60, 100, 124, 228, 357, 957, 1000, 2044, 2048, Gaussian and
     one-hot queries alike: the two-sided bounds are the reference's own and are not tuned to the device.  Measured here:
     the emulation's keys stay within 0.16 of the model's margin and its bands within 0.25 of their tolerance.
  4. The same emulation with the kernel's tail group left out, or read against the query elements four places down, fails
     those checks at d = 1000 -- while its sides still hold every exact key of test_band_probe's rows: soundness alone does
     not see either fault.
  5. A nibble step of the element a position probe reads back is far above the model's margin (check (c) sees a single
     wrong code), for the one-hot query and for its stand-in."""
import json

import numpy as np
import pytest

import scan_i4_inputs as si4
import scan_i4_model as M

EMULATED = (1, 3, 4, 28, 30, 60, 100, 124, 228, 357, 957, 1000, 2044, 2048)


def test_the_list_is_the_rule():
    widths = json.load(open(si4.LIST))
    assert all(type(w) is int for w in widths) and widths == sorted(set(widths))
    assert set(widths) == si4.rule() and len(widths) == 55
    lib = si4.band_lib()
    for d in widths:
        ld, ngf, t = si4.shape(d)
        assert lib.scan_i4_width_ok(d) == 1, d
        assert lib.scan_i4_groups_of(d) == ngf + (t > 0), d
    assert lib.scan_i4_width_ok(2049) == 0  # the family ends at eight chunks of 256


def test_the_shapes_the_list_reaches():
    shapes = {d: si4.shape(d) for d in si4.WIDTHS}
    small = {(ngf, t) for _, ngf, t in shapes.values() if ngf < 4}
    assert small == {(ngf, t) for ngf in range(4) for t in range(8)} - {(0, 0)}
    assert {(ngf, t) for _, ngf, t in shapes.values() if 4 <= ngf <= 9} == {(ngf, t) for ngf in (4, 5, 8, 9) for t in (0, 7)}
    padded = {d for d in shapes if d % 4}
    assert padded == {1, 2, 3, 29, 30, 101, 125, 957, 961, 2045}
    inline = {d for d, (ld, _, t) in shapes.items() if ld <= si4.SCAN_Q_INLINE and ld > 900}
    assert inline == {956, 957, 960} and shapes[956][2] == 7 and shapes[957][2] == 0
    assert {d: shapes[d][2] for d in (961, 964, 992)} == {961: 1, 964: 1, 992: 0}  # the first widths past the edge, with a tail
    assert {shapes[d][1:] for d in (2044, 2045, 2048)} == {(63, 7), (64, 0)}


@pytest.mark.parametrize("d", si4.WIDTHS)
def test_model_band_is_the_headers(d):
    sh = si4.shard(d)
    qs = list(si4.corpus(d)[1]) + [si4.one_hot(d, 0), si4.one_hot(d, d - 1), si4.near_one_hot(d, d // 2)]
    for q in qs:
        ok, coef = si4.header_band(q, sh.max_norm, sh.max_abs)
        mine = M.band(q, sh.dim, sh.ld, sh.max_norm, sh.max_abs)
        assert ok
        assert [np.float32(v).view(np.uint32) for v in mine] == [v.view(np.uint32) for v in coef], (d, mine, coef)


def test_every_scan_of_the_sweep_runs():
    """The sweep's check (a) counts one 4-bit scan per query: no query of any width may leave more than the share of the
    rows to the int8 scan (two in a row would deny the route).  The model's upper counts are 10 .. 220 of 1061 rows."""
    most = {d: max(si4.shard(d).survivors(q, si4.K)[1] for q in si4.corpus(d)[1]) for d in si4.WIDTHS}
    print(most)
    assert max(most.values()) <= si4.SHARE_ROWS - 100 and si4.SHARE_ROWS == 339


@pytest.mark.parametrize("d", EMULATED)
def test_emulation_is_inside_the_bounds(d):
    sh = M.Shard(si4.corpus(d)[0])
    worst = {"key": 0.0, "band": 0.0, "sound": 0.0}
    fails = []
    for i, q in enumerate(list(si4.corpus(d)[1]) + [si4.one_hot(d, j) for j in si4.positions(d)[-3:]]):
        lo, up = si4.emulate(sh, q, M.band(q, sh.dim, sh.ld, sh.max_norm, sh.max_abs))
        r = si4.check_sides(lo, up, sh, q, "d=%d query %d" % (d, i), fails)
        worst = {key: max(worst[key], r[key]) for key in worst}
    print("d=%d: emulation within %.3f of the margin, %.3f of the band's tolerance; |key - exact| / w %.3f" % (d, worst["key"], worst["band"], worst["sound"]))
    assert not fails, "\n".join(fails)


def _wrong_emulation(sh, q, coef, fault):
    """the emulation of a kernel with a fault in its tail group (d = 1000: ngf = 31, the tail's eight elements 992..999)"""
    full = sh.ld // 32 * 32
    if fault == "skipped":
        q2 = np.array(q, np.float32)
        q2[full:] = 0.0  # no FMA of the tail group runs
        lo, up = si4.emulate(sh, q2, coef)
    else:
        q2 = np.array(q, np.float32)
        q2[full:] = q[full - 4:sh.dim - 4]  # the tail's codes against the query elements four places down
        lo, up = si4.emulate(sh, q2, coef)
    return lo, up


@pytest.mark.parametrize("fault", ["skipped", "shifted"])
def test_a_wrong_tail_fails_the_two_sided_checks_and_not_soundness(fault):
    d = 1000
    sh = si4.shard(d)
    q = si4.corpus(d)[1][0]
    coef = M.band(q, sh.dim, sh.ld, sh.max_norm, sh.max_abs)
    fails = []
    si4.check_sides(*_wrong_emulation(sh, q, coef, fault), sh, q, fault, fails)
    assert any("margin" in f for f in fails), fails
    fails = []
    j = 995  # a position probe inside the tail group
    e = si4.one_hot(d, j)
    si4.check_sides(*_wrong_emulation(sh, e, M.band(e, sh.dim, sh.ld, sh.max_norm, sh.max_abs), fault), sh, e, fault, fails)
    assert any("margin" in f for f in fails), fails
    # test_band_probe's own rows and query: every exact key still inside [lower, upper]
    rows, q, n_adv = si4.band_probe_rows(d, 4096)
    sh = M.Shard(rows)
    lo, up = _wrong_emulation(sh, q, M.band(q, sh.dim, sh.ld, sh.max_norm, sh.max_abs), fault)
    exact = sh.exact_keys(q)
    lo, up = lo.astype(np.float64), up.astype(np.float64)
    ratio = np.abs((lo + up) / 2 - exact) / ((up - lo) / 2)
    print("%s: worst |key - exact| / w on test_band_probe's rows %.3f" % (fault, ratio.max()))
    assert np.all(lo <= exact) and np.all(exact <= up) and ratio[:n_adv].max() >= 0.85


@pytest.mark.parametrize("d", [3, 100, 1000, 2045])
def test_a_nibble_step_is_far_above_the_margin(d):
    sh = si4.shard(d)
    lowest = float("inf")
    for j in si4.positions(d):
        for q in (si4.one_hot(d, j), si4.near_one_hot(d, j)):
            step = si4.nibble_step_in_margins(sh, q, j)
            lowest = min(lowest, step)
            assert step > 10.0, (d, j)
    print("d=%d: a nibble step is at least %.0f margins" % (d, lowest))
