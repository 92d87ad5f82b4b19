"""Inputs and checks of the 4-bit first pass's width sweep (tests/test_gpu_scan_i4_widths.py), usable without a GPU
(tests/test_host_scan_i4_widths.py): the width list and the rule it is written by, the sweep's corpus, the header's band
through a library of its own (tests/cpp/scan_i4_band_lib.cpp, g++), a NumPy emulation of scan_i4_kernel's f32 arithmetic
in the kernel's own order, and the checks a pair of sides -- the device's or the emulation's -- is held to.

scan_i4_kernel<4> works in groups of 32 elements, four groups to a register buffer, two buffers, loads past the last
group clamped to it; a row that ends inside a group takes tail >> 2 of its eight quads.  With ld = round_up(d, 4) a row's
shape is ngf = ld / 32 against the buffer depth, ngf mod 4, and t = (ld mod 32) / 4.

The two-sided checks against the model (scan_i4_model.Shard.key_and_band: key x, band w, margin) on sides (lo, up):
  key    |(lo + up) / 2 - x| <= margin
  band   |(up - lo) / 2 - w| <= 1e-6 w + 2^-23 max(|lo|, |up|)
The second tolerance is derived, not measured: the model's own 1e-6 w for forming w in f32, plus the two roundings by
which the probe hands w over as lower + 2 w (lower = fl(x - w), upper = fl(lower + 2 w): 2^-24 of either side each)."""
import ctypes
import functools
import json
import os
import subprocess
import tempfile

import numpy as np

import scan_i4_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST = os.path.join(ROOT, "tests", "golden", "scan_i4_width_sweep.json")
WIDTHS = json.load(open(LIST))
TILE = 64
N = 16 * TILE + 37
NQ, K = 4, 10
SHARE_ROWS = int(M.MAX_SHARE * N)  # 339: two scans in a row above it and the route is denied
SCAN_Q_INLINE = 960  # tsh_kernels.hip.h: up to here the query rides in the kernel-argument segment
ZERO_ROW, ONE_ROW, MAX_ROW, TINY_ROW = 5, 7 * TILE + 63, N - 1, 3 * TILE


def rule():
    """The list's rule (ld = round_up(d, 4), ngf = ld / 32, t = (ld mod 32) / 4)."""
    want = {32 * ngf + 4 * t for ngf in range(4) for t in range(8)} - {0}  # every tail under every ngf mod 4, all clamped
    assert len(want) == 31 and min(want) == 4 and max(want) == 124
    want |= {32 * ngf + 4 * t for ngf in (4, 5, 8, 9) for t in (0, 7)}  # one and two full trips of the buffer
    want |= {1, 2, 3, 29, 30, 101, 125}  # pad elements inside ld
    want |= {956, 957, 960, 961, 964, 992}  # the inline-query edge
    want |= {2044, 2045, 2048}  # the top of the int8 family
    return want


def shape(d):
    """(ld, ngf, t)"""
    ld = (d + 3) // 4 * 4
    return ld, ld // 32, (ld % 32) // 4


@functools.lru_cache(maxsize=1)
def band_lib():
    """tsh_scan_i4_band.h and tsh_scan_widths.h by g++"""
    workdir = tempfile.mkdtemp(prefix="scan_i4_band_")
    so = os.path.join(workdir, "libscan_i4_band.so")
    src = os.path.join(ROOT, "tests", "cpp", "scan_i4_band_lib.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    fp = ctypes.POINTER(ctypes.c_float)
    lib.scan_i4_band_of.restype = ctypes.c_int
    lib.scan_i4_band_of.argtypes = [ctypes.c_int, fp, ctypes.c_float, ctypes.c_float, fp]
    lib.scan_i4_width_ok.restype = ctypes.c_int
    lib.scan_i4_width_ok.argtypes = [ctypes.c_int]
    lib.scan_i4_groups_of.restype = ctypes.c_int
    lib.scan_i4_groups_of.argtypes = [ctypes.c_int]
    return lib


def header_band(q, max_norm, max_abs):
    """(ok, (a_s, a_r, a_c, a_v, beta, qbias)) of scan_i4_band itself"""
    q = np.ascontiguousarray(q, np.float32)
    out = (ctypes.c_float * 6)()
    ok = band_lib().scan_i4_band_of(len(q), q.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), float(max_norm), float(max_abs), out)
    return bool(ok), tuple(np.float32(v) for v in out)


@functools.lru_cache(maxsize=4)
def corpus(d, n=N):
    """(rows, queries) of one width: Gaussian rows of norms U(0.5, 2), four of them replaced -- a zero row (scale floor
    2^-126, rho tiny), a row with one non-zero element, the last, a row of +-max (codes +-127: nibbles 15 and 0) and a row
    2^-100 of the others.  Read-only: shared by the tests of a width."""
    rng = np.random.default_rng(7000 + d)
    rows, qs = M.spread_corpus(rng, n, d)
    rows[ZERO_ROW] = 0.0
    rows[ONE_ROW] = 0.0
    rows[ONE_ROW, d - 1] = -1.25
    rows[MAX_ROW] = np.where(rng.random(d) < 0.5, -1.75, 1.75).astype(np.float32)
    rows[TINY_ROW] = (rng.standard_normal(d) * 2.0 ** -100).astype(np.float32)
    rows.setflags(write=False)
    qs.setflags(write=False)
    return rows, qs


@functools.lru_cache(maxsize=4)
def shard(d):
    return M.Shard(corpus(d)[0])


def band_probe_rows(d, n=N):
    """test_gpu_scan_i4.test_band_probe's rows at this width: (rows, q, adversarial rows' count).  The first half sits 7.49
    codes off every nibble's midpoint with the sign of q_j (the L1 side's worst case), one element pinning the scale."""
    rng = np.random.default_rng(9400 + d)
    rows, qs = M.spread_corpus(rng, n, d, nq=1)
    q = qs[0]
    s0 = np.ldexp(1.0, -rng.integers(0, 12, size=n // 2))[:, None]
    nib = rng.integers(1, 15, size=(n // 2, d))
    adv = ((16 * nib + 8 - 128) + np.where(q > 0, 7.49, -7.49)[None, :]) * s0
    adv[np.arange(n // 2), np.arange(n // 2) % d] = 127.0 * s0[:, 0]  # pins every row's scale to its s0
    rows[: n // 2] = adv.astype(np.float32)
    return rows, q, n // 2


def positions(d):
    """Elements a one-hot query reads back: 0..7, 28..31, the first and last element of the last full group, every element
    of the tail group, and d - 1."""
    ld, ngf, t = shape(d)
    js = set(range(8)) | set(range(28, 32)) | {d - 1}
    if ngf:
        js |= {32 * (ngf - 1), 32 * ngf - 1}
    js |= set(range(32 * ngf, d))
    return sorted(j for j in js if j < d)


def one_hot(d, j):
    q = np.zeros(d, np.float32)
    q[j] = 1.0
    return q


def near_one_hot(d, j):
    """e_j + 2^-12 g, g Gaussian: for a library that refuses a one-hot query"""
    q = (np.random.default_rng(31 * d + j).standard_normal(d) * 2.0 ** -12).astype(np.float32)
    q[j] += np.float32(1.0)
    return q


def nibble_step_in_margins(sh, q, j):
    """One nibble step of element j -- 16 s_i |q_j| in the dot, twice that in the key -- in units of the model's margin:
    the smallest over the rows of ordinary magnitude (the zero row and the row of 2^-100 have no step to speak of beside
    the band's absolute terms)."""
    _, _, margin = sh.key_and_band(q)
    s = sh.s.astype(np.float64)
    rows = s > 2.0 ** -20
    return float(np.min(32.0 * s[rows] * abs(float(q[j])) / margin[rows]))


def emulate(sh, q, coef):
    """(lower, upper) as tsh_probe_scan_i4_keys hands them over, by scan_i4_kernel's own f32 arithmetic in its own order:
    four chains, chain c taking the elements j = c mod 4 in ascending order (quad i of a group is its elements 4 i .. 4 i +
    3, byte b on chain b), every step one f32 FMA; the chains added as (0 + 1) + (2 + 3); t = fma(16, sum, -qbias);
    dot = fl(s t); key = fma(-2, dot, sq); w as scan_i4_w; lower = fl(key - w), upper = fl(lower + 2 w).  An FMA is formed
    in f64 and rounded to f32: nibble x f32 is exact there and the sum is good to 2^-53, so the double rounding can
    differ from the device's single one only at an exact f64 tie -- never by more than the last f32 bit."""
    a_s, a_r, a_c, a_v, beta, qb = (np.float32(v) for v in coef)
    f32, f64 = np.float32, np.float64
    qp = np.zeros(sh.ld, f64)
    qp[:sh.dim] = np.asarray(q, f32)
    h = np.full((sh.n, sh.ld), 8.0)  # (pad elements: the code of zero, against a zero of the staged query)
    h[:, :sh.dim] = sh.h
    acc = np.zeros((sh.n, 4), f32)
    for j0 in range(0, sh.ld, 4):
        acc = (h[:, j0:j0 + 4] * qp[j0:j0 + 4] + acc.astype(f64)).astype(f32)
    total = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    t = (16.0 * total.astype(f64) - f64(qb)).astype(f32)
    dot = sh.s * t
    x = (sh.sq.astype(f64) - 2.0 * dot.astype(f64)).astype(f32)
    alt = (f64(a_r) * sh.rho.astype(f64) + (a_c * sh.s).astype(f64)).astype(f32)
    wq = np.minimum(a_s * sh.s, alt)
    w = wq + (f64(a_v) * np.sqrt(sh.sq).astype(f64) + f64(beta)).astype(f32)
    lower = (x - w).astype(f32)
    return lower, (lower + f32(2.0) * w).astype(f32)


def check_sides(lo, up, sh, q, what, fails, exact=None):
    """Checks (b) / (c) of the sweep for one query: every side finite, up > lo, lo <= exact <= up, and the two-sided
    checks of the module docstring.  Misses are appended to `fails`.  Returns the worst ratios {"sound": |mid - exact| / w,
    "key": |mid - x| / margin, "band": |w - w_model| / its tolerance}."""
    lo, up = np.asarray(lo, np.float64), np.asarray(up, np.float64)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(up))):
        fails.append(what + ": a side is not finite")
        return {"sound": float("inf"), "key": float("inf"), "band": float("inf")}
    exact = sh.exact_keys(q) if exact is None else exact
    x, w, margin = sh.key_and_band(q)
    mid, half = (lo + up) / 2, (up - lo) / 2
    if not np.all(up > lo):
        fails.append("%s: %d rows without a positive band" % (what, int(np.sum(~(up > lo)))))
    out_of = ~((lo <= exact) & (exact <= up))
    if out_of.any():
        fails.append("%s: the exact key of %d rows lies outside [lower, upper], first row %d" % (what, int(out_of.sum()), int(np.argmax(out_of))))
    r_key = np.abs(mid - x) / margin
    r_band = np.abs(half - w) / (1e-6 * w + 2.0 ** -23 * np.maximum(np.abs(lo), np.abs(up)))
    if not np.all(r_key <= 1.0):
        i = int(np.argmax(r_key))
        fails.append("%s: the key of %d rows is off the model's by more than its margin, worst row %d by %.3g margins" % (what, int(np.sum(~(r_key <= 1.0))), i, r_key[i]))
    if not np.all(r_band <= 1.0):
        i = int(np.argmax(r_band))
        fails.append("%s: the band of %d rows is off the model's by more than its tolerance, worst row %d by %.3g" % (what, int(np.sum(~(r_band <= 1.0))), i, r_band[i]))
    with np.errstate(divide="ignore", invalid="ignore"):
        sound = float(np.max(np.abs(mid - exact) / half))
    return {"sound": sound, "key": float(r_key.max()), "band": float(r_band.max())}
