"""A NumPy model of the 4-bit first pass (tostore_amd/csrc/tsh_scan_i4.hip.h), restated from tsh_scan_i4_band.h: the int8
copy's scales and codes, the high nibbles, rho, the band's coefficients, every row's lower and upper side, the threshold
from the tile minima of the upper sides, and the rows that survive.  The device forms the nibble sum in f32 chains; the
model forms it exactly (f64 over integers times f32 is exact to ~2^-53) and carries a margin per row for the difference,
so it returns the survivors as a pair (at least, at most)."""
import numpy as np

U = 2.0 ** -24
U2 = 2.0 ** -23
TINY = 1.17549435e-38
GROUP = 32
MAX_SHARE = 0.32  # SCAN_I4_MAX_SHARE, tsh_lib.hip: the measured break-even less the spread


def int8_copy(rows):
    """(scale, biased bytes) as rows8_convert_kernel makes them: f32 arithmetic throughout."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    mx = np.abs(rows).max(axis=1).astype(np.float32)
    s = (mx / np.float32(127.0)).astype(np.float32)
    low = s.astype(np.float64) * 127.0 < mx.astype(np.float64)
    s = np.where(low, np.nextafter(s, np.float32(np.inf)), s).astype(np.float32)
    s = np.maximum(s, np.float32(TINY))
    c = np.clip(np.rint((rows / s[:, None]).astype(np.float32)), -127, 127)
    return s, (c + 128).astype(np.uint8)


def nibbles(biased):
    return (biased >> 4).astype(np.int64)


def rho_of(rows, s, h):
    """|v_i - recon4_i|_2 over the row's dim elements, rounded up, as rows4_convert_kernel sums it: the pad elements up to
    ld (code 8: 8 s_i each) meet no query element and are left out."""
    recon = (16 * h + 8 - 128).astype(np.float64) * s.astype(np.float64)[:, None]
    r = np.sqrt(((rows.astype(np.float64) - recon) ** 2).sum(axis=1)) * (1.0 + 1e-6)
    f = r.astype(np.float32)
    return np.where(f.astype(np.float64) < r, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def _up(x):
    f = np.float32(x)
    return np.nextafter(f, np.float32(np.inf)) if float(f) < x else f


def band(q, dim, ld, max_norm, max_abs):
    """scan_i4_band: (a_s, a_r, a_c, a_v, beta, qbias), f32 -- the header's values bit for bit (test_host_scan_i4_widths.py):
    the three sums over q run element by element, as the header's loop does."""
    q64 = np.asarray(q, dtype=np.float64)[:dim]
    groups = (ld + GROUP - 1) // GROUP
    q1, qs, qn2 = (np.add.accumulate(x)[-1] for x in (np.abs(q64), q64, q64 * q64))
    qn = np.sqrt(qn2) * (1.0 + 1e-6)
    smax = float(max_abs) / 127.0 * (1.0 + 1e-6)
    gam = (8.0 * groups + 8.0) * U2
    kar = 256.0 * gam + 512.0 * U
    kap4 = 8.5 + 2.0 ** -16 + kar
    under = TINY * ((dim + 4.0) * smax + 2.0 + 2.0 * q1 + qn)
    mx = float(max_norm) * (1.0 + 1e-6)
    g64 = (dim + 4.0) * 2.0 ** -52
    a_s, a_r, a_c = 2.0 * kap4 * q1, 2.0 * qn, 2.0 * kar * q1
    a_v = U2 * (3.0 * mx + 4.0 * qn) + g64 * mx
    beta = 2.0 * under + g64 * qn * (qn + 2.0 * mx)
    return tuple(_up(x * 1.001) for x in (a_s, a_r, a_c, a_v, beta)) + (np.float32(120.0 * qs),)


class Shard:
    """What the conversion leaves per shard: shared by the queries of a test."""

    def __init__(self, rows):
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.n, self.dim = self.rows.shape
        self.ld = (self.dim + 3) // 4 * 4
        self.s, biased = int8_copy(self.rows)
        self.h = nibbles(biased)
        self.rho = rho_of(self.rows, self.s, self.h)
        r64 = self.rows.astype(np.float64)
        self.sq = np.einsum("ij,ij->i", r64, r64).astype(np.float32)
        self.max_norm = np.float32(np.sqrt(self.sq.astype(np.float64).max()) * (1 + 1e-6))
        self.max_abs = np.abs(self.rows).max()

    def sides(self, q):
        """(lower, upper, margin) per row, f64: margin covers the device's f32 chain and epilogue against this model's."""
        x, w, margin = self.key_and_band(q)
        return x - w, x + w, margin

    def key_and_band(self, q):
        """(key, band, margin) per row, f64: the middle of [lower, upper] and half its width."""
        a_s, a_r, a_c, a_v, beta, qb = (float(x) for x in band(q, self.dim, self.ld, self.max_norm, self.max_abs))
        q64 = np.asarray(q, dtype=np.float64)
        acc = self.h.astype(np.float64) @ q64
        s, rho, sq = (x.astype(np.float64) for x in (self.s, self.rho, self.sq))
        dot = s * (16.0 * acc - qb)
        x = sq - 2.0 * dot
        w = np.minimum(a_s * s, a_r * rho + a_c * s) + a_v * np.sqrt(sq) + beta
        # the device's own roundings: the chain, the bias, the scale (a_c s covers twice their sum), four epilogue roundings
        margin = a_c * s + 4.0 * U2 * (np.abs(x) + w) + 1e-6 * w
        return x, w, margin

    def survivors(self, q, k):
        """(at least, at most) rows whose lower side is at or below tau = the k-th smallest tile minimum of upper sides;
        fewer than k tiles: every row."""
        lo, up, m = self.sides(q)
        n_tiles = (self.n + 63) // 64
        if n_tiles < k:
            return self.n, self.n
        pad = n_tiles * 64 - self.n
        tmin_lo = np.pad(up - m, (0, pad), constant_values=np.inf).reshape(n_tiles, 64).min(axis=1)
        tmin_hi = np.pad(up + m, (0, pad), constant_values=np.inf).reshape(n_tiles, 64).min(axis=1)
        tau_lo, tau_hi = np.partition(tmin_lo, k - 1)[k - 1], np.partition(tmin_hi, k - 1)[k - 1]
        return int((lo + m <= tau_lo).sum()), int((lo - m <= tau_hi).sum())

    def exact_keys(self, q):
        r64, q64 = self.rows.astype(np.float64), np.asarray(q, dtype=np.float64)
        return np.einsum("ij,ij->i", r64, r64) - 2.0 * (r64 @ q64)


def spread_corpus(rng, n, d, nq=4, lo=0.5, hi=2.0):
    """The headline's kind of corpus: Gaussian rows whose norms differ by a factor U(lo, hi)."""
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows *= rng.uniform(lo, hi, size=(n, 1)).astype(np.float32)
    return rows, rng.standard_normal((nq, d)).astype(np.float32)


def unit_corpus(rng, n, d, nq=4):
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True).astype(np.float32)
    return rows, rng.standard_normal((nq, d)).astype(np.float32)
