"""Inputs of tests/test_gpu_batch_shapes.py, and the properties those tests rest on, checkable without a GPU
(tests/test_host_batch_shape_inputs.py runs every builder and every check here).

Everything the constructions need to know about a batched call -- the sample's size and place, the workgroup tiles, the
candidate cap, the order of the tiles, the keys' error bounds -- comes from tsh_batch_plan.h and tsh_batch_tiles.h
themselves, compiled by g++ (tests/cpp/batch_plan_lib.cpp), never from the library under test.

A construction is a corpus of Gaussian filler rows, Gaussian queries, and PLANTED rows: a group of near-equal queries
(usually one) owns a set of positions, and the row at each is lam * q + noise -- nearer to the group's queries than any
filler row by a wide gap.  check() proves from f64 keys alone that
  1. for every owning query the live, kept rows it owns are the top of its exact ranking, the best other row at least
     8 D behind (D: the widest bound any of the three key kernels claims for a key of this query, batch_delta2) -- so
     each of them is a CERTAIN survivor of the filtered pass: its key is below the k-th smallest, which the threshold
     covers;
  2. at least half of the planted rows lie outside the sample window;
  3. for every query, the rows whose exact key is within 4 D of the k-th smallest exact key of the sample window's
     live rows number less than cand_cap / 2: no candidate list can overflow, so nothing may be redone.
"""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, IP, COS = 0, 1, 2
METRIC_NAMES = ("l2", "ip", "cosine")
K = 8
N_PLANTED = 8192 + 60 * 256 + 37  # a sample, 60 whole tiles of the filtered pass and a ragged one


def f16_hits():
    """entries of a wave's hit list in the fp16 kernel's epilogue (tsh_batch_f16.hip.h)"""
    text = open(os.path.join(ROOT, "tostore_amd", "csrc", "tsh_batch_f16.hip.h")).read()
    return int(re.search(r"constexpr\s+int\s+F16_HITS\s*=\s*(\d+)\s*;", text).group(1))


class PlanLib:
    FIELDS = ("tile", "nq_pad", "kern", "hchunks", "tile_n", "n_sample", "k_est", "cand_cap", "want_group", "listed", "scan_rows")

    def __init__(self, workdir):
        so = os.path.join(str(workdir), "libbatch_plan.so")
        src = os.path.join(ROOT, "tests", "cpp", "batch_plan_lib.cpp")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
        lib = ctypes.CDLL(so)
        i64p, f32p, i32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
        c_int, c_i64, c_f = ctypes.c_int, ctypes.c_int64, ctypes.c_float
        lib.batch_plan_of.restype = None
        lib.batch_plan_of.argtypes = [c_int, c_int, c_i64, c_f, c_f, c_f, c_int, c_int, c_int, c_int, c_i64, i64p]
        lib.batch_band_of.restype = c_int
        lib.batch_band_of.argtypes = [c_int, c_int, c_i64, c_f, c_f, c_f, c_int, ctypes.c_double, f32p]
        lib.batch_sample_window_of.restype = None
        lib.batch_sample_window_of.argtypes = [i32p, ctypes.c_int32, c_i64, c_i64, c_int, i64p]
        lib.batch_tile_slot.restype = None
        lib.batch_tile_slot.argtypes = [c_int, c_int, c_int, ctypes.POINTER(c_int)]
        self.lib = lib

    @staticmethod
    def norms(rows):
        """(max |v|, min |v|, max |x|) as the ingest pass keeps them: f32, rounded outwards"""
        r64 = rows.astype(np.float64)
        nrm = np.sqrt(np.einsum("ij,ij->i", r64, r64))
        return (float(np.nextafter(np.float32(nrm.max()), np.float32(np.inf))), float(np.nextafter(np.float32(nrm.min()), np.float32(0))),
                float(np.abs(rows).max()))

    def plan(self, metric, d, n_rows, kernel, nq, k, group=True, kept=-1):
        """plan_batch for a shard of n_rows rows, a forced key kernel and a call of nq queries: a dict of FIELDS (with the
        kernel forced, nothing of it depends on the rows' norms: unit rows stand in)"""
        mx, mn, ab = 1.0, 1.0, 1.0
        out = (ctypes.c_int64 * len(self.FIELDS))()
        self.lib.batch_plan_of(metric, d, n_rows, mx, mn, ab, kernel, int(group), nq, k, kept, out)
        return dict(zip(self.FIELDS, [int(v) for v in out]))

    def bound(self, metric, d, n_rows, norms, kernel, q, key_max):
        """D: |key - exact| <= D for every row of the shard, by batch_delta2 (alpha at the longest row; the chain term of
        the fp16 L2 / inner-product keys at the largest key magnitude)"""
        mx, mn, ab = norms  # (of norms(rows))
        out = (ctypes.c_float * 3)()
        q64 = q.astype(np.float64)
        assert self.lib.batch_band_of(metric, d, n_rows, mx, mn, ab, kernel, float(q64 @ q64), out) == 1
        return float(out[0]) / 2.0 + float(out[1]) * mx * (1.0 + 1e-6) + float(out[2]) * key_max

    def sample_window(self, keep, n_sample, group):
        """(s0, kept rows in the window) of sample_window() for a keep mask over the rows"""
        n = len(keep)
        words = (n + 63) // 64
        per = np.add.reduceat(np.asarray(keep, np.int32), np.arange(0, n, 64))
        pre = np.ascontiguousarray(np.concatenate([[0], np.cumsum(per)]), np.int32)
        assert len(pre) == words + 1
        out = (ctypes.c_int64 * 2)()
        self.lib.batch_sample_window_of(pre.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), words, n, n_sample, int(group), out)
        return int(out[0]), int(out[1])

    def tile_slot(self, q_tiles, n_tiles, b):
        out = (ctypes.c_int * 2)()
        self.lib.batch_tile_slot(q_tiles, n_tiles, b, out)
        return int(out[0]), int(out[1])


def exact_keys_many(rows, qs, metric):
    """f64 keys [nq, rows] of the operation the key kernels approximate -- test_gpu_bands._exact_keys for many queries
    at once (L2 as |q|^2 + |v|^2 - 2 q.v in f64: its own rounding, ~1e-15 (|q|^2 + |v|^2), is nothing beside an f32
    bound).  test_gpu_batch_shapes holds a few rows of it to _exact_keys itself."""
    r64, q64 = rows.astype(np.float64), np.atleast_2d(qs).astype(np.float64)
    dots = q64 @ r64.T
    vsq = np.einsum("ij,ij->i", r64, r64)
    if metric == L2:
        return np.einsum("ij,ij->i", q64, q64)[:, None] + vsq[None, :] - 2.0 * dots
    if metric == IP:
        return -dots
    return -dots / np.sqrt(vsq)[None, :]


def bits(keep):
    return np.packbits(np.asarray(keep, bool), bitorder="little")


def edge_positions(n_rows, extra=()):
    """The rows at which a tile, wave-column or lane-half edge of the key kernels falls, the ones named first that a
    short list must not miss: `extra` (the sample window's ends), 8191 / 8192, 16383 / 16384, the first row of the
    ragged tile and the last row; then the first and last row of every 256- and 128-row tile; then of every 64-row
    wave column; then rows 31 / 32 of every column (the two halves of a wave's lanes); then, for lists longer than
    all of those, rows 1 / 62 and 30 / 33 of every column.  (Within a kind the units come in a fixed shuffled order, so
    that a list cut short still reaches every part of the shard.)"""
    first = list(extra) + [8191, 8192, 16383, 16384, n_rows // 256 * 256, n_rows - 1]
    shuffle = np.random.default_rng(20261020)
    cols = shuffle.permutation(np.arange(0, n_rows, 64))
    order = first
    for unit in (256, 128, 64):
        starts = shuffle.permutation(np.arange(0, n_rows, unit))
        order = order + [int(v) for pair in zip(starts, starts + unit - 1) for v in pair]
    for a, b in ((31, 32), (1, 62), (30, 33)):
        order = order + [int(v) for pair in zip(cols + a, cols + b) for v in pair]
    seen, out = set(), []
    for p in order:
        if 0 <= p < n_rows and p not in seen:
            seen.add(p)
            out.append(p)
    return out


class Planted:
    """rows, qs, groups [(queries, positions)], live, keep (None: no mask), k"""

    def __init__(self, metric, d, rows, qs, groups, k):
        self.metric, self.d, self.rows, self.qs, self.groups, self.k = metric, d, rows, qs, groups, k
        self.live = np.ones(len(rows), bool)
        self.keep = None

    @property
    def present(self):
        return self.live if self.keep is None else self.live & self.keep

    def planted_positions(self):
        return np.concatenate([np.asarray(p) for _, p in self.groups])


def build(rng, metric, d, nq, n_rows, groups, k=K, normalize=None, near=1e-3, etas=None, spread=False):
    """Gaussian filler and queries; per group (queries, positions): the group's queries are its first query plus `near`
    of its size in noise, and row positions[j] is lam * q + eta_j * noise, eta_j growing with j so that the planted rows
    of a group have distinct keys.  lam: 1, and 2 for inner product -- twice as long as a filler row, or a long filler
    row would beat the planted ones.  etas: per group, the noise's size at each position as a part of |q| instead (0.01
    ... 0.09 by default).  spread: the filler rows' norms range over [0.5, 2]."""
    rows = rng.standard_normal((n_rows, d), dtype=np.float32)
    if spread:
        rows *= rng.uniform(0.5, 2.0, size=(n_rows, 1)).astype(np.float32)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    lam = 2.0 if metric == IP else 1.0
    for g, (queries, positions) in enumerate(groups):
        base = qs[queries[0]].copy()
        size = float(np.linalg.norm(base))
        for q in queries[1:]:
            qs[q] = base + np.float32(near * size / np.sqrt(d)) * rng.standard_normal(d, dtype=np.float32)
        eta = 0.01 * (1.0 + np.arange(len(positions)) * (8.0 / max(len(positions), 8)))
        if etas is not None and etas[g] is not None:
            eta = np.asarray(etas[g], np.float64)
        eta = eta * size / np.sqrt(d)
        rows[np.asarray(positions)] = lam * base[None, :] + eta[:, None].astype(np.float32) * rng.standard_normal((len(positions), d), dtype=np.float32)
    if metric == COS:
        qs = np.stack([normalize(q) for q in qs])
    return Planted(metric, d, rows, qs, groups, k)


def check(lib, c, n_sample, s0=0, need_outside=0.5):
    """Properties 1-3 of the module docstring, from f64 keys.  Returns (exact keys, D per query)."""
    exact = exact_keys_many(c.rows, c.qs, c.metric)
    present = c.present
    assert np.abs(c.qs).max(axis=1).min() >= np.abs(c.qs).max() / 128  # (the fp16 kernel answers smaller queries alone)
    key_max = float(np.abs(exact).max())
    masked = np.where(present[None, :], exact, np.inf)
    nq = len(c.qs)
    norms = lib.norms(c.rows)
    D = np.array([max(lib.bound(c.metric, c.d, len(c.rows), norms, kern, c.qs[i], key_max) for kern in (0, 1, 2)) for i in range(nq)])
    for queries, positions in c.groups:  # 1.
        own = np.asarray(positions)[present[np.asarray(positions)]]
        assert 1 <= len(own), "a group with no live, kept row"
        for q in queries:
            order = np.argsort(masked[q], kind="stable")
            n_own = min(len(own), c.k)
            assert set(order[:n_own].tolist()) <= set(own.tolist()), (q, "its planted rows are not its nearest")
            other = np.setdiff1d(np.arange(len(c.rows)), own)
            gap = masked[q][other].min() - np.sort(masked[q][own])[n_own - 1]
            assert gap >= 8.0 * D[q], (q, gap, D[q])
    pos = c.planted_positions()
    outside = np.mean((pos < s0) | (pos >= s0 + n_sample))  # 2.
    assert outside >= need_outside, outside
    in_window = masked[:, s0:s0 + n_sample]  # 3.
    assert np.all(np.sum(np.isfinite(in_window), axis=1) >= c.k)
    kth = np.sort(in_window, axis=1)[:, c.k - 1]
    cap = min(lib.plan(c.metric, c.d, len(c.rows), kern, nq, c.k, kept=-1 if c.keep is None else int(c.keep.sum()))["cand_cap"] for kern in (0, 1, 2))
    n_cand = np.sum(masked <= (kth + 4.0 * D)[:, None], axis=1)
    assert n_cand.max() < cap // 2, (int(n_cand.max()), cap)
    return exact, D


def round_robin_groups(nq, positions, per_query=K):
    """position j of the list goes to query j % nq: each query's rows are spread over the whole list"""
    assert len(positions) >= nq * per_query
    return [((q,), [positions[q + nq * j] for j in range(per_query)]) for q in range(nq)]


# ---- (b) planted neighbours at every edge -------------------------------------------------------------------------
def planted_edges(rng, lib, metric, d, nq, normalize, variant="plain"):
    """variant: "plain"; "tombstoned" (every query's nearest planted row and one whole planted wave column outside the
    sample die); "masked" (an id-range mask that keeps about two thirds of the rows, so that the sample window moves:
    planted rows at both ends of the window for an ungrouped and for a norm-grouped plane, and per query one decoy --
    nearer than any kept row -- among the rows the mask drops).  Returns (Planted, {group: (s0, n_sample)})."""
    n = N_PLANTED
    n_sample = {lib.plan(metric, d, n, kern, nq, K)["n_sample"] for kern in (0, 1, 2)}
    assert len(n_sample) == 1
    n_sample = n_sample.pop()
    assert 0 < n_sample < n
    windows = {False: (0, n_sample), True: (0, n_sample)}
    keep = None
    extra = [n_sample - 1, n_sample]
    if variant == "masked":
        keep = np.arange(n) >= 9000
        assert 0.6 < keep.mean() < 0.7
        for group in (False, True):
            s0, best = lib.sample_window(keep, n_sample, group)
            assert s0 > 0 and best >= K
            windows[group] = (s0, n_sample)
        assert windows[False][0] != windows[True][0]  # (both are exercised: fp16 keys of L2 / IP take the grouped one)
        extra = [v for s0, _ in windows.values() for v in (s0 - 1, s0, s0 + n_sample - 1, s0 + n_sample)]
    positions = edge_positions(n, extra)
    if keep is not None:
        # the window holds more than half of the kept rows: 300 more rows behind both windows, early in the list, keep
        # half of the planted rows outside either
        dropped = [p for p in positions if not keep[p]]
        behind = max(s0 for s0, _ in windows.values()) + n_sample
        edges = set(positions)
        more = [p for p in range(behind + 2, n, 5) if p not in edges][:300]
        positions = [p for p in positions if keep[p]]
        positions = positions[:16] + more + positions[16:]
    groups = round_robin_groups(nq, positions)
    c = build(rng, metric, d, nq, n, groups, normalize=normalize)
    c.keep = keep
    if variant == "masked":  # decoys: the nearest row of all, dropped by the mask
        lam = 2.0 if metric == IP else 1.0
        for q in range(nq):
            c.rows[dropped[q]] = np.float32(lam) * (c.qs[q] if metric != COS else c.qs[q] * np.float32(3.0))
        assert len(set(dropped[:nq])) == nq
    if variant == "tombstoned":
        exact = exact_keys_many(c.rows, c.qs, metric)
        c.live[np.argmin(exact, axis=1)] = False
        col = next(p // 64 for p in positions if p >= n_sample + 256 and p % 64 == 0)
        c.live[col * 64:(col + 1) * 64] = False
        assert np.isin(np.arange(col * 64, (col + 1) * 64), c.planted_positions()).sum() >= 2
    return c, windows


# ---- (c) the fp16 epilogue's crowds -------------------------------------------------------------------------------
def lane_of(query_row, mi):
    """(32 x 32 block of the wave patch, lane half) that holds query row `query_row` of a 32 mi-row wave patch: the C/D map
    of the 32 x 32 MFMA, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)"""
    r = query_row % (32 * mi)
    return r // 32, (r % 32) // 4 % 2


CROWD_NQS = (257, 100)  # tile 256: a wave patch is 128 queries in four blocks; tile 128: 64 queries in two


def epilogue_crowds(rng, lib, metric, normalize, flush, nq=257):
    """d = 64, 257 or 100 queries, position = id (cosine, or an ungrouped plane).  Every crowd is one 64-row aligned run (one
    wave column) outside the sample, owned by near-equal queries of the first wave patch (128 queries; 64 of 100 -- two
    blocks only, where three survivors of a lane cannot avoid sharing a block: no "triple" there):
      flush = None   k = 8:   "pair": queries 0, 1 -- one lane, one block: two survivors of a lane inside ONE block (crowded);
                              a dead row in its middle
                              "triple": queries 8, 40, 72 -- one lane, three blocks: more than two survivors per lane and
                              none of them crowded
                              "ragged pair": queries 16, 17 on the last rows of the shard's ragged tile
      flush = "walk" k = 64:  queries 0, 1, 2, 3 own a whole run of 64 rows: 256 certain survivors of one wave patch, more
                              than its hit list holds, crowded: the list is flushed inside the register-by-register walk
      flush = "fast" k = 64:  queries 0, 4, 32, 36: two lanes, two blocks, every lane holds two survivors in two blocks:
                              the list is flushed on the straight path
    Every other query owns K rows at edge positions as in planted_edges."""
    d, n = 64, N_PLANTED
    k = 64 if flush else K
    n_sample = lib.plan(metric, d, n, 2, nq, k, group=False)["n_sample"]
    mi = lib.plan(metric, d, n, 2, nq, k, group=False)["tile"] // 64
    assert mi == (4 if nq > 128 else 2)
    run = lambda tile, col: n_sample + tile * 256 + col * 64
    ragged0 = n // 256 * 256
    if flush is None:
        crowds = {"pair": ((0, 1), list(range(run(3, 1) + 20, run(3, 1) + 29))),  # nine rows: the middle one dies
                  "triple": ((8, 40, 72), list(range(run(9, 2) + 28, run(9, 2) + 36))),
                  "ragged pair": ((16, 17), list(range(n - 8, n)))}
        assert lane_of(0, mi) == lane_of(1, mi)
        if mi == 4:
            blocks = [lane_of(q, mi) for q in (8, 40, 72)]
            assert len({b for b, _ in blocks}) == 3 and len({h for _, h in blocks}) == 1
        else:
            del crowds["triple"]
        assert lane_of(16, mi) == lane_of(17, mi) and ragged0 <= n - 8 and (n - 8) // 64 == (n - 1) // 64
    elif flush == "walk":
        crowds = {"flush": ((0, 1, 2, 3), list(range(run(5, 3), run(5, 3) + 64)))}
        assert len({lane_of(q, mi) for q in (0, 1, 2, 3)}) == 1
    else:
        crowds = {"flush": ((0, 4, 32, 36), list(range(run(5, 3), run(5, 3) + 64)))}
        lanes = [lane_of(q, mi) for q in (0, 4, 32, 36)]
        assert len(set(lanes)) == 4 and sorted(lanes) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for queries, positions in crowds.values():
        assert max(queries) < 32 * mi and min(positions) >= n_sample and min(positions) // 64 == max(positions) // 64
    if flush:
        assert 4 * 64 > f16_hits() and len(crowds["flush"][1]) == 64
    owned = {q for queries, _ in crowds.values() for q in queries}
    taken = {p for _, positions in crowds.values() for p in positions}
    rest = [q for q in range(nq) if q not in owned]
    positions = [p for p in edge_positions(n, [n_sample - 1, n_sample]) if p // 64 not in {t // 64 for t in taken}]
    groups = list(crowds.values())
    for i, (_, pos) in enumerate(round_robin_groups(len(rest), positions)):
        groups.append(((rest[i],), pos))
    c = build(rng, metric, d, nq, n, groups, k=k, normalize=normalize)
    if flush is None:
        c.live[crowds["pair"][1][4]] = False
    return c, n_sample


# ---- (d) the persistent loop ---------------------------------------------------------------------------------------
PERSISTENT_NQ = 600


def persistent_rows(cus):
    """rows of a shard whose filtered fp16 pass (600 queries: three query tiles) has more tiles than `cus` and not a
    multiple of it: the sample, cus // 3 + 3 whole tiles and a ragged one (256 CUs: 8192 + 88 * 256 + 37)"""
    return 8192 + (cus // 3 + 3) * 256 + 37


def persistent(rng, lib, metric, cus, normalize):
    """d = 64, k = 8, 600 queries.  The filtered launch runs min(tiles, cus) workgroups; workgroup b scores the slots b,
    b + grid ... of the tile order.  Every slot past the grid -- some workgroup's SECOND tile -- gets planted rows owned
    by queries of that slot's query tile, in that slot's row tile (sixteen, or as many as a ragged tile has for the slots
    that share it); the other planted rows sit at edge positions.  Returns (Planted, n_sample, second slots
    [(slot, query tile, row tile, changed)]): changed = the workgroup's first slot had another query tile."""
    d, nq = 64, PERSISTENT_NQ
    n = persistent_rows(cus)
    plan = lib.plan(metric, d, n, 2, nq, K, group=False)
    n_sample, tile, tile_n = plan["n_sample"], plan["tile"], plan["tile_n"]
    q_tiles, n_tiles = plan["nq_pad"] // tile, (n - n_sample + tile_n - 1) // tile_n
    total = q_tiles * n_tiles
    assert q_tiles == 3 and total > cus and total % cus != 0, (q_tiles, n_tiles, cus)
    grid = min(total, cus)
    second = []
    for b in range(grid, total):
        qt, nt = lib.tile_slot(q_tiles, n_tiles, b)
        qt0, _ = lib.tile_slot(q_tiles, n_tiles, b % grid)
        second.append((b, qt, nt, qt0 != qt))
    assert any(ch for _, _, _, ch in second)
    owned = {q: [] for q in range(nq)}
    taken = set()
    sharing = {}
    for _, _, nt, _ in second:
        sharing[nt] = sharing.get(nt, 0) + 1
    turn = {}
    for b, qt, nt, _ in second:
        r0, r1 = n_sample + nt * tile_n, min(n_sample + (nt + 1) * tile_n, n)
        spots = [p for p in edge_positions(n) if r0 <= p < r1] + [p for p in range(r0, r1) if p % 64 not in (0, 1, 30, 31, 32, 33, 62, 63)]
        spots = [p for p in spots if p not in taken]
        spots = spots[:min(16, (r1 - r0) // sharing[nt])]
        queries = [q for q in range(qt * tile, min((qt + 1) * tile, nq))]
        assert len(spots) >= 8
        for p in spots:
            t = turn.get(qt, 0)
            q = queries[t % len(queries)]
            turn[qt] = t + 1
            if len(owned[q]) < K:
                owned[q].append(p)
                taken.add(p)
    in_second = {q: list(v) for q, v in owned.items()}
    free = [p for p in edge_positions(n, [n_sample - 1, n_sample]) if p not in taken]
    edges = set(free) | taken
    free = free + [int(p) for p in rng.permutation(n) if p not in edges]  # (more planted rows than there are edges)
    outside, inside = iter([p for p in free if p >= n_sample]), iter([p for p in free if p < n_sample])
    for j in range(K):
        for q in range(nq):
            if len(owned[q]) < K:
                owned[q].append(next(outside))
    # What a workgroup that kept ANOTHER query tile's thresholds would get wrong: the queries of the first two query
    # tiles own K more rows INSIDE the sample, a little further off than their K rows outside -- their thresholds, the
    # K-th key of the sample, are as strict as a planted row -- and the rows of the last query tile's queries are far
    # noisier (0.6 |q|: still well ahead of every filler row), below a threshold that is a filler row's key.  Under a
    # first-tile threshold they would all be dropped.  L2: filler norms over [0.5, 2], so that |v|^2 of another tile's
    # rows (c_v, loaded a tile ahead) is no stand-in for a row's own.
    etas = []
    for q in range(nq):
        if q < 2 * tile:
            owned[q] = owned[q] + [next(inside) for _ in range(K)]
            etas.append(np.concatenate([0.01 + 0.005 * np.arange(K), 0.10 + 0.005 * np.arange(K)]))
        else:
            etas.append(0.60 + 0.005 * np.arange(K))
    c = build(rng, metric, d, nq, n, [((q,), owned[q]) for q in range(nq)], normalize=normalize, etas=etas, spread=metric == L2)
    exact = exact_keys_many(c.rows, c.qs, metric)
    kth = np.sort(exact[:, :n_sample], axis=1)[:, K - 1]  # the thresholds' exact stand-ins
    loose_rows = np.array([exact[q, owned[q]].min() for q in range(2 * tile, nq)])
    assert loose_rows.min() > np.percentile(kth[:2 * tile], 99), "a first-tile threshold would let the last tile's rows pass"
    # every second slot holds planted (query, row) pairs of its own tiles
    for b, qt, nt, _ in second:
        pairs = [(q, p) for q in range(qt * tile, min((qt + 1) * tile, nq)) for p in in_second[q] if (p - n_sample) // tile_n == nt]
        assert len(pairs) >= 8, (b, qt, nt, len(pairs))
    return c, n_sample, second
