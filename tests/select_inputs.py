"""The case table of the select sweep (tests/test_host_select_inputs.py on the CPU, tests/test_gpu_select.py on the GPU):
every case names its rows (planted from a seed), metric, k, block capacity, tombstones and the path of the K2 select and
the host's wide-band pass it is meant to reach -- in the words of tests/select_model.py's path_name().

How rows are planted.  A case is a list of KEYS, one per row, and the rows are made to have them:
  L2             row = q + sqrt(key) u, u a random unit vector of the seed (every element of the row takes part)
  inner product  row = -key q / |q|^2 (the key is -q.row)
  "axis"         L2, q = (0.5, 0, ...), row = (0.5 + x, 0, ...) with x a multiple of 2^-23 in [1, 1.5): q - row is exact and
                 the key is x^2 rounded once, so keys can be planted a few ulps apart
Rows that are the same row have the same key, bit for bit, in every kernel (a row's sum does not depend on its place in
the tile).  Keys that are not the same are GAP = 2^-7 apart, relatively, wherever a decision of the select rests on their
order: test_host_select_inputs.py holds every threshold the model names (U, tau, the refined tau, the radix select's
k-th key) to be the only key value within 2^-8 of itself, and the GPU test holds the scan's own error band to a quarter of
that.  Everything that is no neighbour of anything sits at FAR.  Cases whose decisions rest on no order of distinct keys
are named in GAP_EXEMPT with the reason.

The plain plant: 1300 ranked keys 4 G^j, rank j in tile order[j % T] of a permutation of the seed, at a lane of the seed --
the first T ranks are the tile minima --, every other row at FAR.  T tiles: the last holds 37 rows, except where T itself is the edge under test.
"""
import numpy as np

L2, IP = 0, 1
GAP = 2.0 ** -7
G = 1.0 + GAP
FAR = {L2: 1.0e6, IP: 64.0}
D = 8
RANKED = 1300  # tile minima that are distinct; the rest are FAR
ROW_BASE = 1000003  # global id of every shard's first row: not 0, not a multiple of 64


def entries_default(k):
    from select_model import plan

    return plan().default_entries(k)


class Case:
    def __init__(self, name, group, tiles, k, path, metric=L2, entries=None, plant="ranked", last=37, **kw):
        self.name, self.group, self.tiles, self.k, self.path, self.metric = name, group, tiles, k, path, metric
        self.entries, self.plant, self.last, self.kw = entries, plant, last, kw
        self.dim = kw.get("dim", D)
        self.f16 = bool(kw.get("f16"))  # the fp16 store: set_scan_f16(2)
        self.seed = 9000 + sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100000

    def __repr__(self):
        return self.name

    @property
    def n(self):
        return (self.tiles - 1) * 64 + self.last

    def block_entries(self):
        return entries_default(self.k) if self.entries is None else self.entries


def _ranked(c, rng, keys, live, first=4.0):
    """RANKED distinct keys first G^j: rank j in tile order[j % T] (the first T of them are the tile minima, in that order)"""
    T = c.tiles
    order = rng.permutation(T)
    lanes = [rng.permutation(min(64, c.n - t * 64)) for t in range(T)] if T < RANKED else None
    for j in range(RANKED):
        t = order[j % T]
        lane = int(lanes[t][j // T]) if lanes else int(rng.integers(0, min(64, c.n - t * 64)))
        keys[t * 64 + lane] = first * G ** j
    return order


def plant_keys(c):
    """-> (f64 key per row, live[] per row).  The keys are targets: make_rows gives the rows that have them."""
    rng = np.random.default_rng(c.seed)
    n, T, far = c.n, c.tiles, FAR[c.metric]
    keys = np.full(n, far, np.float64)
    live = np.ones(n, bool)
    p = c.plant
    if p == "ranked":
        _ranked(c, rng, keys, live)
    elif p == "signed":  # inner product: 525 negative keys -1 .. -60, then positive ones 1 .. 62, one per tile
        order = rng.permutation(T)
        vals = np.concatenate([-(G ** np.arange(524, -1, -1)), G ** np.arange(530)])
        for j, t in enumerate(order[:len(vals)]):
            keys[t * 64 + int(rng.integers(0, min(64, n - t * 64)))] = vals[j]
    elif p == "ulps":  # 300 keys 2 ulps apart round the k-th, below them k - 150 ranked ones, "axis" rows
        x0 = 1.25
        lo = c.k - 150
        where = rng.permutation(n)
        keys[:] = 1.4375 ** 2  # FAR of the axis form: x = 1.4375
        keys[where[:lo]] = (1.0 + np.arange(lo) * 2.0 ** -13) ** 2  # x = 1 .. 1.11
        keys[where[lo:lo + 300]] = (x0 + np.arange(300) * 2.0 ** -23) ** 2
    elif p == "tied_kth":  # k - 500 ranked keys, then one row 2000 times: the k-th key is tied across k
        where = rng.permutation(n)
        lo = c.k - 500
        keys[where[:lo]] = 4.0 * G ** np.arange(lo)
        keys[where[lo:lo + 2000]] = 4.0 * G ** (lo + 1)
    elif p == "one_live":  # one live row per tile
        order = _ranked(c, rng, keys, live)
        live[:] = False
        for t in range(T):
            rows_in = min(64, n - t * 64)
            m = np.argmin(keys[t * 64:t * 64 + rows_in])
            live[t * 64 + m] = True
    elif p == "copies":  # `copies` copies of one nearest row in every tile
        for t in range(T):
            rows_in = min(64, n - t * 64)
            lanes = rng.choice(rows_in, c.kw["copies"], replace=False)
            keys[t * 64 + lanes] = 4.0
    elif p == "cluster":  # the best 384 rows fill six tiles; the other tiles' minima are ranked above them
        order = rng.permutation(T)
        order = order[order != T - 1]  # (whole tiles)
        ck = (G ** np.arange(384)) if c.metric == L2 else -(G ** np.arange(383, -1, -1)) / 4.0  # IP: -4.9 .. -0.25
        ck = rng.permutation(ck)
        for i, t in enumerate(order[:6]):
            keys[t * 64:(t + 1) * 64] = ck[i * 64:(i + 1) * 64]
        first = 32.0 if c.metric == L2 else 1.0
        for j, t in enumerate(order[6:6 + 520]):  # (up to 57: below FAR of either metric)
            keys[t * 64 + int(rng.integers(0, 64))] = first * G ** j
    elif p == "live_tiles":  # `live_tiles` tiles alive, every live row its own key; the rest tombstoned, whole tiles
        order = rng.permutation(T - 1)[:c.kw["live_tiles"]]
        live[:] = False
        per = c.kw["live_per_tile"]
        vals = rng.permutation(4.0 * G ** np.arange(len(order) * per))
        for i, t in enumerate(order):
            lanes = np.sort(rng.choice(64, per, replace=False)) if per < 64 else np.arange(64)
            if per == 1 and i == 0:
                lanes = np.array([63])  # a tile whose one live row is its last lane
            live[t * 64 + lanes] = True
            keys[t * 64 + lanes] = vals[i * per:(i + 1) * per]
    elif p == "flood_loose":  # one copy of a row in every tile, and ten nearer rows in tiles of ONE four-thread group
        for t in range(T):
            keys[t * 64 + int(rng.integers(0, min(64, n - t * 64)))] = 16.0
        for j, t in enumerate([0, 1, 2, 3, 1024, 1025, 1026, 1027, 2048, 2049]):  # threads 0 .. 3 own tiles tid + 1024 i
            keys[t * 64 + 5 + j] = 4.0 * G ** j
    elif p == "layout":  # one copy of a row at 1024 in every tile, and nearer rows 4 G^j in the tiles named: WHICH threads
        for t in range(T):  # and groups of the select hold them decides how loose the prefilter's bound U is
            keys[t * 64 + int(rng.integers(0, min(64, n - t * 64)))] = 1024.0
        for j, t in enumerate(c.kw["small"]):
            keys[t * 64 + int(rng.integers(0, 64))] = 4.0 * G ** j
    elif p == "list":  # a WHERE set of `kept` rows, each its own key; every other row NEARER than all of them
        keys[:] = 1.0
        kept = np.sort(rng.choice(n, c.kw["kept"], replace=False))
        keys[kept] = rng.permutation(4.0 * G ** np.arange(len(kept)))
        if c.kw.get("live_kept") is not None:  # tombstoned after the mask was made: only the nearest live_kept stay
            order = kept[np.argsort(keys[kept])]
            live[order[c.kw["live_kept"]:]] = False
    elif p == "f16_edge":  # 40 tile minima 1024 x 1.25^j, and 41 rows from 0.01 to 10^4 above the k-th of them, in the tiles
        order = rng.permutation(T - 1)  # of the nearer minima: whatever the rows' bands are, some of these rows pass the
        keys[:] = 1.0e7                 # select's per-row rule and the others fail it
        lanes = [rng.permutation(64) for _ in range(T)]
        for j, t in enumerate(order):
            keys[t * 64 + lanes[t][0]] = 1024.0 * 1.25 ** j
        kth = 1024.0 * 1.25 ** (c.k - 1)
        for j in range(41):
            t = order[j % (c.k - 1)]
            keys[t * 64 + lanes[t][1 + j // (c.k - 1)]] = kth + 0.01 * 2.0 ** (j / 2.0)
    elif p == "f16_cluster":  # the best 320 rows, 8 apart, fill five tiles; the other tiles' minima from 8192 x 1.25^j
        order = rng.permutation(T - 1)
        keys[:] = 1.0e7
        ck = rng.permutation(1024.0 + 8.0 * np.arange(320))
        for i, t in enumerate(order[:5]):
            keys[t * 64:(t + 1) * 64] = ck[i * 64:(i + 1) * 64]
        for j, t in enumerate(order[5:]):
            keys[t * 64 + int(rng.integers(0, 64))] = 8192.0 * 1.25 ** j
    elif p == "f16_copies":  # eight copies of one row in every tile: more ties than the block holds
        keys[:] = 1.0e7
        for t in range(T):
            keys[t * 64 + rng.choice(min(64, n - t * 64), 8, replace=False)] = 1024.0
    else:
        raise ValueError(p)
    return keys, live


def kept_rows(c):
    """The rows a list case's WHERE set keeps (ascending local ids): the rows whose key is not the filler's."""
    assert c.plant == "list"
    keys, _ = plant_keys(c)
    return np.nonzero(keys != 1.0)[0]


def list_order(c):
    """... as the list scan holds them: ascending, padded with -1 to whole tiles of 64"""
    kept = kept_rows(c)
    out = np.full((len(kept) + 63) // 64 * 64, -1, np.int64)
    out[:len(kept)] = kept
    return out


def make_rows(c, keys):
    """-> (rows f32 [n, D], query f32 [D]) whose keys are `keys` up to the roundings of f32"""
    rng = np.random.default_rng(c.seed + 1)
    n = len(keys)
    D = c.dim
    if c.plant == "ulps":
        q = np.zeros(D, np.float32)
        q[0] = 0.5
        rows = np.zeros((n, D), np.float32)
        x = np.sqrt(keys)
        assert np.all(x * 2.0 ** 23 == np.round(x * 2.0 ** 23)) and np.all((x >= 1) & (x < 1.5))
        rows[:, 0] = (0.5 + x).astype(np.float32)
        assert np.array_equal(rows[:, 0].astype(np.float64), 0.5 + x)
        return rows, q
    q = rng.standard_normal(D).astype(np.float32)
    q64 = q.astype(np.float64)
    # one direction per distinct key: rows of the same key are the same row
    vals, inv = np.unique(keys, return_inverse=True)
    if c.metric == L2:
        u = rng.standard_normal((len(vals), D))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        proto = q64[None, :] + np.sqrt(vals)[:, None] * u
    else:
        proto = -vals[:, None] * q64[None, :] / (q64 @ q64)
    return proto.astype(np.float32)[inv], q


def exact_keys(rows, q, metric):
    """f64 keys of the rows as they are (after their rounding to f32)"""
    r, q = rows.astype(np.float64), q.astype(np.float64)
    return ((r - q) ** 2).sum(axis=1) if metric == L2 else -(r @ q)


A, B, C, Dg, E, F, Gg, H = "A", "B", "C", "D", "E", "F", "G", "H"
CASES = [
    # ---- A: variant edges
    Case("A-t64-k10", A, 64, 10, "NT256-regs none/short-small", last=64),
    Case("A-t65-k10", A, 65, 10, "NT256-regs none/short-small"),
    Case("A-t512-k10", A, 512, 10, "NT256-regs none/short-small", last=64),
    Case("A-t513-k10", A, 513, 10, "NT1024-regs groups4/short-small"),
    Case("A-t512-k256", A, 512, 256, "NT256-regs none/short-small", last=64),
    Case("A-t512-k257", A, 512, 257, "NT1024-regs none/short-small", last=64),
    Case("A-t16384-k100", A, 16384, 100, "NT1024-regs groups4/short-small", last=64),
    Case("A-t16385-k100", A, 16385, 100, "NT1024-mem groups4/short-small"),
    # ---- B: prefilter groups
    Case("B-t1100-k128", B, 1100, 128, "NT1024-regs groups4/short-small"),
    Case("B-t1100-k129", B, 1100, 129, "NT1024-regs plain/short-small"),
    Case("B-t1100-k512", B, 1100, 512, "NT1024-regs plain/short-large"),
    Case("B-t1100-k513", B, 1100, 513, "NT1024-regs groups2k/short-large"),
    Case("B-t1100-k1024", B, 1100, 1024, "NT1024-regs groups2k/short-large"),
    Case("B-t1024-k1024", B, 1024, 1024, "NT1024-regs groups2k/short-large", last=64),
    Case("B-t1023-k1024", B, 1023, 1024, "NT1024-regs all-tiles refined-mem"),
    # ---- C: k beyond the scheme
    Case("C-t1100-k1025", C, 1100, 1025, "NT1024-regs all-tiles refined-mem"),
    Case("C-t4097-k1025", C, 4097, 1025, "NT1024-regs all-tiles over radix-found"),
    Case("C-ulps", C, 4097, 1025, "NT1024-regs all-tiles over radix-found", plant="ulps"),
    Case("C-tied-kth", C, 4097, 1025, "NT1024-regs all-tiles over radix-found overflow", plant="tied_kth"),
    Case("C-ip-signed", C, 4097, 1025, "NT1024-regs all-tiles over radix-found", metric=IP, plant="signed"),
    Case("C-not-found", C, 4097, 5000, "NT1024-regs all-tiles over radix-not_found", plant="one_live"),
    # ---- D: ties across tiles
    Case("D-t4200", Dg, 4200, 10, "NT1024-regs groups4/flooded over filter overflow", plant="copies", copies=1),
    Case("D-t4096", Dg, 4096, 10, "NT1024-regs groups4/short-large refined-mem-diff0 filter overflow", plant="copies", copies=1, last=64),
    Case("D-flood-loose", Dg, 4200, 10, "NT1024-regs groups4/flooded over filter overflow", plant="flood_loose"),
    # (thread tid of sixteen waves owns tiles tid + 1024 i; threads 4 g .. 4 g + 3 are one group of groups4, a thread's even
    # and odd i two groups of groups2k.)  k = 129 nearer minima in 129 threads but 128 four-thread groups: the plain bisect
    # bounds them exactly, groups4 would not; k = 512 of them in 511 threads but 512 half-threads: the plain bisect's U is
    # the tie, the list floods and tau = U -- groups2k would have bounded them exactly
    Case("D-k129-thread-pair", Dg, 4200, 129, "NT1024-regs plain/short-small", plant="layout", small=[0, 1] + [4 * g for g in range(1, 128)]),
    Case("D-k512-parity-pair", Dg, 4200, 512, "NT1024-regs plain/flooded over filter overflow", plant="layout",
         small=[0, 1024] + list(range(1, 511))),
    # ---- E: refinement limits, clustered neighbours
    Case("E-nt256-k64", E, 100, 64, "NT256-regs none/short-small refined-regs", plant="cluster"),
    Case("E-nt256-k65", E, 100, 65, "NT256-regs none/short-small refined-mem", plant="cluster"),
    Case("E-nt1024-k256", E, 600, 256, "NT1024-regs plain/short-small refined-regs", plant="cluster"),
    Case("E-nt1024-k257", E, 600, 257, "NT1024-regs plain/short-small refined-mem", plant="cluster"),
    Case("E-ip-k64", E, 100, 64, "NT256-regs none/short-small refined-regs-top31", metric=IP, plant="cluster"),
    Case("E-ip-k257", E, 600, 257, "NT1024-regs plain/short-small refined-mem-top31", metric=IP, plant="cluster"),
    Case("E-five-copies", E, 64, 10, "NT256-regs none/short-small refined-regs-diff0 filter overflow", plant="copies", copies=5, last=64),
    # ---- F: dead tiles
    Case("F-40-live-tiles", F, 300, 50, "NT256-regs none/short-small tau-nan refined-regs", plant="live_tiles", live_tiles=40, live_per_tile=64),
    Case("F-30-live-rows", F, 300, 50, "NT256-regs none/short-small tau-nan", plant="live_tiles", live_tiles=30, live_per_tile=1),
    # ---- G: list scans (n rows, `kept` of them in the WHERE set: tiles of list positions)
    Case("G-21-tiles-k10", Gg, 512, 10, "NT256-regs list:none/short-small", plant="list", kept=1300, last=64),
    Case("G-21-tiles-k100", Gg, 512, 100, "NT256-regs list-radix", plant="list", kept=1300, last=64),
    Case("G-21-tiles-k1300", Gg, 512, 1300, "NT1024-regs list-radix", plant="list", kept=1300, last=64),
    Case("G-21-tiles-k1301", Gg, 512, 1301, "NT1024-regs list-radix tau-nan", plant="list", kept=1300, last=64),
    Case("G-full-tiles-k1344", Gg, 512, 1344, "NT1024-regs list-radix", plant="list", kept=1344, last=64),
    Case("G-full-tiles-k1345", Gg, 512, 1345, "NT1024-regs list:all-tiles", plant="list", kept=1344, last=64),
    Case("G-79-tiles-k100", Gg, 2048, 100, "NT1024-regs list-radix", plant="list", kept=5000, last=64),
    Case("G-79-tiles-60-live", Gg, 2048, 100, "NT1024-regs list-radix tau-nan", plant="list", kept=5000, live_kept=60, last=64),
    # ---- H: the fp16 store (d = 256, 40 tiles): keys are stored upper sides, a row passes by its own band
    Case("H-f16-plain", H, 40, 10, "NT256-regs f16:none/short-small", plant="f16_edge", dim=256, f16=True),
    Case("H-f16-refined", H, 40, 10, "NT256-regs f16:none/short-small refined-regs", plant="f16_cluster", dim=256, f16=True),
    Case("H-f16-overflow", H, 40, 10, "NT256-regs f16:none/short-small refined-regs-diff0 overflow redone", plant="f16_copies",
         dim=256, f16=True, f32_path="NT256-regs none/short-small refined-regs-diff0 filter overflow"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# decisions that rest on no order of two distinct keys: the reason a case's thresholds are not held to the gap
GAP_EXEMPT = {
    "C-ulps": "the keys round the k-th are 2 ulps apart on purpose: its path rests on M and k alone, and the GPU test holds "
              "the block to the model run on the scan's own keys, whichever of them is the k-th",
    "H-f16-plain": "rows planted from 0.01 to 10^4 above the k-th key on purpose: which of them pass is the per-row rule of the "
                   "fp16 store, decided by the scan's own keys and bands",
    "H-f16-refined": "the cluster's keys are 8 apart, about a row's band: the second emit's per-row rule decides among them",
    "H-f16-overflow": "the fp16 store's band is per cent of a key, not 2^-8 of it; the case is one tie and FAR rows 10^4 times off",
}

# every path the table reaches, in the words of select_model.path_name(), written out: the host test holds the table to
# this list (a case that leaves with its path is noticed), the GPU test the union of what the kernels' keys made the model
# say
PATHS = [
    "NT1024-mem groups4/short-small",
    "NT1024-regs all-tiles over radix-found",
    "NT1024-regs all-tiles over radix-found overflow",
    "NT1024-regs all-tiles over radix-not_found",
    "NT1024-regs all-tiles refined-mem",
    "NT1024-regs groups2k/short-large",
    "NT1024-regs groups4/flooded over filter overflow",
    "NT1024-regs groups4/short-large refined-mem-diff0 filter overflow",
    "NT1024-regs groups4/short-small",
    "NT1024-regs list-radix",
    "NT1024-regs list-radix tau-nan",
    "NT1024-regs list:all-tiles",
    "NT1024-regs none/short-small",
    "NT1024-regs plain/flooded over filter overflow",
    "NT1024-regs plain/short-large",
    "NT1024-regs plain/short-small",
    "NT1024-regs plain/short-small refined-mem",
    "NT1024-regs plain/short-small refined-mem-top31",
    "NT1024-regs plain/short-small refined-regs",
    "NT256-regs f16:none/short-small",
    "NT256-regs f16:none/short-small refined-regs",
    "NT256-regs f16:none/short-small refined-regs-diff0 overflow redone",
    "NT256-regs list-radix",
    "NT256-regs list:none/short-small",
    "NT256-regs none/short-small",
    "NT256-regs none/short-small refined-mem",
    "NT256-regs none/short-small refined-regs",
    "NT256-regs none/short-small refined-regs-diff0 filter overflow",
    "NT256-regs none/short-small refined-regs-top31",
    "NT256-regs none/short-small tau-nan",
    "NT256-regs none/short-small tau-nan refined-regs",
]
assert PATHS == sorted(PATHS) and {c.path for c in CASES} <= set(PATHS)

# cases whose path another case reaches too: taking one out loses no path, they are held by the rule that put them
# there -- each stands on one side of an edge whose other side (or whose neighbour) takes the same path
HELD_BY_RULE = {
    "A-t64-k10": "64 / 65 tiles: the last whole tile of four waves' registers, the same path either side",
    "A-t65-k10": "64 / 65 tiles",
    "A-t512-k10": "512 tiles: the last of the four-wave variant (513: A-t513-k10)",
    "A-t512-k256": "k = 256: the last of the four-wave variant (257: A-t512-k257)",
    "A-t513-k10": "513 tiles: the first with a prefilter",
    "A-t16384-k100": "16384 tiles: the last whose minima stay in registers (16385: A-t16385-k100)",
    "B-t1100-k128": "k = 128: the last of groups4 (129: B-t1100-k129)",
    "B-t1100-k513": "k = 513: the first of groups2k (512: B-t1100-k512)",
    "B-t1100-k1024": "k = 1024: the last narrow k (1025: C-t1100-k1025)",
    "B-t1024-k1024": "M == k: the last narrow M (1023: B-t1023-k1024)",
    "B-t1023-k1024": "M < k by one",
    "C-t1100-k1025": "k beyond the scheme by one",
    "C-t4097-k1025": "4097 tiles: over by one",
    "C-ulps": "the radix select's last round",
    "C-ip-signed": "the radix select over keys of both signs",
    "D-t4200": "4200 tiles of one tie: flooded",
    "D-k129-thread-pair": "k = 129 by the plain thread minima, not by four-thread groups: the layout tells them apart",
    "B-t1100-k129": "k = 129: the first of the plain bisect (128: B-t1100-k128)",
    "D-flood-loose": "flooded with a tau below U among the minima: the bound that is written out is U",
    "G-21-tiles-k1300": "k = the kept rows (1301: G-21-tiles-k1301)",
    "G-full-tiles-k1344": "64 M == k (64 M < k: G-full-tiles-k1345)",
    "G-79-tiles-k100": "79 list tiles: block_kth_radix by sixteen waves (by four: G-21-tiles-k100)",
    "G-21-tiles-k1301": "fewer kept rows than k by one",
    "G-79-tiles-60-live": "kept rows tombstoned after the mask was made",
}
