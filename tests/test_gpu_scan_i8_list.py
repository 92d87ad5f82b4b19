"""GPU: the one launch between the coarse int8 scan and the exact path (i8_list_kernel, tsh_scan_i8.hip.h).

The scan leaves two minima per tile -- of the upper and of the lower sides of its rows' bands -- and one workgroup turns
them into the survivor list: the threshold, the tiles whose lower minimum is at or below it, those tiles' ballots, the
ascending id list.  Every index here forces the route for dense and masked scans on small shapes (both options 2) at the
narrowest row width (four floats), switches the batched path and the exact path off, and every case is held bit for bit
-- ids, distances, counts -- to the oracle and to the same search with TSH_OPT_SCAN_I8 = 0; each says how many of its
queries it expects redone through the f32 scan (tsh_scan_i8_stats).

The corpora: background rows of small norm, a query of norm 8 along the first axis, and "winners" next to the query.  A
winner's key is about -64 with a band of about 0.5; no background key is below -30, so which rows survive is known."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2 = 0
D = 4
TILE = 64
CAP = 4096  # I8_LIST_CAP


def _open(rows):
    from tostore_amd import HipVectorIndex

    idx = HipVectorIndex(D, L2, capacity_rows=len(rows))
    idx.set_scan_i8(2)
    idx.set_scan_i8_masked(2)
    idx.set_exact_scan_rows(0)
    idx.set_batch_min_nq(0)
    idx.append(0, rows)
    return idx


def _same(got, ref, what):
    assert np.array_equal(got[2], ref[2]), "counts differ from " + what
    assert np.array_equal(got[0], ref[0]), "ids differ from " + what
    assert np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), "distance bits differ from " + what


def _check(idx, oracle_mod, rows, q, k, redone, keep=None):
    """One query: the oracle's answer over the int8 copy, redone `redone` times; the same answer with the route off."""
    qs = q[None, :]
    ref = oracle_mod.search_heap_many_mt(rows, qs, L2, k, None, keep)
    s0 = idx.scan_i8_stats()
    got = idx.search(qs, k)
    s1 = idx.scan_i8_stats()
    _same(got, ref, "the oracle's")
    assert s1["scans"] - s0["scans"] == 1 and s1["redone"] - s0["redone"] == redone, (s0, s1)
    idx.set_scan_i8(0)
    plain = idx.search(qs, k)
    idx.set_scan_i8(2)
    assert idx.scan_i8_stats()["scans"] == s1["scans"]  # (option 0 kept the route off)
    _same(got, plain, "the answer with TSH_OPT_SCAN_I8 = 0")
    return ref


def _query(rng):
    q = (0.1 * rng.standard_normal(D)).astype(np.float32)
    q[0] = 8.0
    return q


def _background(rng, n):
    return (0.3 * rng.standard_normal((n, D))).astype(np.float32)


def _near(rng, q, n):
    return (q[None, :] + 0.01 * rng.standard_normal((n, D))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _corpus_1100():
    rng = np.random.default_rng(1100)
    rows = _background(rng, 1100 * TILE)
    rows.setflags(write=False)
    return rows, _query(rng)


def test_winners_in_one_tile(hip_lib, oracle_mod):
    """1 100 tiles, the k = 64 nearest rows all in tile 5: the threshold comes from background tiles."""
    base, q = _corpus_1100()
    rng = np.random.default_rng(1)
    rows = base.copy()
    rows[5 * TILE:6 * TILE] = _near(rng, q, TILE)
    with _open(rows) as idx:
        ref = _check(idx, oracle_mod, rows, q, 64, 0)
    assert sorted(ref[0][0]) == list(range(5 * TILE, 6 * TILE))


def test_winners_spread_over_the_waves_runs(hip_lib, oracle_mod):
    """One winner in each of tiles 0, 17, 34, ..., 1088 (65 tiles): candidate tiles in nine of the sixteen waves' runs."""
    base, q = _corpus_1100()
    rng = np.random.default_rng(2)
    rows = base.copy()
    where = np.array([t * TILE + (7 * t) % TILE for t in range(0, 1100, 17)])
    assert len(where) == 65 and where[-1] // TILE == 1088
    rows[where] = _near(rng, q, len(where))
    with _open(rows) as idx:
        ref = _check(idx, oracle_mod, rows, q, 64, 0)
    assert np.isin(ref[0][0], where).all()


@pytest.mark.parametrize("n", [4097, 4159, 4160, 4161])
def test_row_counts_at_tile_edges(hip_lib, oracle_mod, n):
    """A last tile of 1, 63, 64 and 1 rows; the winner is the last row."""
    rng = np.random.default_rng(n)
    q = _query(rng)
    rows = _background(rng, n)
    rows[n - 1] = _near(rng, q, 1)[0]
    with _open(rows) as idx:
        ref = _check(idx, oracle_mod, rows, q, 10, 0)
    assert ref[0][0][0] == n - 1


@pytest.mark.parametrize("case", ["4096_copies", "4097_copies", "4096_tiles", "4097_tiles"])
def test_capacity_both_ways(hip_lib, oracle_mod, case):
    """Duplicates of the query's nearest row, k = 64: 4 096 survivors fit the list and 4 097 do not, whether they fill 64
    tiles (and one row of a 65th) or sit one to a tile -- 4 097 candidate tiles are an overflow before any key is read."""
    rng = np.random.default_rng(77)
    q = _query(rng)
    twin = _near(rng, q, 1)[0]
    if case.endswith("copies"):
        rows = _background(rng, 100 * TILE)
        where = np.arange(10 * TILE, 74 * TILE)
        if case == "4097_copies":
            where = np.append(where, 80 * TILE + 3)
    else:
        n_tiles = 4097
        rows = _background(rng, n_tiles * TILE)
        tiles = np.arange(4096 if case == "4096_tiles" else 4097)
        where = tiles * TILE + (5 * tiles) % TILE
    rows[where] = twin
    over = case.startswith("4097")
    assert len(where) == (CAP + 1 if over else CAP)
    with _open(rows) as idx:
        ref = _check(idx, oracle_mod, rows, q, 64, 1 if over else 0)
    assert np.array_equal(ref[0][0], where[:64])  # ties: the lowest ids first


def test_masked_dead_tiles_and_a_dead_winner(hip_lib, oracle_mod):
    """Tombstones: every row of the tiles between winner tiles whose number is 3, 4 or 5 mod 17, the lone winner of tile 34,
    and a random 5 % of the rest."""
    base, q = _corpus_1100()
    rng = np.random.default_rng(3)
    rows = base.copy()
    where = np.array([t * TILE + (7 * t) % TILE for t in range(0, 1100, 17)])
    rows[where] = _near(rng, q, len(where))
    live = rng.random(len(rows)) >= 0.05
    live[where] = True
    for t in range(1100):
        if t % 17 in (3, 4, 5):
            live[t * TILE:(t + 1) * TILE] = False
    dead_winner = where[2]
    assert dead_winner // TILE == 34
    live[dead_winner] = False
    keep = np.packbits(live, bitorder="little")
    with _open(rows) as idx:
        idx.set_deleted(np.nonzero(~live)[0])
        ref = _check(idx, oracle_mod, rows, q, 64, 0, keep)
    assert dead_winner not in ref[0][0] and np.isin(ref[0][0], where).all()


@pytest.mark.parametrize("n_tiles,live_tiles,redone", [
    (100, 80, 1),  # 5 120 live rows in fewer than k tiles: every live row survives, more than the list takes
    (100, 50, 0),  # 3 200: they fit
    (60, 40, 0),   # a shard of fewer than 4 096 rows
])
def test_masked_fewer_live_tiles_than_k(hip_lib, oracle_mod, n_tiles, live_tiles, redone):
    rng = np.random.default_rng(100 * n_tiles + live_tiles)
    q = _query(rng)
    rows = _background(rng, n_tiles * TILE)
    rows[[70, 33 * TILE + 1]] = _near(rng, q, 2)
    live = np.zeros(len(rows), bool)
    for t in rng.choice(n_tiles, live_tiles, replace=False):
        live[t * TILE:(t + 1) * TILE] = True
    live[:2 * TILE] = True  # (the first winner's tile and its neighbour; the second winner's is live or not by the draw)
    live[2 * TILE:3 * TILE] = False
    keep = np.packbits(live, bitorder="little")
    n_live_tiles = int(live.reshape(n_tiles, TILE).any(axis=1).sum())
    assert n_live_tiles < 100 and (live.sum() > CAP) == bool(redone)
    with _open(rows) as idx:
        idx.set_deleted(np.nonzero(~live)[0])
        ref = _check(idx, oracle_mod, rows, q, 100, redone, keep)
    assert ref[0][0][0] in (70, 33 * TILE + 1)


def test_above_16384_tiles(hip_lib, oracle_mod):
    """16 385 tiles: the threshold and the candidate tiles from global memory, a run of 17 x 64 tiles per wave.  Winners in
    tile 0, in a middle tile and in the last one."""
    n_tiles = 16385
    rng = np.random.default_rng(16385)
    q = _query(rng)
    rows = _background(rng, n_tiles * TILE)
    where = np.concatenate([np.arange(0, 20), 8000 * TILE + np.arange(20, 40), 16384 * TILE + np.arange(44, 64)])
    rows[where] = _near(rng, q, len(where))
    with _open(rows) as idx:
        ref = _check(idx, oracle_mod, rows, q, 64, 0)
    assert np.isin(where, ref[0][0]).all()
