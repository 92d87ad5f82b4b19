"""CPU: the inputs of tests/test_gpu_batch_shapes.py (tests/batch_shape_inputs.py) are what that file says they are.
Every builder of its planted-neighbour, epilogue-crowd and persistent-loop tests runs here, and check() proves from f64
keys and from tsh_batch_plan.h / tsh_batch_tiles.h themselves (g++, tests/cpp/batch_plan_lib.cpp) that each planted row
is a certain survivor of the filtered pass, that half of them lie outside the sample, and that no candidate list can
overflow -- so that on the GPU a dropped row or a redone query is the kernels' doing, not the inputs'."""
import numpy as np
import pytest

import batch_shape_inputs as bsi
from batch_shape_inputs import COS, IP, L2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return bsi.PlanLib(tmp_path_factory.mktemp("batch_plan"))


def test_the_plan_the_constructions_assume(lib):
    """the sample of a 23 589-row shard is a true part of it, made of whole tiles of either shape; the tiles are 128
    queries (256 for more than 128 on kernels 1 and 2: their 128-query tile needs a batch of at most 128) x 128 rows (256
    for fp16 keys); the fp16 planes are padded to
    ring turns of one, two and three at d = 40, 160 and 264"""
    for metric in (L2, IP, COS):
        for kern in (0, 1, 2):
            for nq in (100, 130, 257):
                p = lib.plan(metric, 40, bsi.N_PLANTED, kern, nq, bsi.K)
                assert p["kern"] == kern and 0 < p["n_sample"] < bsi.N_PLANTED and p["n_sample"] % 256 == 0
                assert p["tile"] == (256 if nq > 128 and kern != 0 else 128) and p["tile_n"] == (256 if kern == 2 else p["tile"])
                assert p["k_est"] == bsi.K and not p["listed"]
    assert [lib.plan(COS, d, bsi.N_PLANTED, 2, 130, bsi.K)["hchunks"] for d in (40, 160, 264)] == [4, 8, 12]
    assert bsi.f16_hits() == 128


def test_edge_positions_name_every_edge():
    n = bsi.N_PLANTED
    pos = bsi.edge_positions(n, [8191, 8192])
    assert len(pos) == len(set(pos)) and min(pos) == 0 and max(pos) == n - 1
    want = {8191, 8192, 16383, 16384, n // 256 * 256, n - 1}
    for c in range(0, n, 64):
        want |= {p for p in (c, c + 31, c + 32, c + 63) if p < n}
    assert want <= set(pos)
    assert set(pos[:6]) >= {8191, 8192, 16383, 16384}


@pytest.mark.parametrize("variant", ["plain", "tombstoned", "masked"])
@pytest.mark.parametrize("nq", [100, 130, 257])
@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_planted_edges(lib, oracle_mod, metric, nq, variant):
    for d in ((40, 160, 264) if variant == "plain" else (40,)):
        rng = np.random.default_rng(100 * d + 10 * metric + nq)
        c, windows = bsi.planted_edges(rng, lib, metric, d, nq, oracle_mod.normalize_f32, variant)
        for s0, n_sample in set(windows.values()):
            bsi.check(lib, c, n_sample, s0)
        owners = {q for queries, _ in c.groups for q in queries}
        assert {0, 31, 32, 63, 64, nq - 1} <= owners and (nq < 130 or {127, 128} <= owners) and (nq < 257 or {255, 256} <= owners)
        pos = set(c.planted_positions().tolist())
        n_sample = windows[False][1]
        named = {8191, 8192, 16383, 16384, bsi.N_PLANTED // 256 * 256, bsi.N_PLANTED - 1}
        if variant == "masked":
            for s0, _ in windows.values():
                named |= {s0 - 1, s0, s0 + n_sample - 1, s0 + n_sample}
            named = {p for p in named if c.keep[p]}  # (the others hold decoys)
            assert windows[False][0] > 0 and windows[True][0] > 0
        else:
            named |= {n_sample - 1, n_sample}
        assert named <= pos, named - pos
        if variant == "tombstoned":
            assert (~c.live).sum() >= nq + 60


@pytest.mark.parametrize("nq", bsi.CROWD_NQS)
@pytest.mark.parametrize("flush", [None, "walk", "fast"])
@pytest.mark.parametrize("metric", [L2, COS])
def test_epilogue_crowds(lib, oracle_mod, metric, flush, nq):
    rng = np.random.default_rng(300 + metric)
    c, n_sample = bsi.epilogue_crowds(rng, lib, metric, oracle_mod.normalize_f32, flush, nq)
    bsi.check(lib, c, n_sample)
    assert len(c.qs) == nq and [len(q) for q, _ in c.groups[:3]] == ([4, 1, 1] if flush else [2, 3, 2] if nq > 128 else [2, 2, 1])
    if flush:
        queries, positions = c.groups[0]
        assert len(queries) * len(positions) > bsi.f16_hits() and c.k == 64


@pytest.mark.parametrize("cus", [256, 304, 128])
@pytest.mark.parametrize("metric", [L2, COS])
def test_persistent(lib, oracle_mod, metric, cus):
    rng = np.random.default_rng(400 + metric)
    c, n_sample, second = bsi.persistent(rng, lib, metric, cus, oracle_mod.normalize_f32)
    bsi.check(lib, c, n_sample)
    assert len(c.rows) == bsi.persistent_rows(cus) and (cus != 256 or len(c.rows) == 8192 + 88 * 256 + 37)
    assert second and any(changed for _, _, _, changed in second)
