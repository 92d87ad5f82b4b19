"""CPU: the NumPy model of the 4-bit first pass (tests/scan_i4_model.py) on the corpora tests/test_gpu_scan_i4.py uses.
Every exact key lies inside the model's [lower, upper]; and each corpus lies on the side of the deny threshold
(SCAN_I4_MAX_SHARE = 0.32 of the rows) its GPU test assumes, with a margin of 0.10 of the rows: the spread-norm corpora
leave at most 0.22 of their rows to the int8 scan, the unit-norm corpus at least 0.42."""
import numpy as np
import pytest

import scan_i4_model as M

MARGIN = 0.10


@pytest.mark.parametrize("n,d,ks", [(20_037, 768, (100, 10, 1)), (40_000, 100, (10,)), (20_037, 1000, (100,)), (8_200, 2048, (100,))])
def test_spread_corpora_stay_below_the_threshold(n, d, ks):
    rng = np.random.default_rng(100 * d)
    rows, qs = M.spread_corpus(rng, n, d)
    sh = M.Shard(rows)
    for q in qs:
        lo, up, _ = sh.sides(q)
        exact = sh.exact_keys(q)
        assert np.all(lo <= exact) and np.all(exact <= up)
        for k in ks:
            least, most = sh.survivors(q, k)
            print("n=%d d=%d k=%d: %d..%d survivors (%.3f of the rows)" % (n, d, k, least, most, most / n))
            assert k <= least <= most <= (M.MAX_SHARE - MARGIN) * n
            assert most - least <= 0.01 * n  # the model's margins decide all but a sliver of the rows


def test_unit_corpus_stays_above_the_threshold():
    n, d, k = 20_037, 768, 100
    rows, qs = M.unit_corpus(np.random.default_rng(100 * d), n, d)
    sh = M.Shard(rows)
    for q in qs:
        least, most = sh.survivors(q, k)
        print("unit rows: %d..%d survivors (%.3f of the rows)" % (least, most, least / n))
        assert least >= (M.MAX_SHARE + MARGIN) * n


def test_few_tiles_keep_every_row():
    rows, qs = M.spread_corpus(np.random.default_rng(5), 3_000, 64)
    assert M.Shard(rows).survivors(qs[0], 100) == (3_000, 3_000)
