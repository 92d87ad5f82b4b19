"""GPU: a pipelined call's queries are finalised as their blocks land (SearchOut::on_block, tsh_lib.hip).

56 000 x 768 f32 rows are just above the 160 MiB below which two threads submit a call's queries: here one thread does,
and it orders and cuts query q into the caller's arrays while the GPU scans the next ones.  Whatever the call's size --
a lone query, fewer than the pipeline's depth of 8, exactly that, one more, 64, 65 -- every query's ids, distances and
count must be, bit for bit, what the same query gives when asked alone; with a distance threshold that cuts some lists
short; and page after page of a cursor search over a multi-query call.  The 65-query call is held to the oracle too."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2 = 0
N, D, K = 56_000, 768, 100
SIZES = (1, 7, 8, 9, 64, 65)


@functools.lru_cache(maxsize=None)
def _corpus():
    rng = np.random.default_rng(56)
    rows = rng.standard_normal((N, D), dtype=np.float32)
    rows *= rng.uniform(0.5, 2.0, size=(N, 1)).astype(np.float32)
    qs = rng.standard_normal((65, D), dtype=np.float32)
    rows.setflags(write=False)
    qs.setflags(write=False)
    return rows, qs


@pytest.fixture(scope="module")
def index(hip_lib):
    from tostore_amd import HipVectorIndex

    rows, _ = _corpus()
    assert rows.nbytes > 160 << 20
    with HipVectorIndex(D, L2, capacity_rows=N) as idx:
        idx.set_batch_min_nq(0)  # the single-query pipeline for every call
        idx.append(0, rows)
        yield idx


def _same(got, ref, what):
    assert np.array_equal(got[2], ref[2]), "counts differ: " + what
    assert np.array_equal(got[0], ref[0]), "ids differ: " + what
    assert np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), "distance bits differ: " + what


def _one_by_one(fn, qs, *extra):
    parts = [fn(qs[i:i + 1], *[e[i:i + 1] if isinstance(e, np.ndarray) else e for e in extra]) for i in range(len(qs))]
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))


def test_calls_equal_lone_queries(index, oracle_mod):
    rows, qs = _corpus()
    lone = _one_by_one(lambda q: index.search(q, K), qs)
    _same(lone, oracle_mod.search_heap_many_mt(rows, qs, L2, K), "lone queries against the oracle")
    assert (lone[2] == K).all()
    for nq in SIZES:
        _same(index.search(qs[:nq], K), tuple(x[:nq] for x in lone), "a call of %d" % nq)


def test_calls_equal_lone_queries_with_a_threshold(index, oracle_mod):
    """A threshold at the median of the queries' 50th distances: about half the lists are cut short."""
    rows, qs = _corpus()
    full = index.search(qs, K)
    thr = float(np.median(full[1][:, 49]))
    lone = _one_by_one(lambda q: index.search(q, K, thr), qs)
    _same(lone, oracle_mod.search_heap_many_mt(rows, qs, L2, K, thr), "lone queries against the oracle")
    assert (lone[2] < K).any() and (lone[2] > 0).any() and len(set(lone[2].tolist())) > 2
    for nq in SIZES:
        _same(index.search(qs[:nq], K, thr), tuple(x[:nq] for x in lone), "a call of %d" % nq)


def test_cursor_pages_of_a_multi_query_call(index):
    """Three pages of 40 for nine queries at once against the same pages asked query by query."""
    _, qs = _corpus()
    qs = qs[:9]
    k = 40
    after = (np.full(len(qs), -np.inf), np.zeros(len(qs), np.int64))
    seen = []
    for page in range(3):
        got = index.search_after(qs, k, after)
        lone = _one_by_one(lambda q, a_d, a_i: index.search_after(q, k, (a_d, a_i)), qs, after[0], after[1])
        _same(got, lone, "page %d" % page)
        assert (got[2] == k).all()
        seen.append(got[0])
        after = (got[1][:, -1].copy(), got[0][:, -1].copy())
    whole = index.search(qs, 3 * k)
    assert np.array_equal(np.concatenate(seen, axis=1), whole[0])
