"""CPU: the sharded cursor entries (tsh_search_shard_after, tsh_search_shard_begin_after, tsh_merge_candidates_after,
tsh_search_sharded_after; include/tostore_hip.h).  The merge is pure host code: hand-built blocks of the oracle's exact
sums, merged behind a cursor, must give the oracle's list after that cursor -- ids equal, distances bit for bit.  The
device entries validate their cursor arrays and refuse to compute without a device; the bindings carry all four."""
import ctypes
import math
import os
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, IP, COS = 0, 1, 2
NAMES = ("tsh_search_shard_after", "tsh_search_shard_begin_after", "tsh_merge_candidates_after", "tsh_search_sharded_after")


def _block(entries, cands, k, metric, row_base=0):
    """A candidate block exactly as the device writes it (tsh_kernels.hip.h BlockHeader/BlockEntry)."""
    b = bytearray(64 + 24 * entries)
    struct.pack_into("<8IqqI", b, 0, len(cands), entries, 0, 0, 0, 1 if len(cands) > entries else 0, k, metric,
                     row_base, 0, 0)
    for i, (rid, s0, s1) in enumerate(cands[:entries]):
        struct.pack_into("<qdd", b, 64 + 24 * i, rid, s0, s1)
    return bytes(b)


def _same_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


@pytest.fixture(scope="module")
def corpus(oracle_mod):
    """600 x 16 rows in three "shards" with a crowd of ties that spans two of them, one query per metric with the
    oracle's full list, and per shard every row's exact sums as block entries (computed once, never changed)."""
    rng = np.random.default_rng(41)
    n, d = 600, 16
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[180:230] = rows[20]  # ties with row 20, on both sides of the boundary at 200
    rows[405] = rows[20]      # ... and one in the third shard
    bounds = [(0, 200), (200, 400), (400, 600)]
    out = {"rows": rows, "bounds": bounds, "d": d, "n": n}
    for metric in (L2, IP, COS):
        q = rng.standard_normal(d).astype(np.float32)
        if metric == COS:
            q = oracle_mod.normalize_f32(q)
        eids, edist = oracle_mod.search_exhaustive(rows, q, metric, n)
        cands = [[(i,) + oracle_mod.exact_sums(q, rows[i], metric) for i in range(lo, hi)] for lo, hi in bounds]
        out[metric] = (q, eids, edist, cands)
    return out


def _merge(corpus, metric, k, after, thr=None, cands=None, entries=256):
    from tostore_amd.sharded import merge_candidate_blocks

    q, _, _, all_cands = corpus[metric]
    cands = all_cands if cands is None else cands
    blocks = b"".join(_block(entries, c, k, metric, lo) for c, (lo, _) in zip(cands, corpus["bounds"]))
    return merge_candidate_blocks(metric, corpus["d"], q, k, thr, np.frombuffer(blocks, np.uint8), len(cands), entries, after=after)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_merge_after_is_the_oracle_list_after_the_cursor(corpus, metric):
    """The blocks hold rows before the cursor, the cursor's own row and rows tied with the cursor's distance, in
    different blocks: the answer is the oracle's list past the cursor, cut to k -- at every position of the crowd."""
    q, eids, edist, _ = corpus[metric]
    k = 9
    first = int(np.flatnonzero(eids == 20)[0])  # the crowd: row 20, rows 180 .. 229 and row 405, in id order
    assert np.array_equal(eids[first:first + 52], np.asarray([20] + list(range(180, 230)) + [405]))
    for at in (0, 5, first - 1, first, first + 10, first + 20, first + 21, first + 50, first + 51, 300, 590, 598, 599):
        ids, dist, cnt = _merge(corpus, metric, k, (float(edist[at]), int(eids[at])))
        want = min(k, 599 - at)
        assert cnt[0] == want, at
        assert np.array_equal(ids[0, :want], eids[at + 1:at + 1 + want]), at
        assert _same_dist(dist[0, :want], edist[at + 1:at + 1 + want]), at
        assert np.all(ids[0, want:] == -1) and np.all(np.isnan(dist[0, want:]))
    # a threshold cuts the page
    at = first + 45
    ids, dist, cnt = _merge(corpus, metric, k, (float(edist[at]), int(eids[at])), thr=float(edist[at + 6]))
    last = at + 6
    while last + 1 < 600 and edist[last + 1] == edist[at + 6]:
        last += 1
    want = min(k, last - at)
    assert cnt[0] == want and np.array_equal(ids[0, :want], eids[at + 1:at + 1 + want])
    # a cursor per query: two queries, two cursors, blocks in [block][query] layout
    from tostore_amd.sharded import merge_candidate_blocks

    cands = corpus[metric][3]
    blocks = b"".join(_block(256, c, k, metric, lo) * 2 for c, (lo, _) in zip(cands, corpus["bounds"]))
    after = [(float(edist[3]), int(eids[3])), (float(edist[400]), int(eids[400]))]
    ids, dist, cnt = merge_candidate_blocks(metric, corpus["d"], np.stack([q, q]), k, None, np.frombuffer(blocks, np.uint8), 3, 256, after=after)
    for i, at in enumerate((3, 400)):
        assert cnt[i] == k and np.array_equal(ids[i], eids[at + 1:at + 1 + k]) and _same_dist(dist[i], edist[at + 1:at + 1 + k])


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_minus_inf_cursor_is_the_plain_merge(corpus, metric):
    k = 25
    p_ids, p_dist, p_cnt = _merge(corpus, metric, k, None)
    for any_id in (0, -7, 2**40):
        a_ids, a_dist, a_cnt = _merge(corpus, metric, k, (-math.inf, any_id))
        assert np.array_equal(a_cnt, p_cnt) and np.array_equal(a_ids, p_ids)
        assert np.array_equal(a_dist.view(np.uint64), p_dist.view(np.uint64))


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_cursor_that_names_no_row(corpus, metric):
    q, eids, edist, _ = corpus[metric]
    k = 6
    a, b = float(edist[299]), float(edist[300])
    mid = (a + b) / 2
    assert a < mid < b
    ids, dist, cnt = _merge(corpus, metric, k, (mid, 0))
    assert cnt[0] == k and np.array_equal(ids[0], eids[300:306]) and _same_dist(dist[0], edist[300:306])
    # at a row's distance, an id no row has: below every tied id, and above
    ids, _, _ = _merge(corpus, metric, k, (b, -1))
    assert np.array_equal(ids[0], eids[300:306])
    ids, _, _ = _merge(corpus, metric, k, (b, 2**40))
    assert np.array_equal(ids[0], eids[301:307])
    # past everything
    assert _merge(corpus, metric, k, (float(edist[-1]), 2**40))[2][0] == 0
    assert _merge(corpus, metric, k, (math.inf, 0))[2][0] == 0
    assert _merge(corpus, metric, k, (math.nan, 0))[2][0] == 0


def test_signed_zero_and_nan_order():
    """double.compareTo as tests/cpp/after_band_test.cpp pins it for the cursor filter: -inf < negatives < -0.0 < 0.0 <
    positives < +inf < NaN, every NaN the one last key, ties by id; an entry follows the cursor iff it is strictly greater
    in (key, id).  IP makes every double a distance exactly (distance = -sum0)."""
    from tostore_amd.sharded import merge_candidate_blocks

    ladder = [-math.inf, -3.5, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.0000000000000002, math.inf, math.nan]
    ids_at = (0, 6, 7, 8, 2**41)
    # every (rung, id) as one entry, split over three blocks
    ent = [(rid, -v, 0.0) for v in ladder for rid in ids_at]
    ent[-1] = (ent[-1][0], math.copysign(math.nan, 1.0), 0.0)  # (a NaN of the other sign: the same key)
    order = [(j, rid) for j in range(len(ladder)) for rid in ids_at]
    perm = np.random.default_rng(2).permutation(len(ent))
    parts = [[ent[i] for i in perm[a::3]] for a in range(3)]
    blocks = b"".join(_block(64, p, len(ent), IP) for p in parts)
    buf = np.frombuffer(blocks, np.uint8)
    k = len(ent)
    for i, cv in enumerate(ladder):
        for cid in (-1, 0, 7, 2**40):
            ids, dist, cnt = merge_candidate_blocks(IP, 4, np.zeros(4, np.float32), k, None, buf, 3, 64, after=(cv, cid))
            want = [(j, rid) for j, rid in order if j > i or (j == i and rid > cid)]
            if cv == -math.inf:
                want = order  # "from the start", whatever the id: the -inf rows themselves included
            assert cnt[0] == len(want), (cv, cid)
            assert ids[0, :cnt[0]].tolist() == [rid for _, rid in want], (cv, cid)
            for g, (j, _) in zip(dist[0, :cnt[0]], want):
                w = ladder[j]
                assert (math.isnan(g) and math.isnan(w)) or (g == w and math.copysign(1, g) == math.copysign(1, w)), (cv, cid)


def test_merge_after_reports_truncated_blocks():
    from tostore_amd import _ffi
    from tostore_amd.sharded import merge_candidate_blocks

    cands = [(i, float(i), 0.0) for i in range(300)]
    blk = _block(128, cands, 10, L2)
    with pytest.raises(_ffi.TshError) as e:
        merge_candidate_blocks(L2, 4, np.zeros(4, np.float32), 10, None, np.frombuffer(blk, np.uint8), 1, 128, after=(2.0, 4))
    assert e.value.code == _ffi.TSH_E_OVERFLOW and e.value.needed_entries >= 300
    ids, dist, cnt = merge_candidate_blocks(L2, 4, np.zeros(4, np.float32), 10, None,
                                            np.frombuffer(_block(e.value.needed_entries, cands, 10, L2), np.uint8), 1,
                                            e.value.needed_entries, after=(2.0, 4))
    assert cnt[0] == 10 and ids[0].tolist() == list(range(5, 15)) and dist[0].tolist() == [math.sqrt(i) for i in range(5, 15)]


def test_argument_validation():
    """NULL cursor arrays are TSH_E_BAD_ARG on all four entries, before anything else is looked at; with cursors and
    no device the device entries answer TSH_E_NO_DEVICE."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    q = np.zeros(4, np.float32)
    qp = q.ctypes.data_as(_ffi.p_f32)
    ad, ai = np.zeros(1), np.zeros(1, np.int64)
    adp, aip = ad.ctypes.data_as(_ffi.p_f64), ai.ctypes.data_as(_ffi.p_i64)
    ids, dist, cnt, need = np.zeros(3, np.int64), np.zeros(3), np.zeros(1, np.int32), ctypes.c_int32(0)
    idp, dp, cp = ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64), cnt.ctypes.data_as(_ffi.p_i32)
    blk = np.frombuffer(_block(8, [(1, 1.0, 0.0)], 3, L2), np.uint8)
    bp = blk.ctypes.data_as(ctypes.c_void_p)
    st = ctypes.c_void_p(1)
    for a, b in ((None, aip), (adp, None), (None, None)):
        assert L.tsh_merge_candidates_after(L2, 4, qp, 1, 3, math.nan, a, b, bp, 1, 8, idp, dp, cp, ctypes.byref(need)) == _ffi.TSH_E_BAD_ARG
        assert "after_dist" in _ffi.last_error()
        assert L.tsh_search_shard_after(None, qp, 1, 3, None, a, b, 8, bp, None) == _ffi.TSH_E_BAD_ARG
        assert L.tsh_search_shard_begin_after(None, qp, 1, 3, None, a, b, 8, bp, 0, ctypes.byref(st)) == _ffi.TSH_E_BAD_ARG
        assert not st.value  # (a failed begin leaves no handle behind)
        st = ctypes.c_void_p(1)
        assert L.tsh_search_sharded_after(None, None, qp, 1, 3, math.nan, None, a, b, idp, dp, cp) == _ffi.TSH_E_BAD_ARG
    # a valid call of the host entry
    assert L.tsh_merge_candidates_after(L2, 4, qp, 1, 3, math.nan, adp, aip, bp, 1, 8, idp, dp, cp, ctypes.byref(need)) == 0
    assert cnt[0] == 1 and ids[0] == 1 and dist[0] == 1.0
    if L.tsh_device_count() > 0:
        return
    assert L.tsh_search_shard_after(None, qp, 1, 3, None, adp, aip, 8, bp, None) == _ffi.TSH_E_NO_DEVICE
    assert L.tsh_search_shard_begin_after(None, qp, 1, 3, None, adp, aip, 8, bp, 0, ctypes.byref(st)) == _ffi.TSH_E_NO_DEVICE
    assert L.tsh_search_sharded_after(None, None, qp, 1, 3, math.nan, None, adp, aip, idp, dp, cp) == _ffi.TSH_E_NO_DEVICE
    assert "no HIP device" in _ffi.last_error()


def test_bindings_carry_the_four_entries():
    import inspect

    from tostore_amd import _ffi, sharded

    bridge = open(os.path.join(ROOT, "tostore_amd", "dart", "tostore_hip_bridge.dart")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header = open(os.path.join(ROOT, "include", "tostore_hip.h")).read()
    src = inspect.getsource(sharded)
    for name in NAMES:
        assert name in _ffi.SIGNATURES and hasattr(_ffi.lib(), name), name
        assert name + "(" in header and "'%s'" % name in bridge and "`%s`" % name in integration, name
        assert "." + name + "(" in src, name + " is not called by sharded.py"
    for method in ("searchShardAfter", "shardStreamBeginAfter", "mergeCandidatesAfter", "searchShardedAfter"):
        assert method + "(" in bridge and method in integration, method
    for fn in (sharded.merge_candidate_blocks, sharded.ShardedSearcher.search, sharded.ShardedSearcher.search_many,
               sharded.CommSearcher.search, sharded.CommSearcher.search_many):
        assert inspect.signature(fn).parameters["after"].default is None, fn
