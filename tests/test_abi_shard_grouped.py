"""CPU: the sharded entries of the plain grouped search (tsh_search_shard_grouped, tsh_search_shard_begin_grouped,
tsh_merge_candidates_grouped, tsh_search_sharded_grouped; include/tostore_hip.h).  The merge is pure host code:
hand-built blocks of the oracle's exact sums -- a 64-byte header plus 24-byte entries, a group's rows split over the
blocks -- must merge to the oracle's list with repeated groups dropped: ids equal, distances bit for bit.  The device
entries validate their arguments and refuse to compute without a device; the bindings carry all four."""
import ctypes
import math
import os
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, IP, COS = 0, 1, 2
NAMES = ("tsh_search_shard_grouped", "tsh_search_shard_begin_grouped", "tsh_merge_candidates_grouped",
         "tsh_search_sharded_grouped")


def _block(entries, cands, k, metric, row_base=0):
    """A candidate block exactly as the device writes it (tsh_kernels.hip.h BlockHeader/BlockEntry)."""
    b = bytearray(64 + 24 * entries)
    struct.pack_into("<8IqqI", b, 0, len(cands), entries, 0, 0, 0, 1 if len(cands) > entries else 0, k, metric,
                     row_base, 0, 0)
    for i, (rid, s0, s1) in enumerate(cands[:entries]):
        struct.pack_into("<qdd", b, 64 + 24 * i, rid, s0, s1)
    return bytes(b)


def _first_of_each_group(eids, edist, group_of, k):
    """The specification over an oracle list: (ids, dist, groups)"""
    keep, groups, seen = [], [], set()
    for i, gid in enumerate(eids):
        if len(keep) >= k:
            break
        g = int(group_of[gid]) if 0 <= gid < len(group_of) and group_of[gid] >= 0 else -1
        if g >= 0:
            if g in seen:
                continue
            seen.add(g)
        keep.append(i)
        groups.append(g)
    keep = np.asarray(keep, np.int64)
    return eids[keep], edist[keep], np.asarray(groups, np.int32)


def _same(got, want, what):
    ids, dist, cnt, grp = got
    wi, wd, wg = want
    c = int(cnt[0])
    assert c == len(wi), (what, c, len(wi))
    assert np.array_equal(ids[0, :c], wi), (what, ids[0, :c][:12], wi[:12])
    assert np.array_equal(dist[0, :c].view(np.uint64), wd.view(np.uint64)), (what, dist[0, :c][:12], wd[:12])
    assert np.array_equal(grp[0, :c], wg), (what, grp[0, :c][:12], wg[:12])
    assert np.all(ids[0, c:] == -1) and np.all(np.isnan(dist[0, c:])) and np.all(grp[0, c:] == -1), what


N, D = 600, 16
SPLITS = {1: [(0, 600)], 2: [(0, 237), (237, 600)], 5: [(0, 100), (100, 101), (101, 237), (237, 500), (500, 600)]}


@pytest.fixture(scope="module")
def corpus(oracle_mod):
    """600 x 16 rows with a crowd of ties that spans the blocks, one query per metric with the oracle's full list and
    every row's exact sums (computed once, never changed)."""
    rng = np.random.default_rng(43)
    rows = rng.standard_normal((N, D)).astype(np.float32)
    rows[180:250] = rows[20]  # ties with row 20, on both sides of the boundary at 237
    rows[505] = rows[20]      # ... and one in the last block
    out = {"rows": rows}
    for metric in (L2, IP, COS):
        q = rng.standard_normal(D).astype(np.float32)
        if metric == COS:
            q = oracle_mod.normalize_f32(q)
        eids, edist = oracle_mod.search_exhaustive(rows, q, metric, N)
        cands = [(i,) + oracle_mod.exact_sums(q, rows[i], metric) for i in range(N)]
        out[metric] = (q, eids, edist, cands)
    return out


def _layouts():
    rng = np.random.default_rng(5)
    mix = rng.integers(0, 60, N).astype(np.int32)
    mix[rng.random(N) < 0.3] = -3
    return {
        "mod50": (np.arange(N) % 50).astype(np.int32),       # every group has rows in every block
        "runs7": (np.arange(N) // 7).astype(np.int32),       # runs that straddle the block edges
        "mix": mix,
        "short": (np.arange(300) % 11).astype(np.int32),     # the array ends before the rows do: the rest is ungrouped
    }


def _merge(corpus, metric, k, group_of, n_blocks=2, thr=None, entries=640):
    from tostore_amd.sharded import merge_candidate_blocks

    q, _, _, cands = corpus[metric]
    blocks = b"".join(_block(entries, cands[lo:hi], k, metric, lo) for lo, hi in SPLITS[n_blocks])
    return merge_candidate_blocks(metric, D, q, k, thr, np.frombuffer(blocks, np.uint8), n_blocks, entries, group_of=group_of)


@pytest.mark.parametrize("metric", [L2, IP, COS])
@pytest.mark.parametrize("n_blocks", [1, 2, 5])
def test_grouped_merge_is_the_oracle_list_with_repeated_groups_dropped(corpus, metric, n_blocks):
    _, eids, edist, _ = corpus[metric]
    for name, group_of in _layouts().items():
        n_groups = len(_first_of_each_group(eids, edist, group_of, N + 1)[0])
        for k in (1, 7, 100, n_groups, n_groups + 5):  # (the last: k larger than the number of groups)
            _same(_merge(corpus, metric, k, group_of, n_blocks), _first_of_each_group(eids, edist, group_of, k), (name, k))


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_every_row_ungrouped_is_the_plain_merge_and_one_group_is_one_entry(corpus, metric):
    from tostore_amd.sharded import merge_candidate_blocks

    q, eids, edist, cands = corpus[metric]
    k, entries = 25, 640
    blocks = np.frombuffer(b"".join(_block(entries, cands[lo:hi], k, metric, lo) for lo, hi in SPLITS[5]), np.uint8)
    p_ids, p_dist, p_cnt = merge_candidate_blocks(metric, D, q, k, None, blocks, 5, entries)
    for group_of in (np.full(N, -1, np.int32), np.zeros(0, np.int32)):  # all -1, and n_group_of = 0
        g_ids, g_dist, g_cnt, g_grp = merge_candidate_blocks(metric, D, q, k, None, blocks, 5, entries, group_of=group_of)
        assert np.array_equal(g_cnt, p_cnt) and np.array_equal(g_ids, p_ids) and np.all(g_grp == -1)
        assert np.array_equal(g_dist.view(np.uint64), p_dist.view(np.uint64))
    ids, dist, cnt, grp = _merge(corpus, metric, k, np.full(N, 4, np.int32), 5)
    assert cnt[0] == 1 and ids[0, 0] == eids[0] and grp[0, 0] == 4
    assert dist[0, :1].view(np.uint64)[0] == edist[:1].view(np.uint64)[0]
    assert np.all(ids[0, 1:] == -1) and np.all(np.isnan(dist[0, 1:])) and np.all(grp[0, 1:] == -1)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_threshold_is_strict_about_its_own_distance(corpus, metric, oracle_mod):
    """A row AT the threshold stays, a row one ulp beyond it goes -- before the groups are dropped, so a group whose best
    row fails the threshold does not appear at all."""
    q, eids, edist, _ = corpus[metric]
    group_of = _layouts()["mod50"]
    dk = float(_first_of_each_group(eids, edist, group_of, 10)[1][-1])
    for thr in (dk, float(np.nextafter(dk, -np.inf)), float(np.nextafter(dk, np.inf)), math.inf, -math.inf, float(edist[0])):
        lst = oracle_mod.search_exhaustive(corpus["rows"], q, metric, N, thr)
        for k in (1, 10, 100):
            _same(_merge(corpus, metric, k, group_of, 5, thr=thr), _first_of_each_group(lst[0], lst[1], group_of, k), (thr, k))


def test_signed_zero_nan_and_the_id_tie_break():
    """double.compareTo: -0.0 before 0.0, every NaN last; two groups' equal bests in different blocks: the smaller id
    first, and the other group still appears.  IP makes every double a distance exactly (distance = -sum0)."""
    from tostore_amd.sharded import merge_candidate_blocks

    q = np.zeros(4, np.float32)
    # block 0: group 0's rows 40 (0.0) and 41 (NaN), group 1's row 42 (-0.0); block 1: group 2's row 7 (-0.0: ties with 42,
    # smaller id), group 3's row 8 (NaN only), group 0's row 9 (0.0: ties with 40, smaller id -- it represents group 0)
    b0 = [(40, -0.0, 0.0), (41, math.nan, 0.0), (42, 0.0, 0.0)]
    b1 = [(7, 0.0, 0.0), (8, math.nan, 0.0), (9, -0.0, 0.0)]
    group_of = np.full(64, -1, np.int32)
    group_of[[40, 41, 9]] = 0
    group_of[42] = 1
    group_of[7] = 2
    group_of[8] = 3
    buf = np.frombuffer(_block(8, b0, 10, IP) + _block(8, b1, 10, IP), np.uint8)
    ids, dist, cnt, grp = merge_candidate_blocks(IP, 4, q, 10, None, buf, 2, 8, group_of=group_of)
    assert cnt[0] == 4
    assert ids[0, :4].tolist() == [7, 42, 9, 8] and grp[0, :4].tolist() == [2, 1, 0, 3]
    assert [math.copysign(1, x) for x in dist[0, :3]] == [-1.0, -1.0, 1.0] and np.all(dist[0, :3] == 0.0)
    assert math.isnan(dist[0, 3])
    # cut inside the tie: the smaller id wins the one place
    ids, _, cnt, grp = merge_candidate_blocks(IP, 4, q, 1, None, buf, 2, 8, group_of=group_of)
    assert cnt[0] == 1 and ids[0, 0] == 7 and grp[0, 0] == 2
    # the same two rows in the SAME group: one entry, the smaller id
    group_of[42] = 2
    ids, _, cnt, grp = merge_candidate_blocks(IP, 4, q, 10, None, buf, 2, 8, group_of=group_of)
    assert cnt[0] == 3 and ids[0, :3].tolist() == [7, 9, 8] and grp[0, :3].tolist() == [2, 0, 3]


def test_grouped_merge_reports_truncated_blocks():
    from tostore_amd import _ffi
    from tostore_amd.sharded import merge_candidate_blocks

    cands = [(i, float(i), 0.0) for i in range(300)]
    group_of = (np.arange(300) // 3).astype(np.int32)
    blk = _block(128, cands, 10, L2)
    with pytest.raises(_ffi.TshError) as e:
        merge_candidate_blocks(L2, 4, np.zeros(4, np.float32), 10, None, np.frombuffer(blk, np.uint8), 1, 128, group_of=group_of)
    assert e.value.code == _ffi.TSH_E_OVERFLOW and e.value.needed_entries >= 300
    ne = e.value.needed_entries
    ids, dist, cnt, grp = merge_candidate_blocks(L2, 4, np.zeros(4, np.float32), 10, None,
                                                 np.frombuffer(_block(ne, cands, 10, L2), np.uint8), 1, ne, group_of=group_of)
    assert cnt[0] == 10 and ids[0].tolist() == list(range(0, 30, 3)) and grp[0].tolist() == list(range(10))
    assert dist[0].tolist() == [math.sqrt(i) for i in range(0, 30, 3)]


def test_argument_validation():
    """The grouped entries' own argument errors are answered before a device is looked for: both mask forms at once and
    a NULL groups handle are TSH_E_BAD_ARG; a bad group array is TSH_E_BAD_ARG in the merge; out_group is nullable; with
    good arguments and no device the device entries answer TSH_E_NO_DEVICE."""
    from tostore_amd import _ffi

    L = _ffi.lib()
    q = np.zeros(4, np.float32)
    qp = q.ctypes.data_as(_ffi.p_f32)
    ids, dist, cnt, grp, need = np.zeros(3, np.int64), np.zeros(3), np.zeros(1, np.int32), np.zeros(3, np.int32), ctypes.c_int32(0)
    idp, dp, cp, gp = (ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64), cnt.ctypes.data_as(_ffi.p_i32),
                       grp.ctypes.data_as(_ffi.p_i32))
    blk = np.frombuffer(_block(8, [(1, 1.0, 0.0), (2, 4.0, 0.0)], 3, L2), np.uint8)
    bp = blk.ctypes.data_as(ctypes.c_void_p)
    mask = np.full(1, 255, np.uint8)
    mp = mask.ctypes.data_as(_ffi.p_u8)
    fake = ctypes.c_void_p(8)  # (never dereferenced: the checks below stop before it is)
    group_of = np.zeros(4, np.int32)
    gop = group_of.ctypes.data_as(_ffi.p_i32)
    st = ctypes.c_void_p(1)
    # both mask forms at once
    assert L.tsh_search_shard_grouped(None, qp, 1, 3, mp, fake, fake, 8, bp, None) == _ffi.TSH_E_BAD_ARG
    assert "at most one" in _ffi.last_error()
    assert L.tsh_search_shard_begin_grouped(None, qp, 1, 3, mp, fake, fake, 8, bp, 0, ctypes.byref(st)) == _ffi.TSH_E_BAD_ARG
    assert not st.value  # (a failed begin leaves no handle behind)
    # NULL groups
    st = ctypes.c_void_p(1)
    assert L.tsh_search_shard_grouped(None, qp, 1, 3, None, None, None, 8, bp, None) == _ffi.TSH_E_BAD_ARG
    assert "groups is NULL" in _ffi.last_error()
    assert L.tsh_search_shard_begin_grouped(None, qp, 1, 3, None, None, None, 8, bp, 0, ctypes.byref(st)) == _ffi.TSH_E_BAD_ARG
    assert not st.value
    # the collective answers what is the same on every rank locally: a NULL communicator
    assert L.tsh_search_sharded_grouped(None, None, qp, 1, 3, math.nan, None, None, fake, idp, dp, gp, cp) in (
        _ffi.TSH_E_BAD_ARG, _ffi.TSH_E_NO_DEVICE)
    # the merge: a NULL array with a length, a negative length
    assert L.tsh_merge_candidates_grouped(L2, 4, qp, 1, 3, math.nan, None, 4, bp, 1, 8, idp, dp, gp, cp, ctypes.byref(need)) == _ffi.TSH_E_BAD_ARG
    assert "group_of" in _ffi.last_error()
    assert L.tsh_merge_candidates_grouped(L2, 4, qp, 1, 3, math.nan, gop, -1, bp, 1, 8, idp, dp, gp, cp, ctypes.byref(need)) == _ffi.TSH_E_BAD_ARG
    assert L.tsh_merge_candidates_grouped(3, 4, qp, 1, 3, math.nan, gop, 4, bp, 1, 8, idp, dp, gp, cp, ctypes.byref(need)) == _ffi.TSH_E_BAD_ARG
    assert L.tsh_merge_candidates_grouped(L2, 4, qp, 1, 3, math.nan, gop, 4, bp, 1, 8, None, dp, gp, cp, ctypes.byref(need)) == _ffi.TSH_E_BAD_ARG
    # valid calls of the host entry: rows 1 and 2 share group 0; out_group and needed_entries are nullable; k <= 0
    assert L.tsh_merge_candidates_grouped(L2, 4, qp, 1, 3, math.nan, gop, 4, bp, 1, 8, idp, dp, gp, cp, ctypes.byref(need)) == 0
    assert cnt[0] == 1 and ids[0] == 1 and dist[0] == 1.0 and grp[0] == 0 and ids[1] == -1 and math.isnan(dist[1]) and grp[1] == -1
    assert L.tsh_merge_candidates_grouped(L2, 4, qp, 1, 3, math.nan, None, 0, bp, 1, 8, idp, dp, None, cp, None) == 0
    assert cnt[0] == 2 and ids[:2].tolist() == [1, 2]
    assert L.tsh_merge_candidates_grouped(L2, 4, qp, 1, 0, math.nan, gop, 4, bp, 1, 8, None, None, None, cp, None) == 0
    assert cnt[0] == 0
    if L.tsh_device_count() > 0:
        return
    assert L.tsh_search_shard_grouped(None, qp, 1, 3, None, None, fake, 8, bp, None) == _ffi.TSH_E_NO_DEVICE
    assert L.tsh_search_shard_begin_grouped(None, qp, 1, 3, mp, None, fake, 8, bp, 0, ctypes.byref(st)) == _ffi.TSH_E_NO_DEVICE
    assert L.tsh_search_sharded_grouped(None, None, qp, 1, 3, math.nan, None, None, fake, idp, dp, gp, cp) == _ffi.TSH_E_NO_DEVICE
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
    for method in ("searchShardGrouped", "shardStreamBeginGrouped", "mergeCandidatesGrouped", "searchShardedGrouped"):
        assert method + "(" in bridge and method in integration, method
    for fn in (sharded.ShardedSearcher.search, sharded.ShardedSearcher.search_many, sharded.CommSearcher.search,
               sharded.CommSearcher.search_many):
        assert inspect.signature(fn).parameters["groups"].default is None, fn
    assert inspect.signature(sharded.merge_candidate_blocks).parameters["group_of"].default is None
    # the header no longer lists the sharded entries as missing under tsh_search_grouped
    assert "The tsh_search_shard* and tsh_search_sharded* entries." not in header.split("int32_t tsh_search_grouped(")[0]
