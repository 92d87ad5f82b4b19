"""GPU: consecutive big-shard scans on two streams (TSH_OPT_SCAN_STREAMS, tostore_amd/csrc/tsh_scan_overlap.h).

A big shard's scans over its int8 or fp16 copy alternate between the two scan streams when queries overlap, as small
shards' scans always have: the launch shapes differ (several waves per workgroup, a workgroup per two or four tiles), the
host side behind the decision -- the stream with fewer scans out, a tail queue per scan stream, the last query's tail
in order -- is the same.  The smallest shard that takes the big launch shape (d = 256, 6144 tiles and a ragged one:
403 MB of rows), the batched path off, held to the oracle: ids, counts and distance bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2 = 0
D, K, NQ = 256, 20, 24
N = 6144 * 64 + 37


def _same(got, ref, what=""):
    assert np.array_equal(got[2], ref[2]), "counts differ from the oracle's " + what
    assert np.array_equal(got[0], ref[0]), "ids differ from the oracle's " + what
    assert np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64)), "distance bits differ from the oracle's " + what


@pytest.fixture(scope="module")
def shard(oracle_mod):
    """Rows, 24 queries and the oracle's answer over all rows: made once, read only."""
    rng = np.random.default_rng(17)
    rows = rng.standard_normal((N, D), dtype=np.float32)
    rows *= rng.uniform(0.5, 2.0, size=(N, 1)).astype(np.float32)
    qs = rng.standard_normal((NQ, D), dtype=np.float32)
    ref = oracle_mod.search_heap_many_mt(rows, qs, L2, K)
    for a in (rows, qs) + tuple(ref):
        a.setflags(write=False)
    return {"rows": rows, "qs": qs, "ref": ref, "answers": {}}


def _open(rows, streams, i8=2, f16_masked=1):
    from tostore_amd import HipVectorIndex

    idx = HipVectorIndex(D, L2, capacity_rows=len(rows))
    idx.set_scan_i8(i8)
    idx.set_scan_f16_masked(f16_masked)
    idx.set_scan_streams(streams)
    idx.set_batch_min_nq(0)
    idx.append(0, rows)
    return idx


def _i8_call(shard, streams):
    """One call of 24 queries on the int8 route with TSH_OPT_SCAN_STREAMS = streams: the answer, kept per value."""
    if streams not in shard["answers"]:
        with _open(shard["rows"], streams) as idx:
            s0 = idx.scan_i8_stats()
            got = idx.search(shard["qs"], K)
            s1 = idx.scan_i8_stats()
        assert s1["scans"] - s0["scans"] == NQ and s1["redone"] == 0, (streams, s0, s1)
        shard["answers"][streams] = got
    return shard["answers"][streams]


def test_int8_route_two_streams_and_one(hip_lib, shard):
    """(a) 24 scans over the int8 copy on two streams: the oracle's answer, nothing redone; on one stream the same arrays."""
    two = _i8_call(shard, 2)
    _same(two, shard["ref"], "two streams")
    one = _i8_call(shard, 1)
    for a, b in zip(two, one):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), "one stream against two"


def test_fp16_masked_route_two_streams(hip_lib, oracle_mod, shard):
    """(b) one row deleted: every scan is a masked scan over the fp16 copy, in the dense shape (it keeps most rows)."""
    rows, qs = shard["rows"], shard["qs"]
    dead = int(shard["ref"][0][0, 0])  # the first query's nearest row
    live = np.ones(N, bool)
    live[dead] = False
    ref = oracle_mod.search_heap_many_mt(rows, qs, L2, K, None, np.packbits(live, bitorder="little"))
    assert not (ref[0] == dead).any()
    with _open(rows, 2, i8=0, f16_masked=2) as idx:
        idx.set_deleted(np.array([dead]))
        s0 = idx.scan_f16_stats()
        _same(idx.search(qs, K), ref, "fp16 masked, two streams")
        s1 = idx.scan_f16_stats()
        assert s1["scans"] - s0["scans"] == NQ and s1["redone"] == s0["redone"], (s0, s1)
        assert idx.scan_i8_stats()["scans"] == 0


def test_tickets_two_streams(hip_lib, shard):
    """(c) eight tickets out before the first wait, int8 route, two streams: every ticket is the oracle's answer."""
    ref = shard["ref"]
    with _open(shard["rows"], 2) as idx:
        s0 = idx.scan_i8_stats()
        tickets = [idx.submit(q, K) for q in shard["qs"][:8]]
        for i, t in enumerate(tickets):
            ids, dist = idx.wait(t)
            assert np.array_equal(ids, ref[0][i, :ref[2][i]]), i
            assert np.array_equal(dist.view(np.uint64), ref[1][i, :ref[2][i]].view(np.uint64)), i
        s1 = idx.scan_i8_stats()
        assert s1["scans"] - s0["scans"] == 8 and s1["redone"] == 0, (s0, s1)


def test_default_rule(hip_lib, shard):
    """(d) TSH_OPT_SCAN_STREAMS = 0: whichever way the rule routes this shard's int8 scans, the oracle's answer and
    case (a)'s."""
    got = _i8_call(shard, 0)
    _same(got, shard["ref"], "the rule")
    for a, b in zip(got, _i8_call(shard, 2)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the rule against two streams"
