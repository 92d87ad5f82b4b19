"""GPU: WHERE masks whose bits do NOT stop at the last row.  A caller's bitmap may be sized for capacity (every byte past
the last row 0xFF), or be the global one a rank is handed, its neighbours' rows kept; the library slices it to each
shard's rows (tsh_host_sync.h slice_mask) and must count, list and scan the shard's own rows only.  Every case: ids
and distances bit for bit equal to oracle_mod.search_exhaustive over the rows that are kept and live, the pointer and
the handle form of the same bitmap identical and taking the same route (the counters say which), HipMask.kept the
exact count.  The kept counts sit on the limits a few ghost rows would tip over: 16 384 rows for the exact path and
the batched listed mode, one kept row in 24 for the list scan and the listed mode."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
L2, IP, COS = 0, 1, 2
ROUTE = ("exact_scans", "list_scans", "batch_launches", "fallback_searches")


def _bits(keep):
    return np.packbits(np.asarray(keep, bool), bitorder="little")


def _cap_bits(keep, cap):
    """keep (one bool per row id) as a bitmap sized for `cap` row ids: every bit past len(keep) set"""
    full = np.ones(cap, bool)
    full[:len(keep)] = keep
    return _bits(full)


def _queries(oracle_mod, rng, nq, d, metric):
    q = rng.standard_normal((nq, d)).astype(np.float32)
    return np.stack([oracle_mod.normalize_f32(x) for x in q]) if metric == COS else q


def _oracle(oracle_mod, rows, qs, metric, k, eff, base=0):
    """per query (ids, dist): the exhaustive oracle over the rows `eff` keeps (their ids, + base)"""
    sel = np.flatnonzero(eff)
    sub = np.ascontiguousarray(rows[sel])
    out = []
    for q in qs:
        i, dist = oracle_mod.search_exhaustive(sub, q, metric, k)
        out.append((sel[i] + base, dist))
    return out


def _agree(got, want):
    ids, dist, cnt = got
    for i, (e, ed) in enumerate(want):
        assert cnt[i] == len(e), (i, cnt[i], len(e))
        assert np.array_equal(ids[i, :cnt[i]], e), i
        assert np.array_equal(dist[i, :cnt[i]].view(np.uint64), ed.view(np.uint64)), i


def _pair(idx, qs, k, bits, m, want):
    """the pointer form and the handle of one bitmap: both the oracle's answer, by the same route -> that route"""
    c0 = idx.counters()
    a = idx.search(qs, k, None, bits)
    c1 = idx.counters()
    b = idx.search(qs, k, None, m)
    c2 = idx.counters()
    _agree(a, want)
    _agree(b, want)
    ra = {c: c1[c] - c0[c] for c in ROUTE}
    rb = {c: c2[c] - c1[c] for c in ROUTE}
    assert ra == rb, ("the pointer and the handle took different routes", ra, rb)
    if ra["batch_launches"]:
        assert c1["batch_kernel_last"] == c2["batch_kernel_last"]
    assert ra["fallback_searches"] == 0
    return ra


def _tickets(idx, qs, k, bits, m, want):
    for form in (bits, m):
        ts = [idx.submit(q, k, form) for q in qs]
        for t, (e, ed) in zip(ts, want):
            ids, dist = idx.wait(t)
            assert np.array_equal(ids, e) and np.array_equal(dist.view(np.uint64), ed.view(np.uint64))


def _scan_paths(idx):
    """the three single-query settings (conftest's scan_path, per index): exact + wide pick, exact + one-workgroup
    select, the f32 pre-filter"""
    yield "exact"
    idx.set_exact_select(False)
    yield "exact_select"
    idx.set_exact_select(True)
    idx.set_exact_scan_rows(0)
    yield "prefilter"
    idx.set_exact_scan_rows(16384)


def _every_route(oracle_mod, idx, rows, rng, metric, bits, m, eff, base=0, ks=(1, 100), listed=None):
    """nq = 1 on every scan path, a multi-query call below the batch threshold, tickets, the batched kernels 0 / 1 / 2"""
    d = rows.shape[1]
    qs = _queries(oracle_mod, rng, 4, d, metric)
    routes = {}
    idx.set_batch_min_nq(0)
    for ki, k in enumerate(ks):
        want = _oracle(oracle_mod, rows, qs, metric, k, eff, base)
        for path in _scan_paths(idx):
            routes[(k, path)] = _pair(idx, qs[:1], k, bits, m, want[:1])
        idx.set_batch_min_nq(16)  # (four queries: below the threshold, one by one)
        assert _pair(idx, qs, k, bits, m, want)["batch_launches"] == 0
        _tickets(idx, qs[:2], k, bits, m, want[:2])
        idx.set_batch_min_nq(2)
        for kern in (2, 1, 0):  # (2 first: its listed mode builds no fp16 copy of the shard, which the check below sees)
            idx.set_batch_kernel(kern)
            r0 = idx.counters()["bytes_resident"]
            r = _pair(idx, qs, k, bits, m, want)
            assert r["batch_launches"] >= 1, (kern, r)
            if kern == 2 and ki == 0 and listed is not None:  # (the first batched call on this index: no fp16 copy yet)
                grew = idx.counters()["bytes_resident"] - r0
                assert grew < listed, ("a dense pass built the fp16 copy of the shard: not listed mode", grew)
        idx.set_batch_kernel(3)
        idx.set_batch_min_nq(0)
    return routes


# rows, d, metric, kept: rows % 8 in {1, 7}, rows % 64 in {1, 63}; the kept count on the limit the capacity's ghost bits
# in the last byte (7, 1, 7 of them) would tip over -- 16 384 for the exact path and listed mode with 16 384 * 24 =
# 393 216 < rows (list scan and listed mode), 341 * 24 <= 8191 < 342 * 24, 170 * 24 <= 4097 < 171 * 24 (listed mode)
@pytest.mark.parametrize("n,d,metric,kept", [(393_217, 100, L2, 16_384), (8_191, 768, COS, 341), (4_097, 4, IP, 170)])
def test_one_index_ragged_length_capacity_bitmap(hip_lib, oracle_mod, n, d, metric, kept):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(n)
    cap = (n + 7) // 8 * 8 + 64
    rows = rng.standard_normal((cap, d)).astype(np.float32)
    keep = np.zeros(n, bool)
    keep[rng.choice(n - 1, kept - 1, replace=False)] = True
    keep[n - 1] = True  # (the last row shares its byte with the ghost bits)
    bits = _cap_bits(keep, cap)
    with HipVectorIndex(d, metric, capacity_rows=cap) as idx:
        idx.append(0, rows[:n])
        with idx.make_mask(bits) as m:
            assert m.kept == kept
            routes = _every_route(oracle_mod, idx, rows[:n], rng, metric, bits, m, keep,
                                  listed=n * d // 2 if n * d >= 20_000_000 else None)  # (the fp16 copy: 2 n d bytes)
            # a lone query reads the kept rows' list -- by their exact sums, or by the list scan: the route one ghost
            # row more would have closed (past 16 384 kept rows, or past one in 24)
            assert routes[(100, "exact")] == {"exact_scans": 1, "list_scans": 1, "batch_launches": 0, "fallback_searches": 0}
            assert routes[(100, "prefilter")] == {"exact_scans": 0, "list_scans": 1, "batch_launches": 0, "fallback_searches": 0}
            # fewer kept rows than k: the last row and two more
            few = np.zeros(n, bool)
            few[[0, n // 2, n - 1]] = True
            fb = _cap_bits(few, cap)
            with idx.make_mask(fb) as mf:
                assert mf.kept == 3
                qs = _queries(oracle_mod, rng, 2, d, metric)
                idx.set_batch_min_nq(0)
                _pair(idx, qs, 8, fb, mf, _oracle(oracle_mod, rows[:n], qs, metric, 8, few))
                idx.set_batch_min_nq(2)
                _pair(idx, qs, 8, fb, mf, _oracle(oracle_mod, rows[:n], qs, metric, 8, few))
                idx.set_batch_min_nq(0)
            # the ghost positions filled: those rows are inside the caller's bytes, so they are kept now
            idx.append(n, rows[n:])
            eff = np.ones(cap, bool)
            eff[:n] = keep
            assert m.kept == kept + cap - n
            qs = _queries(oracle_mod, rng, 3, d, metric)
            for nq_min in (0, 2):
                idx.set_batch_min_nq(nq_min)
                _pair(idx, qs, 100, bits, m, _oracle(oracle_mod, rows, qs, metric, 100, eff))


# a shard handle: row_base % 8 in {0, 3} x rows % 8 in {0, 5}; the global bitmap keeps 90 % of the neighbours' rows on
# both sides, the shard's own at 208 / 5000 (208 * 24 <= 5000 < 209 * 24: listed mode) and at 40 % (dense)
@pytest.mark.parametrize("base,n,metric", [(12_344, 5_000, L2), (12_347, 5_005, IP), (12_344, 5_005, COS), (12_347, 5_000, L2)])
def test_shard_handle_inside_a_global_bitmap(hip_lib, oracle_mod, base, n, metric):
    from tostore_amd import HipVectorIndex

    rng = np.random.default_rng(base + n + metric)
    d = 100
    rows = rng.standard_normal((n, d)).astype(np.float32)
    total = base + n + 203
    with HipVectorIndex(d, metric, capacity_rows=n, shard_device=0, row_base=base) as idx:
        idx.append(base, rows)
        for kept in (208, 2000):
            g = rng.random(total) < 0.9
            keep = np.zeros(n, bool)
            keep[rng.choice(n, kept, replace=False)] = True
            g[base:base + n] = keep
            bits = _bits(g)
            with idx.make_mask(bits) as m:
                assert m.kept == kept
                _every_route(oracle_mod, idx, rows, rng, metric, bits, m, keep, base, ks=(100,))


def test_in_process_shards_partly_filled(hip_lib, oracle_mod):
    """n_devices = 3 in one process (sharing the one GPU): capacity 70 000 puts the shards at 0, 23 360, 46 720; 30 001
    rows fill the first, end the second inside a byte (6641 rows), leave the third empty.  The bitmap is sized for
    capacity."""
    from tostore_amd import HipVectorIndex, _ffi

    rng = np.random.default_rng(33)
    cap, n, d, k = 70_000, 30_001, 64, 50
    rows = rng.standard_normal((n, d)).astype(np.float32)
    os.environ["TSH_SHARDS_SHARE_DEVICES"] = "1"
    _ffi.enable_test_hooks()
    try:
        with HipVectorIndex(d, L2, capacity_rows=cap, n_devices=3) as idx:
            idx.append(0, rows)
            for frac in (0.02, 0.5):
                keep = rng.random(n) < frac
                keep[n - 1] = True
                bits = _cap_bits(keep, cap)
                with idx.make_mask(bits) as m:
                    assert m.kept == int(keep.sum())
                    qs = _queries(oracle_mod, rng, 3, d, L2)
                    want = _oracle(oracle_mod, rows, qs, L2, k, keep)
                    idx.set_batch_min_nq(0)
                    _pair(idx, qs[:1], k, bits, m, want[:1])
                    _pair(idx, qs, k, bits, m, want)
                    _tickets(idx, qs, k, bits, m, want)
                    idx.set_batch_min_nq(2)
                    assert _pair(idx, qs, k, bits, m, want)["batch_launches"] >= 1
    finally:
        _ffi.enable_test_hooks(False)
        del os.environ["TSH_SHARDS_SHARE_DEVICES"]


def test_per_rank_shards_from_one_global_bitmap(hip_lib, oracle_mod, tmp_path):
    """tsh_index_open_ngh_shard, W = 3 ranks of 12 350 rows (ranges [0, 4117), [4117, 8234), [8234, 12 350): bases and
    ends inside bytes), every rank's handle made from the same global bitmap, sized for capacity.  The ranks' kept
    counts sum to the global one; their candidate blocks (pointer form), merged, and their top k (handle), merged, are
    the oracle's answer over the kept, live rows."""
    import torch

    from oracle import ngh_dir
    from tostore_amd import HipVectorIndex, _ffi
    from tostore_amd.sharded import merge_candidate_blocks

    rng = np.random.default_rng(44)
    n, d, W, k = 12_350, 100, 3, 40
    v = (rng.standard_normal((n, d)) * 0.4).astype(np.float32)
    deleted = sorted(set(rng.integers(0, n, 300).tolist()))
    root = tmp_path / "ngh"
    ngh_dir.write_ngh_dir(str(root), v, metric=L2, precision=1, deleted=deleted)
    _, vec, dead = ngh_dir.read_ngh_dir(str(root))
    L = _ffi.lib()
    for frac in (0.03, 0.6):
        keep = rng.random(n) < frac
        keep[[4116, 4117, 8233, 8234, n - 1]] = True
        bits = _cap_bits(keep, n + 70)
        eff = keep & ~dead
        qs = _queries(oracle_mod, rng, 3, d, L2)
        want = _oracle(oracle_mod, vec, qs, L2, k, eff)
        shards, masks = [], []
        try:
            for r in range(W):
                idx, info = HipVectorIndex.open_ngh_shard(str(root), W, r, device=0)
                shards.append(idx)
                masks.append(idx.make_mask(bits))
                lo, hi = info["row_base"], info["row_end"]
                assert masks[-1].kept == int(keep[lo:hi].sum()), r
            assert sum(m.kept for m in masks) == int(keep.sum())
            entries = L.tsh_default_block_entries(k)
            bb = L.tsh_candidate_block_bytes(entries)
            q = np.ascontiguousarray(qs, np.float32)
            bufs = []
            for idx in shards:
                buf = torch.empty(len(q) * bb, dtype=torch.uint8, device="cuda")
                _ffi.check(L.tsh_search_shard(idx._h, q.ctypes.data_as(_ffi.p_f32), len(q), k,
                                              bits.ctypes.data_as(_ffi.p_u8), entries, ctypes.c_void_p(buf.data_ptr()), None))
                bufs.append(buf)
            _agree(merge_candidate_blocks(L2, d, q, k, None, torch.cat(bufs).cpu().numpy(), W, entries), want)
            # each rank's own top k with its handle (global ids), merged by (distance, id)
            per = [idx.search(qs, k, None, m) for idx, m in zip(shards, masks)]
            for idx, m, got in zip(shards, masks, per):
                assert _pair(idx, qs, k, bits, m, [(got[0][i, :got[2][i]], got[1][i, :got[2][i]]) for i in range(len(qs))]) is not None
            for i, (e, ed) in enumerate(want):
                ids = np.concatenate([g[0][i, :g[2][i]] for g in per])
                dist = np.concatenate([g[1][i, :g[2][i]] for g in per])
                o = np.lexsort((ids, dist))[:k]
                assert np.array_equal(ids[o], e) and np.array_equal(dist[o].view(np.uint64), ed.view(np.uint64)), i
        finally:
            for m in masks:
                m.close()
            for idx in shards:
                idx.close()
