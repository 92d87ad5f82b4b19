"""GPU: mask handles in the sharded entries (tsh_search_shard_masked, tsh_search_shard_begin_masked; include/tostore_hip.h).
One corpus of 13 001 x 256 rows in three shard handles on the test box's GPU -- every shard large enough for a selective
handle to get its device list, no base a multiple of 8.  The yardstick of every case: the blocks the handle entry writes,
merged on the host, equal the merge of the POINTER entry's blocks for the bitmap the handle was made from -- ids equal,
distances bit for bit -- and both equal oracle.search_exhaustive over the kept live rows."""
import ctypes
import math
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L2, IP, COS = 0, 1, 2
N, D = 13_001, 256
BOUNDS = [(0, 4099), (4099, 8713), (8713, N)]
K = 10
START = (-math.inf, 0)


def _bits(keep, n_bytes=None):
    b = np.packbits(np.asarray(keep, bool), bitorder="little")
    return b if n_bytes is None else b[:n_bytes].copy()


def _extended(bits, n_rows):
    """the bitmap zero-extended to n_rows bits (what a handle makes of a bitmap that ends early)"""
    out = np.zeros((n_rows + 7) // 8, np.uint8)
    m = min(len(out), len(bits))
    out[:m] = bits[:m]
    return out


def _same(a, b, what=""):
    assert np.array_equal(a[2], b[2]), "counts differ " + what
    assert np.array_equal(a[0], b[0]), "ids differ " + what
    da, db = np.asarray(a[1], np.float64), np.asarray(b[1], np.float64)
    nan = np.isnan(da)  # (a NaN distance is one key, whatever its payload; the padding behind a short list is NaN too)
    assert np.array_equal(nan, np.isnan(db)), "NaN distances differ " + what
    assert np.array_equal(da[~nan].view(np.uint64), db[~nan].view(np.uint64)), "distance bits differ " + what


def _decode(block):
    count, entries = struct.unpack_from("<II", block, 0)
    return count, entries, [struct.unpack_from("<qdd", block, 64 + 24 * i) for i in range(min(count, entries))]


def _canonical(block):
    """a block up to the order of its entries (places drawn with atomic adds) and its generation tag"""
    count, entries, got = _decode(block)
    return count, entries, sorted(struct.pack("<qdd", *e) for e in got)


@pytest.fixture(scope="module")
def corpus(oracle_mod):
    """Rows, 64 queries per metric (cosine: normalised) and the two masks most cases share; computed once, never changed."""
    rng = np.random.default_rng(20261)
    rows = rng.standard_normal((N, D)).astype(np.float32)
    qs = {}
    for metric in (L2, IP, COS):
        q = rng.standard_normal((64, D)).astype(np.float32)
        qs[metric] = np.stack([oracle_mod.normalize_f32(x) for x in q]) if metric == COS else q
    few = rng.random(N) < 0.03
    half = rng.random(N) < 0.5
    return {"rows": rows, "qs": qs, "few": few, "half": half}


class Shards:
    """Shard handles (global ids) over one corpus on device 0 and the device buffer their blocks land in, [shard][query]."""

    def __init__(self, rows, metric, bounds=BOUNDS):
        from tostore_amd import HipVectorIndex

        self.metric, self.d, self.bounds = metric, rows.shape[1], list(bounds)
        self.idx = []
        for lo, hi in bounds:
            s = HipVectorIndex(self.d, metric, shard_device=0, row_base=lo)
            self.idx.append(s)
            s.append(lo, rows[lo:hi])
        self._bufs = {}

    def close(self):
        for s in self.idx:
            s.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def each(self, fn):
        for s in self.idx:
            fn(s)

    def handles(self, bits):
        """every shard's own handle of the same GLOBAL bitmap (n_bytes = len(bits))"""
        return [s.make_mask(bits) for s in self.idx]

    def _buffer(self, nq, entries):
        import torch

        from tostore_amd import _ffi

        bb = _ffi.lib().tsh_candidate_block_bytes(entries)
        key = (nq, entries)
        if key not in self._bufs:
            if len(self._bufs) > 4:
                self._bufs.clear()
            self._bufs[key] = torch.empty(len(self.idx) * nq * bb, dtype=torch.uint8, device="cuda")
        return self._bufs[key], bb

    def blocks(self, qs, k, mask=None, handles=None, after=None, entries=None):
        """One shard search per shard -> host copy [shard, nq * bb].  handles: the *_masked entry (an entry of the list
        may be None: no filter); else the pointer entry with `mask` (a bitmap for every shard's rows, or None)."""
        from tostore_amd import _ffi

        L = _ffi.lib()
        q = np.ascontiguousarray(qs, dtype=np.float32).reshape(-1, self.d)
        nq = q.shape[0]
        entries = L.tsh_default_block_entries(k) if entries is None else entries
        buf, bb = self._buffer(nq, entries)
        import torch

        buf.fill_(0xA5)
        torch.cuda.synchronize()  # (the library writes the blocks on streams of its own)
        qp = q.ctypes.data_as(_ffi.p_f32)
        ad = ai = None
        if after is not None:
            ad = np.ascontiguousarray(np.broadcast_to(np.asarray(after[0], dtype=np.float64).reshape(-1), (nq,)))
            ai = np.ascontiguousarray(np.broadcast_to(np.asarray(after[1], dtype=np.int64).reshape(-1), (nq,)))
        adp = None if ad is None else ad.ctypes.data_as(_ffi.p_f64)
        aip = None if ai is None else ai.ctypes.data_as(_ffi.p_i64)
        mp = None if mask is None else mask.ctypes.data_as(_ffi.p_u8)
        for g, s in enumerate(self.idx):
            at = ctypes.c_void_p(buf.data_ptr() + g * nq * bb)
            if handles is not None:
                h = None if handles[g] is None else handles[g].handle()
                _ffi.check(L.tsh_search_shard_masked(s._h, qp, nq, k, h, adp, aip, entries, at, None))
            elif after is None:
                _ffi.check(L.tsh_search_shard(s._h, qp, nq, k, mp, entries, at, None))
            else:
                _ffi.check(L.tsh_search_shard_after(s._h, qp, nq, k, mp, adp, aip, entries, at, None))
        return buf.cpu().numpy().reshape(len(self.idx), nq * bb), bb, entries

    def merged(self, qs, k, mask=None, handles=None, after=None, entries=None):
        from tostore_amd.sharded import merge_candidate_blocks

        q = np.ascontiguousarray(qs, dtype=np.float32).reshape(-1, self.d)
        host, bb, entries = self.blocks(q, k, mask, handles, after, entries)
        cur = None
        if after is not None:
            cur = (np.ascontiguousarray(np.broadcast_to(np.asarray(after[0], dtype=np.float64).reshape(-1), (len(q),))),
                   np.ascontiguousarray(np.broadcast_to(np.asarray(after[1], dtype=np.int64).reshape(-1), (len(q),))))
        return merge_candidate_blocks(self.metric, self.d, q, k, None, host, len(self.idx), entries, after=cur)


def _oracle(oracle_mod, rows, qs, metric, k, keep_bits):
    """(ids[nq,k], dist[nq,k], count[nq]) of search_exhaustive over the kept rows, padded as the merge pads"""
    q = np.asarray(qs, np.float32).reshape(-1, rows.shape[1])
    ids = np.full((len(q), k), -1, np.int64)
    dist = np.full((len(q), k), np.nan)
    cnt = np.zeros(len(q), np.int32)
    for i, x in enumerate(q):
        with np.errstate(all="ignore"):
            e_ids, e_dist = oracle_mod.search_exhaustive(rows, x, metric, k, None, keep_bits)
        cnt[i] = len(e_ids)
        ids[i, :cnt[i]], dist[i, :cnt[i]] = e_ids, e_dist
    return ids, dist, cnt


def _both_forms(sh, oracle_mod, rows, qs, k, bits, what, handle_bits=None, keep_bits=None):
    """The yardstick: handle blocks merged == pointer blocks merged == the oracle.  handle_bits: what the handles are
    made from when that is not `bits` itself (a bitmap that ends early; `bits` is then its zero-extension)."""
    hs = sh.handles(bits if handle_bits is None else handle_bits)
    try:
        by_handle = sh.merged(qs, k, handles=hs)
    finally:
        for h in hs:
            h.close()
    by_pointer = sh.merged(qs, k, mask=bits)
    _same(by_handle, by_pointer, what + ": handle against pointer")
    _same(by_handle, _oracle(oracle_mod, rows, qs, sh.metric, k, bits if keep_bits is None else keep_bits), what + ": against the oracle")
    return by_handle


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_selective_mask_exact_path_and_list_scan(hip_lib, oracle_mod, corpus, metric):
    """Cases 1 and 2: a keep-3 % mask takes the exact path over the handle's list; with the exact path off
    (TSH_OPT_EXACT_SCAN_ROWS = 0) the same list is scanned by the list scan."""
    rows, qs, bits = corpus["rows"], corpus["qs"][metric][:6], _bits(corpus["few"])
    with Shards(rows, metric) as sh:
        sh.each(lambda s: s.set_batch_min_nq(0))  # (every query its own search)
        c0 = [s.counters() for s in sh.idx]
        _both_forms(sh, oracle_mod, rows, qs, K, bits, "keep 3 %, exact path")
        c1 = [s.counters() for s in sh.idx]
        # (the exact sums of the listed rows: both counters move)
        assert all(b["exact_scans"] > a["exact_scans"] and b["list_scans"] > a["list_scans"] for a, b in zip(c0, c1)), (c0, c1)
        sh.each(lambda s: s.set_exact_scan_rows(0))
        _both_forms(sh, oracle_mod, rows, qs, K, bits, "keep 3 %, list scan")
        c2 = [s.counters() for s in sh.idx]
        assert all(b["list_scans"] > a["list_scans"] and b["exact_scans"] == a["exact_scans"] for a, b in zip(c1, c2)), (c1, c2)


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_dense_mask_on_every_tile_scan(hip_lib, oracle_mod, corpus, metric):
    """Case 3: a keep-50 % mask on the f32 masked tile scan, then forced onto the fp16 copy, then onto the int8 copy."""
    rows, qs, bits = corpus["rows"], corpus["qs"][metric][:6], _bits(corpus["half"])
    with Shards(rows, metric) as sh:
        sh.each(lambda s: (s.set_exact_scan_rows(0), s.set_batch_min_nq(0)))
        f0, i0 = [s.scan_f16_stats()["scans"] for s in sh.idx], [s.scan_i8_stats()["scans"] for s in sh.idx]
        c0 = [s.counters() for s in sh.idx]
        _both_forms(sh, oracle_mod, rows, qs, K, bits, "keep 50 %, f32")
        c1 = [s.counters() for s in sh.idx]
        assert all(b["scan_launches"] > a["scan_launches"] and b["list_scans"] == a["list_scans"] and b["exact_scans"] == a["exact_scans"]
                   for a, b in zip(c0, c1)), (c0, c1)
        assert [s.scan_f16_stats()["scans"] for s in sh.idx] == f0 and [s.scan_i8_stats()["scans"] for s in sh.idx] == i0
        sh.each(lambda s: s.set_scan_f16_masked(2))
        hs = sh.handles(bits)
        ref = _oracle(oracle_mod, rows, qs, metric, K, bits)
        _same(sh.merged(qs, K, handles=hs), ref, "keep 50 %, fp16, handle")
        f1 = [s.scan_f16_stats()["scans"] for s in sh.idx]
        assert all(b - a >= len(qs) for a, b in zip(f0, f1)), (f0, f1)  # the route ran, behind the handle
        _same(sh.merged(qs, K, mask=bits), ref, "keep 50 %, fp16, pointer")
        sh.each(lambda s: (s.set_scan_f16_masked(1), s.set_scan_i8_masked(2)))
        _same(sh.merged(qs, K, handles=hs), ref, "keep 50 %, int8, handle")
        i1 = [s.scan_i8_stats()["scans"] for s in sh.idx]
        assert all(b - a >= len(qs) for a, b in zip(i0, i1)), (i0, i1)
        _same(sh.merged(qs, K, mask=bits), ref, "keep 50 %, int8, pointer")


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_batched_route(hip_lib, oracle_mod, corpus, metric):
    """Case 4: 64 queries with TSH_OPT_BATCH_MIN_NQ = 2: the batched path's listed mode (3 %) and dense mode (50 %)
    read the handle's list and words."""
    rows, qs = corpus["rows"], corpus["qs"][metric]
    with Shards(rows, metric) as sh:
        sh.each(lambda s: s.set_batch_min_nq(2))
        for name in ("few", "half"):
            bits = _bits(corpus[name])
            hs = sh.handles(bits)
            b0 = [s.counters()["batch_launches"] for s in sh.idx]
            by_handle = sh.merged(qs, K, handles=hs)
            b1 = [s.counters()["batch_launches"] for s in sh.idx]
            assert all(b > a for a, b in zip(b0, b1)), (name, b0, b1)
            _same(by_handle, sh.merged(qs, K, mask=bits), name + ": handle against pointer")
            _same(by_handle, _oracle(oracle_mod, rows, qs, metric, K, bits), name + ": against the oracle")


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_shard_edges(hip_lib, oracle_mod, corpus, metric):
    """Case 5."""
    rows, qs, half = corpus["rows"], corpus["qs"][metric][:3], corpus["half"]
    with Shards(rows, metric) as sh:
        # bits on the two rows just outside a shard's range only: that shard's blocks are empty, its neighbours answer
        for g, (lo, hi) in enumerate(BOUNDS):
            keep = np.zeros(N, bool)
            keep[[i for i in (lo - 1, hi) if 0 <= i < N]] = True
            hs = sh.handles(_bits(keep))
            host, bb, _ = sh.blocks(qs, K, handles=hs)
            assert all(_decode(host[g, i * bb:(i + 1) * bb].tobytes())[0] == 0 for i in range(len(qs))), g
            _both_forms(sh, oracle_mod, rows, qs, K, _bits(keep), "outside shard %d" % g)
        # a bitmap whose n_bytes ends inside the second shard: its tail and the whole third shard are not kept
        short = _bits(half, 6000 // 8)
        full = _extended(short, N)
        hs = sh.handles(short)
        host, bb, _ = sh.blocks(qs, K, handles=hs)
        assert all(_decode(host[2, i * bb:(i + 1) * bb].tobytes())[0] == 0 for i in range(len(qs)))
        got = _both_forms(sh, oracle_mod, rows, qs, K, full, "bitmap ends inside shard 1", handle_bits=short)
        assert got[0].max() < 6000
        # nothing kept in one shard
        keep = half.copy()
        keep[BOUNDS[1][0]:BOUNDS[1][1]] = False
        got = _both_forms(sh, oracle_mod, rows, qs, K, _bits(keep), "shard 1 keeps nothing")
        assert not ((got[0] >= BOUNDS[1][0]) & (got[0] < BOUNDS[1][1])).any()
        # everything kept: the unmasked call
        ones = _bits(np.ones(N, bool))
        got = _both_forms(sh, oracle_mod, rows, qs, K, ones, "keeps everything")
        _same(got, sh.merged(qs, K, mask=None), "keeps everything: against the unmasked call")


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_appends_tombstones_and_quarantined_rows(hip_lib, oracle_mod, corpus, metric):
    """Cases 6, 7 and 8: rows appended after the handle was made are not returned through it; a row tombstoned after it
    was made is gone; a row kept out of the scan (a NaN element) is in the block exactly when the mask keeps it."""
    rng = np.random.default_rng(77 + metric)
    rows, qs = corpus["rows"].copy(), corpus["qs"][metric][:3]
    bad = 5000  # (shard 1)
    rows[bad, 3] = np.nan
    keep = corpus["few"].copy()
    keep[bad] = True
    bits = _bits(keep)
    with Shards(rows, metric) as sh:
        assert [s.counters()["quarantined_rows"] for s in sh.idx] == [0, 1, 0]
        hs = sh.handles(bits)
        k_all = 512  # (more than the mask keeps: the NaN row is the list's last entry)
        assert int(keep.sum()) < k_all
        ref = _oracle(oracle_mod, rows, qs, metric, k_all, bits)
        got = sh.merged(qs, k_all, handles=hs)
        _same(got, ref, "quarantined row kept")
        _same(got, sh.merged(qs, k_all, mask=bits), "quarantined row kept: handle against pointer")
        assert all(bad in got[0][i, :got[2][i]] for i in range(len(qs)))
        keep_out = keep.copy()
        keep_out[bad] = False
        hs_out = sh.handles(_bits(keep_out))
        got = sh.merged(qs, k_all, handles=hs_out)
        _same(got, _oracle(oracle_mod, rows, qs, metric, k_all, _bits(keep_out)), "quarantined row not kept")
        assert not (got[0] == bad).any()
        # appended rows: near copies of the queries, which an unmasked search returns first
        extra = np.repeat(qs, 20, axis=0) + 1e-3 * rng.standard_normal((60, D)).astype(np.float32)
        sh.idx[2].append(N, extra)
        grown = np.concatenate([rows, extra])
        unmasked = sh.merged(qs, K, mask=None)
        assert (unmasked[0] >= N).any()
        wide = _extended(bits, N + 60)
        got = sh.merged(qs, K, handles=hs)
        assert got[0].max() < N
        _same(got, sh.merged(qs, K, mask=wide), "after an append: handle against the zero-extended pointer mask")
        _same(got, _oracle(oracle_mod, grown, qs, metric, K, wide), "after an append: against the oracle")
        # a tombstone: the first query's nearest kept row
        victim = int(got[0][0, 0])
        for s, (lo, hi) in zip(sh.idx, [BOUNDS[0], BOUNDS[1], (BOUNDS[2][0], N + 60)]):
            if lo <= victim < hi:
                s.set_deleted([victim])
        alive = np.unpackbits(wide, bitorder="little")[:N + 60].astype(bool)
        alive[victim] = False
        got = sh.merged(qs, K, handles=hs)
        assert not (got[0] == victim).any()
        _same(got, sh.merged(qs, K, mask=wide), "after a tombstone: handle against pointer")
        _same(got, _oracle(oracle_mod, grown, qs, metric, K, _bits(alive)), "after a tombstone: against the oracle")


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_cursor_behind_a_handle(hip_lib, oracle_mod, corpus, metric):
    """Case 9: a page walk with k = 7 to exhaustion behind the 50 % mask concatenates to the oracle's masked list; a
    cursor of -inf equals the cursor-less handle call byte for byte after the merge."""
    rows, q, bits = corpus["rows"], corpus["qs"][metric][0], _bits(corpus["half"])
    k = 7
    e_ids, e_dist = oracle_mod.search_exhaustive(rows, q, metric, N, None, bits)
    with Shards(rows, metric) as sh:
        hs = sh.handles(bits)
        plain = sh.merged(q, k, handles=hs)
        start = sh.merged(q, k, handles=hs, after=START)
        _same(start, plain, "-inf cursor against no cursor")
        assert start[0].tobytes() == plain[0].tobytes() and start[1].tobytes() == plain[1].tobytes()
        _same(start, sh.merged(q, k, mask=bits, after=START), "-inf cursor: handle against pointer")
        ids_all, dist_all, cur, pages = [], [], START, 0
        while True:
            ids, dist, cnt = sh.merged(q, k, handles=hs, after=cur)
            c = int(cnt[0])
            pages += 1
            assert pages <= len(e_ids) // k + 2, "the walk does not end"
            ids_all.append(ids[0, :c].copy())
            dist_all.append(dist[0, :c].copy())
            if c < k:
                break
            cur = (float(dist[0, c - 1]), int(ids[0, c - 1]))
        ids_all, dist_all = np.concatenate(ids_all), np.concatenate(dist_all)
        assert np.array_equal(ids_all, e_ids) and np.array_equal(dist_all.view(np.uint64), e_dist.view(np.uint64))
        assert pages == len(e_ids) // k + 1
        # one page deep in the list, both forms
        at = 3000
        cur = (float(e_dist[at]), int(e_ids[at]))
        _same(sh.merged(q, k, handles=hs, after=cur), sh.merged(q, k, mask=bits, after=cur), "page behind row 3000")


@pytest.mark.parametrize("metric", [L2, IP, COS])
def test_ties_overflow_the_blocks(hip_lib, oracle_mod, corpus, metric):
    """Case 10: 300 copies of one row inside one shard, kept by the mask, blocks of 128 entries: the merge answers
    TSH_E_OVERFLOW with the entry count to retry with, and the retry with that count succeeds.  (On the f32 tile scan,
    whose keys cannot tell the copies apart; the exact path orders ties by id itself and never overflows.)"""
    from tostore_amd import _ffi
    from tostore_amd.sharded import merge_candidate_blocks

    rows = corpus["rows"].copy()
    rows[5000:5300] = rows[17]
    q = oracle_mod.normalize_f32(rows[17]) if metric == COS else rows[17].copy()
    keep = corpus["half"].copy()
    keep[5000:5300] = True
    keep[17] = True
    bits = _bits(keep)
    with Shards(rows, metric) as sh:
        sh.each(lambda s: s.set_exact_scan_rows(0))
        hs = sh.handles(bits)
        host, bb, entries = sh.blocks(q, K, handles=hs, entries=128)
        count, ent, got = _decode(host[1, :bb].tobytes())
        assert ent == 128 and count >= 300 and len(got) == 128
        with pytest.raises(_ffi.TshError) as e:
            merge_candidate_blocks(metric, D, q, K, None, host, 3, 128)
        assert e.value.code == _ffi.TSH_E_OVERFLOW and e.value.needed_entries >= 300
        need = int(e.value.needed_entries)
        by_handle = sh.merged(q, K, handles=hs, entries=need)
        _same(by_handle, sh.merged(q, K, mask=bits, entries=need), "retry: handle against pointer")
        _same(by_handle, _oracle(oracle_mod, rows, q, metric, K, bits), "retry: against the oracle")
        assert by_handle[0][0].tolist() == [17] + list(range(5000, 5000 + K - 1))


def test_progressive_form(hip_lib, oracle_mod, corpus):
    """Case 11: tsh_search_shard_begin_masked, 20 queries, step 5, _progress at 5 / 10 / 20, _end, then the handle is
    destroyed: the blocks of tsh_search_shard_masked behind the same handle (case 3's f32 route)."""
    import torch

    from tostore_amd import _ffi
    from tostore_amd.sharded import merge_candidate_blocks

    L = _ffi.lib()
    metric = L2
    rows, qs, bits = corpus["rows"], np.ascontiguousarray(corpus["qs"][metric][:20]), _bits(corpus["half"])
    nq = len(qs)
    ref = _oracle(oracle_mod, rows, qs, metric, K, bits)
    with Shards(rows, metric) as sh:
        sh.each(lambda s: (s.set_exact_scan_rows(0), s.set_batch_min_nq(0)))
        hs = sh.handles(bits)
        want, bb, entries = sh.blocks(qs, K, handles=hs)
        got = np.empty_like(want)
        for g, s in enumerate(sh.idx):
            buf = torch.full((nq * bb,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            st = ctypes.c_void_p()
            _ffi.check(L.tsh_search_shard_begin_masked(s._h, qs.ctypes.data_as(_ffi.p_f32), nq, K, hs[g].handle(), None, None,
                                                       entries, ctypes.c_void_p(buf.data_ptr()), 5, ctypes.byref(st)))
            try:
                for upto in (5, 10, 20):
                    done = ctypes.c_int32(0)
                    _ffi.check(L.tsh_search_shard_progress(st, upto, ctypes.byref(done)))
                    assert done.value >= upto
                    part = buf.cpu().numpy()  # (host-synchronised: the leading blocks are final)
                    for i in range(upto):
                        assert _canonical(part[i * bb:(i + 1) * bb].tobytes()) == _canonical(want[g, i * bb:(i + 1) * bb].tobytes()), (g, i)
            finally:
                rc = L.tsh_search_shard_end(st)
            _ffi.check(rc)
            hs[g].close()  # tsh_mask_destroy, after _end
            got[g] = buf.cpu().numpy()
        _same(merge_candidate_blocks(metric, D, qs, K, None, got, 3, entries), ref, "progressive form against the oracle")


def test_errors_and_no_filter(hip_lib, oracle_mod, corpus):
    """Case 12."""
    import torch

    from tostore_amd import HipVectorIndex, _ffi

    L = _ffi.lib()
    metric = L2
    rows, qs, bits = corpus["rows"], np.ascontiguousarray(corpus["qs"][metric][:3]), _bits(corpus["half"])
    with Shards(rows, metric) as sh:
        # mask = NULL: the unmasked pointer call
        _same(sh.merged(qs, K, handles=[None, None, None]), sh.merged(qs, K, mask=None), "NULL handle against no mask")
        entries = L.tsh_default_block_entries(K)
        bb = L.tsh_candidate_block_bytes(entries)
        buf = torch.zeros(len(qs) * bb, dtype=torch.uint8, device="cuda")
        qp, bp = qs.ctypes.data_as(_ffi.p_f32), ctypes.c_void_p(buf.data_ptr())
        # a handle of another shard handle
        other = sh.idx[1].make_mask(bits)
        assert L.tsh_search_shard_masked(sh.idx[0]._h, qp, len(qs), K, other.handle(), None, None, entries, bp, None) == _ffi.TSH_E_BAD_ARG
        assert "another index" in _ffi.last_error()
        st = ctypes.c_void_p(1)
        assert L.tsh_search_shard_begin_masked(sh.idx[0]._h, qp, len(qs), K, other.handle(), None, None, entries, bp, 0,
                                               ctypes.byref(st)) == _ffi.TSH_E_BAD_ARG
        assert not st.value
        # the Python searcher raises what the library says, and ValueError for a closed handle
        from tostore_amd.sharded import ShardedSearcher

        searcher = ShardedSearcher(sh.idx[0])
        mine = sh.idx[0].make_mask(bits)  # (no process group: the searcher merges this shard's blocks alone)
        local = _extended(_bits(corpus["half"][:BOUNDS[0][1]]), N)
        ref = _oracle(oracle_mod, rows, qs, metric, K, local)
        _same(searcher.search(qs, K, row_mask=mine), ref, "ShardedSearcher.search with a HipMask")
        _same(searcher.search_many(qs, K, row_mask=mine, group=2), ref, "ShardedSearcher.search_many with a HipMask")
        with pytest.raises(_ffi.TshError) as e:
            searcher.search(qs, K, row_mask=other)
        assert e.value.code == _ffi.TSH_E_BAD_ARG
        other.close()
        with pytest.raises(ValueError):
            searcher.search(qs, K, row_mask=other)
        with pytest.raises(ValueError):
            searcher.search_many(qs, K, row_mask=other)
        # a handle orphaned by tsh_index_destroy (the raw ABI: HipVectorIndex.close would close its masks first)
        lone = HipVectorIndex(D, metric, shard_device=0, row_base=24)
        lone.append(24, rows[:100])
        mh = ctypes.c_void_p()
        _ffi.check(L.tsh_mask_create(lone._h, bits.ctypes.data_as(_ffi.p_u8), len(bits), ctypes.byref(mh)))
        lone.close()
        assert L.tsh_search_shard_masked(sh.idx[0]._h, qp, len(qs), K, mh, None, None, entries, bp, None) == _ffi.TSH_E_BAD_ARG
        _ffi.check(L.tsh_mask_destroy(mh))
