"""GPU: the K2 select (select_kernel: select_tau, select_body and its step (f)) and the host's wide-band pass
(run_fallback: radix_hist_kernel, filter_kernel) held to a model of their keys, branch by branch.

Per case of tests/select_inputs.py -- a shard-mode index of d = 8 with a row base that is not 0, the f32 tile scan forced
(no batched path, no exact path, no fp16 or int8 copy):
  (a) probe_scan_keys gives every row's f32 key and the scan's band; tests/select_model.py turns them into the predicted
      header, candidate set and path; the path is the case's intended one, and the band at every threshold the model
      names is below a quarter of the planted gap (a case outside that is "inputs outside their design": a failure).
  (b) tsh_search_shard with the case's `entries`; the device block's count, entries, tau_key, band_key, tiles_hit,
      flags & 3, k, row_base and shard_rows equal the model's; the ids equal the model's set (global ids) when it fits,
      and are distinct members of it when the block overflowed; every entry's s0 / s1 are the oracle's f64 sums of that
      row, bit for bit.
  (c) merge_candidate_blocks equals oracle.search_exhaustive; where count > entries the merge raises TSH_E_OVERFLOW and
      the call is repeated ONCE with entries = count, as the block's protocol prescribes.
  (d) fallback_searches and candidates_total move as the path predicts; no exact scan, a list scan in group G only.
The last test holds the union of the paths the kernels' own keys took to the list the host test holds the table to.

Flooded implies over: a flooded short list holds more than SEL_LIST_CAP tile minima <= U, tau = U, the band is at or
above tau, so more than SEL_LIST_CAP tiles are hit (case D-t4200).  Group E's cluster fills six tiles, not three: 192
rows would not overflow tsh_default_block_entries(64) = 256 and step (f) would not run.

List scans (group G) run behind both forms of a mask, pointer and handle.  No probe returns list-order keys and
scan_list_kernel's sums are not known to equal the tile scan's bit for bit, so there tau_key is held to the probed band
round the model's value and band_key to band_of(the tau_key in the block); everything else, the candidate set included,
is exact -- the planted gap makes that sound.  Every row outside the WHERE set is NEARER than every row inside it.

The fp16 store (group H: set_scan_f16(2), d = 256, 40 tiles).  Keys and the rows' bands w come from probe_scan_f16_keys,
whose w is scan_f16_w of the inputs the select reads (see _run_case); tau_key is the model's, band_key is read from the
header (held to the band of that tau under twice the largest w) and the candidate set must be exactly {live rows:
stored <= band and stored - 2 w (1 + 2^-20) <= tau}.  The plain and the refined case plant rows that only the per-row
rule sends away; the overflowing case is redone through the f32 scan (scan_f16_stats: redone + 1) and its block is
held to the model of the f32 keys.  The 2^-8 gap is not asked of group H: the fp16 band is per cent of a key.

Measured on one MI355X, the whole module: 55 tests in 5.8 s.  Wall seconds per group, rows made, index filled, probed,
searched and checked: A 0.97 (eight cases, two of them 1.05 M rows), B 0.44, C 0.46, D 0.39, E 0.39, F 0.11, G 0.97 (eight
cases, both mask forms), H 0.16 (H-f16-plain: 37 rows at or below the band, 27 candidates; H-f16-refined: 25 and 10).  Counters per case: searches + 1, fallback_searches + 1 exactly where the model's path ends in
the wide-band pass (C-t4097-k1025, C-ulps, C-tied-kth, C-ip-signed, C-not-found, D-t4200, D-t4096, D-flood-loose,
D-k512-parity-pair, E-five-copies), candidates_total + the model's count, list_scans + 1 in group G only.

Mutation record.  Each line is one comparison of the device or host code changed on a scratch copy (values only: no
index, loop bound or capacity), the library rebuilt, and this module run against it; the cases named are the ones that
failed.  Nothing of it is committed.
  wave_kth_bisect: c < k -> c <= k              every narrow case whose tau is a bisect's: A-*, B-t1100-*, B-t1024-k1024,
                                                D-k129-thread-pair, E-nt256-*, E-nt1024-*, E-ip-*, G-21-tiles-k10 (23 tests)
  groups2k at k > 511                           D-k512-parity-pair
  groups4 at k <= 129                           D-k129-thread-pair
  M > SEL_PREFILTER_MIN -> >=                   NONE, and none can: at 512 tiles the prefilter's U only shortens a short list
                                                that 512 minima cannot flood, tau is the exact k-th minimum either way and
                                                nothing of U reaches the block.  The edge is held where it is decided, on
                                                the CPU (tests/cpp/select_plan_test.cpp: sel_prefilter at 512 / 513)
  step (f)'s in-registers test negated          B-t1023-k1024, C-t1100-k1025 (from registers the bisect then counts the
                                                first 256 hit tiles only; the memory path serves any count, so the
                                                other direction changes nothing)
  s_cnt[slot] < k -> <=                         every refined case with diff != 0: B-t1023-k1024, C-t1100-k1025, E-nt256-*,
                                                E-nt1024-*, E-ip-*, F-40-live-tiles
  run_fallback: cum + hist[b] >= remaining -> > C-t4097-k1025, C-ip-signed
  band_of without its round-up                  the cases whose f64 band rounds down to the nearest float: A-t512-k256,
                                                B-t1100-k128 / k512 / k513 / k1024, B-t1024-k1024, B-t1023-k1024, D-t4200,
                                                E-nt256-k65, E-nt1024-k256, E-ip-k64, E-ip-k257, G-full-tiles-k1344
  list shortcut: M * 64 >= k -> >               G-full-tiles-k1344 (both mask forms)
  flooded: tau from the bisect, not s.U         D-flood-loose, D-k512-parity-pair
(The record was taken before group H was added; the mutants were not run against it.)
"""
import ctypes
import time

import numpy as np
import pytest

import select_inputs as si
import select_model as sm

pytestmark = pytest.mark.gpu

HEADER = np.dtype([("count", "<u4"), ("entries", "<u4"), ("tau_key", "<u4"), ("band_key", "<u4"), ("tiles_hit", "<u4"), ("flags", "<u4"),
                   ("k", "<u4"), ("metric", "<u4"), ("row_base", "<i8"), ("shard_rows", "<i8"), ("pad", "<u4", (4,))])
ENTRY = np.dtype([("id", "<i8"), ("s0", "<f8"), ("s1", "<f8")])
assert HEADER.itemsize == 64 and ENTRY.itemsize == 24


@pytest.fixture(scope="module")
def reached():
    """What the cases of this module leave for its last test: case name -> the path the kernels' own keys took, and
    group -> wall seconds.  Every case test takes it, so does the test that reads it."""
    return {"paths": {}, "seconds": {}}


def _bits(live):
    return np.packbits(np.asarray(live, bool), bitorder="little")


def _search_block(torch, idx, q, k, entries, mask=None):
    """mask: None, the GLOBAL keep bitmap (pointer form) or a HipMask (handle form)"""
    from tostore_amd import _ffi
    from tostore_amd.backend import HipMask

    L = _ffi.lib()
    buf = torch.zeros(L.tsh_candidate_block_bytes(entries), dtype=torch.uint8, device="cuda")
    qp, out = q.ctypes.data_as(_ffi.p_f32), ctypes.c_void_p(buf.data_ptr())
    if isinstance(mask, HipMask):
        _ffi.check(L.tsh_search_shard_masked(idx._h, qp, 1, k, mask.handle(), None, None, entries, out, None))
    else:
        _ffi.check(L.tsh_search_shard(idx._h, qp, 1, k, None if mask is None else mask.ctypes.data_as(_ffi.p_u8), entries, out, None))
    blk = buf.cpu().numpy()
    return blk, blk[:64].view(HEADER)[0], blk[64:].view(ENTRY)


def _run_case(c, hip_lib, oracle_mod, reached, form=None):
    import torch

    from tostore_amd import HipVectorIndex, _ffi
    from tostore_amd.backend import HipMask
    from tostore_amd.sharded import merge_candidate_blocks

    t_start = time.perf_counter()
    B = si.ROW_BASE
    keys64, live = si.plant_keys(c)
    rows, q = si.make_rows(c, keys64)
    n, k, entries = c.n, c.k, c.block_entries()
    assert entries == hip_lib.tsh_default_block_entries(k) or c.entries is not None
    with HipVectorIndex(c.dim, c.metric, shard_device=0, row_base=B) as idx:
        idx.set_batch_min_nq(0)
        idx.set_exact_scan_rows(0)
        idx.set_scan_f16(2 if c.f16 else 0)
        idx.set_scan_i8(0)
        idx.append(B, rows)
        listed = c.plant == "list"
        mask = order = None
        if listed:  # the WHERE set, made before any of its rows is tombstoned
            kept = np.zeros(B + n, bool)
            kept[B + si.kept_rows(c)] = True
            mask = _bits(kept)
            if form == "handle":
                mask = HipMask(idx, mask)
            order = si.list_order(c)
            live_kept = live & kept[B:]
        if not live.all():
            idx.set_deleted(B + np.nonzero(~live)[0])

        # ---- (a)
        keys, eps_rel, delta_abs = idx.probe_scan_keys(q)
        assert keys.shape == (n,) and not np.isnan(keys[live]).any()
        m = sm.select_model(keys, k, entries, eps_rel, delta_abs, live=live, list_order=order, row_base=B, shard_rows=n)
        want_path = c.path
        if c.f16:
            # the fp16 store: the select reads the stored upper sides and w = scan_f16_w(alpha, beta, |row|^2) per row -- what
            # probe_scan_f16_keys returns (tsh_probe_scan_f16_keys runs scan_f16_w_kernel on the shard's d_sqnorm with the
            # band's alpha and beta; fill_scan_f16_args hands the select the same three).  Its delta_abs = 2 w_max 1.0001
            # comes from the shard's norm BOUND and is not probed: estimated from the largest w for the path, and the band
            # of the tau that is written out read from the header below
            stored, w16 = idx.probe_scan_f16_keys(q)
            assert not np.isnan(stored[live]).any() and np.all(w16[live] > 0)
            delta16 = np.float32(2.0 * float(w16.max()) * 1.0001)
            m16 = sm.select_model(stored, k, entries, 0.0, delta16, live=live, w=w16, row_base=B, shard_rows=n)
            reached["paths"][c.name] = sm.path_name(m16.path)
            print("%s: %s; header %s" % (c.name, sm.path_name(m16.path), m16.header))
            assert sm.path_name(m16.path) == c.path
            want_path = c.kw.get("f32_path")  # (an overflowed fp16 scan is redone through the f32 scan: the block is m's)
            assert (want_path is not None) == m16.path["redone"]
        else:
            reached["paths"][c.name + (":" + form if form else "")] = sm.path_name(m.path)
        print("%s: %s; header %s" % (c.name, sm.path_name(m.path), m.header))
        assert want_path is None or sm.path_name(m.path) == want_path
        if c.name not in si.GAP_EXEMPT:
            for key in (m.tau0, m.header["tau_key"], getattr(m, "radix_kth", sm.KEY_NAN), m.U if m.path["prefilter"] != "none" else sm.KEY_NAN):
                if key < sm.KEY_NAN:
                    t = abs(float(sm.key2f(np.uint32(key)).reshape(-1)[0]))
                    band = eps_rel * t + delta_abs
                    print("  threshold %.6g: band %.3g, a quarter of the gap %.3g" % (t, band, t * 2.0 ** -8 / 4))
                    assert band < t * 2.0 ** -8 / 4, "inputs outside their design"

        # ---- (b)
        c0, f0 = idx.counters(), idx.scan_f16_stats()
        blk, h, ent = _search_block(torch, idx, q, k, entries, mask)
        c1, f1 = idx.counters(), idx.scan_f16_stats()
        assert f1["scans"] - f0["scans"] == (1 if c.f16 else 0)
        assert f1["redone"] - f0["redone"] == (1 if c.f16 and m16.path["redone"] else 0)
        if c.f16 and not m16.path["redone"]:
            # band_key is read from the header: it must be the band of the model's tau under a delta_abs between twice the
            # largest row band and that with the norm bound's slack; the model then takes it for that tau
            assert int(h["tau_key"]) == m16.header["tau_key"]
            assert sm.band_of(int(h["tau_key"]), 0.0, np.float32(delta16 * (1.0 - 1e-6))) <= int(h["band_key"]) \
                <= sm.band_of(int(h["tau_key"]), 0.0, np.float32(delta16 * 1.001))
            m = sm.select_model(stored, k, entries, 0.0, delta16, live=live, w=w16, row_base=B, shard_rows=n,
                                band_known={int(h["tau_key"]): int(h["band_key"])})
            assert sm.path_name(m.path) == c.path
            # the per-row rule decides: rows at or below the band are sent away by it
            band_f = float(sm.key2f(np.uint32(m.header["band_key"])).reshape(-1)[0])
            print("  rows at or below the band: %d, candidates: %d" % (int(np.sum(stored[live] <= band_f)), m.header["count"]))
            assert int(np.sum(stored[live] <= band_f)) > m.header["count"]
        got = {f: int(h[f]) for f in m.spec}
        got["flags"] &= 3
        print("  block %s" % got)
        want = {f: m.header[f] for f in m.spec}
        if listed:
            # no probe returns list-order keys and scan_list_kernel's sums are not known to be the tile scan's bit for bit:
            # tau_key within the probed band of the model's, band_key the band of the tau_key that is there
            for f in ("tau_key", "band_key"):
                assert (got[f] >= sm.KEY_NAN) == (want[f] >= sm.KEY_NAN), f
            if want["tau_key"] < sm.KEY_NAN:
                tg, tw = (float(sm.key2f(np.uint32(x)).reshape(-1)[0]) for x in (got["tau_key"], want["tau_key"]))
                assert abs(tg - tw) <= eps_rel * abs(tw) + delta_abs, (tg, tw)
                assert got["band_key"] == sm.band_of(got["tau_key"], eps_rel, delta_abs)
            got["tau_key"], got["band_key"] = want["tau_key"], want["band_key"]
        assert got == want
        held = ent[:min(int(h["count"]), entries)]
        ids = held["id"] - B
        assert len(np.unique(ids)) == len(ids)
        if m.ids is not None:
            assert np.array_equal(np.sort(ids), m.ids)
        else:
            assert len(ids) == entries and np.isin(ids, m.all_ids).all()
        for e, i in zip(held, ids):
            s0, s1 = oracle_mod.exact_sums(q, rows[i], c.metric)
            assert np.float64(e["s0"]).view(np.uint64) == np.float64(s0).view(np.uint64), (c.name, int(i))
            assert np.float64(e["s1"]).view(np.uint64) == np.float64(s1).view(np.uint64), (c.name, int(i))

        # ---- (d)
        assert c1["fallback_searches"] - c0["fallback_searches"] == m.fallbacks
        assert c1["candidates_total"] - c0["candidates_total"] == m.candidates
        assert c1["searches"] - c0["searches"] == 1
        assert c1["list_scans"] - c0["list_scans"] == (1 if listed else 0) and c1["exact_scans"] == c0["exact_scans"]

        # ---- (c)
        if int(h["count"]) > entries:
            with pytest.raises(_ffi.TshError) as e:
                merge_candidate_blocks(c.metric, c.dim, q, k, None, blk, 1, entries)
            assert e.value.code == _ffi.TSH_E_OVERFLOW and e.value.needed_entries >= int(h["count"])
            entries = int(h["count"])
            blk, h, ent = _search_block(torch, idx, q, k, entries, mask)
            assert int(h["count"]) <= entries and not int(h["flags"]) & sm.FLAG_LIST_OVERFLOW
            assert np.array_equal(np.sort(ent[:int(h["count"])]["id"] - B), m.all_ids)
        ids, dist, cnt = merge_candidate_blocks(c.metric, c.dim, q, k, None, blk, 1, entries)
        if listed:
            live = live_kept
        eids, edist = oracle_mod.search_exhaustive(rows, q, c.metric, k, None, None if live.all() else _bits(live))
        assert cnt[0] == len(eids) == min(k, int(live.sum()))
        assert np.array_equal(ids[0, :cnt[0]], eids + B)
        assert np.array_equal(dist[0, :cnt[0]].view(np.uint64), edist.view(np.uint64))
    reached["seconds"][c.group] = reached["seconds"].get(c.group, 0.0) + time.perf_counter() - t_start


def _group(g):
    return pytest.mark.parametrize("c", [c for c in si.CASES if c.group == g], ids=repr)


@_group("A")
def test_variant_edges(hip_lib, oracle_mod, reached, c):
    _run_case(c, hip_lib, oracle_mod, reached)


@_group("B")
def test_prefilter_groups(hip_lib, oracle_mod, reached, c):
    _run_case(c, hip_lib, oracle_mod, reached)


@_group("C")
def test_k_beyond_the_scheme(hip_lib, oracle_mod, reached, c):
    _run_case(c, hip_lib, oracle_mod, reached)


@_group("D")
def test_ties_across_tiles(hip_lib, oracle_mod, reached, c):
    _run_case(c, hip_lib, oracle_mod, reached)


@_group("E")
def test_refinement_limits(hip_lib, oracle_mod, reached, c):
    _run_case(c, hip_lib, oracle_mod, reached)


@_group("F")
def test_dead_tiles(hip_lib, oracle_mod, reached, c):
    _run_case(c, hip_lib, oracle_mod, reached)


@_group("G")
@pytest.mark.parametrize("form", ["pointer", "handle"])
def test_list_scans(hip_lib, oracle_mod, reached, c, form):
    _run_case(c, hip_lib, oracle_mod, reached, form)


@_group("H")
def test_f16_store(hip_lib, oracle_mod, reached, c):
    _run_case(c, hip_lib, oracle_mod, reached)


def test_every_enumerated_path_was_reached(reached):
    """The union of the paths the kernels' keys took is the list tests/test_host_select_inputs.py holds the table to.
    It reads what the case tests left in the module's `reached` fixture: it is about the module as a whole and fails
    when some of its cases were deselected."""
    print("wall seconds per group: %s" % {g: round(s, 2) for g, s in sorted(reached["seconds"].items())})
    ran = sorted({name.split(":")[0] for name in reached["paths"]})
    assert ran == sorted(c.name for c in si.CASES), "not every case of the module has run"
    assert sorted(set(reached["paths"].values())) == si.PATHS
