"""The K2 select and the host's wide-band pass, restated in NumPy over integer keys: "keys in, header and candidate set
out".  No GPU and nothing of the library under test: tests/test_host_select_inputs.py runs it on f64 keys rounded to f32,
tests/test_gpu_select.py on the keys the scan kernel itself produced (probe_scan_keys) and holds the block
tsh_search_shard leaves to it.

What is restated, each from the kernel text (tostore_amd/csrc/tsh_kernels.hip.h, run_fallback in tsh_lib.hip):
  f2key / key2f      the order-preserving map float <-> uint32; KEY_NAN, KEY_DEAD
  band_of            tau + |tau| eps_rel + delta_abs in f64, rounded UP to the next float (+-0 -> the smallest positive,
                     negative -> towards zero); KEY_NAN from KEY_NAN, from +inf and from a band that is not finite
  tile minima        of 64 keys, KEY_DEAD for a tile without a live row
  select_tau         narrow or not; U = the k-th smallest of the group minima from the thread layout (thread tid owns tiles
                     tid + i NT; four neighbouring threads a group up to k = 128 with sixteen waves; a thread's even and
                     odd tiles two groups above k = 512); the short list of minima <= U; tau = its k-th smallest, or U
                     when more than SEL_LIST_CAP entries flooded it; KEY_DEAD -> KEY_NAN
  the list shortcut  a list scan of fewer tiles than k: tau = the k-th smallest key of the M x 64 list positions
  steps (d)-(f)      hit tiles, over, the first emit, the refinement's bisect bit by bit from the common prefix of the
                     smallest hit key and tau (diff == 0 and top == 31 included), the second emit
  the fp16 store     a row passes when stored <= band and stored - 2 w (1 + 2^-20) <= tau in f64
  run_fallback       the four radix rounds over the live keys (its "fewer than k live keys" exit), h_band_of, the filter

Every branch CONDITION comes from tostore_amd/csrc/tsh_select_plan.h, the header the kernel is compiled from, through a
shared object g++ builds from tests/cpp/select_plan_lib.cpp: plan().  Nothing of it is retyped here.

Fields of the header and whether they are specified (Model.spec: the tests assert exactly those):
  count       always: the kernel's second (or only) emit; 0 when over; after the wide-band pass, what its filter counted
  tau_key, band_key, tiles_hit   always the KERNEL's: run_fallback rewrites count and flags only, so after a host radix
              select band_key is NOT the band the filter used (Model.filter_band is)
  flags & 3   FLAG_LIST_OVERFLOW | FLAG_TAU_REFINED as the kernel left them, or, after the wide-band pass, overflow alone
              (run_fallback assigns flags: the refined bit is lost there, and the model says so)
  k, row_base, shard_rows, entries   always
  (the fp16 store: band_key is READ from the header, see band_known; an overflowed fp16 block is never seen -- the
              query is redone through the f32 scan and the block is that select's)
  ids         the candidate set, when count <= entries (an overflowed block holds `entries` of them, which ones is the
              order of the kernels' atomics: unspecified)
Left unasserted: metric and pad[] (constants of the call, held by tests/test_gpu_shard_stream.py), and the ORDER of the
entries (atomics).
"""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_DEAD = 0xFFFFFFFF
KEY_NAN = 0xFFFFFFFE
FLAG_LIST_OVERFLOW, FLAG_TAU_REFINED = 1, 2
VARIANTS = ("NT256-regs", "NT1024-regs", "NT1024-mem")
_PLAN = None


class Plan:
    """tsh_select_plan.h behind ctypes."""

    def __init__(self, so):
        self.lib = lib = ctypes.CDLL(so)
        c = (ctypes.c_int * 4)()
        lib.sp_constants(c)
        self.THREADS, self.VPT, self.LIST_CAP, self.PREFILTER_MIN = (int(x) for x in c)
        i, u = ctypes.c_int, ctypes.c_uint
        for name, args in (("sp_variant", (i, i, i)), ("sp_variant_threads", (i,)), ("sp_variant_in_regs", (i,)),
                           ("sp_narrow", (i, i, u, i)), ("sp_prefilter", (i, i)), ("sp_groups4", (i, u)), ("sp_groups2k", (u,)),
                           ("sp_short_small", (u,)), ("sp_flooded", (u,)), ("sp_over", (u,)), ("sp_refines", (u, i)),
                           ("sp_refine_in_regs", (i, u)), ("sp_list_shortcut", (i, u)), ("sp_default_entries", (i,))):
            f = getattr(lib, name)
            f.restype, f.argtypes = ctypes.c_int, list(args)
            setattr(self, name[3:], f)


def plan():
    """The header's functions, compiled once per process."""
    global _PLAN
    if _PLAN is None:
        d = tempfile.mkdtemp(prefix="select_plan_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libselect_plan.so")
        src = os.path.join(ROOT, "tests", "cpp", "select_plan_lib.cpp")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src], check=True)
        _PLAN = Plan(so)
    return _PLAN


# ---- keys ----------------------------------------------------------------------------------------------------------------
def f2key(f):
    """float32 array -> uint32 keys (NaN -> KEY_NAN)"""
    f = np.ascontiguousarray(f, np.float32)
    b = f.view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(f), np.uint32(KEY_NAN), k).astype(np.uint32)


def key2f(k):
    k = np.asarray(k, np.uint32)
    b = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return b.view(np.float32)


def band_of(tau_key, eps_rel, delta_abs, round_up=True):
    """tau widened by the f32 error band, rounded UP to the next float (round_up=False: what a band_of without its round-up
    would give -- the host test shows that the table tells the two apart)."""
    if tau_key >= KEY_NAN:
        return KEY_NAN
    t = np.float32(key2f(np.uint32(tau_key)).reshape(-1)[0])
    if t == np.inf:
        return KEY_NAN
    with np.errstate(over="ignore"):
        w = np.float64(t) + abs(np.float64(t)) * np.float64(np.float32(eps_rel)) + np.float64(np.float32(delta_abs))
        f = np.float32(w)
    if round_up and np.float64(f) < w:
        b = int(np.float32(f).view(np.uint32))
        if b & 0x7FFFFFFF == 0:
            b = 1
        elif b & 0x80000000:
            b -= 1
        else:
            b += 1
        f = np.uint32(b).view(np.float32)
    if not f < np.inf:
        return KEY_NAN
    return int(f2key(np.float32(f)).reshape(-1)[0])


def kth_smallest(v, k):
    """wave_kth_bisect / block_kth_radix: the smallest X with count(v <= X) >= k -- the k-th smallest of v, which holds k
    values or more wherever the kernel calls them."""
    assert 1 <= k <= len(v), (k, len(v))
    return int(np.partition(np.asarray(v, np.uint32), k - 1)[k - 1])


class Model:
    """What the select predicts.  header: dict of the specified fields; ids: the candidate set (local ids, sorted) or None
    where it is not specified; path: the path record; spec: the names of the header fields a test asserts."""


def _bisect_refine(hit_keys_sorted, lo, tau, k):
    """Step (f): from the common prefix of lo and tau, one bit at a time.  -> (X, diff0, top31)"""
    diff = lo ^ tau
    if diff == 0:
        return lo, True, False
    top = diff.bit_length() - 1
    X = 0 if top == 31 else (lo >> (top + 1)) << (top + 1)
    for bit in range(top, -1, -1):
        T = X | ((1 << bit) - 1)
        c = int(np.searchsorted(hit_keys_sorted, T, side="right"))
        if c < k:
            X |= 1 << bit
    return X, False, top == 31


def select_model(keys, k, cand_cap, eps_rel, delta_abs, live=None, list_order=None, w=None, row_base=0, shard_rows=None,
                 band_round_up=True, band_known=None):
    """keys: f32 key per row, NaN = a dead row; live: optionally which rows are alive (the rest count as NaN whatever
    their key -- the keys of a dead TILE are stale on the device).  list_order: the row ids of a list scan in list order
    (padding: -1).  w: per-row band of the fp16 store (keys are then the stored upper sides).
    band_known: {tau_key: band_key} read from a block's header -- the fp16 store's delta_abs (2 w_max 1.0001, from the
    shard's norm bound) is not probed, so the band of the tau that is written out is taken from there and delta_abs
    serves only the tau that is not."""
    P = plan()
    band_known = band_known or {}

    def band_for(t):
        return band_known[t] if t in band_known else band_of(t, eps_rel, delta_abs, band_round_up)

    keys = np.ascontiguousarray(keys, np.float32)
    n_rows = len(keys)
    shard_rows = n_rows if shard_rows is None else shard_rows
    uk = f2key(keys)
    dead = np.isnan(keys) if live is None else ~np.asarray(live, bool)
    uk[dead] = KEY_DEAD
    has_list = list_order is not None
    if has_list:
        lo_ids = np.asarray(list_order, np.int64)
        pos_keys = np.where(lo_ids >= 0, uk[np.clip(lo_ids, 0, n_rows - 1)], np.uint32(KEY_DEAD)).astype(np.uint32)
        ids_of = lo_ids
    else:
        pos_keys = uk
        ids_of = np.arange(n_rows, dtype=np.int64)
    M = (len(pos_keys) + 63) // 64
    pk = np.full(M * 64, KEY_DEAD, np.uint32)
    pk[:len(pos_keys)] = pos_keys
    wk = None
    if w is not None:
        assert not has_list
        wk = np.zeros(M * 64, np.float64)
        wk[:n_rows] = np.asarray(w, np.float64)
    gmin = pk.reshape(M, 64).min(axis=1)

    path = {}
    variant = P.variant(M, k, int(has_list))
    NT = P.variant_threads(variant)
    path["variant"] = VARIANTS[variant]
    path["list"] = has_list
    path["f16"] = wk is not None
    assert P.variant_in_regs(variant) or M > P.VPT * P.THREADS
    assert not P.variant_in_regs(variant) or M <= P.VPT * NT  # the thread's share fits its registers

    # ---- select_tau
    narrow = bool(P.narrow(NT, M, k, 0))
    path["narrow"] = narrow
    tau, U, n = KEY_NAN, KEY_DEAD, 0
    path["prefilter"] = "none"
    path["short"] = "none"
    path["flooded"] = False
    if narrow:
        if P.prefilter(1, M):
            nvals = -(-M // NT)
            g = np.full(nvals * NT, KEY_DEAD, np.uint32)
            g[:M] = gmin
            g = g.reshape(nvals, NT)  # g[i, tid] = the minimum of tile tid + i NT
            if P.groups2k(k):
                path["prefilter"] = "groups2k"
                even = g[0::2].min(axis=0)
                odd = g[1::2].min(axis=0) if nvals > 1 else np.full(NT, KEY_DEAD, np.uint32)
                groups = np.concatenate([even, odd])
            elif P.groups4(NT, k):
                path["prefilter"] = "groups4"
                groups = g.min(axis=0).reshape(NT // 4, 4).min(axis=1)
            else:
                path["prefilter"] = "plain"
                groups = g.min(axis=0)
            U = kth_smallest(groups, k)
        short = gmin[gmin <= np.uint32(U)]
        n = len(short)
        if P.flooded(n):
            path["flooded"] = True
            tau = U
        else:
            path["short"] = "small" if P.short_small(n) else "large"
            tau = kth_smallest(short, k)
        if tau == KEY_DEAD:
            tau = KEY_NAN
    path["tau_nan"] = narrow and tau == KEY_NAN  # fewer than k live tiles
    # ---- the list shortcut
    path["list_radix"] = False
    if has_list and P.list_shortcut(M, k):
        path["list_radix"] = True
        x = kth_smallest(pk, k)
        tau = KEY_NAN if x >= KEY_DEAD else x
        path["tau_nan"] = tau == KEY_NAN  # fewer than k live rows in the list
    band = band_for(tau)

    # ---- (d) hit tiles, (e) emit
    hit = gmin <= np.uint32(band)
    nt = int(hit.sum())
    over = bool(P.over(nt))
    path["over"] = over
    hit_rows = np.repeat(hit, 64)

    def emit(bnd, tk):
        ok = hit_rows & (pk <= np.uint32(bnd))
        if wk is not None and bnd < KEY_NAN and tk < KEY_NAN:
            lower = key2f(pk).astype(np.float64) - 2.0 * (wk * (1.0 + 9.5367431640625e-07))
            ok &= lower <= np.float64(key2f(np.uint32(tk)).reshape(-1)[0])
        return ok

    tau_out, band_out = tau, band
    cand = np.zeros(M * 64, bool)
    path["refined"] = "none"
    path["diff0"] = path["top31"] = False
    if not over:
        cand = emit(band, tau)
        first = int(cand.sum())
        if P.refines(first, cand_cap):
            path["refined"] = "regs" if P.refine_in_regs(NT, nt) else "mem"
            hk = np.sort(pk[hit_rows])
            X, path["diff0"], path["top31"] = _bisect_refine(hk, int(hk[0]), tau, k)
            tau_out, band_out = X, band_for(X)
            cand = emit(band_out, X)
    count = 0 if over else int(cand.sum())
    flags = FLAG_LIST_OVERFLOW if (over or count > cand_cap) else 0
    if tau_out != tau:
        flags |= FLAG_TAU_REFINED

    # ---- run_fallback
    m = Model()
    m.kernel_count, m.kernel_flags = count, flags
    m.filter_band = None
    path["host_radix"] = "none"
    # (an overflowed fp16 scan is not widened over its stored keys: the query is redone through the f32 scan, whose
    # block is a model run of its own over the f32 keys)
    path["redone"] = wk is not None and bool(flags & FLAG_LIST_OVERFLOW)
    path["fallback"] = bool(flags & FLAG_LIST_OVERFLOW) and wk is None
    if path["fallback"]:
        n_keys = M * 64 if not has_list else len(pos_keys)
        live_tile = np.repeat(gmin != np.uint32(KEY_DEAD), 64)
        in_range = np.arange(M * 64) < n_keys
        fb = band_out
        if fb >= KEY_NAN and k < n_keys:
            lk = pk[live_tile & in_range & (pk != np.uint32(KEY_DEAD))]
            prefix, remaining, found, rounds_deciding = 0, k, True, []
            for shift in (24, 16, 8, 0):
                sel = lk if shift == 24 else lk[(lk >> np.uint32(shift + 8)) == np.uint32(prefix >> (shift + 8))]
                hist = np.bincount(((sel >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256)
                cum, b = 0, 0
                while b < 256 and cum + int(hist[b]) < remaining:
                    cum += int(hist[b])
                    b += 1
                if b == 256:
                    found = False
                    break
                rounds_deciding.append(int(np.count_nonzero(hist)))
                remaining -= cum
                prefix |= b << shift
            path["host_radix"] = "found" if found else "not_found"
            m.radix_bins = rounds_deciding  # occupied bins per round (1: the round decided nothing)
            if found:
                fb = band_of(prefix, eps_rel, delta_abs, band_round_up)
                m.radix_kth = prefix
        cand = live_tile & in_range & (pk <= np.uint32(fb))
        count = int(cand.sum())
        flags = FLAG_LIST_OVERFLOW if count > cand_cap else 0
        m.filter_band = fb
    path["overflow"] = bool(flags & FLAG_LIST_OVERFLOW)

    m.header = dict(count=count, entries=cand_cap, tau_key=tau_out, band_key=band_out, tiles_hit=nt, flags=flags & 3, k=k,
                    row_base=row_base, shard_rows=shard_rows)
    m.spec = ("count", "entries", "tau_key", "band_key", "tiles_hit", "flags", "k", "row_base", "shard_rows")
    ids = np.sort(ids_of[:len(pos_keys)][cand[:len(pos_keys)]])
    assert np.all(ids >= 0)
    m.all_ids = ids  # every candidate, whether the block holds them or not
    m.ids = ids if count <= cand_cap else None
    m.path = path
    m.tau0, m.U, m.short_n, m.n_tiles = tau, U, n, M
    m.fallbacks = 1 if path["fallback"] else 0
    m.candidates = count  # what the search adds to candidates_total
    return m


def path_name(path):
    """One word per path, the enumerated list of tests/select_inputs.py is made of these."""
    p = [path["variant"]]
    if path["list_radix"]:
        p.append("list-radix")
    elif not path["narrow"]:
        p.append("all-tiles")
    elif path["flooded"]:
        p.append(path["prefilter"] + "/flooded")
    else:
        p.append(path["prefilter"] + "/short-" + path["short"])
    if path["tau_nan"]:
        p.append("tau-nan")
    if path["over"]:
        p.append("over")
    if path["refined"] != "none":
        p.append("refined-" + path["refined"] + ("-diff0" if path["diff0"] else "") + ("-top31" if path["top31"] else ""))
    if path["host_radix"] != "none":
        p.append("radix-" + path["host_radix"])
    elif path["fallback"]:
        p.append("filter")
    if path["overflow"]:
        p.append("overflow")
    if path["list"] and not path["list_radix"]:
        p[1] = "list:" + p[1]
    if path["f16"]:
        p[1] = "f16:" + p[1]
        if path["redone"]:
            p.append("redone")
    return " ".join(p)
