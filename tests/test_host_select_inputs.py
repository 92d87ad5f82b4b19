"""CPU: the case table of the select sweep (tests/select_inputs.py) against the model of the select
(tests/select_model.py), on f64 keys of the planted rows rounded to f32 -- no GPU.  Every case reaches the path it is
meant to reach; the table reaches exactly the enumerated paths; taking any one case out loses a path, or the case is
named as held by rule only; and wherever a decision of the select rests on the order of two keys, the threshold is the
only key value within 2^-8 of itself, so that the scan's own roundings (held to a quarter of that on the GPU) cannot
move a case onto another path."""
import numpy as np
import pytest

import select_inputs as si
import select_model as sm

_CACHE = {}
# the scan's band as tsh_lib.hip's compute_band forms it for one chunk of four-element groups (the GPU test takes the
# probed one): it only has to be of the right size here
EPS_L2 = np.float32(3.0 * 12.0 * 2.0 ** -23)


def _model(c, **kw):
    key = (c.name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        keys, live = si.plant_keys(c)
        rows, q = si.make_rows(c, keys)
        ek = si.exact_keys(rows, q, c.metric)
        if c.metric == si.L2:
            eps, delta = EPS_L2, np.float32(si.D * 7.9e-31)
        else:
            qn = np.linalg.norm(q.astype(np.float64))
            eps, delta = 0.0, np.float32(2.0 * 10.0 * 2.0 ** -23 * qn * np.linalg.norm(rows.astype(np.float64), axis=1).max() * 1.0001)
        seen, w = ek, None
        if c.f16:
            # the fp16 store on the CPU: a stand-in of the right form and size -- the stored key is the reduced key (|q|^2
            # left out) plus the row's band w = 2^-9 |q| |row|, the select's delta_abs twice the largest band
            r64, q64 = rows.astype(np.float64), q.astype(np.float64)
            w = (2.0 ** -9 * np.linalg.norm(q64) * np.linalg.norm(r64, axis=1)).astype(np.float32)
            seen = (ek - q64 @ q64 + w).astype(np.float32).astype(np.float64)
            eps, delta = 0.0, np.float32(2.0 * w.max() * 1.0001)
        _CACHE[key] = (sm.select_model(seen.astype(np.float32), c.k, c.block_entries(), eps, delta, live=live, w=w,
                                        list_order=si.list_order(c) if c.plant == "list" else None, **kw), ek, live, seen)
    return _CACHE[key]


@pytest.mark.parametrize("c", si.CASES, ids=repr)
def test_case_reaches_its_path(c):
    m, ek, live, _ = _model(c)
    assert sm.path_name(m.path) == c.path
    assert c.block_entries() >= c.k  # (step (f) counts on it)
    h = m.header
    assert h["k"] == c.k and h["entries"] == c.block_entries() and h["shard_rows"] == c.n
    # the candidates hold the true neighbours: the k smallest exact keys of the live rows, ties included
    if c.plant == "list":
        live = live & np.isin(np.arange(c.n), si.kept_rows(c))
    order = np.argsort(np.where(live, ek, np.inf), kind="stable")
    want = order[:min(c.k, int(live.sum()))]
    assert np.isin(want, m.all_ids).all()


def test_the_table_reaches_the_enumerated_paths():
    got = sorted({sm.path_name(_model(c)[0].path) for c in si.CASES})
    assert got == si.PATHS
    words = " ".join(got)
    for w in ("NT256-regs", "NT1024-regs", "NT1024-mem", "none/", "groups4/", "plain/", "groups2k/", "short-small", "short-large",
              "flooded", "all-tiles", "tau-nan", " over", "refined-regs", "refined-mem", "diff0", "top31", "radix-found",
              "radix-not_found", "filter", "overflow", "list-radix", "f16:", "redone"):
        assert w in words, w


def test_a_dropped_case_is_noticed():
    unnoticed = []
    for c in si.CASES:
        rest = {sm.path_name(_model(x)[0].path) for x in si.CASES if x is not c}
        if rest == set(si.PATHS):
            unnoticed.append(c.name)
    assert sorted(unnoticed) == sorted(si.HELD_BY_RULE)


@pytest.mark.parametrize("c", si.CASES, ids=repr)
def test_thresholds_stand_alone(c):
    """U, tau, the refined tau and the radix select's k-th key: no other key value of a live row within 2^-8 of them."""
    m, _, live, ek = _model(c)  # (the keys the select sees: the fp16 store's are the stored upper sides)
    thr = {"tau": m.tau0, "tau_out": m.header["tau_key"], "kth": getattr(m, "radix_kth", sm.KEY_NAN)}
    if m.path["prefilter"] != "none":
        thr["U"] = m.U
    if c.plant == "list":
        live = live & np.isin(np.arange(c.n), si.kept_rows(c))
    vals = np.unique(ek[live].astype(np.float32)).astype(np.float64)
    checked = crowded = 0
    for name, key in thr.items():
        if key >= sm.KEY_NAN:
            continue
        t = float(sm.key2f(np.uint32(key)).reshape(-1)[0])
        near = vals[(np.abs(vals - t) < abs(t) * 2.0 ** -8) & (vals != t)]
        if c.name in si.GAP_EXEMPT:
            crowded += len(near) > 0
            continue
        assert len(near) == 0, (c.name, name, t, near[:4])
        checked += 1
    # (C-ulps is exempt because it IS crowded; group H because the fp16 band is per cent of a key, not 2^-8 of it)
    assert crowded > 0 or c.name != "C-ulps", "the exemption is not needed"
    # (no finite threshold at all -- fewer live keys than k -- is a path that rests on no order of keys)
    assert checked > 0 or c.name in si.GAP_EXEMPT or all(k >= sm.KEY_NAN for k in thr.values())
    assert set(si.GAP_EXEMPT) <= set(si.BY_NAME)


def test_the_band_round_up_shows():
    """A band_of without its round-up to the next float gives another band_key wherever the f64 band rounds DOWN to its
    nearest float (about every other finite band): the header check of the GPU test sees it in those cases.  The
    candidate SETS do not change -- the gap is there to keep them still."""
    differ = [c.name for c in si.CASES if _model(c)[0].header["band_key"] != _model(c, band_round_up=False)[0].header["band_key"]]
    print(differ)
    assert differ


def test_the_ulps_case_stands_on_the_last_radix_round():
    """C-ulps: the keys planted round the k-th share their upper three bytes with it or differ in the third alone, so the
    radix select's LAST round has several occupied bins to choose among (and the k-th key is one of the planted 300)."""
    c = si.BY_NAME["C-ulps"]
    m, ek, live, _ = _model(c)
    assert m.path["host_radix"] == "found" and len(m.radix_bins) == 4
    assert m.radix_bins[3] > 1, m.radix_bins
    kth = float(sm.key2f(np.uint32(m.radix_kth)).reshape(-1)[0])
    planted = (1.25 + np.arange(300) * 2.0 ** -23) ** 2
    assert planted.min() <= kth <= planted.max()
    assert np.sum(ek.astype(np.float32) == np.float32(kth)) >= 1


def test_the_f16_cases_decide_by_the_per_row_rule():
    """Group H: in the plain and the refined case rows lie at or below the band that the per-row rule sends away -- a second
    emit without the rule would count more."""
    for name in ("H-f16-plain", "H-f16-refined"):
        c = si.BY_NAME[name]
        m, _, live, seen = _model(c)
        band = float(sm.key2f(np.uint32(m.header["band_key"])).reshape(-1)[0])
        assert int(np.sum(seen[live] <= band)) > m.header["count"] >= c.k, name


def test_held_by_rule_names_cases():
    assert set(si.HELD_BY_RULE) <= set(si.BY_NAME)
