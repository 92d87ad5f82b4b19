"""GPU: seeded fuzz over SEQUENCES of calls on the routes that came after test_fuzz_call_sequences (test_gpu_fuzz.py):
cursor pages (search_after, submit(after=)), counts (search_count), the fp16 and int8 copies of the rows forced on at
sizes far below their 256 MiB gate (set_scan_f16 / _masked, set_scan_i8 / _masked = 2 with set_exact_scan_rows(0)) and the
two scan streams -- interleaved with appends (new ids, gaps, overwrites, growth past the capacity, rows that move the
fp16 scale, quarantined rows, a crowd of more than AFTER_SIDE_CAP identical rows), deletes, option changes and mask
handles held across them, on one handle and on a handle over three shards.  Every answer must equal the oracle's list
(search_exhaustive over a NumPy model of the rows) -- ids equal, distances bit for bit, counts with ==.

_plan(seed, case) draws a whole case without touching the GPU or the oracle; values that depend on distances are NAMES
in the plan ("the entry at rank r of the oracle's list, one ulp above") that _run resolves from the oracle only, never
from the library's answer.  The plan also fixes the coverage: tests/test_host_fuzz_plan.py reads the conditions off the
plans on the CPU; the counters the library keeps are asserted per seed here.

Replay one case: TSH_FUZZ_VERBOSE=1 prints every step; a failure's message carries seed/case/step, the op, d, the
metric, the option vector, the mask form, the threshold and the cursor.

Measured on one MI355X (per seed: six cases of 30 steps; scans and redos count once per shard):
  seed      fp16 scans/redone  rows converted (first builds)  int8 scans/redone  cursor searches/redone  counts/redone  list  exact   time
  routes 1       78 / 1              23237 (10556)                 63 / 1              125 / 0             232 / 1       7     10    0.92 s
  routes 2      100 / 0              18549 (3981)                  88 / 0              109 / 1             187 / 1      15     11    0.87 s
  routes 3      129 / 0              18782 (3844)                  95 / 2              101 / 1             179 / 0      38      8    0.91 s
  routes 4       39 / 2              25431 (3813)                 128 / 0              114 / 1             179 / 0      19     12    0.87 s
  ties 1         54 / 0              17881 (4741)                 122 / 0              136 / 5             213 / 0       6     11    0.87 s
  ties 2         50 / 1              19593 (7578)                  72 / 0              114 / 3             159 / 2       3     17    0.80 s
against 1.07 s, 0.77 s and 0.64 s for test_fuzz_call_sequences[1..3] on the same machine (0.95 / 0.80 / 0.75 s and
0.75 - 0.83 s for these seeds inside a run of the whole suite).  The redone share stays far below the cap of one half
with per-row scaling by uniform(0.1, 30): the scaling was left as it is.

Held against four wrong-answer builds of the library, each a one-line change of the host code: a copy that an
overwrite does not invalidate, all_live kept after a delete, an fp16 copy not converted again when its scale changes,
a side-list redo that drops its mask.  Every one fails these tests (the third in routes 1, case 2: the searches behind
the row of 3e5 appended as a new id); none of them is in the tree.
"""
import math
import os

import numpy as np
import pytest

from test_gpu_fuzz import _spoil_some
from test_gpu_search_count import _past

pytestmark = pytest.mark.gpu

WIDTHS = (8, 100, 256, 264, 768, 1000)
F16_WIDTHS = (256, 264, 768, 1000)  # scan_f16_supported: at least 256 elements, a multiple of 8 (264, 1000 end inside a chunk)
STEPS = 30
CASES = 6
ROUTE_SEEDS = (1, 2, 3, 4)
TIES_SEEDS = (1, 2)
MASK_FORMS = ("none", "byte", "fresh", "held")
BYTE_KINDS = ("50", "2", "run")
LIST_MIN_ROWS = 4096  # row_list_pays: a shard of fewer rows scans a selective mask as tiles, whatever it keeps
DEFAULT_OPTS = {"f16": 1, "f16m": 1, "i8": 1, "i8m": 1, "streams": 0, "exact_rows": 16384, "exact_select": True, "batch_min_nq": 1}
# A case's copy route forced on over an otherwise independent draw.  strict: the exact path (which would answer these
# small shards whole) off and the other pair off as well, so that the scans do run on this copy (an int8 route that
# applies is taken before the fp16 one); loose: only what the route cannot do without -- the other pair, the exact path
# under the int8 pair (whose value 2 overrides it) and everything else stay as drawn
ROUTE_OPTS = {
    ("f16", True): {"f16": 2, "f16m": 2, "i8": 0, "i8m": 0, "exact_rows": 0},
    ("i8", True): {"f16": 0, "f16m": 0, "i8": 2, "i8m": 2, "exact_rows": 0},
    ("f16", False): {"f16": 2, "f16m": 2, "exact_rows": 0},
    ("i8", False): {"i8": 2, "i8m": 2},
}


def _max_rows(d):
    return 9000 if d <= 264 else 4000


def _round_up(v, m):
    return (v + m - 1) // m * m


# ---- the plan ---------------------------------------------------------------------------------------------------------
class _PlanState:
    """What the plan knows of the index without any data: which ids are present, alive, possibly quarantined; the
    options in force; whether a handle is held; an upper bound of the row store's capacity."""

    def __init__(self, d, shards, cap, limit):
        # limit: what ordinary appends stay below -- one id under the hard limit, kept for the row that moves the scale
        self.d, self.shards, self.limit = d, shards, limit - 1
        self.per = _round_up(-(-cap // shards), 64) if shards > 1 else 0  # a shard's rows on a handle over several
        self.present = np.zeros(0, bool)
        self.alive = np.zeros(0, bool)
        self.spoiled = np.zeros(0, bool)
        self.opts = dict(DEFAULT_OPTS)
        self.held = False
        self.cap_est = _round_up(max(cap, 1), 64)
        self.grew = False
        self.crowd = None  # (first, n) of the block of identical rows

    @property
    def n(self):
        return len(self.present)

    def dense(self):
        return bool(self.n and np.all(self.present & self.alive & ~self.spoiled))

    def append(self, first, n, spoil):
        end = first + n
        if end > self.n:
            grow = end - self.n
            self.present = np.concatenate([self.present, np.zeros(grow, bool)])
            self.alive = np.concatenate([self.alive, np.zeros(grow, bool)])
            self.spoiled = np.concatenate([self.spoiled, np.zeros(grow, bool)])
        self.present[first:end] = True
        self.alive[first:end] = True
        self.spoiled[first:end] = spoil
        if end > self.cap_est:  # shard_reserve: at least half as much again
            self.cap_est = max(_round_up(end, 64), _round_up(self.cap_est + self.cap_est // 2, 64))

    def delete(self, ids):
        self.alive[np.asarray(ids, np.int64)] = False


def _sub(rng):
    return int(rng.integers(0, 2**31 - 1))


def _draw_mask(rng, st, form=None, kind=None, over=None):
    if form is None:
        forms, w = ["none", "byte", "fresh"], [0.35, 0.3, 0.15]
        if st.held:
            forms, w = forms + ["held"], w + [0.2]
        form = str(rng.choice(forms, p=np.asarray(w) / sum(w)))
    m = {"form": form}
    if form in ("byte", "fresh"):
        m.update(kind=kind or str(rng.choice(BYTE_KINDS, p=[0.5, 0.25, 0.25])), seed=_sub(rng), at=float(rng.random()), frac=float(rng.uniform(0.01, 0.4)))
    if over:  # a run laid over a range of ids: (first, length)
        m.update(kind="run", range=(int(over[0]), int(over[1])))
    if form == "fresh":
        st.held = True  # made in this step and held for the steps to come
    return m


def _draw_thr(rng, st, tie=False):
    ulp = int(rng.choice([0, 1, -1]))
    if tie and st.crowd and rng.random() < 0.6:
        return ("row", st.crowd[0] + st.crowd[1] // 2, ulp)
    if rng.random() < 0.4:
        return None
    return ("rank", float(rng.random()), ulp)


def _draw_cursor(rng, st, tie=False):
    if tie and st.crowd and rng.random() < 0.6:
        return ("tie", st.crowd[0] + int(rng.integers(0, st.crowd[1])))
    kind = str(rng.choice(["start", "rank", "rank_id_minus", "rank_big", "between"], p=[0.15, 0.4, 0.15, 0.15, 0.15]))
    return (kind,) if kind == "start" else (kind, float(rng.random()))


def _block_spec(rng, n, kind="normal", scale=None, spoil=None):
    return {"kind": kind, "seed": _sub(rng), "n": int(n),
            "scale": bool(rng.random() < 0.3) if scale is None else scale,
            "spoil": bool(rng.random() < 0.15) if spoil is None else spoil}


def _plan_append(rng, st, what=None):
    n_now = st.n
    limit = st.limit if st.shards > 1 or st.grew else min(st.limit, int(0.6 * _max_rows(st.d)))
    if what is None:
        what = str(rng.choice(["end", "gap", "overwrite", "bigrow"], p=[0.4, 0.15, 0.4, 0.05]))
    if what in ("end", "gap") and n_now + 21 >= limit:
        what = "overwrite"
    if what == "growth" and st.shards > 1:
        what = "overwrite"  # (a handle over several shards: appends stay inside capacity_rows)
    if what == "end":
        first, n = n_now, int(rng.integers(1, min(3000, limit - n_now) + 1))
    elif what == "gap":
        first = n_now + int(rng.integers(1, 21))
        n = int(rng.integers(1, min(3000, limit - first) + 1))
    elif what == "overwrite":  # 1..3000 stored rows, deleted ones included (they live again); may run past the end
        first = int(rng.integers(0, n_now))
        n = int(rng.integers(1, min(3000, limit - first) + 1))
    elif what == "fill":  # up to LIST_MIN_ROWS and a little more: from there on a shard lists a selective mask's rows
        first, n = n_now, max(LIST_MIN_ROWS + int(rng.integers(1, 200)) - n_now, 1)
        assert n <= 3000 and first + n <= limit
    elif what == "growth":  # past the capacity: the row store and both copies reallocate
        first = n_now
        n = st.cap_est + int(rng.integers(1, 100)) - n_now
        assert first + n <= st.limit, "the plan left no room to grow past the capacity"
        st.grew = True
    elif what == "crowd":  # more ties than AFTER_SIDE_CAP = 1024
        n = int(rng.integers(1100, 1501))
        first = int(rng.integers(0, n_now - n + 1))
        st.crowd = (first, n)
    elif what == "bigrow_new":  # one row whose largest element is about 3e5 -- the fp16 scale's exponent moves -- as a
        # NEW id: no stored row is overwritten, so the copy keeps its watermark and only the changed scale can make the
        # library convert the rows below it again (the id kept free by _PlanState.limit)
        first, n = n_now, 1
        assert first + n <= st.limit + 1
    else:  # "bigrow": the same row over a stored one (the overwrite rebuilds the copy whatever the scale)
        first, n = int(rng.integers(0, n_now)), 1
    if what == "crowd":
        block = _block_spec(rng, n, "crowd", scale=False, spoil=False)
    elif what in ("bigrow", "bigrow_new"):
        block = _block_spec(rng, n, "bigrow", scale=False, spoil=False)
    else:
        block = _block_spec(rng, n)
    st.append(first, n, block["spoil"])
    return {"op": "append", "what": what, "first": first, "block": block}


def _plan_delete(rng, st, what=None):
    if what is None:
        what = str(rng.choice(["ids", "tile", "last"], p=[0.6, 0.25, 0.15]))
    if what == "tile" and st.n >= 64:
        t = int(rng.integers(0, st.n // 64))
        ids = list(range(64 * t, 64 * t + 64))
    elif what == "last":
        ids = [st.n - 1]
    else:
        # (any id below the index's length: one may repeat, name a row deleted before or an id inside a gap that was
        # never appended -- the library ignores those, and the model's `alive` bit of an absent id changes nothing)
        what = "ids"
        ids = [int(x) for x in rng.integers(0, st.n, size=int(rng.integers(1, 49)))]
        if st.shards > 1 and st.per < st.n:  # ... and on several shards, the two rows either side of the first edge
            ids += [st.per - 1, st.per]
    st.delete(ids)
    return {"op": "delete", "what": what, "ids": ids}


def _plan_option(rng, st, route=None, strict=True):
    o = {"f16": int(rng.choice([0, 2])), "f16m": int(rng.choice([0, 2])), "i8": int(rng.choice([0, 2])),
         "i8m": int(rng.choice([0, 2])), "streams": int(rng.choice([0, 1, 2])), "exact_rows": int(rng.choice([0, 0, 700, 16384])),
         "exact_select": bool(rng.random() < 0.5), "batch_min_nq": int(rng.choice([0, 2]))}
    if route:
        o.update(ROUTE_OPTS[(route, strict)])
    st.opts = dict(o)
    return {"op": "option", "opts": o}


def _plan_search(rng, st, mask=None):
    nq = int(rng.integers(2, 10)) if st.opts["batch_min_nq"] == 0 and rng.random() < 0.4 else 1
    dense = st.dense()
    m = _draw_mask(rng, st, mask)
    return {"op": "search", "nq": nq, "k": int(rng.choice([1, 5, 40, 300])), "thr": _draw_thr(rng, st), "mask": m,
            "qseed": _sub(rng), "opts": dict(st.opts), "dense": dense and m["form"] == "none"}


def _plan_small_mutation(rng, st, what=None):
    """an overwrite or a delete that leaves the index's length alone: between two pages of a walk"""
    if what == "append" or (what is None and rng.random() < 0.5):
        first = int(rng.integers(0, st.n))
        n = int(rng.integers(1, min(300, st.n - first) + 1))
        block = _block_spec(rng, n)
        st.append(first, n, block["spoil"])
        return {"op": "append", "what": "overwrite", "first": first, "block": block}
    return _plan_delete(rng, st)


def _plan_pages(rng, st, mask=None, tie=False, thr="draw", cursor=None, between=None, over=None):
    m = _draw_mask(rng, st, mask, over=over)
    pages = int(rng.integers(2, 5))
    step = {"op": "pages", "pages": pages, "k": int(rng.choice([1, 7, 64])), "mask": m, "qseed": _sub(rng),
            "thr": _draw_thr(rng, st, tie) if thr == "draw" else thr,
            "cursor": _draw_cursor(rng, st, tie) if cursor is None else cursor,
            "count_around": bool(rng.random() < 0.4), "between": None, "opts": dict(st.opts)}
    if between or rng.random() < 0.3:
        step["between"] = (int(rng.integers(0, pages - 1)), _plan_small_mutation(rng, st, between))
    return step


def _plan_count(rng, st, mask=None, tie=False, thr="draw", cursors="draw", kind=None):
    m = _draw_mask(rng, st, mask, kind)
    if cursors == "draw":
        r = rng.random()
        cursors = None if r < 0.25 else [_draw_cursor(rng, st, tie) for _ in range(5 if r > 0.75 else 1)]
    return {"op": "count", "mask": m, "qseed": _sub(rng), "thr": _draw_thr(rng, st, tie) if thr == "draw" else thr,
            "cursors": cursors, "opts": dict(st.opts)}


def _plan_tickets(rng, st):
    tickets = []
    for _ in range(int(rng.integers(1, 5))):
        kind = str(rng.choice(["plain", "byte", "handle", "after"]))
        form = {"plain": "none", "byte": "byte", "handle": "held" if st.held else "fresh"}.get(kind)
        if kind == "after":
            form = str(rng.choice(["none", "byte", "held" if st.held else "fresh"]))
        t = {"kind": kind, "k": int(rng.choice([1, 5, 40, 300])), "mask": _draw_mask(rng, st, form), "qseed": _sub(rng),
             "cursor": _draw_cursor(rng, st) if kind == "after" else None,
             "wait_thr": _draw_thr(rng, st) if rng.random() < 0.4 else None}
        tickets.append(t)
    return {"op": "tickets", "tickets": tickets, "count_between": bool(rng.random() < 0.4), "qseed": _sub(rng), "opts": dict(st.opts)}


def _plan(seed, case, ties=False):
    """One case, drawn whole: {"d", "metric", "capacity", "shards", "route", "steps"}.  No GPU, no oracle, no rows."""
    rng = np.random.default_rng([7000 if ties else 5000, seed, case])
    d = WIDTHS[(case + seed) % len(WIDTHS)]
    metric = (case + 2 * seed) % 3
    shards = 3 if case % 3 == 2 else 1
    # even cases force the fp16 pair where the width has one, every other case the int8 pair
    route = "f16" if case % 2 == 0 and d in F16_WIDTHS else "i8"
    n0 = int(rng.integers(1500, 2200 if d >= 768 else 3000))
    n0 += n0 % 64 == 0  # never a multiple of the tile
    if shards == 1:
        cap = int(rng.integers(64, 1500))  # the first append already grows past it
        limit = _max_rows(d)
    else:  # three shards of round_up(ceil(cap / 3), 64) rows: the first append spans the first edge at least
        cap = int(rng.integers(n0 + 200, min(_max_rows(d), 2 * n0) + 1))
        limit = cap
    st = _PlanState(d, shards, cap, limit)
    kinds = ("overwrite", "growth", "delete")
    dead = ("tile", "last", "ids")[case % 3]  # (the forced deletes: every kind over a seed's cases; "ids" on three shards)
    crowd = ties or case == 4
    forced = {
        1: lambda: _plan_search(rng, st, "none"),  # under the default options: the exact path answers so small an index
        2: lambda: _plan_option(rng, st, route),
        3: lambda: _plan_search(rng, st, "none"),  # (nothing deleted, spoiled or skipped so far: a dense scan)
        4: lambda: _plan_search(rng, st, "byte"),
        5: lambda: _plan_pages(rng, st, "fresh"),
        6: lambda: _plan_count(rng, st, "held"),
        10: lambda: _plan_delete(rng, st, dead) if kinds[case % 3] == "delete" else _plan_append(rng, st, kinds[case % 3]),
        11: lambda: _plan_pages(rng, st, "held", tie=ties, between="delete" if case % 2 else "append"),
        12: lambda: _plan_option(rng, st, route, strict=False),
        13: lambda: _plan_search(rng, st, "held"),
        14: lambda: _plan_search(rng, st, "none"),
        15: lambda: _plan_search(rng, st, "fresh"),
        16: lambda: _plan_delete(rng, st, dead) if kinds[(case + 1) % 3] == "delete" else _plan_append(rng, st, kinds[(case + 1) % 3]),
        17: lambda: _plan_count(rng, st, "fresh", tie=ties),
        18: lambda: _plan_append(rng, st, "gap" if case % 2 else "end"),
        19: lambda: _plan_count(rng, st, "byte", kind="2"),  # a selective mask (the list scan: see below)
        21: lambda: _plan_delete(rng, st, dead) if kinds[(case + 2) % 3] == "delete" else _plan_append(rng, st, kinds[(case + 2) % 3]),
        22: lambda: _plan_pages(rng, st, "byte", tie=ties) if case % 2 else _plan_count(rng, st, "byte", tie=ties),
        23: lambda: _plan_tickets(rng, st),
    }
    if shards == 1 and d <= 264:  # the sizes that may hold LIST_MIN_ROWS rows in one shard: filled up to there first
        forced[19] = lambda: _plan_append(rng, st, "fill")
        forced[20] = lambda: _plan_count(rng, st, "byte", kind="2")
    if crowd:  # the crowd, then a walk and a count at its distance behind no mask: the side-list redo fires here, in the
        # middle of the sequence, and every later cursor and count job of the handle follows it
        forced[7] = lambda: _plan_append(rng, st, "crowd")
        # (odd cases: behind a fresh handle that keeps the crowd and little else -- the redo must keep its mask)
        forced[8] = lambda: _plan_pages(rng, st, "fresh" if case % 2 else "none", thr=None, cursor=("tie", st.crowd[0] + st.crowd[1] // 2),
                                        over=(max(0, st.crowd[0] - 40), st.crowd[1] + 90) if case % 2 else None)
        forced[9] = lambda: _plan_count(rng, st, "none", thr=("row", st.crowd[0] + st.crowd[1] // 2, 0), cursors=None)
    if case % 2 == 0:  # late in the case: the fp16 scale's exponent moves between two forced-fp16 searches -- a search
        # that leaves the copy current, the row as a new id (nothing overwritten, nothing reallocated), two searches
        forced[24] = lambda: _plan_option(rng, st, route)
        forced[25] = lambda: _plan_search(rng, st, "none")
        forced[26] = lambda: _plan_append(rng, st, "bigrow_new")
        forced[27] = lambda: _plan_search(rng, st, "none")
        forced[28] = lambda: _plan_search(rng, st, "byte")
    block0 = _block_spec(rng, n0, spoil=False)
    st.append(0, n0, False)
    steps = [{"op": "append", "what": "end", "first": 0, "block": block0}]
    ops = ["append", "delete", "option", "search", "tickets", "pages", "count"]
    weights = np.asarray([3, 2, 2, 4, 2, 3, 3], float)
    for i in range(1, STEPS):
        if i in forced:
            steps.append(forced[i]())
            continue
        op = str(rng.choice(ops, p=weights / weights.sum()))
        if op == "append":
            steps.append(_plan_append(rng, st))
        elif op == "delete":
            steps.append(_plan_delete(rng, st))
        elif op == "option":
            steps.append(_plan_option(rng, st))
        elif op == "search":
            steps.append(_plan_search(rng, st))
        elif op == "tickets":
            steps.append(_plan_tickets(rng, st))
        elif op == "pages":
            steps.append(_plan_pages(rng, st, tie=ties))
        else:
            steps.append(_plan_count(rng, st, tie=ties))
    return {"seed": seed, "case": case, "ties": ties, "d": d, "metric": metric, "capacity": cap, "shards": shards,
            "route": route, "steps": steps}


# ---- the execution ----------------------------------------------------------------------------------------------------
def _block(spec, d):
    """The rows of a planned block, generated on demand from its seed"""
    rng = np.random.default_rng(spec["seed"])
    n = spec["n"]
    if spec["kind"] == "crowd":
        return np.tile(rng.standard_normal(d).astype(np.float32), (n, 1))
    rows = rng.standard_normal((n, d)).astype(np.float32)
    if spec["scale"]:
        rows *= rng.uniform(0.1, 30.0, (n, 1)).astype(np.float32)
    if spec["kind"] == "bigrow":
        rows[0, int(rng.integers(0, d))] = 3.0e5
    if spec["spoil"]:
        _spoil_some(rng, rows)
    return rows


def _mask_bits(spec, n):
    rng = np.random.default_rng(spec["seed"])
    if spec["kind"] == "run":  # WHERE id BETWEEN ...
        kb = np.zeros(n, bool)
        a0, length = spec.get("range") or (int(spec["at"] * n), max(1, int(spec["frac"] * n)))
        kb[a0:a0 + length] = True
        return kb
    return rng.random(n) < (0.5 if spec["kind"] == "50" else 0.02)


def _ulp(v, ulp):
    v = float(v)
    return v if ulp == 0 else float(np.nextafter(v, np.inf if ulp > 0 else -np.inf))


def _same_dist(a, b, nan_ok):
    """bit for bit; where rows were spoiled a NaN equals a NaN (their payloads are nobody's promise)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    if not nan_ok:
        return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


class _Runner:
    def __init__(self, plan, oracle, idx, make_mask):
        self.plan, self.oracle, self.idx, self.make_mask = plan, oracle, idx, make_mask
        self.d, self.metric = plan["d"], plan["metric"]
        self.model = np.zeros((0, self.d), np.float32)
        self.present = np.zeros(0, bool)
        self.alive = np.zeros(0, bool)
        self.held = None  # (handle, its bitmap as made)
        self.nan_ok = False  # a block was spoiled: NaN distances can occur from now on
        self.opts = dict(DEFAULT_OPTS)
        self.f16_first_rows = None  # the model's length when the fp16 copy was first built
        self.tag = ""

    # -- the model ---------------------------------------------------------------------------------------------------
    def append(self, step):
        block = _block(step["block"], self.d)
        first, n = step["first"], len(block)
        self.nan_ok = self.nan_ok or step["block"]["spoil"]
        self.idx.append(first, block)
        if first + n > len(self.model):
            grow = first + n - len(self.model)
            self.model = np.concatenate([self.model, np.zeros((grow, self.d), np.float32)])
            self.present = np.concatenate([self.present, np.zeros(grow, bool)])
            self.alive = np.concatenate([self.alive, np.zeros(grow, bool)])
        self.model[first:first + n] = block
        self.present[first:first + n] = True
        self.alive[first:first + n] = True  # a (re)written row is live again

    def delete(self, step):
        ids = np.asarray(step["ids"], np.int64)
        self.idx.set_deleted(ids)
        self.alive[ids] = False

    def mutate(self, step):
        self.append(step) if step["op"] == "append" else self.delete(step)

    def option(self, step):
        o, idx = step["opts"], self.idx
        idx.set_scan_f16(o["f16"])
        idx.set_scan_f16_masked(o["f16m"])
        idx.set_scan_i8(o["i8"])
        idx.set_scan_i8_masked(o["i8m"])
        idx.set_scan_streams(o["streams"])
        idx.set_exact_scan_rows(o["exact_rows"])
        idx.set_exact_select(o["exact_select"])
        idx.set_batch_min_nq(o["batch_min_nq"])
        self.opts = dict(o)

    # -- what a step's names mean --------------------------------------------------------------------------------------
    def queries(self, seed, nq):
        qs = np.random.default_rng(seed).standard_normal((nq, self.d)).astype(np.float32)
        if self.metric == 2:
            qs = np.stack([self.oracle.normalize_f32(q) for q in qs])
        return qs

    def mask(self, spec, temps=None):
        """-> (what the library is given, the kept rows as the model sees them or None).  A fresh handle replaces the
        held one (temps: kept open there instead, for tickets that still read the old one)."""
        n = len(self.model)
        form = spec["form"]
        if form == "none":
            return None, None
        if form == "held":
            kb = np.zeros(n, bool)  # rows appended since it was made are not kept
            m = min(n, len(self.held[1]))
            kb[:m] = self.held[1][:m]
            return self.held[0], kb
        kb = _mask_bits(spec, n)
        bits = np.packbits(kb, bitorder="little")
        if form == "byte":
            return bits, kb
        if self.held is not None:
            temps.append(self.held[0]) if temps is not None else self.held[0].close()
        self.held = (self.make_mask(self.idx, bits), kb)
        return self.held[0], kb

    def eff_bits(self, kb):
        eff = self.present & self.alive
        return np.packbits(eff if kb is None else eff & kb, bitorder="little")

    def full(self, q, thr, kb):
        """the oracle's whole ordered list under a threshold and a mask"""
        with np.errstate(all="ignore"):
            return self.oracle.search_exhaustive(self.model, q, self.metric, len(self.model), thr, self.eff_bits(kb))

    def row_dist(self, q, rid):
        rid = min(rid, len(self.model) - 1)
        with np.errstate(all="ignore"):
            return float(self.oracle.all_distances(q, self.model[rid:rid + 1], self.metric)[0])

    def thr(self, name, q, l0):
        if name is None:
            return None
        if name[0] == "row":
            return _ulp(self.row_dist(q, name[1]), name[2])
        if len(l0[0]) == 0:
            return 0.5
        return _ulp(l0[1][int(name[1] * len(l0[0]))], name[2])

    def cursor(self, name, q, l0):
        if name is None:
            return None
        if name[0] == "start":
            return (-math.inf, 0)
        if name[0] == "tie":  # inside the crowd of ties (or wherever that row is by now)
            return (self.row_dist(q, name[1]), int(name[1]))
        eids, edist = l0
        if len(eids) == 0:
            return (0.5, 0)
        r = int(name[1] * len(eids))
        dd, i = float(edist[r]), int(eids[r])
        if name[0] == "rank":
            return (dd, i)
        if name[0] == "rank_id_minus":
            return (dd, i - 1)
        if name[0] == "rank_big":
            return (dd, 2**62)
        nxt = float(edist[min(r + 1, len(eids) - 1)])  # "between": a distance between two rows, on no row
        return (dd + (nxt - dd) / 2 if np.isfinite(dd) and np.isfinite(nxt) else dd, 0)

    @staticmethod
    def after(l, cursor):
        """the slice of an oracle list past a cursor"""
        past = _past(l[0], l[1], cursor)
        return l[0][len(l[0]) - past:], l[1][len(l[1]) - past:]

    # -- the steps ---------------------------------------------------------------------------------------------------------
    def search(self, step):
        qs = self.queries(step["qseed"], step["nq"])
        mask, kb = self.mask(step["mask"])
        thr = self.thr(step["thr"], qs[0], self.full(qs[0], None, kb))
        tag = f"{self.tag} thr={thr!r}"
        ids, dist, cnt = self.idx.search(qs, step["k"], thr, mask)
        for i in range(step["nq"]):
            eids, edist = self.full(qs[i], thr, kb)
            eids, edist = eids[:step["k"]], edist[:step["k"]]
            assert cnt[i] == len(eids), f"{tag} q{i}: count {cnt[i]} != {len(eids)}"
            assert np.array_equal(ids[i, :cnt[i]], eids), f"{tag} q{i}: ids"
            assert _same_dist(dist[i, :cnt[i]], edist, self.nan_ok), f"{tag} q{i}: distances"

    def pages(self, step):
        q = self.queries(step["qseed"], 1)[0]
        mask, kb = self.mask(step["mask"])
        l0 = self.full(q, None, kb)
        thr, cur, k = self.thr(step["thr"], q, l0), self.cursor(step["cursor"], q, l0), step["k"]
        for page in range(step["pages"]):
            tag = f"{self.tag} thr={thr!r} page={page} cursor={cur!r}"
            eids, edist = self.after(self.full(q, thr, kb), cur)
            if step["count_around"]:
                before = int(self.idx.search_count(q, thr, mask, cur)[0])
                assert before == len(eids), f"{tag}: count before the page {before} != {len(eids)}"
            ids, dist, cnt = self.idx.search_after(q, k, cur, thr, mask)
            c = int(cnt[0])
            assert c == min(k, len(eids)), f"{tag}: count {c} != {min(k, len(eids))}"
            assert np.array_equal(ids[0, :c], eids[:c]), f"{tag}: ids"
            assert _same_dist(dist[0, :c], edist[:c], self.nan_ok), f"{tag}: distances"
            if c:
                cur = (float(edist[c - 1]), int(eids[c - 1]))  # (the oracle's entry, not the library's)
            if step["count_around"]:
                left = int(self.idx.search_count(q, thr, mask, cur)[0])
                assert left == before - c, f"{tag}: count after the page {left} != {before} - {c}"
            if step["between"] and step["between"][0] == page:
                # the next page is the slice of the NEW list past the old cursor: a cursor is a value, not a position
                # (an overwrite or a delete: the index keeps its length, and the mask its meaning)
                self.mutate(step["between"][1])

    def count(self, step):
        q = self.queries(step["qseed"], 1)[0]
        mask, kb = self.mask(step["mask"])
        l0 = self.full(q, None, kb)
        thr = self.thr(step["thr"], q, l0)
        lt = self.full(q, thr, kb)
        if step["cursors"] is None:
            got = self.idx.search_count(q, thr, mask)
            assert got.tolist() == [len(lt[0])], f"{self.tag} thr={thr!r} cursor=None: {got.tolist()} != {len(lt[0])}"
            return
        cursors = [self.cursor(c, q, l0) for c in step["cursors"]]
        a_dist = np.asarray([c[0] for c in cursors], np.float64)
        a_id = np.asarray([c[1] for c in cursors], np.int64)
        got = self.idx.search_count(np.tile(q, (len(cursors), 1)), thr, mask, (a_dist, a_id))
        want = [_past(lt[0], lt[1], c) for c in cursors]
        assert got.tolist() == want, f"{self.tag} thr={thr!r} cursors={cursors!r}: {got.tolist()} != {want}"

    def tickets(self, step):
        temps, out = [], []
        try:
            for t in step["tickets"]:  # all submitted before any is waited for
                q = self.queries(t["qseed"], 1)[0]
                mask, kb = self.mask(t["mask"], temps)
                l0 = self.full(q, None, kb)
                cur = self.cursor(t["cursor"], q, l0)
                ticket = self.idx.submit(q, t["k"], mask, after=cur)
                out.append((ticket, t, q, kb, cur, self.thr(t["wait_thr"], q, l0)))
            if step["count_between"]:  # a count on another context while the tickets are out
                q = self.queries(step["qseed"], 1)[0]
                got = int(self.idx.search_count(q)[0])
                want = len(self.full(q, None, None)[0])
                assert got == want, f"{self.tag}: count between submit and wait {got} != {want}"
            for n_t, (ticket, t, q, kb, cur, thr) in enumerate(out):  # in submission order
                ids, dist = self.idx.wait(ticket, thr)
                out[n_t] = None
                eids, edist = self.full(q, thr, kb)
                if cur is not None:
                    eids, edist = self.after((eids, edist), cur)
                eids, edist = eids[:t["k"]], edist[:t["k"]]
                tag = f"{self.tag} ticket {n_t} {t['kind']} k={t['k']} mask={t['mask']['form']} thr={thr!r} cursor={cur!r}"
                assert np.array_equal(ids, eids), f"{tag}: ids"
                assert _same_dist(dist, edist, self.nan_ok), f"{tag}: distances"
        finally:
            for o in out:  # (a failed assertion: appends, deletes and the close wait for every open ticket)
                if o is not None:
                    self.idx.wait(o[0])
            for h in temps:
                h.close()

    def run(self):
        plan = self.plan
        verbose = os.environ.get("TSH_FUZZ_VERBOSE")
        for n_step, step in enumerate(plan["steps"]):
            op = step["op"]
            what = step.get("what") or (step.get("mask") or {}).get("form")
            self.tag = (f"routes{'-ties' if plan['ties'] else ''} {plan['seed']}/{plan['case']}/{n_step} {op}({what}) d={self.d} "
                        f"metric={self.metric} shards={plan['shards']} n={len(self.model)} opts={self.opts} "
                        f"mask={step.get('mask')} thr={step.get('thr')} cursor={step.get('cursor', step.get('cursors'))}")
            if verbose:
                print(self.tag, {k: v for k, v in step.items() if k in ("nq", "k", "pages", "first", "count_around")}, flush=True)
            if op in ("append", "delete"):
                self.mutate(step)
            elif op == "option":
                self.option(step)
            else:
                getattr(self, op)(step)
                if self.f16_first_rows is None and self.idx.scan_f16_stats()["rows_converted"] > 0:
                    self.f16_first_rows = len(self.model)


def _run(plan, oracle):
    """Executes a planned case on a HipVectorIndex against the NumPy model -> the library's own counters at its end"""
    from tostore_amd import HipMask, HipVectorIndex, _ffi

    share = os.environ.get("TSH_SHARDS_SHARE_DEVICES")
    if plan["shards"] > 1:  # several shards of one handle on one GPU: a test hook, obeyed only once asked for
        os.environ["TSH_SHARDS_SHARE_DEVICES"] = "1"
        _ffi.enable_test_hooks()
    try:
        with HipVectorIndex(plan["d"], plan["metric"], capacity_rows=plan["capacity"], n_devices=plan["shards"]) as idx:
            r = _Runner(plan, oracle, idx, HipMask)
            r.run()
            f16, i8 = idx.scan_f16_stats(), idx.scan_i8_stats()
            after, count, c = idx.search_after_stats(), idx.search_count_stats(), idx.counters()
            if r.held is not None:
                r.held[0].close()
            return {"f16_scans": f16["scans"], "f16_redone": f16["redone"], "f16_rows_converted": f16["rows_converted"],
                    "f16_first_rows": r.f16_first_rows or 0, "i8_scans": i8["scans"], "i8_redone": i8["redone"],
                    "after_searches": after["searches"], "after_redone": after["redone"], "count_searches": count["searches"],
                    "count_redone": count["redone"], "list_scans": c["list_scans"], "exact_scans": c["exact_scans"]}
    finally:
        if plan["shards"] > 1:
            _ffi.enable_test_hooks(False)
            if share is None:
                os.environ.pop("TSH_SHARDS_SHARE_DEVICES", None)
            else:
                os.environ["TSH_SHARDS_SHARE_DEVICES"] = share


def _seed(oracle, seed, ties):
    total = {}
    for case in range(CASES):
        for k, v in _run(_plan(seed, case, ties), oracle).items():
            total[k] = total.get(k, 0) + int(v)
    print(f"routes{'-ties' if ties else ''} seed {seed}: {total}", flush=True)
    # every route ran inside the sequences (the library's own counters; each index starts from zero) ...
    for key in ("f16_scans", "i8_scans", "after_searches", "count_searches", "list_scans", "exact_scans"):
        assert total[key] > 0, (key, total)
    # ... the fp16 copy was rebuilt or extended after its first build ...
    assert total["f16_rows_converted"] > total["f16_first_rows"] > 0, total
    # ... and "everything was redone through f32" does not pass for coverage (a redo is a correct answer: no redone == 0)
    assert 2 * total["f16_redone"] < total["f16_scans"], total
    assert 2 * total["i8_redone"] < total["i8_scans"], total
    return total


@pytest.mark.parametrize("seed", ROUTE_SEEDS)
def test_fuzz_route_sequences(hip_lib, oracle_mod, seed):
    _seed(oracle_mod, seed, False)


@pytest.mark.parametrize("seed", TIES_SEEDS)
def test_fuzz_route_sequences_ties(hip_lib, oracle_mod, seed):
    """Every case holds a block of 1100..1500 identical rows -- more than the side list's 1024 -- and its walks and counts
    have thresholds and cursors at that crowd's distance: the side-list redo fires in the middle of a sequence."""
    total = _seed(oracle_mod, seed, True)
    assert total["after_redone"] + total["count_redone"] > 0, total
