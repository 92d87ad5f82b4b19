"""CPU: the plans of tests/test_gpu_fuzz_routes.py, read without a GPU.  _plan is deterministic, keeps to the shapes the
fuzz promises, and every seed's plans meet the coverage conditions that can be read off a plan: the fuzz guarantees its
coverage by construction, and this is where the construction is held to it."""
import pytest

from test_gpu_fuzz_routes import BYTE_KINDS, CASES, DEFAULT_OPTS, F16_WIDTHS, LIST_MIN_ROWS, MASK_FORMS, ROUTE_SEEDS, STEPS, TIES_SEEDS, WIDTHS, _max_rows, _plan

ALL_SEEDS = [(s, False) for s in ROUTE_SEEDS] + [(s, True) for s in TIES_SEEDS]


def _plans(seed, ties):
    return [_plan(seed, case, ties) for case in range(CASES)]


def _flat(step):
    """a step and the mutation planned between two of its pages, in the order they run"""
    return [step] + ([step["between"][1]] if step.get("between") else [])


@pytest.mark.parametrize("seed,ties", ALL_SEEDS)
def test_plan_is_deterministic(seed, ties):
    assert _plans(seed, ties) == _plans(seed, ties)
    assert _plan(seed, 0, ties) != _plan(seed + 1, 0, ties) and _plan(seed, 0, ties) != _plan(seed, 1, ties)


@pytest.mark.parametrize("seed,ties", ALL_SEEDS)
def test_plan_keeps_to_the_shapes(seed, ties):
    for plan in _plans(seed, ties):
        d, steps = plan["d"], plan["steps"]
        assert d in WIDTHS and plan["metric"] in (0, 1, 2) and plan["shards"] in (1, 3) and len(steps) == STEPS
        assert plan["shards"] == (3 if plan["case"] % 3 == 2 else 1)  # one case in three
        first = steps[0]
        assert first["op"] == "append" and first["first"] == 0 and first["block"]["n"] % 64 != 0
        n, edges = 0, {"append": set(), "delete": set()}
        per = (-(-plan["capacity"] // 3) + 63) // 64 * 64  # a shard's rows on a handle over three
        for step in steps:
            for s in _flat(step):
                if s["op"] == "append":
                    assert 1 <= s["block"]["n"] <= 3000 and 0 <= s["first"] <= n + 20
                    if s["what"] == "overwrite":
                        assert s["first"] < n
                    if s["what"] == "crowd":
                        assert 1100 <= s["block"]["n"] <= 1500 and s["first"] + s["block"]["n"] <= n
                    end = s["first"] + s["block"]["n"]
                    edges["append"] |= {e for e in (per, 2 * per) if s["first"] < e < end}
                    n = max(n, end)
                    assert n <= _max_rows(d)
                    if plan["shards"] == 3:
                        assert n <= plan["capacity"]  # appends stay inside capacity_rows
                elif s["op"] == "delete":
                    assert 1 <= len(s["ids"]) <= 64 and all(0 <= i < n for i in s["ids"])  # (gaps and repeats included)
                    if s["what"] == "tile":
                        assert len(s["ids"]) == 64 and s["ids"][0] % 64 == 0
                    if s["what"] == "last":
                        assert s["ids"] == [n - 1]
                    edges["delete"] |= {e for e in (per, 2 * per) if e - 1 in s["ids"] and e in s["ids"]}  # one call, both sides
            if step["op"] == "option":
                o = step["opts"]
                assert all(o[key] in (0, 2) for key in ("f16", "f16m", "i8", "i8m"))  # never 1: auto means "off" at these sizes
                assert o["streams"] in (0, 1, 2) and o["exact_rows"] in (0, 700, 16384) and o["batch_min_nq"] in (0, 2)
            if step["op"] == "search":
                assert step["k"] in (1, 5, 40, 300) and 1 <= step["nq"] <= 9
                assert step["nq"] == 1 or step["opts"]["batch_min_nq"] == 0  # pipelined single-query scans, never the batched path
            if step["op"] == "pages":
                assert 2 <= step["pages"] <= 4 and step["k"] in (1, 7, 64)
            if step["op"] == "tickets":
                assert 1 <= len(step["tickets"]) <= 4
        if plan["shards"] == 3:  # an append and a delete each span a shard edge
            assert edges["append"] and edges["delete"], edges


@pytest.mark.parametrize("seed,ties", ALL_SEEDS)
def test_plan_meets_the_coverage_conditions(seed, ties):
    plans = _plans(seed, ties)
    steps = [s for p in plans for s in p["steps"]]
    flat = [s for step in steps for s in _flat(step)]
    # each op, and each kind of append and delete
    assert {s["op"] for s in steps} == {"append", "delete", "option", "search", "tickets", "pages", "count"}
    assert {s["what"] for s in flat if s["op"] == "append"} >= {"end", "gap", "overwrite", "growth", "crowd", "bigrow_new"}
    assert {s["what"] for s in flat if s["op"] == "delete"} == {"ids", "tile", "last"}
    blocks = [s["block"] for s in flat if s["op"] == "append"]
    assert any(b["scale"] for b in blocks) and any(b["spoil"] for b in blocks) and not all(b["scale"] or b["spoil"] for b in blocks)
    # each mask form under each of search, pages and count; every byte mask; every ticket kind
    for op in ("search", "pages", "count"):
        assert {s["mask"]["form"] for s in steps if s["op"] == op} == set(MASK_FORMS), op
    assert {s["mask"]["kind"] for s in steps if s.get("mask", {}).get("form") in ("byte", "fresh")} == set(BYTE_KINDS)
    tickets = [t for s in steps if s["op"] == "tickets" for t in s["tickets"]]
    assert {t["kind"] for t in tickets} == {"plain", "byte", "handle", "after"}
    assert any(t["wait_thr"] for t in tickets) and any(s["count_between"] for s in steps if s["op"] == "tickets")
    assert max(len(s["tickets"]) for s in steps if s["op"] == "tickets") >= 3
    # every way to name a threshold and a cursor
    assert {(s["thr"] or ("none", 0, 0))[2] for s in steps if s["op"] in ("search", "pages", "count")} == {0, 1, -1}
    assert any(s["thr"] is None for s in steps if s["op"] in ("search", "pages", "count"))
    cursors = [s["cursor"] for s in steps if s["op"] == "pages"] + [c for s in steps if s["op"] == "count" for c in s["cursors"] or [None]]
    assert {c[0] if c else None for c in cursors} >= {None, "start", "rank", "rank_id_minus", "rank_big", "between"}
    assert any(s["op"] == "count" and s["cursors"] and len(s["cursors"]) == 5 for s in steps)
    pages = [s for s in steps if s["op"] == "pages"]
    assert any(s["count_around"] for s in pages)
    assert {s["between"][1]["op"] for s in pages if s["between"]} == {"append", "delete"}
    # a page walk and a count directly after an overwrite, after a growth past the capacity and after a delete
    for p in plans:
        p["after"] = {(a["what"] if a["op"] == "append" else a["op"], b["op"]) for a, b in zip(p["steps"][:-1], p["steps"][1:])}
    for what in ("overwrite", "growth", "delete"):
        for op in ("pages", "count"):
            assert any((what, op) in p["after"] for p in plans), (what, op)
    # the paths beside the copies: in every case a search under the default options (the exact path answers so small an
    # index) before any option is set, and a count behind a keep-2 % mask (the list scan, at the widths it serves)
    for p in plans:
        assert p["steps"][1]["op"] == "search" and p["steps"][1]["opts"] == DEFAULT_OPTS and p["steps"][1]["dense"]
        assert any(s["op"] == "count" and s["mask"].get("kind") == "2" for s in p["steps"])
    # ... at least once on a shard large enough to list the mask's rows, at a width the list scan serves
    def rows_at(p, step):
        n = 0
        for s in p["steps"]:
            if s is step:
                return n
            for a in _flat(s):
                if a["op"] == "append":
                    n = max(n, a["first"] + a["block"]["n"])

    assert any(p["shards"] == 1 and p["d"] in (100, 256, 264) and rows_at(p, s) >= LIST_MIN_ROWS
               for p in plans for s in p["steps"] if s["op"] == "count" and s["mask"].get("kind") == "2")
    # every metric, a handle over three shards, every width
    assert {p["metric"] for p in plans} == {0, 1, 2} and {p["shards"] for p in plans} == {1, 3}
    assert {p["d"] for p in plans} == set(WIDTHS)
    # the fp16 pair forced on an eligible width with the exact path off, during a dense search and during a masked one;
    # the same for the int8 pair -- and a masked one after an overwrite, a growth or an append (the copy is rebuilt or
    # extended, not only built)
    for pair, keys in (("f16", ("f16", "f16m")), ("i8", ("i8", "i8m"))):
        hits = {"dense": set(), "masked": set(), "later": set()}
        for p in plans:
            if pair == "f16" and p["d"] not in F16_WIDTHS:
                continue
            changed = False
            for s in p["steps"][1:]:
                changed = changed or (s["op"] == "append" and s["what"] in ("overwrite", "growth", "end"))
                if s["op"] != "search" or s["opts"]["exact_rows"] != 0 or any(s["opts"][key] != 2 for key in keys):
                    continue
                if s["dense"]:
                    hits["dense"].add(p["shards"])
                if s["mask"]["form"] != "none":
                    hits["masked"].add(p["shards"])
                    if changed:
                        hits["later"].add(p["shards"])
        assert hits["dense"] and hits["masked"] and hits["later"], (pair, hits)
    # The fp16 scale's exponent moves between two forced-fp16 searches, and nothing but the scale can make the library
    # convert the stored rows again: on an eligible width, a dense-or-masked search with the fp16 pair forced and the int8
    # pair off, then directly the row of 3e5 as a NEW id inside a tile the row store already holds (no overwrite resets
    # the copy's watermark, no reallocation drops the copy), then directly two such searches
    def forced_f16(step):
        o = step.get("opts", {})
        return step["op"] == "search" and (o["f16"], o["f16m"], o["i8"], o["i8m"], o["exact_rows"]) == (2, 2, 0, 0, 0)

    rescaled = 0
    for p in plans:
        n = 0
        for i, a in enumerate(p["steps"]):
            if a["op"] == "append":
                if (a["what"] == "bigrow_new" and p["d"] in F16_WIDTHS and a["first"] == n and n % 64 and a["block"]["n"] == 1
                        and forced_f16(p["steps"][i - 1]) and forced_f16(p["steps"][i + 1]) and forced_f16(p["steps"][i + 2])):
                    rescaled += 1
                n = max(n, a["first"] + a["block"]["n"])
            for b in _flat(a)[1:]:
                if b["op"] == "append":
                    n = max(n, b["first"] + b["block"]["n"])
    assert rescaled >= 2, rescaled
    if ties:  # every case holds the crowd, and walks and counts stand at its distance behind no mask and behind masks
        for p in plans:
            at = [i for i, s in enumerate(p["steps"]) if s["op"] == "append" and s["what"] == "crowd"]
            assert len(at) == 1
            rest = p["steps"][at[0] + 1:]
            first, n = p["steps"][at[0]]["first"], p["steps"][at[0]]["block"]["n"]
            walk = rest[0]  # behind no mask, or (odd cases) behind a fresh handle whose run keeps the whole crowd
            assert walk["op"] == "pages" and walk["cursor"] == ("tie", first + n // 2) and walk["thr"] is None
            if p["case"] % 2:
                a0, length = walk["mask"]["range"]
                assert walk["mask"]["form"] == "fresh" and a0 <= first and first + n <= a0 + length
            else:
                assert walk["mask"]["form"] == "none"
            assert any(s["op"] == "count" and s["thr"] and s["thr"][0] == "row" and s["mask"]["form"] == "none" for s in rest)
            assert any(s["op"] in ("pages", "count") for s in rest[2:])  # cursor and count jobs after the redo
