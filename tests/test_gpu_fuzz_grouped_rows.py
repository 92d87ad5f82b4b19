"""GPU: random sequences of appends, deletes, tsh_groups_set and rows-per-group searches on one index and one groups
handle, every search held to the oracle (search_exhaustive, then the specification in Python) under a random mask,
threshold, k and m.  Some 200 steps over three seeds (one per metric) on at most 3000 rows; the state the oracle needs --
rows, tombstones, the group array -- is kept beside the index."""
import numpy as np
import pytest

from test_gpu_search_grouped_rows import _same, _spec

pytestmark = pytest.mark.gpu

MAX_ROWS = 3000


def _set(group_of, first, g):
    """What tsh_groups_set does to the array: extended with "ungrouped" where it was shorter, then overwritten"""
    if first + len(g) > len(group_of):
        group_of = np.concatenate([group_of, np.full(first + len(g) - len(group_of), -1, np.int32)])
    group_of[first:first + len(g)] = g
    return group_of


@pytest.mark.parametrize("seed,metric,d", [(1, 0, 24), (2, 1, 257), (3, 2, 8)])
def test_fuzz_grouped_rows_sequences(hip_lib, oracle_mod, seed, metric, d):
    from tostore_amd import HipMask, HipVectorIndex

    rng = np.random.default_rng(9500 + seed)
    n_groups = 400
    rows = np.zeros((0, d), np.float32)
    alive = np.zeros(0, bool)
    group_of = np.zeros(0, np.int32)  # the handle's array: may be shorter than the rows (ungrouped beyond it)
    centres = rng.standard_normal((n_groups, d)).astype(np.float32)
    searches = 0
    with HipVectorIndex(d, metric) as idx, idx.make_groups(group_of, n_groups) as h:
        for step in range(70):
            n = len(rows)
            what = rng.choice(["append", "delete", "set", "search", "search", "search"]) if n else "append"
            if what == "append" and n < MAX_ROWS:
                m = int(rng.integers(1, 400))
                m = min(m, MAX_ROWS - n)
                # documents: runs of rows around a common centre, so a near group has many near rows; some exact duplicates
                g = np.repeat(rng.integers(0, n_groups, m), rng.integers(1, 9))[:m].astype(np.int32)
                block = (centres[g] + 0.1 * rng.standard_normal((m, d))).astype(np.float32)
                dup = rng.random(m) < 0.1
                block[dup] = centres[g[dup]]
                idx.append(n, block)
                rows = np.concatenate([rows, block])
                alive = np.concatenate([alive, np.ones(m, bool)])
                if rng.random() < 0.7:  # the feed's companion: the new rows' groups (else they stay ungrouped for a while)
                    g[rng.random(m) < 0.1] = -1
                    h.set(n, g)
                    group_of = _set(group_of, n, g)
            elif what == "delete":
                ids = rng.choice(n, int(rng.integers(1, max(n // 10, 2))), replace=False)
                idx.set_deleted(ids.astype(np.int64))
                alive[ids] = False
            elif what == "set" and len(group_of):
                a = int(rng.integers(0, len(group_of)))
                m = int(rng.integers(1, 200))
                g = rng.integers(-1, n_groups, m).astype(np.int32)
                if rng.random() < 0.5:
                    g[:] = g[0]  # a whole range becomes one group
                h.set(a, g)
                group_of = _set(group_of, a, g)
            if what != "search" and rng.random() < 0.5:
                continue
            n = len(rows)
            q = (centres[rng.integers(0, n_groups)] + 0.3 * rng.standard_normal(d)).astype(np.float32)
            if metric == 2:
                q = oracle_mod.normalize_f32(q)
            keep = alive.copy()
            mask = None
            kind = rng.choice(["none", "half", "few", "handle"])
            if kind != "none":
                sel = rng.random(n) < (0.01 if kind == "few" else 0.5)
                keep &= sel
                mask = np.packbits(sel, bitorder="little")
            full = oracle_mod.search_exhaustive(rows, q, metric, n, None, np.packbits(keep, bitorder="little"))
            k = int(rng.choice([1, 3, 10, 100, 450]))
            m = int(rng.choice([1, 2, 3, 7, 64]))
            thr = None
            if len(full[0]) and rng.random() < 0.5:
                dk = float(full[1][min(int(rng.integers(0, 4 * k)), len(full[0]) - 1)])
                thr = float(rng.choice([dk, np.nextafter(dk, -np.inf), np.nextafter(dk, np.inf)]))
                full = oracle_mod.search_exhaustive(rows, q, metric, n, thr, np.packbits(keep, bitorder="little"))
            want = _spec(full, group_of, k, m)
            if kind == "handle":
                with HipMask(idx, mask) as mh:
                    got = idx.search_grouped_rows(q, k, m, h, thr, mh)
            else:
                got = idx.search_grouped_rows(q, k, m, h, thr, mask)
            _same(got, want, (seed, step, what, kind, k, m, thr, n))
            searches += 1
        assert searches >= 30
        s = idx.search_grouped_rows_stats()
        assert s["searches"] == searches and idx.search_grouped_stats()["searches"] == 0
