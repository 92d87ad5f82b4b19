"""Host-side mirror of the seam the HIP path plugs into.

`HipVectorIndex` wraps one `tsh_index*` handle (the device-resident copy of an
index's raw-vector column).  `HipVectorBackend.search` has the signature and
result shape of `NghGraphEngine.search`
(/root/reference/lib/src/core/ngh_graph_engine.dart:67-135; result class
:26-40), so `VectorIndexManager` can call it where the reference calls the
graph engine (/root/reference/lib/src/core/vector_index_manager.dart:538-548).
"""
from __future__ import annotations

import ctypes
import math
import weakref
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _ffi
from ._ffi import METRIC_COSINE, METRIC_IP, METRIC_L2  # noqa: F401


@dataclass
class NghSearchResult:
    """ref: core/ngh_graph_engine.dart:26-40 (nodeId, distance, primaryKey)."""
    nodeId: int
    distance: float
    primaryKey: Optional[str] = None


def _f32c(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


class _HipHandle:
    """What the device-resident handles share (`HipMask`, `HipGroups`, `HipAttr`, `HipTags`): `_h`, the library's pointer,
    NULL once closed; `_destroy`, the name of the library's destroy function; `_closed`, what `handle()` says then."""
    _destroy = _closed = ""

    def handle(self):
        """The pointer to pass to the library; ValueError once the handle (or its index) was closed."""
        if not self._h:
            raise ValueError(self._closed)
        return self._h

    def close(self) -> None:
        if self._h:
            getattr(_ffi.lib(), self._destroy)(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

class HipMask(_HipHandle):
    """A WHERE row set that lives on the device (`tsh_mask*`, include/tostore_hip.h): the keep bitmap is uploaded once
    and -- when it is selective -- compacted into the list of kept row ids on the device; searches that pass the
    handle (`HipVectorIndex.search(..., row_mask=handle)`) do no host work on the mask.  The natural row sets are the
    ones that serve many queries in the reference: a WHERE's primary keys mapped through the pk -> nodeId tree
    (/root/reference/lib/src/core/vector_index_manager.dart:1223-1378) and the complement of the tombstones
    (/root/reference/lib/src/core/ngh_page.dart:105-108).  Rows appended after the mask was made are not kept; rows
    deleted later are dropped as always.  Destroy before the index (close / context manager); an index that is closed
    first closes its masks, and a closed mask is refused by every search (ValueError), never taken for "no filter"."""
    _destroy, _closed = "tsh_mask_destroy", "the mask is closed (or its index was)"

    def __init__(self, index: "HipVectorIndex", bits):
        bits = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)
        self._h = ctypes.c_void_p()
        self.index = index
        _ffi.check(_ffi.lib().tsh_mask_create(index._h, bits.ctypes.data_as(_ffi.p_u8), bits.shape[0],
                                              ctypes.byref(self._h)))
        index._live_masks().add(self)

    @classmethod
    def _where(cls, index: "HipVectorIndex", attr: "HipAttr", lo: int, hi: int, negate: bool, with_mask, combine) -> "HipMask":
        """A handle made on the device from one range term over an attribute column (`tsh_mask_create_range`)."""
        ops = {"and": _ffi.TSH_MASK_AND, "or": _ffi.TSH_MASK_OR, _ffi.TSH_MASK_AND: _ffi.TSH_MASK_AND, _ffi.TSH_MASK_OR: _ffi.TSH_MASK_OR}
        if combine not in ops:
            raise ValueError("combine is 'and' or 'or'")
        # (a closed attr or with_mask raises here: NULL would read as "no attr" / "no with")
        a = attr.handle()
        w = with_mask.handle() if with_mask is not None else None
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        self.index = index
        _ffi.check(_ffi.lib().tsh_mask_create_range(index._h, a, int(lo), int(hi), 1 if negate else 0, w, ops[combine],
                                                    ctypes.byref(self._h)))
        index._live_masks().add(self)
        return self

    @classmethod
    def _where_clauses(cls, index: "HipVectorIndex", clauses, with_mask, combine) -> "HipMask":
        """A handle made on the device from a whole clause in one launch (`tsh_mask_create_where`)."""
        ops = {"and": _ffi.TSH_MASK_AND, "or": _ffi.TSH_MASK_OR, _ffi.TSH_MASK_AND: _ffi.TSH_MASK_AND, _ffi.TSH_MASK_OR: _ffi.TSH_MASK_OR}
        if combine not in ops:
            raise ValueError("combine is 'and' or 'or'")
        flat = [(c, t) for c, clause in enumerate(clauses) for t in clause]
        if any(len(clause) == 0 for clause in clauses):
            raise ValueError("an empty clause: every clause is the OR of at least one term")
        terms = (_ffi.TshWhereTerm * max(len(flat), 1))()
        sets = []  # (the IN terms' arrays: alive until the call returns; the library copies them)
        for rec, (c, t) in zip(terms, flat):
            if not isinstance(t, (WhereRange, WhereIn)):
                raise TypeError("a term is a WhereRange or a WhereIn")
            # (a closed attr raises here: NULL would read as "no attr")
            rec.attr = t.attr.handle()
            rec.negate, rec.clause, rec.reserved = (1 if t.negate else 0), c, 0
            if isinstance(t, WhereIn):
                v = np.ascontiguousarray(t.values, dtype=np.int64).reshape(-1)
                sets.append(v)
                rec.kind, rec.n_set = _ffi.TSH_TERM_IN, v.shape[0]
                rec.set = v.ctypes.data_as(_ffi.p_i64) if v.shape[0] else None
            else:
                rec.kind, rec.lo, rec.hi = _ffi.TSH_TERM_RANGE, int(t.lo), int(t.hi)
        w = with_mask.handle() if with_mask is not None else None
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        self.index = index
        _ffi.check(_ffi.lib().tsh_mask_create_where(index._h, ctypes.cast(terms, _ffi.p_void), len(flat), w, ops[combine],
                                                    ctypes.byref(self._h)))
        del sets
        index._live_masks().add(self)
        return self

    @classmethod
    def _tags(cls, index: "HipVectorIndex", tags: "HipTags", values, need, negate: bool, with_mask, combine) -> "HipMask":
        """A handle made on the device from one HAS ANY / HAS ALL term over a tag column (`tsh_mask_create_tags`)."""
        ops = {"and": _ffi.TSH_MASK_AND, "or": _ffi.TSH_MASK_OR, _ffi.TSH_MASK_AND: _ffi.TSH_MASK_AND, _ffi.TSH_MASK_OR: _ffi.TSH_MASK_OR}
        if combine not in ops:
            raise ValueError("combine is 'and' or 'or'")
        if need == "any":
            n = _ffi.TSH_TAGS_ANY
        elif need == "all":
            n = _ffi.TSH_TAGS_ALL
        elif isinstance(need, (int, np.integer)) and not isinstance(need, bool) and need >= 1:
            n = int(need)
        else:
            raise ValueError("need is 'any', 'all' or a count of at least 1")
        # (a closed tags or with_mask raises here: NULL would read as "no tags" / "no with")
        t = tags.handle()
        w = with_mask.handle() if with_mask is not None else None
        v = np.ascontiguousarray(values, dtype=np.int64).reshape(-1)
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        self.index = index
        _ffi.check(_ffi.lib().tsh_mask_create_tags(index._h, t, v.ctypes.data_as(_ffi.p_i64) if v.shape[0] else None, v.shape[0], n,
                                                   1 if negate else 0, w, ops[combine], ctypes.byref(self._h)))
        index._live_masks().add(self)
        return self

    def bits(self, n_bytes: Optional[int] = None) -> np.ndarray:
        """The handle's GLOBAL bitmap as it stands (`tsh_mask_read`): bit i, LSB first, = row id i; uint8, by default
        one bit per row id the index holds now.  Bytes past what the handle knows read 0."""
        if n_bytes is None:
            n_bytes = (int(self.index.size) + 7) // 8  # (size: one past the last row id, a shard handle's base included)
        out = np.zeros(max(int(n_bytes), 0), dtype=np.uint8)
        _ffi.check(_ffi.lib().tsh_mask_read(self.handle(), out.ctypes.data_as(_ffi.p_u8), int(n_bytes)))
        return out

    @property
    def kept(self) -> int:
        n = _ffi.lib().tsh_mask_kept(self.handle())
        if n < 0:
            _ffi.check(int(n))
        return int(n)


class HipGroups(_HipHandle):
    """The group of every row (`tsh_groups*`, include/tostore_hip.h), for `HipVectorIndex.search_grouped`: entry i of
    `group_of` (int32) is the group of GLOBAL row id i -- a document, a video, a product --, at least 0 and below
    `n_groups`, or negative for a row that stands for itself.  Rows beyond the array are ungrouped; `set()` extends or
    overwrites a range, as the append feed does for the rows.  An index that is closed first closes its groups, and a
    closed handle is refused by every search (ValueError)."""
    _destroy, _closed = "tsh_groups_destroy", "the groups handle is closed (or its index was)"

    def __init__(self, index: "HipVectorIndex", group_of, n_groups: int):
        g = np.ascontiguousarray(group_of, dtype=np.int32).reshape(-1)
        self._h = ctypes.c_void_p()
        self.index = index
        self.n_groups = int(n_groups)
        _ffi.check(_ffi.lib().tsh_groups_create(index._h, g.ctypes.data_as(_ffi.p_i32), g.shape[0], self.n_groups,
                                                ctypes.byref(self._h)))
        # the array as the handle holds it: what a sharded caller's host merge looks the groups up in
        # (sharded.merge_candidate_blocks; the library's own collective reads the handle's copy)
        self.group_of = g.copy()
        index._live_masks().add(self)

    def set(self, first_row_id: int, group_of) -> None:
        """Entries [first_row_id, first_row_id + len(group_of)) of the array, extended where it was shorter."""
        g = np.ascontiguousarray(group_of, dtype=np.int32).reshape(-1)
        _ffi.check(_ffi.lib().tsh_groups_set(self.handle(), int(first_row_id), g.shape[0], g.ctypes.data_as(_ffi.p_i32)))
        end = int(first_row_id) + g.shape[0]
        if g.shape[0] and end > self.group_of.shape[0]:
            self.group_of = np.concatenate([self.group_of, np.full(end - self.group_of.shape[0], -1, dtype=np.int32)])
        self.group_of[int(first_row_id):end] = g


ATTR_NULL = _ffi.TSH_ATTR_NULL


@dataclass
class WhereRange:
    """A term of `HipVectorIndex.make_mask_clauses`: keeps the rows whose `attr` is not NULL and for which
    (lo <= value <= hi) != negate.  lo > hi is the empty range."""
    attr: "HipAttr"
    lo: int
    hi: int
    negate: bool = False


@dataclass
class WhereIn:
    """A term of `HipVectorIndex.make_mask_clauses`: keeps the rows whose `attr` is not NULL and for which
    (value in values) != negate.  `values` (int64) come in any order, duplicates allowed, an ATTR_NULL among them is
    ignored; no values: the empty set."""
    attr: "HipAttr"
    values: Sequence[int]
    negate: bool = False


def f64_order_key(a) -> np.ndarray:
    """int64 keys of a double (or datetime-as-double) column for `HipVectorIndex.make_attr`: ordered as Dart's
    double.compareTo orders the values (-0.0 before 0.0, NaN last, every NaN the same key), so a range over the values is
    a range over the keys.  NaNs are made the positive quiet NaN first; with b the value's bits as int64 the key is b
    for b >= 0 and b ^ 0x7FFFFFFFFFFFFFFF below: no key is ATTR_NULL (that would be the bits of -NaN with a full payload)."""
    v = np.array(a, dtype=np.float64, copy=True).reshape(-1)
    nan = np.isnan(v)
    b = v.view(np.int64)
    b[nan] = 0x7FF8000000000000  # the positive quiet NaN's bits
    return np.where(b >= 0, b, b ^ np.int64(0x7FFFFFFFFFFFFFFF))


class HipAttr(_HipHandle):
    """One scalar attribute of every row, kept on the device (`tsh_attr*`, include/tostore_hip.h), for
    `HipVectorIndex.make_mask_where`: entry i of `values` (int64) belongs to GLOBAL row id i; `ATTR_NULL` says the row
    has no value, and rows beyond the array read as NULL.  `set()` extends or overwrites a range, as the append feed does
    for the rows.  Doubles go in by `f64_order_key`.  An index that is closed first closes its attributes, and a closed
    handle is refused (ValueError)."""
    _destroy, _closed = "tsh_attr_destroy", "the attribute handle is closed (or its index was)"

    def __init__(self, index: "HipVectorIndex", values):
        v = np.ascontiguousarray(values, dtype=np.int64).reshape(-1)
        self._h = ctypes.c_void_p()
        self.index = index
        _ffi.check(_ffi.lib().tsh_attr_create(index._h, v.ctypes.data_as(_ffi.p_i64), v.shape[0], ctypes.byref(self._h)))
        index._live_masks().add(self)

    def set(self, first_row_id: int, values) -> None:
        """Entries [first_row_id, first_row_id + len(values)) of the column, extended with NULLs where it was shorter."""
        v = np.ascontiguousarray(values, dtype=np.int64).reshape(-1)
        _ffi.check(_ffi.lib().tsh_attr_set(self.handle(), int(first_row_id), v.shape[0], v.ctypes.data_as(_ffi.p_i64)))


def _tags_csr(lists):
    """(offsets, values), both int64 and contiguous, of a tag column given as a list of iterables (one per row) or as an
    (offsets, values) pair of arrays already."""
    if isinstance(lists, tuple) and len(lists) == 2:
        off = np.ascontiguousarray(lists[0], dtype=np.int64).reshape(-1)
        vals = np.ascontiguousarray(lists[1], dtype=np.int64).reshape(-1)
        if off.shape[0] == 0:
            off = np.zeros(1, dtype=np.int64)
        return off, vals
    rows = [np.asarray(list(r), dtype=np.int64).reshape(-1) for r in lists]
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    if rows:
        np.cumsum([r.shape[0] for r in rows], out=off[1:])
    vals = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    return off, np.ascontiguousarray(vals, dtype=np.int64)


class HipTags(_HipHandle):
    """One array-valued attribute of every row, kept on the device as CSR (`tsh_tags*`, include/tostore_hip.h), for
    `HipVectorIndex.make_mask_tags`: row i holds a SET of int64 values (group ids of an ACL, tags, labels; strings go in
    through a dictionary of the caller's).  `lists` is a list of iterables, one per GLOBAL row id, or an
    `(offsets, values)` pair.  A list that holds `ATTR_NULL` makes the row a NULL row, as a row beyond the column is; an
    empty list is the empty set, not NULL.  `set()` overwrites or extends a range of rows, as the append feed does for the
    rows.  An index that is closed first closes its tag columns, and a closed handle is refused (ValueError)."""
    _destroy, _closed = "tsh_tags_destroy", "the tags handle is closed (or its index was)"

    def __init__(self, index: "HipVectorIndex", lists):
        off, vals = _tags_csr(lists)
        self._h = ctypes.c_void_p()
        self.index = index
        _ffi.check(_ffi.lib().tsh_tags_create(index._h, off.ctypes.data_as(_ffi.p_i64), off.shape[0] - 1,
                                              vals.ctypes.data_as(_ffi.p_i64) if vals.shape[0] else None, ctypes.byref(self._h)))
        index._live_masks().add(self)

    def set(self, first_row_id: int, lists) -> None:
        """Rows [first_row_id, first_row_id + len(lists)) of the column; rows between its old end and first_row_id become
        NULL rows."""
        off, vals = _tags_csr(lists)
        _ffi.check(_ffi.lib().tsh_tags_set(self.handle(), int(first_row_id), off.shape[0] - 1, off.ctypes.data_as(_ffi.p_i64),
                                           vals.ctypes.data_as(_ffi.p_i64) if vals.shape[0] else None))


class HipVectorIndex:
    """Owner of one `tsh_index*`.  Destroy exactly once (close / context manager)."""

    def __init__(self, dim: int, metric: int, capacity_rows: int = 0, n_devices: int = 1,
                 *, shard_device: Optional[int] = None, row_base: int = 0):
        self._h = ctypes.c_void_p()
        L = _ffi.lib()
        if shard_device is None:
            _ffi.check(L.tsh_index_create(dim, metric, capacity_rows, n_devices, ctypes.byref(self._h)))
        else:
            _ffi.check(L.tsh_index_create_shard(dim, metric, capacity_rows, shard_device, row_base,
                                                ctypes.byref(self._h)))
        self.dim, self.metric, self.row_base = dim, metric, row_base

    @classmethod
    def open_ngh(cls, ngh_dir: str, max_entries_per_dir: int = 500, n_devices: int = 1):
        """Cold start from `<index>/ngh` (meta.json + rawvec + graph tombstones) as the reference lays it
        out (/root/reference/lib/src/core/path_manager.dart:275-324).  Returns (index, info dict)."""
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        info = _ffi.TshNghInfo()
        _ffi.check(_ffi.lib().tsh_index_open_ngh(str(ngh_dir).encode(), max_entries_per_dir, n_devices,
                                                 ctypes.byref(self._h), ctypes.byref(info)))
        self.dim, self.metric, self.row_base = info.dimensions, info.metric, 0
        return self, {k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"}

    @classmethod
    def open_ngh_shard(cls, ngh_dir: str, world: int, rank: int, device: int = -1, max_entries_per_dir: int = 500):
        """Cold start of ONE rank's row range [rank * ceil(N / world), ...) of `<index>/ngh` as a shard handle
        (global ids): only the partition files / pages that hold the range are read
        (/root/reference/lib/src/model/ngh_index_meta.dart:480-490).  Returns (index, info dict)."""
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        info = _ffi.TshNghInfo()
        _ffi.check(_ffi.lib().tsh_index_open_ngh_shard(str(ngh_dir).encode(), max_entries_per_dir, device, world, rank,
                                                       ctypes.byref(self._h), ctypes.byref(info)))
        self.dim, self.metric, self.row_base = info.dimensions, info.metric, info.row_base
        return self, {k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"}

    def make_mask(self, bits) -> "HipMask":
        """A device-resident row set for many searches (bit i of `bits`, LSB first, keeps GLOBAL row id i)."""
        return HipMask(self, bits)

    def make_groups(self, group_of, n_groups: int) -> "HipGroups":
        """The rows' groups for search_grouped (entry i of `group_of`: the group of GLOBAL row id i, negative: none)."""
        return HipGroups(self, group_of, n_groups)

    def make_attr(self, values) -> "HipAttr":
        """A scalar attribute column on the device (entry i of `values`, int64: GLOBAL row id i; ATTR_NULL: no value)."""
        return HipAttr(self, values)

    def make_mask_where(self, attr: "HipAttr", lo: int, hi: int, negate: bool = False, with_mask: Optional["HipMask"] = None,
                        combine="and") -> "HipMask":
        """A mask handle made ON the device from one range term: keeps the rows whose attribute is not NULL and for which
        (lo <= value <= hi) != negate, and-ed / or-ed (`combine`) with `with_mask` when one is given.  lo > hi is the
        empty range.  Conjunctions, IN-lists and NOT are chains of calls; close the intermediates.  A snapshot: later
        `attr.set()` calls and appends do not change it."""
        return HipMask._where(self, attr, lo, hi, negate, with_mask, combine)

    def make_mask_clauses(self, clauses, with_mask: Optional["HipMask"] = None, combine="and") -> "HipMask":
        """A mask handle made ON the device from a whole WHERE in one launch (`tsh_mask_create_where`): `clauses` is a list
        of clauses, each a list of `WhereRange` / `WhereIn` terms; a clause is the OR of its terms, the result the AND of
        the clauses, and-ed / or-ed (`combine`) with `with_mask` when one is given.  `tenant = 7 AND ts BETWEEN a AND b AND
        NOT flag = 1` is `[[WhereRange(t, 7, 7)], [WhereRange(ts, a, b)], [WhereRange(f, 1, 1, negate=True)]]`.  At most 32
        terms over 8 attributes and 4096 set values in one call; more is chained through `with_mask`.  A snapshot, as
        `make_mask_where`'s."""
        return HipMask._where_clauses(self, clauses, with_mask, combine)

    def make_tags(self, lists) -> "HipTags":
        """An array-valued attribute column on the device: `lists` is a list of iterables of int64 (entry i: the set of
        GLOBAL row id i; one that holds ATTR_NULL: no value) or an `(offsets, values)` CSR pair."""
        return HipTags(self, lists)

    def make_mask_tags(self, tags: "HipTags", values, need="any", negate: bool = False, with_mask: Optional["HipMask"] = None,
                       combine="and") -> "HipMask":
        """A mask handle made ON the device from one HAS ANY / HAS ALL term (`tsh_mask_create_tags`): keeps the rows whose
        set is not NULL and for which (the row holds at least t distinct values of `values`) != negate -- t is 1 for
        need="any", the number of distinct values for need="all", or the count given -- and-ed / or-ed (`combine`) with
        `with_mask` when one is given.  At most 4096 distinct values; scalar clauses are chained through `with_mask`.  A
        snapshot: later `tags.set()` calls and appends do not change it."""
        return HipMask._tags(self, tags, values, need, negate, with_mask, combine)

    def facets(self, column, keys, row_mask: Optional["HipMask"] = None, kind="values"):
        """Facet counts ON the device (`tsh_attr_facets` / `tsh_tags_facets`): over the rows a search under `row_mask` (None
        or a HipMask) could return, `(counts, other, null, total)` -- counts[j] (int64) for every key as given, the rows
        with a value in no bucket, the rows without a value, and all of them.  `column` is a `HipAttr` -- kind="values":
        the rows whose value == keys[j], keys in any order; kind="edges": keys[j] <= value < keys[j + 1], the last bucket
        open, keys strictly ascending -- or a `HipTags`: the rows whose set holds keys[j].  At most 4096 distinct keys.  The
        column is read as it stands: no snapshot."""
        if not isinstance(column, (HipAttr, HipTags)):
            raise TypeError("column must be a HipAttr or a HipTags")
        ch = column.handle()  # (a closed handle raises here, before the library is called)
        mh = None
        if row_mask is not None:
            if not isinstance(row_mask, HipMask):
                raise TypeError("row_mask must be a HipMask (or None)")
            mh = row_mask.handle()
        if kind not in ("values", "edges"):
            raise ValueError("kind must be 'values' or 'edges'")
        if isinstance(column, HipTags) and kind != "values":
            raise ValueError("a tag column counts by value: kind must be 'values'")
        k = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        counts, rest = np.zeros(k.shape[0], dtype=np.int64), np.zeros(3, dtype=np.int64)
        pk = k.ctypes.data_as(_ffi.p_i64) if k.shape[0] else None
        pc = counts.ctypes.data_as(_ffi.p_i64) if k.shape[0] else None
        pr = rest.ctypes.data_as(_ffi.p_i64)
        if isinstance(column, HipAttr):
            code = _ffi.TSH_FACET_EDGES if kind == "edges" else _ffi.TSH_FACET_VALUES
            _ffi.check(_ffi.lib().tsh_attr_facets(self._h, ch, mh, code, pk, k.shape[0], pc, pr))
        else:
            _ffi.check(_ffi.lib().tsh_tags_facets(self._h, ch, mh, pk, k.shape[0], pc, pr))
        return counts, int(rest[0]), int(rest[1]), int(rest[2])

    def _live_masks(self) -> "weakref.WeakSet":
        """The masks and groups handles made for this index and not yet closed: close() closes them before it destroys
        the index."""
        s = self.__dict__.get("_masks")
        if s is None:
            s = self._masks = weakref.WeakSet()
        return s

    # -- lifetime -----------------------------------------------------------
    def close(self) -> None:
        for m in list(self.__dict__.get("_masks", ())):
            m.close()
        if self._h:
            _ffi.lib().tsh_index_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data feed (mirrors _writeRawVector / deleteBatch) --------------------
    def append(self, first_row_id: int, rows) -> None:
        rows = _f32c(rows)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be n x {self.dim}")
        _ffi.check(_ffi.lib().tsh_index_append(self._h, first_row_id, rows.shape[0],
                                               rows.ctypes.data_as(_ffi.p_f32)))

    def append_device(self, first_row_id: int, n_rows: int, device_ptr: int) -> None:
        _ffi.check(_ffi.lib().tsh_index_append_device(self._h, first_row_id, n_rows,
                                                      ctypes.c_void_p(device_ptr)))

    def set_deleted(self, ids: Sequence[int]) -> None:
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        _ffi.check(_ffi.lib().tsh_index_set_deleted(self._h, ids.ctypes.data_as(_ffi.p_i64), ids.shape[0]))

    def load_rawvec_file(self, path: str, page_size: int, precision: int, first_row_id: int,
                         max_rows: int) -> int:
        out = ctypes.c_int64(0)
        _ffi.check(_ffi.lib().tsh_index_load_rawvec_file(self._h, path.encode(), page_size, precision,
                                                         first_row_id, max_rows, ctypes.byref(out)))
        return out.value

    def pq_encode(self, first_row_id: int, n_rows: int, codebook, subspaces: int, centroids: int = 256) -> np.ndarray:
        """PQ codes (n_rows x subspaces, uint8) of resident rows; mirrors batchPqEncode
        (/root/reference/lib/src/core/compute_tasks.dart:2292-2326)."""
        cb = _f32c(codebook).reshape(-1)
        sub_dim = self.dim // subspaces
        if cb.shape[0] != subspaces * centroids * sub_dim:
            raise ValueError("codebook must hold subspaces*centroids*(dim//subspaces) floats")
        codes = np.empty((n_rows, subspaces), dtype=np.uint8)
        _ffi.check(_ffi.lib().tsh_index_pq_encode(self._h, first_row_id, n_rows, cb.ctypes.data_as(_ffi.p_f32),
                                                  subspaces, centroids, codes.ctypes.data_as(_ffi.p_u8)))
        return codes

    @staticmethod
    def pq_train(samples, subspaces: int, init_index, centroids: int = 256, iterations: int = 10,
                 device: int = 0) -> np.ndarray:
        """Codebook (subspaces x centroids x subDim, float32) from host samples; mirrors the per-sub-space
        trainPqSubspace tasks (/root/reference/lib/src/core/compute_tasks.dart:2135-2266) given the
        initial sample indices the reference draws from Random(42 + m)."""
        s = _f32c(samples)
        if s.ndim != 2:
            raise ValueError("samples must be n x dim")
        n, dim = s.shape
        init = np.ascontiguousarray(init_index, dtype=np.int32)
        if init.size != subspaces * centroids:
            raise ValueError("init_index must hold subspaces*centroids indices")
        out = np.empty((subspaces, centroids, dim // subspaces), dtype=np.float32)
        _ffi.check(_ffi.lib().tsh_pq_train(device, s.ctypes.data_as(_ffi.p_f32), n, dim, subspaces, centroids,
                                           iterations, init.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                           out.ctypes.data_as(_ffi.p_f32)))
        return out

    @property
    def size(self) -> int:
        return _ffi.lib().tsh_index_size(self._h)

    def counters(self) -> dict:
        c = _ffi.TshCounters()
        _ffi.check(_ffi.lib().tsh_get_counters(self._h, ctypes.byref(c)))
        return {k: getattr(c, k) for k, _ in c._fields_}

    # -- search ---------------------------------------------------------------
    def mask_arg(self, row_mask):
        """(array kept alive by the caller, pointer) of a keep mask for the C ABI.  The ABI carries no mask
        length: the library reads ceil(size / 8) bytes (bit i = GLOBAL row id i), so a short buffer is
        rejected here, for every entry point that takes a mask."""
        if row_mask is None:
            return None, None
        row_mask = np.ascontiguousarray(row_mask, dtype=np.uint8).reshape(-1)
        need = (self.size + 7) // 8
        if row_mask.shape[0] < need:
            raise ValueError(f"row_mask needs {need} bytes (one bit per row id below {self.size}), got {row_mask.shape[0]}")
        return row_mask, row_mask.ctypes.data_as(_ffi.p_u8)

    def search(self, queries, k: int, distance_threshold: Optional[float] = None, row_mask=None):
        """Raw C-ABI search: (ids[nq,k], dist[nq,k], count[nq])."""
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"queries must be nq x {self.dim}")
        nq, kk = q.shape[0], max(int(k), 0)
        # (the library fills the slots past a query's count with -1 / NaN itself: pre-filling 1.6 MB here cost a
        # 1024-query call 0.3 ms)
        ids = np.empty((nq, max(kk, 1)), dtype=np.int64)
        dist = np.empty((nq, max(kk, 1)), dtype=np.float64)
        cnt = np.zeros(nq, dtype=np.int32)
        thr = math.nan if distance_threshold is None else float(distance_threshold)
        if isinstance(row_mask, HipMask):  # a mask handle: resident on the device, nothing to prepare
            _ffi.check(_ffi.lib().tsh_search_masked(self._h, q.ctypes.data_as(_ffi.p_f32), nq, int(k), thr, row_mask.handle(),
                                                    ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64),
                                                    cnt.ctypes.data_as(_ffi.p_i32)))
            return ids[:, :kk], dist[:, :kk], cnt
        row_mask, mp = self.mask_arg(row_mask)
        _ffi.check(_ffi.lib().tsh_search(self._h, q.ctypes.data_as(_ffi.p_f32), nq, int(k), thr, mp,
                                         ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64),
                                         cnt.ctypes.data_as(_ffi.p_i32)))
        return ids[:, :kk], dist[:, :kk], cnt

    def search_after(self, queries, k: int, after, distance_threshold: Optional[float] = None, row_mask=None):
        """The next k rows past a cursor: (ids[nq,k], dist[nq,k], count[nq]) like search(), holding for every query the
        first k entries, in the reference's order (distance by double.compareTo, ties by id), that are strictly greater
        than its cursor.  after: one (distance, id) pair for all queries, or (distances[nq], ids[nq]); the last entry of
        the page before continues a list, (-inf, anything) starts one.  A page shorter than k is the last one.
        row_mask: None, a byte mask or a HipMask."""
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"queries must be nq x {self.dim}")
        nq, kk = q.shape[0], max(int(k), 0)
        a_dist = np.ascontiguousarray(np.broadcast_to(np.asarray(after[0], dtype=np.float64).reshape(-1), (nq,)))
        a_id = np.ascontiguousarray(np.broadcast_to(np.asarray(after[1], dtype=np.int64).reshape(-1), (nq,)))
        ids = np.empty((nq, max(kk, 1)), dtype=np.int64)
        dist = np.empty((nq, max(kk, 1)), dtype=np.float64)
        cnt = np.zeros(nq, dtype=np.int32)
        thr = math.nan if distance_threshold is None else float(distance_threshold)
        handle, mp = None, None
        if isinstance(row_mask, HipMask):
            handle = row_mask.handle()
        else:
            row_mask, mp = self.mask_arg(row_mask)
        _ffi.check(_ffi.lib().tsh_search_after(self._h, q.ctypes.data_as(_ffi.p_f32), nq, int(k), thr, mp, handle,
                                               a_dist.ctypes.data_as(_ffi.p_f64), a_id.ctypes.data_as(_ffi.p_i64),
                                               ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64),
                                               cnt.ctypes.data_as(_ffi.p_i32)))
        return ids[:, :kk], dist[:, :kk], cnt

    def search_after_stats(self) -> dict:
        """The cursor searches' counters, per shard search: all of them, rows sent to the side list, searches redone with a
        larger side list, searches answered without a floor pass on the device."""
        out = (ctypes.c_int64 * 4)()
        _ffi.check(_ffi.lib().tsh_search_after_stats(self._h, out))
        return {"searches": out[0], "side_rows": out[1], "redone": out[2], "no_floor": out[3]}

    def search_count(self, queries, distance_threshold: Optional[float] = None, row_mask=None, after=None) -> np.ndarray:
        """How many rows search_after() would return with k = infinity: count[nq] (int64), under the same threshold, mask
        (None, a byte mask or a HipMask), tombstones and cursor.  after: None for the whole list -- search()'s -- or a
        cursor as search_after() takes it; count(after = a page's last entry) is what is left past that page.  One scan
        and a pass over its keys per query: no page is fetched."""
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"queries must be nq x {self.dim}")
        nq = q.shape[0]
        a_dist = a_id = pd = pi = None
        if after is not None:
            a_dist = np.ascontiguousarray(np.broadcast_to(np.asarray(after[0], dtype=np.float64).reshape(-1), (nq,)))
            a_id = np.ascontiguousarray(np.broadcast_to(np.asarray(after[1], dtype=np.int64).reshape(-1), (nq,)))
            pd, pi = a_dist.ctypes.data_as(_ffi.p_f64), a_id.ctypes.data_as(_ffi.p_i64)
        cnt = np.zeros(nq, dtype=np.int64)
        thr = math.nan if distance_threshold is None else float(distance_threshold)
        handle, mp = None, None
        if isinstance(row_mask, HipMask):
            handle = row_mask.handle()
        else:
            row_mask, mp = self.mask_arg(row_mask)
        _ffi.check(_ffi.lib().tsh_search_count(self._h, q.ctypes.data_as(_ffi.p_f32), nq, thr, mp, handle, pd, pi,
                                               cnt.ctypes.data_as(_ffi.p_i64)))
        return cnt

    def search_count_stats(self) -> dict:
        """The counts' counters, per shard search: all of them, rows sent to the side list, counts redone with a larger
        side list, counts answered without a window pass on the device."""
        out = (ctypes.c_int64 * 4)()
        _ffi.check(_ffi.lib().tsh_search_count_stats(self._h, out))
        return {"searches": out[0], "side_rows": out[1], "redone": out[2], "no_window": out[3]}

    def search_grouped(self, queries, k: int, groups: "HipGroups", distance_threshold: Optional[float] = None, row_mask=None):
        """The nearest row of each of the k nearest groups: (ids[nq,k], dist[nq,k], group[nq,k], count[nq]).  The list
        search() would return with k = infinity, every entry dropped whose group occurred earlier in it, cut to k; group
        is -1 for a row that stands for itself.  row_mask: None, a byte mask or a HipMask."""
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"queries must be nq x {self.dim}")
        if not isinstance(groups, HipGroups):
            raise TypeError("groups must be a HipGroups (HipVectorIndex.make_groups)")
        nq, kk = q.shape[0], max(int(k), 0)
        ids = np.empty((nq, max(kk, 1)), dtype=np.int64)
        dist = np.empty((nq, max(kk, 1)), dtype=np.float64)
        grp = np.empty((nq, max(kk, 1)), dtype=np.int32)
        cnt = np.zeros(nq, dtype=np.int32)
        thr = math.nan if distance_threshold is None else float(distance_threshold)
        handle, mp = None, None
        if isinstance(row_mask, HipMask):
            handle = row_mask.handle()
        else:
            row_mask, mp = self.mask_arg(row_mask)
        _ffi.check(_ffi.lib().tsh_search_grouped(self._h, q.ctypes.data_as(_ffi.p_f32), nq, int(k), thr, mp, handle, groups.handle(),
                                                 ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64),
                                                 grp.ctypes.data_as(_ffi.p_i32), cnt.ctypes.data_as(_ffi.p_i32)))
        return ids[:, :kk], dist[:, :kk], grp[:, :kk], cnt

    def search_grouped_stats(self) -> dict:
        """The grouped searches' counters, per shard search: all of them, rows sent to the side list, searches redone with a
        larger side list, searches answered without the group passes on the device (safe mode)."""
        out = (ctypes.c_int64 * 4)()
        _ffi.check(_ffi.lib().tsh_search_grouped_stats(self._h, out))
        return {"searches": out[0], "side_rows": out[1], "redone": out[2], "no_device_passes": out[3]}

    def search_grouped_after(self, queries, k: int, groups: "HipGroups", after, distance_threshold: Optional[float] = None, row_mask=None):
        """The next k groups past a cursor: (ids[nq,k], dist[nq,k], group[nq,k], count[nq]) like search_grouped(), holding
        the first k entries of the grouped list that are strictly greater than the cursor.  A group whose best row is at
        or before the cursor is consumed: none of its rows comes back.  after: as search_after() takes it; the last entry
        of the page before continues the list, (-inf, anything) starts it -- search_grouped()'s answer.  A page shorter
        than k is the last one.  row_mask: None, a byte mask or a HipMask."""
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"queries must be nq x {self.dim}")
        if not isinstance(groups, HipGroups):
            raise TypeError("groups must be a HipGroups (HipVectorIndex.make_groups)")
        nq, kk = q.shape[0], max(int(k), 0)
        a_dist = np.ascontiguousarray(np.broadcast_to(np.asarray(after[0], dtype=np.float64).reshape(-1), (nq,)))
        a_id = np.ascontiguousarray(np.broadcast_to(np.asarray(after[1], dtype=np.int64).reshape(-1), (nq,)))
        ids = np.empty((nq, max(kk, 1)), dtype=np.int64)
        dist = np.empty((nq, max(kk, 1)), dtype=np.float64)
        grp = np.empty((nq, max(kk, 1)), dtype=np.int32)
        cnt = np.zeros(nq, dtype=np.int32)
        thr = math.nan if distance_threshold is None else float(distance_threshold)
        handle, mp = None, None
        if isinstance(row_mask, HipMask):
            handle = row_mask.handle()
        else:
            row_mask, mp = self.mask_arg(row_mask)
        _ffi.check(_ffi.lib().tsh_search_grouped_after(self._h, q.ctypes.data_as(_ffi.p_f32), nq, int(k), thr, mp, handle, groups.handle(),
                                                       a_dist.ctypes.data_as(_ffi.p_f64), a_id.ctypes.data_as(_ffi.p_i64),
                                                       ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64),
                                                       grp.ctypes.data_as(_ffi.p_i32), cnt.ctypes.data_as(_ffi.p_i32)))
        return ids[:, :kk], dist[:, :kk], grp[:, :kk], cnt

    def count_groups(self, queries, groups: "HipGroups", distance_threshold: Optional[float] = None, row_mask=None, after=None) -> np.ndarray:
        """How many entries search_grouped_after() would return with k = infinity: count[nq] (int64), under the same
        threshold, mask, tombstones and cursor.  after: None for the whole grouped list, or a cursor; count(after = a page's
        last entry) is count(None) minus the entries returned so far."""
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"queries must be nq x {self.dim}")
        if not isinstance(groups, HipGroups):
            raise TypeError("groups must be a HipGroups (HipVectorIndex.make_groups)")
        nq = q.shape[0]
        a_dist = a_id = pd = pi = None
        if after is not None:
            a_dist = np.ascontiguousarray(np.broadcast_to(np.asarray(after[0], dtype=np.float64).reshape(-1), (nq,)))
            a_id = np.ascontiguousarray(np.broadcast_to(np.asarray(after[1], dtype=np.int64).reshape(-1), (nq,)))
            pd, pi = a_dist.ctypes.data_as(_ffi.p_f64), a_id.ctypes.data_as(_ffi.p_i64)
        cnt = np.zeros(nq, dtype=np.int64)
        thr = math.nan if distance_threshold is None else float(distance_threshold)
        handle, mp = None, None
        if isinstance(row_mask, HipMask):
            handle = row_mask.handle()
        else:
            row_mask, mp = self.mask_arg(row_mask)
        _ffi.check(_ffi.lib().tsh_search_grouped_count(self._h, q.ctypes.data_as(_ffi.p_f32), nq, thr, mp, handle, groups.handle(), pd, pi,
                                                       cnt.ctypes.data_as(_ffi.p_i64)))
        return cnt

    def search_grouped_after_stats(self) -> dict:
        """The grouped cursor searches' and group counts' counters, per shard job: the searches, the counts, rows sent to the
        side list, jobs redone with a larger side list, jobs answered by the exact-all route."""
        out = (ctypes.c_int64 * 5)()
        _ffi.check(_ffi.lib().tsh_search_grouped_after_stats(self._h, out))
        return {"searches": out[0], "counts": out[1], "side_rows": out[2], "redone": out[3], "exact_all": out[4]}

    def search_grouped_rows(self, queries, k: int, rows_per_group: int, groups: "HipGroups", distance_threshold: Optional[float] = None,
                            row_mask=None):
        """The rows_per_group nearest rows of each of the k nearest groups: (ids[nq,k,m], dist[nq,k,m], group[nq,k],
        rows[nq,k], count[nq]).  The winning groups are search_grouped()'s, in its order; of each the first m entries of
        the list search() would return with k = infinity, in that list's order.  Unused slots read id -1 and distance NaN,
        an unused group -1 and 0 rows.  rows_per_group: 1 to 64.  row_mask: None, a byte mask or a HipMask."""
        q = _f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"queries must be nq x {self.dim}")
        if not isinstance(groups, HipGroups):
            raise TypeError("groups must be a HipGroups (HipVectorIndex.make_groups)")
        nq, kk, mm = q.shape[0], max(int(k), 0), max(int(rows_per_group), 0)
        ids = np.empty((nq, max(kk, 1), max(mm, 1)), dtype=np.int64)
        dist = np.empty((nq, max(kk, 1), max(mm, 1)), dtype=np.float64)
        grp = np.empty((nq, max(kk, 1)), dtype=np.int32)
        rows = np.empty((nq, max(kk, 1)), dtype=np.int32)
        cnt = np.zeros(nq, dtype=np.int32)
        thr = math.nan if distance_threshold is None else float(distance_threshold)
        handle, mp = None, None
        if isinstance(row_mask, HipMask):
            handle = row_mask.handle()
        else:
            row_mask, mp = self.mask_arg(row_mask)
        # (the C entry lays slot (q, i, j) at (q k + i) m + j: the arrays above have that shape only for k, m >= 1 -- a
        # trivial call writes no slot)
        _ffi.check(_ffi.lib().tsh_search_grouped_rows(self._h, q.ctypes.data_as(_ffi.p_f32), nq, int(k), int(rows_per_group), thr, mp, handle,
                                                      groups.handle(), ids.ctypes.data_as(_ffi.p_i64), dist.ctypes.data_as(_ffi.p_f64),
                                                      grp.ctypes.data_as(_ffi.p_i32), rows.ctypes.data_as(_ffi.p_i32),
                                                      cnt.ctypes.data_as(_ffi.p_i32)))
        return ids[:, :kk, :mm], dist[:, :kk, :mm], grp[:, :kk], rows[:, :kk], cnt

    def search_grouped_rows_stats(self) -> dict:
        """The rows-per-group searches' counters, per shard job: the searches, groups their mark passes marked, member rows
        sent on for exact sums, jobs redone with larger lists, jobs answered by the exact-all route."""
        out = (ctypes.c_int64 * 5)()
        _ffi.check(_ffi.lib().tsh_search_grouped_rows_stats(self._h, out))
        return {"searches": out[0], "marked_groups": out[1], "member_rows": out[2], "redone": out[3], "exact_all": out[4]}

    # -- asynchronous single-query form (several queries in flight) -----------------
    def submit(self, query, k: int, row_mask=None, after=None) -> tuple:
        """after: a (distance, id) cursor -- the ticket answers search_after() instead of search()."""
        q = _f32c(query).reshape(-1)
        if q.shape[0] != self.dim:
            raise ValueError(f"query must have {self.dim} elements")
        t = ctypes.c_int32(-1)
        if after is not None:
            handle, mp = None, None
            if isinstance(row_mask, HipMask):
                handle = row_mask.handle()
            else:
                row_mask, mp = self.mask_arg(row_mask)
            _ffi.check(_ffi.lib().tsh_search_submit_after(self._h, q.ctypes.data_as(_ffi.p_f32), int(k), mp, handle,
                                                          float(after[0]), int(after[1]), ctypes.byref(t)))
            return (t.value, int(k))
        if isinstance(row_mask, HipMask):
            _ffi.check(_ffi.lib().tsh_search_submit_masked(self._h, q.ctypes.data_as(_ffi.p_f32), int(k), row_mask.handle(),
                                                           ctypes.byref(t)))
            return (t.value, int(k))
        row_mask, mp = self.mask_arg(row_mask)
        _ffi.check(_ffi.lib().tsh_search_submit(self._h, q.ctypes.data_as(_ffi.p_f32), int(k), mp,
                                                ctypes.byref(t)))
        return (t.value, int(k))

    def ready(self, ticket: tuple) -> bool:
        """True once the ticket's kernels have finished (wait() will not block on the GPU).  Never blocks."""
        rc = _ffi.lib().tsh_search_ready(self._h, ticket[0])
        if rc < 0:
            _ffi.check(rc)
        return rc == 1

    def wait(self, ticket: tuple, distance_threshold: Optional[float] = None):
        t, k = ticket
        ids = np.empty(k, dtype=np.int64)
        dist = np.empty(k, dtype=np.float64)
        cnt = ctypes.c_int32(0)
        thr = math.nan if distance_threshold is None else float(distance_threshold)
        _ffi.check(_ffi.lib().tsh_search_wait(self._h, t, thr, ids.ctypes.data_as(_ffi.p_i64),
                                              dist.ctypes.data_as(_ffi.p_f64), ctypes.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value]

    def set_batch_min_nq(self, nq: int) -> None:
        """When search() uses the batched matrix-core path: 0 never, 1 by estimated cost (default), n >= 2 from n
        queries per call on.  Results are identical."""
        _ffi.check(_ffi.lib().tsh_index_set_option(self._h, _ffi.TSH_OPT_BATCH_MIN_NQ, int(nq)))

    def set_scan_f16(self, mode: int) -> None:
        """Dense single-query scans over the fp16 copy of the rows (half the HBM bytes): 0 never, 1 auto (default: shards
        whose row store is larger than 256 MiB), 2 every eligible scan whatever the size.  Results are identical."""
        _ffi.check(_ffi.lib().tsh_index_set_option(self._h, _ffi.TSH_OPT_SCAN_F16, int(mode)))

    def set_scan_f16_masked(self, mode: int) -> None:
        """The same for tile scans behind a row mask, tombstones, quarantined rows or gaps of absent ids: 0 never, 1 auto
        (default: shards whose row store is larger than 256 MiB), 2 every eligible masked scan whatever the size.
        set_scan_f16(0) switches both off.  Results are identical."""
        _ffi.check(_ffi.lib().tsh_index_set_option(self._h, _ffi.TSH_OPT_SCAN_F16_MASKED, int(mode)))

    def scan_f16_stats(self) -> dict:
        """The fp16 scan's counters: scans launched, queries redone through the f32 scan, rows converted, copy bytes."""
        out = (ctypes.c_int64 * 4)()
        _ffi.check(_ffi.lib().tsh_scan_f16_stats(self._h, out))
        return {"scans": out[0], "redone": out[1], "rows_converted": out[2], "copy_bytes": out[3]}

    def probe_scan_f16_keys(self, query):
        """(stored upper-side key of every row from the fp16 scan kernel, every row's band w): tests of the error model."""
        q = _f32c(query).reshape(-1)
        keys = np.empty(self.size - self.row_base, dtype=np.float32)
        w = np.empty(self.size - self.row_base, dtype=np.float32)
        _ffi.check(_ffi.lib().tsh_probe_scan_f16_keys(self._h, q.ctypes.data_as(_ffi.p_f32), keys.ctypes.data_as(_ffi.p_f32),
                                                      w.ctypes.data_as(_ffi.p_f32)))
        return keys, w

    def set_scan_i8(self, mode: int) -> None:
        """Dense, all-live single-query scans as a coarse pass over the int8 copy of the rows (a quarter of the HBM bytes)
        whose survivors the exact scan + select answer: 0 never, 1 auto (default: shards whose row store is larger
        than 256 MiB), 2 every eligible scan whatever the size.  Results are identical."""
        _ffi.check(_ffi.lib().tsh_index_set_option(self._h, _ffi.TSH_OPT_SCAN_I8, int(mode)))

    def set_scan_i8_masked(self, mode: int) -> None:
        """The same coarse int8 pass for tile scans behind a row mask, tombstones, quarantined rows or gaps of absent ids:
        0 never, 1 auto (default: shards whose row store is larger than 256 MiB, unless set_scan_f16_masked(2) forced the
        fp16 masked route), 2 every eligible masked scan whatever the size.  set_scan_i8(0) switches both off;
        set_scan_i8(2) does not force this one.  Results are identical."""
        _ffi.check(_ffi.lib().tsh_index_set_option(self._h, _ffi.TSH_OPT_SCAN_I8_MASKED, int(mode)))

    def set_scan_i4(self, mode: int) -> None:
        """A 4-bit first pass in front of the dense L2 int8 scan (half a byte per element; the int8 scan then reads only the
        rows it could not rule out): 0 never, 1 auto (default: L2 shards whose row store is larger than 1400 MiB), 2 every
        eligible scan whatever the size.  Denied for a while when too many rows survive it.  Results are identical."""
        _ffi.check(_ffi.lib().tsh_index_set_option(self._h, _ffi.TSH_OPT_SCAN_I4, int(mode)))

    def scan_i4_stats(self) -> dict:
        """The 4-bit pass's counters: scans it ran in, rows it left to the int8 scan, rows converted, plane bytes, times
        the route was denied, eligible scans a denial still covers."""
        out = (ctypes.c_int64 * 6)()
        _ffi.check(_ffi.lib().tsh_scan_i4_stats(self._h, out))
        return {"scans": out[0], "survivors": out[1], "rows_converted": out[2], "copy_bytes": out[3], "denials": out[4],
                "denied_left": out[5]}

    def probe_scan_i4_keys(self, query):
        """(lower side, upper side) of every row's key from the 4-bit scan kernel: tests of the error model."""
        q = _f32c(query).reshape(-1)
        lo = np.empty(self.size - self.row_base, dtype=np.float32)
        up = np.empty(self.size - self.row_base, dtype=np.float32)
        _ffi.check(_ffi.lib().tsh_probe_scan_i4_keys(self._h, q.ctypes.data_as(_ffi.p_f32), lo.ctypes.data_as(_ffi.p_f32),
                                                     up.ctypes.data_as(_ffi.p_f32)))
        return lo, up

    def set_scan_streams(self, mode: int) -> None:
        """On how many streams the scans of overlapping single queries run: 0 by the scan's drain share (default: two for
        scans of fewer than 6144 tiles and for a big shard's scans over its int8 or fp16 copy), 1 always one, 2 two
        whenever queries overlap.  On two streams a sampled scan's own duration (counters()["scan_us_sum"]) is about
        twice its share of the HBM time.  Results are identical."""
        _ffi.check(_ffi.lib().tsh_index_set_option(self._h, _ffi.TSH_OPT_SCAN_STREAMS, int(mode)))

    def scan_i8_stats(self) -> dict:
        """The int8 scan's counters: scans launched (dense and masked), queries redone through another scan, rows converted,
        copy bytes."""
        out = (ctypes.c_int64 * 4)()
        _ffi.check(_ffi.lib().tsh_scan_i8_stats(self._h, out))
        return {"scans": out[0], "redone": out[1], "rows_converted": out[2], "copy_bytes": out[3]}

    def probe_scan_i8_keys(self, query):
        """(lower side, upper side) of every row's key from the int8 scan kernel: tests of the error model."""
        q = _f32c(query).reshape(-1)
        lo = np.empty(self.size - self.row_base, dtype=np.float32)
        up = np.empty(self.size - self.row_base, dtype=np.float32)
        _ffi.check(_ffi.lib().tsh_probe_scan_i8_keys(self._h, q.ctypes.data_as(_ffi.p_f32), lo.ctypes.data_as(_ffi.p_f32),
                                                     up.ctypes.data_as(_ffi.p_f32)))
        return lo, up

    def set_exact_scan_rows(self, rows: int) -> None:
        """Single-query searches with at most `rows` rows to look at (a selective mask's kept rows, a small index) take
        the exact sums of all of them and select among the exact distances (two dispatches, no f32 pre-filter):
        0 never, default and maximum 16384.  Results are identical."""
        _ffi.check(_ffi.lib().tsh_index_set_option(self._h, _ffi.TSH_OPT_EXACT_SCAN_ROWS, int(rows)))

    def set_exact_select(self, wide: bool) -> None:
        """What follows the exact scan of a short search: True (default) the wide pick (one workgroup per 256 rows, the
        cut from the scan's key histogram, k rows plus the cut bin's few others), False the one-workgroup select that
        ranks exactly k rows.  Results are identical."""
        _ffi.check(_ffi.lib().tsh_index_set_option(self._h, _ffi.TSH_OPT_EXACT_SELECT, 1 if wide else 0))

    def set_batch_hub(self, on: bool) -> None:
        """Batched searches (fp16 keys, L2 / inner product) also bound the k-th key by the index's hub rows -- the 4096
        shortest (L2) / longest (inner product) -- beside the sample's estimate (default off: it pays for itself on no corpus measured).  Results are identical."""
        _ffi.check(_ffi.lib().tsh_index_set_option(self._h, _ffi.TSH_OPT_BATCH_HUB, 1 if on else 0))

    def set_batch_group(self, on: bool) -> None:
        """The fp16 copy of an L2 / inner-product index holds its rows by norm inside blocks of 8192 (default on) or in
        row order.  Results are identical; the copy is rebuilt by the next batched search."""
        _ffi.check(_ffi.lib().tsh_index_set_option(self._h, _ffi.TSH_OPT_BATCH_GROUP, 1 if on else 0))

    def set_batch_kernel(self, kind: int) -> None:
        """Batched pre-filter keys: 0 f32 MFMA, 1 bf16x3, 2 f16, 3 auto (default: f16, but bf16x3 for an L2
        index whose norms spread too far or whose fp16 candidate lists kept overflowing).  Results are identical."""
        _ffi.check(_ffi.lib().tsh_index_set_option(self._h, _ffi.TSH_OPT_BATCH_KERNEL, int(kind)))

    def bench_batch(self, queries, k: int, iters: int = 3):
        """(avg microseconds of the matrix-core passes, algorithmic flops) for one batch."""
        q = _f32c(queries)
        us, fl = ctypes.c_double(0), ctypes.c_double(0)
        _ffi.check(_ffi.lib().tsh_bench_batch(self._h, q.ctypes.data_as(_ffi.p_f32), q.shape[0], int(k), iters,
                                              ctypes.byref(us), ctypes.byref(fl)))
        return us.value, fl.value

    def probe_scan_keys(self, query):
        """(f32 key of every row from the scan kernel, eps_rel, delta_abs): tests of the error model."""
        q = _f32c(query).reshape(-1)
        keys = np.empty(self.size - self.row_base, dtype=np.float32)
        er, da = ctypes.c_float(0), ctypes.c_float(0)
        _ffi.check(_ffi.lib().tsh_probe_scan_keys(self._h, q.ctypes.data_as(_ffi.p_f32), keys.ctypes.data_as(_ffi.p_f32),
                                                  ctypes.byref(er), ctypes.byref(da)))
        return keys, er.value, da.value

    def probe_batch_keys(self, queries, k: int):
        """(keys[nq, rows] of the batched key kernel in use, delta2[nq]): tests of the error model."""
        q = _f32c(queries)
        keys = np.empty((q.shape[0], self.size - self.row_base), dtype=np.float32)
        d2 = np.empty(q.shape[0], dtype=np.float32)
        _ffi.check(_ffi.lib().tsh_probe_batch_keys(self._h, q.ctypes.data_as(_ffi.p_f32), q.shape[0], int(k),
                                                   keys.ctypes.data_as(_ffi.p_f32), d2.ctypes.data_as(_ffi.p_f32)))
        return keys, d2

    def probe_batch_row_band(self, nq: int):
        """(alpha2[nq], beta2[nq]) of the last probe_batch_keys call: 2 |key - exact| <= alpha2 |v| + beta2 per row."""
        a2 = np.empty(nq, dtype=np.float32)
        b2 = np.empty(nq, dtype=np.float32)
        _ffi.check(_ffi.lib().tsh_probe_batch_row_band(self._h, int(nq), a2.ctypes.data_as(_ffi.p_f32),
                                                       b2.ctypes.data_as(_ffi.p_f32)))
        return a2, b2

    def bench_scan(self, query, iters: int = 20, row_mask=None) -> float:
        q = _f32c(query)
        out = ctypes.c_double(0)
        row_mask, mp = self.mask_arg(row_mask)
        _ffi.check(_ffi.lib().tsh_bench_scan(self._h, q.ctypes.data_as(_ffi.p_f32), iters, mp,
                                             ctypes.byref(out)))
        return out.value


class HipVectorBackend:
    """Drop-in for `NghGraphEngine.search` backed by a `HipVectorIndex`.

    ref: core/ngh_graph_engine.dart:67-135.  The scan is exhaustive (ef -> infinity), so by default `efSearch`
    changes nothing and the k=100 / default-ef trap of :80-82,168 (at most 64 rows returned) does not exist here.
    `honourEfCap=True` (the hook's `hipHonourEfCap`, tostore_amd/dart/hip_vector_hook.dart) brings the reference's
    row COUNT back for callers that depend on it: the answer is cut to `min(topK, ef)` rows with
    `ef = min(efSearch ?? metaEfSearch, max(5 topK, 32))` (:80-82; the result heap holds ef entries, :168), and an
    index whose graph has no entry point (`medoidNodeId < 0`, :78) answers nothing.  The rows are still the exact
    nearest ones -- which the reference's own ef rows need not be.
    """

    def __init__(self, index: HipVectorIndex, *, honourEfCap: bool = False, metaEfSearch: int = 64,
                 medoidNodeId: int = 0):
        self.index = index
        self.honourEfCap = honourEfCap
        self.metaEfSearch = metaEfSearch  # NghIndexMeta.efSearch (model/ngh_index_meta.dart:196: default 64)
        self.medoidNodeId = medoidNodeId  # NghIndexMeta.medoidNodeId (-1 until the first insert picked one)

    def search(self, *, query, topK: int, efSearch: Optional[int] = None,
               distanceThreshold: Optional[float] = None, rowMask=None, after=None) -> list:
        """after: a (distance, nodeId) cursor -- the answer is the next topK rows past it (HipVectorIndex.search_after)."""
        # ref: :78  `if (meta.totalVectors == 0 || meta.medoidNodeId < 0) return const []`
        if self.index.size == 0 or topK <= 0:
            return []
        if self.honourEfCap:
            if self.medoidNodeId < 0:
                return []
            ef = min(self.metaEfSearch if efSearch is None else efSearch, max(topK * 5, 32))  # :80-82
            topK = min(topK, max(ef, 0))
            if topK <= 0:
                return []
        if after is not None:
            ids, dist, cnt = self.index.search_after(query, topK, after, distanceThreshold, rowMask)
        else:
            ids, dist, cnt = self.index.search(query, topK, distanceThreshold, rowMask)
        n = int(cnt[0])
        return [NghSearchResult(nodeId=int(ids[0, i]), distance=float(dist[0, i])) for i in range(n)]
