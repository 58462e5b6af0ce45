"""Metadata as typed columns in HBM, and filters compiled to a program the device runs over them (include/fvdb.h,
"metadata columns").

Three parts:
  * the encoder: the value a dotted path reaches in one row's metadata (`metadata_filter.get_field` itself) becomes a
    tag and an eight-byte payload, an array additionally a list of element tags and payloads;
  * the compiler: a `MetadataFilter` becomes a postfix program over three-valued results, or None when it exceeds the
    engine's limits;
  * `MetadataColumns`: one `fvdb_meta` table, a column per path the first time a filter names it, and
    `evaluate(flt, metadata)` -> the uint64 ids of the matching rows in slot order, exactly the array
    `[rid for rid in rows if name in metadata and flt.matches(metadata[name])]`.

What the device cannot decide (a value tagged COMPLEX: an object compared whole, a nested list, an integer outside
int64, a value of any type that is not exactly None / bool / int / float / str / list / dict) it reports as "unknown"
for that slot, and `evaluate` decides those slots with `flt.matches` and merges them in.  So the result is exact
whatever the metadata hold; COMPLEX only costs host time.
"""
import ctypes as C
import struct
import time

import numpy as np

from . import _capi
from ._capi import u32p, u64p, u8p
from .metadata_filter import _MISSING, get_field

MISSING, NULL, BOOL, INT, FLOAT, STRING, ARRAY, COMPLEX, NEVER = 0, 1, 2, 3, 4, 5, 6, 7, 15  # FVDB_META_*
OP_EQUALS, OP_IN, OP_RANGE, OP_AND, OP_OR = 1, 2, 3, 4, 5                                   # FVDB_META_OP_*
IN_HAS_COMPLEX, IN_HAS_ANY = 1, 2
RANGE_HAS_MIN, RANGE_MIN_INCLUSIVE, RANGE_HAS_MAX, RANGE_MAX_INCLUSIVE = 1, 2, 4, 8
MAX_PROGRAM, MAX_STACK, MAX_CONSTS = 1024, 16, 65536                                         # FVDB_META_MAX_*
_AND_OR_CHUNK = 8  # operands folded per AND / OR instruction: keeps a wide combinator shallow on the stack
_M64 = (1 << 64) - 1
_SIGN = 1 << 63


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- the encoder ------------------------------------------------------------------------------------------------------
def encode_scalar(v, strings, intern):
    """(tag, payload) of a value that is not a list.  `strings`: the table's dictionary (str -> dense code); a string
    it does not hold is given the next code when `intern`, else it is NEVER (a constant that equals nothing)."""
    t = type(v)
    if v is None:
        return NULL, 0
    if t is bool:
        return BOOL, int(v)
    if t is int:
        return (INT, v & _M64) if -_SIGN <= v < _SIGN else (COMPLEX, 0)
    if t is float:
        return FLOAT, f64_bits(v)
    if t is str:
        code = strings.get(v)
        if code is None:
            if not intern:
                return NEVER, 0
            code = strings[v] = len(strings)
        return STRING, code
    return COMPLEX, 0  # an object compared whole, a nested list, any other Python type


def encode_value(v, strings):
    """(tag, payload, elements) of the value a path reached: `elements` is None, or for an ARRAY the list of its
    elements' (tag, payload) — a nested list or object is a COMPLEX element."""
    if v is _MISSING:
        return MISSING, 0, None
    if type(v) is list:
        return ARRAY, len(v), [encode_scalar(x, strings, True) for x in v]
    tag, payload = encode_scalar(v, strings, True)
    return tag, payload, None


def encode_cell(metadata, path, strings):
    return encode_value(get_field(metadata, path), strings)


def ordered_key(tag, payload):
    """The key constants and cells of one tag are compared by (include/fvdb.h): equal keys <=> equal values, key order =
    value order.  None for a FLOAT NaN, which equals nothing."""
    if tag == INT:
        return payload ^ _SIGN
    if tag == FLOAT:
        if (payload << 1) & _M64 == 0:
            payload = 0
        if payload & (_SIGN - 1) > 0x7FF0000000000000:
            return None
        return (~payload & _M64) if payload >> 63 else (payload | _SIGN)
    return payload if tag in (BOOL, STRING) else 0


def encode_constant(c, strings):
    """(tag, key) of a filter constant: COMPLEX for one only the host can compare (a list, an object, a wide integer),
    NEVER for one that equals no cell."""
    if type(c) is list:
        return COMPLEX, 0
    tag, payload = encode_scalar(c, strings, False)
    if tag in (COMPLEX, NEVER):
        return tag, 0
    key = ordered_key(tag, payload)
    return (NEVER, 0) if key is None else (tag, key)


# ---- the compiler -----------------------------------------------------------------------------------------------------
class Program:
    """instrs [n][4] uint32, const_tags [c] uint32, const_keys [c] uint64, depth = the deepest the stack gets."""

    def __init__(self, instrs, const_tags, const_keys, depth):
        self.instrs = np.ascontiguousarray(np.asarray(instrs, np.uint32).reshape(-1, 4))
        self.const_tags = np.ascontiguousarray(np.asarray(const_tags, np.uint32))
        self.const_keys = np.ascontiguousarray(np.asarray(const_keys, np.uint64))
        self.depth = depth


def filter_paths(flt):
    """The dotted paths a filter names, in first-use order."""
    out = []

    def walk(f):
        if f.kind in ("and", "or"):
            for g in f.filters:
                walk(g)
        elif f.field not in out:
            out.append(f.field)

    walk(flt)
    return out


def compile_filter(flt, column_of, strings):
    """The postfix program of `flt` over the columns `column_of[path]`, or None when it exceeds the engine's limits
    (MAX_PROGRAM instructions, MAX_STACK results on the stack, MAX_CONSTS constants)."""
    instrs, ctags, ckeys = [], [], []
    depth = [0, 0]  # now, deepest

    def push():
        depth[0] += 1
        depth[1] = max(depth[1], depth[0])

    def const(tag, key):
        ctags.append(tag)
        ckeys.append(key)
        return len(ctags) - 1

    def emit(f):
        k = f.kind
        if k == "equals":
            tag, key = encode_constant(f.value, strings)
            instrs.append((OP_EQUALS, column_of[f.field], const(tag, key), 0))
            push()
        elif k == "in":
            enc = [encode_constant(v, strings) for v in f.values]
            flags = (IN_HAS_ANY if enc else 0) | (IN_HAS_COMPLEX if any(t == COMPLEX for t, _ in enc) else 0)
            keep = sorted({e for e in enc if e[0] not in (COMPLEX, NEVER)})
            first = len(ctags)
            for tag, key in keep:
                const(tag, key)
            instrs.append((OP_IN | flags << 8, column_of[f.field], first, len(keep)))
            push()
        elif k == "range":
            flags = (RANGE_HAS_MIN if f.min is not None else 0) | (RANGE_MIN_INCLUSIVE if f.min_inclusive else 0) | \
                    (RANGE_HAS_MAX if f.max is not None else 0) | (RANGE_MAX_INCLUSIVE if f.max_inclusive else 0)
            first = const(FLOAT, f64_bits(f.min if f.min is not None else 0.0))
            const(FLOAT, f64_bits(f.max if f.max is not None else 0.0))
            instrs.append((OP_RANGE | flags << 8, column_of[f.field], first, 0))
            push()
        elif k in ("and", "or"):
            op = OP_AND if k == "and" else OP_OR
            held = 0  # results of this combinator on the stack
            for g in f.filters:
                emit(g)
                held += 1
                if held == _AND_OR_CHUNK:
                    instrs.append((op, held, 0, 0))
                    depth[0] -= held - 1
                    held = 1
            if held != 1 or len(f.filters) == 1:
                instrs.append((op, held, 0, 0))
                depth[0] -= held
                push()
        else:
            raise AssertionError(k)
        if len(instrs) > MAX_PROGRAM or len(ctags) > MAX_CONSTS:
            raise OverflowError

    try:
        emit(flt)
    except OverflowError:
        return None
    if depth[1] > MAX_STACK:
        return None
    return Program(instrs, ctags, ckeys, depth[1])


# ---- the table --------------------------------------------------------------------------------------------------------
class MetaTable:
    """fvdb_meta: the engine's table, over numpy arrays."""

    def __init__(self, ctx):
        self.ctx, self.lib = ctx, ctx.lib
        h = C.c_void_p()
        ctx.check(self.lib.fvdb_meta_create(ctx.h, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.fvdb_meta_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        out = _capi.MetaInfo()
        self.ctx.check(self.lib.fvdb_meta_info(self.h, C.byref(out)))
        return {n: int(getattr(out, n)) for n, _ in out._fields_}

    def set_rows(self, first, ids, present):
        ids = np.ascontiguousarray(ids, np.uint64)
        present = np.ascontiguousarray(present, np.uint8)
        assert ids.size == present.size
        self.ctx.check(self.lib.fvdb_meta_set_rows(self.h, int(first), ids.size, ids.ctypes.data_as(u64p), present.ctypes.data_as(u8p)))

    def set_present(self, slots, present):
        slots = np.ascontiguousarray(slots, np.uint32)
        present = np.ascontiguousarray(present, np.uint8)
        assert slots.size == present.size
        self.ctx.check(self.lib.fvdb_meta_set_present(self.h, slots.ctypes.data_as(u32p), present.ctypes.data_as(u8p), slots.size))

    def add_column(self):
        out = C.c_uint32()
        self.ctx.check(self.lib.fvdb_meta_add_column(self.h, C.byref(out)))
        return int(out.value)

    def set_cells(self, column, slots, tags, vals, elem_tags=(), elem_vals=()):
        slots = np.ascontiguousarray(slots, np.uint32)
        tags = np.ascontiguousarray(tags, np.uint8)
        vals = np.ascontiguousarray(vals, np.uint64)
        et = np.ascontiguousarray(elem_tags, np.uint8)
        ev = np.ascontiguousarray(elem_vals, np.uint64)
        assert slots.size == tags.size == vals.size and et.size == ev.size
        self.ctx.check(self.lib.fvdb_meta_set_cells(self.h, int(column), slots.ctypes.data_as(u32p), tags.ctypes.data_as(u8p),
                                                    vals.ctypes.data_as(u64p), slots.size, et.ctypes.data_as(u8p),
                                                    ev.ctypes.data_as(u64p), et.size))

    def eval(self, program):
        """Runs the program; (matches, unknown) counts.  The arrays stay on the device until fetch()."""
        m, u = C.c_uint64(), C.c_uint64()
        p = program
        self.ctx.check(self.lib.fvdb_meta_eval(self.h, p.instrs.ctypes.data_as(u32p), p.instrs.shape[0], p.const_tags.ctypes.data_as(u32p),
                                               p.const_keys.ctypes.data_as(u64p), p.const_tags.size, C.byref(m), C.byref(u)))
        self._counts = (int(m.value), int(u.value))
        return self._counts

    def fetch(self):
        """(ids, unknown_slots, unknown_ranks) of the last eval()."""
        m, u = self._counts
        ids, us, ur = np.empty(m, np.uint64), np.empty(u, np.uint32), np.empty(u, np.uint32)
        self.ctx.check(self.lib.fvdb_meta_eval_fetch(self.h, ids.ctypes.data_as(u64p), us.ctypes.data_as(u32p), ur.ctypes.data_as(u32p)))
        return ids, us, ur

    def result_pointers(self):
        """Device addresses of the three result arrays and their counts (for work that stays in HBM)."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        m, u = C.c_uint64(), C.c_uint64()
        self.ctx.check(self.lib.fvdb_meta_eval_dev(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(m), C.byref(u)))
        return a.value, b.value, c.value, int(m.value), int(u.value)

    def keys_of_ids_dev(self, column, ids_dev, n, out_tag_dev, out_key_dev):
        """Enqueues the key lookup of n ids in device memory (fvdb_group_keys_of_ids_dev): one
        (tag u8, canon word u64) per id into the two device arrays.  No synchronisation."""
        self.ctx.check(self.lib.fvdb_group_keys_of_ids_dev(self.h, int(column), ids_dev, int(n), out_tag_dev, out_key_dev))

    def keys_of_ids(self, column, ids):
        """The same for a host array of ids: (tags u8 [n], words u64 [n])."""
        ids = np.ascontiguousarray(ids, np.uint64)
        if ids.size == 0:
            self.keys_of_ids_dev(column, None, 0, None, None)  # still refuses a column outside the table
            return np.zeros(0, np.uint8), np.zeros(0, np.uint64)
        bufs = []
        try:
            bufs.append(self.ctx.upload(ids))
            bufs.append(self.ctx.alloc(ids.size))
            bufs.append(self.ctx.alloc(ids.size * 8))
            self.keys_of_ids_dev(column, bufs[0], ids.size, bufs[1], bufs[2])
            return self.ctx.download(bufs[1], ids.shape, np.uint8), self.ctx.download(bufs[2], ids.shape, np.uint64)
        finally:
            for p in bufs:
                self.ctx.free(p)


def cells_arrays(cells):
    """(tags, vals, elem_tags, elem_vals) numpy arrays of a list of encode_value() results, as fvdb_meta_set_cells takes them."""
    tags = np.fromiter((c[0] for c in cells), np.uint8, len(cells))
    vals = np.fromiter((c[1] for c in cells), np.uint64, len(cells))
    elems = [e for c in cells if c[2] for e in c[2]]
    et = np.fromiter((e[0] for e in elems), np.uint8, len(elems))
    ev = np.fromiter((e[1] for e in elems), np.uint64, len(elems))
    return tags, vals, et, ev


class MetadataColumns:
    """One fvdb_meta for a session: slot i = the i-th row id of `rows` (row id -> name in the metadata map), present
    where the name has an entry.  Columns appear the first time a filter names their path."""

    _strings_by_code = None  # decode_key's list of the dictionary's strings by code, rebuilt when the dictionary has grown

    def __init__(self, ctx, rows, metadata):
        self.table = MetaTable(ctx)
        self.ids, self.names, self.slot_of = [], [], {}
        self.columns, self.strings = {}, {}
        self.sync_rows(list(rows), rows, metadata)

    def close(self):
        self.table.close()

    # -- keeping in step with the session ----------------------------------------------------------------------------
    def sync_rows(self, rids, rows, metadata):
        """The listed row ids as they are now: new ones get the next slots, known ones keep theirs; presence and the
        cells of every existing column are rewritten."""
        self.metadata = metadata  # the map the table mirrors: group_column builds a column from it
        slots = []
        first = len(self.ids)
        for rid in rids:
            s = self.slot_of.get(rid)
            if s is None:
                s = self.slot_of[rid] = len(self.ids)
                self.ids.append(rid)
                self.names.append(rows[rid])
            else:
                self.names[s] = rows[rid]
            slots.append(s)
        slots = sorted(set(slots))
        if not slots:
            return
        if len(self.ids) > first:
            self.table.set_rows(first, self.ids[first:], [self.names[s] in metadata for s in range(first, len(self.ids))])
        old = [s for s in slots if s < first]
        if old:
            self.table.set_present(old, [self.names[s] in metadata for s in old])
        for path, col in self.columns.items():
            self._write_cells(path, col, slots, metadata)

    def set_absent(self, rid):
        self.set_absent_many([rid])

    def set_absent_many(self, rids):
        """The listed row ids have no entry in the metadata map any more (ids the table never saw are skipped)."""
        slots = sorted({self.slot_of[rid] for rid in rids if rid in self.slot_of})
        if slots:
            self.table.set_present(slots, [0] * len(slots))

    def _write_cells(self, path, col, slots, metadata):
        cells = []
        for s in slots:
            md = metadata.get(self.names[s])
            cells.append((MISSING, 0, None) if md is None else encode_cell(md, path, self.strings))
        self.table.set_cells(col, slots, *cells_arrays(cells))

    def ensure_column(self, path, metadata):
        """The column of `path`, built in one pass over the rows the first time."""
        col = self.columns.get(path)
        if col is None:
            col = self.table.add_column()
            if self.ids:
                self._write_cells(path, col, range(len(self.ids)), metadata)
            self.columns[path] = col
        return col

    # -- group keys ------------------------------------------------------------------------------
    def group_column(self, path, metadata=None):
        """The column whose cells are the group keys of `path`, built on first use as a "resident" filter builds it, from
        `metadata` or else from the map of the last sync_rows."""
        return self.ensure_column(path, self.metadata if metadata is None else metadata)

    def decode_key(self, tag, word):
        """The Python value of a group key (tag, canon word) as fvdb_group_keys_of_ids_dev writes it: a string by its
        dictionary code, an int from its two's complement, a float from its bits, a bool, None for NULL.  MISSING (a
        group made of one candidate without a key) decodes to `metadata_filter._MISSING`."""
        tag, word = int(tag), int(word)
        if tag == NULL:
            return None
        if tag == BOOL:
            return bool(word)
        if tag == INT:
            return word - (1 << 64) if word >> 63 else word
        if tag == FLOAT:
            return struct.unpack("<d", struct.pack("<Q", word))[0]
        if tag == STRING:
            if self._strings_by_code is None or len(self._strings_by_code) != len(self.strings):
                self._strings_by_code = list(self.strings)  # codes are dense and handed out in insertion order
            return self._strings_by_code[word]
        if tag == MISSING:
            return _MISSING
        raise ValueError(f"tag {tag} is no group key")

    # -- evaluation ----------------------------------------------------------------------------------------------------
    def evaluate(self, flt, metadata):
        """(ids, info): the uint64 ids of the rows whose metadata match `flt`, in slot order; info = route ("device" or
        "host"), slots, matches, unknown (slots decided on the host), columns_created, ms_build / ms_kernel / ms_fetch /
        ms_merge."""
        t0 = time.perf_counter()
        created = [p for p in filter_paths(flt) if p not in self.columns]
        for p in created:
            self.ensure_column(p, metadata)
        program = compile_filter(flt, self.columns, self.strings)
        t1 = time.perf_counter()
        info = {"route": "device", "slots": len(self.ids), "matches": 0, "unknown": 0, "columns_created": created,
                "ms_build": (t1 - t0) * 1e3, "ms_kernel": 0.0, "ms_fetch": 0.0, "ms_merge": 0.0}
        if program is None:  # beyond the engine's limits: the walk over the map, as "pushdown" does it
            ids = np.fromiter((rid for rid, name in zip(self.ids, self.names) if name in metadata and flt.matches(metadata[name])),
                              np.uint64)
            info.update(route="host", matches=int(ids.size), ms_merge=(time.perf_counter() - t1) * 1e3)
            return ids, info
        self.table.eval(program)
        t2 = time.perf_counter()
        ids, unknown, ranks = self.table.fetch()
        t3 = time.perf_counter()
        if unknown.size:  # what the device could not decide, decided here and merged in, in slot order
            mds = (metadata.get(self.names[s]) for s in unknown.tolist())
            yes = np.fromiter((md is not None and flt.matches(md) for md in mds), np.bool_, unknown.size)
            if yes.any():
                extra = np.fromiter((self.ids[s] for s in unknown[yes].tolist()), np.uint64)
                ids = np.insert(ids, ranks[yes].astype(np.int64), extra)
        t4 = time.perf_counter()
        info.update(matches=int(ids.size), unknown=int(unknown.size), ms_kernel=(t2 - t1) * 1e3, ms_fetch=(t3 - t2) * 1e3,
                    ms_merge=(t4 - t3) * 1e3)
        return ids, info
