"""Shared by the metadata-column tests: a pure-Python interpreter of the filter program over encoded cells (the
statement of the three-valued rules the kernel must follow, independent of the engine), and the randomized metadata and
filters both the no-GPU and the GPU test draw from a fixed seed."""
import math
import random
import struct

import fvdb_import

fv = fvdb_import.load()
MC = fv.metadata_columns
MetadataFilter = fv.metadata_filter.MetadataFilter

T, F, U = 1, 0, 2
SCALARS = (MC.NULL, MC.BOOL, MC.INT, MC.FLOAT, MC.STRING)


def _f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _eq(tag, payload, ctag, ckey):
    """A scalar cell (or element) against a constant that is neither COMPLEX nor NEVER-by-tag.  The constant's key is
    decoded as include/fvdb.h states it and the VALUES are compared, so nothing here goes through the module's own
    key function."""
    if tag != ctag:
        return False
    if tag == MC.INT:
        return payload == ckey ^ (1 << 63)                # the int64 with its sign bit flipped
    if tag == MC.FLOAT:                                   # sign bit set: a non-negative f64; else all bits flipped
        bits = ckey ^ (1 << 63) if ckey >> 63 else ~ckey & ((1 << 64) - 1)
        return _f64(payload) == _f64(bits)                # f64 values: 0.0 == -0.0, a NaN equals nothing
    return payload == ckey if tag in (MC.BOOL, MC.STRING) else True  # NULL equals NULL


def leaf_equals(cell, ctag, ckey):
    tag, payload, elems = cell
    if tag == MC.MISSING:
        return F
    if tag == MC.COMPLEX:
        return U
    if tag != MC.ARRAY:
        return U if ctag == MC.COMPLEX else (T if _eq(tag, payload, ctag, ckey) else F)
    if not elems:
        return F
    if ctag == MC.COMPLEX:
        return U
    r = F
    for et, ep in elems:
        if et == MC.COMPLEX:
            r = U
        elif _eq(et, ep, ctag, ckey):
            return T
    return r


def leaf_in(cell, consts, flags):
    tag, payload, _ = cell
    open_ = U if flags & MC.IN_HAS_COMPLEX else F
    if tag == MC.MISSING:
        return F
    if tag == MC.COMPLEX:
        return U if flags & MC.IN_HAS_ANY else F
    if tag == MC.ARRAY:
        return open_
    return T if any(_eq(tag, payload, ct, ck) for ct, ck in consts) else open_


def leaf_range(cell, lo_bits, hi_bits, flags):
    tag, payload, _ = cell
    if tag == MC.COMPLEX:
        return U
    if tag == MC.INT:
        x = float(payload - (1 << 64) if payload >> 63 else payload)  # Python's float(int): to nearest even
    elif tag == MC.FLOAT:
        x = _f64(payload)
    else:
        return F
    lo, hi = _f64(lo_bits), _f64(hi_bits)
    lo_ok = not flags & MC.RANGE_HAS_MIN or (x >= lo if flags & MC.RANGE_MIN_INCLUSIVE else x > lo)
    hi_ok = not flags & MC.RANGE_HAS_MAX or (x <= hi if flags & MC.RANGE_MAX_INCLUSIVE else x < hi)
    return T if lo_ok and hi_ok else F


def interpret(program, cells_of_column):
    """The program's result (T, F or U) on one slot; cells_of_column[col] = that slot's encode_value() triple."""
    stack = []
    ct, ck = program.const_tags.tolist(), program.const_keys.tolist()
    for op_flags, a, b, c in program.instrs.tolist():
        op, flags = op_flags & 0xFF, op_flags >> 8
        if op == MC.OP_EQUALS:
            stack.append(leaf_equals(cells_of_column[a], ct[b], ck[b]))
        elif op == MC.OP_IN:
            stack.append(leaf_in(cells_of_column[a], list(zip(ct[b:b + c], ck[b:b + c])), flags))
        elif op == MC.OP_RANGE:
            stack.append(leaf_range(cells_of_column[a], ck[b], ck[b + 1], flags))
        else:
            args = [stack.pop() for _ in range(a)]
            assert len(args) == a
            if op == MC.OP_AND:
                stack.append(F if F in args else (U if U in args else T))
            else:
                assert op == MC.OP_OR
                stack.append(T if T in args else (U if U in args else F))
        assert len(stack) <= MC.MAX_STACK
    assert len(stack) == 1
    return stack[0]


# ---- the randomized population ------------------------------------------------------------------------------------------
NAN = float("nan")
INTS = [0, 1, -1, 7, 2 ** 53, 2 ** 53 + 1, 2 ** 63 - 1, -2 ** 63]
FLOATS = [0.0, -0.0, 1.0, 2.5, float(2 ** 53), NAN, math.inf, -math.inf]
STRINGS = ["", "a", "A", "1", "é漢"]
PLAIN_SCALARS = [None, True, False] + INTS + FLOATS + STRINGS
PLAIN_ARRAYS = [[], [1], ["a"], [1, "a", 1.0, True, None], ["A", "a", ""], [2 ** 53 + 1, 0.0, -0.0], [NAN, 1.0], [False, 0]]
COMPLEX_VALUES = [[[1], [2]], [1, [2], "a"], {"x": 1}, 2 ** 63, -2 ** 63 - 1, [2 ** 64, 1], [{"a": 1}, "a"], ["a", [1]]]
COMPLEX_CONSTANTS = [[1], ["a", "A"], {"x": 1}, 2 ** 63, []]
PLAIN_PATHS = ["a", "b", "tags", "obj.x", "obj.y.z", "s.t", "nope"]  # "s.t" runs through a scalar; "nope" is never there
COMPLEX_PATHS = PLAIN_PATHS + ["obj", "obj.y"]                     # an object reached whole


def random_metadata(rng, complex_too):
    def value(arrays=True):
        r = rng.random()
        if complex_too and r < 0.12:
            return rng.choice(COMPLEX_VALUES)
        if arrays and r < 0.35:
            return rng.choice(PLAIN_ARRAYS)
        return rng.choice(PLAIN_SCALARS)

    md = {}
    for f in ("a", "b"):
        if rng.random() < 0.85:
            md[f] = value()
    if rng.random() < 0.8:
        md["tags"] = rng.choice(PLAIN_ARRAYS) if rng.random() < 0.8 else value()
    if rng.random() < 0.8:
        md["obj"] = {"x": value(), "y": {"z": value()}} if rng.random() < 0.8 else value()
    if rng.random() < 0.7:
        md["s"] = rng.choice(PLAIN_SCALARS)
    return md


def random_filter_json(rng, complex_too, depth=0):
    paths = COMPLEX_PATHS if complex_too else PLAIN_PATHS

    def constant():
        if complex_too and rng.random() < 0.15:
            return rng.choice(COMPLEX_CONSTANTS)
        c = rng.choice(PLAIN_SCALARS + ["zzz-not-in-any-row"])
        return c

    def leaf():
        kind = rng.choice(("equals", "equals", "in", "range"))
        if kind == "equals":
            return rng.choice(paths), constant()
        if kind == "in":
            return rng.choice(paths), {"$in": [constant() for _ in range(rng.choice((0, 1, 2, 5, 20)))]}
        lo_op, hi_op = rng.choice(("$gte", "$gt", None)), rng.choice(("$lte", "$lt", None))
        if lo_op is None and hi_op is None:
            lo_op = "$gte"
        bounds = INTS + FLOATS + [-3, 0.5, 9.007199254740993e15]
        spec = {}
        if lo_op:
            spec[lo_op] = rng.choice(bounds)
        if hi_op:
            spec[hi_op] = rng.choice(bounds)
        return rng.choice(paths), spec

    r = rng.random()
    if depth < 3 and r < 0.45:
        return {rng.choice(("$and", "$or")): [random_filter_json(rng, complex_too, depth + 1) for _ in range(rng.choice((0, 1, 2, 3, 3)))]}
    if r < 0.6:  # several fields in one object: implicit AND
        return dict(leaf() for _ in range(rng.choice((2, 3))))
    return dict([leaf()])


def population(seed, rows, filters, complex_too):
    """(list of metadata dicts, list of filter JSON) from a fixed seed."""
    rng = random.Random(seed)
    mds = [random_metadata(rng, complex_too) for _ in range(rows)]
    return mds, [random_filter_json(rng, complex_too) for _ in range(filters)]


def interpreter_counts(mds, flt_json):
    """Encodes every row's cells for the filter's paths, compiles the filter, runs the interpreter: (per-row results,
    number of unknown rows).  Strings are interned over all rows first, as a table built before the filter does."""
    flt = MetadataFilter.from_json(flt_json)
    paths = MC.filter_paths(flt)
    strings, columns = {}, {p: i for i, p in enumerate(paths)}
    cells = [[MC.encode_cell(md, p, strings) for p in paths] for md in mds]
    program = MC.compile_filter(flt, columns, strings)
    assert program is not None
    res = [interpret(program, row) for row in cells]
    return flt, res, sum(r == U for r in res)
