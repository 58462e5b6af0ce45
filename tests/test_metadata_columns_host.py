"""metadata_columns.py without a GPU: the encoder's tags and payloads, the compiler's programs, and the three-valued rules
(the interpreter of tests/_meta_cases.py over encoded cells) against MetadataFilter.matches on the randomized population
the GPU session test uses."""
import math
import struct

import numpy as np

import _meta_cases as K

MC = K.MC
MetadataFilter = K.MetadataFilter


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_encoder_tags_and_payloads():
    s = {}
    enc = lambda md, path: MC.encode_cell(md, path, s)  # noqa: E731
    assert enc({}, "a") == (MC.MISSING, 0, None)
    assert enc({"a": None}, "a") == (MC.NULL, 0, None)
    assert enc({"a": True}, "a") == (MC.BOOL, 1, None) and enc({"a": False}, "a") == (MC.BOOL, 0, None)
    assert enc({"a": 1}, "a") == (MC.INT, 1, None)
    assert enc({"a": -1}, "a") == (MC.INT, (1 << 64) - 1, None)
    assert enc({"a": 2 ** 63 - 1}, "a") == (MC.INT, 2 ** 63 - 1, None)
    assert enc({"a": -2 ** 63}, "a") == (MC.INT, 1 << 63, None)
    assert enc({"a": 2 ** 63}, "a") == (MC.COMPLEX, 0, None) and enc({"a": -2 ** 63 - 1}, "a") == (MC.COMPLEX, 0, None)
    assert enc({"a": 1.0}, "a") == (MC.FLOAT, bits(1.0), None)
    assert enc({"a": -0.0}, "a") == (MC.FLOAT, 1 << 63, None)
    assert enc({"a": math.inf}, "a") == (MC.FLOAT, 0x7FF0000000000000, None)
    tag, payload, _ = enc({"a": math.nan}, "a")
    assert tag == MC.FLOAT and payload & 0x7FFFFFFFFFFFFFFF > 0x7FF0000000000000
    # strings: dense codes in first-seen order, exact (case and emptiness matter, no hashing)
    assert [enc({"a": x}, "a") for x in ("", "a", "A", "é漢", "a")] == \
        [(MC.STRING, 0, None), (MC.STRING, 1, None), (MC.STRING, 2, None), (MC.STRING, 3, None), (MC.STRING, 1, None)]
    assert s == {"": 0, "a": 1, "A": 2, "é漢": 3}
    assert enc({"a": {"x": 1}}, "a") == (MC.COMPLEX, 0, None)        # an object compared whole
    assert enc({"a": {"x": 1}}, "a.x") == (MC.INT, 1, None)          # reached by a dotted path
    assert enc({"a": {"x": {"y": "A"}}}, "a.x.y") == (MC.STRING, 2, None)
    assert enc({"a": 5}, "a.x") == (MC.MISSING, 0, None)             # a path through a scalar
    assert enc({"a": [1]}, "a.0") == (MC.MISSING, 0, None)           # or through an array
    assert enc({"a": []}, "a") == (MC.ARRAY, 0, [])
    assert enc({"a": [1, "a", 1.0, True, None, [2], {"k": 1}, 2 ** 64]}, "a") == (MC.ARRAY, 8, [
        (MC.INT, 1), (MC.STRING, 1), (MC.FLOAT, bits(1.0)), (MC.BOOL, 1), (MC.NULL, 0), (MC.COMPLEX, 0), (MC.COMPLEX, 0), (MC.COMPLEX, 0)])
    assert enc({"a": (1, 2)}, "a") == (MC.COMPLEX, 0, None) and enc({"a": np.int64(3)}, "a") == (MC.COMPLEX, 0, None)
    tags, vals, et, ev = MC.cells_arrays([enc({"a": [1, "A"]}, "a"), enc({"a": -1}, "a"), enc({}, "a"), enc({"a": []}, "a")])
    assert tags.tolist() == [MC.ARRAY, MC.INT, MC.MISSING, MC.ARRAY] and vals.tolist() == [2, (1 << 64) - 1, 0, 0]
    assert et.tolist() == [MC.INT, MC.STRING] and ev.tolist() == [1, 2]


def test_constants_and_ordered_keys():
    s = {"a": 0, "b": 1}
    assert MC.encode_constant("b", s) == (MC.STRING, 1)
    assert MC.encode_constant("zzz", s) == (MC.NEVER, 0) and s == {"a": 0, "b": 1}  # a constant is never interned
    assert MC.encode_constant(math.nan, s) == (MC.NEVER, 0)
    assert MC.encode_constant(0.0, s) == MC.encode_constant(-0.0, s) == (MC.FLOAT, 1 << 63)
    assert MC.encode_constant(1, s)[0] == MC.INT and MC.encode_constant(1.0, s)[0] == MC.FLOAT
    assert MC.encode_constant(True, s) == (MC.BOOL, 1) and MC.encode_constant(None, s) == (MC.NULL, 0)
    for c in ([1], {"x": 1}, 2 ** 63, []):
        assert MC.encode_constant(c, s) == (MC.COMPLEX, 0)
    ints = [-2 ** 63, -5, -1, 0, 1, 2 ** 53, 2 ** 63 - 1]
    keys = [MC.encode_constant(v, s)[1] for v in ints]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    floats = [-math.inf, -2.5, -5e-324, 0.0, 5e-324, 1.0, float(2 ** 53), math.inf]
    keys = [MC.encode_constant(v, s)[1] for v in floats]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def compiled(flt_json, columns=None, strings=None):
    flt = MetadataFilter.from_json(flt_json)
    columns = columns if columns is not None else {p: i for i, p in enumerate(MC.filter_paths(flt))}
    return MC.compile_filter(flt, columns, {} if strings is None else strings)


def test_compiler_programs():
    s = {"even": 4}
    p = compiled({"tag": "even"}, strings=s)
    assert p.instrs.tolist() == [[MC.OP_EQUALS, 0, 0, 0]] and p.const_tags.tolist() == [MC.STRING] and p.const_keys.tolist() == [4]
    assert p.depth == 1 and p.instrs.dtype == np.uint32 and p.const_keys.dtype == np.uint64
    p = compiled({"n": {"$in": [3, 1, 3, "odd", [1], math.nan, 1.0]}}, strings=s)  # sorted by (tag, key), distinct; "odd": no code
    assert p.instrs.tolist() == [[MC.OP_IN | (MC.IN_HAS_ANY | MC.IN_HAS_COMPLEX) << 8, 0, 0, 3]]
    assert p.const_tags.tolist() == [MC.INT, MC.INT, MC.FLOAT]
    assert p.const_keys.tolist() == [1 ^ (1 << 63), 3 ^ (1 << 63), bits(1.0) | (1 << 63)]
    assert compiled({"n": {"$in": []}}).instrs.tolist() == [[MC.OP_IN, 0, 0, 0]]
    p = compiled({"n": {"$gte": 1, "$lt": 2.5}})
    flags = MC.RANGE_HAS_MIN | MC.RANGE_MIN_INCLUSIVE | MC.RANGE_HAS_MAX
    assert p.instrs.tolist() == [[MC.OP_RANGE | flags << 8, 0, 0, 0]]
    assert p.const_tags.tolist() == [MC.FLOAT, MC.FLOAT] and p.const_keys.tolist() == [bits(1.0), bits(2.5)]
    p = compiled({"n": {"$gt": 0}})  # an absent bound keeps its "inclusive" default and has no HAS flag
    assert p.instrs.tolist() == [[MC.OP_RANGE | (MC.RANGE_HAS_MIN | MC.RANGE_MAX_INCLUSIVE) << 8, 0, 0, 0]]
    # implicit AND over several fields, in the order written
    p = compiled({"a": 1, "b": {"$in": [2]}, "c": {"$lte": 3}})
    assert [r[0] & 0xFF for r in p.instrs.tolist()] == [MC.OP_EQUALS, MC.OP_IN, MC.OP_RANGE, MC.OP_AND]
    assert p.instrs[-1].tolist() == [MC.OP_AND, 3, 0, 0] and [r[1] for r in p.instrs.tolist()[:3]] == [0, 1, 2] and p.depth == 3
    assert compiled({"$and": []}).instrs.tolist() == [[MC.OP_AND, 0, 0, 0]]
    assert compiled({"$or": []}).instrs.tolist() == [[MC.OP_OR, 0, 0, 0]]
    # nesting, and a path named twice shares its column
    p = compiled({"$or": [{"a": 1}, {"$and": [{"b": 2}, {"$or": [{"a": 3}, {"c": 4}]}]}]})
    assert [(r[0], r[1]) for r in p.instrs.tolist()] == [(MC.OP_EQUALS, 0), (MC.OP_EQUALS, 1), (MC.OP_EQUALS, 0), (MC.OP_EQUALS, 2),
                                                         (MC.OP_OR, 2), (MC.OP_AND, 2), (MC.OP_OR, 2)]
    assert p.depth == 4
    # a wide combinator is folded eight operands at a time, so it stays shallow
    p = compiled({"$or": [{"a": i} for i in range(20)]})
    assert [r[1] for r in p.instrs.tolist() if r[0] == MC.OP_OR] == [8, 8, 6] and p.depth == 8 and len(p.instrs) == 23


def nested(depth):
    f = {"a": 0}
    for i in range(depth - 1):
        f = {"$and": [{"a": i + 1}, f]}
    return f


def test_compiler_limits():
    assert compiled(nested(MC.MAX_STACK)).depth == MC.MAX_STACK
    assert compiled(nested(MC.MAX_STACK + 1)) is None                                   # the stack
    assert compiled({"a": {"$in": list(range(MC.MAX_CONSTS))}}) is not None
    assert compiled({"a": {"$in": list(range(MC.MAX_CONSTS + 1))}}) is None             # the constant pool
    assert compiled({"$or": [{"a": i} for i in range(800)]}) is not None
    assert compiled({"$or": [{"a": i} for i in range(1000)]}) is None                   # the program


def check_population(complex_too, seed, rows, filters):
    mds, flts = K.population(seed, rows, filters, complex_too)
    unknown_total, decided = 0, [0, 0]
    for fj in flts:
        flt, res, unknown = K.interpreter_counts(mds, fj)
        unknown_total += unknown
        for md, r in zip(mds, res):
            if r != K.U:
                assert (r == K.T) == flt.matches(md), (fj, md)
                decided[r] += 1
    return unknown_total, decided


def test_interpreter_agrees_with_matches_on_the_plain_population():
    # no COMPLEX value and no list / object / wide-integer constant: nothing may be left unknown
    unknown, decided = check_population(False, 20240521, 400, 300)
    assert unknown == 0 and decided[0] > 1000 and decided[1] > 1000


def test_interpreter_agrees_with_matches_on_the_full_population():
    unknown, decided = check_population(True, 20240522, 400, 300)
    assert unknown > 0 and decided[0] > 1000 and decided[1] > 1000


def test_plain_population_covers_every_leaf_kind_and_tag():
    mds, flts = K.population(20240521, 400, 300, False)
    seen = set()
    for fj in flts:
        flt = MetadataFilter.from_json(fj)
        strings = {}
        paths = MC.filter_paths(flt)
        cells = [[MC.encode_cell(md, p, strings) for p in paths] for md in mds]
        prog = MC.compile_filter(flt, {p: i for i, p in enumerate(paths)}, strings)
        for op_flags, a, b, c in prog.instrs.tolist():
            op = op_flags & 0xFF
            if op in (MC.OP_EQUALS, MC.OP_IN, MC.OP_RANGE):
                seen.update((op, row[a][0]) for row in cells)
    tags = (MC.MISSING, MC.NULL, MC.BOOL, MC.INT, MC.FLOAT, MC.STRING, MC.ARRAY)
    assert seen == {(op, t) for op in (MC.OP_EQUALS, MC.OP_IN, MC.OP_RANGE) for t in tags}
