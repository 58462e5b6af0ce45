"""fvdb_meta_eval on the device against numpy (include/fvdb.h, "metadata columns"): cells are built as numpy arrays and
the expected row ids, unknown slots and merge ranks are computed with numpy from the rules the header states.  Outputs
must be equal element for element, order included."""
import numpy as np
import pytest

import fvdb_import

fv = fvdb_import.load()
MC = fv.metadata_columns
pytestmark = pytest.mark.gpu

T, F, U = 1, 0, 2
SIGN = np.uint64(1 << 63)
u64 = lambda x: np.uint64(x & ((1 << 64) - 1))  # noqa: E731
fbits = lambda x: int(np.float64(x).view(np.uint64))  # noqa: E731


@pytest.fixture(scope="module")
def ctx():
    c = fv.Context(0)
    yield c
    c.close()


# ---- numpy statement of the rules -------------------------------------------------------------------------------------
def np_key(tags, vals):
    tags, vals = np.asarray(tags, np.uint8), np.asarray(vals, np.uint64)
    key, nan = np.zeros(vals.shape, np.uint64), np.zeros(vals.shape, bool)
    i = tags == MC.INT
    key[i] = vals[i] ^ SIGN
    f = tags == MC.FLOAT
    v = vals[f].copy()
    v[(v << np.uint64(1)) == 0] = 0
    nan[f] = (v & ~SIGN) > np.uint64(0x7FF0000000000000)
    key[f] = np.where((v >> np.uint64(63)).astype(bool), ~v, v | SIGN)
    b = (tags == MC.BOOL) | (tags == MC.STRING)
    key[b] = vals[b]
    return key, nan


def np_eq(tags, vals, ctag, ckey):
    key, nan = np_key(tags, vals)
    return (np.asarray(tags) == ctag) & (key == np.uint64(ckey)) & ~nan


def fkey(x):
    """The key of a FLOAT constant, from the numpy statement above (not from the module under test)."""
    key, nan = np_key([MC.FLOAT], [fbits(x)])
    assert not nan[0]
    return int(key[0])


class Column:
    """tags / vals per slot (vals of an ARRAY cell = its length) and the elements of the ARRAY cells, flat, in slot order."""

    def __init__(self, tags, vals, etags=(), evals=()):
        self.tags, self.vals = np.asarray(tags, np.uint8), np.asarray(vals, np.uint64)
        self.etags, self.evals = np.asarray(etags, np.uint8), np.asarray(evals, np.uint64)
        lens = np.where(self.tags == MC.ARRAY, self.vals, 0).astype(np.int64)
        self.off = np.concatenate([[0], np.cumsum(lens)])
        assert self.off[-1] == self.etags.size == self.evals.size
        self.scalar = (self.tags >= MC.NULL) & (self.tags <= MC.STRING)

    def elems(self, s):
        return self.etags[self.off[s]:self.off[s + 1]], self.evals[self.off[s]:self.off[s + 1]]

    def write(self, table, col):
        table.set_cells(col, np.arange(self.tags.size), self.tags, self.vals, self.etags, self.evals)


def exp_equals(c, ctag, ckey):
    res = np.full(c.tags.size, F)
    res[c.tags == MC.COMPLEX] = U
    if ctag == MC.COMPLEX:
        res[c.scalar] = U
    else:
        res[c.scalar & np_eq(c.tags, c.vals, ctag, ckey)] = T
    for s in np.nonzero(c.tags == MC.ARRAY)[0]:
        et, ev = c.elems(s)
        if et.size == 0:
            res[s] = F
        elif ctag == MC.COMPLEX:
            res[s] = U
        else:
            res[s] = T if np_eq(et, ev, ctag, ckey).any() else (U if (et == MC.COMPLEX).any() else F)
    return res


def exp_in(c, ctags, ckeys, flags):
    open_ = U if flags & MC.IN_HAS_COMPLEX else F
    res = np.full(c.tags.size, open_)
    res[c.tags == MC.MISSING] = F
    res[c.tags == MC.COMPLEX] = U if flags & MC.IN_HAS_ANY else F
    hit = np.zeros(c.tags.size, bool)
    for ct, ck in zip(ctags, ckeys):
        hit |= np_eq(c.tags, c.vals, ct, ck)
    res[c.scalar & hit] = T
    return res


def exp_range(c, lo, hi, flags):
    x = np.full(c.tags.size, np.nan)
    f = c.tags == MC.FLOAT
    x[f] = c.vals[f].view(np.float64)
    i = c.tags == MC.INT
    x[i] = [float(int(v)) for v in c.vals[i].view(np.int64)]  # Python's float(int): to nearest even
    with np.errstate(invalid="ignore"):
        lo_ok = (x >= lo if flags & MC.RANGE_MIN_INCLUSIVE else x > lo) if flags & MC.RANGE_HAS_MIN else np.ones(x.size, bool)
        hi_ok = (x <= hi if flags & MC.RANGE_MAX_INCLUSIVE else x < hi) if flags & MC.RANGE_HAS_MAX else np.ones(x.size, bool)
    res = np.where((f | i) & lo_ok & hi_ok, T, F)
    res[c.tags == MC.COMPLEX] = U
    return res


def check(table, program, ids, present, res):
    """The table's outputs for `program` against the per-slot results `res` (numpy T / F / U)."""
    present = np.asarray(present, bool)
    match, unknown = present & (res == T), present & (res == U)
    m, u = table.eval(program)
    got_ids, got_unknown, got_rank = table.fetch()
    assert (m, u) == (int(match.sum()), int(unknown.sum()))
    assert np.array_equal(got_ids, ids[match])
    assert np.array_equal(got_unknown, np.nonzero(unknown)[0].astype(np.uint32))
    assert np.array_equal(got_rank, (np.cumsum(match) - match)[unknown].astype(np.uint32))


def program(instrs, ctags=(), ckeys=()):
    return MC.Program(instrs, ctags, ckeys, 0)


def make_table(ctx, n, present=None):
    t = MC.MetaTable(ctx)
    ids = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(1 << 40)) ^ np.uint64(0x5555)
    present = np.ones(n, np.uint8) if present is None else np.asarray(present, np.uint8)
    t.set_rows(0, ids, present)
    return t, ids, present


# ---- slot counts and presence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1000, 262400])
def test_slot_counts_and_presence_patterns(ctx, n):
    # 262 400 slots = 1025 workgroups: the block scan of the two count arrays takes a second chunk
    s = np.arange(n)
    col = Column(np.where(s % 11 == 5, MC.COMPLEX, MC.INT), np.where(s % 11 == 5, 0, s % 7))
    patterns = [np.ones(n, bool), np.zeros(n, bool), s % 2 == 0, s == n - 1]
    t, ids, _ = make_table(ctx, n, patterns[0])
    c = t.add_column()
    col.write(t, c)
    prog = program([(MC.OP_EQUALS, c, 0, 0)], [MC.INT], [u64(3) ^ SIGN])
    res = exp_equals(col, MC.INT, u64(3) ^ SIGN)
    assert (res == T).any() or n < 4
    for i, present in enumerate(patterns):
        if i:
            t.set_rows(0, ids, present)
        check(t, prog, ids, present, res)
        assert t.info()["present"] == int(present.sum()) and t.info()["slots"] == n
    t.set_present(np.arange(0, n, 3), np.ones(len(range(0, n, 3)), np.uint8))  # on top of "only the last slot"
    present = patterns[3] | (s % 3 == 0)
    check(t, prog, ids, present, res)
    assert t.info()["present"] == int(present.sum())
    t.close()


# ---- one program per leaf kind and tag ------------------------------------------------------------------------------------
INT_CELLS = [0, 1, -1, 3, 2 ** 53, 2 ** 53 + 1, 2 ** 63 - 1, -2 ** 63]
FLOAT_CELLS = [0.0, -0.0, 1.0, 2.5, float("nan"), float("inf"), float("-inf"), float(2 ** 53), 9007199254740994.0]


def zoo(n, seed):
    """n cells drawn from every tag: the scalars above, strings 0..7, arrays of length 0, 1 and 70."""
    rng = np.random.default_rng(seed)
    scal = [(MC.MISSING, 0), (MC.NULL, 0), (MC.BOOL, 0), (MC.BOOL, 1), (MC.COMPLEX, 0)] + [(MC.INT, int(u64(v))) for v in INT_CELLS] + \
           [(MC.FLOAT, fbits(v)) for v in FLOAT_CELLS] + [(MC.STRING, k) for k in range(8)]
    tags, vals, et, ev = [], [], [], []
    for _ in range(n):
        r = rng.random()
        if r < 0.75:
            tg, v = scal[rng.integers(len(scal))]
        else:
            tg, v = MC.ARRAY, int(rng.choice([0, 1, 1, 70]))
            pick = rng.integers(0, len(scal) - 1, v) + 1  # any scalar element or COMPLEX, never MISSING
            et += [scal[p][0] for p in pick]
            ev += [scal[p][1] for p in pick]
        tags.append(tg)
        vals.append(v)
    return Column(tags, vals, et, ev)


@pytest.fixture(scope="module")
def zoo_table(ctx):
    n = 1000
    col = zoo(n, 7)
    present = np.arange(n) % 13 != 4
    t, ids, _ = make_table(ctx, n, present)
    c = t.add_column()
    col.write(t, c)
    yield t, ids, present, col, c
    t.close()


EQ_CONSTANTS = [(MC.NULL, 0), (MC.BOOL, 0), (MC.BOOL, 1), (MC.STRING, 0), (MC.STRING, 5), (MC.STRING, 99), (MC.NEVER, 0), (MC.COMPLEX, 0)] + \
               [(MC.INT, int(u64(v) ^ SIGN)) for v in INT_CELLS] + \
               [(MC.FLOAT, fkey(v)) for v in FLOAT_CELLS if v == v]


def test_equals_every_tag(zoo_table):
    t, ids, present, col, c = zoo_table
    seen = set()
    for ctag, ckey in EQ_CONSTANTS:
        res = exp_equals(col, ctag, ckey)
        seen.update(res[present].tolist())
        check(t, program([(MC.OP_EQUALS, c, 0, 0)], [ctag], [ckey]), ids, present, res)
    assert seen == {T, F, U}
    zero = exp_equals(col, MC.FLOAT, fkey(0.0))  # 0.0 == -0.0; a NaN cell equals nothing
    minus = (col.tags == MC.FLOAT) & (col.vals == SIGN)
    assert minus.any() and zero[minus].all() and (col.tags == MC.FLOAT).sum() > 20


@pytest.mark.parametrize("count", [1, 16, 17, 1000])
def test_in_of_many_constants(zoo_table, count):
    t, ids, present, col, c = zoo_table
    rng = np.random.default_rng(count)
    ints = list(dict.fromkeys(INT_CELLS + [int(v) for v in rng.integers(-10 ** 6, 10 ** 6, 3 * count)]))[:count]  # distinct
    assert len(ints) == count
    consts = sorted((MC.INT, int(u64(v) ^ SIGN)) for v in ints)
    for flags in (MC.IN_HAS_ANY, MC.IN_HAS_ANY | MC.IN_HAS_COMPLEX):
        res = exp_in(col, [a for a, _ in consts], [b for _, b in consts], flags)
        assert (res == T).any()
        check(t, program([(MC.OP_IN | flags << 8, c, 0, count)], [a for a, _ in consts], [b for _, b in consts]), ids, present, res)


def test_in_every_tag(zoo_table):
    t, ids, present, col, c = zoo_table
    consts = sorted([(MC.NULL, 0), (MC.BOOL, 1), (MC.STRING, 2), (MC.STRING, 7), (MC.INT, int(u64(-1) ^ SIGN)), (MC.INT, int(u64(2 ** 63 - 1) ^ SIGN))] +
                    [(MC.FLOAT, fkey(v)) for v in (0.0, float("inf"), float("-inf"), 2.5)] +
                    [(MC.INT, int(u64(v) ^ SIGN)) for v in range(100, 120)])
    ct, ck = [a for a, _ in consts], [b for _, b in consts]
    for lo, n in ((0, len(consts)), (0, 9), (3, 4)):  # a binary search, a linear scan, a window of the pool
        res = exp_in(col, ct[lo:lo + n], ck[lo:lo + n], MC.IN_HAS_ANY)
        check(t, program([(MC.OP_IN | MC.IN_HAS_ANY << 8, c, lo, n)], ct, ck), ids, present, res)
    check(t, program([(MC.OP_IN, c, 0, 0)]), ids, present, exp_in(col, [], [], 0))                       # {"$in": []}
    check(t, program([(MC.OP_IN | 3 << 8, c, 0, 0)]), ids, present, exp_in(col, [], [], 3))              # only COMPLEX constants


def test_range_over_ints_and_floats(zoo_table):
    t, ids, present, col, c = zoo_table
    bounds = [float(2 ** 53), 9007199254740994.0, float(2 ** 63), -float(2 ** 63), 0.0, -0.0, 1.0, float("inf"), float("-inf"), float("nan")]
    every = MC.RANGE_HAS_MIN | MC.RANGE_MIN_INCLUSIVE | MC.RANGE_HAS_MAX | MC.RANGE_MAX_INCLUSIVE
    for lo in bounds:
        for hi, flags in ((float("inf"), MC.RANGE_HAS_MIN | MC.RANGE_MIN_INCLUSIVE), (float("inf"), MC.RANGE_HAS_MIN), (lo, every),
                          (lo, MC.RANGE_HAS_MAX), (lo, MC.RANGE_HAS_MAX | MC.RANGE_MAX_INCLUSIVE), (float(2 ** 63), every)):
            res = exp_range(col, lo, hi, flags)
            check(t, program([(MC.OP_RANGE | flags << 8, c, 0, 0)], [MC.FLOAT, MC.FLOAT], [fbits(lo), fbits(hi)]), ids, present, res)
    # 2^53 + 1 rounds to 2^53 (ties to even): inside [2^53, 2^53], as float(int) says
    res = exp_range(col, float(2 ** 53), float(2 ** 53), every)
    odd = (col.tags == MC.INT) & (col.vals == np.uint64(2 ** 53 + 1))
    assert odd.any() and res[odd].all() and float(2 ** 53 + 1) == float(2 ** 53)
    # 2^63 - 1 rounds up to 2^63
    res = exp_range(col, float(2 ** 63), float("inf"), every)
    top = (col.tags == MC.INT) & (col.vals == np.uint64(2 ** 63 - 1))
    assert top.any() and res[top].all()
    for v in INT_CELLS:  # every listed int is a cell of the zoo
        assert ((col.tags == MC.INT) & (col.vals == u64(v))).any(), v
    for v in FLOAT_CELLS:
        assert ((col.tags == MC.FLOAT) & (col.vals == np.uint64(fbits(v)))).any(), v


def test_arrays_match_first_last_absent(ctx):
    k = lambda v: int(u64(v) ^ SIGN)  # noqa: E731
    fill = list(range(100, 170))
    rows = [[], [5], [6], [5] + fill[1:], fill[:-1] + [5], fill, [5] * 70]
    tags = [MC.ARRAY] * len(rows)
    et = [MC.INT] * sum(len(r) for r in rows)
    ev = [int(u64(v)) for r in rows for v in r]
    # with COMPLEX elements: before a match (true), alone (unknown), beside a miss (unknown)
    rows2 = [(MC.COMPLEX, 0), (MC.INT, 5)], [(MC.COMPLEX, 0)], [(MC.INT, 6), (MC.COMPLEX, 0)], [(MC.INT, 5), (MC.COMPLEX, 0)]
    for r in rows2:
        et += [a for a, _ in r]
        ev += [b for _, b in r]
    col = Column(tags + [MC.ARRAY] * len(rows2), [len(r) for r in rows] + [len(r) for r in rows2], et, ev)
    t, ids, present = make_table(ctx, col.tags.size)
    c = t.add_column()
    col.write(t, c)
    res = exp_equals(col, MC.INT, k(5))
    assert res.tolist() == [F, T, F, T, T, F, T, T, U, U, T]
    check(t, program([(MC.OP_EQUALS, c, 0, 0)], [MC.INT], [k(5)]), ids, present, res)
    check(t, program([(MC.OP_EQUALS, c, 0, 0)], [MC.FLOAT], [fkey(5.0)]), ids, present,
          exp_equals(col, MC.FLOAT, fkey(5.0)))  # INT never equals FLOAT
    check(t, program([(MC.OP_EQUALS, c, 0, 0)], [MC.COMPLEX], [0]), ids, present, exp_equals(col, MC.COMPLEX, 0))
    check(t, program([(MC.OP_IN | MC.IN_HAS_ANY << 8, c, 0, 1)], [MC.INT], [k(5)]), ids, present, np.full(col.tags.size, F))  # $in does not look inside
    check(t, program([(MC.OP_RANGE | MC.RANGE_HAS_MIN << 8, c, 0, 0)], [MC.FLOAT] * 2, [fbits(0.0)] * 2), ids, present, np.full(col.tags.size, F))
    info = t.info()
    assert info["live_elements"] == col.etags.size and info["dead_elements"] == 0 and info["columns"] == 1 and info["hbm_bytes"] > 0
    t.close()


# ---- AND / OR ---------------------------------------------------------------------------------------------------------------
def kleene(op, args):
    order = np.array([0, 2, 1])  # F < U < T
    back = np.array([F, U, T])
    ranks = np.stack([order[a] for a in args])
    return back[ranks.min(axis=0) if op == MC.OP_AND else ranks.max(axis=0)]


def test_and_or_tables_and_depth_limit(ctx):
    n = 27 * 3
    s = np.arange(n)
    cells = [(MC.INT, 1), (MC.INT, 0), (MC.COMPLEX, 0)]  # EQUALS 1: true, false, unknown
    cols = [Column([cells[(s_ // 3 ** j) % 3][0] for s_ in s], [cells[(s_ // 3 ** j) % 3][1] for s_ in s]) for j in range(3)]
    t, ids, present = make_table(ctx, n)
    cs = []
    for col in cols:
        cs.append(t.add_column())
        col.write(t, cs[-1])
    one = int(u64(1) ^ SIGN)
    leaf = [exp_equals(col, MC.INT, one) for col in cols]
    L = lambda j: (MC.OP_EQUALS, cs[j], 0, 0)  # noqa: E731
    for op in (MC.OP_AND, MC.OP_OR):
        check(t, program([L(0), L(1), L(2), (op, 3, 0, 0)], [MC.INT], [one]), ids, present, kleene(op, leaf))
        check(t, program([L(0), L(1), (op, 2, 0, 0)], [MC.INT], [one]), ids, present, kleene(op, leaf[:2]))
        check(t, program([L(1), (op, 1, 0, 0)], [MC.INT], [one]), ids, present, leaf[1])
    check(t, program([(MC.OP_AND, 0, 0, 0)]), ids, present, np.full(n, T))  # an empty AND is true
    check(t, program([(MC.OP_OR, 0, 0, 0)]), ids, present, np.full(n, F))   # an empty OR is false
    # an empty OR under an AND, an empty AND under an OR
    check(t, program([L(0), (MC.OP_OR, 0, 0, 0), (MC.OP_AND, 2, 0, 0)], [MC.INT], [one]), ids, present, np.full(n, F))
    check(t, program([L(0), (MC.OP_AND, 0, 0, 0), (MC.OP_OR, 2, 0, 0)], [MC.INT], [one]), ids, present, np.full(n, T))
    # nested to the depth limit: 16 leaves on the stack, folded from the top by alternating AND 2 / OR 2
    instrs = [L(j % 3) for j in range(MC.MAX_STACK)]
    stack = [leaf[j % 3] for j in range(MC.MAX_STACK)]
    for j in range(MC.MAX_STACK - 1):
        op = MC.OP_AND if j % 2 == 0 else MC.OP_OR
        instrs.append((op, 2, 0, 0))
        b, a = stack.pop(), stack.pop()
        stack.append(kleene(op, [a, b]))
    check(t, program(instrs, [MC.INT], [one]), ids, present, stack[0])
    assert set(stack[0].tolist()) == {T, F, U}
    check(t, program([L(j % 3) for j in range(16)] + [(MC.OP_OR, 16, 0, 0)], [MC.INT], [one]), ids, present, kleene(MC.OP_OR, [leaf[j % 3] for j in range(16)]))
    # one past it
    deeper = [L(j % 3) for j in range(MC.MAX_STACK + 1)] + [(MC.OP_AND, 2, 0, 0)] * MC.MAX_STACK
    with pytest.raises(fv.engine.Unsupported):
        t.eval(program(deeper, [MC.INT], [one]))
    with pytest.raises(fv.engine.Unsupported):
        t.eval(program([L(0)] * (MC.MAX_PROGRAM + 1), [MC.INT], [one]))
    with pytest.raises(fv.engine.Unsupported):
        t.eval(program([L(0)], [MC.INT] * (MC.MAX_CONSTS + 1), [one] * (MC.MAX_CONSTS + 1)))
    for bad in ([(MC.OP_EQUALS, 3, 0, 0)],                       # a column the table does not have
                [(MC.OP_EQUALS, cs[0], 1, 0)],                   # a constant beyond the pool
                [(MC.OP_IN, cs[0], 0, 2)],
                [(MC.OP_RANGE, cs[0], 0, 0)],                    # needs two FLOAT constants
                [L(0), L(1)],                                    # two results left
                [L(0), (MC.OP_AND, 2, 0, 0)],                    # underflow
                [(9, 0, 0, 0)], []):
        with pytest.raises(fv.engine.InvalidConfig):
            t.eval(program(bad, [MC.INT], [one]))
    with pytest.raises(fv.engine.InvalidConfig):  # IN constants must be sorted
        t.eval(program([(MC.OP_IN, cs[0], 0, 2)], [MC.INT, MC.INT], [one, one - 1]))
    check(t, program([L(0)], [MC.INT], [one]), ids, present, leaf[0])  # the table still answers
    t.close()


# ---- mutations -----------------------------------------------------------------------------------------------------------
def test_column_added_after_rows_and_cells_rewritten(ctx):
    n = 300
    t, ids, present = make_table(ctx, n)
    c0 = t.add_column()
    col0 = Column(np.full(n, MC.INT), np.arange(n) % 5)
    col0.write(t, c0)
    c1 = t.add_column()  # after the rows: MISSING everywhere
    seven = int(u64(7) ^ SIGN)
    eq1 = program([(MC.OP_EQUALS, c1, 0, 0)], [MC.INT], [seven])
    check(t, eq1, ids, present, np.full(n, F))
    check(t, program([(MC.OP_EQUALS, c0, 0, 0)], [MC.INT], [int(u64(2) ^ SIGN)]), ids, present, exp_equals(col0, MC.INT, int(u64(2) ^ SIGN)))
    want = np.full(n, F)
    # slot 10 rewritten three times: [7, 1, 1] -> [1, 1, 1, 1, 7] -> [1, 1] -> the scalar 7
    for cell, elems, result, live, dead in (((MC.ARRAY, 3), [7, 1, 1], T, 3, 0), ((MC.ARRAY, 5), [1, 1, 1, 1, 7], T, 5, 3),
                                            ((MC.ARRAY, 2), [1, 1], F, 2, 8), ((MC.INT, 7), [], T, 0, 10)):
        t.set_cells(c1, [10], [cell[0]], [cell[1]], [MC.INT] * len(elems), elems)
        want[10] = result
        check(t, eq1, ids, present, want)
        info = t.info()
        assert (info["live_elements"], info["dead_elements"]) == (live, dead)
    # rows appended after the columns exist: MISSING in both until cells are set; the table grows past its first capacity
    more = 2000
    ids2 = np.arange(more, dtype=np.uint64) + np.uint64(1 << 50)
    t.set_rows(n, ids2, np.ones(more, np.uint8))
    ids_all, present_all = np.concatenate([ids, ids2]), np.ones(n + more, bool)
    want = np.concatenate([want, np.full(more, F)])
    check(t, eq1, ids_all, present_all, want)
    t.set_cells(c1, [n + more - 1], [MC.INT], [7])
    want[-1] = T
    check(t, eq1, ids_all, present_all, want)
    check(t, program([(MC.OP_EQUALS, c0, 0, 0)], [MC.INT], [int(u64(2) ^ SIGN)]), ids_all, present_all,
          np.concatenate([exp_equals(col0, MC.INT, int(u64(2) ^ SIGN)), np.full(more, F)]))
    a, b, c, m, u = t.result_pointers()
    assert a and m == int((col0.vals == 2).sum()) and u == 0
    for bad in (lambda: t.set_cells(c1, [5, 5], [MC.INT] * 2, [1, 2]), lambda: t.set_cells(c1, [n + more], [MC.INT], [1]),
                lambda: t.set_cells(7, [0], [MC.INT], [1]), lambda: t.set_cells(c1, [0], [9], [1]),
                lambda: t.set_cells(c1, [0], [MC.ARRAY], [2], [MC.INT], [1]), lambda: t.set_cells(c1, [0], [MC.ARRAY], [1], [MC.ARRAY], [1]),
                lambda: t.set_cells(c1, [0], [MC.BOOL], [2]), lambda: t.set_cells(c1, [0], [MC.ARRAY], [1], [MC.BOOL], [2]),
                lambda: t.set_present([n + more], [1]), lambda: t.set_rows(n + more + 1, [1], [1])):
        with pytest.raises(fv.engine.InvalidConfig):
            bad()
    t.close()


def test_empty_table(ctx):
    t = MC.MetaTable(ctx)
    with pytest.raises(fv.engine.InvalidConfig):
        t._counts = (0, 0)
        t.fetch()
    assert t.eval(program([(MC.OP_AND, 0, 0, 0)])) == (0, 0)
    assert [a.size for a in t.fetch()] == [0, 0, 0]
    t.close()
