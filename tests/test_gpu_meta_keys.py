"""GPU: the key lookup of grouped search (fvdb_group_keys_of_ids_dev) against
_group_cases.keys_of_ids over a host copy of the same table.

One table of 5000 slots filled in three set_rows calls (the second crosses a growth of the table's arrays; every lookup
after a set_rows follows a rebuild of the id index).  The ids differ only in their high words for a stretch, the id 0 is
a row, one id sits in two slots (the lowest answers), one slot carries FVDB_NO_ID, and the column holds cells of every
tag, +0.0 / -0.0 / NaN / infinity among the floats."""
import numpy as np
import pytest

import fvdb_import
import _group_cases as G

pytestmark = pytest.mark.gpu

SLOTS = 5000
RUNS = ((0, 700), (700, 2600), (2600, SLOTS))  # 700 < 1024 (the first capacity) < 2600 < 5000


def host_table():
    rng = np.random.default_rng(9)
    ids = np.arange(SLOTS, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(5)
    ids[100:400] = (np.arange(300, dtype=np.uint64) + np.uint64(1)) << np.uint64(32)  # the same (zero) low word, different high words
    ids[401:600] = ((np.arange(199, dtype=np.uint64) + np.uint64(1)) << np.uint64(40)) | np.uint64(77)
    ids[3] = 0
    ids[4200] = ids[37]        # a duplicated id: slot 37 answers
    ids[2700] = ids[650]       # the same across two set_rows calls
    ids[50] = G.NO_ID          # never entered, never found
    assert len(set(ids.tolist())) == SLOTS - 2
    present = (rng.random(SLOTS) < 0.9).astype(np.uint8)
    present[[3, 37, 650, 4200, 2700]] = 1
    tags = rng.integers(0, 8, SLOTS).astype(np.uint8)
    vals = rng.integers(0, 40, SLOTS).astype(np.uint64)
    floats = np.flatnonzero(tags == G.FLOAT)
    special = [G.f64_bits(x) for x in (0.0, -0.0, float("nan"), float("inf"), -float("inf"), 1.0, -1.5)] + [0xFFF8000000000001]
    vals[floats] = np.asarray(special, np.uint64)[rng.integers(0, len(special), floats.size)]
    vals[tags == G.BOOL] &= np.uint64(1)
    vals[tags == G.INT] -= np.uint64(20)  # wraps: negative int64 words
    tags[37], vals[37], tags[4200], vals[4200] = G.STRING, 11, G.STRING, 12
    tags[3], vals[3] = G.INT, 0
    return ids, present, tags, vals


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    c = fv.Context(0)
    yield c
    c.close()


def write_cells(table, col, slots, tags, vals):
    """cells as set_cells takes them: an ARRAY cell of `val % 3` NULL elements (the key lookup never reads them)"""
    slots = np.asarray(slots, np.uint32)
    t, v = tags[slots].copy(), vals[slots].copy()
    arr = t == G.ARRAY
    v[arr] %= np.uint64(3)
    v[(t == G.MISSING) | (t == G.NULL) | (t == G.COMPLEX)] = 0
    n_el = int(v[arr].sum())
    table.set_cells(col, slots, t, v, np.full(n_el, G.NULL, np.uint8), np.zeros(n_el, np.uint64))


def queries(ids, lo, hi):
    """ids of the slots so far, ids that are in no slot (a present id with one high bit flipped, 1, 2^63), FVDB_NO_ID, 0"""
    rng = np.random.default_rng(hi)
    known = ids[:hi]
    absent = np.concatenate([known[lo:lo + 50] ^ np.uint64(1 << 47), np.asarray([1, 1 << 63, G.NO_ID, 0, G.NO_ID - 1], np.uint64)])
    return rng.permutation(np.concatenate([known, absent, known[:300]]))


def test_keys_follow_the_table_through_growth_rebuild_and_mutation(fv, ctx):
    ids, present, tags, vals = host_table()
    mc = fv.metadata_columns
    table = mc.MetaTable(ctx)
    try:
        before = table.info()["hbm_bytes"]
        col = None
        for lo, hi in RUNS:
            table.set_rows(lo, ids[lo:hi], present[lo:hi])
            if col is None:
                spare = table.add_column()  # a column the lookup must not read
                col = table.add_column()
                assert (spare, col) == (0, 1)
            write_cells(table, col, np.arange(lo, hi), tags, vals)
            q = queries(ids, lo, hi)
            got_t, got_k = table.keys_of_ids(col, q)
            want_t, want_k = G.keys_of_ids(q, ids[:hi], present[:hi], tags[:hi], vals[:hi])
            assert np.array_equal(got_t, want_t) and np.array_equal(got_k, want_k), f"after slots {lo}..{hi}"
            # the spare column is MISSING everywhere: every key is none
            t0, k0 = table.keys_of_ids(spare, q[:500])
            assert not t0.any() and not k0.any()
        # what the cases above must have exercised
        q = np.asarray([0, ids[37], ids[650], ids[50], ids[150], ids[150] ^ np.uint64(1 << 47)], np.uint64)
        assert int(q[5]) not in set(ids.tolist())
        t, k = table.keys_of_ids(col, q)
        assert (t[0], k[0]) == (G.INT, 0)              # the id 0 is an ordinary id
        assert (t[1], k[1]) == (G.STRING, 11)          # the lowest of two slots
        assert t[3] == G.MISSING and t[5] == G.MISSING  # FVDB_NO_ID although a slot carries it; an id in no slot
        assert table.info()["hbm_bytes"] >= before + 16384 * 12  # the index: 2^14 cells of 12 bytes for 5000 slots

        # presence is read at lookup time: cleared and set again with no set_rows (so no rebuild) in between
        table.set_present([37], [0])
        present[37] = 0
        t, k = table.keys_of_ids(col, q)
        assert (t[1], k[1]) == (G.MISSING, 0)  # NOT the copy in slot 4200
        table.set_present([37], [1])
        present[37] = 1
        t, k = table.keys_of_ids(col, q)
        assert (t[1], k[1]) == (G.STRING, 11)
        # so is the cell
        tags[[37, 650]], vals[[37, 650]] = (G.FLOAT, G.BOOL), (G.f64_bits(-0.0), 1)
        write_cells(table, col, [37, 650], tags, vals)
        t, k = table.keys_of_ids(col, q)
        assert (t[1], k[1]) == (G.FLOAT, 0) and (t[2], k[2]) == (G.BOOL, 1)
        allq = queries(ids, 0, SLOTS)
        got_t, got_k = table.keys_of_ids(col, allq)
        want_t, want_k = G.keys_of_ids(allq, ids, present, tags, vals)
        assert np.array_equal(got_t, want_t) and np.array_equal(got_k, want_k)
        assert sorted(set(want_t.tolist())) == [G.MISSING, G.NULL, G.BOOL, G.INT, G.FLOAT, G.STRING]

        # rewriting existing slots through set_rows moves ids: the next lookup sees the new owner
        ids[10], ids[11] = ids[11], ids[10]
        table.set_rows(10, ids[10:12], present[10:12])
        got_t, got_k = table.keys_of_ids(col, allq)
        want_t, want_k = G.keys_of_ids(allq, ids, present, tags, vals)
        assert np.array_equal(got_t, want_t) and np.array_equal(got_k, want_k)
    finally:
        table.close()


def test_refusals_before_anything_is_enqueued(fv, ctx):
    mc = fv.metadata_columns
    table = mc.MetaTable(ctx)
    lib = fv._capi.load()
    p = ctx.alloc(64)
    try:
        assert lib.fvdb_group_keys_of_ids_dev(table.h, 0, p, 1, p, p) == 6       # no column yet
        col = table.add_column()
        assert lib.fvdb_group_keys_of_ids_dev(table.h, col + 1, p, 1, p, p) == 6  # one past the last column
        assert lib.fvdb_group_keys_of_ids_dev(table.h, col + 1, None, 0, None, None) == 6
        assert lib.fvdb_group_keys_of_ids_dev(table.h, col, None, 0, None, None) == 0
        assert lib.fvdb_group_keys_of_ids_dev(table.h, col, None, 1, p, p) == 6
        assert lib.fvdb_group_keys_of_ids_dev(table.h, col, p, 1 << 31, p, p) == 12
        assert lib.fvdb_group_keys_of_ids_dev(None, col, p, 1, p, p) == 6
        # an empty table: every id is in no slot
        t, k = table.keys_of_ids(col, np.asarray([0, 5, G.NO_ID], np.uint64))
        assert not t.any() and not k.any()
    finally:
        ctx.free(p)
        table.close()
