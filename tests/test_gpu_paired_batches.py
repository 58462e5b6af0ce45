"""HybridIndex.search_dev_begin / search_dev_end with one IVF chain for two batches in flight.
The reference for every comparison is the blocking search_dev of the same batch on the same index: ids, hit counts and
the bit patterns of the distances must be equal, whichever batch shared a chain with which.  Whether ONE chain served
two batches is read from the plan's counters (IVFIndex.last_stats of the last chain enqueued): rows_scanned is the sum
over the probed lists of (queries probing the list) x (rows in it), so a joint chain shows the sum of its two batches
and a chain of one batch shows that batch's figure."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fvdb_import
from _data import bits
from _paired_child import D, K, KW, LOOP_SIZES, NPROBE, batch, build_index, pipelined

pytestmark = pytest.mark.gpu

# batch sizes the tests draw from: B >= 32 engages the matrix-core filter, below it the exact scan runs
SIZES = (64, 64, 33, 47, 20, 20, 5, 5)


class Fixture:
    pass


@pytest.fixture(scope="module")
def env():
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    e = Fixture()
    e.fv, e.ctx = fv, ctx
    e.g, e.x = build_index(fv, ctx)
    e.q = [batch(e.x, B, 500 + j) for j, B in enumerate(SIZES)]
    e.qdev = [ctx.upload(q) for q in e.q]
    e.want, e.rows = [], []
    for j, B in enumerate(SIZES):  # computed once, shared by every test, never changed
        e.want.append(e.g.search_dev(e.qdev[j], B, K, **KW))
        e.rows.append(e.g.ivf().last_stats()["rows_scanned"])
    yield e
    del e.g
    ctx.close()


def same(got, want):
    assert np.array_equal(got.counts, want.counts)
    assert np.array_equal(got.ids, want.ids)
    assert np.array_equal(bits(got.distances), bits(want.distances))


def last_rows(e):
    return e.g.ivf().last_stats()["rows_scanned"]


def begin(e, slot, j, **kw):
    e.g.search_dev_begin(slot, e.qdev[j], SIZES[j], kw.pop("k", K), **dict(KW, **kw))


def test_reference_has_both_parts(env):
    # the comparison means something only if both parts contribute neighbours and the lists are really scanned
    e = env
    assert e.g.recent_count() > 6000 and e.g.historical_count() > 15000
    assert all(r > 0 for r in e.rows)
    w = e.want[0]
    assert (w.counts == K).all()
    hist_only = e.g.search_dev(e.qdev[0], SIZES[0], K, search_recent=False, **KW)
    rec_only = e.g.search_dev(e.qdev[0], SIZES[0], K, search_historical=False, **KW)
    assert not np.array_equal(hist_only.ids, w.ids) and not np.array_equal(rec_only.ids, w.ids)


@pytest.mark.parametrize("a,b", [(0, 1), (2, 3)], ids=["64+64", "33+47"])
def test_pair_equals_blocking_and_runs_one_chain(env, a, b):
    e = env
    begin(e, 0, a)
    begin(e, 1, b)
    ra, rb = e.g.search_dev_end(0), e.g.search_dev_end(1)
    same(ra, e.want[a])
    same(rb, e.want[b])
    assert last_rows(e) == e.rows[a] + e.rows[b]


@pytest.mark.parametrize("a,b", [(4, 5), (6, 7)], ids=["20+20", "5+5"])
def test_small_batches_pair(env, a, b):
    # 20 + 20: alone each batch takes the exact scan (B < 32), together the filter; 5 + 5: the exact scan both ways
    e = env
    begin(e, 0, a)
    begin(e, 1, b)
    rb, ra = e.g.search_dev_end(1), e.g.search_dev_end(0)
    same(ra, e.want[a])
    same(rb, e.want[b])
    assert last_rows(e) == e.rows[a] + e.rows[b]


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)], ids=["begin-order", "reverse"])
def test_three_batches(env, order):
    # the third has no partner: its chain starts at its own end
    e = env
    js = (0, 2, 3)
    for slot, j in enumerate(js):
        begin(e, slot, j)
    got = {}
    for slot in order:
        got[slot] = e.g.search_dev_end(slot)
    for slot, j in enumerate(js):
        same(got[slot], e.want[j])


def test_slot_reuse_before_the_partner_is_collected(env):
    # the launching slot (1) is collected and begun again while its partner (0) still has to read the joint block
    e = env
    begin(e, 0, 0)
    begin(e, 1, 2)            # pairs 0 and 1, launched from slot 1
    r1 = e.g.search_dev_end(1)
    begin(e, 1, 3)            # slot 1 again: waiting
    begin(e, 2, 1)            # pairs 1 and 2
    assert last_rows(e) == e.rows[3] + e.rows[1]
    r0 = e.g.search_dev_end(0)
    r1b = e.g.search_dev_end(1)
    r2 = e.g.search_dev_end(2)
    same(r0, e.want[0])
    same(r1, e.want[2])
    same(r1b, e.want[3])
    same(r2, e.want[1])


@pytest.mark.parametrize("other", [dict(ivf_n_probe=NPROBE // 2), dict(k=7)], ids=["n_probe", "k"])
def test_incompatible_partners_run_two_chains(env, other):
    e = env
    k2 = other.get("k", K)
    want_b = e.g.search_dev(e.qdev[1], SIZES[1], k2, **dict(KW, **{x: v for x, v in other.items() if x != "k"}))
    rows_b = last_rows(e)
    begin(e, 0, 0)
    begin(e, 1, 1, **other)   # cannot share: slot 0's chain goes alone, slot 1 waits
    ra, rb = e.g.search_dev_end(0), e.g.search_dev_end(1)
    same(ra, e.want[0])
    same(rb, want_b)
    assert last_rows(e) == rows_b  # the last chain served the second batch alone


@pytest.mark.parametrize("depth", [1, 2, 3, 8])
def test_pipelined_loops(env, depth):
    e = env
    js = (0, 2, 3, 1)  # 64, 33, 47, 64
    res = pipelined(e.g, [e.qdev[j] for j in js], [SIZES[j] for j in js], 24, depth)
    for i, r in enumerate(res):
        same(r, e.want[js[i % 4]])


def test_waiting_batch_then_mutation_and_blocking_search(env):
    e = env
    begin(e, 0, 0)  # waiting
    with pytest.raises(e.fv.FvdbError):  # refused while a slot is in flight, as ever
        e.g.insert_with_timestamp(10 ** 9, e.x[0] + 1, KW["now"], KW["now"])
    same(e.g.search_dev_end(0), e.want[0])
    begin(e, 0, 2)  # waiting
    same(e.g.search_dev(e.qdev[3], SIZES[3], K, **KW), e.want[3])
    same(e.g.search_dev_end(0), e.want[2])


def test_flags(env):
    e = env
    want = {}
    for flags in (dict(search_historical=False), dict(search_recent=False)):
        for j in (0, 2):
            want[(j, tuple(flags))] = e.g.search_dev(e.qdev[j], SIZES[j], K, **dict(KW, **flags))
    # without a historical part a batch never waits: the one waiting stays the one waiting
    begin(e, 0, 0)                               # waiting
    begin(e, 1, 2, search_historical=False)
    same(e.g.search_dev_end(1), want[(2, ("search_historical",))])
    begin(e, 1, 2)                               # pairs with slot 0
    assert last_rows(e) == e.rows[0] + e.rows[2]
    same(e.g.search_dev_end(0), e.want[0])
    same(e.g.search_dev_end(1), e.want[2])
    # the IVF part alone
    begin(e, 0, 0, search_recent=False)
    begin(e, 1, 2, search_recent=False)
    assert last_rows(e) == e.rows[0] + e.rows[2]
    same(e.g.search_dev_end(0), want[(0, ("search_recent",))])
    same(e.g.search_dev_end(1), want[(2, ("search_recent",))])


def test_switch_off_in_a_fresh_process(env, tmp_path):
    # FVDB_HYBRID_PAIR is read once, so the other setting needs a process of its own
    e = env
    out = str(tmp_path / "off.npz")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_paired_child.py")
    subprocess.run([sys.executable, child, out], env=dict(os.environ, FVDB_HYBRID_PAIR="0"), check=True, timeout=120)
    off = np.load(out)
    qdev = [e.ctx.upload(batch(e.x, B, 700 + j)) for j, B in enumerate(LOOP_SIZES)]
    res = pipelined(e.g, qdev, LOOP_SIZES, 8, 3)
    for i, r in enumerate(res):
        assert np.array_equal(r.ids, off[f"ids{i}"])
        assert np.array_equal(bits(r.distances), off[f"dist{i}"])
        assert np.array_equal(r.counts, off[f"counts{i}"])
    alone = []
    for j in (0, 1):
        e.g.search_dev(qdev[j], LOOP_SIZES[j], K, **KW)
        alone.append(last_rows(e))
    e.g.search_dev_begin(0, qdev[0], LOOP_SIZES[0], K, **KW)
    e.g.search_dev_begin(1, qdev[1], LOOP_SIZES[1], K, **KW)
    a, b = e.g.search_dev_end(0), e.g.search_dev_end(1)
    assert np.array_equal(a.ids, off["a_ids"]) and np.array_equal(b.ids, off["b_ids"])
    assert last_rows(e) == alone[0] + alone[1]      # here: one chain for both
    assert int(off["rows_last"][0]) == alone[1]     # switched off: the last chain served the second batch alone
