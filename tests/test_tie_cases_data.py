"""What test_gpu_tie_rules.py rests on, checked on the CPU with the oracle alone: the hand-built cases of _tie_cases.py
tie where they say and nowhere else, a search that the table lets finish without a restart has an answer that does not
depend on which of the tied nodes a list names first (that is what makes a restart-free answer legitimate, whatever the
kernel does), every family holds a restart-expected case whose answer does depend on it, and the table is what the
rules restated in Python give.  The lattice graphs of the fuzz are checked the same way: the restated rule leaves between
1 and B - 1 queries per batch to the restated heaps, so neither side of the rule runs empty there."""
import functools

import numpy as np
import pytest

import oracle as orc
import _tie_cases as tc
from _data import bits

ALL = [c for case in tc.CASES for c in tc.both(case)]
NAMES = [c.name for c in ALL]


@functools.lru_cache(maxsize=None)
def _built():
    orc.build()
    return True


def oracle_of(case, d=8, rows=None):
    """the oracle with the case's graph restored (M, M0, ef_construction = 4, 8, ef), its ids and the origin query"""
    _built()
    x, ids, levels, off, nbrs, entry, q = tc.graph(case, d)
    o = orc.HNSWIndex(4, 8, case.ef, seed=1)
    o.restore(ids, x if rows is None else rows(x), levels, off, nbrs, entry)
    return o, ids, q


def oracle_answer(case, search, d=8):
    """(nodes, distance bits) of the oracle's search of the origin"""
    o, ids, q = oracle_of(case, d)
    for i in search.deleted:
        o.mark_deleted(int(ids[i]))
    oi, od, oc = o.batch_search(q[None], search.k, case.ef)
    c = int(oc[0])
    return (oi[0, :c].astype(np.int64) - tc.ID_BASE).tolist(), bits(od[0, :c]).tolist()


def oracle_lists_after_insert(case, d=8):
    """layer-0 lists after the origin row went in at level 0: the new node's first, then node by node"""
    o, ids, q = oracle_of(case, d)
    o.insert(tc.INSERT_ID, q, 0)
    assert o.level(tc.INSERT_ID) == 0 and o.entry_point() == int(ids[-1] if case.top else ids[0])
    node = lambda v: -1 if v == tc.INSERT_ID else v - tc.ID_BASE
    return [[node(v) for v in o.neighbors(int(i), 0)] for i in [tc.INSERT_ID] + ids.tolist()]


def test_every_case_has_a_mirror_and_the_rows_are_exact_in_fp16():
    assert len(set(NAMES)) == len(NAMES) == 2 * len(tc.CASES)
    for case in tc.CASES:
        plain, mirror = tc.both(case)
        assert (plain.adj != mirror.adj) != (plain.coords != mirror.coords), case.name
        assert sorted(map(sorted, plain.adj)) == sorted(map(sorted, mirror.adj)), case.name
        for d in (8, 384):
            x = tc.graph(case, d)[0]
            assert np.array_equal(x, x.astype(np.float16).astype(np.float32)) and np.array_equal(x * 8, np.round(x * 8))
        assert len(case.adj) == len(case.coords) and max(map(len, case.adj)) <= 6  # one more link stays below M0 = 8
        for i, row in enumerate(case.adj):
            assert i not in row and len(set(row)) == len(row) and max(row) < len(case.adj), (case.name, i)
        assert {s.family for s in case.searches} <= {"twin", "max", "cut"}
    # all three outcomes of the table are there: finished, restarted, and both for one case at different k
    assert any(not s.restart for c in ALL for s in c.searches) and any(s.restart for c in ALL for s in c.searches)


@pytest.mark.parametrize("case", ALL, ids=NAMES)
def test_the_tied_nodes_and_no_others_have_bit_equal_distances(case):
    _built()
    for d in (8, 384):
        x, ids, levels, off, nbrs, entry, q = tc.graph(case, d)
        db = bits(orc.l2_batch(q, x))
        assert np.array_equal(db, bits(tc.distances(case).astype(np.float32))), "a distance is not |(x, y)| exactly"
        groups = {}
        for i, v in enumerate(db.tolist()):
            groups.setdefault(v, []).append(i)
        assert sorted(tuple(g) for g in groups.values() if len(g) > 1) == sorted(tuple(sorted(t)) for t in case.ties)
    assert set(case.tied) <= {i for t in case.ties for i in t}


@pytest.mark.parametrize("case", [tc.plain(c) for c in tc.CASES], ids=[c.name for c in tc.CASES])
def test_a_search_that_may_finish_does_not_depend_on_the_exchange(case):
    mirror = tc.exchanged(tc.BY_NAME[case.name])
    for s, sm in zip(case.searches, mirror.searches):
        a, b = oracle_answer(case, s), oracle_answer(mirror, sm)
        assert len(a[0]) == min(s.k, len(case.coords) - len(s.deleted))
        if case.name == "E1":  # no two members ever share a place in a heap: list order is the input, and it decides
            assert not s.restart and not sm.restart and a[0] == [0, 3] and b[0] == [0, 4] and a[1] != b[1]
        elif not (s.restart and sm.restart):
            # the same nodes — not merely the same up to renaming the tied ones, which are in no such answer — and bits
            assert a == b, (case.name, s, a, b)
            assert not set(a[0]) & {i for t in case.ties for i in t}, (case.name, s, a)


def test_every_family_has_a_restart_whose_answer_depends_on_the_exchange():
    depends = {"twin": [], "max": [], "cut": []}
    for case in tc.CASES:
        plain, mirror = tc.both(case)
        for s, sm in zip(plain.searches, mirror.searches):
            if s.restart and sm.restart and oracle_answer(plain, s)[0] != oracle_answer(mirror, sm)[0]:
                depends[s.family].append((case.name, s.k))
    print(depends)
    assert ("T1", 4) in depends["twin"] and ("M3", 3) in depends["max"] and ("T1", 3) in depends["cut"], depends


@pytest.mark.parametrize("case", [tc.plain(c) for c in tc.CASES], ids=[c.name for c in tc.CASES])
def test_an_insert_that_may_finish_does_not_depend_on_the_exchange(case):
    mirror = tc.exchanged(tc.BY_NAME[case.name])
    a, b = oracle_lists_after_insert(case), oracle_lists_after_insert(mirror)
    assert a[0] == sorted(a[0], key=lambda v: tc.distances(case)[v]) and 0 < len(a[0]) <= case.ef
    for v in a[0]:  # linked back, nothing pruned
        assert a[1 + v] == (case.adj + [[0]])[v] + [-1]
    if case.name == "E1":
        assert not case.insert_restart and a[0] == [0, 3] and b[0] == [0, 4]
    elif not (case.insert_restart and mirror.insert_restart):
        assert b == tc.exchange_lists(case, a), (case.name, a, b)
        assert not set(a[0]) & {i for t in case.ties for i in t}


@pytest.mark.parametrize("case", ALL, ids=NAMES)
def test_the_table_is_the_rule_restated(case):
    tc.EVENTS.clear()
    for s in case.searches:
        restart, nodes = tc.restated_search(case, s.k, s.deleted)
        assert restart == s.restart, (case.name, s)
        if not restart:  # where the rule lets the sorted list answer, it answers as the heaps do
            assert nodes == oracle_answer(case, s)[0], (case.name, s)
    assert tc.EVENTS["twin"] + tc.EVENTS["amb"] + tc.EVENTS["ended"] > 0 or case.name.startswith("E1"), "the case meets no tie at the top of a heap"
    assert tc.restated_insert(case) == case.insert_restart
    # The sorted list's lane swap (an expanded member trades places with the unexpanded one in the last lane) is met by
    # no case, and cannot be: a newcomer goes in front of its equals and a pop takes the lowest lane, so the expanded one of
    # two equals in front of an unexpanded one was popped as a twin, and what its expansion admits below the pair's
    # distance ends the attempt (d < twin_d) before anything leaves.  The set form of the insert has no such order.
    assert tc.EVENTS["swap"] == 0


@functools.lru_cache(maxsize=None)
def lattice_prediction(seed):
    """per (k, ef) of the fuzz: how many of the batch's queries the restated rule sends to the restated heaps; every
    answer it lets the sorted list give is checked against the oracle's on the way"""
    _built()
    x, ids, levels, off, nbrs, entry, dead, lists = tc.lattice_graph(seed, 8)
    q = tc.lattice_queries(seed, 8)
    o = orc.HNSWIndex(4, 8, 8, seed=1)
    o.restore(ids, x, levels, off, nbrs, entry)
    deleted = np.zeros(ids.size, bool)
    for i in dead:
        o.mark_deleted(int(i))
        deleted[int(i) - tc.ID_BASE] = True
    dist = np.stack([orc.l2_batch(row, x) for row in q])
    out = {}
    for k, ef in tc.LATTICE_K_EF:
        oi, od, oc = o.batch_search(q, k, ef)
        restarts = 0
        for b in range(q.shape[0]):
            restart, nodes = tc.restated_walk(dist[b], lists, deleted, 0, ef, k)
            restarts += restart
            if not restart:
                assert nodes == (oi[b, :oc[b]].astype(np.int64) - tc.ID_BASE).tolist(), (seed, k, ef, b)
        out[(k, ef)] = restarts
    return out


@pytest.mark.parametrize("seed", tc.LATTICE_SEEDS)
def test_the_lattice_leaves_work_to_both_sides_of_the_rule(seed):
    x, ids, levels, off, nbrs, entry, dead, lists = tc.lattice_graph(seed, 384)
    assert len(tc.LATTICE_SEEDS) >= 8 and x.shape == (64, 384) and not x[:, 2:].any() and np.abs(x).max() <= 4
    assert dead.size == (8 if seed % 2 else 0) and int(ids[0]) not in dead.tolist()
    for i, row in enumerate(lists):
        assert (i + 1) % 64 in row and i not in row and len(set(row)) == len(row) and 1 <= len(row) <= 7
    tc.EVENTS.clear()
    got = lattice_prediction(seed)
    print(seed, got, dict(tc.EVENTS))
    for (k, ef), restarts in got.items():
        if ef == 1:
            assert restarts == 0
        else:
            assert 1 <= restarts <= tc.LATTICE_B - 1, (seed, k, ef, restarts)
