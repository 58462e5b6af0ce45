"""GPU: the tie rules of the sorted-register searches, pinned branch by branch.

hnsw_search_fast_kernel (kernels_graph_fast.h) and the device insert's search (ef_search_layer<EXACT = false>,
kernels_graph_build.h) hand a query to the restated heaps only where equal distances meet at the top of a heap; the
branches that go on WITHOUT a restart — a benign twin pop, a benign tied maximum, a tie past the entries that are read —
answer themselves.  The hand-built graphs of _tie_cases.py walk into each branch by construction; per case the answer is
the oracle's bit for bit and the restart counter moves by exactly what the table says (0 or the whole batch), so a
kernel that restarted where it need not, or went on where it must not, fails here even when its answers are right.
The lattice fuzz is wide where the table is narrow: small integer coordinates, small ef, a few hundred queries per
batch of which some restart and some do not.  test_tie_cases_data.py checks the cases themselves on the CPU."""
import gc

import numpy as np
import pytest

import fvdb_import
import oracle as orc
import _tie_cases as tc
from _data import bits
from test_gpu_device_insert import same_graph
from test_tie_cases_data import ALL, NAMES, lattice_prediction

pytestmark = pytest.mark.gpu

B = 64
FORMS = [(8, "f32"), (384, "f32"), (384, "f16")]  # 384 dims: hnsw_search_fast_kernel<3, 16, true>, the headline form


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()
    gc.collect()


def restored(fv, ctx, case, d, dtype, deleted=()):
    """the case's graph in the index and in the oracle, (M, M0, ef_construction) = (4, 8, ef); the rows are exact in fp16"""
    x, ids, levels, off, nbrs, entry, q = tc.graph(case, d)
    gh, oh = fv.HNSWIndex(ctx, 4, 8, case.ef, seed=1, row_dtype=dtype), orc.HNSWIndex(4, 8, case.ef, seed=1)
    gh.restore(ids, x, levels, off, nbrs, entry)
    oh.restore(ids, x, levels, off, nbrs, entry)
    for i in deleted:
        gh.mark_deleted(int(ids[i]))
        oh.mark_deleted(int(ids[i]))
    return gh, oh, q


def warmed_up(gh, q, k, ef):
    """the counters' first zeroing is queued on another stream than the first search: deltas are taken after one search
    and one read"""
    assert gh.device_traversal()
    assert gh.search_info(q.shape[0], ef)["kernel"] == "sorted_register"
    gh.search(q, k, ef)
    gh.tie_restarts()


def counted(gh, q, k, ef):
    q0, r0 = gh.tie_restarts()
    got = gh.search(q, k, ef)
    q1, r1 = gh.tie_restarts()
    assert q1 - q0 == q.shape[0], "the batch was not served by the device traversal"
    return got, r1 - r0


def same_as_oracle(got, want, what):
    oi, od, oc = want
    assert np.array_equal(got.counts, oc), f"{what}: hit counts differ from the oracle's"
    live = np.arange(oi.shape[1])[None, :] < oc[:, None].astype(np.int64)
    bad = np.flatnonzero(((got.ids != oi) & live).any(axis=1))
    assert bad.size == 0, f"{what}: ids differ from the oracle's in {bad.size} queries, first {bad[:8]}"
    bad = np.flatnonzero(((bits(got.distances) != bits(od)) & live).any(axis=1))
    assert bad.size == 0, f"{what}: distances not bit-identical in {bad.size} queries, first {bad[:8]}"


@pytest.mark.parametrize("d,dtype", FORMS)
@pytest.mark.parametrize("case", ALL, ids=NAMES)
def test_hand_built_case_answers_and_restarts_as_the_table_says(fv, ctx, case, d, dtype):
    for deleted in sorted({s.deleted for s in case.searches}):
        gh, oh, q1 = restored(fv, ctx, case, d, dtype, deleted)
        q = np.repeat(q1[None], B, axis=0)
        warmed_up(gh, q, 1, case.ef)
        for s in case.searches:
            if s.deleted != deleted:
                continue
            what = f"{case.name} k {s.k} deleted {s.deleted}"
            got, restarts = counted(gh, q, s.k, case.ef)
            print(f"[tie_rules] case {case.name:5s} d {d:3d} {dtype} k {s.k} deleted {list(s.deleted)}: {restarts} of {B} restarted, "
                  f"table {B if s.restart else 0}")
            for f in ("ids", "distances", "counts"):
                a = getattr(got, f)
                assert np.array_equal(a, np.repeat(a[:1], B, axis=0)), f"{what}: the {B} copies of the query disagree in {f}"
            oi, od, oc = oh.batch_search(q[:1], s.k, case.ef)
            same_as_oracle(got, tuple(np.repeat(a, B, axis=0) for a in (oi, od, oc)), what)
            gh.set_device_traversal(False)
            host = gh.search(q, s.k, case.ef)
            gh.set_device_traversal(True)
            assert np.array_equal(host.counts, got.counts) and np.array_equal(host.ids, got.ids), f"{what}: host walk differs"
            assert np.array_equal(bits(host.distances), bits(got.distances)), f"{what}: host walk differs"
            assert restarts == (B if s.restart else 0), f"{what}: {restarts} of {B} queries restarted, the table says " \
                                                         f"{'all' if s.restart else 'none'} ({case.why})"
        assert gh.device_fallbacks() == 0
        del gh
    gc.collect()


@pytest.mark.parametrize("d,dtype", FORMS)
@pytest.mark.parametrize("seed", tc.LATTICE_SEEDS)
def test_lattice_fuzz_traversal(fv, ctx, seed, d, dtype):
    x, ids, levels, off, nbrs, entry, dead, lists = tc.lattice_graph(seed, d)
    q = tc.lattice_queries(seed, d)
    gh, oh = fv.HNSWIndex(ctx, 4, 8, 8, seed=1, row_dtype=dtype), orc.HNSWIndex(4, 8, 8, seed=1)
    gh.restore(ids, x, levels, off, nbrs, entry)
    oh.restore(ids, x, levels, off, nbrs, entry)
    for i in dead:
        gh.mark_deleted(int(i))
        oh.mark_deleted(int(i))
    warmed_up(gh, q, 1, 3)
    predicted = lattice_prediction(seed)
    for k, ef in tc.LATTICE_K_EF:
        assert gh.search_info(q.shape[0], ef)["kernel"] == "sorted_register"
        got, restarts = counted(gh, q, k, ef)
        print(f"[tie_rules] lattice seed {seed} d {d:3d} {dtype} deleted {dead.size} k {k} ef {ef}: {restarts} of {q.shape[0]} "
              f"restarted, restated rule {predicted[(k, ef)]}")
        same_as_oracle(got, oh.batch_search(q, k, ef), f"seed {seed} k {k} ef {ef}")
        if ef == 1:
            assert restarts == 0  # one member: no two of anything
        else:
            assert 1 <= restarts <= q.shape[0] - 1, f"seed {seed} k {k} ef {ef}: {restarts} restarts say nothing about one side"
        # the rule restated in Python (_tie_cases.py) decides every query of the batch the same way
        assert restarts == predicted[(k, ef)], f"seed {seed} k {k} ef {ef}: {restarts} restarts, the restated rule has " \
                                               f"{predicted[(k, ef)]}"
    assert gh.device_fallbacks() == 0
    del gh
    gc.collect()


@pytest.mark.parametrize("d,dtype", [(8, "f32"), (384, "f16")])
@pytest.mark.parametrize("case", ALL, ids=NAMES)
def test_hand_built_case_insert_links_and_restarts_as_the_table_says(fv, ctx, case, d, dtype):
    gh, oh, q = restored(fv, ctx, case, d, dtype)
    gh.set_device_insert(True, 1)
    before = gh.insert_stats()
    gh.insert(tc.INSERT_ID, q, 0)
    oh.insert(tc.INSERT_ID, q, 0)
    st = gh.insert_stats()
    assert st["host_path_inserts"] == 0 and st["n_done"] - before["n_done"] == 1
    restarts = st["tie_restarts"] - before["tie_restarts"]
    print(f"[tie_rules] insert case {case.name:5s} d {d:3d} {dtype}: {restarts} restart, table {int(case.insert_restart)}")
    same_graph(gh, oh)
    assert restarts == int(case.insert_restart), f"{case.name}: {restarts} restarts of the insert's search, the table says " \
                                                  f"{int(case.insert_restart)} ({case.why})"
    del gh
    gc.collect()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("M,M0,efc", [(4, 8, 4), (6, 12, 8), (6, 12, 40)])
def test_lattice_insert_builds_the_oracles_graph(fv, ctx, M, M0, efc, mode):
    n, seed = 300, efc
    x = tc.lattice_rows(seed, n)
    ids = np.arange(n, dtype=np.uint64) + tc.ID_BASE
    levels = orc.rng_levels(seed, n)
    gh, oh = fv.HNSWIndex(ctx, M, M0, efc, seed=seed), orc.HNSWIndex(M, M0, efc, seed=seed)
    gh.set_device_insert(True, mode)
    assert gh.batch_insert(ids, x, levels) == (n, 0)
    oh.batch_insert(ids, x, levels)
    st = gh.insert_stats()
    print(f"[tie_rules] lattice insert M {M} M0 {M0} ef_construction {efc} mode {mode}: {st['tie_restarts']} restarts in "
          f"{st['n_done']} device inserts, {st['host_path_inserts']} by the host algorithm")
    same_graph(gh, oh)
    assert st["host_path_inserts"] == 0 and st["n_done"] == n
    assert st["tie_restarts"] > 0
    del gh
    gc.collect()
