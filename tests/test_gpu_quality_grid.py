"""GPU: search quality over a grid of ef and n_probe from one exact search, through the index
classes and the session.  Every entry of a grid must equal, in the bits of avg_recall and avg_precision, what the
single-point call it replaces returns for that pair: evaluate_search_quality (its wide form above k = 256), or, where
that call has no such option (one part switched off), the host recomputation of _exact_ref.host_quality on search()
against search_exact().

The graph is the one of test_graph_quality_equals_the_host_recomputation (2000 x 8, one Gaussian, M 16), the hybrid index
the one of test_hybrid_quality_equals_the_host_recomputation_with_duplicate_ids (900 x 16, 9 lists, half the rows due
for migration a day later)."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture
import _exact_ref as R

pytestmark = pytest.mark.gpu

E_DIM, E_INVALID, E_UNSUPPORTED = 3, 6, 12
DAY = 86400.0
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def same_figures(got_recall, got_precision, want, what):
    print(f"{what}: grid {got_recall}, {got_precision}; single call {want['avg_recall']}, {want['avg_precision']}")
    assert bits(got_recall) == bits(want["avg_recall"]), f"{what}: recall {got_recall} vs {want['avg_recall']}"
    assert bits(got_precision) == bits(want["avg_precision"]), f"{what}: precision {got_precision} vs {want['avg_precision']}"


# ---- the graph --------------------------------------------------------------------------------------------------------
N_GRAPH, D_GRAPH = 2000, 8
EFS = (50, 10, 2000, 10)


@pytest.fixture(scope="module")
def graph(fv, ctx):
    x = mixture(N_GRAPH, D_GRAPH, n_comp=1, seed=41)
    x[N_GRAPH // 2 + 1] = x[2]
    ids = np.arange(N_GRAPH, dtype=np.uint64) + 100
    g = fv.HNSWIndex(ctx, 16, 32, 100, seed=41)
    assert g.batch_insert(ids, x, orc.rng_levels(41, N_GRAPH)) == (N_GRAPH, 0)
    return g, mixture(40, D_GRAPH, n_comp=1, seed=42)


@pytest.mark.parametrize("k", [10, 300])
def test_recall_by_ef_equals_the_single_calls(graph, k):
    g, q = graph
    curve = g.recall_by_ef(q, k, EFS)
    assert curve["efs"] == list(EFS) and curve["queries_evaluated"] == 40 and curve["avg_query_time_ms"] > 0
    assert curve["avg_recall"].shape == (4,) and curve["avg_precision"].dtype == np.float32
    single = g.evaluate_search_quality if k <= 256 else g.evaluate_search_quality_wide
    for i, ef in enumerate(EFS):
        same_figures(curve["avg_recall"][i], curve["avg_precision"][i], single(q, k, ef), f"k={k} ef={ef}")
    assert bits(curve["avg_recall"][1]) == bits(curve["avg_recall"][3]), "a repeated ef gives the same figures"
    assert len(set(bits(curve["avg_recall"]).tolist())) >= 3, "the listed efs do not differ in recall: the test shows nothing"


def test_smallest_ef(graph):
    g, q = graph
    assert g.smallest_ef(q, 10, 1.0, EFS) == 2000
    assert g.smallest_ef(q, 10, 1.0, (50, 10)) is None
    assert g.smallest_ef(q, 10, 0.0, EFS) == 10
    low = float(g.recall_by_ef(q, 10, (10,))["avg_recall"][0])
    assert g.smallest_ef(q, 10, low, (2000, 50, 10)) == 10  # reached exactly: compared in f32


def test_graph_sub_batches_change_nothing(graph, monkeypatch):
    g, q = graph
    q = np.concatenate([q, mixture(10, D_GRAPH, n_comp=1, seed=43)])  # B = 50
    k = 10
    monkeypatch.delenv("FVDB_QUALITY_GRID_BYTES", raising=False)
    whole = g.recall_by_ef(q, k, EFS)
    # a query of this grid: truth k * 8 + 4, per ef k * 16 + 8, per pair 8 bytes; room for 20 of them: 20 + 20 + 10
    per_query = k * 8 + 4 + len(EFS) * (k * 16 + 8) + len(EFS) * 8
    for budget in (20 * per_query, 1):  # 1: one query per sub-batch
        monkeypatch.setenv("FVDB_QUALITY_GRID_BYTES", str(budget))
        parts = g.recall_by_ef(q, k, EFS)
        assert np.array_equal(bits(parts["avg_recall"]), bits(whole["avg_recall"])), f"budget {budget}"
        assert np.array_equal(bits(parts["avg_precision"]), bits(whole["avg_precision"])), f"budget {budget}"


# ---- the hybrid index -------------------------------------------------------------------------------------------------
N_HYB, D_HYB, NLIST, K = 900, 16, 9, 10
HEFS, NPROBES = (10, 20, 60), (1, 2, 9, 20)
LOW_EFS = (1, 3, 60)  # below k = 10 the recent part holds at most ef rows
NOW = 500 * DAY
LATER = NOW + DAY


def hybrid_rows():
    x = mixture(N_HYB, D_HYB, n_comp=6, seed=51)
    q = np.concatenate([mixture(20, D_HYB, n_comp=6, seed=52), x[[0, 2, 4]]])
    return x, q


def build_hybrid(fv, ctx, dtype, trained=True):
    x, _ = hybrid_rows()
    ids = np.arange(N_HYB, dtype=np.uint64)
    age = np.where(np.arange(N_HYB) % 2 == 0, 6.5 * DAY, 40 * DAY)
    h = fv.HybridIndex(ctx, max_connections=6, max_connections_layer_0=12, ef_construction=40, n_clusters=NLIST, n_probe=2,
                       row_dtype=dtype)
    if trained:
        h.set_ivf_centroids(x[:NLIST])
        h.bulk_insert(ids, x, NOW - age, NOW)
    else:
        h.initialize(x[:5])  # fewer rows than min_ivf_training_size: the graph alone
        assert not h.is_ivf_trained()
        h.bulk_insert(ids[::2], x[::2], NOW - age[::2], NOW)
    return h


@pytest.fixture(scope="module", params=["f32", "f16"])
def hybrid(request, fv, ctx):
    """the index AFTER its first quality_grid call at LATER, which took the migration step, with that call's result"""
    h = build_hybrid(fv, ctx, request.param)
    _, q = hybrid_rows()
    before = h.historical_count()
    grid = h.quality_grid(q, K, HEFS, NPROBES, now=LATER)
    assert h.historical_count() > before and h.historical_count() > N_HYB // 2, "the grid call did not take the migration step"
    return h, q, grid


def test_quality_grid_equals_the_single_calls(hybrid):
    h, q, grid = hybrid
    assert grid["efs"] == list(HEFS) and grid["n_probes"] == list(NPROBES)
    assert grid["avg_recall"].shape == (3, 4) and grid["avg_precision"].shape == (3, 4)
    assert grid["queries_evaluated"] == q.shape[0] and grid["avg_query_time_ms"] > 0
    for i, ef in enumerate(HEFS):
        for j, p in enumerate(NPROBES):
            want = h.evaluate_search_quality(q, K, now=LATER, hnsw_ef=ef, ivf_n_probe=p)
            same_figures(grid["avg_recall"][i, j], grid["avg_precision"][i, j], want, f"{h.row_dtype} ef={ef} n_probe={p}")
    # a migrated row still sits in the graph: some result holds an id twice, and the grid counted it twice
    res = h.search(q, K, now=LATER, hnsw_ef=20, ivf_n_probe=2)
    assert any(len(set(res.ids[b, :res.counts[b]].tolist())) < res.counts[b] for b in range(q.shape[0])), "no duplicate id"
    # n_probe 9 and 20 both search every list
    assert np.array_equal(bits(grid["avg_recall"][:, 2]), bits(grid["avg_recall"][:, 3]))
    assert len(set(bits(grid["avg_recall"][0]).tolist())) >= 2, "the columns do not differ: the test shows nothing"
    # On a graph of 450 nodes every ef >= k may find the same rows; an ef below k returns at most ef rows, so these rows
    # of the grid must differ
    low = h.quality_grid(q, K, LOW_EFS, (2, 9), now=LATER)
    for i, ef in enumerate(LOW_EFS):
        for j, p in enumerate((2, 9)):
            want = h.evaluate_search_quality(q, K, now=LATER, hnsw_ef=ef, ivf_n_probe=p)
            same_figures(low["avg_recall"][i, j], low["avg_precision"][i, j], want, f"{h.row_dtype} ef={ef} n_probe={p}")
    assert len(set(bits(low["avg_recall"][:, 0]).tolist())) >= 2, "the rows do not differ: the test shows nothing"
    # the same call again (no migration left to take) gives the same grid
    again = h.quality_grid(q, K, HEFS, NPROBES, now=LATER)
    assert np.array_equal(bits(again["avg_recall"]), bits(grid["avg_recall"]))
    assert np.array_equal(bits(again["avg_precision"]), bits(grid["avg_precision"]))


def host_figures(h, q, k, ef, p, **parts):
    res = h.search(q, k, now=LATER, hnsw_ef=ef, ivf_n_probe=p, **parts)
    truth = h.search_exact(q, k, now=LATER, **parts)
    ar, ap = R.host_quality(res, truth, k)
    return dict(avg_recall=ar, avg_precision=ap)


def test_one_part_switched_off(hybrid):
    h, q, _ = hybrid
    grid = h.quality_grid(q, K, HEFS, NPROBES, now=LATER, search_recent=False)
    assert grid["avg_recall"].shape == (3, 4)
    for j, p in enumerate(NPROBES):
        want = host_figures(h, q, K, 50, p, search_recent=False)
        for i in range(len(HEFS)):  # every row is the historical-only value
            same_figures(grid["avg_recall"][i, j], grid["avg_precision"][i, j], want, f"historical only, n_probe={p}, row {i}")
    lists_only = h.quality_grid(q, K, (), NPROBES, now=LATER, search_recent=False)  # the recent list may then be empty
    assert lists_only["avg_recall"].shape == (1, 4)
    assert np.array_equal(bits(lists_only["avg_recall"][0]), bits(grid["avg_recall"][0]))
    grid = h.quality_grid(q, K, HEFS, NPROBES, now=LATER, search_historical=False)
    for i, ef in enumerate(HEFS):
        want = host_figures(h, q, K, ef, 10, search_historical=False)
        for j in range(len(NPROBES)):  # every column is the recent-only value
            same_figures(grid["avg_recall"][i, j], grid["avg_precision"][i, j], want, f"recent only, ef={ef}, column {j}")
    # neither part: every result and the truth are empty
    grid = h.quality_grid(q, K, HEFS, NPROBES, now=LATER, search_recent=False, search_historical=False)
    assert np.all(grid["avg_recall"] == 1) and np.all(grid["avg_precision"] == 0)


def test_untrained_lists_leave_every_column_the_recent_only_value(fv, ctx):
    h = build_hybrid(fv, ctx, "f32", trained=False)
    _, q = hybrid_rows()
    for efs in (HEFS, LOW_EFS):
        grid = h.quality_grid(q, K, efs, NPROBES, now=NOW)
        for i, ef in enumerate(efs):
            want = h.evaluate_search_quality(q, K, now=NOW, hnsw_ef=ef, ivf_n_probe=2)
            for j in range(len(NPROBES)):
                same_figures(grid["avg_recall"][i, j], grid["avg_precision"][i, j], want, f"untrained, ef={ef}, column {j}")
    assert len(set(bits(grid["avg_recall"][:, 0]).tolist())) >= 2, "the rows do not differ: the test shows nothing"


def test_hybrid_sub_batches_change_nothing(hybrid, monkeypatch):
    h, q, _ = hybrid
    q = np.concatenate([q, mixture(27, D_HYB, n_comp=6, seed=53)])  # B = 50
    monkeypatch.delenv("FVDB_QUALITY_GRID_BYTES", raising=False)
    whole = h.quality_grid(q, K, HEFS, NPROBES, now=LATER)
    # a query of this grid: truth k * 8 + 4, per listed ef and n_probe k * 16 + 8, per pair 8 bytes; room for 20: 20 + 20 + 10
    per_query = K * 8 + 4 + (len(HEFS) + len(NPROBES)) * (K * 16 + 8) + len(HEFS) * len(NPROBES) * 8
    monkeypatch.setenv("FVDB_QUALITY_GRID_BYTES", str(20 * per_query))
    parts = h.quality_grid(q, K, HEFS, NPROBES, now=LATER)
    assert np.array_equal(bits(parts["avg_recall"]), bits(whole["avg_recall"]))
    assert np.array_equal(bits(parts["avg_precision"]), bits(whole["avg_precision"]))
    for ef, p in ((20, 2), (60, 9)):
        want = h.evaluate_search_quality(q, K, now=LATER, hnsw_ef=ef, ivf_n_probe=p)
        i, j = HEFS.index(ef), NPROBES.index(p)
        same_figures(parts["avg_recall"][i, j], parts["avg_precision"][i, j], want, f"three sub-batches, ef={ef} n_probe={p}")


def test_operating_points_come_from_the_grid(fv, hybrid):
    h, q, grid = hybrid
    target = float(grid["avg_recall"][1, 1])  # reached by (20, 2) exactly
    pts = h.operating_points(q, K, target, HEFS, NPROBES, now=LATER)
    assert pts == fv.index.pareto_points(grid, target) and pts, "operating_points is the Pareto set of quality_grid"
    assert [p["ef"] for p in pts] == sorted(p["ef"] for p in pts)
    for p in pts:
        i, j = HEFS.index(p["ef"]), NPROBES.index(p["n_probe"])
        assert bits(p["avg_recall"]) == bits(grid["avg_recall"][i, j]) and p["avg_recall"] >= np.float32(target)
    assert not any(p["n_probe"] == 20 for p in pts), "n_probe 20 never beats n_probe 9 on nine lists"
    assert h.operating_points(q, K, 2.0, HEFS, NPROBES, now=LATER) == []


# ---- the session ------------------------------------------------------------------------------------------------------
def test_session_quality_grid_agrees_with_the_index_call(fv, ctx):
    x, q = hybrid_rows()
    now = 100 * DAY
    s = fv.VectorDbSession(ctx, now=now, max_connections=6, max_connections_layer_0=12, ef_construction=40, n_clusters=NLIST)
    try:
        s.index.set_ivf_centroids(x[:NLIST])
        ids = np.arange(N_HYB, dtype=np.uint64) + 1
        s.index.bulk_insert(ids[:600], x[:600], np.full(600, now - 30 * DAY), now)
        s.add_vectors([{"id": f"doc-{i}", "vector": x[600 + i].tolist(), "metadata": {}} for i in range(120)])
        a = s.quality_grid([v.tolist() for v in q], K, list(HEFS), list(NPROBES))
        b = s.index.quality_grid(q, K, HEFS, NPROBES, now=s.now)
        assert a["efs"] == list(HEFS) and a["n_probes"] == list(NPROBES) and a["queries_evaluated"] == q.shape[0]
        assert np.array_equal(bits(a["avg_recall"]), bits(b["avg_recall"]))
        assert np.array_equal(bits(a["avg_precision"]), bits(b["avg_precision"]))
        one = s.evaluate_search_quality([v.tolist() for v in q], K, {"hnswEf": 20, "ivfNProbe": 2})
        same_figures(a["avg_recall"][1, 1], a["avg_precision"][1, 1], one, "session, ef=20 n_probe=2")
        with pytest.raises(fv.session.SessionError):
            s.quality_grid([], K, HEFS, NPROBES)
        with pytest.raises(fv.session.SessionError, match="dimension"):
            s.quality_grid([[0.0] * (D_HYB + 1)], K, HEFS, NPROBES)
    finally:
        s.destroy()
    with pytest.raises(fv.session.SessionError, match="destroyed"):
        s.quality_grid([v.tolist() for v in q], K, HEFS, NPROBES)


# ---- refusals, in the order the design states -------------------------------------------------------------------------
def raw_grid(h, q, B, dim, k, efs, n_probes, sr=1, sh=1, out=True):
    """fvh_hybrid_quality_grid with nothing checked on the way down"""
    e, p = np.asarray(efs, np.uint32), np.asarray(n_probes, np.uint32)
    r = np.zeros(max(e.size, 1) * max(p.size, 1), np.float32)
    pr = np.zeros_like(r)
    return h.lib.fvh_hybrid_quality_grid(h.h, None if q is None else q.ctypes.data_as(f32p), B, dim, k, sr, sh, 0, 0,
                                         e.ctypes.data_as(u32p) if e.size else None, e.size,
                                         p.ctypes.data_as(u32p) if p.size else None, p.size, LATER,
                                         r.ctypes.data_as(f32p) if out else None, pr.ctypes.data_as(f32p), None, None)


def test_hybrid_refusals_in_order(fv, ctx, hybrid):
    h, q, _ = hybrid
    B, d = q.shape
    wrong = np.ascontiguousarray(mixture(B, d + 4, n_comp=4, seed=62))
    # 1. a sharded index, whatever else is wrong with the call
    x, _ = hybrid_rows()
    s = fv.HybridIndex(ctx, max_connections=4, max_connections_layer_0=8, ef_construction=16, n_clusters=4, n_probe=2)
    s.set_ivf_centroids(x[:4])
    ids = np.arange(200, dtype=np.uint64)
    s.bulk_insert_sharded(ids, x[:200], NOW - np.where(ids % 2 == 0, DAY, 30 * DAY), NOW, 0, 2)
    with pytest.raises(fv.Unsupported, match="sharded") as e:
        s.quality_grid(q, K, HEFS, NPROBES, now=NOW)
    assert e.value.status == E_UNSUPPORTED
    with pytest.raises(fv.Unsupported, match="sharded"):
        s.operating_points(q, K, 0.9, HEFS, NPROBES, now=NOW)
    assert raw_grid(s, q, B, d, K, HEFS, NPROBES) == E_UNSUPPORTED  # the host mirror refuses by itself too
    assert raw_grid(s, None, 0, d + 4, 0, (), ()) == E_UNSUPPORTED   # ... before anything else
    # 2. no queries, null pointers, no listed value for a part that is searched: before k and the dimension
    assert raw_grid(h, q, 0, d + 4, 0, HEFS, NPROBES) == E_INVALID
    assert raw_grid(h, None, B, d + 4, 0, HEFS, NPROBES) == E_INVALID
    assert raw_grid(h, q, B, d + 4, 0, HEFS, NPROBES, out=False) == E_INVALID
    assert raw_grid(h, q, B, d + 4, 0, (), NPROBES) == E_INVALID
    assert raw_grid(h, q, B, d + 4, 0, HEFS, ()) == E_INVALID
    assert raw_grid(h, q, B, d, K, (), NPROBES, sr=0) == 0 and raw_grid(h, q, B, d, K, HEFS, (), sh=0) == 0
    with pytest.raises(fv.InvalidConfig):
        h.quality_grid(np.zeros((0, d), np.float32), K, HEFS, NPROBES, now=LATER)
    with pytest.raises(fv.InvalidConfig):
        h.quality_grid(q, K, (), NPROBES, now=LATER)
    # 3. k, before the dimension
    for k in (0, 4097):
        assert raw_grid(h, wrong, B, d + 4, k, HEFS, NPROBES) == E_UNSUPPORTED
        with pytest.raises(fv.Unsupported):
            h.quality_grid(q, k, HEFS, NPROBES, now=LATER)
    assert raw_grid(h, q, B, d, K, [10] * 65, NPROBES) == E_UNSUPPORTED
    # 4. the dimension, before any search runs
    assert raw_grid(h, wrong, B, d + 4, K, HEFS, NPROBES) == E_DIM
    assert raw_grid(h, wrong, B, d + 4, K, (0,), (0,)) == E_DIM
    with pytest.raises(fv.DimensionMismatch):
        h.quality_grid(wrong, K, HEFS, NPROBES, now=LATER)
    # 5. what the underlying search refuses comes back as that search's code
    with pytest.raises(fv.FvdbError) as e:
        h.quality_grid(q, K, HEFS, (2, 0), now=LATER)
    assert e.value.status == h.lib.fvh_ivf_search(
        h.ivf().h, q.ctypes.data_as(f32p), B, d, K, 0, np.empty((B, K), np.uint64).ctypes.data_as(u64p),
        np.empty((B, K), np.float32).ctypes.data_as(f32p), np.zeros(B, np.uint32).ctypes.data_as(u32p)) != 0
    with pytest.raises(fv.Unsupported):
        h.quality_grid(q, K, (20, 0), NPROBES, now=LATER)  # ef = 0: the traversal's own refusal


def test_graph_refusals_in_order(fv, graph):
    g, q = graph
    B, d = q.shape
    wrong = np.ascontiguousarray(mixture(B, d + 4, n_comp=1, seed=62))

    def raw(qq, B_, dim, k, efs, out=True):
        e = np.asarray(efs, np.uint32)
        r, pr = np.zeros(max(e.size, 1), np.float32), np.zeros(max(e.size, 1), np.float32)
        return g.lib.fvh_hnsw_quality_by_ef(g.h, None if qq is None else qq.ctypes.data_as(f32p), B_, dim, k,
                                            e.ctypes.data_as(u32p) if e.size else None, e.size,
                                            r.ctypes.data_as(f32p) if out else None, pr.ctypes.data_as(f32p), None, None)

    assert raw(q, 0, d + 4, 0, EFS) == E_INVALID
    assert raw(None, B, d + 4, 0, EFS) == E_INVALID
    assert raw(q, B, d + 4, 0, ()) == E_INVALID
    assert raw(q, B, d + 4, 0, EFS, out=False) == E_INVALID
    for k in (0, 4097):
        assert raw(wrong, B, d + 4, k, EFS) == E_UNSUPPORTED
    assert raw(q, B, d, 10, [10] * 65) == E_UNSUPPORTED
    assert raw(wrong, B, d + 4, 10, EFS) == E_DIM
    with pytest.raises(fv.InvalidConfig):
        g.recall_by_ef(np.zeros((0, d), np.float32), 10, EFS)
    with pytest.raises(fv.InvalidConfig):
        g.recall_by_ef(q, 10, ())
    with pytest.raises(fv.Unsupported):
        g.recall_by_ef(q, 4097, EFS)
    with pytest.raises(fv.DimensionMismatch):
        g.recall_by_ef(wrong, 10, EFS)
    with pytest.raises(fv.Unsupported):
        g.recall_by_ef(q, 10, (10, 0))  # ef = 0: the traversal's own refusal
