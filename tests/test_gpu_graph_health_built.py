"""GPU: the graph-health job on a graph the device insert built, through deletes and a vacuum; that it disturbs nothing a
search sees; and the hybrid index's and the session's views of it."""
import numpy as np
import pytest

import fvdb_import
from _data import bits, mixture
from _graph_health_check import agrees

pytestmark = pytest.mark.gpu

N, D, M, M0, EFC = 3000, 8, 8, 16, 50


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    c = fv.Context(0)
    yield c
    c.close()


def built(fv, ctx, seed, row_dtype="f32"):
    x = mixture(N, D, n_comp=6, seed=seed)
    ids = np.arange(N, dtype=np.uint64) * 3 + 7
    h = fv.HNSWIndex(ctx, M, M0, EFC, seed=seed, row_dtype=row_dtype)
    assert h.batch_insert(ids, x) == (N, 0)
    assert h.insert_stats()["host_path_inserts"] == 0  # linked on the device: the host never held these lists
    return h, x, ids


@pytest.mark.parametrize("row_dtype", ["f32", "f16"])
def test_built_graph_through_deletes_and_a_vacuum(fv, ctx, row_dtype):
    h, x, ids = built(fv, ctx, 41, row_dtype)
    got, _ = agrees(fv, h, "device")
    assert got["n_live"] == N and got["dangling"] == 0
    rng = np.random.default_rng(5)
    dead = rng.choice(N, int(0.4 * N), replace=False)
    for r in dead:
        h.mark_deleted(int(ids[r]))
    got, _ = agrees(fv, h, "device")
    assert got["n_live"] == N - dead.size and got["dangling"] > 0
    # the point of the bound: a node outside R is returned by no search, its own vector as the query included
    lost = h.unreachable_ids()
    assert lost.size == got["unreachable_live"]
    if lost.size:
        row_of = {int(i): r for r, i in enumerate(ids)}
        res = h.search(x[[row_of[int(i)] for i in lost]], 10, 200)
        for b, i in enumerate(lost):
            assert int(i) not in res.ids[b, :int(res.counts[b])].tolist()
    removed = h.vacuum()
    assert removed == dead.size
    got, _ = agrees(fv, h, "device")  # by id, on the new export
    assert got["dangling"] == 0 and got["dangling0"] == 0 and got["n_nodes"] == got["n_live"] == N - dead.size


def test_no_interference(fv, ctx):
    h, x, ids = built(fv, ctx, 43)
    for r in range(0, N, 5):
        h.mark_deleted(int(ids[r]))
    q = mixture(16, D, n_comp=6, seed=44)
    allowed = ids[1::2]
    h.scan_cutoff = 0  # the masked traversal, whose mask a change to the graph would invalidate
    before = h.search(q, 10, 64), h.search_allowed(q, 10, 64, allowed)
    builds, ties, fallbacks = h.mask_builds(), h.tie_restarts(), h.device_fallbacks()
    assert builds >= 1
    health = h.graph_health()
    assert health["path"] == "device" and health["n_live"] == N - len(range(0, N, 5))
    assert h.unreachable_ids().size == health["unreachable_live"] and h.component_labels()[1].size == N
    assert h.tie_restarts() == ties and h.device_fallbacks() == fallbacks  # the traversal's counters are not the job's
    after = h.search(q, 10, 64), h.search_allowed(q, 10, 64, allowed)
    for a, b in zip(before, after):
        assert np.array_equal(a.counts, b.counts) and np.array_equal(a.ids, b.ids)
        assert np.array_equal(bits(a.distances), bits(b.distances))
    assert h.mask_builds() == builds  # the cached mask is still valid: the job is no mutation
    assert h.device_fallbacks() == fallbacks


def test_hybrid_and_session_views(fv, ctx):
    n, d = 400, 8
    x = mixture(n, d, n_comp=4, seed=46)
    hyb = fv.HybridIndex(ctx, max_connections=8, max_connections_layer_0=16, ef_construction=40, hnsw_seed=3)
    hyb.initialize(x[:64])
    for i in range(n):
        hyb.insert(1000 + i, x[i], now=0.0)
    for i in range(0, n, 3):
        hyb.delete(1000 + i, now=0.0)
    got, _ = agrees(fv, hyb.hnsw(), "device")
    assert got["n_nodes"] == n and got["n_live"] == n - len(range(0, n, 3))

    s = fv.VectorDbSession(ctx, max_connections=8, max_connections_layer_0=16, ef_construction=40)
    s.add_vectors([{"id": f"doc-{i}", "vector": x[i].tolist(), "metadata": {}} for i in range(200)])
    for i in range(0, 200, 4):
        s.delete_vector(f"doc-{i}")
    a, b = s.index.hnsw().graph_health(), s.graph_health()
    how = ("ms",)  # a duration: the one field two runs of the same job do not share
    assert {k: v for k, v in a.items() if k not in how} == {k: v for k, v in b.items() if k not in how}
    assert b["path"] == "device" and b["n_live"] == 150 and b["n_nodes"] == 200
    assert sorted(s.get_stats()) == ["hnsw_deleted_count", "hnsw_vector_count", "index_type", "ivf_deleted_count",
                                     "ivf_vector_count", "total_deleted_count", "vector_count"]
