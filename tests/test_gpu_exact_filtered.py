"""GPU: the filtered route of the exact search — an fp16 matrix-core filter over a mirror of the
graph's rows, the survivors scored by the reference's fold — must return the ids, distance bits, counts and padding of the
numpy restatement (_exact_ref.py), ties to the lower node.  Shapes: rows around the 32-row block and the 512-row slice,
widths around the 16-dimension step of the matrix instruction and at both ends of the query-operand placement (LDS up to
d = 384 here, HBM at 2048), batches around the 32-query tile, every k class.  Graphs are rings installed with restore():
the scan reads rows and liveness flags, never links."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture
import _exact_ref as R

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = 6, 12
DAY = 86400.0
BK = [(1, 1), (33, 10), (70, 65), (3, 256)]


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def stored(x, dtype):
    return R.rounded(x) if dtype == "f16" else np.asarray(x, np.float32)


def ring_graph(fv, ctx, ids, x, dtype="f32"):
    n = len(ids)
    g = fv.HNSWIndex(ctx, 4, 8, 16, seed=1, row_dtype=dtype)
    if n == 1:
        g.insert(int(ids[0]), x[0], 0)
    else:
        g.restore(ids, x, np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64), np.roll(ids, -1), int(ids[0]))
    return g


def same(got, want, what):
    wi, wd, wc = want
    assert np.array_equal(got.counts, wc), f"{what}: counts differ: {got.counts[:8]} vs {wc[:8]}"
    assert np.array_equal(got.ids, wi), f"{what}: ids differ (first bad query {np.flatnonzero((got.ids != wi).any(1))[:3]})"
    assert np.array_equal(bits(got.distances), bits(wd)), f"{what}: distances are not bit-identical"


def check_all(g, q, dist, ids, what, live=None, allowed=None):
    for B, k in BK:
        got = g.search_exact_filtered(q[:B], k, allowed=allowed)
        same(got, R.exact_topk(dist[:B], k, live=live, ids=ids), f"{what} B={B} k={k}")


def case(n, d, dtype, seed=0):
    x = mixture(n, d, n_comp=8, seed=seed + d + n)
    ids = np.arange(n, dtype=np.uint64) + 1000
    q = mixture(70, d, n_comp=8, seed=seed + d + n + 1)
    return x, ids, q, R.fold_distances(q, stored(x, dtype))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, None, 3000])
def test_row_counts_around_block_and_slice(fv, ctx, n, dtype):
    if n is None:  # one slice and one row: the least at which two workgroups share a query
        tiny = ring_graph(fv, ctx, np.arange(2, dtype=np.uint64), mixture(2, 33, n_comp=1, seed=1))
        tiny.search_exact_filtered(mixture(1, 33, n_comp=1, seed=2), 1)
        n = tiny.exact_filter_info()["min_slice_rows"] + 1
    x, ids, q, dist = case(n, 33, dtype)
    g = ring_graph(fv, ctx, ids, x, dtype)
    check_all(g, q, dist, ids, f"n={n} {dtype}")  # k = 256 and 65 are above the live count of the small graphs
    got = g.search_exact_filtered(q[:3], 256)
    m = min(n, 256)
    assert np.all(got.ids[:, m:] == R.NO_ID) and np.all(np.isposinf(got.distances[:, m:]))
    info = g.exact_filter_info()
    assert info["mirror_rows"] == n and info["rebuilds"] == 0 and info["unbounded_queries"] == 0


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("d", [10, 16, 17, 384, 2048])
def test_widths_around_the_instruction_step_and_the_lds_limit(fv, ctx, d, dtype):
    x, ids, q, dist = case(3000, d, dtype)
    g = ring_graph(fv, ctx, ids, x, dtype)
    check_all(g, q, dist, ids, f"d={d} {dtype}")
    info = g.exact_filter_info()
    assert info["lds_bytes"][2] <= info["lds_limit"] and info["queries_in_lds"][0] == (d <= 384)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_deleted_nodes_and_allow_sets(fv, ctx, dtype):
    n = 3000
    x, ids, q, dist = case(n, 33, dtype, seed=5)
    g = ring_graph(fv, ctx, ids, x, dtype)
    third = np.zeros(n, bool)
    third[::3] = True
    check_all(g, q, dist, ids, "allow-set", live=third, allowed=ids[third])
    live = np.ones(n, bool)
    live[1::3] = False
    for i in ids[~live]:
        g.mark_deleted(int(i))
    check_all(g, q, dist, ids, "a third deleted", live=live)
    check_all(g, q, dist, ids, "deleted and allow-set", live=live & third, allowed=ids[third])
    small = ring_graph(fv, ctx, ids[:130], x[:130], dtype)
    for i in ids[:130]:
        small.mark_deleted(int(i))
    got = small.search_exact_filtered(q[:5], 10)
    assert np.all(got.counts == 0) and np.all(got.ids == R.NO_ID) and np.all(np.isposinf(got.distances))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_ties_across_a_block_and_a_slice_boundary_go_to_the_lower_node(fv, ctx, dtype):
    n, d = 3000, 33
    x = R.with_duplicates(mixture(n, d, n_comp=8, seed=7), [(31, 32), (511, 512), (40, 2900)])
    ids = np.arange(n, dtype=np.uint64) + 1000
    q = np.concatenate([x[[31, 511, 40]], mixture(30, d, n_comp=8, seed=8)])
    g = ring_graph(fv, ctx, ids, x, dtype)
    dist = R.fold_distances(q, stored(x, dtype))
    for k in (1, 2, 10):
        same(g.search_exact_filtered(q, k), R.exact_topk(dist, k, ids=ids), f"duplicates k={k}")
    assert list(g.search_exact_filtered(q[:3], 1).ids[:, 0]) == [1031, 1511, 1040]
    top = g.search_exact_filtered(q[:3], 2)
    assert top.ids.tolist() == [[1031, 1032], [1511, 1512], [1040, 3900]]
    assert np.array_equal(bits(top.distances[:, 0]), bits(top.distances[:, 1]))


def test_near_ties_overflow_every_arena_and_the_answer_stays_exact(fv, ctx):
    n, d, B = 3000, 384, 6
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(d) + 1e-3 * rng.standard_normal((n, d))).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64)
    q = rng.standard_normal((B, d)).astype(np.float32)
    g = ring_graph(fv, ctx, ids, x)
    same(g.search_exact_filtered(q, 10), R.exact_topk(R.fold_distances(q, x), 10, ids=ids), "near ties")
    info = g.exact_filter_info()
    assert info["fallback_queries"] == B and info["unbounded_queries"] == 0 and info["exact_pairs"] >= B * n


def test_rows_beyond_the_fp16_range_are_answered_over_all_rows(fv, ctx):
    n, d, B = 700, 33, 5
    x, ids, q, _ = case(n, d, "f32", seed=13)
    x, q = x * np.float32(1e5), q * np.float32(1e5)
    assert np.abs(x).max() > 65504
    g = ring_graph(fv, ctx, ids, x)
    same(g.search_exact_filtered(q[:B], 10), R.exact_topk(R.fold_distances(q[:B], x), 10, ids=ids), "scaled by 1e5")
    info = g.exact_filter_info()
    assert info["unbounded_queries"] == B and info["fallback_queries"] == 0 and info["exact_pairs"] == B * n


def test_the_mirror_extends_after_an_append_and_rebuilds_after_a_vacuum(fv, ctx):
    n, extra, d = 300, 100, 33
    x = mixture(n + extra, d, n_comp=6, seed=17)
    ids = np.arange(n + extra, dtype=np.uint64) + 100
    q = mixture(33, d, n_comp=6, seed=18)
    dist = R.fold_distances(q, x)
    g = fv.HNSWIndex(ctx, 6, 12, 40, seed=17)
    levels = orc.rng_levels(17, n + extra)
    assert g.batch_insert(ids[:n], x[:n], levels[:n]) == (n, 0)
    same(g.search_exact_filtered(q, 10), R.exact_topk(dist[:, :n], 10, ids=ids[:n]), "before the append")
    assert g.exact_filter_info()["mirror_rows"] == n
    assert g.batch_insert(ids[n:], x[n:], levels[n:]) == (extra, 0)
    same(g.search_exact_filtered(q, 10), R.exact_topk(dist, 10, ids=ids), "after the append")
    info = g.exact_filter_info()
    assert info["mirror_rows"] == n + extra and info["build_rows"] == extra and info["rebuilds"] == 0
    live = np.ones(n + extra, bool)
    live[1::3] = False
    live[levels == levels.max()] = True  # the entry point stays, so the vacuum reclaims the rows and renumbers the nodes
    for i in ids[~live]:
        g.mark_deleted(int(i))
    assert g.vacuum() == int((~live).sum()) and g.vacuum_info()["path"] == "resident"
    same(g.search_exact_filtered(q, 10), R.exact_topk(dist, 10, live=live, ids=ids), "after the vacuum")
    info = g.exact_filter_info()
    assert info["mirror_rows"] == int(live.sum()) and info["rebuilds"] == 1


def test_the_filter_drops_most_pairs_on_normal_rows(fv, ctx):
    """The cap is a condition: 2 E is about 2 here and the spread of |x - q|^2 about 55 around 768, so a handful of rows
    a slice lie within the margin of the k-th; a numpy emulation of the rounds gives 0.045 B n pairs and no overflow."""
    n, d, B, k = 3000, 384, 70, 10
    rng = np.random.default_rng(0)
    x, q = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((B, d)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64)
    g = ring_graph(fv, ctx, ids, x)
    same(g.search_exact_filtered(q, k), R.exact_topk(R.fold_distances(q, x), k, ids=ids), "normal rows")
    info = g.exact_filter_info()
    print(f"exact_pairs={info['exact_pairs']} of {B * n}, fallback_queries={info['fallback_queries']}")
    assert info["fallback_queries"] == 0 and info["exact_pairs"] < 0.5 * B * n


def test_refusals_leave_the_outputs_untouched(fv, ctx):
    n, B, k = 200, 4, 5
    lib = ctx.lib
    sentinel = np.full((B, 256), 0x5A5A5A5A, np.uint32)

    def refused(g, d, k, mask=None):
        q_dev = ctx.upload(mixture(B, d, n_comp=2, seed=3))
        out = [ctx.upload(sentinel) for _ in range(3)]
        rc = lib.fvdb_graph_search_flat_mfma_dev_slot(g._graph(), None, 0, mask, q_dev, B, k, *out)
        ctx.synchronize()
        assert all(np.array_equal(ctx.download(p, sentinel.shape, np.uint32), sentinel) for p in out)
        for p in out + [q_dev]:
            ctx.free(p)
        return rc

    ids = np.arange(n, dtype=np.uint64)
    g = ring_graph(fv, ctx, ids, mixture(n, 16, n_comp=4, seed=61))
    assert refused(g, 16, 0) == E_UNSUPPORTED and refused(g, 16, 257) == E_UNSUPPORTED
    wide = ring_graph(fv, ctx, ids[:4], mixture(4, 2049, n_comp=1, seed=62))
    assert refused(wide, 2049, k) == E_UNSUPPORTED and b"2048" in lib.fvdb_last_error(ctx.h)
    nodes = np.ascontiguousarray(np.arange(0, n, 2, dtype=np.uint32))
    mask = C.c_void_p()
    ctx.check(lib.fvdb_mask_create_graph(g._graph(), nodes.ctypes.data_as(C.POINTER(C.c_uint32)), nodes.size, C.byref(mask)))
    g.mark_deleted(1)
    assert refused(g, 16, k, mask) == E_INVALID and b"stale mask" in lib.fvdb_last_error(ctx.h)
    lib.fvdb_mask_destroy(mask)
    for bad in (0, 257):
        with pytest.raises(fv.Unsupported):
            g.search_exact_filtered(mixture(B, 16, n_comp=2, seed=3), bad)


def test_hybrid_filtered_equals_hybrid_exact(fv, ctx):
    n, d, nlist, k = 1200, 24, 12, 10
    x = mixture(n, d, n_comp=8, seed=31)
    ids = np.arange(n, dtype=np.uint64) + 10
    now = 1000 * DAY
    age = np.where(np.arange(n) % 3 == 0, 5 * DAY, 30 * DAY)  # 400 recent rows, 800 historical ones
    h = fv.HybridIndex(ctx, max_connections=6, max_connections_layer_0=12, ef_construction=40, n_clusters=nlist, n_probe=3)
    h.set_ivf_centroids(x[:nlist])
    h.bulk_insert(ids, x, now - age, now)
    q = np.concatenate([mixture(12, d, n_comp=8, seed=32), x[[0, 1, 2, 5]]])
    for kw in ({}, {"search_historical": False}):
        want = h.search_exact(q, k, now=now, **kw)
        same(h.search_exact_filtered(q, k, now=now, **kw), (want.ids, want.distances, want.counts), f"hybrid {kw}")
    assert h.hnsw().exact_filter_info()["mirror_rows"] == h.recent_count()
