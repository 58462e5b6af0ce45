"""GPU: exact search at k up to 4096 over the graph and the hybrid index, and search quality on top of it (DESIGN.md
section 9q).

Ids, distance bits and counts of every wide exact search must equal the numpy restatement of the reference's distance
and of the result rule (_exact_ref.py, proven against the oracle in test_exact_search_symbols.py); the hand-built cases
come from _exact_wide_cases.py, whose stated properties test_exact_wide_data.py proves on the CPU.  Shapes are the
smallest at which the two kernels can go wrong: row counts around the 64-row tile, a graph of 71 tiles whose last one is
part-filled, k at both ends, at 256 / 257 and above the live count, a tie group that holds the cut, batches that leave a
query group part-filled, arenas forced into several sub-batches.

The scan reads the row store and the liveness flags, never the links, so its graphs are installed with restore() as a
ring; the tests that also traverse build theirs with the device insert."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture
import _exact_ref as R
import _exact_wide_cases as W

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = 6, 12
DAY = 86400.0
NO_ID = R.NO_ID
WIDE_KS = (1, 10, 256, 257, 1000, 4096)


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def ring_graph(fv, ctx, ids, x, dtype):
    """an HNSWIndex holding rows x under ids, node i = row i; links: a ring on layer 0 (the scan never reads them)"""
    n = len(ids)
    g = fv.HNSWIndex(ctx, 4, 8, 16, seed=1, row_dtype=dtype)
    if n == 1:
        g.insert(int(ids[0]), x[0], 0)
    else:
        g.restore(ids, x, np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64), np.roll(ids, -1), int(ids[0]))
    return g


def same(got, want, what=""):
    wi, wd, wc = want
    assert np.array_equal(got.counts, wc), f"{what}: counts differ: {got.counts[:8]} vs {wc[:8]}"
    assert np.array_equal(got.ids, wi), f"{what}: ids differ (first bad query {np.flatnonzero((got.ids != wi).any(1))[:3]})"
    assert np.array_equal(bits(got.distances), bits(wd)), f"{what}: distances are not bit-identical"


def triple(r):
    return r.ids, r.distances, r.counts


# ---- 1. tile and arena edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", [(130, "f32"), (10, "f16")])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_graphs_around_the_tile_size_and_k_above_the_live_count(fv, ctx, n, d, dtype):
    x = mixture(n, d, n_comp=4, seed=n + d)
    if n > 2:
        x[n - 1] = x[0]  # a tie between the first and the last lane in use
    ids = np.arange(n, dtype=np.uint64) * 3 + 5
    q = np.concatenate([mixture(4, d, n_comp=4, seed=n), x[:1]])
    g = ring_graph(fv, ctx, ids, x, dtype)
    dist = R.fold_distances(q, W.stored(x, dtype))
    for k in (1, 10, 257, 4096):
        got = g.search_exact_wide(q, k)
        same(got, R.exact_topk(dist, k, ids=ids), f"n={n} k={k}")
        m = min(n, k)
        assert np.all(got.counts == m)
        # the padding words of the last tile (63 of them at n = 65) are never results
        assert np.all(got.ids[:, m:] == NO_ID) and np.all(np.isposinf(got.distances[:, m:]))
        assert np.all(np.isfinite(got.distances[:, :m]))


# ---- 2. the cut inside the graph, 3. register path = wide path --------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("d", [10, 130, 384])
def test_wide_scan_equals_the_reference_fold_and_the_register_path(fv, ctx, d, dtype):
    x, ids, q, dist = W.cut_case(d, dtype)
    g = ring_graph(fv, ctx, ids, x, dtype)
    for rows in (slice(29, 30), slice(27, 32), slice(0, 33)):  # B = 1, 5, 33: every one holds a query on a duplicated row
        for k in WIDE_KS:
            what = f"d={d} {dtype} B={rows.stop - rows.start} k={k}"
            got = g.search_exact_wide(q[rows], k)
            same(got, R.exact_topk(dist[rows], k, ids=ids), what)
            if k <= 256:
                same(got, triple(g.search_exact(q[rows], k)), what + ": wide vs register path")
    # the ties are there, and the lower node index wins
    top = g.search_exact_wide(q[29:33], 3)
    assert list(top.ids[0]) == [1010, 1011, 1012] and list(top.ids[1, :2]) == [1255, 1256]
    assert list(top.ids[2, :2]) == [1700, 3100] and list(top.ids[3, :2]) == [1003, 1004]


# ---- 4. ties at the cut -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_tie_group_at_the_cut_is_taken_in_node_order(fv, ctx, dtype):
    x, ids, v, q_on, q_50 = W.tie_case(dtype)
    dist = W.tie_dist(dtype)
    g = ring_graph(fv, ctx, ids, x, dtype)
    group = ids[W.GROUP]
    # (a) the query ON the vector: 600 words of bits 0, the lowest node indices win
    for k in (1, 257, 600, 601):
        got = g.search_exact_wide(q_on[None], k)
        same(got, R.exact_topk(dist[0:1], k, ids=ids), f"(a) k={k}")
        m = min(k, 600)
        assert list(got.ids[0, :m]) == list(group[:m]) and np.all(bits(got.distances[0, :m]) == 0)
    # (b) exactly 50 rows are strictly nearer; inside the group the result is nodes 100, 101, ... in order
    for k in (50, 51, 257, 649, 650, 651):
        got = g.search_exact_wide(q_50[None], k)
        same(got, R.exact_topk(dist[1:2], k, ids=ids), f"(b) k={k}")
        m = min(k, 650) - 50
        assert list(got.ids[0, 50:50 + m]) == list(group[:m])
        assert not set(got.ids[0, :50].tolist()) & set(group.tolist())
    # both queries in one batch
    same(g.search_exact_wide(np.stack([q_on, q_50]), 300), R.exact_topk(dist, 300, ids=ids), "(a)+(b) k=300")


def test_a_graph_of_identical_rows(fv, ctx):
    x, ids, q, dist = W.same_rows_case()
    g = ring_graph(fv, ctx, ids, x, "f32")
    for k in (1, 64, 299, 300, 301):
        got = g.search_exact_wide(q, k)
        same(got, R.exact_topk(dist, k, ids=ids), f"(c) k={k}")
        m = min(k, 300)
        assert np.all(got.ids[:, :m] == ids[:m]) and np.all(got.counts == m)


# ---- 5. liveness ------------------------------------------------------------------------------------------------------
def built_graph(fv, ctx, n, d, seed, dtype="f32", n_comp=6, M=6, efc=40):
    x = mixture(n, d, n_comp=n_comp, seed=seed)
    x[n // 2 + 1] = x[2]
    ids = np.arange(n, dtype=np.uint64) + 100
    g = fv.HNSWIndex(ctx, M, 2 * M, efc, seed=seed, row_dtype=dtype)
    assert g.batch_insert(ids, x, orc.rng_levels(seed, n)) == (n, 0)
    return g, ids, x


def test_deleted_nodes_are_never_returned_and_vacuum_renumbers(fv, ctx):
    n, d = 300, 10
    g, ids, x = built_graph(fv, ctx, n, d, seed=5)
    q = np.concatenate([mixture(8, d, n_comp=6, seed=6), x[2:3]])
    dist = R.fold_distances(q, x)
    live = np.ones(n, bool)
    live[1::3] = False  # a third of the nodes; node 0 (the entry point) stays
    for i in ids[~live]:
        g.mark_deleted(int(i))
    for k in (10, 257):
        same(g.search_exact_wide(q, k), R.exact_topk(dist, k, live=live, ids=ids), f"a third deleted, k={k}")
    assert g.vacuum() == int((~live).sum())
    for k in (10, 257):
        same(g.search_exact_wide(q, k), R.exact_topk(dist, k, live=live, ids=ids), f"after vacuum, k={k}")


def test_every_node_deleted_gives_counts_of_zero(fv, ctx):
    n, d = 130, 10
    x = mixture(n, d, n_comp=4, seed=8)
    ids = np.arange(n, dtype=np.uint64)
    g = ring_graph(fv, ctx, ids, x, "f32")
    for i in ids:
        g.mark_deleted(int(i))
    for k in (10, 300):
        got = g.search_exact_wide(mixture(5, d, n_comp=4, seed=9), k)
        assert np.all(got.counts == 0) and np.all(got.ids == NO_ID) and np.all(np.isposinf(got.distances))
    # and an index that never held a row
    got = fv.HNSWIndex(ctx, 4, 8, 16).search_exact_wide(mixture(5, d, n_comp=4, seed=9), 300)
    assert np.all(got.counts == 0) and np.all(got.ids == NO_ID)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_allow_sets_of_one_row_seventy_rows_and_every_row(fv, ctx, dtype):
    n, d = 700, 130
    x = R.with_duplicates(mixture(n, d, n_comp=6, seed=21), [(4, 6), (4, 300), (255, 257)])
    ids = np.arange(n, dtype=np.uint64) + 50
    g = ring_graph(fv, ctx, ids, x, dtype)
    for i in ids[5::7]:
        g.mark_deleted(int(i))
    live = np.ones(n, bool)
    live[5::7] = False
    q = np.concatenate([mixture(9, d, n_comp=6, seed=22), x[[4, 255]]])
    dist = R.fold_distances(q, W.stored(x, dtype))
    for name, nodes in (("one row", np.array([4])), ("70 rows", np.arange(0, n, 10)), ("every row", np.arange(n))):
        allowed_nodes = np.zeros(n, bool)
        allowed_nodes[nodes] = True
        allowed = np.concatenate([ids[allowed_nodes], np.array([7, 10 ** 9], np.uint64)])  # two ids the index does not hold
        for k in (1, 10, 300):
            got = g.search_exact_wide_allowed(q, k, allowed)
            same(got, R.exact_topk(dist, k, live=live & allowed_nodes, ids=ids), f"allowed: {name}, k={k}")
            if k <= 256:
                same(got, triple(g.search_exact_allowed(q, k, allowed)), f"allowed: {name}, k={k}: wide vs register path")
    none = g.search_exact_wide_allowed(q, 300, np.array([7], np.uint64))
    assert np.all(none.counts == 0) and np.all(none.ids == NO_ID)


def c_call(fv, ctx, gh, mask, q, k, q_dev=None):
    """fvdb_graph_search_flat_wide_dev_slot through ctypes: (status, SearchResults with node indices as ids)"""
    B = q.shape[0]
    own = q_dev is None
    if own:
        q_dev = ctx.upload(q)
    out = (ctx.alloc(B * k * 4), ctx.alloc(B * k * 4), ctx.alloc(B * 4))
    rc = ctx.lib.fvdb_graph_search_flat_wide_dev_slot(gh, None, 0, mask, q_dev, B, k, *out)
    got = None
    if rc == 0:
        ctx.synchronize()
        got = fv.index.SearchResults(ctx.download(out[0], (B, k), np.uint32).astype(np.uint64),
                                     ctx.download(out[1], (B, k), np.float32), ctx.download(out[2], (B,), np.uint32))
    for p in out + ((q_dev,) if own else ()):
        ctx.free(p)
    return rc, got


def as_nodes(want):
    """a reference triple with ids = node indices, as the C entry point writes them: NO_ROW is 32 bits wide"""
    wi, wd, wc = want
    wi = wi.copy()
    wi[wi == NO_ID] = np.uint64(0xFFFFFFFF)
    return wi, wd, wc


def test_c_entry_point_under_a_mask_and_its_refusals(fv, ctx):
    n, d = 200, 16
    x = mixture(n, d, n_comp=4, seed=61)
    ids = np.arange(n, dtype=np.uint64)
    g = ring_graph(fv, ctx, ids, x, "f32")
    q = mixture(4, d, n_comp=4, seed=62)
    lib, gh = ctx.lib, g._graph()
    nodes = np.ascontiguousarray(np.arange(0, n, 2, dtype=np.uint32))
    mask = C.c_void_p()
    ctx.check(lib.fvdb_mask_create_graph(gh, nodes.ctypes.data_as(C.POINTER(C.c_uint32)), nodes.size, C.byref(mask)))
    allowed = np.zeros(n, bool)
    allowed[::2] = True
    dist = R.fold_distances(q, x)
    for k in (5, 300):  # 300 > the 100 allowed nodes
        rc, got = c_call(fv, ctx, gh, mask, q, k)
        assert rc == 0
        same(got, as_nodes(R.exact_topk(dist, k, live=allowed)), f"the C entry point under a mask, k={k}")
    rc, got = c_call(fv, ctx, gh, None, q, 300)
    assert rc == 0
    same(got, as_nodes(R.exact_topk(dist, 300)), "the C entry point without a mask")
    for k in (0, 4097):
        rc, _ = c_call(fv, ctx, gh, mask, q, k)
        assert rc == E_UNSUPPORTED and b"FVDB_MAX_K_WIDE" in lib.fvdb_last_error(ctx.h)
    other = ring_graph(fv, ctx, ids[:70], x[:70], "f32")
    rc, _ = c_call(fv, ctx, other._graph(), mask, q, 5)
    assert rc == E_INVALID and b"another graph" in lib.fvdb_last_error(ctx.h)
    g.mark_deleted(int(ids[1]))
    rc, _ = c_call(fv, ctx, gh, mask, q, 5)
    assert rc == E_INVALID and b"stale mask" in lib.fvdb_last_error(ctx.h)
    lib.fvdb_mask_destroy(mask)


# ---- 6. sub-batches ---------------------------------------------------------------------------------------------------
def test_forced_sub_batches_change_nothing(fv, ctx, monkeypatch):
    n, d = 2891, 10  # 46 tiles: 2944 arena words = 11776 bytes per query
    x = R.with_duplicates(mixture(n, d, n_comp=8, seed=71), [(3, 4), (255, 256)])
    ids = np.arange(n, dtype=np.uint64) + 9
    q = np.concatenate([mixture(31, d, n_comp=8, seed=72), x[[3, 255]]])
    assert q.shape[0] == 33
    g = ring_graph(fv, ctx, ids, x, "f32")
    dist = R.fold_distances(q, x)
    monkeypatch.delenv("FVDB_FLAT_WIDE_ARENA_BYTES", raising=False)
    plain = {k: g.search_exact_wide(q, k) for k in (10, 300)}
    for k, got in plain.items():
        same(got, R.exact_topk(dist, k, ids=ids), f"unforced, k={k}")
    # room for 12 queries: sub-batches of 12, 12 and 9; then one word: one query per sub-batch
    for budget in (12 * 2944 * 4, 4):
        monkeypatch.setenv("FVDB_FLAT_WIDE_ARENA_BYTES", str(budget))
        assert 33 * 2944 * 4 > 2 * max(budget, 2944 * 4), "at least three sub-batches"
        for k in (10, 300):
            same(g.search_exact_wide(q, k), triple(plain[k]), f"arena budget {budget}, k={k}")


# ---- 7. the hybrid index ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_hybrid_exact_wide_is_the_merge_of_the_two_exact_parts(fv, ctx, dtype):
    n, d, nlist, k = 800, 24, 8, 300
    x = mixture(n, d, n_comp=8, seed=31)
    ids = np.arange(n, dtype=np.uint64) + 10
    now = 1000 * DAY
    age = np.where(np.arange(n) % 2 == 0, 5 * DAY, 30 * DAY)  # 400 recent rows, 400 historical ones: both parts cross 256
    age[:60:2] = 6.5 * DAY                                    # recent now, due for migration half a day later
    h = fv.HybridIndex(ctx, max_connections=6, max_connections_layer_0=12, ef_construction=40, n_clusters=nlist,
                       n_probe=3, row_dtype=dtype)
    h.set_ivf_centroids(x[:nlist])
    h.bulk_insert(ids, x, now - age, now)
    recent = np.flatnonzero(age < 7 * DAY)
    assert h.recent_count() == recent.size == 400
    xs = W.stored(x, dtype)
    q = np.concatenate([mixture(8, d, n_comp=8, seed=32), x[[0, 2, 4]]])  # three queries on rows about to migrate

    def check(now_):
        both = h.search_exact_wide(q, k, now=now_)
        r = h.search_exact_wide(q, k, now=now_, search_historical=False)
        hi = h.search_exact_wide(q, k, now=now_, search_recent=False)
        same(r, R.exact_topk(R.fold_distances(q, xs[recent]), k, ids=ids[recent]), "recent-only")
        same(r, triple(h.hnsw().search_exact_wide(q, k)), "recent-only vs the graph's own search_exact_wide")
        every = h.ivf().search(q, k, n_probe=nlist)
        same(hi, triple(every), "historical-only vs the every-list search")
        assert np.all(r.counts == k) and np.all(hi.counts == k)
        for b in range(q.shape[0]):
            wi, wd = R.merge_parts([(r.ids[b, :r.counts[b]], r.distances[b, :r.counts[b]]),
                                    (hi.ids[b, :hi.counts[b]], hi.distances[b, :hi.counts[b]])], k)
            assert both.counts[b] == wi.size
            assert np.array_equal(both.ids[b, :wi.size], wi) and np.array_equal(bits(both.distances[b, :wi.size]), bits(wd))
        return both

    check(now)
    # at k <= 256 the wide form is the register form
    same(h.search_exact_wide(q, 10, now=now), triple(h.search_exact(q, 10, now=now)), "hybrid k=10: wide vs register path")
    hist_before = h.historical_count()
    later = now + 1 * DAY  # rows 0, 2, .., 58 are now 7.5 days old: the search's own migration step copies them to the lists
    both = check(later)
    assert h.historical_count() > hist_before
    # a migrated row still sits in the graph: it is returned twice, as search() returns it
    assert list(both.ids[8, :2]) == [10, 10]


# ---- 8. search quality ------------------------------------------------------------------------------------------------
def test_graph_quality_wide_equals_the_host_recomputation(fv, ctx):
    n, d, k = 2000, 8, 300
    g, ids, x = built_graph(fv, ctx, n, d, seed=41, n_comp=1, M=16, efc=100)
    q = mixture(40, d, n_comp=1, seed=42)
    truth = g.search_exact_wide(q, k)
    same(truth, R.exact_topk(R.fold_distances(q, x), k, ids=ids), "the truth itself")
    for ef in (2000, 10):
        res = g.search(q, k, ef)
        sq = g.evaluate_search_quality_wide(q, k, ef)
        ar, ap = R.host_quality(res, truth, k)
        print(f"ef={ef}: avg_recall={sq['avg_recall']} avg_precision={sq['avg_precision']} host={ar},{ap}")
        assert sq["queries_evaluated"] == 40 and sq["avg_query_time_ms"] > 0
        assert bits(sq["avg_recall"]) == bits(ar), f"ef={ef}: recall {sq['avg_recall']} vs host {ar}"
        assert bits(sq["avg_precision"]) == bits(ap), f"ef={ef}: precision {sq['avg_precision']} vs host {ap}"
    # at k = 10 the wide form is evaluate_search_quality
    for ef in (2000, 10):
        a, b = g.evaluate_search_quality_wide(q, 10, ef), g.evaluate_search_quality(q, 10, ef)
        assert bits(a["avg_recall"]) == bits(b["avg_recall"]) and bits(a["avg_precision"]) == bits(b["avg_precision"])
        assert a["queries_evaluated"] == b["queries_evaluated"]


def test_hybrid_quality_wide_equals_the_host_recomputation(fv, ctx):
    n, d, nlist, k = 2000, 16, 9, 300
    x = mixture(n, d, n_comp=1, seed=51)
    ids = np.arange(n, dtype=np.uint64)
    now = 500 * DAY
    age = np.where(np.arange(n) % 2 == 0, 6.5 * DAY, 40 * DAY)
    h = fv.HybridIndex(ctx, max_connections=16, max_connections_layer_0=32, ef_construction=100, n_clusters=nlist, n_probe=2)
    h.set_ivf_centroids(x[:nlist])
    h.bulk_insert(ids, x, now - age, now)
    q = np.concatenate([mixture(20, d, n_comp=1, seed=52), x[[0, 2, 4]]])
    later = now + DAY  # a migration is due: the evaluation takes that step once, then both searches see the same rows
    for ef in (2000, 10):
        sq = h.evaluate_search_quality_wide(q, k, now=later, hnsw_ef=ef, ivf_n_probe=2)
        res = h.search(q, k, now=later, hnsw_ef=ef, ivf_n_probe=2)
        truth = h.search_exact_wide(q, k, now=later)
        ar, ap = R.host_quality(res, truth, k)
        print(f"hybrid ef={ef}: avg_recall={sq['avg_recall']} avg_precision={sq['avg_precision']} host={ar},{ap}")
        assert sq["queries_evaluated"] == q.shape[0]
        assert bits(sq["avg_recall"]) == bits(ar) and bits(sq["avg_precision"]) == bits(ap)
    a = h.evaluate_search_quality_wide(q, 10, now=later, hnsw_ef=20, ivf_n_probe=2)
    b = h.evaluate_search_quality(q, 10, now=later, hnsw_ef=20, ivf_n_probe=2)
    assert bits(a["avg_recall"]) == bits(b["avg_recall"]) and bits(a["avg_precision"]) == bits(b["avg_precision"])


# ---- 9. errors --------------------------------------------------------------------------------------------------------
def test_errors(fv, ctx):
    n, d = 200, 16
    x = mixture(n, d, n_comp=4, seed=61)
    ids = np.arange(n, dtype=np.uint64)
    g = ring_graph(fv, ctx, ids, x, "f32")
    q = mixture(4, d, n_comp=4, seed=62)
    for k in (0, 4097):
        for call in (lambda: g.search_exact_wide(q, k), lambda: g.search_exact_wide_allowed(q, k, ids[:5]),
                     lambda: g.evaluate_search_quality_wide(q, k, 50)):
            with pytest.raises(fv.Unsupported) as e:
                call()
            assert e.value.status == E_UNSUPPORTED
    with pytest.raises(fv.DimensionMismatch):
        g.search_exact_wide(mixture(4, d + 4, n_comp=4, seed=62), 300)
    with pytest.raises(fv.DimensionMismatch):
        g.evaluate_search_quality_wide(mixture(4, d + 4, n_comp=4, seed=62), 300, 50)
    with pytest.raises(fv.InvalidConfig):
        g.evaluate_search_quality_wide(np.zeros((0, d), np.float32), 300, 50)
    # the hybrid forms: k, the dimension, an empty query set, a sharded index
    h = fv.HybridIndex(ctx, max_connections=4, max_connections_layer_0=8, ef_construction=16, n_clusters=4, n_probe=2)
    h.set_ivf_centroids(x[:4])
    now = 100 * DAY
    h.bulk_insert(ids, x, now - np.where(ids % 2 == 0, DAY, 30 * DAY), now)
    for k in (0, 4097):
        for call in (lambda: h.search_exact_wide(q, k, now=now), lambda: h.evaluate_search_quality_wide(q, k, now=now)):
            with pytest.raises(fv.Unsupported):
                call()
    with pytest.raises(fv.DimensionMismatch):
        h.search_exact_wide(mixture(4, d + 4, n_comp=4, seed=62), 300, now=now)
    with pytest.raises(fv.InvalidConfig):
        h.evaluate_search_quality_wide(np.zeros((0, d), np.float32), 300, now=now)
    s = fv.HybridIndex(ctx, max_connections=4, max_connections_layer_0=8, ef_construction=16, n_clusters=4, n_probe=2)
    s.set_ivf_centroids(x[:4])
    s.bulk_insert_sharded(ids, x, now - np.where(ids % 2 == 0, DAY, 30 * DAY), now, 0, 2)
    for call in (lambda: s.search_exact_wide(q, 300, now=now), lambda: s.evaluate_search_quality_wide(q, 300, now=now)):
        with pytest.raises(fv.Unsupported, match="sharded") as e:
            call()
        assert e.value.status == E_UNSUPPORTED
    # the host mirror refuses by itself too
    ids_o, ds_o, cnt_o = np.empty((4, 300), np.uint64), np.empty((4, 300), np.float32), np.zeros(4, np.uint32)
    rc = s.lib.fvh_hybrid_search_exact_wide(s.h, q.ctypes.data_as(C.POINTER(C.c_float)), 4, d, 300, 1, 1, float(now),
                                            ids_o.ctypes.data_as(C.POINTER(C.c_uint64)), ds_o.ctypes.data_as(C.POINTER(C.c_float)),
                                            cnt_o.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == E_UNSUPPORTED
