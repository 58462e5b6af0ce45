"""GPU: exact search over the graph and the hybrid index, and search quality on top of it.

Ids, distance bits and counts of every exact search must equal the numpy restatement of the reference's distance and of
the result rule (_exact_ref.py, proven against the oracle in test_exact_search_symbols.py) on the rows the test
inserted — `x.astype(float16).astype(float32)` for an fp16 index.  Shapes are the smallest at which the scan kernel can
go wrong: row counts around the 64-row tile, a graph of several row slices (so the merge runs), widths that are not a
multiple of the 32-dimension chunk nor of 16, batches that leave a query group part-filled, k at both ends.

The scan reads the row store and the liveness flags, never the links, so the graphs it is checked on are installed with
restore() as a ring (one neighbour per node): thousands of nodes in milliseconds.  The tests that also traverse
(search quality, the hybrid index, vacuum) build their graphs with the device insert."""
import ctypes as C
import functools

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture
import _exact_ref as R

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = 6, 12
DAY = 86400.0
NO_ID = R.NO_ID
DIMS = [10, 130, 384, 768]
DTYPES = ["f32", "f16"]
BIG = 2891  # 46 tiles of 64 rows, the last one part-filled: 12 slices of 4 tiles at every batch size used here


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


# ---- tile and slice edges, ties, both row elements --------------------------------------------------------------------
# duplicated rows: 2x, 3x, across the slice boundary at row 256, and far apart in different slices
DUPS = [(3, 4), (10, 11), (10, 12), (255, 256), (700, 2100)]


@functools.lru_cache(maxsize=None)
def big_case(d, dtype):
    x = R.with_duplicates(mixture(BIG, d, n_comp=8, seed=d), DUPS)
    ids = np.arange(BIG, dtype=np.uint64) + 1000
    xs = stored(x, dtype)
    # 29 free queries, then four ON duplicated rows: distance-0 ties, at the k = 1 cut and across a slice boundary
    # (x, not xs: an fp16 index keeps these queries f32, so their ties are between equal non-zero distances)
    q = np.concatenate([mixture(29, d, n_comp=8, seed=d + 1), x[[10, 255, 700, 3]]])
    return x, ids, q, R.fold_distances(q, xs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_scan_equals_the_reference_fold_at_every_batch_and_k(fv, ctx, d, dtype):
    x, ids, q, dist = big_case(d, dtype)
    g = ring_graph(fv, ctx, ids, x, dtype)
    assert g.row_dtype == dtype
    for rows in (slice(29, 30), slice(27, 32), slice(0, 33)):  # B = 1, 5, 33: every one holds a query on a duplicated row
        for k in (1, 10, 256):
            got = g.search_exact(q[rows], k)
            same(got, R.exact_topk(dist[rows], k, ids=ids), f"d={d} {dtype} B={rows.stop - rows.start} k={k}")
    # the ties are there, and the lower node index wins — at the k = 1 cut too, and across the slice boundary
    top = g.search_exact(q[29:33], 3)
    assert list(top.ids[0]) == [1010, 1011, 1012] and list(top.ids[1, :2]) == [1255, 1256]
    assert list(top.ids[2, :2]) == [1700, 3100] and list(top.ids[3, :2]) == [1003, 1004]
    assert bits(top.distances[0, 0]) == bits(top.distances[0, 2]) and bits(top.distances[1, 0]) == bits(top.distances[1, 1])
    assert list(g.search_exact(q[29:33], 1).ids[:, 0]) == [1010, 1255, 1700, 1003]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [10, 130])
def test_scan_equals_the_reference_fold_on_both_sides_of_each_list_width(fv, ctx, d, dtype):
    """k = 64 | 65 and 128 | 129: the widest list of one register per lane, both ends of the two-register list (the scan
    and the merge of k in 65..128 run nowhere else) and the first k of the four-register one"""
    x, ids, q, dist = big_case(d, dtype)
    g = ring_graph(fv, ctx, ids, x, dtype)
    for rows in (slice(27, 32), slice(0, 33)):  # B = 5, 33
        for k in (64, 65, 128, 129):
            got = g.search_exact(q[rows], k)
            same(got, R.exact_topk(dist[rows], k, ids=ids), f"d={d} {dtype} B={rows.stop - rows.start} k={k}")
    # under an allow-set the same kernels run with the mask's flags: 100 rows of every slice, duplicated ones among
    # them, k below and above their number
    nodes = np.concatenate([[10, 11, 12, 255, 256], np.arange(95) * 30 + 7])
    allowed_nodes = np.zeros(BIG, bool)
    allowed_nodes[nodes] = True
    assert allowed_nodes.sum() == 100
    for k in (65, 128):
        got = g.search_exact_allowed(q, k, ids[nodes])
        same(got, R.exact_topk(dist, k, live=allowed_nodes, ids=ids), f"d={d} {dtype} allowed, k={k}")
        assert np.all(got.counts == min(k, 100))


@pytest.mark.parametrize("d,dtype", [(130, "f32"), (10, "f16")])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_graphs_around_the_tile_size_and_k_above_the_live_count(fv, ctx, n, d, dtype):
    x = mixture(n, d, n_comp=4, seed=n + d)
    if n > 2:
        x[n - 1] = x[0]  # a tie between the first and the last lane in use
    ids = np.arange(n, dtype=np.uint64) * 3 + 5
    q = np.concatenate([mixture(4, d, n_comp=4, seed=n), x[:1]])
    g = ring_graph(fv, ctx, ids, x, dtype)
    dist = R.fold_distances(q, stored(x, dtype))
    for k in (1, 10, 256):
        got = g.search_exact(q, k)
        same(got, R.exact_topk(dist, k, ids=ids), f"n={n} k={k}")
        m = min(n, k)
        assert np.all(got.counts == m)
        assert np.all(got.ids[:, m:] == NO_ID) and np.all(np.isposinf(got.distances[:, m:]))


# ---- liveness ---------------------------------------------------------------------------------------------------------
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
    for k in (10, 256):
        same(g.search_exact(q, k), R.exact_topk(dist, k, live=live, ids=ids), f"a third deleted, k={k}")
    assert g.vacuum() == int((~live).sum())
    # the survivors keep their order under new node indices: the answer is the one before the vacuum
    for k in (10, 256):
        same(g.search_exact(q, k), R.exact_topk(dist, k, live=live, ids=ids), f"after vacuum, k={k}")


def test_every_node_deleted_gives_counts_of_zero(fv, ctx):
    n, d = 130, 10
    x = mixture(n, d, n_comp=4, seed=8)
    ids = np.arange(n, dtype=np.uint64)
    g = ring_graph(fv, ctx, ids, x, "f32")
    for i in ids:
        g.mark_deleted(int(i))
    got = g.search_exact(mixture(5, d, n_comp=4, seed=9), 10)
    assert np.all(got.counts == 0) and np.all(got.ids == NO_ID) and np.all(np.isposinf(got.distances))
    # and an index that never held a row
    got = fv.HNSWIndex(ctx, 4, 8, 16).search_exact(mixture(5, d, n_comp=4, seed=9), 10)
    assert np.all(got.counts == 0) and np.all(got.ids == NO_ID)


@pytest.mark.parametrize("dtype", DTYPES)
def test_allow_set_equals_the_allowed_scan_bit_for_bit(fv, ctx, dtype):
    """two independent kernels — the gather scan behind search_allowed and the flat tile scan — one answer"""
    n, d = 700, 130
    x = R.with_duplicates(mixture(n, d, n_comp=6, seed=21), [(4, 6), (4, 300), (255, 257)])
    ids = np.arange(n, dtype=np.uint64) + 50
    g = ring_graph(fv, ctx, ids, x, dtype)
    for i in ids[5::7]:
        g.mark_deleted(int(i))
    live = np.ones(n, bool)
    live[5::7] = False
    allowed_nodes = np.zeros(n, bool)
    allowed_nodes[::2] = True
    allowed = np.concatenate([ids[allowed_nodes], np.array([7, 10 ** 9], np.uint64)])  # two ids the index does not hold
    q = np.concatenate([mixture(9, d, n_comp=6, seed=22), x[[4, 255]]])
    dist = R.fold_distances(q, stored(x, dtype))
    g.scan_cutoff = 2 ** 64 - 1
    for k in (1, 10, 256):
        got = g.search_exact_allowed(q, k, allowed)
        same(got, R.exact_topk(dist, k, live=live & allowed_nodes, ids=ids), f"allowed, k={k}")
        other = g.search_allowed(q, k, 50, allowed)
        same(got, (other.ids, other.distances, other.counts), f"flat scan vs allowed scan, k={k}")
    none = g.search_exact_allowed(q, 10, np.array([7], np.uint64))
    assert np.all(none.counts == 0) and np.all(none.ids == NO_ID)


# ---- the hybrid index -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_hybrid_exact_is_the_merge_of_the_two_exact_parts(fv, ctx, dtype):
    n, d, nlist, k = 1200, 24, 12, 10
    x = mixture(n, d, n_comp=8, seed=31)
    ids = np.arange(n, dtype=np.uint64) + 10
    now = 1000 * DAY
    age = np.where(np.arange(n) % 3 == 0, 5 * DAY, 30 * DAY)  # 400 recent rows, 800 historical ones
    age[:60] = 6.5 * DAY                                      # recent now, due for migration half a day later
    h = fv.HybridIndex(ctx, max_connections=6, max_connections_layer_0=12, ef_construction=40, n_clusters=nlist,
                       n_probe=3, row_dtype=dtype)
    h.set_ivf_centroids(x[:nlist])
    h.bulk_insert(ids, x, now - age, now)
    n_recent = h.recent_count()
    recent = np.flatnonzero(age < 7 * DAY)
    assert n_recent == recent.size
    xs = stored(x, dtype)
    q = np.concatenate([mixture(12, d, n_comp=8, seed=32), x[[0, 1, 2, 5]]])  # four queries on rows about to migrate

    def check(now_):
        both = h.search_exact(q, k, now=now_)
        r = h.search_exact(q, k, now=now_, search_historical=False)
        hi = h.search_exact(q, k, now=now_, search_recent=False)
        # the recent part: the numpy restatement on the graph's rows (node order = insertion order of the recent rows)
        same(r, R.exact_topk(R.fold_distances(q, xs[recent]), k, ids=ids[recent]), "recent-only")
        g_r = h.hnsw().search_exact(q, k)
        same(r, (g_r.ids, g_r.distances, g_r.counts), "recent-only vs the graph's own search_exact")
        # the list part: IVFIndex's every-list search
        ivf = h.ivf()
        every = ivf.search(q, k, n_probe=nlist)
        same(hi, (every.ids, every.distances, every.counts), "historical-only vs the every-list search")
        e2 = ivf.search_exact(q, k)
        same(hi, (e2.ids, e2.distances, e2.counts), "IVFIndex.search_exact")
        # mixed: the usual merge of the two
        for b in range(q.shape[0]):
            wi, wd = R.merge_parts([(r.ids[b, :r.counts[b]], r.distances[b, :r.counts[b]]),
                                    (hi.ids[b, :hi.counts[b]], hi.distances[b, :hi.counts[b]])], k)
            assert both.counts[b] == wi.size
            assert np.array_equal(both.ids[b, :wi.size], wi) and np.array_equal(bits(both.distances[b, :wi.size]), bits(wd))
        return both

    check(now)
    hist_before = h.historical_count()
    later = now + 1 * DAY  # rows 0..59 are now 7.5 days old: the search's own migration step copies them to the lists
    both = check(later)
    assert h.historical_count() > hist_before
    # a migrated row still sits in the graph: it is returned twice, as search() returns it
    dup = [b for b in range(q.shape[0]) if len(set(both.ids[b, :both.counts[b]].tolist())) < both.counts[b]]
    assert dup, "no query saw a migrated row twice"
    assert list(both.ids[12, :2]) == [10, 10]


# ---- search quality ---------------------------------------------------------------------------------------------------
def test_graph_quality_equals_the_host_recomputation(fv, ctx):
    # One Gaussian in 8 dimensions, 32 links on layer 0: the reference keeps a node's nearest M links, which cuts a
    # clustered data set into islands the walk cannot leave; here every node is reachable, so a walk with ef = n visits
    # the whole graph and its k best are the exact ones.
    n, d, k = 2000, 8, 10
    g, ids, x = built_graph(fv, ctx, n, d, seed=41, n_comp=1, M=16, efc=100)
    q = mixture(40, d, n_comp=1, seed=42)
    truth = g.search_exact(q, k)
    same(truth, R.exact_topk(R.fold_distances(q, x), k, ids=ids), "the truth itself")
    for ef in (2000, 10):
        res = g.search(q, k, ef)
        sq = g.evaluate_search_quality(q, k, ef)
        ar, ap = R.host_quality(res, truth, k)
        print(f"ef={ef}: avg_recall={sq['avg_recall']} avg_precision={sq['avg_precision']} host={ar},{ap}")
        assert sq["queries_evaluated"] == 40 and sq["avg_query_time_ms"] > 0
        assert bits(sq["avg_recall"]) == bits(ar), f"ef={ef}: recall {sq['avg_recall']} vs host {ar}"
        assert bits(sq["avg_precision"]) == bits(ap), f"ef={ef}: precision {sq['avg_precision']} vs host {ap}"
        if ef == 2000:
            assert sq["avg_precision"] == np.float32(1.0)


def test_hybrid_quality_equals_the_host_recomputation_with_duplicate_ids(fv, ctx):
    n, d, nlist, k = 900, 16, 9, 10
    x = mixture(n, d, n_comp=6, seed=51)
    ids = np.arange(n, dtype=np.uint64)
    now = 500 * DAY
    age = np.where(np.arange(n) % 2 == 0, 6.5 * DAY, 40 * DAY)
    h = fv.HybridIndex(ctx, max_connections=6, max_connections_layer_0=12, ef_construction=40, n_clusters=nlist, n_probe=2)
    h.set_ivf_centroids(x[:nlist])
    h.bulk_insert(ids, x, now - age, now)
    q = np.concatenate([mixture(20, d, n_comp=6, seed=52), x[[0, 2, 4]]])
    later = now + DAY  # a migration is due: the evaluation takes that step once, then both searches see the same rows
    sq = h.evaluate_search_quality(q, k, now=later, hnsw_ef=20, ivf_n_probe=2)
    assert h.historical_count() > n // 2
    res = h.search(q, k, now=later, hnsw_ef=20, ivf_n_probe=2)
    truth = h.search_exact(q, k, now=later)
    assert any(len(set(res.ids[b, :res.counts[b]].tolist())) < res.counts[b] for b in range(q.shape[0])), "no duplicate id"
    ar, ap = R.host_quality(res, truth, k)
    print(f"hybrid: avg_recall={sq['avg_recall']} avg_precision={sq['avg_precision']} host={ar},{ap}")
    assert sq["queries_evaluated"] == q.shape[0]
    assert bits(sq["avg_recall"]) == bits(ar) and bits(sq["avg_precision"]) == bits(ap)


def test_quality_kernel_on_caller_supplied_blocks(fv, ctx):
    B, k = 3, 3
    res = np.array([[1, 2, 9], [4, 5, 6], [7, 7, 8]], np.uint64)
    truth = np.array([[1, 2, 3], [0, 0, 0], [7, 1, 2]], np.uint64)
    rc_, tc_ = np.array([3, 3, 3], np.uint32), np.array([3, 0, 3], np.uint32)
    bufs = [ctx.upload(a) for a in (res, rc_, truth, tc_)]
    out = (ctx.alloc(B * 4), ctx.alloc(B * 4))
    ctx.check(ctx.lib.fvdb_search_quality_lists_dev(ctx.h, *bufs, B, k, *out))
    ctx.synchronize()
    f = np.float32
    assert np.array_equal(ctx.download(out[0], (B,), np.float32), np.array([f(2) / f(3), 1, f(2) / f(3)], np.float32))
    assert np.array_equal(ctx.download(out[1], (B,), np.float32), np.array([f(2) / f(3), 0, f(2) / f(3)], np.float32))
    for p in bufs + list(out):
        ctx.free(p)


# ---- errors -----------------------------------------------------------------------------------------------------------
def test_errors(fv, ctx):
    n, d = 200, 16
    x = mixture(n, d, n_comp=4, seed=61)
    ids = np.arange(n, dtype=np.uint64)
    g = ring_graph(fv, ctx, ids, x, "f32")
    q = mixture(4, d, n_comp=4, seed=62)
    for k in (0, 257):
        for call in (lambda: g.search_exact(q, k), lambda: g.search_exact_allowed(q, k, ids[:5]),
                     lambda: g.evaluate_search_quality(q, k, 50)):
            with pytest.raises(fv.Unsupported) as e:
                call()
            assert e.value.status == E_UNSUPPORTED
    with pytest.raises(fv.DimensionMismatch):
        g.search_exact(mixture(4, d + 4, n_comp=4, seed=62), 5)
    with pytest.raises(fv.InvalidConfig):
        g.evaluate_search_quality(np.zeros((0, d), np.float32), 5, 50)
    # a stale mask, and a mask of another graph, through the C ABI
    lib, gh = ctx.lib, g._graph()
    nodes = np.ascontiguousarray(np.arange(0, n, 2, dtype=np.uint32))
    mask = C.c_void_p()
    ctx.check(lib.fvdb_mask_create_graph(gh, nodes.ctypes.data_as(C.POINTER(C.c_uint32)), nodes.size, C.byref(mask)))
    B, k = 4, 5
    q_dev = ctx.upload(q)
    out = (ctx.alloc(B * k * 4), ctx.alloc(B * k * 4), ctx.alloc(B * 4))
    ctx.check(lib.fvdb_graph_search_flat_dev_slot(gh, None, 0, mask, q_dev, B, k, *out))
    ctx.synchronize()
    got = fv.index.SearchResults(ctx.download(out[0], (B, k), np.uint32).astype(np.uint64), ctx.download(out[1], (B, k), np.float32),
                                 ctx.download(out[2], (B,), np.uint32))
    allowed = np.zeros(n, bool)
    allowed[::2] = True
    same(got, R.exact_topk(R.fold_distances(q, x), k, live=allowed), "the C entry point under a mask")
    assert lib.fvdb_graph_search_flat_dev_slot(gh, None, 0, mask, q_dev, B, 0, *out) == E_UNSUPPORTED
    assert lib.fvdb_graph_search_flat_dev_slot(gh, None, 0, mask, q_dev, B, 257, *out) == E_UNSUPPORTED
    other = ring_graph(fv, ctx, ids[:70], x[:70], "f32")
    rc = lib.fvdb_graph_search_flat_dev_slot(other._graph(), None, 0, mask, q_dev, B, k, *out)
    assert rc == E_INVALID and b"another graph" in lib.fvdb_last_error(ctx.h)
    g.mark_deleted(int(ids[1]))
    rc = lib.fvdb_graph_search_flat_dev_slot(gh, None, 0, mask, q_dev, B, k, *out)
    assert rc == E_INVALID and b"stale mask" in lib.fvdb_last_error(ctx.h)
    lib.fvdb_mask_destroy(mask)
    for p in out + (q_dev,):
        ctx.free(p)
    # the hybrid forms: k, an empty query set, a sharded index
    h = fv.HybridIndex(ctx, max_connections=4, max_connections_layer_0=8, ef_construction=16, n_clusters=4, n_probe=2)
    h.set_ivf_centroids(x[:4])
    now = 100 * DAY
    h.bulk_insert(ids, x, now - np.where(ids % 2 == 0, DAY, 30 * DAY), now)
    for k in (0, 257):
        with pytest.raises(fv.Unsupported):
            h.search_exact(q, k, now=now)
    with pytest.raises(fv.DimensionMismatch):
        h.search_exact(mixture(4, d + 4, n_comp=4, seed=62), 5, now=now)
    with pytest.raises(fv.InvalidConfig):
        h.evaluate_search_quality(np.zeros((0, d), np.float32), 5, now=now)
    s = fv.HybridIndex(ctx, max_connections=4, max_connections_layer_0=8, ef_construction=16, n_clusters=4, n_probe=2)
    s.set_ivf_centroids(x[:4])
    s.bulk_insert_sharded(ids, x, now - np.where(ids % 2 == 0, DAY, 30 * DAY), now, 0, 2)
    for call in (lambda: s.search_exact(q, 5, now=now), lambda: s.evaluate_search_quality(q, 5, now=now)):
        with pytest.raises(fv.Unsupported, match="sharded") as e:
            call()
        assert e.value.status == E_UNSUPPORTED
    # the host mirror refuses by itself too
    ids_o, ds_o, cnt_o = np.empty((4, 5), np.uint64), np.empty((4, 5), np.float32), np.zeros(4, np.uint32)
    rc = s.lib.fvh_hybrid_search_exact(s.h, q.ctypes.data_as(C.POINTER(C.c_float)), 4, d, 5, 1, 1, float(now),
                                       ids_o.ctypes.data_as(C.POINTER(C.c_uint64)), ds_o.ctypes.data_as(C.POINTER(C.c_float)),
                                       cnt_o.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == E_UNSUPPORTED
