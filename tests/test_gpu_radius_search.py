"""GPU: radius search over the graph — HNSWIndex.search_radius / count_within and the C entry
points under them.

Ids, distance bits, counts and totals must equal _radius_ref.radius_answer, the numpy restatement built on the
reference's own f32 distance (_exact_ref.py); the hand-built cases are _exact_wide_cases.py's, whose properties at the
radii used here test_radius_ref.py proves on the CPU.  Shapes are the exact-wide tests': 4500 rows (71 tiles, the last
part-filled), 33 queries.  The radii put every query on each of the selection's three steps: an empty ball, a ball that
fits the cap (counted, gathered, sorted, no radix pass), a ball above the cap (the fall-through to the radix select), and
batches that mix them.  count_within is checked against the totals in every case."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture
import _exact_ref as R
import _exact_wide_cases as W
import _radius_ref as RR

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = 6, 12
NO_ID = R.NO_ID
INF = np.float32(np.inf)


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
    g.restore(ids, x, np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64), np.roll(ids, -1), int(ids[0]))
    return g


def same(got, want, what=""):
    """(SearchResults, totals) against radius_answer's (ids, distances, counts, totals), bit for bit"""
    res, totals = got
    wi, wd, wc, wt = want
    assert totals.dtype == np.uint32 and np.array_equal(totals, wt), f"{what}: totals differ: {totals[:8]} vs {wt[:8]}"
    assert np.array_equal(res.counts, wc), f"{what}: counts differ: {res.counts[:8]} vs {wc[:8]}"
    assert np.array_equal(res.ids, wi), f"{what}: ids differ (first bad query {np.flatnonzero((res.ids != wi).any(1))[:3]})"
    assert np.array_equal(bits(res.distances), bits(wd)), f"{what}: distances are not bit-identical"


def check(g, q, dist, radius, m, ids, what, live=None, allowed=None):
    """search_radius and count_within against the reference; returns the (results, totals) pair"""
    got = g.search_radius(q, radius, m, allowed=allowed)
    want = RR.radius_answer(dist, radius, m, live=live, ids=ids)
    same(got, want, what)
    counted = g.count_within(q, radius, allowed=allowed)
    assert counted.dtype == np.uint32 and np.array_equal(counted, want[3]), f"{what}: count_within differs from the totals"
    return got


# ---- 1. the boundary is inclusive and exact; 2. the three steps of the selection --------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("d", [10, 384])
def test_balls_in_the_4500_row_graph(fv, ctx, d, dtype):
    x, ids, q, dist = W.cut_case(d, dtype)
    g = ring_graph(fv, ctx, ids, x, dtype)
    what = f"d={d} {dtype}"
    r37 = RR.kth_distance(dist, 37)
    # the 37th-nearest distance holds 37 rows, the f32 value just below it 36 (test_radius_ref.py: no duplicate sits there)
    for m in (64, 37, 36, 4096):
        res, totals = check(g, q, dist, r37, m, ids, f"{what} r37 m={m}")
        assert np.all(totals == 37) and np.all(res.counts == min(m, 37))
    res, totals = check(g, q, dist, RR.below(r37), 64, ids, f"{what} below r37")
    assert np.all(totals == 36)
    # a radius below every distance: total 0, count 0, all-tail outputs
    free = slice(0, 29)
    res, totals = check(g, q[free], dist[free], RR.below(dist[free].min()), 64, ids, f"{what} below every distance")
    assert np.all(totals == 0) and np.all(res.counts == 0) and np.all(res.ids == NO_ID) and np.all(np.isposinf(res.distances))
    # one batch with mixed radii: empty, small, above the cap, and +inf
    mixed = r37.copy()
    mixed[0::4] = RR.below(dist[free].min())
    mixed[1::4] = RR.kth_distance(dist, 300)[1::4]
    mixed[2::4] = INF
    for m in (64, 4096):
        res, totals = check(g, q, dist, mixed, m, ids, f"{what} mixed radii m={m}")
        assert np.all(totals[0:29:4] == 0) and np.all(totals[1::4] >= 300) and np.all(totals[2::4] == W.N) and np.all(totals[3::4] == 37)
    # +inf: every live row is in the ball; the results are the wide exact search's — the fall-through to the radix select
    res, totals = check(g, q, dist, INF, 4096, ids, f"{what} +inf m=4096")
    assert np.all(totals == W.N) and np.all(res.counts == 4096)
    wide = g.search_exact_wide(q, 4096)
    assert np.array_equal(res.ids, wide.ids) and np.array_equal(bits(res.distances), bits(wide.distances))
    res, totals = check(g, q[27:32], dist[27:32], INF, 1, ids, f"{what} +inf m=1")
    assert np.all(totals == W.N) and np.all(res.counts == 1)
    if dtype == "f32":  # radius 0: the four queries that sit ON duplicated rows
        res, totals = check(g, q, dist, 0.0, 8, ids, f"{what} radius 0")
        assert list(totals[29:33]) == [3, 2, 2, 2] and np.all(totals[:29] == 0)
        assert list(res.ids[29, :3]) == [1010, 1011, 1012] and list(res.ids[31, :2]) == [1700, 3100]


# ---- 3. ties at the radius and at the cap -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_tie_group_on_the_boundary(fv, ctx, dtype):
    x, ids, v, q_on, q_50 = W.tie_case(dtype)
    dist = W.tie_dist(dtype)
    g = ring_graph(fv, ctx, ids, x, dtype)
    group = ids[W.GROUP]
    g_50 = dist[1, 100]
    # q_50 at the group's distance: the 50 nearer rows, then nodes 100.. in node order; the cap cuts INSIDE the group
    res, totals = check(g, q_50[None], dist[1:2], g_50, 300, ids, "q_50 m=300")
    assert totals[0] == 650 and res.counts[0] == 300
    assert list(res.ids[0, 50:300]) == list(group[:250]) and not set(res.ids[0, :50].tolist()) & set(group.tolist())
    res, totals = check(g, q_50[None], dist[1:2], g_50, 650, ids, "q_50 m=650")
    assert totals[0] == 650 and res.counts[0] == 650 and list(res.ids[0, 50:650]) == list(group)
    res, totals = check(g, q_50[None], dist[1:2], g_50, 4096, ids, "q_50 m=4096")
    assert totals[0] == 650 and res.counts[0] == 650
    res, totals = check(g, q_50[None], dist[1:2], RR.below(g_50), 300, ids, "q_50 just below the group")
    assert totals[0] == 50 and res.counts[0] == 50
    # q_on at radius 0: 600 words of bits 0, the lowest node indices win
    res, totals = check(g, q_on[None], dist[0:1], 0.0, 64, ids, "q_on m=64")
    assert totals[0] == 600 and list(res.ids[0]) == list(group[:64]) and np.all(bits(res.distances[0]) == 0)
    # both in one batch, a radius each
    check(g, np.stack([q_on, q_50]), dist, np.array([0.0, g_50], np.float32), 300, ids, "q_on + q_50")


def test_a_graph_of_identical_rows(fv, ctx):
    x, ids, q, dist = W.same_rows_case()
    g = ring_graph(fv, ctx, ids, x, "f32")
    common = dist[:, 0].copy()
    for m in (1, 64, 299, 300, 301):
        res, totals = check(g, q, dist, common, m, ids, f"same rows m={m}")
        k = min(m, 300)
        assert np.all(totals == 300) and np.all(res.counts == k) and np.all(res.ids[:, :k] == ids[:k])
    res, totals = check(g, q, dist, RR.below(common), 64, ids, "same rows, just below")
    assert np.all(totals == 0) and np.all(res.counts == 0)


# ---- 4. liveness ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_deleted_nodes_and_an_allow_set_are_in_neither_results_nor_totals(fv, ctx, dtype):
    n, d = 700, 130
    x = R.with_duplicates(mixture(n, d, n_comp=6, seed=21), [(4, 6), (4, 300), (255, 257)])
    ids = np.arange(n, dtype=np.uint64) + 50
    g = ring_graph(fv, ctx, ids, x, dtype)
    live = np.ones(n, bool)
    live[5::7] = False
    for i in ids[~live]:
        g.mark_deleted(int(i))
    q = np.concatenate([mixture(9, d, n_comp=6, seed=22), x[[4, 255]]])
    dist = R.fold_distances(q, W.stored(x, dtype))
    r = RR.kth_distance(dist, 120)  # over all rows: some of the 120 are deleted
    for m in (10, 300):
        res, totals = check(g, q, dist, r, m, ids, f"{dtype} deleted m={m}", live=live)
        assert np.all(totals < 120) and np.all(totals > 0)
        check(g, q, dist, INF, m, ids, f"{dtype} deleted +inf m={m}", live=live)
    for name, nodes in (("one row", np.array([4])), ("70 rows", np.arange(0, n, 10)), ("every row", np.arange(n))):
        allowed_nodes = np.zeros(n, bool)
        allowed_nodes[nodes] = True
        allowed = np.concatenate([ids[allowed_nodes], np.array([7, 10 ** 9], np.uint64)])  # two ids the index does not hold
        for radius in (r, INF):
            check(g, q, dist, radius, 300, ids, f"{dtype} allowed: {name}", live=live & allowed_nodes, allowed=allowed)
    res, totals = g.search_radius(q, INF, 300, allowed=np.array([7], np.uint64))
    assert np.all(totals == 0) and np.all(res.counts == 0) and np.all(res.ids == NO_ID)
    assert np.all(g.count_within(q, INF, allowed=np.array([7], np.uint64)) == 0)


def test_an_index_that_never_held_a_row(fv, ctx):
    g = fv.HNSWIndex(ctx, 4, 8, 16)
    q = mixture(5, 10, n_comp=4, seed=9)
    res, totals = g.search_radius(q, INF, 300)
    assert np.all(totals == 0) and np.all(res.counts == 0) and np.all(res.ids == NO_ID)
    assert np.all(g.count_within(q, INF) == 0)


# ---- 5. the C entry points: device pointers, a mask, the refusals -----------------------------------------------------
def c_call(fv, ctx, gh, mask, q, radius, m):
    """fvdb_graph_search_flat_radius_dev_slot and fvdb_graph_count_within_dev_slot through ctypes:
    (status, (SearchResults with node indices as ids, totals), status of the count, its totals)"""
    B = q.shape[0]
    q_dev, r_dev = ctx.upload(q), ctx.upload(np.ascontiguousarray(radius, np.float32))
    out = (ctx.alloc(B * max(m, 1) * 4), ctx.alloc(B * max(m, 1) * 4), ctx.alloc(B * 4), ctx.alloc(B * 4), ctx.alloc(B * 4))
    rc = ctx.lib.fvdb_graph_search_flat_radius_dev_slot(gh, None, 0, mask, q_dev, B, r_dev, m, *out[:4])
    rc2 = ctx.lib.fvdb_graph_count_within_dev_slot(gh, None, 0, mask, q_dev, B, r_dev, out[4])
    got = counted = None
    ctx.synchronize()
    if rc == 0:
        got = (fv.index.SearchResults(ctx.download(out[0], (B, m), np.uint32).astype(np.uint64),
                                      ctx.download(out[1], (B, m), np.float32), ctx.download(out[2], (B,), np.uint32)),
               ctx.download(out[3], (B,), np.uint32))
    if rc2 == 0:
        counted = ctx.download(out[4], (B,), np.uint32)
    for p in out + (q_dev, r_dev):
        ctx.free(p)
    return rc, got, rc2, counted


def as_nodes(want):
    wi, wd, wc, wt = want
    wi = wi.copy()
    wi[wi == NO_ID] = np.uint64(0xFFFFFFFF)  # FVDB_NO_ROW is 32 bits wide
    return wi, wd, wc, wt


def test_c_entry_points_under_a_mask_and_their_refusals(fv, ctx):
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
    radius = RR.kth_distance(dist, 40)
    for m in (5, 300):
        rc, got, rc2, counted = c_call(fv, ctx, gh, mask, q, radius, m)
        assert rc == 0 and rc2 == 0
        want = as_nodes(RR.radius_answer(dist, radius, m, live=allowed))
        same(got, want, f"the C entry point under a mask, m={m}")
        assert np.array_equal(counted, want[3])
    rc, got, rc2, counted = c_call(fv, ctx, gh, None, q, radius, 300)
    assert rc == 0 and rc2 == 0
    same(got, as_nodes(RR.radius_answer(dist, radius, 300)), "the C entry point without a mask")
    assert np.all(counted == 40)
    # the device forms do not inspect the radii: a negative or NaN one has an empty ball, -0.0 is 0.0
    odd = np.array([-1.0, np.nan, -0.0, -np.inf], np.float32)
    rc, got, rc2, counted = c_call(fv, ctx, gh, None, np.concatenate([q[:3], x[:1]]), odd, 8)
    assert rc == 0 and rc2 == 0
    assert list(got[1]) == [0, 0, 0, 0] and list(counted) == [0, 0, 0, 0] and np.all(got[0].counts == 0)
    rc, got, rc2, counted = c_call(fv, ctx, gh, None, x[:1], np.array([-0.0], np.float32), 8)
    assert list(got[1]) == [1] and list(counted) == [1] and got[0].ids[0, 0] == 0
    for m in (0, 4097):
        rc, _, _, _ = c_call(fv, ctx, gh, mask, q, radius, m)
        assert rc == E_UNSUPPORTED and b"FVDB_MAX_K_WIDE" in lib.fvdb_last_error(ctx.h)
    other = ring_graph(fv, ctx, ids[:70], x[:70], "f32")
    rc, _, rc2, _ = c_call(fv, ctx, other._graph(), mask, q, radius, 5)
    assert rc == E_INVALID and rc2 == E_INVALID and b"another graph" in lib.fvdb_last_error(ctx.h)
    g.mark_deleted(int(ids[1]))
    rc, _, rc2, _ = c_call(fv, ctx, gh, mask, q, radius, 5)
    assert rc == E_INVALID and rc2 == E_INVALID and b"stale mask" in lib.fvdb_last_error(ctx.h)
    lib.fvdb_mask_destroy(mask)


def test_refusals_of_the_host_forms(fv, ctx):
    n, d = 200, 16
    x = mixture(n, d, n_comp=4, seed=61)
    ids = np.arange(n, dtype=np.uint64)
    g = ring_graph(fv, ctx, ids, x, "f32")
    q = mixture(4, d, n_comp=4, seed=62)
    for m in (0, 4097):
        for call in (lambda: g.search_radius(q, 1.0, m), lambda: g.search_radius(q, 1.0, m, allowed=ids[:5])):
            with pytest.raises(fv.Unsupported) as e:
                call()
            assert e.value.status == E_UNSUPPORTED
    for bad in (-1.0, np.nan, [1.0, 1.0, -1e-30, 1.0], -np.inf):
        for call in (lambda: g.search_radius(q, bad, 10), lambda: g.search_radius(q, bad, 10, allowed=ids[:5]),
                     lambda: g.count_within(q, bad), lambda: g.count_within(q, bad, allowed=ids[:5])):
            with pytest.raises(fv.InvalidConfig) as e:
                call()
            assert e.value.status == E_INVALID
    with pytest.raises(fv.InvalidConfig):
        g.search_radius(q, [1.0, 2.0], 10)  # two radii for four queries
    with pytest.raises(fv.DimensionMismatch):
        g.search_radius(mixture(4, d + 4, n_comp=4, seed=62), 1.0, 10)
    with pytest.raises(fv.DimensionMismatch):
        g.count_within(mixture(4, d + 4, n_comp=4, seed=62), 1.0)
