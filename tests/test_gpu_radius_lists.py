"""GPU: radius search over the probed lists and over the hybrid index — IVFIndex.search_radius,
HybridIndex.search_radius and the engine entry points under them.

The list scan's ball is defined on the rows the k-search at the same n_probe would score, in its order: the oracle's
batch_search at a k above the row count IS that order (probe rank, position, a stable sort by distance), so the CPU
answer is its prefix within the radius and the total is that prefix's length.  The index is _any_nprobe_data.main_case
(3000 rows, 300 lists), probed on either side of the 256 lists whose rank bases the selection stages in LDS."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture
import _any_nprobe_data as D
import _exact_ref as R
import _exact_wide_cases as W
import _radius_ref as RR

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED, E_NONFINITE = 6, 12, 9
DAY = 86400.0
NO_ID = R.NO_ID
INF = np.float32(np.inf)
NLIST = D.NLIST


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(fv, ctx):
    """the index, its oracle, 33 queries (four ON stored rows) and, per n_probe, the oracle's full scan-order answer"""
    d = 20
    x, ids, cents = D.main_case(d, seed=4500)
    g = fv.IVFIndex(ctx, n_clusters=NLIST, n_probe=4)
    g.set_trained(cents)
    g.batch_insert(ids, x)
    o, cl = D.oracle_index(x, ids, cents)
    q = np.concatenate([mixture(29, d, n_comp=40, seed=4501), x[[5, 900, 1500, 2999]]])
    full = {p: o.batch_search(q, x.shape[0], p, threads=8) for p in (3, 256, 257, NLIST)}
    return dict(g=g, o=o, x=x, ids=ids, cents=cents, q=q, full=full)


def cut(full, radius, m):
    """(ids [B, m], distances [B, m], counts, totals): the prefix of a full scan-order answer within the radius, capped"""
    fi, fd, fc = full
    B = fi.shape[0]
    r = np.broadcast_to(np.asarray(radius, np.float32).reshape(-1), (B,))
    out_i = np.full((B, m), NO_ID, np.uint64)
    out_d = np.full((B, m), np.inf, np.float32)
    cnt, tot = np.zeros(B, np.uint32), np.zeros(B, np.uint32)
    for b in range(B):
        n = int(fc[b])
        t = int((bits(fd[b, :n]) <= RR.word(r[b])).sum())  # ascending distances: a prefix
        assert np.all(bits(fd[b, :t]) <= RR.word(r[b]))
        c = min(t, m)
        out_i[b, :c], out_d[b, :c], cnt[b], tot[b] = fi[b, :c], fd[b, :c], c, t
    return out_i, out_d, cnt, tot


def same(got, want, what=""):
    res, totals = got
    wi, wd, wc, wt = want
    assert totals.dtype == np.uint32 and np.array_equal(totals, wt), f"{what}: totals differ: {totals[:8]} vs {wt[:8]}"
    assert np.array_equal(res.counts, wc), f"{what}: counts differ: {res.counts[:8]} vs {wc[:8]}"
    assert np.array_equal(res.ids, wi), f"{what}: ids differ (first bad query {np.flatnonzero((res.ids != wi).any(1))[:3]})"
    assert np.array_equal(bits(res.distances), bits(wd)), f"{what}: distances are not bit-identical"


def radii_of(full, B):
    """the 10th and the 300th distance of every query (the last one where fewer rows are scanned), a batch that mixes
    zero / small / large / +inf, and +inf"""
    fd, fc = full[1], full[2].astype(np.int64)
    assert np.all(fc >= 1)
    rows = np.arange(B)
    r10, r300 = fd[rows, np.minimum(9, fc - 1)].copy(), fd[rows, np.minimum(299, fc - 1)].copy()
    mixed = r10.copy()
    mixed[0::4] = 0
    mixed[1::4] = r300[1::4]
    mixed[2::4] = INF
    return {"r10": r10, "r300": r300, "mixed": mixed, "inf": INF, "zero": np.float32(0)}


# ---- 1. the probed lists, on either side of 256 probes ----------------------------------------------------------------
@pytest.mark.parametrize("n_probe", [3, 256, 257, NLIST])
def test_search_radius_is_the_k_search_cut_at_the_radius(world, n_probe):
    g, q, full = world["g"], world["q"], world["full"][n_probe]
    for name, radius in radii_of(full, q.shape[0]).items():
        for m in (1, 64, 4096):
            what = f"n_probe={n_probe} {name} m={m}"
            got = g.search_radius(q, radius, m, n_probe=n_probe)
            want = cut(full, radius, m)
            same(got, want, what)
            # and the wide search at k = m, cut at the radius: the same rows in the same order
            wide = g.search(q, m, n_probe=n_probe)
            for b in range(q.shape[0]):
                c = int(got[0].counts[b])
                assert c == min(m, int(got[1][b]))
                assert np.array_equal(got[0].ids[b, :c], wide.ids[b, :c]), what
                assert np.array_equal(bits(got[0].distances[b, :c]), bits(wide.distances[b, :c])), what
                if c < int(wide.counts[b]):  # the first row the radius leaves out is beyond it
                    rb = radius if np.ndim(radius) == 0 else radius[b]
                    assert bits(wide.distances[b, c:c + 1])[0] > RR.word(rb), what
    # the four queries ON stored rows: radius 0 finds them
    res, totals = g.search_radius(q, 0.0, 8, n_probe=n_probe)
    assert np.all(totals[29:] >= 1) and list(res.ids[29:, 0]) == list(world["ids"][[5, 900, 1500, 2999]])


def test_totals_count_the_probed_lists_only(world):
    g, q, full = world["g"], world["q"], world["full"]
    t3 = g.search_radius(q, INF, 16, n_probe=3)[1]
    t_all = g.search_radius(q, INF, 16, n_probe=NLIST)[1]
    assert np.array_equal(t3, full[3][2]) and np.all(t_all == world["x"].shape[0]) and np.all(t3 < t_all)
    r = full[NLIST][1][:, 299].copy()  # the 300th distance over every list
    few = g.search_radius(q, r, 16, n_probe=3)[1]
    assert np.all(g.search_radius(q, r, 16, n_probe=NLIST)[1] >= 300) and np.all(few < 300)
    assert np.array_equal(few, cut(full[3], r, 16)[3])


def test_rows_outside_an_allow_set_are_in_neither_results_nor_totals(world):
    g, q, x, ids, cents = world["g"], world["q"], world["x"], world["ids"], world["cents"]
    rng = np.random.default_rng(45)
    allowed = ids[rng.random(ids.size) < 0.3]
    o, _ = D.oracle_index(x, ids, cents)
    keep = set(int(i) for i in allowed)
    for i in ids:
        if int(i) not in keep:
            o.mark_deleted(int(i))
    for n_probe in (3, 257):
        full = o.batch_search(q, x.shape[0], n_probe, threads=8)
        r = world["full"][257][1][:, 99].copy()  # the 100th distance of the UNFILTERED 257-probe search: ~30 allowed rows inside
        for radius, name in ((r, "r100"), (INF, "inf")):
            for m in (16, 4096):
                got = g.search_radius(q, radius, m, n_probe=n_probe, allowed=allowed)
                same(got, cut(full, radius, m), f"allowed n_probe={n_probe} {name} m={m}")
                assert np.isin(got[0].ids[got[0].ids != NO_ID], allowed).all()
        assert np.all(g.search_radius(q, r, 16, n_probe=n_probe, allowed=allowed)[1] < 100)
    res, totals = g.search_radius(q, INF, 16, n_probe=NLIST, allowed=np.array([1], np.uint64))  # an id the index does not hold
    assert np.all(totals == 0) and np.all(res.counts == 0) and np.all(res.ids == NO_ID)


# ---- 2. the engine's device-pointer form and the refusals -------------------------------------------------------------
def test_engine_entry_points_and_refusals(fv, ctx, world):
    g, q, full = world["g"], world["q"], world["full"][257]
    lib, h = ctx.lib, g._dev()
    B, m = q.shape[0], 64
    radius = np.ascontiguousarray(full[1][:, 9])
    # the host mirror's refusals
    for bad_m in (0, 4097):
        with pytest.raises(fv.Unsupported) as e:
            g.search_radius(q, radius, bad_m, n_probe=257)
        assert e.value.status == E_UNSUPPORTED
        with pytest.raises(fv.Unsupported):
            g.search_radius(q, radius, bad_m, n_probe=257, allowed=world["ids"][:9])
    for bad in (-1.0, np.nan, -np.inf):
        for allowed in (None, world["ids"][:9]):
            with pytest.raises(fv.InvalidConfig) as e:
                g.search_radius(q, bad, m, n_probe=257, allowed=allowed)
            assert e.value.status == E_INVALID
    qbad = q.copy()
    qbad[3, 1] = np.nan
    with pytest.raises(fv.engine.NonFiniteInput):
        g.search_radius(qbad, radius, m, n_probe=257)
    with pytest.raises(fv.DimensionMismatch):
        g.search_radius(mixture(4, q.shape[1] + 4, n_comp=4, seed=1), 1.0, m)
    with pytest.raises(fv.engine.NotTrained):
        fv.IVFIndex(ctx, n_clusters=4, n_probe=2).search_radius(q, 1.0, m)
    # the device-pointer form: the same answer; it does not inspect the radii (negative / NaN: an empty ball)
    q_dev, r_dev = ctx.upload(q), ctx.upload(radius)
    out = (ctx.alloc(B * m * 8), ctx.alloc(B * m * 4), ctx.alloc(B * 4), ctx.alloc(B * 4))
    ctx.check(lib.fvdb_ivf_search_radius_dev_slot(h, None, 0, None, q_dev, B, r_dev, m, 257, *out))
    ctx.synchronize()
    got = (fv.index.SearchResults(ctx.download(out[0], (B, m), np.uint64), ctx.download(out[1], (B, m), np.float32),
                                  ctx.download(out[2], (B,), np.uint32)), ctx.download(out[3], (B,), np.uint32))
    same(got, cut(full, radius, m), "fvdb_ivf_search_radius_dev_slot")
    odd = ctx.upload(np.where(np.arange(B) % 2 == 0, np.float32(-1), np.float32(np.nan)).astype(np.float32))
    ctx.check(lib.fvdb_ivf_search_radius_dev_slot(h, None, 0, None, q_dev, B, odd, m, 257, *out))
    ctx.synchronize()
    assert np.all(ctx.download(out[3], (B,), np.uint32) == 0) and np.all(ctx.download(out[2], (B,), np.uint32) == 0)
    for bad_m in (0, 4097):
        assert lib.fvdb_ivf_search_radius_dev_slot(h, None, 0, None, q_dev, B, r_dev, bad_m, 257, *out) == E_UNSUPPORTED
        assert b"FVDB_MAX_K_WIDE" in lib.fvdb_last_error(ctx.h)
    assert lib.fvdb_ivf_search_radius_dev_slot(h, None, 0, None, q_dev, B, None, m, 257, *out) == E_INVALID
    for p in out + (q_dev, r_dev, odd):
        ctx.free(p)


# ---- 3. the hybrid index ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_hybrid_radius_is_the_merge_of_the_two_parts_and_the_sum_of_their_totals(fv, ctx, dtype):
    n, d, nlist = 800, 24, 8
    x = mixture(n, d, n_comp=8, seed=31)
    ids = np.arange(n, dtype=np.uint64) + 10
    now = 1000 * DAY
    age = np.where(np.arange(n) % 2 == 0, 5 * DAY, 30 * DAY)
    age[:60:2] = 6.5 * DAY  # recent now, due for migration half a day later
    h = fv.HybridIndex(ctx, max_connections=6, max_connections_layer_0=12, ef_construction=40, n_clusters=nlist,
                       n_probe=3, row_dtype=dtype)
    h.set_ivf_centroids(x[:nlist])
    h.bulk_insert(ids, x, now - age, now)
    recent = np.flatnonzero(age < 7 * DAY)
    hist = np.flatnonzero(age >= 7 * DAY)
    assert h.recent_count() == recent.size == 400
    xs = W.stored(x, dtype)
    q = np.concatenate([mixture(8, d, n_comp=8, seed=32), x[[0, 2, 4]]])  # three queries on rows about to migrate
    B = q.shape[0]
    d_all = R.fold_distances(q, xs)
    # no two rows of a query are equally far: the historical part's order does not depend on the lists' layout
    assert all(np.unique(bits(d_all[b])).size == n for b in range(B))
    r_small, r_large = RR.kth_distance(d_all, 20), RR.kth_distance(d_all, 500)

    def check(now_, hist_rows, what):
        for radius, m in ((r_small, 64), (r_large, 64), (r_large, 4096), (INF, 300), (np.float32(0), 8)):
            got, totals = h.search_radius(q, radius, m, now=now_, ivf_n_probe=nlist)
            rp = RR.radius_answer(d_all[:, recent], radius, m, ids=ids[recent])
            hp = RR.radius_answer(d_all[:, hist_rows], radius, m, ids=ids[hist_rows])
            assert np.array_equal(totals, rp[3] + hp[3]), f"{what} m={m}: totals {totals} vs {rp[3]} + {hp[3]}"
            for b in range(B):
                wi, wd = R.merge_parts([(rp[0][b, :rp[2][b]], rp[1][b, :rp[2][b]]), (hp[0][b, :hp[2][b]], hp[1][b, :hp[2][b]])], m)
                assert got.counts[b] == wi.size, f"{what} m={m} query {b}"
                assert np.array_equal(got.ids[b, :wi.size], wi) and np.array_equal(bits(got.distances[b, :wi.size]), bits(wd))
                assert np.all(got.ids[b, wi.size:] == NO_ID)
            # the parts alone
            same(h.search_radius(q, radius, m, now=now_, ivf_n_probe=nlist, search_historical=False), rp, f"{what} recent-only")
            same(h.search_radius(q, radius, m, now=now_, ivf_n_probe=nlist, search_recent=False), hp, f"{what} historical-only")
        return h.search_radius(q, r_small, 64, now=now_, ivf_n_probe=nlist)

    check(now, hist, "before the migration")
    later = now + 1 * DAY  # rows 0, 2, .., 58 are 7.5 days old: the search's own migration step copies them to the lists
    hist_before = h.historical_count()
    res, totals = check(later, np.sort(np.concatenate([hist, np.arange(0, 60, 2)])), "after the migration")
    assert h.historical_count() > hist_before
    # a migrated row still sits in the graph: returned twice and counted twice, as search() returns it twice
    assert list(res.ids[8, :2]) == [10, 10] and totals[8] >= 2
    # under an allow-set both parts are filtered
    allowed = ids[::3]
    got, totals = h.search_radius(q, r_large, 4096, now=later, ivf_n_probe=nlist, allowed=allowed)
    assert np.isin(got.ids[got.ids != NO_ID], allowed).all() and np.all(totals == got.counts) and np.all(totals > 0)
    assert np.all(totals < h.search_radius(q, r_large, 4096, now=later, ivf_n_probe=nlist)[1])


def test_hybrid_refusals(fv, ctx):
    n, d = 200, 16
    x = mixture(n, d, n_comp=4, seed=61)
    ids = np.arange(n, dtype=np.uint64)
    q = mixture(4, d, n_comp=4, seed=62)
    now = 100 * DAY
    kw = dict(max_connections=4, max_connections_layer_0=8, ef_construction=16, n_clusters=4, n_probe=2)
    h = fv.HybridIndex(ctx, **kw)
    h.set_ivf_centroids(x[:4])
    h.bulk_insert(ids, x, now - np.where(ids % 2 == 0, DAY, 30 * DAY), now)
    for m in (0, 4097):
        with pytest.raises(fv.Unsupported):
            h.search_radius(q, 1.0, m, now=now)
    for bad in (-1.0, np.nan):
        with pytest.raises(fv.InvalidConfig):
            h.search_radius(q, bad, 10, now=now)
    with pytest.raises(fv.DimensionMismatch):
        h.search_radius(mixture(4, d + 4, n_comp=4, seed=62), 1.0, 10, now=now)
    s = fv.HybridIndex(ctx, **kw)
    s.set_ivf_centroids(x[:4])
    s.bulk_insert_sharded(ids, x, now - np.where(ids % 2 == 0, DAY, 30 * DAY), now, 0, 2)
    with pytest.raises(fv.Unsupported, match="sharded") as e:
        s.search_radius(q, 1.0, 10, now=now)
    assert e.value.status == E_UNSUPPORTED
    # the host mirror refuses by itself too
    f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    r = np.ones(4, np.float32)
    io, do, co, to = np.empty((4, 10), np.uint64), np.empty((4, 10), np.float32), np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    rc = s.lib.fvh_hybrid_search_radius(s.h, q.ctypes.data_as(f32p), 4, d, r.ctypes.data_as(f32p), 10, 2, 1, 1, None, 0, float(now),
                                        io.ctypes.data_as(u64p), do.ctypes.data_as(f32p), co.ctypes.data_as(u32p),
                                        to.ctypes.data_as(u32p))
    assert rc == E_UNSUPPORTED
