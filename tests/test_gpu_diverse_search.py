"""GPU: search_diverse of the three index classes.

The result must equal _mmr_ref.mmr_answer applied to that index's OWN search(fetch_k) result (search_allowed under an
allow-set) and its own get_vectors rows: ids, distance bits, ranks and counts.  The candidates' order, the lookup of each
candidate's row by id (the lowest list location; the recent part before the historical one) and the gather with its
zero-padded stride are what these tests add to test_gpu_mmr_select.py, which checks the kernel alone."""
import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture
import _mmr_ref as M

pytestmark = pytest.mark.gpu

DAY = 86400.0
SETTINGS = [(0.0, False), (0.25, True), (0.5, False), (0.5, True), (1.0, False), (1.0, True)]  # (lam, distinct)


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def rows_of(index, cand, d):
    """the candidates' rows [B, fetch_k, d] as the index itself returns them by id, and their pairwise folds; fetched once"""
    B, fetch_k = cand.ids.shape
    rows = np.zeros((B, fetch_k, d), np.float32)
    pairs = np.zeros((B, fetch_k, fetch_k), np.float32)
    for b in range(B):
        n = int(cand.counts[b])
        if n and hasattr(index, "get_vectors"):
            got, found = index.get_vectors(cand.ids[b, :n])
            assert found.all()
            rows[b, :n] = got
        elif n:  # the graph class returns one row at a time
            rows[b, :n] = [index.get_vector_by_id(int(i)) for i in cand.ids[b, :n]]
        pairs[b, :n, :n] = M.R.fold_distances(rows[b, :n], rows[b, :n])
    return rows, pairs


def reference(index, cand, k, lam, distinct, d, fetched=None):
    """mmr_answer on the candidates `cand` (a SearchResults of fetch_k) with the rows the index itself returns by id"""
    rows, pairs = fetched or rows_of(index, cand, d)
    return M.mmr_answer(cand.ids, cand.distances, rows, cand.counts, k, lam, distinct, pairs=pairs)


def same(got, want, what):
    res, ranks = got
    wi, wd, wr, wc = want
    assert ranks.dtype == np.uint32 and res.ids.dtype == np.uint64
    assert np.array_equal(res.counts, wc), f"{what}: counts differ: {res.counts[:8]} vs {wc[:8]}"
    bad = np.flatnonzero((ranks != wr).any(1))
    assert bad.size == 0, f"{what}: ranks differ in queries {bad[:4]}: {ranks[bad[0]][:12]} vs {wr[bad[0]][:12]}"
    assert np.array_equal(res.ids, wi), f"{what}: ids differ"
    assert np.array_equal(bits(res.distances), bits(wd)), f"{what}: distances are not bit-identical"


def check(index, search, diverse, d, fetch_k, ks, what):
    cand = search(fetch_k)
    fetched = rows_of(index, cand, d)
    for k in ks:
        for lam, distinct in SETTINGS:
            same(diverse(k, fetch_k, lam, distinct), reference(index, cand, k, lam, distinct, d, fetched),
                 f"{what} fetch_k={fetch_k} k={k} lam={lam} distinct={distinct}")
    return cand


# ---- the inverted lists -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("d", [20, 384])
def test_ivf_search_diverse(fv, ctx, d, dtype):
    n, nlist, n_probe = 3000, 16, 5
    x = mixture(n, d, n_comp=12, seed=7 + d)
    x[1500:1520] = x[40:60]  # the same rows under other ids: the paraphrases a diverse search is for
    ids = np.arange(n, dtype=np.uint64) + 1000
    ix = fv.IVFIndex(ctx, n_clusters=nlist, n_probe=n_probe, row_dtype=dtype)
    ix.set_trained(x[:nlist])
    assert ix.batch_insert(ids, x) == (n, 0)
    q = np.concatenate([mixture(13, d, n_comp=12, seed=8), x[[40, 41, 1500]]])
    what = f"ivf d={d} {dtype}"
    check(ix, lambda f: ix.search(q, f, n_probe), lambda k, f, lam, dis: ix.search_diverse(q, k, f, lam, dis, n_probe=n_probe),
          d, 32, (1, 10, 32), what)
    check(ix, lambda f: ix.search(q, f, n_probe), lambda k, f, lam, dis: ix.search_diverse(q, k, f, lam, dis, n_probe=n_probe),
          d, 65, (10,), what)
    # under an allow-set
    allowed = ids[(np.arange(n) % 3) != 1]
    check(ix, lambda f: ix.search_allowed(q, f, allowed, n_probe),
          lambda k, f, lam, dis: ix.search_diverse(q, k, f, lam, dis, n_probe=n_probe, allowed=allowed), d, 32, (10,), what + " allowed")
    few = ids[[5, 40, 1500, 2000]]  # fewer allowed rows than k
    cand = check(ix, lambda f: ix.search_allowed(q, f, few, nlist),
                 lambda k, f, lam, dis: ix.search_diverse(q, k, f, lam, dis, n_probe=nlist, allowed=few), d, 16, (10,), what + " four allowed")
    assert np.all(cand.counts == 4)
    # with deleted rows
    for i in ids[40:50]:
        ix.mark_deleted(int(i))
    cand = check(ix, lambda f: ix.search(q, f, n_probe), lambda k, f, lam, dis: ix.search_diverse(q, k, f, lam, dis, n_probe=n_probe),
                 d, 32, (10,), what + " deleted")
    assert not set(cand.ids.ravel().tolist()) & set(ids[40:50].tolist())
    # lam = 1 without distinct is the search of fetch_k cut at k, bit for bit
    res, ranks = ix.search_diverse(q, 10, 32, 1.0, False, n_probe=n_probe)
    assert np.array_equal(res.ids, cand.ids[:, :10]) and np.array_equal(bits(res.distances), bits(cand.distances[:, :10]))
    assert np.array_equal(ranks, np.tile(np.arange(10, dtype=np.uint32), (q.shape[0], 1)))


def test_a_batch_larger_than_one_staging_sub_batch(fv, ctx):
    n, d, nlist = 2000, 20, 8
    x = mixture(n, d, n_comp=8, seed=21)
    ids = np.arange(n, dtype=np.uint64)
    ix = fv.IVFIndex(ctx, n_clusters=nlist, n_probe=4)
    ix.set_trained(x[:nlist])
    assert ix.batch_insert(ids, x) == (n, 0)
    q = mixture(23, d, n_comp=8, seed=22)
    whole = ix.search_diverse(q, 10, 32, 0.5, True)
    try:
        # room for 5 queries' candidates (32 rows of 20 floats each): 23 queries take five sub-batches, the last of 3
        assert fv.index.set_diverse_stage_bytes(5 * 32 * 20 * 4) == 5 * 32 * 20 * 4
        parts = ix.search_diverse(q, 10, 32, 0.5, True)
        assert fv.index.set_diverse_stage_bytes(1) == 1  # below one query: one query at a time
        single = ix.search_diverse(q, 10, 32, 0.5, True)
    finally:
        assert fv.index.set_diverse_stage_bytes(0) == 256 << 20
    for name, got in (("five at a time", parts), ("one at a time", single)):
        same(got, (whole[0].ids, whole[0].distances, whole[1], whole[0].counts), name)
    same(whole, reference(ix, ix.search(q, 32), 10, 0.5, True, d), "the whole batch")


# ---- the graph --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("d", [20, 384])
def test_hnsw_search_diverse(fv, ctx, d, dtype):
    n, ef = 2000, 64
    x = mixture(n, d, n_comp=6, seed=3 + d)
    x[1000:1010] = x[20:30]
    ids = np.arange(n, dtype=np.uint64) + 100
    g = fv.HNSWIndex(ctx, 8, 16, 60, seed=5, row_dtype=dtype)
    assert g.batch_insert(ids, x, orc.rng_levels(5, n)) == (n, 0)
    q = np.concatenate([mixture(13, d, n_comp=6, seed=4), x[[20, 21, 1000]]])
    what = f"hnsw d={d} {dtype}"
    check(g, lambda f: g.search(q, f, ef), lambda k, f, lam, dis: g.search_diverse(q, k, f, ef, lam, dis), d, 32, (1, 10, 32), what)
    # fetch_k above ef: the walk returns at most ef rows, so there are fewer candidates than fetch_k
    cand = check(g, lambda f: g.search(q, f, 20), lambda k, f, lam, dis: g.search_diverse(q, k, f, 20, lam, dis), d, 40, (10, 30), what + " ef=20")
    assert np.all(cand.counts <= 20)
    allowed = ids[(np.arange(n) % 2) == 0]
    check(g, lambda f: g.search_allowed(q, f, ef, allowed), lambda k, f, lam, dis: g.search_diverse(q, k, f, ef, lam, dis, allowed=allowed),
          d, 32, (10,), what + " allowed")
    for i in ids[20:25]:
        g.mark_deleted(int(i))
    cand = check(g, lambda f: g.search(q, f, ef), lambda k, f, lam, dis: g.search_diverse(q, k, f, ef, lam, dis), d, 32, (10,), what + " deleted")
    assert not set(cand.ids.ravel().tolist()) & set(ids[20:25].tolist())


def test_an_empty_graph_has_nothing_to_choose_from(fv, ctx):
    g = fv.HNSWIndex(ctx, 8, 16, 60, seed=5)
    res, ranks = g.search_diverse(np.zeros((3, 20), np.float32), 5, 16, 50)
    assert np.all(res.counts == 0) and np.all(res.ids == M.NO_ID) and np.all(np.isposinf(res.distances)) and np.all(ranks == M.NO_ROW)


# ---- the hybrid index: a migrated row sits in both parts ----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("d", [20, 384])
def test_hybrid_search_diverse_before_and_after_a_migration(fv, ctx, d, dtype):
    n, nlist, k, fetch_k = 2100, 12, 10, 32
    # One Gaussian: the reference keeps a node's nearest M links, which cuts a clustered data set into islands the walk
    # cannot leave; here the walk reaches the rows the four last queries sit on, so it returns the migrated twins.
    x = mixture(n, d, n_comp=1, seed=31 + d)
    ids = np.arange(n, dtype=np.uint64) + 10
    now = 1000 * DAY
    age = np.where(np.arange(n) % 3 == 0, 5 * DAY, 30 * DAY)  # 700 recent rows, 1400 historical ones
    age[:60] = 6.5 * DAY                                      # recent now, due for migration half a day later
    h = fv.HybridIndex(ctx, max_connections=8, max_connections_layer_0=16, ef_construction=60, n_clusters=nlist, n_probe=3,
                       row_dtype=dtype)
    h.set_ivf_centroids(x[:nlist])
    h.bulk_insert(ids, x, now - age, now)
    q = np.concatenate([mixture(12, d, n_comp=1, seed=32), x[[0, 1, 2, 5]]])  # four queries on rows about to migrate
    kw = dict(hnsw_ef=64, ivf_n_probe=4)
    what = f"hybrid d={d} {dtype}"

    def run(now_, tag, **more):
        kw2 = dict(kw, **more)
        search = (lambda f: h.search_allowed(q, f, kw2["allowed"], now=now_, **kw)) if "allowed" in more else \
                 (lambda f: h.search(q, f, now=now_, **kw2))
        return check(h, search, lambda k_, f, lam, dis: h.search_diverse(q, k_, f, lam, dis, now=now_, **kw2), d, fetch_k, (k,),
                     f"{what} {tag}")

    run(now, "before")
    run(now, "before, recent only", search_historical=False)
    run(now, "before, historical only", search_recent=False)
    hist_before = h.historical_count()
    later = now + 1 * DAY  # rows 0..59 are now 7.5 days old: the search's own migration step copies them to the lists
    cand = run(later, "after")
    assert h.historical_count() > hist_before
    # a migrated row still sits in the graph: the candidates hold it twice, as search() returns it
    dup = [b for b in range(q.shape[0]) if len(set(cand.ids[b, :cand.counts[b]].tolist())) < cand.counts[b]]
    assert dup, "no query saw a migrated id twice among its candidates"
    assert list(cand.ids[12, :2]) == [10, 10]
    # lam = 1 without distinct: search(fetch_k)[:k] bit for bit, the twin included
    res, ranks = h.search_diverse(q, k, fetch_k, 1.0, False, now=later, **kw)
    assert np.array_equal(res.ids, cand.ids[:, :k]) and np.array_equal(bits(res.distances), bits(cand.distances[:, :k]))
    assert list(res.ids[12, :2]) == [10, 10]
    # lam = 1 with distinct: the de-duplicated search — unique ids, each the first of its copies, still nearest first
    res, ranks = h.search_diverse(q, k, fetch_k, 1.0, True, now=later, **kw)
    for b in range(q.shape[0]):
        c = int(res.counts[b])
        got = res.ids[b, :c].tolist()
        assert len(set(got)) == c
        first = list(dict.fromkeys(cand.ids[b, :cand.counts[b]].tolist()))[:k]
        assert got == first
        assert np.all(np.diff(bits(res.distances[b, :c]).astype(np.int64)) >= 0)
    assert res.ids[12, 0] == 10 and res.ids[12, 1] != 10
    # at lam < 1 the twin (m = 0 once its copy is picked) is demoted even without distinct.  (Not at lam = 0.5 HERE: the
    # query is the picked row itself, so every other candidate has m = dq and a gain of exactly 0 as well.)
    res, ranks = h.search_diverse(q, 2, fetch_k, 0.25, False, now=later, **kw)
    assert res.ids[12, 0] == 10 and res.ids[12, 1] != 10
    # under an allow-set, after the migration
    allowed = ids[(np.arange(n) % 5) != 3]
    run(later, "after, allowed", allowed=allowed)
    # one allow-set per query
    sets = [None, allowed, ids[:300]]
    group = np.arange(q.shape[0], dtype=np.uint32) % 3
    cand = h.search_allowed_groups(q, fetch_k, sets, group, now=later, **kw)
    fetched = rows_of(h, cand, d)
    for lam, distinct in SETTINGS:
        same(h.search_diverse_groups(q, k, fetch_k, sets, group, lam, distinct, now=later, **kw),
             reference(h, cand, k, lam, distinct, d, fetched), f"{what} groups lam={lam} distinct={distinct}")


def test_refusals(fv, ctx):
    d = 8
    x = mixture(200, d, n_comp=2, seed=1)
    ids = np.arange(200, dtype=np.uint64)
    ix = fv.IVFIndex(ctx, n_clusters=4, n_probe=2)
    ix.set_trained(x[:4])
    ix.batch_insert(ids, x)
    g = fv.HNSWIndex(ctx, 4, 8, 20, seed=1)
    g.batch_insert(ids, x, orc.rng_levels(1, 200))
    h = fv.HybridIndex(ctx, n_clusters=4, n_probe=2)
    h.set_ivf_centroids(x[:4])
    h.bulk_insert(ids, x, np.zeros(200), 1.0)
    q = x[:3]
    calls = [lambda k, f, lam: ix.search_diverse(q, k, f, lam), lambda k, f, lam: g.search_diverse(q, k, f, 30, lam),
             lambda k, f, lam: h.search_diverse(q, k, f, lam, now=1.0)]
    for call in calls:
        for k, f in ((1, 0), (1, 257), (300, 300)):
            with pytest.raises(fv.Unsupported):
                call(k, f, 0.5)
        for k, f, lam in ((0, 8, 0.5), (9, 8, 0.5), (2, 8, float("nan")), (2, 8, -0.1), (2, 8, 1.01)):
            with pytest.raises(fv.InvalidConfig):
                call(k, f, lam)
        res, ranks = call(2, 8, 0.5)
        assert np.all(res.counts == 2)
    with pytest.raises(fv.DimensionMismatch):
        ix.search_diverse(np.zeros((1, d + 1), np.float32), 2, 8)
    # A sharded index refuses with Unsupported (HybridIndex::search_diverse, and _refuse_when_sharded before it).  An index
    # becomes sharded only through bulk_insert_sharded or attach_comm; the first needs no communicator.
    hs = fv.HybridIndex(ctx, n_clusters=4, n_probe=2)
    hs.set_ivf_centroids(x[:4])
    hs.bulk_insert_sharded(ids, x, np.zeros(200), 30 * DAY, rank=0, world=2)
    with pytest.raises(fv.Unsupported):
        hs.search_diverse(q, 2, 8, now=30 * DAY)
