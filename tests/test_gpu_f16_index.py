"""GPU: row_dtype="f16" on the index classes: IVFIndex, HybridIndex, VectorDbSession and the
chunked loader.  The classes are given unrounded rows and round them once at the door; the CPU oracle is given
`x.astype(float16).astype(float32)`.  Ids and f32 distance bits must be the oracle's, a row must read back as the same
rounded value wherever it lives (graph store, a list after migration, a chunked file), and training data, centroids
and queries stay f32."""
import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture
from test_gpu_ivf_maintenance import assert_same_index, assert_same_results, restated_retrain

pytestmark = pytest.mark.gpu
DAY = 86400.0


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def rounded(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def same(g, ref):
    oi, od, oc = ref
    assert np.array_equal(g.counts, oc), f"hit counts differ: {g.counts[:8]} vs {oc[:8]}"
    for b in range(len(g)):
        n = int(oc[b])
        assert np.array_equal(g.ids[b, :n], oi[b, :n]), f"query {b}: ids differ"
        assert np.array_equal(bits(g.distances[b, :n]), bits(od[b, :n])), f"query {b}: distances not bit-identical"


# ---- IVFIndex -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [20, 384])
def test_ivf_index_is_the_oracle_on_the_rounded_rows(fv, ctx, d):
    n, nlist = 3000, 16
    x = mixture(n, d, n_comp=20, seed=d)
    xr = rounded(x)
    ids = np.arange(n, dtype=np.uint64) * 3 + 11
    rows = {int(i): xr[j] for j, i in enumerate(ids)}
    cfg = dict(n_clusters=nlist, n_probe=4, max_iterations=12, seed=7)
    g, o = fv.IVFIndex(ctx, row_dtype="f16", **cfg), orc.IVFIndex(**cfg)
    assert g.row_dtype == "f16"
    gres, ores = g.train(x[:256]), o.train(x[:256])  # training data stays f32: the same centroids
    assert gres["iterations"] == ores["iterations"]
    assert g.batch_insert(ids, x) == (n, 0)
    o.batch_insert(ids, xr)
    q = mixture(32, d, n_comp=20, seed=d + 1)
    assert_same_index(g, o, nlist, q)
    for k, npb in ((10, 4), (300, 4), (300, nlist)):  # the register top-k and the wide selection
        assert_same_results(g.search(q, k, npb), *o.batch_search(q, k, npb))
    got, found = g.get_vectors(ids[::7])
    assert found.all() and np.array_equal(bits(got), bits(xr[::7]))
    assert np.array_equal(bits(g.export_list(0)[0]), bits(np.stack([rows[int(i)] for i in o.list_ids(0)])))
    one = mixture(1, d, seed=5)[0]  # a single insert goes through the same door
    g.insert(10 ** 6, one)
    o.insert(10 ** 6, rounded(one))
    rows[10 ** 6] = rounded(one)
    assert np.array_equal(bits(g.get_vector_by_id(10 ** 6)), bits(rounded(one)))

    # maintenance: the rows stay in HBM as halves; lists and searches are the restated oracle's
    dead = set(int(i) for i in ids[5:600:17])
    for i in dead:
        g.mark_deleted(i)
        o.mark_deleted(i)
    new = dict(n_clusters=24, n_probe=5, max_iterations=12, seed=99)
    o2, ores, _ = restated_retrain(o, nlist, rows, dead, **new)
    res = g.retrain(24, n_probe=5, max_iterations=12, seed=99)
    assert res["converged"] == ores["converged"] and res["vectors_reassigned"] == n + 1
    assert g.row_dtype == "f16" and g.n_clusters == 24
    assert_same_index(g, o2, 24, q, dead)
    o3, _, _ = restated_retrain(o2, 24, rows, dead, n_clusters=27, n_probe=5, max_iterations=12, seed=99)
    assert g.add_clusters(3) == dict(clusters_added=3, vectors_reassigned=n + 1)
    assert_same_index(g, o3, 27, q, dead)
    assert g.vacuum() == len(dead)
    o3.vacuum()
    assert_same_index(g, o3, 27, q)
    assert_same_results(g.search(q, 300, 27), *o3.batch_search(q, 300, 27))
    extra = mixture(100, d, n_comp=20, seed=6)  # life goes on: new rows are rounded like the old ones
    eid = np.arange(100, dtype=np.uint64) + 2 * 10 ** 6
    g.batch_insert(eid, extra)
    o3.batch_insert(eid, rounded(extra))
    assert_same_index(g, o3, 27, q)
    got, found = g.get_vectors(eid)
    assert found.all() and np.array_equal(bits(got), bits(rounded(extra)))


def test_ivf_index_refuses_a_row_that_rounds_to_infinity_like_an_infinite_row(fv, ctx):
    d = 16
    x = mixture(200, d, seed=3)
    g, f = fv.IVFIndex(ctx, n_clusters=4, n_probe=2, row_dtype="f16"), fv.IVFIndex(ctx, n_clusters=4, n_probe=2)
    for i in (g, f):
        i.set_trained(x[:4])
    bad, inf = x[10].copy(), x[10].copy()
    bad[2], inf[2] = 70000.0, np.inf
    for i in (g, f):
        with pytest.raises(fv.NonFiniteInput):
            i.insert(1, inf)
    with pytest.raises(fv.NonFiniteInput):
        g.insert(1, bad)
    assert g.total_vectors() == 0
    f.insert(1, bad)  # an f32 index keeps the value
    assert f.get_vector_by_id(1)[2] == np.float32(70000.0)


# ---- HybridIndex ----------------------------------------------------------------------------------------------------
KW = dict(max_connections=6, max_connections_layer_0=12, ef_construction=30, n_clusters=8, n_probe=3, auto_migrate=False)


@pytest.mark.parametrize("resident", [True, False])
def test_hybrid_index_before_and_after_migration(fv, ctx, resident):
    n, d, now = 2000, 64, 1000 * DAY
    x = mixture(n, d, n_comp=8, seed=64)
    xr = rounded(x)
    rng = np.random.default_rng(64)
    ages = np.where(rng.random(n) < 0.5, 1 * DAY, 30 * DAY)  # half old: straight to the lists; half recent: graph nodes
    levels = orc.rng_levels(64, n)
    g, o = fv.HybridIndex(ctx, row_dtype="f16", **KW), orc.HybridIndex(**KW)
    assert g.row_dtype == "f16" and g.hnsw().row_dtype == "f16" and g.ivf().row_dtype == "f16"
    g.set_resident_migration(resident)
    for h, rows in ((g, x), (o, xr)):
        h.set_ivf_centroids(x[:8])  # centroids stay f32
        for i in range(n):
            h.insert_with_timestamp(i, rows[i], now - ages[i], now, int(levels[i]))
    assert (g.recent_count(), g.historical_count()) == (o.recent_count(), o.historical_count())
    q = mixture(32, d, n_comp=8, seed=65)
    every = np.arange(n, dtype=np.uint64)

    def check():
        for kws in (dict(now=now), dict(now=now, hnsw_ef=100, ivf_n_probe=8), dict(now=now, search_recent=False, ivf_n_probe=8)):
            a = g.search(q, 10, **kws)
            for qi in range(q.shape[0]):
                r = o.search(q[qi], 10, **kws)
                m = int(a.counts[qi])
                assert m == len(r) and np.array_equal(a.ids[qi, :m], r.ids), (kws, qi)
                assert np.array_equal(bits(a.distances[qi, :m]), bits(r.distances)), (kws, qi)
        got, found = g.get_vectors(every)
        assert found.all() and np.array_equal(bits(got), bits(xr))

    check()
    recent = np.flatnonzero(ages < 7 * DAY)
    moved = g.migrate_with_threshold(0.5 * DAY, now)
    assert moved == o.migrate_with_threshold(0.5 * DAY, now) == recent.size
    assert g.migration_info()["path"] == ("resident" if resident else "host")
    check()  # a row that moved from the graph to a list reads back as the same value
    got, found = g.ivf().get_vectors(recent.astype(np.uint64))  # ... from the list itself too
    assert found.all() and np.array_equal(bits(got), bits(xr[recent]))
    gi, oi = g.ivf(), o.ivf()
    for c in range(8):
        rows, lid, _ = gi.export_list(c)
        assert lid.tolist() == oi.list_ids(c).tolist(), f"list {c}"
        assert np.array_equal(bits(rows), bits(xr[lid.astype(np.int64)])), f"list {c}"


def test_hybrid_filtered_searches_and_the_sharded_refusal(fv, ctx):
    n, d, now = 1200, 64, 1000 * DAY
    x = mixture(n, d, n_comp=8, seed=66)
    xr = rounded(x)
    rng = np.random.default_rng(66)
    ages = np.where(rng.random(n) < 0.4, 1 * DAY, 30 * DAY)
    levels = orc.rng_levels(66, n)
    kw = dict(KW, auto_migrate=True)

    def make(cls, rows, *a, **extra):
        h = cls(*a, **kw, **extra)
        h.set_ivf_centroids(x[:8])
        for i in range(n):
            h.insert_with_timestamp(i, rows[i], now - ages[i], now, int(levels[i]))
        return h

    g = make(fv.HybridIndex, x, ctx, row_dtype="f16")
    g.hnsw().scan_cutoff = 0
    q = mixture(24, d, n_comp=8, seed=67)
    ids = np.arange(n, dtype=np.uint64)
    for frac in (0.5, 0.05):
        allowed = ids[rng.random(n) < frac]
        o = make(orc.HybridIndex, xr)
        keep = set(int(i) for i in allowed)
        for i in range(n):
            if i not in keep:
                o.delete(i, now)
        same(g.search_allowed(q, 10, allowed, now=now, hnsw_ef=50, ivf_n_probe=4),
             o.batch_search(q, 10, now=now, hnsw_ef=50, ivf_n_probe=4))
    # search_with_filter: 3 k candidates from the plain search, the first k that match
    o = make(orc.HybridIndex, xr)
    odd = lambda i: i % 2 == 1  # noqa: E731
    got = g.search_with_filter(q, 10, odd, now=now)
    oi, od, oc = o.batch_search(q, 30, now=now, hnsw_ef=50, ivf_n_probe=10)
    for b in range(q.shape[0]):
        keep = [j for j in range(int(oc[b])) if odd(int(oi[b, j]))][:10]
        assert got.counts[b] == len(keep) and np.array_equal(got.ids[b, :len(keep)], oi[b, keep])
        assert np.array_equal(bits(got.distances[b, :len(keep)]), bits(od[b, keep]))
    # a sharded fp16 hybrid is not served, and says why
    for call in (lambda: g.attach_comm(1), lambda: g.bulk_insert_sharded(ids, x, now - ages, now, 0, 2)):
        with pytest.raises(fv.Unsupported, match="f16") as e:
            call()
        assert e.value.status == 12  # FVDB_E_UNSUPPORTED
    assert g.lib.fvh_hybrid_attach_comm(g.h, 1) == 12 and g.lib.fvh_hybrid_attach_comm(g.h, None) == 0


# ---- session and chunked files --------------------------------------------------------------------------------------
def test_session_returns_the_rounded_inputs(fv, ctx):
    rng = np.random.default_rng(990)
    vecs = rng.standard_normal((60, 12))  # doubles, like a JS caller's numbers
    hybrid_config = {"row_dtype": "f16"}
    s = fv.VectorDbSession(ctx, **hybrid_config)
    assert s.index.row_dtype == "f16"
    s.add_vectors([{"id": f"doc-{i}", "vector": vecs[i].tolist(), "metadata": {"n": i}} for i in range(60)])
    want = {f"doc-{i}": [float(v) for v in rounded(np.float32(vecs[i]))] for i in range(60)}
    q = vecs[3].tolist()
    got = s.search(q, 5, {"includeVectors": True})
    assert got and got[0]["id"] == "doc-3" and all(r["vector"] == want[r["id"]] for r in got)
    plain = fv.VectorDbSession(ctx)
    plain.add_vectors([{"id": f"doc-{i}", "vector": rounded(np.float32(vecs[i])).tolist(), "metadata": {"n": i}} for i in range(60)])
    ref = plain.search(q, 5, {"includeVectors": True})
    assert [(r["id"], r["score"], r["vector"]) for r in got] == [(r["id"], r["score"], r["vector"]) for r in ref]
    s.delete_vector("doc-3")
    assert all(r["id"] != "doc-3" for r in s.search(q, 5))
    s.vacuum()
    s.now += 30 * DAY  # the rows have aged: the search migrates them to the lists, and they read back the same
    got = s.search(q, 5, {"includeVectors": True})
    assert got and all(r["vector"] == want[r["id"]] for r in got)
    plain.delete_vector("doc-3")
    plain.vacuum()
    plain.now += 30 * DAY
    ref = plain.search(q, 5, {"includeVectors": True})
    assert [(r["id"], r["score"], r["vector"]) for r in got] == [(r["id"], r["score"], r["vector"]) for r in ref]


def test_chunked_save_of_an_f16_index_loads_back_with_the_same_answers(fv, ctx, tmp_path):
    ck = fv.chunked
    n, d, now = 700, 16, 1000 * DAY
    x = mixture(n, d, n_comp=8, seed=5)
    kw = dict(max_connections=8, max_connections_layer_0=16, ef_construction=40, n_clusters=8, n_probe=4)
    g = fv.HybridIndex(ctx, row_dtype="f16", **kw)
    g.set_ivf_centroids(x[:8].copy())
    table = {}
    for i in range(n):
        v = fv.VectorId(f"doc-{i}")
        table[v.row_id()] = v.bytes
        g.insert_with_timestamp(v.row_id(), x[i], now - (1 if i % 3 else 30) * DAY - i, now)
    ck.save_index_chunked(g, str(tmp_path), "idx", id_table=table, now=now, chunk_size=256)
    h, _ = ck.load_index_chunked(ctx, str(tmp_path), "idx", now=now, row_dtype="f16", **kw)
    f, _ = ck.load_index_chunked(ctx, str(tmp_path), "idx", now=now, **kw)
    assert h.row_dtype == "f16" and f.row_dtype == "f32"
    assert (h.recent_count(), h.historical_count()) == (g.recent_count(), g.historical_count())
    q = mixture(25, d, n_comp=8, seed=77)
    a = g.search(q, 10, now=now, hnsw_ef=40, ivf_n_probe=8)
    for other in (h, f):  # the file holds the rounded values: they are the same rows in either storage
        b = other.search(q, 10, now=now, hnsw_ef=40, ivf_n_probe=8)
        assert np.array_equal(a.counts, b.counts) and np.array_equal(a.ids, b.ids)
        assert np.array_equal(bits(a.distances), bits(b.distances))
    assert h.store_bytes() > 0 and 2 * h.store_bytes() == f.store_bytes()
    rid = np.array(sorted(table), np.uint64)
    (ga, gf), (ha, hf) = g.get_vectors(rid), h.get_vectors(rid)
    assert gf.all() and hf.all() and np.array_equal(bits(ga), bits(ha))
