"""GPU: search_grouped of the three index classes.

The result must equal _group_cases.select_batch applied to that index's OWN search(fetch_k) result (search_allowed under
an allow-set) with each candidate's key taken from the metadata map on the host: every output array exactly, ids and f32
distance bits included.  fetch_k = 64 runs the register route and the small selection, fetch_k = 600 the wide route and
the full one.  What these tests add to test_gpu_group_select.py and test_gpu_meta_keys.py, which check the two kernels
alone: the candidates' order, the column built from the map on first use, and the join through the id index."""
import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture
import _group_cases as G

pytestmark = pytest.mark.gpu

DAY = 86400.0
N, D = 2000, 16
MODES = ((True, "drop"), (False, "own"), (True, "own"), (False, "drop"))  # (distinct, missing)
SHAPES = ((1, 1), (5, 2), (40, 3))                                        # (k, group_size)


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def metadata_map(ids):
    """name -> metadata for every row but a few (no entry: no key), a few dozen distinct keys per path"""
    rows, md = {}, {}
    for i, rid in enumerate(ids.tolist()):
        name = f"row{i}"
        rows[rid] = name
        if i % 97 == 13:
            continue  # in the index, not in the map
        m = {"doc": f"doc{i % 37}", "n": {"shard": i % 29}, "score": [1.0, 1, "1", True, 0.0, -0.0, float("nan"), None][i % 8]}
        if i % 11 == 0:
            del m["doc"]          # the field is missing
        if i % 53 == 0:
            m["doc"] = ["a", "b"]  # an array has no key
        if i % 59 == 0:
            m["doc"] = {"x": 1}    # nor has an object
        md[name] = m
    return rows, md


def host_keys(fv, cols, rows, md, path, cand):
    """key_tag / key_val [B][fetch_k] of the candidates, from the map (after the column exists: the codes are the table's)"""
    mc = fv.metadata_columns
    tag = np.zeros(cand.ids.shape, np.uint8)
    val = np.zeros(cand.ids.shape, np.uint64)
    for b in range(cand.ids.shape[0]):
        for c in range(int(cand.counts[b])):
            m = md.get(rows.get(int(cand.ids[b, c])))
            if m is None:
                continue
            t, payload, _ = mc.encode_cell(m, path, dict(cols.strings))  # a copy: a lookup must not hand out codes
            key = G.cell_key(t, payload)
            if key is not None:
                tag[b, c], val[b, c] = key
    return tag, val


def same(res, want, what):
    got = dict(ids=res.ids, dist=res.distances, rank=res.ranks, members=res.members, total=res.totals, key_tag=res.key_tags,
               key_val=res.key_words, groups=res.groups, flags=res.flags)
    for name in G.NAMES:
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if name == "dist":
            g, w = bits(g), bits(w)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {name} differs first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"


def check(fv, cols, rows, md, search, grouped, fetch_k, what, paths=("doc", "n.shard", "score")):
    cand = search(fetch_k)
    assert cand.counts.max() > 0, what
    seen = set()
    for p, path in enumerate(paths):
        cols.group_column(path)
        tag, val = host_keys(fv, cols, rows, md, path, cand)
        seen |= set(zip(tag.ravel().tolist(), val.ravel().tolist()))
        for s, (k, gs) in enumerate(SHAPES):
            distinct, missing = MODES[(p + s) % 4]
            want = G.select_batch(cand.ids, cand.distances, cand.counts, tag, val, k, gs, distinct, G.DROP if missing == "drop" else G.OWN)
            same(grouped(k, gs, fetch_k, path, distinct, missing), want, f"{what} fetch_k={fetch_k} path={path} k={k} gs={gs} "
                                                                         f"distinct={distinct} missing={missing}")
    return cand, seen


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_ivf_search_grouped(fv, ctx, dtype):
    nlist, n_probe = 16, 6
    x = mixture(N, D, n_comp=10, seed=5)
    ids = (np.arange(N, dtype=np.uint64) << np.uint64(33)) + np.uint64(7)  # 64-bit ids: the low words are all equal
    rows, md = metadata_map(ids)
    ix = fv.IVFIndex(ctx, n_clusters=nlist, n_probe=n_probe, row_dtype=dtype)
    ix.set_trained(x[:nlist])
    assert ix.batch_insert(ids, x) == (N, 0)
    cols = fv.metadata_columns.MetadataColumns(ctx, rows, md)
    q = np.concatenate([mixture(9, D, n_comp=10, seed=6), x[[0, 13, 110]]])
    try:
        run = lambda k, gs, f, path, dis, mis: ix.search_grouped(q, k, gs, f, cols, path, dis, mis, n_probe=n_probe)  # noqa: E731
        fetch_ks = (64, 600) if dtype == "f32" else (64,)
        for fetch_k in fetch_ks:
            cand, seen = check(fv, cols, rows, md, lambda f: ix.search(q, f, n_probe), run, fetch_k, f"ivf {dtype}")
            assert {t for t, _ in seen} >= {G.MISSING, G.NULL, G.BOOL, G.INT, G.FLOAT, G.STRING}
        if dtype == "f16":
            return
        assert cand.counts.max() > 256  # the wide route was taken
        allowed = ids[(np.arange(N) % 3) != 1]
        for fetch_k in fetch_ks:
            check(fv, cols, rows, md, lambda f: ix.search_allowed(q, f, allowed, n_probe),
                  lambda k, gs, f, path, dis, mis: ix.search_grouped(q, k, gs, f, cols, path, dis, mis, n_probe=n_probe, allowed=allowed),
                  fetch_k, "ivf allowed", paths=("doc",))
        # a deleted row is no candidate; a row whose entry left the map has no key any more
        for i in ids[[0, 110]]:
            ix.mark_deleted(int(i))
        gone = rows[int(ids[1])]
        del md[gone]
        cols.set_absent(int(ids[1]))
        cand, _ = check(fv, cols, rows, md, lambda f: ix.search(q, f, n_probe), run, 64, "ivf deleted", paths=("doc",))
        assert not set(cand.ids.ravel().tolist()) & set(ids[[0, 110]].tolist())
        # the completeness facts: a list of 64 that was cut, and one that was not (more room than candidates)
        res = ix.search_grouped(q, 40, 1, 64, cols, "doc", n_probe=n_probe)
        assert all(res.cut(b) for b in range(len(res))) and not any(res.groups_complete(b) for b in range(len(res)))  # 37 docs < 40
        res = ix.search_grouped(q[:2], 40, 1, 4096, cols, "doc", n_probe=n_probe)
        assert not res.cut(0) and res.groups_complete(0) and int(res.groups[0]) <= 37 and res.group_complete(0, 0)
    finally:
        cols.close()


def test_hnsw_search_grouped(fv, ctx):
    x = mixture(N, D, n_comp=1, seed=8)
    ids = np.arange(N, dtype=np.uint64) + 100
    rows, md = metadata_map(ids)
    g = fv.HNSWIndex(ctx, 8, 16, 60, seed=5)
    assert g.batch_insert(ids, x, orc.rng_levels(5, N)) == (N, 0)
    cols = fv.metadata_columns.MetadataColumns(ctx, rows, md)
    q = np.concatenate([mixture(9, D, n_comp=1, seed=9), x[[0, 13, 110]]])
    try:
        for fetch_k, ef in ((64, 80), (600, 700)):
            check(fv, cols, rows, md, lambda f: g.search(q, f, ef), lambda k, gs, f, path, dis, mis: g.search_grouped(q, k, gs, f, ef, cols, path, dis, mis),
                  fetch_k, f"hnsw ef={ef}")
        allowed = ids[(np.arange(N) % 2) == 0]
        check(fv, cols, rows, md, lambda f: g.search_allowed(q, f, 80, allowed),
              lambda k, gs, f, path, dis, mis: g.search_grouped(q, k, gs, f, 80, cols, path, dis, mis, allowed=allowed), 64, "hnsw allowed",
              paths=("doc",))
        g.mark_deleted(int(ids[0]))
        cand, _ = check(fv, cols, rows, md, lambda f: g.search(q, f, 80), lambda k, gs, f, path, dis, mis: g.search_grouped(q, k, gs, f, 80, cols, path, dis, mis),
                        64, "hnsw deleted", paths=("doc",))
        assert int(ids[0]) not in set(cand.ids.ravel().tolist())
        # fetch_k above ef: fewer candidates than fetch_k, so a list that was not cut
        res = g.search_grouped(q, 5, 2, 64, 20, cols, "doc")
        assert not any(res.cut(b) for b in range(len(res)))
    finally:
        cols.close()


def test_hybrid_search_grouped_with_rows_in_both_parts(fv, ctx):
    n, nlist = 2100, 12
    x = mixture(n, D, n_comp=1, seed=31)
    ids = np.arange(n, dtype=np.uint64) + 10
    rows, md = metadata_map(ids)
    now = 1000 * DAY
    age = np.where(np.arange(n) % 3 == 0, 5 * DAY, 30 * DAY)
    age[:60] = 6.5 * DAY  # recent now, due for migration half a day later
    h = fv.HybridIndex(ctx, max_connections=8, max_connections_layer_0=16, ef_construction=60, n_clusters=nlist, n_probe=3)
    h.set_ivf_centroids(x[:nlist])
    h.bulk_insert(ids, x, now - age, now)
    cols = fv.metadata_columns.MetadataColumns(ctx, rows, md)
    q = np.concatenate([mixture(8, D, n_comp=1, seed=32), x[[0, 1, 2, 5]]])  # four queries on rows about to migrate
    try:
        for fetch_k, kw in ((64, dict(hnsw_ef=64, ivf_n_probe=4)), (600, dict(hnsw_ef=300, ivf_n_probe=12))):
            check(fv, cols, rows, md, lambda f: h.search(q, f, now=now, **kw),
                  lambda k, gs, f, path, dis, mis: h.search_grouped(q, k, gs, f, cols, path, dis, mis, now=now, **kw), fetch_k, "hybrid before")
        later = now + 1 * DAY  # the search's own migration step copies rows 0..59 to the lists; they still sit in the graph
        kw = dict(hnsw_ef=64, ivf_n_probe=4)
        before = h.historical_count()
        cand, _ = check(fv, cols, rows, md, lambda f: h.search(q, f, now=later, **kw),
                        lambda k, gs, f, path, dis, mis: h.search_grouped(q, k, gs, f, cols, path, dis, mis, now=later, **kw), 64, "hybrid after")
        assert h.historical_count() > before
        assert list(cand.ids[9, :2]) == [11, 11], "the migrated row was not returned twice"  # query 9 sits on row 1 (doc1)
        # distinct on: the twin takes one seat of its group; off: two
        on = h.search_grouped(q, 3, 4, 64, cols, "doc", True, "drop", now=later, **kw)
        off = h.search_grouped(q, 3, 4, 64, cols, "doc", False, "drop", now=later, **kw)
        assert on.ids[9, 0, 0] == 11 and on.ids[9, 0, 1] != 11 and list(off.ids[9, 0, :2]) == [11, 11]
        assert int(off.totals[9, 0]) > int(on.totals[9, 0])
        for fetch_k in (64, 600):
            kw = dict(hnsw_ef=64 if fetch_k == 64 else 300, ivf_n_probe=4)
            allowed = ids[(np.arange(n) % 5) != 3]
            check(fv, cols, rows, md, lambda f: h.search_allowed(q, f, allowed, now=later, **kw),
                  lambda k, gs, f, path, dis, mis: h.search_grouped(q, k, gs, f, cols, path, dis, mis, now=later, allowed=allowed, **kw),
                  fetch_k, "hybrid after, allowed", paths=("doc", "n.shard"))
        h.delete(int(ids[3]), later)
        cand, _ = check(fv, cols, rows, md, lambda f: h.search(q, f, now=later, **kw),
                        lambda k, gs, f, path, dis, mis: h.search_grouped(q, k, gs, f, cols, path, dis, mis, now=later, **kw), 64, "hybrid deleted",
                        paths=("doc",))
        assert int(ids[3]) not in set(cand.ids.ravel().tolist())
    finally:
        cols.close()


def test_refusals(fv, ctx):
    d = 8
    x = mixture(200, d, n_comp=2, seed=1)
    ids = np.arange(200, dtype=np.uint64)
    rows, md = metadata_map(ids)
    ix = fv.IVFIndex(ctx, n_clusters=4, n_probe=2)
    ix.set_trained(x[:4])
    ix.batch_insert(ids, x)
    g = fv.HNSWIndex(ctx, 4, 8, 20, seed=1)
    g.batch_insert(ids, x, orc.rng_levels(1, 200))
    h = fv.HybridIndex(ctx, n_clusters=4, n_probe=2)
    h.set_ivf_centroids(x[:4])
    h.bulk_insert(ids, x, np.zeros(200), 1.0)
    cols = fv.metadata_columns.MetadataColumns(ctx, rows, md)
    q = x[:3]
    try:
        calls = [lambda k, gs, f, **kw: ix.search_grouped(q, k, gs, f, cols, "doc", **kw),
                 lambda k, gs, f, **kw: g.search_grouped(q, k, gs, f, 30, cols, "doc", **kw),
                 lambda k, gs, f, **kw: h.search_grouped(q, k, gs, f, cols, "doc", now=1.0, **kw)]
        for call in calls:
            for k, gs, f in ((1, 1, 0), (1, 1, 4097), (4097, 1, 8), (586, 7, 8), (1, 4097, 8)):
                with pytest.raises(fv.Unsupported):
                    call(k, gs, f)
            for k, gs, f in ((0, 1, 8), (1, 0, 8)):
                with pytest.raises(fv.InvalidConfig):
                    call(k, gs, f)
            with pytest.raises(fv.InvalidConfig):
                call(2, 2, 8, missing="keep")
            res = call(2, 2, 8)
            assert np.all(res.groups == 2) and res.ids.shape == (3, 2, 2)
        with pytest.raises(fv.DimensionMismatch):
            ix.search_grouped(np.zeros((1, d + 1), np.float32), 2, 1, 8, cols, "doc")
        hs = fv.HybridIndex(ctx, n_clusters=4, n_probe=2)
        hs.set_ivf_centroids(x[:4])
        hs.bulk_insert_sharded(ids, x, np.zeros(200), 30 * DAY, rank=0, world=2)
        with pytest.raises(fv.Unsupported):
            hs.search_grouped(q, 2, 1, 8, cols, "doc", now=30 * DAY)
    finally:
        cols.close()
