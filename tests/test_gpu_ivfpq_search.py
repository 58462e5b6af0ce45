"""GPU: the inverted file over PQ codes (fvdb_ivfpq_*) against tests/_pq_ref.py restricted to the
probed lists: ids, f32 distance bits and counts of the ADC and the refined search, under deletions and an allow-set, with
lists of 0, 1, 63, 64, 65 and 1150 rows filled over several adds, one to three code words a row, table sizes that give QT
4, 2 and 1 on a 160 KiB LDS; and bit
equality with PQIndex when every list is probed."""
import numpy as np
import pytest

import fvdb_import
import _pq_ref as ref

pytestmark = pytest.mark.gpu

NO_ID = np.iinfo(np.uint64).max
NLIST = 8
SIZES = [0, 1, 63, 64, 65, 1150, 800, 857]  # rows of list 0 .. 7: 3000 in all
GEOMS = [(8, 8, 256), (10, 3, 256), (24, 24, 256), (384, 48, 256)]  # one short word; uneven subspaces; two words; three
SEED = 39  # a draw whose nearest-centroid choices are unambiguous at every d used here (asserted below)
GAP = 1e-3
NQ = 34


def ranking(cents, v):
    """f64: every row of v's centroids by ascending distance (ties to the lower id), and those distances"""
    d2 = np.stack([((v.astype(np.float64) - c.astype(np.float64)) ** 2).sum(1) for c in cents], axis=1)
    order = np.argsort(d2, axis=1, kind="stable")
    return order, np.sqrt(np.take_along_axis(d2, order, axis=1))


def make_case(d, m, ksub):
    rng = np.random.default_rng(SEED)
    cents = (rng.standard_normal((NLIST, d)) * (1.0 + 0.5 * np.arange(NLIST))[:, None]).astype(np.float32)
    label = rng.permutation(np.repeat(np.arange(NLIST), SIZES))
    x = (cents[label] + 0.1 * rng.standard_normal((label.size, d))).astype(np.float32)
    big = np.flatnonzero(label == 5)
    x[big[1::9]] = x[big[0]]  # duplicated rows: equal keys but for the ordinal
    q = (cents[np.arange(NQ) % NLIST] + 0.1 * rng.standard_normal((NQ, d))).astype(np.float32)
    q[1] = x[3]
    order, dist = ranking(cents, x)
    assert np.array_equal(order[:, 0], label) and np.all(dist[:, 1] - dist[:, 0] >= GAP * dist[:, 1])
    probes, pd = ranking(cents, q)
    assert np.all(pd[:, 1:] - pd[:, :-1] >= GAP * pd[:, 1:])  # the reference's probe order is the only one
    books = [(2.0 * rng.standard_normal((ksub, dj))).astype(np.float32) for _, dj in ref.geom(d, m)]  # drawn, not trained
    codes = ref.encode(x, books, d, m)
    return dict(d=d, m=m, ksub=ksub, cents=cents, x=x, q=q, label=label, probes=probes, books=books,
                dist=ref.adc(ref.tables(q, books, d, m), codes), ids=np.arange(label.size, dtype=np.uint64) * 3 + 7)


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    c = fv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(fv, ctx):
    out = {}
    for g in GEOMS + [(10, 3, 2)]:
        case = make_case(*g)
        case["pq"] = fv.ProductQuantizer(ctx, g[0], g[1], g[2])
        case["pq"].set_codebooks(ref.join_books(case["books"]), g[2])
        out[g] = case
    return out


def build(fv, ctx, case, refine=None):
    ix = fv.IVFPQIndex(ctx, case["pq"], NLIST, refine_rows=refine)
    ix.set_centroids(case["cents"])
    n = case["x"].shape[0]
    for a in range(0, n, 1100):  # several adds: blocks are completed across calls
        ix.add(case["ids"][a:a + 1100], case["x"][a:a + 1100])
    assert ix.rows() == n and ix.live() == n and list(ix.list_sizes()) == SIZES
    return ix


@pytest.fixture(scope="module")
def indexes(fv, ctx, cases):
    out = {g: build(fv, ctx, cases[g]) for g in cases}
    yield out
    for ix in out.values():
        ix.close()


def want_adc(case, B, nprobe, live, k):
    """per query: ref.select over the rows that are live and lie in its first nprobe lists (add-order indices)"""
    out = []
    for b in range(B):
        rows = np.flatnonzero(live & np.isin(case["label"], case["probes"][b, :nprobe])).astype(np.uint32)
        out.append(ref.select(np.ascontiguousarray(case["dist"][b, rows]), rows, k))
    return out


def check(res, want, ids):
    for b, (rows, dist) in enumerate(want):
        c = rows.size
        assert res.counts[b] == c, (b, res.counts[b], c)
        assert np.array_equal(res.ids[b, :c], ids[rows]), (b, res.ids[b, :c], ids[rows])
        assert np.array_equal(res.distances[b, :c].view(np.uint32), dist.view(np.uint32)), b
        assert np.all(res.ids[b, c:] == NO_ID) and np.all(np.isinf(res.distances[b, c:]))


@pytest.mark.parametrize("nprobe", [1, 3, NLIST])
@pytest.mark.parametrize("geom", GEOMS + [(10, 3, 2)])
def test_probed_search(cases, indexes, geom, nprobe):
    case, ix = cases[geom], indexes[geom]
    live = np.ones(case["label"].size, bool)
    info = ix.info()
    qt = info["queries_per_workgroup"]
    per, limit = geom[1] * case["pq"].info()["table_stride"] * 4, info["lds_limit"]  # bytes of one query's table
    fits = [q for q in (4, 2, 1) if 2 * per * q <= limit] or [q for q in (4, 2, 1) if per * q <= limit]
    assert qt == fits[0] and info["lds_bytes"] == qt * per <= limit
    assert limit != 160 << 10 or qt == {8: 4, 3: 4, 24: 2, 48: 1}[geom[1]]  # the three instantiations, on a 160 KiB LDS
    for B in [1, qt + 1, 33]:
        for k in [1, 10, 65, 256]:  # above the candidates where a query probes the short lists
            check(ix.search(case["q"][:B], k, nprobe), want_adc(case, B, nprobe, live, k), case["ids"])
    info = ix.info()
    assert 1 <= info["last_slices"] <= nprobe and info["pairs"] == 33 * nprobe
    assert info["rows_scored"] == sum(SIZES[L] for b in range(33) for L in case["probes"][b, :nprobe])


@pytest.mark.parametrize("geom", GEOMS)
def test_every_list_probed_equals_flat_index(fv, ctx, cases, indexes, geom):
    case = cases[geom]
    flat = fv.PQIndex(ctx, case["pq"])
    flat.add(case["ids"], case["x"])
    for k in [10, 256]:
        a, b = indexes[geom].search(case["q"], k, NLIST), flat.search(case["q"], k)
        assert np.array_equal(a.ids, b.ids) and np.array_equal(a.counts, b.counts)
        assert np.array_equal(a.distances.view(np.uint32), b.distances.view(np.uint32))
    flat.close()


def test_filters(fv, ctx, cases):
    case = cases[GEOMS[1]]
    n = case["label"].size
    ix = build(fv, ctx, case)
    live = np.ones(n, bool)
    live[2::7] = False
    live[case["label"] == 4] = False  # every row of a list that its own queries probe first
    ix.mark_deleted(case["ids"][~live])
    assert ix.live() == int(live.sum())
    for nprobe in [1, 3]:
        check(ix.search(case["q"], 10, nprobe), want_adc(case, NQ, nprobe, live, 10), case["ids"])
    mask = np.zeros(n, bool)
    mask[1::3] = True
    check(ix.search(case["q"][:9], 65, 3, allowed=case["ids"][mask]), want_adc(case, 9, 3, live & mask, 65), case["ids"])
    ix.mark_deleted(case["ids"][~live], deleted=False)
    check(ix.search(case["q"][:9], 10, 3), want_adc(case, 9, 3, np.ones(n, bool), 10), case["ids"])
    ix.close()


@pytest.mark.parametrize("rows", ["f32", "f16"])
def test_refined_search(fv, ctx, cases, rows):
    case, k, B, nprobe = cases[GEOMS[1]], 10, 9, 3
    ix = build(fv, ctx, case, refine=rows)
    stored = case["x"] if rows == "f32" else case["x"].astype(np.float16).astype(np.float32)  # rounded once
    for fetch_k in [k, 64, 256]:
        res = ix.search(case["q"][:B], k, nprobe, fetch_k=fetch_k)
        cand = want_adc(case, B, nprobe, np.ones(case["label"].size, bool), fetch_k)
        check(res, [ref.refine(case["q"][b], stored, cand[b][0], k) for b in range(B)], case["ids"])
    ix.close()


def test_refusals(fv, ctx, cases):
    case = cases[GEOMS[1]]
    E = fv.engine
    raw = fv.ProductQuantizer(ctx, 10, 3, 256)
    with pytest.raises(E.NotTrained):
        fv.IVFPQIndex(ctx, raw, NLIST)  # quantizer untrained
    raw.close()
    with pytest.raises(E.Unsupported):
        fv.IVFPQIndex(ctx, case["pq"], 16385)
    ix = fv.IVFPQIndex(ctx, case["pq"], NLIST)
    with pytest.raises(E.NotTrained):
        ix.add(case["ids"][:4], case["x"][:4])  # centroids unset
    with pytest.raises(E.NotTrained):
        ix.search(case["q"][:1], 1, 1)
    ix.set_centroids(case["cents"])
    ix.add(case["ids"][:40], case["x"][:40])
    bad = case["x"][40:42].copy()
    bad[1, 5] = np.nan
    with pytest.raises(E.NonFiniteInput):
        ix.add(case["ids"][40:42], bad)
    with pytest.raises(E.NonFiniteInput):
        ix.search(bad, 1, 1)
    with pytest.raises(E.DuplicateVector):
        ix.add(case["ids"][39:41], case["x"][39:41])
    with pytest.raises(E.InvalidConfig):
        ix.search(case["q"][:1], 1, 0)
    with pytest.raises(E.Unsupported):
        ix.search(case["q"][:1], 257, 1)
    with pytest.raises(E.InvalidConfig):
        ix.search(case["q"][:1], 2, 1, fetch_k=4)  # no refine rows
    with pytest.raises(E.Unsupported):
        ix.set_centroids(case["cents"])  # rows are held
    assert ix.rows() == 40 and ix.live() == 40 and int(ix.list_sizes().sum()) == 40  # nothing was written
    live = np.zeros(case["label"].size, bool)
    live[:40] = True
    check(ix.search(case["q"][:5], 10, NLIST), want_adc(case, 5, NLIST, live, 10), case["ids"])
    ix.close()
    # refined: fetch_k above 256
    rix = fv.IVFPQIndex(ctx, case["pq"], NLIST, refine_rows="f32")
    rix.set_centroids(case["cents"])
    with pytest.raises(E.Unsupported):
        rix.search(case["q"][:1], 2, 1, fetch_k=257)
    rix.close()
    # a table that does not fit LDS once: 192 subspaces x 256 entries x 4 bytes
    wide = fv.ProductQuantizer(ctx, 192, 192, 256)
    wide.set_codebooks(np.zeros(192 * 256, np.float32), 256)
    assert wide.info()["queries_per_workgroup"] == 0
    wix = fv.IVFPQIndex(ctx, wide, 2)
    wix.set_centroids(np.eye(2, 192, dtype=np.float32))
    with pytest.raises(E.Unsupported):
        wix.search(np.zeros((1, 192), np.float32), 1, 1)
    wix.close()
    wide.close()
    # changed codebooks invalidate the index
    pq = fv.ProductQuantizer(ctx, 10, 3, 256)
    pq.set_codebooks(ref.join_books(case["books"]), 256)
    vix = fv.IVFPQIndex(ctx, pq, NLIST)
    vix.set_centroids(case["cents"])
    pq.set_codebooks(ref.join_books(case["books"]), 256)
    with pytest.raises(E.InvalidConfig):
        vix.search(case["q"][:1], 1, 1)
    vix.close()
    pq.close()
