"""GPU: search over product-quantizer codes (fvdb_pq_index_*) against the restatement of
tests/_pq_ref.py: ids, distance bits and counts of the ADC search and of the refined search, under deletions and an
allow-set, at every size where the scan takes another path (a partial block, one slice and a row, several slices)."""
import numpy as np
import pytest

import fvdb_import
import _pq_ref as ref

pytestmark = pytest.mark.gpu

GEOMS = [(10, 3, 4), (130, 4, 256), (384, 48, 256)]
NO_ID = np.iinfo(np.uint64).max
N_BIG = 3000  # several slices


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
    """per geometry: the quantizer, its books, N_BIG rows with duplicates, their reference codes and 34 queries"""
    out = {}
    for d, m, ksub in GEOMS:
        rng = np.random.default_rng(d + m)
        x = rng.standard_normal((N_BIG, d)).astype(np.float32)
        x[5::10] = x[3]  # duplicated rows: equal codes must come back in row order
        books = [x[rng.choice(N_BIG, ksub, replace=False), o:o + dj].copy() for o, dj in ref.geom(d, m)]
        pq = fv.ProductQuantizer(ctx, d, m, ksub)
        pq.set_codebooks(ref.join_books(books), ksub)
        q = rng.standard_normal((34, d)).astype(np.float32)
        q[1] = x[3]
        out[(d, m, ksub)] = dict(pq=pq, books=books, x=x, codes=ref.encode(x, books, d, m), q=q, ids=np.arange(N_BIG, dtype=np.uint64) * 3 + 7)
    return out


def check(res, want, ids, k):
    for b, (rows, dist) in enumerate(want):
        c = rows.size
        assert res.counts[b] == c, (b, res.counts[b], c)
        assert np.array_equal(res.ids[b, :c], ids[rows]), (b, res.ids[b, :c], ids[rows])
        assert np.array_equal(res.distances[b, :c].view(np.uint32), dist.view(np.uint32)), b
        assert np.all(res.ids[b, c:] == NO_ID) and np.all(np.isinf(res.distances[b, c:]))


def build(fv, ctx, case, n, refine=None, deleted=None):
    ix = fv.PQIndex(ctx, case["pq"], refine_rows=refine)
    for a in range(0, n, 1100):  # several adds: blocks are completed across calls
        ix.add(case["ids"][a:min(n, a + 1100)], case["x"][a:min(n, a + 1100)])
    live = np.ones(n, bool)
    if deleted is not None and n:
        live[deleted(n)] = False
        ix.mark_deleted(case["ids"][:n][~live])
    assert ix.rows() == n and ix.live() == int(live.sum())
    return ix, live


@pytest.mark.parametrize("n", [0, 1, 64, 65, "slice+1", N_BIG])
def test_adc_sizes(fv, ctx, cases, n):
    d, m, ksub = GEOMS[0]
    case = cases[GEOMS[0]]
    info = case["pq"].info()
    qt = info["queries_per_workgroup"]
    n = info["min_slice_rows"] + 1 if n == "slice+1" else n
    ix, live = build(fv, ctx, case, n, deleted=lambda n: np.arange(2, n, 7))
    for B, k in [(1, 1), (qt, 10), (qt + 1, 64), (33, 65), (5, 256)]:
        res = ix.search(case["q"][:B], k)
        check(res, ref.search(case["q"][:B], case["books"], case["codes"][:n], live, d, m, k), case["ids"], k)
    ix.close()


@pytest.mark.parametrize("geom", GEOMS[1:])
def test_adc_geometries(fv, ctx, cases, geom):
    d, m, ksub = geom
    case = cases[geom]
    qt = case["pq"].info()["queries_per_workgroup"]
    assert qt in (1, 2, 4) and case["pq"].info()["lds_bytes"] <= case["pq"].info()["lds_limit"]
    ix, live = build(fv, ctx, case, N_BIG, deleted=lambda n: np.arange(0, n, 5))
    for B, k in [(qt + 1, 10), (33, 65), (2, 256)]:
        res = ix.search(case["q"][:B], k)
        want = ref.search(case["q"][:B], case["books"], case["codes"], live, d, m, k)
        check(res, want, case["ids"], k)
        # against the f64 distance to the decoded row: three roundings a term, at most d - 1 additions, the root
        dec = ref.decode(case["codes"], case["books"]).astype(np.float64)
        for b, (rows, dist) in enumerate(want):
            exact = np.sqrt(((case["q"][b].astype(np.float64) - dec[rows]) ** 2).sum(axis=1))
            assert np.all(np.abs(dist - exact) <= (d + 4) * 2.0 ** -24 * exact)
    # an allow-set: only its live rows are candidates
    allowed_rows = np.arange(1, N_BIG, 3)
    res = ix.search(case["q"][:3], 10, allowed=case["ids"][allowed_rows])
    mask = np.zeros(N_BIG, bool)
    mask[allowed_rows] = True
    check(res, ref.search(case["q"][:3], case["books"], case["codes"], live & mask, d, m, 10), case["ids"], 10)
    # every row deleted: empty lists, no error
    ix.mark_deleted(case["ids"][live])
    res = ix.search(case["q"][:3], 10)
    assert ix.live() == 0 and np.all(res.counts == 0) and np.all(res.ids == NO_ID)
    ix.close()


@pytest.mark.parametrize("rows", ["f32", "f16"])
@pytest.mark.parametrize("geom", GEOMS[:2])
def test_refined_search(fv, ctx, cases, geom, rows):
    d, m, ksub = geom
    case = cases[geom]
    k, B = 10, 5
    ix, live = build(fv, ctx, case, N_BIG, refine=rows, deleted=lambda n: np.arange(4, n, 9))
    stored = case["x"] if rows == "f32" else case["x"].astype(np.float16).astype(np.float32)  # rounded once
    for fetch_k in [k, 64, 65, 256]:
        res = ix.search(case["q"][:B], k, fetch_k=fetch_k)
        cand = ref.search(case["q"][:B], case["books"], case["codes"], live, d, m, fetch_k)
        check(res, [ref.refine(case["q"][b], stored, cand[b][0], k) for b in range(B)], case["ids"], k)
    ix.close()


def test_fetch_k_needs_refine_rows(fv, ctx, cases):
    case = cases[GEOMS[0]]
    ix, _ = build(fv, ctx, case, 10)
    with pytest.raises(fv.engine.InvalidConfig):
        ix.search(case["q"][:1], 2, fetch_k=4)
    with pytest.raises(fv.engine.Unsupported):
        ix.search(case["q"][:1], 257)
    ix.close()
