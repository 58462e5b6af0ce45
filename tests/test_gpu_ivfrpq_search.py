"""GPU: the inverted file over RESIDUAL PQ codes (fvdb_ivfrpq_create) against tests/_ivfrpq_ref.py
restricted to the probed lists: ids, f32 distance bits and counts, no tolerance.  Lists of 0, 1, 63, 64, 65 and 200 rows
filled over two adds; the last geometry stages a subspace's codebook in two runs."""
import numpy as np
import pytest

import fvdb_import
import _pq_ref as ref
import _ivfrpq_ref as rref

pytestmark = pytest.mark.gpu

NO_ID = np.iinfo(np.uint64).max
SIZES = [0, 1, 63, 64, 65, 200]
NLIST, N, SPLIT, NQ, GAP = len(SIZES), sum(SIZES), 190, 33, 1e-3
GEOMS = [(8, 8, 2), (10, 3, 16), (40, 20, 256), (384, 48, 256), (64, 2, 256)]


def ranking(cents, v):
    """f64: every row of v's centroids by ascending distance, and those distances"""
    d2 = np.stack([((v.astype(np.float64) - c.astype(np.float64)) ** 2).sum(1) for c in cents], axis=1)
    order = np.argsort(d2, axis=1, kind="stable")
    return order, np.sqrt(np.take_along_axis(d2, order, axis=1))


def make_case(d, m, ksub):
    rng = np.random.default_rng(41)
    u = rng.standard_normal(d)  # given centroids: on one line at 0, 1, 3, 7, 15, 31 (x 2), so no two are equally far from a third
    cents = (2.0 * (2.0 ** np.arange(NLIST) - 1)[:, None] * (u / np.linalg.norm(u))[None, :]).astype(np.float32)
    label = rng.permutation(np.repeat(np.arange(NLIST), SIZES))
    x = (cents[label] + 0.1 * rng.standard_normal((N, d))).astype(np.float32)
    big = np.flatnonzero(label == 5)
    x[big[-1]] = x[big[0]]  # identical rows in different adds: the tie goes to the earlier one
    assert big[0] < SPLIT <= big[-1]
    books = [(0.1 * rng.standard_normal((ksub, dj))).astype(np.float32) for _, dj in ref.geom(d, m)]
    codes = rref.codes(x, cents, label, books, d, m)
    q = (cents[np.arange(NQ) % NLIST] + 0.1 * rng.standard_normal((NQ, d))).astype(np.float32)
    q[1:4] = cents[label[:3]] + ref.decode(codes[:3], books)  # c + r^ in f32: v at or just below zero (the clamp)
    order, dist = ranking(cents, x)
    assert np.array_equal(order[:, 0], label) and np.all(dist[:, 1] - dist[:, 0] >= GAP * dist[:, 1])
    probes, pd = ranking(cents, q)
    assert np.all(pd[:, 1:] - pd[:, :-1] >= GAP * pd[:, 1:])  # one probe order only
    return dict(d=d, m=m, cents=cents, x=x, q=q, label=label, probes=probes, books=books, ids=np.arange(N, dtype=np.uint64) * 3 + 7,
                dist=rref.scores(q, cents, label, books, codes, d, m),
                plain=ref.adc(ref.tables(q, books, d, m), ref.encode(x, books, d, m)))


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
    for g in GEOMS:
        out[g] = make_case(*g)
        out[g]["pq"] = fv.ProductQuantizer(ctx, *g)
        out[g]["pq"].set_codebooks(ref.join_books(out[g]["books"]), g[2])
    return out


def build(fv, ctx, case, refine=None, residual=True):
    ix = fv.IVFPQIndex(ctx, case["pq"], NLIST, refine_rows=refine, residual=residual)
    ix.set_centroids(case["cents"])
    ix.add(case["ids"][:SPLIT], case["x"][:SPLIT])
    ix.add(case["ids"][SPLIT:], case["x"][SPLIT:])
    assert ix.rows() == N and list(ix.list_sizes()) == SIZES
    return ix


@pytest.fixture(scope="module")
def indexes(fv, ctx, cases):
    out = {g: build(fv, ctx, cases[g]) for g in cases}
    yield out
    for ix in out.values():
        ix.close()


def want(case, B, nprobe, live, k, dist="dist"):
    out = []
    for b in range(B):
        rows = np.flatnonzero(live & np.isin(case["label"], case["probes"][b, :nprobe])).astype(np.uint32)
        out.append(ref.select(np.ascontiguousarray(case[dist][b, rows]), rows, k))
    return out


def check(res, wanted, ids):
    for b, (rows, dist) in enumerate(wanted):
        c = rows.size
        assert res.counts[b] == c, (b, res.counts[b], c)
        assert np.array_equal(res.ids[b, :c], ids[rows]), (b, res.ids[b, :c], ids[rows])
        assert np.array_equal(res.distances[b, :c].view(np.uint32), dist.view(np.uint32)), (b, res.distances[b, :c], dist)
        assert np.all(res.ids[b, c:] == NO_ID) and np.all(np.isinf(res.distances[b, c:]))


@pytest.mark.parametrize("nprobe", [1, 3, NLIST])
@pytest.mark.parametrize("geom", GEOMS)
def test_probed_search(cases, indexes, geom, nprobe):
    case, ix, live = cases[geom], indexes[geom], np.ones(N, bool)
    assert ix.residual and ix.bytes() > 0
    for B in [1, 5, 33]:  # queries 1..3 sit on decoded rows
        for k in [1, 10, 65]:
            check(ix.search(case["q"][:B], k, nprobe), want(case, B, nprobe, live, k), case["ids"])


def test_filters(fv, ctx, cases):
    case = cases[GEOMS[1]]
    ix = build(fv, ctx, case)
    live = np.ones(N, bool)
    live[2::7] = False
    live[case["label"] == 4] = False  # a list deleted whole
    ix.mark_deleted(case["ids"][~live])
    for nprobe in [1, 3]:
        check(ix.search(case["q"], 10, nprobe), want(case, NQ, nprobe, live, 10), case["ids"])
    mask = np.zeros(N, bool)
    mask[1::3] = True
    check(ix.search(case["q"][:9], 65, 3, allowed=case["ids"][mask]), want(case, 9, 3, live & mask, 65), case["ids"])
    ix.close()


def test_refined_search(fv, ctx, cases):
    case, k, B, nprobe = cases[GEOMS[1]], 10, 9, 3
    ix = build(fv, ctx, case, refine="f32")
    for fetch_k in [k, 64]:
        cand = want(case, B, nprobe, np.ones(N, bool), fetch_k)
        check(ix.search(case["q"][:B], k, nprobe, fetch_k=fetch_k),
              [ref.refine(case["q"][b], case["x"], cand[b][0], k) for b in range(B)], case["ids"])
    ix.close()


@pytest.mark.parametrize("geom", [GEOMS[1], GEOMS[3]])
def test_plain_and_residual_side_by_side(fv, ctx, cases, indexes, geom):
    case, live = cases[geom], np.ones(N, bool)
    plain = build(fv, ctx, case, residual=False)
    assert not plain.residual and plain.bytes() < indexes[geom].bytes()
    for ix, dist in [(plain, "plain"), (indexes[geom], "dist"), (plain, "plain")]:
        check(ix.search(case["q"], 10, 3), want(case, NQ, 3, live, 10, dist), case["ids"])
    plain.close()


def test_refusals(fv, ctx, cases):
    case, E = cases[GEOMS[1]], fv.engine
    pq = fv.ProductQuantizer(ctx, 10, 3, 16)
    with pytest.raises(E.NotTrained):
        fv.IVFPQIndex(ctx, pq, NLIST, residual=True)  # quantizer untrained
    pq.set_codebooks(ref.join_books(case["books"]), 16)
    ix = fv.IVFPQIndex(ctx, pq, NLIST, residual=True)
    with pytest.raises(E.NotTrained):
        ix.add(case["ids"][:4], case["x"][:4])  # centroids unset
    with pytest.raises(E.NotTrained):
        ix.search(case["q"][:1], 1, 1)
    ix.set_centroids(case["cents"])
    ix.add(case["ids"][:40], case["x"][:40])
    pq.set_codebooks(ref.join_books(case["books"]), 16)  # changed codebooks invalidate the index
    with pytest.raises(E.InvalidConfig):
        ix.search(case["q"][:1], 1, 1)
    with pytest.raises(E.InvalidConfig):
        ix.add(case["ids"][40:44], case["x"][40:44])
    ix.close()
    pq.close()


def test_ivf_residuals(fv, ctx, cases):
    case = cases[GEOMS[1]]
    res, lists = fv.ivf_residuals(ctx, case["cents"], case["x"])
    assert np.array_equal(lists, case["label"]) and np.array_equal(res.view(np.uint32), (case["x"] - case["cents"][case["label"]]).view(np.uint32))
