"""GPU: the inverted file over SQ8 codes (fvdb_ivfsq8_*) against tests/_sq8_ref.py restricted to
the probed lists: ids, f32 distance bits and counts of the symmetric and the refined search, under deletions and an
allow-set, with lists of 0, 1, 31, 32, 33 and 1150 rows (three segments), 1 to 3 query groups a list, the query operands
in LDS or not; and bit equality with SQ8Index when every list is probed."""
import numpy as np
import pytest

import fvdb_import
import _sq8_ref as ref

pytestmark = pytest.mark.gpu

NO_ID = np.iinfo(np.uint64).max
NLIST = 8
SIZES = [0, 1, 31, 32, 33, 1150, 876, 877]  # rows of list 0 .. 7: 3000 in all
SEED = 0  # a draw whose nearest-centroid choices are unambiguous at every d used here (asserted below)
GAP = 1e-3


def ranking(cents, v):
    """f64: every row of v's centroids by ascending distance (ties to the lower id), and those distances"""
    d2 = np.stack([((v.astype(np.float64) - c.astype(np.float64)) ** 2).sum(1) for c in cents], axis=1)
    order = np.argsort(d2, axis=1, kind="stable")
    return order, np.sqrt(np.take_along_axis(d2, order, axis=1))


def make_case(d, nq):
    rng = np.random.default_rng(SEED)
    cents = (rng.standard_normal((NLIST, d)) * (0.5 + 0.25 * np.arange(NLIST))[:, None]).astype(np.float32)
    label = rng.permutation(np.repeat(np.arange(NLIST), SIZES))
    x = (cents[label] + 0.3 * rng.standard_normal((label.size, d))).astype(np.float32)
    big = np.flatnonzero(label == 5)
    x[big[1::9]] = x[big[0]]  # duplicated rows: equal keys but for the ordinal
    q = (cents[np.arange(nq) % NLIST] + 0.5 * rng.standard_normal((nq, d))).astype(np.float32)
    q[1] = x[3]
    order, dist = ranking(cents, x)
    assert np.array_equal(order[:, 0], label) and np.all(dist[:, 1] - dist[:, 0] >= GAP * dist[:, 1])
    probes, pd = ranking(cents, q)
    assert np.all(pd[:, 1:] - pd[:, :-1] >= GAP * pd[:, 1:])  # the reference's probe order is the only one
    return dict(d=d, cents=cents, x=x, q=q, label=label, probes=probes, dist=ref.sym_dist(q, x),
                ids=np.arange(label.size, dtype=np.uint64) * 3 + 7)


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    c = fv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    return {33: make_case(33, 70), 384: make_case(384, 70), 2048: make_case(2048, 33)}


def build(fv, ctx, case, refine=None):
    ix = fv.IVFSQ8Index(ctx, case["d"], NLIST, refine_rows=refine)
    ix.set_centroids(case["cents"])
    n = case["x"].shape[0]
    for a in range(0, n, 1100):  # several adds: blocks are completed across calls
        ix.add(case["ids"][a:a + 1100], case["x"][a:a + 1100])
    assert ix.rows() == n and ix.live() == n and list(ix.list_sizes()) == SIZES
    return ix


@pytest.fixture(scope="module")
def indexes(fv, ctx, cases):
    out = {d: build(fv, ctx, cases[d]) for d in cases}
    yield out
    for ix in out.values():
        ix.close()


def candidates(case, b, nprobe, live):
    """the live rows of query b's probed lists, as add-order indices"""
    return np.flatnonzero(live & np.isin(case["label"], case["probes"][b, :nprobe]))


def want_sym(case, B, nprobe, live, k):
    out = []
    for b in range(B):
        rows = candidates(case, b, nprobe, live)
        out.append(ref.top(np.ascontiguousarray(case["dist"][b, rows]), rows, k))
    return out


def check(res, want, ids):
    for b, (rows, dist) in enumerate(want):
        c = rows.size
        assert res.counts[b] == c, (b, res.counts[b], c)
        assert np.array_equal(res.ids[b, :c], ids[rows]), (b, res.ids[b, :c], ids[rows])
        assert np.array_equal(res.distances[b, :c].view(np.uint32), dist.view(np.uint32)), b
        assert np.all(res.ids[b, c:] == NO_ID) and np.all(np.isinf(res.distances[b, c:]))


@pytest.mark.parametrize("nprobe", [1, 3, 8])
@pytest.mark.parametrize("d", [33, 384])
def test_probed_search(cases, indexes, d, nprobe):
    case, ix = cases[d], indexes[d]
    live = np.ones(case["label"].size, bool)
    info = ix.info()
    assert info["segb"] == 16 and info["segments"] == 3 and info["max_list_blocks"] == 36
    for B in [1, 33, 70]:  # at nprobe 8, 70 queries are three groups on every list
        for k in [1, 10, 64, 65, 256]:  # above the candidates where a query probes the short lists
            check(ix.search(case["q"][:B], k, nprobe), want_sym(case, B, nprobe, live, k), case["ids"])
    assert ix.info()["items"] <= ix.info()["item_bound"]


def test_operands_from_hbm(cases, indexes):
    # d = 2048, k = 256: 64 KiB of operands do not fit beside 96 KiB of buffers, a lane reads its query's words itself
    case, ix = cases[2048], indexes[2048]
    info = ix.info()
    assert all(b <= info["lds_limit"] for b in info["lds_bytes"]) and info["queries_in_lds"] == [1, 1, 0]
    live = np.ones(case["label"].size, bool)
    check(ix.search(case["q"], 256, 3), want_sym(case, 33, 3, live, 256), case["ids"])


@pytest.mark.parametrize("d", [33, 384])
def test_every_list_probed_equals_flat_index(fv, ctx, cases, indexes, d):
    case = cases[d]
    flat = fv.SQ8Index(ctx, d)
    flat.add(case["ids"], case["x"])
    for k in [10, 256]:
        a, b = indexes[d].search(case["q"], k, NLIST), flat.search(case["q"], k)
        assert np.array_equal(a.ids, b.ids) and np.array_equal(a.counts, b.counts)
        assert np.array_equal(a.distances.view(np.uint32), b.distances.view(np.uint32))
        # the flat index itself still answers by the definition
        check(b, [ref.top(case["dist"][q], np.arange(case["label"].size), k) for q in range(70)], case["ids"])
    flat.close()


def test_filters(fv, ctx, cases):
    case = cases[33]
    n = case["label"].size
    ix = build(fv, ctx, case)
    live = np.ones(n, bool)
    live[2::7] = False
    live[case["label"] == 4] = False  # every row of a list that its own queries probe first
    ix.mark_deleted(case["ids"][~live])
    assert ix.live() == int(live.sum())
    for nprobe in [1, 3]:
        check(ix.search(case["q"], 10, nprobe), want_sym(case, 70, nprobe, live, 10), case["ids"])
    mask = np.zeros(n, bool)
    mask[1::3] = True
    check(ix.search(case["q"][:9], 65, 3, allowed=case["ids"][mask]), want_sym(case, 9, 3, live & mask, 65), case["ids"])
    ix.mark_deleted(case["ids"][~live], deleted=False)
    check(ix.search(case["q"][:9], 10, 3), want_sym(case, 9, 3, np.ones(n, bool), 10), case["ids"])
    ix.close()


@pytest.mark.parametrize("fetch_k", [10, 64])
@pytest.mark.parametrize("refine", ["decoded", "f32"])
def test_refined_search(fv, ctx, cases, refine, fetch_k):
    case, k, B, nprobe = cases[384], 10, 9, 3
    ix = build(fv, ctx, case, refine=None if refine == "decoded" else refine)
    source = ref.decode(*ref.encode(case["x"])) if refine == "decoded" else case["x"]
    res = ix.search(case["q"][:B], k, nprobe, fetch_k=fetch_k, refine=refine)
    cand = want_sym(case, B, nprobe, np.ones(case["label"].size, bool), fetch_k)
    check(res, [ref.refine(case["q"][b], source, cand[b][0], k) for b in range(B)], case["ids"])
    ix.close()


def test_refusals(fv, ctx, cases):
    case = cases[33]
    ix = fv.IVFSQ8Index(ctx, 33, NLIST)
    with pytest.raises(fv.engine.NotTrained):
        ix.add(case["ids"][:4], case["x"][:4])
    with pytest.raises(fv.engine.NotTrained):
        ix.search(case["q"][:1], 1, 1)
    ix.set_centroids(case["cents"])
    ix.add(case["ids"][:40], case["x"][:40])
    bad = case["x"][40:42].copy()
    bad[1, 5] = np.nan
    with pytest.raises(fv.engine.NonFiniteInput):
        ix.add(case["ids"][40:42], bad)
    with pytest.raises(fv.engine.InvalidConfig):
        ix.search(case["q"][:1], 1, 0)
    with pytest.raises(fv.engine.Unsupported):
        ix.search(case["q"][:1], 257, 1)
    with pytest.raises(fv.engine.Unsupported):
        fv.IVFSQ8Index(ctx, 2049, NLIST)
    assert ix.rows() == 40 and ix.live() == 40 and int(ix.list_sizes().sum()) == 40  # nothing was written
    live = np.zeros(case["label"].size, bool)
    live[:40] = True
    check(ix.search(case["q"][:5], 10, NLIST), want_sym(case, 5, NLIST, live, 10), case["ids"])
    ix.close()
