"""GPU: cosine k-NN search (fvdb_cos_index_*) against tests/_cos_ref.py: ids, f32 similarity bits
and counts, in mode "filter" (fp16 matrix-core filter, exact re-score) and mode "exact", under deletions and an
allow-set, at every size where the scan takes another path."""
import numpy as np
import pytest

import fvdb_import
import _cos_ref as ref

pytestmark = pytest.mark.gpu

NO_ID = np.iinfo(np.uint64).max
N_BIG = 3000  # several slices
MODES = ["filter", "exact"]


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    c = fv.Context(0)
    yield c
    c.close()


def make_case(d, kind="scaled"):
    rng = np.random.default_rng(1000 + d)
    x = rng.standard_normal((N_BIG, d)).astype(np.float32)
    q = rng.standard_normal((70, d)).astype(np.float32)
    if kind == "scaled":
        x *= np.exp2(rng.integers(-30, 31, N_BIG)).astype(np.float32)[:, None]
        x[5::10] = x[3]  # duplicated rows: equal similarities, the earlier row first
        x[11] = 0  # a zero row and a zero query: similarity 0.0
        q[1], q[2] = x[3], 0
    elif kind == "near":
        x = (x[:1] + np.float32(1e-3) * x).astype(np.float32)  # every cosine within the filter's margin of every other
    return dict(x=x, q=q, sim=ref.sims(q, x), ids=np.arange(N_BIG, dtype=np.uint64) * 3 + 7)


@pytest.fixture(scope="module")
def cases():
    memo = {}
    return lambda d, kind="scaled": memo.setdefault((d, kind), make_case(d, kind))


def build(fv, ctx, case, d, n, deleted=None):
    ix = fv.CosineIndex(ctx, d)
    for a in range(0, n, 1100):  # several adds: blocks are completed across calls
        ix.add(case["ids"][a:min(n, a + 1100)], case["x"][a:min(n, a + 1100)])
    live = np.ones(n, bool)
    if deleted is not None and n:
        live[deleted] = False
        ix.mark_deleted(case["ids"][:n][~live])
    assert ix.rows() == n and ix.live() == int(live.sum())
    return ix, live


def check(ix, case, B, k, live, allowed=None):
    """both modes against the reference: ids, similarity bits, counts, padding"""
    rows = np.flatnonzero(live)
    for mode in MODES:
        res = ix.search(case["q"][:B], k, allowed=allowed, mode=mode)
        for b in range(B):
            wr, ws = ref.top(case["sim"][b], rows, k)
            c = wr.size
            assert res.counts[b] == c, (mode, b, res.counts[b], c)
            assert np.array_equal(res.ids[b, :c], case["ids"][wr]), (mode, b)
            assert np.array_equal(res.similarities[b, :c].view(np.uint32), ws.view(np.uint32)), (mode, b)
            assert np.all(res.ids[b, c:] == NO_ID) and np.all(np.isneginf(res.similarities[b, c:]))


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, "slice+1", N_BIG])
def test_sizes(fv, ctx, cases, n):
    d, case = 33, cases(33)
    probe = fv.CosineIndex(ctx, d)
    n = probe.info()["min_slice_rows"] + 1 if n == "slice+1" else n
    probe.close()
    ix, live = build(fv, ctx, case, d, n, deleted=np.arange(6, n, 7))
    for B, k in [(1, 1), (31, 10), (33, 65), (70, 256)]:  # k above the live rows at the small n
        check(ix, case, B, k, live)
    ix.close()


@pytest.mark.parametrize("d", [1, 16, 17, 384, 2048])
def test_dims(fv, ctx, cases, d):
    case = cases(d)  # at d = 1 every value is +-1 or 0: half the rows tie at the cut and arenas overflow
    ix, live = build(fv, ctx, case, d, N_BIG)
    info = ix.info()
    assert all(b <= info["lds_limit"] for b in info["lds_bytes"]) and info["E"] == 2.0 ** -9
    for B, k in [(33, 10), (70, 65), (3, 256)]:
        check(ix, case, B, k, live)
    mask = np.zeros(N_BIG, bool)
    mask[1::3] = True
    check(ix, case, 3, 10, live & mask, allowed=case["ids"][mask])
    ix.mark_deleted(case["ids"])  # every row deleted: empty results, no error
    check(ix, case, 3, 10, np.zeros(N_BIG, bool))
    assert ix.live() == 0
    ix.close()


def test_near_ties(fv, ctx, cases):
    case = cases(384, "near")
    ix, live = build(fv, ctx, case, 384, N_BIG, deleted=np.arange(6, N_BIG, 7))
    check(ix, case, 33, 10, live)
    ix.search(case["q"][:33], 10)
    assert ix.info()["fallback_queries"] == 33  # all rows survive: every arena overflows, the answer is still exact
    ix.close()


def test_the_filter_filters(fv, ctx, cases):
    case = cases(384, "normal")
    ix, live = build(fv, ctx, case, 384, N_BIG)
    B, k = 70, 10
    check(ix, case, B, k, live)
    ix.search(case["q"][:B], k)
    info = ix.info()
    print("exact_pairs", info["exact_pairs"], "of", B * N_BIG, "fallback_queries", info["fallback_queries"])
    assert info["fallback_queries"] == 0 and info["exact_pairs"] < 0.5 * B * N_BIG
    ix.close()


def test_refusals(fv, ctx, cases):
    case = cases(33)
    ix, _ = build(fv, ctx, case, 33, 10)
    for k in [0, 257]:
        with pytest.raises(fv.engine.Unsupported):
            ix.search(case["q"][:1], k)
    with pytest.raises(fv.engine.Unsupported):
        fv.CosineIndex(ctx, 2049)
    bad = case["x"][:1].copy()
    bad[0, 5] = np.inf
    with pytest.raises(fv.engine.NonFiniteInput):
        ix.add([999], bad)
    with pytest.raises(fv.engine.NonFiniteInput):
        ix.search(bad, 1)
    big = np.zeros((1, 33), np.float32)
    big[0, 0] = 2.0 ** 60
    with pytest.raises(fv.engine.Unsupported):
        ix.add([999], big)
    with pytest.raises(fv.engine.Unsupported):
        ix.search(big, 1)
    assert ix.rows() == 10
    ix.close()
