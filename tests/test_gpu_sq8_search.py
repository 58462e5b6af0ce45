"""GPU: search over u8 scalar codes (fvdb_sq8_index_*) against tests/_sq8_ref.py: ids, f32 distance
bits and counts of the symmetric search and of the refined search, under deletions and an allow-set, at every size where
the scan takes another path (a partial block, one slice and a row, several slices, queries in LDS or not)."""
import numpy as np
import pytest

import fvdb_import
import _sq8_ref as ref

pytestmark = pytest.mark.gpu

NO_ID = np.iinfo(np.uint64).max
N_BIG = 3000  # several slices
DIMS = [1, 32, 33, 384, 2048]


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
    """per d: N_BIG rows with duplicates, 70 queries, and the reference's [70][N_BIG] symmetric distances"""
    out = {}
    for d in DIMS:
        rng = np.random.default_rng(d)
        x = rng.standard_normal((N_BIG, d)).astype(np.float32)
        x[5::10] = x[3]  # duplicated rows: equal keys but for the row
        q = rng.standard_normal((70, d)).astype(np.float32)
        q[1] = x[3]
        out[d] = dict(x=x, q=q, dist=ref.sym_dist(q, x), ids=np.arange(N_BIG, dtype=np.uint64) * 3 + 7)
    return out


def want_sym(case, B, n, live, k):
    rows = np.flatnonzero(live[:n])
    return [ref.top(np.ascontiguousarray(case["dist"][b, rows]), rows, k) for b in range(B)]


def check(res, want, ids):
    for b, (rows, dist) in enumerate(want):
        c = rows.size
        assert res.counts[b] == c, (b, res.counts[b], c)
        assert np.array_equal(res.ids[b, :c], ids[rows]), (b, res.ids[b, :c], ids[rows])
        assert np.array_equal(res.distances[b, :c].view(np.uint32), dist.view(np.uint32)), b
        assert np.all(res.ids[b, c:] == NO_ID) and np.all(np.isinf(res.distances[b, c:]))


def build(fv, ctx, case, d, n, refine=None, deleted=None):
    ix = fv.SQ8Index(ctx, d, refine_rows=refine)
    for a in range(0, n, 1100):  # several adds: blocks are completed across calls
        ix.add(case["ids"][a:min(n, a + 1100)], case["x"][a:min(n, a + 1100)])
    live = np.ones(n, bool)
    if deleted is not None and n:
        live[deleted] = False
        ix.mark_deleted(case["ids"][:n][~live])
    assert ix.rows() == n and ix.live() == int(live.sum())
    return ix, live


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, "slice+1", N_BIG])
def test_symmetric_sizes(fv, ctx, cases, n):
    d, case = 33, cases[33]
    probe = fv.SQ8Index(ctx, d)
    n = probe.info()["min_slice_rows"] + 1 if n == "slice+1" else n
    probe.close()
    ix, live = build(fv, ctx, case, d, n, deleted=np.arange(2, n, 7))
    for B, k in [(1, 1), (31, 10), (32, 64), (33, 65), (70, 256)]:  # k above the live rows at the small n
        check(ix.search(case["q"][:B], k), want_sym(case, B, n, live, k), case["ids"])
    ix.close()


@pytest.mark.parametrize("d", [1, 32, 384, 2048])
def test_symmetric_dims(fv, ctx, cases, d):
    case = cases[d]
    ix, live = build(fv, ctx, case, d, N_BIG, deleted=np.arange(0, N_BIG, 5))
    info = ix.info()
    assert all(b <= info["lds_limit"] for b in info["lds_bytes"]) and info["queries_in_lds"][0] == 1
    assert info["queries_in_lds"][2] == (0 if d == 2048 else 1)  # 64 KiB of operands beside 96 KiB of buffers do not fit
    for B, k in [(33, 10), (70, 65), (2, 256)]:
        check(ix.search(case["q"][:B], k), want_sym(case, B, N_BIG, live, k), case["ids"])
    # an allow-set: only its live rows are candidates
    mask = np.zeros(N_BIG, bool)
    mask[1::3] = True
    check(ix.search(case["q"][:3], 10, allowed=case["ids"][mask]), want_sym(case, 3, N_BIG, live & mask, 10), case["ids"])
    # every row deleted: empty lists, no error
    ix.mark_deleted(case["ids"][live])
    res = ix.search(case["q"][:3], 10)
    assert ix.live() == 0 and np.all(res.counts == 0) and np.all(res.ids == NO_ID)
    ix.close()


@pytest.mark.parametrize("rows_code,query_code", [(255, 255), (255, 0), (0, 255)])
def test_code_extremes_at_2048(fv, ctx, rows_code, query_code):
    # every code 255 or 0 but one dim that sets the range: the accumulator and the signed bias at their ends
    d, n = 2048, 40
    def rows(code, count):
        x = np.full((count, d), 1.0 if code else 0.0, np.float32)
        x[:, 0] = 0.0 if code else 1.0
        x *= (1 + np.arange(count, dtype=np.float32))[:, None]
        return x
    x, q = rows(rows_code, n), rows(query_code, 3)
    ix = fv.SQ8Index(ctx, d)
    ids = np.arange(n, dtype=np.uint64)
    ix.add(ids, x)
    check(ix.search(q, 40), ref.search(q, x, np.ones(n, bool), 40), ids)
    ix.close()


@pytest.mark.parametrize("refine", ["decoded", "f32", "f16"])
@pytest.mark.parametrize("d", [33, 384])
def test_refined_search(fv, ctx, cases, d, refine):
    case = cases[d]
    k, B = 10, 5
    ix, live = build(fv, ctx, case, d, N_BIG, refine=None if refine == "decoded" else refine, deleted=np.arange(4, N_BIG, 9))
    source = {"decoded": lambda: ref.decode(*ref.encode(case["x"])), "f32": lambda: case["x"],
              "f16": lambda: case["x"].astype(np.float16).astype(np.float32)}[refine]()  # fp16 rows are rounded once
    for fetch_k in [k, 64, 65, 256]:
        res = ix.search(case["q"][:B], k, fetch_k=fetch_k, refine=refine)
        cand = want_sym(case, B, N_BIG, live, fetch_k)
        check(res, [ref.refine(case["q"][b], source, cand[b][0], k) for b in range(B)], case["ids"])
    ix.close()


def test_refusals(fv, ctx, cases):
    case = cases[33]
    ix, _ = build(fv, ctx, case, 33, 10)
    with pytest.raises(fv.engine.InvalidConfig):
        ix.search(case["q"][:1], 2, fetch_k=4, refine="f32")  # no refine rows
    with pytest.raises(fv.engine.InvalidConfig):
        ix.search(case["q"][:1], 5, fetch_k=4)
    for k, fk in [(257, None), (0, None), (2, 257)]:
        with pytest.raises(fv.engine.Unsupported):
            ix.search(case["q"][:1], k, fetch_k=fk)
    with pytest.raises(fv.engine.NonFiniteInput):
        ix.search(np.full((1, 33), np.inf, np.float32), 1)
    with pytest.raises(fv.engine.Unsupported):
        fv.SQ8Index(ctx, 2049)
    ix.close()
