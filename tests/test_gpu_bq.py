"""GPU: binary quantization (fvdb_bq_*) against tests/_bq_ref.py: the codec's bytes, and ids,
distance bits and counts of the Hamming search and the refined search, under ties, deletions and an allow-set, at every
size where the scan takes another path (a partial block, one slice and a row, several slices, each chunk count)."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import _bq_ref as ref

pytestmark = pytest.mark.gpu

NO_ID = np.iinfo(np.uint64).max
N_BIG = 3000  # several slices
DIMS = [1, 8, 32, 33, 128, 129, 384, 2048]
E_INVALID, E_NONFINITE, E_UNSUPPORTED = 6, 9, 12


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
    """per d: N_BIG rows with duplicates, 70 queries, a centre (zeros at d = 8), and the reference's [70][N_BIG] distances"""
    out = {}
    for d in DIMS:
        rng = np.random.default_rng(d)
        x = rng.standard_normal((N_BIG, d)).astype(np.float32)
        x[5::10] = x[3]  # duplicated rows: equal keys but for the row
        q = rng.standard_normal((70, d)).astype(np.float32)
        q[1] = x[3]
        c = None if d == 8 else (0.25 * rng.standard_normal(d)).astype(np.float32)
        out[d] = dict(x=x, q=q, c=c, ham=ref.hamming(q, x, c), ids=np.arange(N_BIG, dtype=np.uint64) * 3 + 7)
    return out


def check(res, want, ids):
    for b, (rows, dist) in enumerate(want):
        c = rows.size
        assert res.counts[b] == c, (b, res.counts[b], c)
        assert np.array_equal(res.ids[b, :c], ids[rows]), (b, res.ids[b, :c], ids[rows])
        assert np.array_equal(res.distances[b, :c].view(np.uint32), dist.view(np.uint32)), b
        assert np.all(res.ids[b, c:] == NO_ID) and np.all(np.isinf(res.distances[b, c:]))


def build(fv, ctx, case, d, n, refine=None, deleted=None):
    ix = fv.BQIndex(ctx, d, refine_rows=refine, center=case["c"])
    for a in range(0, n, 1100):  # several adds: blocks are completed across calls
        ix.add(case["ids"][a:min(n, a + 1100)], case["x"][a:min(n, a + 1100)])
    live = np.ones(n, bool)
    if deleted is not None and n:
        live[deleted] = False
        ix.mark_deleted(case["ids"][:n][~live])
    assert ix.rows() == n and ix.live() == int(live.sum())
    return ix, live


def raw_encode(fv, ctx, x, center):
    """fvdb_bq_encode into a buffer of 0xAA bytes: (status, the buffer)"""
    n, d = x.shape
    out = np.full((n, (d + 7) // 8), 0xAA, np.uint8)
    f32p = C.POINTER(C.c_float)
    rc = ctx.lib.fvdb_bq_encode(ctx.h, x.ctypes.data_as(f32p), n, d, None if center is None else center.ctypes.data_as(f32p),
                                out.ctypes.data_as(fv._capi.u8p))
    return rc, out


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("d", [1, 31, 32, 33, 127, 128, 129, 384, 2048])
def test_codec(fv, ctx, d, n):
    rng = np.random.default_rng(1000 * d + n)
    x = rng.standard_normal((n, d)).astype(np.float32)
    c = rng.standard_normal(d).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1e38, -1e38], np.float32)
    x.flat[:: 3] = special[np.arange(x.flat[:: 3].size) % 6]
    for center in (None, c):
        y = x.copy()
        if center is not None:
            y[:, ::2] = center[::2]  # values equal to the centre: bit 0
        got = fv.binary_quantize(ctx, y, center)
        assert got.shape == (n, (d + 7) // 8) and np.array_equal(got, ref.encode(y, center))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_codec_refuses_non_finite(fv, ctx, bad):
    x = np.ones((3, 33), np.float32)
    c = np.zeros(33, np.float32)
    for xs, cs in [(x.copy(), None), (x.copy(), c.copy())]:
        (xs if cs is None else cs).flat[7] = bad
        rc, out = raw_encode(fv, ctx, xs, cs)
        assert rc == E_NONFINITE and np.all(out == 0xAA)
    with pytest.raises(fv.engine.NonFiniteInput):
        fv.BQIndex(ctx, 33, center=np.full(33, bad, np.float32))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, "slice+1", N_BIG])
def test_hamming_sizes(fv, ctx, cases, n):
    d, case = 33, cases[33]
    probe = fv.BQIndex(ctx, d)
    tile = probe.info()["queries_per_workgroup"]
    n = probe.info()["min_slice_rows"] + 1 if n == "slice+1" else n
    probe.close()
    ix, live = build(fv, ctx, case, d, n, deleted=np.arange(2, n, 7))
    for B, k in [(1, 1), (tile, 10), (tile + 1, 64), (70, 65), (3, 256)]:  # k above the live rows at the small n
        check(ix.search(case["q"][:B], k), ref.search(case["ham"][:B, :n], live, k), case["ids"])
    info = ix.info()
    assert info["last_pairs"] == 3 * n and (info["last_slices"] > 1) == (n > info["min_slice_rows"])
    ix.close()


@pytest.mark.parametrize("d", [1, 32, 128, 129, 384, 2048])
def test_hamming_dims(fv, ctx, cases, d):
    case = cases[d]
    ix, live = build(fv, ctx, case, d, N_BIG, deleted=np.arange(0, N_BIG, 5))
    info = ix.info()
    assert info["words"] == (d + 31) // 32 and 4 * info["chunks"] >= info["words"]
    assert all(b <= info["lds_limit"] for b in info["lds_bytes"])
    for B, k in [(33, 10), (70, 65), (2, 256)]:
        check(ix.search(case["q"][:B], k), ref.search(case["ham"][:B], live, k), case["ids"])
    # an allow-set meeting the deletions: only its live rows are candidates
    mask = np.zeros(N_BIG, bool)
    mask[1::3] = True
    check(ix.search(case["q"][:3], 10, allowed=case["ids"][mask]), ref.search(case["ham"][:3], live & mask, 10), case["ids"])
    # restored rows are candidates again
    ix.mark_deleted(case["ids"][::10], deleted=False)
    live[::10] = True
    check(ix.search(case["q"][:3], 10), ref.search(case["ham"][:3], live, 10), case["ids"])
    # every row deleted: empty lists, no error
    ix.mark_deleted(case["ids"][live])
    res = ix.search(case["q"][:3], 10)
    assert ix.live() == 0 and np.all(res.counts == 0) and np.all(res.ids == NO_ID)
    ix.close()


@pytest.mark.parametrize("k", [1, 10, 64, 65, 256])
def test_ties(fv, ctx, cases, k):
    # d = 8: at most nine distinct distances, hundreds of rows tie at the k-th; within a distance the order is the row order
    case = cases[8]
    assert np.unique(case["ham"]).size <= 9
    ix, live = build(fv, ctx, case, 8, N_BIG, deleted=np.arange(1, N_BIG, 11))
    check(ix.search(case["q"], k), ref.search(case["ham"], live, k), case["ids"])
    mask = np.zeros(N_BIG, bool)
    mask[::2] = True
    check(ix.search(case["q"][:5], k, allowed=case["ids"][mask]), ref.search(case["ham"][:5], live & mask, k), case["ids"])
    ix.close()


@pytest.mark.parametrize("refine", ["f32", "f16"])
@pytest.mark.parametrize("d", [33, 384])
def test_refined_search(fv, ctx, cases, d, refine):
    case = cases[d]
    k, B = 10, 5
    ix, live = build(fv, ctx, case, d, N_BIG, refine=refine, deleted=np.arange(4, N_BIG, 9))
    source = case["x"] if refine == "f32" else case["x"].astype(np.float16).astype(np.float32)  # fp16 rows are rounded once
    for fetch_k in [k, 64, 65, 256]:
        res = ix.search(case["q"][:B], k, fetch_k=fetch_k)
        cand = ref.search(case["ham"][:B], live, fetch_k)
        want = [ref.top(ref.fold(case["q"][b], source[cand[b][0]]), cand[b][0], k) for b in range(B)]
        check(res, want, case["ids"])
    ix.close()


def test_refusals(fv, ctx, cases):
    case = cases[33]
    plain, _ = build(fv, ctx, case, 33, 10)
    kept, _ = build(fv, ctx, case, 33, 10, refine="f32")
    f32p, u64p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)

    def raw(ix, q, k, fetch_k):
        width = min(max(k, 1), 256)
        ids, dist, cnt = np.full((1, width), 5, np.uint64), np.full((1, width), 5, np.float32), np.full(1, 5, np.uint32)
        rc = ctx.lib.fvdb_bq_index_search(ix.h, q.ctypes.data_as(f32p), 1, k, fetch_k, None, 0, ids.ctypes.data_as(u64p),
                                          dist.ctypes.data_as(f32p), cnt.ctypes.data_as(u32p))
        assert np.all(ids == 5) and np.all(dist == 5) and cnt[0] == 5  # outputs unwritten
        return rc

    q = case["q"][:1].copy()
    assert raw(plain, q, 2, 4) == E_INVALID       # fetch_k without refine rows
    assert raw(kept, q, 5, 4) == E_INVALID        # fetch_k < k
    for k, fk in [(0, 0), (257, 0), (2, 257), (0, 4)]:
        assert raw(kept, q, k, fk) == E_UNSUPPORTED
    assert raw(kept, np.full((1, 33), np.inf, np.float32), 1, 0) == E_NONFINITE
    with pytest.raises(fv.engine.Unsupported):
        kept.search(q, 2, fetch_k=0)
    with pytest.raises(fv.engine.NonFiniteInput):
        kept.add([99], np.full((1, 33), np.nan, np.float32))
    with pytest.raises(fv.engine.Unsupported):
        fv.BQIndex(ctx, 2049)
    assert kept.rows() == 10
    plain.close()
    kept.close()
