"""GPU: the product quantizer's codec (fvdb_pq_*) against the restatement of tests/_pq_ref.py:
encode and decode bit for bit, a Lloyd step bit for bit once the random picks are given, and the refusals."""
import numpy as np
import pytest

import fvdb_import
import _pq_ref as ref

pytestmark = pytest.mark.gpu

GEOMS = [(8, 8), (10, 3), (130, 4), (384, 48)]  # one dim a subspace; uneven last; 32/32/32/34, past one staged chunk; the flagship
SIZES = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    c = fv.Context(0)
    yield c
    c.close()


def make_books(rng, d, m, ksub, lattice):
    books = []
    for _, dj in ref.geom(d, m):
        b = rng.integers(-2, 3, (ksub, dj)).astype(np.float32) if lattice else rng.standard_normal((ksub, dj)).astype(np.float32)
        if ksub >= 2:
            b[ksub - 1] = b[ksub // 3]  # two identical centroids: the lower index must win
        books.append(b)
    return books


@pytest.mark.parametrize("ksub", [1, 2, 256])
@pytest.mark.parametrize("d,m", GEOMS)
@pytest.mark.parametrize("lattice", [False, True])
def test_encode_decode_bits(fv, ctx, d, m, ksub, lattice):
    rng = np.random.default_rng(d * 1000 + m * 10 + ksub + lattice)
    books = make_books(rng, d, m, ksub, lattice)
    x = rng.integers(-2, 3, (130, d)).astype(np.float32) if lattice else rng.standard_normal((130, d)).astype(np.float32)
    x[7, :ref.geom(d, m)[0][1]] = books[0][ksub // 3]  # a row that sits on the duplicated centroid
    want = ref.encode(x, books, d, m)
    assert ksub < 2 or want[7, 0] <= ksub // 3
    pq = fv.ProductQuantizer(ctx, d, m, ksub)
    pq.set_codebooks(ref.join_books(books), ksub)
    assert np.array_equal(pq.codebooks().view(np.uint32), ref.join_books(books).view(np.uint32))
    for n in SIZES:
        codes = pq.encode(x[:n])
        assert np.array_equal(codes, want[:n]), f"n={n}: {np.argwhere(codes != want[:n])[:4]}"
        assert np.array_equal(pq.decode(codes).view(np.uint32), ref.decode(want[:n], books).view(np.uint32))
    pq.close()


@pytest.mark.parametrize("iterations", [0, 1, 3])
def test_train_bits(fv, ctx, iterations):
    n, d, m, ksub, seed = 300, 10, 3, 4, 11
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, d)).astype(np.float32)
    init = np.array([[0, 17, 17, 40], [3, 3, 9, 250], [299, 1, 2, 299]], np.uint32)  # a row twice: the copy stays empty and is refilled
    pq = fv.ProductQuantizer(ctx, d, m, ksub)
    pq.train(x, iterations, init_rows=init, seed=seed)
    want = ref.join_books(ref.train(x, d, m, ksub, iterations, init, seed))
    assert np.array_equal(pq.codebooks().view(np.uint32), want.view(np.uint32))
    pq.train(x, 1, seed=seed)  # drawn initial rows: distinct within a subspace, the stated stream
    assert np.array_equal(pq.codebooks().view(np.uint32), ref.join_books(ref.train(x, d, m, ksub, 1, None, seed)).view(np.uint32))
    pq.close()


def test_fewer_training_rows_than_centroids(fv, ctx):
    x = np.random.default_rng(1).standard_normal((5, 10)).astype(np.float32)
    pq = fv.ProductQuantizer(ctx, 10, 3, 16)
    pq.train(x, 2, seed=3)
    assert pq.info()["ksub_actual"] == 5 and pq.codebooks().size == 5 * 10
    assert np.array_equal(pq.codebooks().view(np.uint32), ref.join_books(ref.train(x, 10, 3, 16, 2, None, 3)).view(np.uint32))
    with pytest.raises(fv.engine.InvalidConfig):
        pq.decode(np.full((1, 3), 5, np.uint8))  # a code >= ksub_actual
    pq.close()


def test_refusals(fv, ctx):
    with pytest.raises(fv.engine.InvalidConfig):
        fv.ProductQuantizer(ctx, 4, 5, 16)
    with pytest.raises(fv.engine.Unsupported):
        fv.ProductQuantizer(ctx, 16, 4, 257)
    with pytest.raises(fv.engine.Unsupported):
        fv.ProductQuantizer(ctx, 300, 2, 16)  # 150 dims in a subspace
    pq = fv.ProductQuantizer(ctx, 8, 2, 4)
    x = np.ones((6, 8), np.float32)
    for call in (lambda: pq.encode(x), lambda: pq.decode(np.zeros((1, 2), np.uint8)), pq.codebooks, lambda: fv.PQIndex(ctx, pq)):
        with pytest.raises(fv.engine.NotTrained):
            call()
    pq.train(x, 0, init_rows=np.array([[0, 1, 2, 3], [0, 1, 2, 3]], np.uint32))
    bad = x.copy()
    bad[3, 5] = np.nan
    with pytest.raises(fv.engine.NonFiniteInput):
        pq.encode(bad)
    with pytest.raises(fv.engine.DimensionMismatch):
        pq.encode(np.ones((2, 9), np.float32))
    pq.close()
