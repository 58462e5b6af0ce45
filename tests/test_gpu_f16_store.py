"""GPU: the row store with fp16 rows (fvdb_store_create_ex(..., FVDB_F16)).  Rows are rounded to
nearest even once, on the device, at append; everything that reads them widens exactly, so every value read back and
every distance is what an f32 store holding `x.astype(float16).astype(float32)` gives, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits

pytestmark = pytest.mark.gpu

DIMS = [20, 128, 130, 384, 768]  # below a block, one block, a padded block and a bit, the BASELINE dimensions
NO_ROW = 0xFFFFFFFF


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def numpy_round(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def edge_values():
    """the ends of the fp16 range and the places where rounding has to decide, both signs"""
    sub = np.float32([2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -25, 2.0 ** -26, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 1e-30])
    ties = np.float32([1 + 1 / 2048, 1 + 3 / 2048, 2 - 2.0 ** -11, 1024 + 0.5, 1026 + 1.0 - 0.5, 0.1, 1 / 3])
    top = np.float32([65504.0, 65519.99, 65520.0, 65536.0, 1e6])
    v = np.concatenate([np.float32([0.0]), sub, ties, top])
    v = np.concatenate([v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(np.inf))])
    return np.concatenate([v, -v]).astype(np.float32)


def data(n, d, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)) * scale).astype(np.float32)


def read_all(store):
    return np.stack([store.get(r) for r in range(store.rows())])


@pytest.mark.parametrize("d", DIMS)
def test_append_get_round_trip_is_numpy_rounding(fv, ctx, d):
    x = data(24, d, seed=d, scale=3.0)
    e = edge_values()
    x.reshape(-1)[: min(e.size, x.size)] = e[: x.size]   # the edge values, over the first rows
    x[-2, d - 1] = e[3]                                   # and in the last element before the pad
    s = fv.RowStore(ctx, d, dtype="f16")
    assert s.append(x[:10]) == 0 and s.append(x[10:]) == 10
    got, want = read_all(s), numpy_round(x)
    assert np.isinf(want).any(), "the overflowing values are stored as infinities (the C ABI's rule)"
    assert np.array_equal(bits(got), bits(want))
    assert ctx.lib.fvdb_store_dtype(s.h) == 1 and s.dtype == "f16"
    s.close()


def test_growth_past_the_initial_capacity_keeps_every_row(fv, ctx):
    d = 130
    x = data(700, d, seed=5)
    s = fv.RowStore(ctx, d, capacity_rows=64, dtype="f16")
    at = 0
    for m in (50, 14, 1, 200, 435):                       # up to the capacity exactly, one past it, then two more growths
        assert s.append(x[at:at + m]) == at
        at += m
    assert s.rows() == 700
    assert np.array_equal(bits(read_all(s)), bits(numpy_round(x)))
    s.close()


@pytest.mark.parametrize("d", [20, 130, 768])
def test_bytes_are_half_the_f32_stores(fv, ctx, d):
    x = data(100, d, seed=6)
    h, f = fv.RowStore(ctx, d, dtype="f16"), fv.RowStore(ctx, d)
    h.append(x)
    f.append(x)
    dpad = (d + 3) // 4 * 4
    assert f.nbytes() == 100 * dpad * 4 and h.nbytes() * 2 == f.nbytes()
    assert ctx.lib.fvdb_store_dtype(f.h) == 0
    h.close()
    f.close()


def expected(q, rounded, cand):
    out = np.full(cand.shape, np.inf, np.float32)
    for b in range(cand.shape[0]):
        ok = cand[b] != NO_ROW
        out[b, ok] = orc.l2_batch(q[b], rounded[cand[b, ok]])
    return out


@pytest.mark.parametrize("d", DIMS)
def test_scoring_equals_the_oracle_on_the_rounded_rows(fv, ctx, d):
    n, B, Cn = 300, 9, 37
    x = data(n, d, seed=100 + d, scale=2.0)
    x[:4] *= np.float32(1e-6)                            # rows that round into the subnormals
    x[4:8] *= np.float32(1e3)
    rounded = numpy_round(x)
    assert np.isfinite(rounded).all() and (bits(rounded) != bits(x)).any()
    rng = np.random.default_rng(d)
    q = data(B, d, seed=200 + d)
    cand = rng.integers(0, n, (B, Cn)).astype(np.uint32)
    cand[rng.random((B, Cn)) < 0.15] = NO_ROW            # pads: +inf
    cand[0, :8] = np.arange(8)
    s = fv.RowStore(ctx, d, capacity_rows=64, dtype="f16")
    s.append(x)
    assert np.array_equal(bits(s.score_candidates(q, cand)), bits(expected(q, rounded, cand)))
    # the hop loop's scorer, its queries taken from the stored rows: widened into the f32 query buffer
    lib = ctx.lib
    sc = C.c_void_p()
    ctx.check(lib.fvdb_scorer_create(s.h, B, Cn, C.byref(sc)))
    try:
        qrows = rng.integers(0, n, B).astype(np.uint32)
        qrows[:2] = (1, 5)
        ctx.check(lib.fvdb_scorer_set_query_rows(sc, qrows.ctypes.data_as(fv._capi.u32p), B))
        np.ctypeslib.as_array(lib.fvdb_scorer_cand_buffer(sc), (B, Cn))[:] = cand
        ctx.check(lib.fvdb_scorer_run(sc, B, Cn))
        got = np.ctypeslib.as_array(lib.fvdb_scorer_dist_buffer(sc), (B, Cn)).copy()
        assert np.array_equal(bits(got), bits(expected(rounded[qrows], rounded, cand)))
        # and with f32 queries from the host, which are not rounded
        ctx.check(lib.fvdb_scorer_set_queries(sc, q.ctypes.data_as(fv._capi.f32p), B))
        ctx.check(lib.fvdb_scorer_run(sc, B, Cn))
        got = np.ctypeslib.as_array(lib.fvdb_scorer_dist_buffer(sc), (B, Cn)).copy()
        assert np.array_equal(bits(got), bits(expected(q, rounded, cand)))
    finally:
        lib.fvdb_scorer_destroy(sc)
    s.close()
