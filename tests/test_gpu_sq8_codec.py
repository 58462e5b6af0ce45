"""GPU: the u8 scalar codec (fvdb_sq8_encode / fvdb_sq8_decode) against tests/_sq8_ref.py: codes and
decoded rows bit for bit, lo / hi by value, and the two refusals."""
import numpy as np
import pytest

import fvdb_import
import _sq8_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    c = fv.Context(0)
    yield c
    c.close()


def rows_for(n, d):
    """random rows, then (as n allows) the special ones, placed from the end"""
    x = np.random.default_rng(n * 4096 + d).standard_normal((n, d)).astype(np.float32)
    ramp = np.arange(d, dtype=np.float32)
    half = ramp.copy()
    half[-1] = 510.0
    special = [
        np.full(d, 3.25, np.float32),                                    # range 0
        half,                                                            # 0, 1, .. and 510 last: i / 510 * 255 = i / 2
        np.where(np.arange(d) % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32),  # +0 and -0
        (ramp + 1) * np.float32(1e-45) * np.where(np.arange(d) % 3 == 0, -1, 1).astype(np.float32),  # subnormals
        np.where(np.arange(d) % 2 == 0, np.float32(1e38), np.float32(-1e38)) * np.linspace(0.5, 1, d).astype(np.float32),
    ]
    for i, s in enumerate(special[:n]):
        x[n - 1 - i] = s
    return x


@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("d", [1, 31, 32, 33, 384])
def test_codec(fv, ctx, n, d):
    x = rows_for(n, d)
    codes, lo, hi = fv.scalar_quantize_u8(ctx, x)
    rc, rlo, rhi = ref.encode(x)
    assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi)  # by value: the sign of a zero is open
    assert np.array_equal(codes, rc)
    out = fv.dequantize_u8(ctx, codes, lo, hi)
    assert np.array_equal(out.view(np.uint32), ref.decode(rc, rlo, rhi).view(np.uint32))


def test_half_products_round_away(fv, ctx):
    # lo = 0, range = 255: v / 255 * 255 for v = i + 0.5 — the reference's own rounding decides each, checked against it
    x = (np.arange(255, dtype=np.float32) + np.float32(0.5))[None, :].copy()
    x[0, 0], x[0, -1] = 0.0, 255.0
    codes, _, _ = fv.scalar_quantize_u8(ctx, x)
    assert np.array_equal(codes, ref.encode(x)[0])


@pytest.mark.parametrize("bad", [np.nan, np.inf, "range"])
def test_refusals_leave_outputs_untouched(fv, ctx, bad):
    x = rows_for(5, 33)
    if bad == "range":
        x[3, 0], x[3, 1] = 3e38, -3e38  # finite elements, hi - lo = inf
    else:
        x[3, 7] = bad
    codes, lo, hi = np.full((5, 33), 77, np.uint8), np.full(5, 5.0, np.float32), np.full(5, 6.0, np.float32)
    import ctypes as C
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = ctx.lib.fvdb_sq8_encode(ctx.h, p(x, C.c_float), 5, 33, p(codes, C.c_uint8), p(lo, C.c_float), p(hi, C.c_float))
    with pytest.raises(fv.engine.NonFiniteInput):
        ctx.check(rc)
    assert np.all(codes == 77) and np.all(lo == 5.0) and np.all(hi == 6.0)
    with pytest.raises(fv.engine.Unsupported):
        fv.scalar_quantize_u8(ctx, np.zeros((1, 2049), np.float32))
