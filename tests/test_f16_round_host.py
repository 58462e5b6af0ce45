"""The host mirror's rounding routine (fvh_round_f16: what an index with row_dtype="f16" applies to every incoming row)
equals numpy's f32 -> float16 -> f32, bit for bit: round to nearest, ties to even, overflow to infinity, subnormals kept."""
import numpy as np
import pytest

import fvdb_import
from _data import bits


@pytest.fixture(scope="module")
def round_f16():
    fv = fvdb_import.load()
    host = fv.load_host()

    def f(x):
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(x)
        f32p = fv._capi.f32p
        host.fvh_round_f16(x.ctypes.data_as(f32p), x.size, out.ctypes.data_as(f32p))
        return out
    return f


def numpy_round(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def same(round_f16, x):
    x = np.asarray(x, np.float32)
    got, want = round_f16(x), numpy_round(x)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, [(x[i], got[i], want[i]) for i in bad[:5]]
    return got


def both_signs(v):
    v = np.asarray(v, np.float32)
    return np.concatenate([v, -v])


def neighbours(v):
    """each value with the f32 just below and just above it"""
    v = np.asarray(v, np.float32)
    return np.concatenate([v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(np.inf))])


def test_zeros_keep_their_sign(round_f16):
    got = same(round_f16, [0.0, -0.0])
    assert bits(got).tolist() == [0, 0x80000000]


def test_subnormal_ends_and_their_neighbours(round_f16):
    smallest, largest = 2.0 ** -24, 1023 * 2.0 ** -24          # fp16 subnormals: k * 2^-24, k = 1 .. 1023
    same(round_f16, both_signs(neighbours([smallest, largest, 2.0 ** -14, 2 * 2.0 ** -24, 1022 * 2.0 ** -24])))
    got = round_f16(np.float32([smallest, largest]))
    assert got.tolist() == [smallest, largest]


def test_below_half_the_smallest_subnormal_is_zero(round_f16):
    half = np.float32(2.0 ** -25)
    x = both_signs([half, np.nextafter(half, np.float32(0)), 2.0 ** -26, 2.0 ** -30, 1e-30, 1e-40, np.float32(1.4e-45)])
    got = same(round_f16, x)
    assert np.all(got == 0) and np.array_equal(np.signbit(got), np.signbit(x))
    assert same(round_f16, [np.nextafter(half, np.float32(1))])[0] == np.float32(2.0 ** -24)  # just above the tie: up


def test_exact_ties_go_to_the_even_mantissa(round_f16):
    # normal range: 1 + (2k + 1) / 2048 lies half way between mantissas k and k + 1
    k = np.arange(0, 1023)
    ties = (1.0 + (2 * k + 1) / 2048.0).astype(np.float32)
    got = same(round_f16, both_signs(neighbours(np.concatenate([ties, ties * 1024, ties * 2.0 ** -10]))))
    even_stays = round_f16(np.float32([1.0 + 1 / 2048.0]))[0]   # between mantissa 0 (even) and 1: stays at 0
    odd_moves = round_f16(np.float32([1.0 + 3 / 2048.0]))[0]    # between mantissa 1 (odd) and 2: moves to 2
    assert even_stays == np.float32(1.0) and odd_moves == np.float32(1.0 + 2 / 1024.0)
    assert got.size == 2 * 3 * 3 * 1023
    # subnormal range: (k + 1/2) * 2^-24
    ks = np.arange(0, 1024)
    same(round_f16, both_signs(neighbours(((ks + 0.5) * 2.0 ** -24).astype(np.float32))))
    # a carry out of the mantissa: 2 - 2^-11 is half way between 2 - 2^-10 (odd) and 2
    assert round_f16(np.float32([2.0 - 2.0 ** -11]))[0] == np.float32(2.0)


def test_top_of_the_range(round_f16):
    got = same(round_f16, both_signs(neighbours([65504.0, 65519.99, 65520.0, 65536.0, 1e5, 3e38])))
    assert round_f16(np.float32([65504.0, 65519.99]))[1] == np.float32(65504.0)
    assert np.isinf(round_f16(np.float32([65520.0]))[0]) and np.isinf(round_f16(np.float32([-65520.0]))[0])
    assert np.isinf(got).sum() > 0
    x = np.float32([np.inf, -np.inf])
    assert np.array_equal(round_f16(x), x)
    assert np.isnan(round_f16(np.float32([np.nan]))[0])


def test_random_bit_patterns(round_f16):
    rng = np.random.default_rng(16)
    u = rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)
    x = u.view(np.float32)
    x = x[np.isfinite(x)]
    same(round_f16, x)
    # the f32 range is mostly outside fp16's: the same number of patterns inside it
    e = rng.integers(127 - 26, 127 + 17, 100000, dtype=np.uint64).astype(np.uint32)
    u = (rng.integers(0, 2, 100000, dtype=np.uint64).astype(np.uint32) << 31) | (e << 23) | \
        rng.integers(0, 2 ** 23, 100000, dtype=np.uint64).astype(np.uint32)
    same(round_f16, u.view(np.float32))


def test_rounding_is_idempotent(round_f16):
    rng = np.random.default_rng(17)
    x = (rng.standard_normal(4096) * 10.0 ** rng.integers(-8, 5, 4096)).astype(np.float32)
    once = round_f16(x)
    assert np.array_equal(bits(round_f16(once)), bits(once))
