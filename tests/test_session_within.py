"""CPU: radius_of_threshold (session.py) — the radius that stands for a score threshold is the
LARGEST f32 distance whose f32 score 1/(1+d) still clears it, so the device's `bits(dist) <= bits(radius)` is the
session's own predicate `score >= threshold` and its total is exact for it."""
import numpy as np
import pytest

import fvdb_import


def score(d):
    return np.float32(1.0) / (np.float32(1.0) + np.float32(d))  # session.rs:291, in f32


def up(v):
    with np.errstate(over="ignore"):  # above the largest finite value lies +inf
        return np.nextafter(np.float32(v), np.float32(np.inf))


ONE = np.float32(1.0)
THRESHOLDS = [ONE, np.nextafter(ONE, np.float32(0)), np.float32(1 - 2.0 ** -23), np.float32(0.999), np.float32(0.75), np.float32(0.5),
              np.float32(1 / 3), np.float32(0.1), np.float32(1e-6), np.float32(1e-30), np.float32(3e-38),
              np.float32(1.1754944e-38), up(np.float32(1.1754944e-38)), np.float32(1.1754942e-38), np.float32(1e-40),
              np.float32(1e-45)]


@pytest.mark.parametrize("t", THRESHOLDS, ids=lambda t: repr(float(t)))
def test_the_radius_is_the_last_distance_that_clears_the_threshold(t):
    fv = fvdb_import.load()
    d = fv.session.radius_of_threshold(t)
    assert isinstance(d, np.float32) and d >= 0
    assert score(d) >= t, f"d = {d} itself fails the predicate"
    if np.isposinf(d):  # only where even the largest finite distance clears it
        assert score(np.finfo(np.float32).max) >= t
    else:
        assert not score(up(d)) >= t, f"the next distance above {d} still clears {t}"


def test_threshold_one_is_distance_zero_or_a_rounding_away():
    fv = fvdb_import.load()
    d = fv.session.radius_of_threshold(1.0)
    assert score(d) == ONE and d < np.float32(1e-7)


def test_a_python_float_threshold_is_compared_as_search_compares_it():
    fv = fvdb_import.load()
    # search() narrows options["threshold"] to f32 before it compares (session.py, search)
    assert fv.session.radius_of_threshold(0.1) == fv.session.radius_of_threshold(np.float32(0.1))


@pytest.mark.parametrize("t", [0.0, -0.0, -1.0, -np.inf])
def test_a_threshold_of_zero_or_less_is_every_distance(t):
    fv = fvdb_import.load()
    assert np.isposinf(fv.session.radius_of_threshold(t))


@pytest.mark.parametrize("t", [up(ONE), 1.5, np.inf])
def test_a_threshold_above_one_is_no_distance(t):
    fv = fvdb_import.load()
    assert fv.session.radius_of_threshold(t) is None


def test_nan_is_refused():
    fv = fvdb_import.load()
    with pytest.raises(fv.session.SessionError):
        fv.session.radius_of_threshold(np.nan)
