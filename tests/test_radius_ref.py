"""CPU: the reference of the radius search (_radius_ref.py) and the properties of the hand-built cases that
test_gpu_radius_search.py leans on, so that a GPU failure is never a data accident."""
import numpy as np
import pytest

from _data import bits
import _exact_ref as R
import _exact_wide_cases as W
import _radius_ref as RR


def test_radius_answer_is_exact_topk_cut_at_the_radius():
    rng = np.random.default_rng(3)
    dist = np.abs(rng.standard_normal((5, 40))).astype(np.float32)
    dist[0, 7] = dist[0, 3]          # a tie
    dist[1, 6] = np.float32(np.nan)  # a live row, never in a ball
    ids = np.arange(40, dtype=np.uint64) * 3 + 1
    live = np.ones(40, bool)
    live[::5] = False
    radius = np.array([dist[0, 3], np.inf, 0.0, 0.5, 1e-30], np.float32)
    for m in (1, 4, 40):
        wi, wd, wc, wt = RR.radius_answer(dist, radius, m, live=live, ids=ids)
        for b in range(5):
            inside = [j for j in range(40) if live[j] and dist[b, j] <= radius[b]]  # f32 <= on non-negative values
            assert wt[b] == len(inside) and wc[b] == min(m, len(inside))
            order = sorted(inside, key=lambda j: (int(bits(dist[b, j])[0]), j))[:m]
            assert list(wi[b, :wc[b]]) == [ids[j] for j in order]
            assert np.array_equal(bits(wd[b, :wc[b]]), bits(dist[b, order]))
            assert np.all(wi[b, wc[b]:] == RR.NO_ID) and np.all(np.isposinf(wd[b, wc[b]:]))
    assert RR.radius_answer(dist, np.inf, 40, live=live)[3][1] == live.sum() - 1  # the NaN row


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("d", [10, 384])
def test_cut_case_the_37th_distance_holds_37_rows(d, dtype):
    x, ids, q, dist = W.cut_case(d, dtype)
    assert dist.shape == (33, W.N)
    r37 = RR.kth_distance(dist, 37)
    assert np.all(RR.radius_answer(dist, r37, 64, ids=ids)[3] == 37), "a duplicate sits on the boundary"
    assert np.all(RR.radius_answer(dist, RR.below(r37), 64, ids=ids)[3] == 36)


def test_cut_case_radius_zero_finds_the_duplicated_rows():
    for d in (10, 384):
        x, ids, q, dist = W.cut_case(d, "f32")
        totals = RR.radius_answer(dist, 0.0, 8, ids=ids)[3]
        assert list(totals[29:33]) == [3, 2, 2, 2] and np.all(totals[:29] == 0)
        below_all = RR.below(dist[:29].min())
        assert below_all >= 0 and np.all(RR.radius_answer(dist[:29], below_all, 8)[3] == 0)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_tie_case_balls(dtype):
    x, ids, v, q_on, q_50 = W.tie_case(dtype)
    dist = W.tie_dist(dtype)
    g_on, g_50 = dist[0, 100], dist[1, 100]
    assert bits(g_on) == 0 and bits(g_50) == bits(np.float32(1.1726685))
    assert np.all(bits(dist[:, W.GROUP]) == bits(dist[:, 100:101]))
    totals = RR.radius_answer(dist, np.array([g_on, g_50], np.float32), 64)[3]
    assert list(totals) == [600, 650]
    assert W.strictly_nearer(dist[1], bits(g_50)) == W.NEARER
    assert RR.radius_answer(dist[1:2], RR.below(g_50), 64)[3][0] == W.NEARER


def test_same_rows_case_one_word_per_query():
    x, ids, q, dist = W.same_rows_case()
    for b in range(3):
        assert np.all(bits(dist[b]) == bits(dist[b, 0])) and dist[b, 0] > 0
    assert np.all(RR.radius_answer(dist, dist[:, 0], 64)[3] == 300)
    assert np.all(RR.radius_answer(dist, RR.below(dist[:, 0]), 64)[3] == 0)
