"""The counting rule of the quality grid against the merge it replaces, with no GPU: the split by
binary search plus prefix counts (_grid_ref.rule, what the device kernels compute) must give, for every case, the
figures of the brute-force stable merge followed by the reference's loop (_exact_ref.host_quality)."""
from types import SimpleNamespace

import numpy as np

from _data import bits
import _exact_ref as X
import _grid_ref as G


def random_case(rng):
    k, rk, hk = (int(rng.integers(1, 9)), int(rng.integers(0, 9)), int(rng.integers(0, 9)))
    vals = rng.integers(0, 5, size=rk + hk).astype(np.float32)  # five distinct distances: heavy ties, within and across parts
    if rng.random() < 0.2:
        vals[vals == 4] = np.inf
    gd, hd = np.sort(vals[:rk]), np.sort(vals[rk:])
    gi = rng.integers(0, 12, size=rk).astype(np.uint64)  # ids shared between the parts and repeated inside one
    hi = rng.integers(0, 12, size=hk).astype(np.uint64)
    truth = rng.integers(0, 12, size=int(rng.integers(0, k + 1))).astype(np.uint64)  # an id may sit twice in the truth
    return gi, gd, hi, hd, truth, k


def test_the_rule_equals_the_stable_merge_on_random_small_cases():
    rng = np.random.default_rng(1)
    seen_tie_at_cut = seen_shared = 0
    for trial in range(4000):
        gi, gd, hi, hd, truth, k = random_case(rng)
        (br, bp), merged = G.brute(gi, gd, hi, hd, truth, k)
        # the brute force itself is the reference's loop on the merged result
        res = SimpleNamespace(ids=merged[None, :], counts=np.array([merged.size]))
        tru = SimpleNamespace(ids=truth[None, :], counts=np.array([truth.size]))
        hr, hp = X.host_quality(res, tru, k)
        assert bits(hr) == bits(br) and bits(hp) == bits(bp), f"trial {trial}: brute force vs host_quality"
        rr, rp = G.rule(gi, gd, hi, hd, truth, k)
        assert bits(rr) == bits(br) and bits(rp) == bits(bp), \
            f"trial {trial}: rule {rr},{rp} vs merge {br},{bp}: G={gi},{gd} H={hi},{hd} T={truth} k={k}"
        L = merged.size
        a = G.split(gd, hd, L)
        seen_tie_at_cut += bool(0 < a <= gd.size and L - a < hd.size and gd[a - 1] == hd[L - a])
        seen_shared += bool(set(gi[:a].tolist()) & set(hi[:L - a].tolist()))
    assert seen_tie_at_cut > 100 and seen_shared > 100, "the cases this test is about did not occur"


def test_the_split_is_the_number_of_recent_entries_in_the_merged_prefix():
    rng = np.random.default_rng(2)
    for _ in range(2000):
        _, gd, _, hd, _, k = random_case(rng)
        part = np.concatenate([np.zeros(gd.size, int), np.ones(hd.size, int)])
        order = np.argsort(np.concatenate([gd, hd]), kind="stable")[:k]
        assert G.split(gd, hd, order.size) == int((part[order] == 0).sum())


def test_hand_cases():
    f = np.float32
    # equal distances across the parts exactly at the cut: the recent entry is in, the historical one is out
    assert G.rule([1], [2.0], [2], [2.0], [1], 1) == (f(1), f(1))
    assert G.rule([1], [2.0], [2], [2.0], [2], 1) == (f(0), f(0))
    # a migrated row: one id in both parts at the same distance, held once at k = 1 and twice at k = 2
    assert G.rule([7], [1.0], [7], [1.0], [7], 1) == (f(1), f(1))
    assert G.rule([7], [1.0], [7], [1.0], [7], 2) == (f(2) / f(1), f(1))
    # an id twice in the truth: min(len(truth), k) counts it twice, the result holds it once
    assert G.rule([7], [1.0], [], [], [7, 7], 2) == (f(1) / f(2), f(1))
    # empty truth, empty result
    assert G.rule([3], [1.0], [], [], [], 4) == (f(1), f(0))
    assert G.rule([], [], [], [], [5], 4) == (f(0), f(0))
    assert G.rule([], [], [], [], [], 4) == (f(1), f(0))


def test_summed_adds_in_query_order():
    v = np.array([[1e8, 1.0, -1e8], [1.0, 1.0, 1.0]], np.float32)
    assert G.summed(v).tolist() == [0.0, 3.0]  # (1e8 + 1) - 1e8 = 0 in f32: left to right, no tree
