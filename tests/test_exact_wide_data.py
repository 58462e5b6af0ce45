"""The hand-built cases of test_gpu_exact_wide.py (_exact_wide_cases.py) have the properties those tests state — proven
here on the CPU with _exact_ref.fold_distances, so that a GPU failure cannot be a data accident (the precedent is
test_tie_cases_data.py)."""
import numpy as np
import pytest

from _data import bits
import _exact_ref as R
import _exact_wide_cases as W


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_tie_group_has_exactly_fifty_strictly_nearer_rows_and_equal_words(dtype):
    x, ids, v, q_on, q_50 = W.tie_case(dtype)
    assert x.shape == (W.N, 10) and ids.size == W.N
    assert np.array_equal(R.rounded(v), v), "the group's vector must survive fp16 storage unchanged"
    assert np.all(x[W.GROUP] == v) and W.GROUP.stop - W.GROUP.start == 600
    dist = W.tie_dist(dtype)
    words = bits(dist)
    # (a) the query ON the vector: the group's 600 words are bits 0
    assert np.all(words[0, W.GROUP] == 0)
    # (b) the group's 600 distances are bit-equal and exactly 50 rows are strictly nearer
    group_words = words[1, W.GROUP]
    assert np.all(group_words == group_words[0]) and group_words[0] != 0
    assert W.strictly_nearer(dist[1], group_words[0]) == W.NEARER
    # no row outside the group shares the group's word: the cut at k = 51..650 falls inside the group alone
    outside = np.ones(W.N, bool)
    outside[W.GROUP] = False
    assert not np.any(words[1, outside] == group_words[0])
    # so the reference's answer at k = 51 is the 50 nearer rows, then node 100
    wi, _, wc = R.exact_topk(dist[1:2], 51, ids=ids)
    assert wc[0] == 51 and wi[0, 50] == ids[100]
    wi, _, _ = R.exact_topk(dist[1:2], 651, ids=ids)
    assert list(wi[0, 50:650]) == list(ids[W.GROUP]) and wi[0, 650] not in set(ids[W.GROUP].tolist())


def test_the_two_row_types_share_one_tie_case():
    a, b = W.tie_case("f32"), W.tie_case("f16")
    for u, w in zip(a, b):
        assert np.array_equal(u, w)


def test_the_distance_zero_case_has_bits_zero():
    for dtype in ("f32", "f16"):
        x, _, v, q_on, _ = W.tie_case(dtype)
        d = R.fold_distances(q_on[None], W.stored(x, dtype)[W.GROUP])
        assert np.all(bits(d) == 0)


def test_same_rows_case_has_one_word_per_query():
    x, ids, q, dist = W.same_rows_case()
    assert x.shape[0] == 300 and np.all(x == x[0])
    w = bits(dist)
    assert np.all(w == w[:, :1])
    wi, _, wc = R.exact_topk(dist, 301, ids=ids)
    assert np.all(wc == 300) and np.array_equal(wi[0, :300], ids) and wi[0, 300] == R.NO_ID


@pytest.mark.parametrize("d", [10, 130, 384])
def test_cut_case_queries_sit_on_duplicated_rows(d):
    x, ids, q, dist = W.cut_case(d, "f32")
    assert x.shape == (W.N, d) and q.shape[0] == 33 and -(-W.N // 64) == 71 and W.N % 64 != 0
    w = bits(dist)
    # queries 29..32 sit on rows 10, 255, 700, 3, each of which has at least one copy
    for b, (row, copy) in zip(range(29, 33), [(10, 11), (255, 256), (700, 2100), (3, 4)]):
        assert w[b, row] == 0 and w[b, copy] == 0
    assert w[29, 12] == 0
