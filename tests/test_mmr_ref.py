"""The diverse selection's numpy reference (_mmr_ref.py) and the hand-built inputs the GPU tests
feed the kernel: this file proves, without a GPU, that the cases have the properties they are built for."""
import numpy as np
import pytest

import _mmr_ref as M

LAMS = (0.0, 0.25, 0.5, 1.0)  # every lam the GPU tests use


def cases():
    return {"random": M.random_case(40, 20, 1), "f16": M.random_case(40, 20, 2, f16=True), "lattice": M.lattice_case(48, 6, 3),
            "twins": M.twins_case(40, 20, 4), "identical": M.identical_case(20, 12),
            "repeats": M.with_repeats(M.random_case(40, 20, 5), [(0, 1), (3, 30), (7, 8), (7, 20)])}


def test_candidates_come_nearest_first_like_a_search():
    for name, (ids, dq, rows) in cases().items():
        assert dq.dtype == np.float32 and np.all(np.diff(dq.view(np.uint32).astype(np.int64)) >= 0), name


@pytest.mark.parametrize("distinct", [False, True])
def test_lam_1_is_the_prefix_of_the_kept_candidates(distinct):
    for name, (ids, dq, rows) in cases().items():
        n = len(ids)
        kept = np.flatnonzero(M.kept_mask(ids, n, distinct))
        for k in (1, 10, n):
            picks = M.mmr_one(ids, dq, rows, n, k, 1.0, distinct)
            assert picks == kept[:k].tolist(), (name, k)
    ids, dq, rows = cases()["repeats"]
    assert len(set(ids.tolist())) < len(ids)  # the case does hold copies
    picks = M.mmr_one(ids, dq, rows, len(ids), len(ids), 1.0, True)
    assert len(picks) == len(set(ids.tolist())) and len(set(ids[picks].tolist())) == len(picks)


@pytest.mark.parametrize("lam", LAMS)
def test_picks_have_unique_ranks_and_the_count_is_min_k_kept(lam):
    for name, (ids, dq, rows) in cases().items():
        for distinct in (False, True):
            n = len(ids)
            kept = int(M.kept_mask(ids, n, distinct).sum())
            for k in (1, 10, n):
                picks = M.mmr_one(ids, dq, rows, n, k, lam, distinct)
                assert len(picks) == min(k, kept) and len(set(picks)) == len(picks), (name, k)
                assert picks[0] == 0  # the first pick is the nearest candidate


@pytest.mark.parametrize("lam", LAMS)
def test_the_brute_force_formulation_agrees(lam):
    for name, (ids, dq, rows) in cases().items():
        for distinct in (False, True):
            pair = M.R.fold_distances(rows, rows)
            for n in (len(ids), 7, 1, 0):
                want = M.mmr_brute(ids, dq, rows, n, 12, lam, distinct)
                assert M.mmr_one(ids, dq, rows, n, 12, lam, distinct) == want, (name, n)
                assert M.mmr_one(ids, dq, rows, n, 12, lam, distinct, pair=pair) == want, (name, n)  # the shared fold


def test_the_tie_inputs_really_tie():
    c = cases()
    # an integer lattice ties where one term of the gain vanishes, not at a fractional lam: measured here, not assumed
    lattice = {lam: M.tie_rounds(c["lattice"], 24, lam, False) for lam in LAMS}
    assert lattice[0.0] > 0 and lattice[1.0] > 0
    # the same row under different ids has equal dq and equal m: a tie at EVERY lam, broken by the smaller position
    for lam in LAMS:
        assert M.tie_rounds(c["twins"], 24, lam, False) > 0, lam
        assert M.tie_rounds(c["identical"], 10, lam, False) > 0, lam
    # with copies of an id kept (distinct off) the copy ties with nothing it should not: it is demoted at lam < 1
    ids, dq, rows = c["repeats"]
    for lam in (0.0, 0.25, 0.5):
        picks = M.mmr_one(ids, dq, rows, len(ids), 10, lam, False)
        assert ids[picks[1]] != ids[picks[0]]  # candidate 1 is candidate 0's copy (m = 0) and is not the second pick


def test_a_twin_has_m_zero_and_lam_0_is_farthest_first():
    ids, dq, rows = cases()["random"]
    n = len(ids)
    picks = M.mmr_one(ids, dq, rows, n, 5, 0.0, False)
    pair = M.R.fold_distances(rows, rows)
    # the second pick is the row farthest from the first, the third maximises the distance to the nearer of the two
    assert picks[1] == int(np.argmax(pair[0]))
    rest = [c for c in range(n) if c not in picks[:2]]
    m = np.minimum(pair[picks[0], rest], pair[picks[1], rest])
    assert picks[2] == rest[int(np.argmax(m))]
    assert np.all(np.diag(pair) == 0)


def test_mmr_answer_shapes_and_tails():
    ids, dq, rows = cases()["repeats"]
    B = 3
    I, D, X = np.stack([ids] * B), np.stack([dq] * B), np.stack([rows] * B)
    counts = np.array([0, 4, len(ids)], np.uint32)
    oi, od, orank, oc = M.mmr_answer(I, D, X, counts, 10, 0.5, True)
    assert oi.dtype == np.uint64 and od.dtype == np.float32 and orank.dtype == np.uint32 and oc.dtype == np.uint32
    assert oc[0] == 0 and np.all(oi[0] == M.NO_ID) and np.all(np.isposinf(od[0])) and np.all(orank[0] == M.NO_ROW)
    assert oc[1] == 3 and np.all(oi[1, 3:] == M.NO_ID)  # candidates 0 and 1 share an id: 3 of the first 4 are kept
    assert oc[2] == 10 and np.array_equal(oi[2], ids[orank[2]]) and np.array_equal(od[2], dq[orank[2]])
