"""GPU: k-means training (src/ivf/core.rs:240-429) against the CPU oracle at the boundaries the training kernels hard-code:
the 8192-element LDS tiles and the 16-groups of the sequential sums (seq_sqsum_mean_kernel, kpp_pick_kernel), the eight
256-dimension register slots of kmeans_update_kernel and the d <= 2048 limit, the 65536-row step of the assignment, and
tied or empty clusters.  Same rows, list count, max_iterations and seed on both sides; everything is compared exactly:
centroids bit for bit, iterations, converged, and both errors as f32.  There is no tolerance anywhere."""
import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def assert_same_training(gc, rg, oc, ro):
    assert rg["iterations"] == ro["iterations"] and rg["converged"] == ro["converged"], (rg, ro)
    for key in ("initial_error", "final_error"):
        assert bits(np.float32(rg[key])) == bits(np.float32(ro[key])), (key, rg, ro)
    differ = np.flatnonzero((bits(gc) != bits(oc)).any(axis=1))
    assert differ.size == 0, f"centroids {differ.tolist()} are not bit-equal"


def train_pair(fv, ctx, x, nlist, max_iterations, seed, coarse_mode=None):
    """The engine-level handle and the oracle trained on the same rows; asserts the parity of the training itself."""
    g = fv.DeviceIVF(ctx, x.shape[1], nlist)
    if coarse_mode is not None:
        g.set_coarse_mode(coarse_mode)
    o = orc.IVFIndex(n_clusters=nlist, n_probe=1, max_iterations=max_iterations, seed=seed)
    ro = o.train(x)
    rg = g.train(x, max_iterations=max_iterations, seed=seed)
    assert_same_training(g.get_centroids(), rg, o.get_centroids(), ro)
    return g, o, ro


def assert_same_lists_and_search(lists, search, o, nlist, q, k, nprobe):
    for c in range(nlist):
        assert lists(c).tolist() == o.list_ids(c).tolist(), f"list {c}: ids or their order differ"
    gi, gd, gc = search(q, k, nprobe)
    oi, od, ocnt = o.batch_search(q, k, nprobe)
    assert np.array_equal(gc, ocnt)
    for b in range(q.shape[0]):
        m = int(ocnt[b])
        assert np.array_equal(gi[b, :m], oi[b, :m]), f"query {b}"
        assert np.array_equal(bits(gd[b, :m]), bits(od[b, :m])), f"query {b}"


# ---- 1. tile and group boundaries of the sequential sums -----------------------------------------------------------
# A left-to-right f32 sum of thousands of unequal squares differs in its low bits from the same sum in any other order,
# so the two errors pin the order of seq_sqsum_mean_kernel; the next k-means++ pick depends on the cumulative sum of
# kpp_pick_kernel, so the centroids pin that one.
@pytest.mark.parametrize("n,nlist", [(8191, 5), (8192, 6), (8193, 7), (16384 + 17, 8), (20000, 6)])
def test_sequential_sums_across_tiles(fv, ctx, n, nlist):
    x = mixture(n, 8, n_comp=nlist + 2, seed=n)
    _, _, ro = train_pair(fv, ctx, x, nlist, max_iterations=6, seed=n % 97)
    assert ro["final_error"] > 0.0 and ro["initial_error"] > ro["final_error"]


# ---- 2. the k-means++ pick lands on a boundary: a hand-built case with a known answer --------------------------------
# Every row is the point A but nine.  Once an A row is the first pick only those nine carry any D^2 mass, so each is
# picked exactly once, after runs of zeros (the 16-at-a-time skip path), at the first and last element of a 16-group and
# of an 8192-tile and at the last row.  An index off by one, a lost tile base or a cumulative sum reset at a tile makes a
# pick land on an A row.
FAR_ROWS = [15, 16, 8191, 8192, 8207, 8208, 16383, 16384, 16384 + 16]


@pytest.mark.parametrize("seed", [1, 2, 5, 8])
@pytest.mark.parametrize("a", [(1.0, -2.0, 3.5, 0.25), (0.1, -1.7, 3.3, 0.3)], ids=["dyadic", "nondyadic"])
def test_pick_on_tile_and_group_boundaries(fv, ctx, a, seed):
    n = 16384 + 17
    x = np.tile(np.array(a, np.float32), (n, 1))
    step = np.array([1.0, -1.0, 0.5, 2.0], np.float32)
    for t in FAR_ROWS:
        x[t] = x[t] + np.float32(3 + t) * step
    o = orc.IVFIndex(n_clusters=10, n_probe=1, max_iterations=1, seed=seed)
    ro = o.train(x)
    oc = o.get_centroids()
    # the precondition of the case, on the oracle alone: the first pick was an A row, the other nine are the far rows
    got = oc[1:][np.argsort(oc[1:, 0])]
    assert np.array_equal(bits(got), bits(x[FAR_ROWS])), "the oracle did not pick the nine far rows: not this case"
    g = fv.DeviceIVF(ctx, 4, 10)
    rg = g.train(x, max_iterations=1, seed=seed)
    assert_same_training(g.get_centroids(), rg, oc, ro)


# ---- 3. the register slots of the centroid update, and the dimension limit -------------------------------------------
# thread t owns the dimensions t, t+256, ...: the first slot only (255, 256), a second slot one thread alone uses (257),
# four slots the last of which is partly used (1000; like 257 a dimension the padded row does not equal), all eight (2048)
@pytest.mark.parametrize("d,n,nlist", [(255, 300, 4), (256, 320, 5), (257, 333, 4), (1000, 400, 6), (2048, 300, 5)])
def test_centroid_update_slots(fv, ctx, d, n, nlist):
    x = mixture(n, d, n_comp=nlist + 1, seed=d)
    train_pair(fv, ctx, x, nlist, max_iterations=6, seed=d)


def test_training_above_2048_dimensions_is_refused(fv, ctx):
    d, nlist = 2049, 4
    x = mixture(40, d, n_comp=4, seed=7)
    g = fv.DeviceIVF(ctx, d, nlist)
    with pytest.raises(fv.Unsupported, match="training supports d <= 2048"):
        g.train(x, max_iterations=3, seed=1)
    # the handle still works
    o = orc.IVFIndex(n_clusters=nlist, n_probe=nlist)
    g.set_centroids(x[:nlist])
    o.set_trained(x[:nlist])
    assert np.array_equal(bits(g.get_centroids()), bits(x[:nlist]))
    assert np.array_equal(g.assign(x), o.assign(x))
    ids = np.arange(40, dtype=np.uint64)
    cl, _ = g.add(x, ids)
    o.batch_insert(ids, x)
    assert np.array_equal(cl, o.assign(x))
    for c in range(nlist):
        assert g.list_export(c)[1].tolist() == o.list_ids(c).tolist()


# ---- 4. ties and empty clusters ---------------------------------------------------------------------------------------
def five_points():
    pts = np.array([[0, 0], [4, 0], [0, 4], [4, 4], [9, 9]], np.float32)
    return pts, np.repeat(pts, 20, axis=0)


def assert_five_points_precondition(o):
    # more lists than distinct rows: the oracle's centroids 5, 6 and 7 repeat centroid 3 = (0, 0), so every copy of
    # (0, 0) ties four ways and belongs to the lowest index; lists 5 to 7 stay empty and keep their centroid
    oc = o.get_centroids()
    assert all(np.array_equal(oc[c], [0.0, 0.0]) for c in (3, 5, 6, 7)), oc
    assert sorted(map(tuple, oc[[0, 1, 2, 4]].tolist())) == [(0.0, 4.0), (4.0, 0.0), (4.0, 4.0), (9.0, 9.0)], oc


@pytest.mark.parametrize("coarse_mode", [0, 1], ids=["proposal", "exact"])
def test_duplicate_centroids_tie_to_the_lowest_list(fv, ctx, coarse_mode):
    # with 8 lists both modes end in the exact scan; the proposal itself is reached by the 80-list case further down
    pts, x = five_points()
    g, o, _ = train_pair(fv, ctx, x, 8, max_iterations=6, seed=3, coarse_mode=coarse_mode)
    assert_five_points_precondition(o)
    ids = np.arange(x.shape[0], dtype=np.uint64) + 7
    cl, _ = g.add(x, ids)
    o.batch_insert(ids, x)
    assert set(cl[:20].tolist()) == {3} and g.list_sizes()[5:].tolist() == [0, 0, 0]
    q = np.vstack([pts, pts + np.float32(0.25)])
    assert_same_lists_and_search(lambda c: g.list_export(c)[1], g.search, o, 8, q, 30, 8)


def test_duplicate_centroids_through_the_index(fv, ctx):
    pts, x = five_points()
    g = fv.IVFIndex(ctx, n_clusters=8, n_probe=8, max_iterations=6, seed=3)
    o = orc.IVFIndex(n_clusters=8, n_probe=8, max_iterations=6, seed=3)
    ro, rg = o.train(x), g.train(x)
    assert_same_training(g.get_centroids(), rg, o.get_centroids(), ro)
    assert_five_points_precondition(o)
    ids = np.arange(x.shape[0], dtype=np.uint64) + 7
    assert g.batch_insert(ids, x) == (x.shape[0], 0)
    o.batch_insert(ids, x)
    q = np.vstack([pts, pts + np.float32(0.25)])

    def search(q, k, nprobe):
        r = g.search(q, k, nprobe)
        return r.ids, r.distances, r.counts

    assert_same_lists_and_search(lambda c: g.export_list(c)[1], search, o, 8, q, 30, 8)


def test_identical_rows(fv, ctx):
    # no D^2 mass: the threshold is zero and every pick is index 0.  List 0 takes every row and its centroid becomes their
    # mean in data order (a hundred additions round: it is not the row); the other three stay empty and keep the row
    x = np.tile(mixture(1, 16, n_comp=1, seed=3), (100, 1))
    g, o, ro = train_pair(fv, ctx, x, 4, max_iterations=5, seed=11)
    assert np.array_equal(bits(o.get_centroids()[1:]), bits(x[:3])) and ro["initial_error"] == 0.0
    assert np.array_equal(g.assign(x), o.assign(x))


@pytest.mark.parametrize("coarse_mode", [0, 1], ids=["proposal", "exact"])
def test_ten_copies_of_forty_rows(fv, ctx, coarse_mode):
    # the reference bench's shape: fewer distinct rows than rows, nearly as many lists as distinct rows
    x = np.tile(mixture(40, 16, seed=17), (10, 1))
    g, o, _ = train_pair(fv, ctx, x, 30, max_iterations=8, seed=4, coarse_mode=coarse_mode)
    assert np.array_equal(g.assign(x), o.assign(x))


@pytest.mark.parametrize("coarse_mode", [0, 1], ids=["proposal", "exact"])
def test_duplicate_centroids_under_the_matrix_core_proposal(fv, ctx, coarse_mode):
    # the coarse stage lets the matrix cores propose only from 64 lists on (and a padded dimension that is a multiple of
    # 16): 80 lists over 70 distinct rows, so at least ten centroids repeat another and their rows tie in the proposal.
    # Eight copies of each row, on a grid of 1/64: their sums are exact and a list's mean is the row itself, so the ties
    # last through every iteration and into the lists
    base = (np.round(mixture(70, 16, n_comp=9, seed=23) * 64) / 64).astype(np.float32)
    x = np.tile(base, (8, 1))
    g, o, _ = train_pair(fv, ctx, x, 80, max_iterations=6, seed=6, coarse_mode=coarse_mode)
    oc = o.get_centroids()
    assert np.unique(bits(oc), axis=0).shape[0] == 70, "the centroids are not the 70 distinct rows: not this case"
    ids = np.arange(x.shape[0], dtype=np.uint64)
    cl, _ = g.add(x, ids)
    o.batch_insert(ids, x)
    assert np.array_equal(cl, o.assign(x))
    assert_same_lists_and_search(lambda c: g.list_export(c)[1], g.search, o, 80, base[:16] + np.float32(0.01), 20, 80)


# ---- 5. more rows than one assignment step --------------------------------------------------------------------------
def test_more_rows_than_one_assignment_step(fv, ctx):
    n, d, nlist = 70_000, 4, 4
    x = mixture(n, d, n_comp=6, seed=70)
    g, o, _ = train_pair(fv, ctx, x, nlist, max_iterations=4, seed=2)
    o.batch_insert(np.arange(n, dtype=np.uint64), x)
    want = np.full(n, nlist, np.uint32)
    for c in range(nlist):
        want[o.list_ids(c).astype(np.int64)] = c
    got = g.assign(x)
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, f"{wrong.size} rows differ, the first at {wrong[:5].tolist()}"
