"""GPU: retrain / add_clusters / optimize_clusters / vacuum with the rows resident in HBM (src/ivf/operations.rs:148-260,
:625-645) against the CPU oracle.  The oracle has no retrain of its own; it is restated from its primitives: the rows in
sequence order (lists ascending, list-position order inside), a fresh index with the new config and the same seed,
train on them, insert them in that order, mark the deleted ids again."""
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


def assert_same_results(g, cpu_ids, cpu_ds, cpu_cnt):
    assert np.array_equal(g.counts, cpu_cnt)
    for b in range(len(g)):
        n = int(cpu_cnt[b])
        assert np.array_equal(g.ids[b, :n], cpu_ids[b, :n]), f"query {b}"
        assert np.array_equal(bits(g.distances[b, :n]), bits(cpu_ds[b, :n])), f"query {b}"


def sequence(o, nlist):
    return np.concatenate([o.list_ids(c) for c in range(nlist)]).astype(np.uint64)


def restated_retrain(o, nlist_old, rows_by_id, dead, **cfg):
    order = sequence(o, nlist_old)
    x = np.stack([rows_by_id[int(i)] for i in order])
    n = orc.IVFIndex(**cfg)
    res = n.train(x)
    n.batch_insert(order, x)
    for i in dead:
        n.mark_deleted(i)
    return n, res, order


def assert_same_index(g, o, nlist, q, dead=()):
    assert np.array_equal(bits(g.get_centroids()), bits(o.get_centroids())), "centroids are not bit-equal"
    for c in range(nlist):
        _, ids, live = g.export_list(c)
        assert ids.tolist() == o.list_ids(c).tolist(), f"list {c}: ids or their order differ"
        assert live.tolist() == [int(i) not in dead for i in ids], f"list {c}: live flags"
    for k, npb in ((10, min(4, nlist)), (1, 1), (25, nlist), (64, min(7, nlist))):
        assert_same_results(g.search(q, k, npb), *o.batch_search(q, k, npb))


def build_pair(fv, ctx, x, ids, nlist, seed, max_iterations=25):
    g = fv.IVFIndex(ctx, n_clusters=nlist, n_probe=min(4, nlist), max_iterations=max_iterations, seed=seed)
    o = orc.IVFIndex(n_clusters=nlist, n_probe=min(4, nlist), max_iterations=max_iterations, seed=seed)
    g.train(x[: max(4 * nlist, 64)])
    o.train(x[: max(4 * nlist, 64)])
    g.batch_insert(ids, x)
    o.batch_insert(ids, x)
    return g, o


# ---- 1. retrain parity ---------------------------------------------------------------------------------------------
# the last case gathers more rows from the lists than one 8192-element tile of the sequential training sums holds
@pytest.mark.parametrize("old,new,d,n", [
    pytest.param(3, 16, 32, 5000, id="3-16-32"), pytest.param(64, 24, 20, 5000, id="64-24-20"),
    pytest.param(8, 12, 10, 5000, id="8-12-10"), pytest.param(5, 9, 12, 9000, id="5-9-12-9000")])
def test_retrain_matches_restated_oracle(fv, ctx, old, new, d, n):
    x = mixture(n, d, n_comp=20, seed=old * 100 + new)
    ids = np.arange(n, dtype=np.uint64) * 3 + 11
    rows = {int(i): x[j] for j, i in enumerate(ids)}
    g, o = build_pair(fv, ctx, x, ids, old, seed=7)
    dead = set(int(i) for i in ids[5:900:17])
    for i in dead:
        g.mark_deleted(i)
        o.mark_deleted(i)
    cfg = dict(n_clusters=new, n_probe=min(5, new), max_iterations=12, seed=99)
    o2, ores, _ = restated_retrain(o, old, rows, dead, **cfg)
    res = g.retrain(new, n_probe=cfg["n_probe"], max_iterations=12, seed=99)
    assert res == dict(old_clusters=old, new_clusters=new, vectors_reassigned=n, converged=ores["converged"])
    assert g.n_clusters == new and g.total_vectors() == n == o2.total_vectors()
    assert g.active_count() == n - len(dead)
    q = mixture(48, d, n_comp=20, seed=5)
    assert_same_index(g, o2, new, q, dead)
    info = g.maintenance_info()
    assert info["rows_in"] == n and info["rows_out"] == n
    assert info["host_bytes"] <= 16 * n + 64 * (old + new) + 4096, "rows must not cross the host link"
    # life goes on in the new partition
    extra = mixture(100, d, n_comp=20, seed=6)
    eid = np.arange(100, dtype=np.uint64) + 10**6
    g.batch_insert(eid, extra)
    o2.batch_insert(eid, extra)
    assert_same_index(g, o2, new, q, dead)


# ---- 2. add_clusters / optimize_clusters parity ----------------------------------------------------------------------
def test_add_clusters_and_optimize_clusters_match(fv, ctx):
    n, d, nlist = 3000, 16, 10
    x = mixture(n, d, n_comp=12, seed=21)
    ids = np.arange(n, dtype=np.uint64) + 1
    rows = {int(i): x[j] for j, i in enumerate(ids)}
    g, o = build_pair(fv, ctx, x, ids, nlist, seed=3, max_iterations=15)
    dead = {int(ids[4]), int(ids[77])}
    for i in dead:
        g.mark_deleted(i)
        o.mark_deleted(i)
    q = mixture(32, d, n_comp=12, seed=22)
    o2, _, _ = restated_retrain(o, nlist, rows, dead, n_clusters=nlist + 5, n_probe=4, max_iterations=15, seed=3)
    assert g.add_clusters(5) == dict(clusters_added=5, vectors_reassigned=n)
    assert g.n_clusters == nlist + 5 and g.total_vectors() == n
    assert_same_index(g, o2, nlist + 5, q, dead)
    # optimize_clusters: same config, fresh centroids from the rows in their present sequence order
    before = g.get_cluster_stats()
    o3, ores, _ = restated_retrain(o2, nlist + 5, rows, dead, n_clusters=nlist + 5, n_probe=4, max_iterations=15, seed=3)
    res = g.optimize_clusters()
    assert res["iterations"] == ores["iterations"] and res["improvement"] >= 0.0
    assert g.total_vectors() == 2 * n, "the reference does not reset total_vectors here: it doubles"
    assert_same_index(g, o3, nlist + 5, q, dead)
    after = g.get_cluster_stats()
    sizes = np.array([o3.get_cluster_size(c) for c in range(nlist + 5)], np.float32)
    var = np.float32(((sizes - sizes.sum(dtype=np.float32) / np.float32(sizes.size)) ** 2).sum(dtype=np.float32) / np.float32(sizes.size))
    assert after["n_clusters"] == nlist + 5 and after["empty_clusters"] == int((sizes == 0).sum())
    assert abs(after["size_variance"] - var) <= 1e-3 * max(var, 1.0)
    assert res["improvement"] == pytest.approx(max(before["size_variance"] - after["size_variance"], 0.0), rel=1e-6)


# ---- 3. the reference's own tests (tests/ivf/operations.rs:122-215) and the error cases -------------------------------
def trained_toy(fv, ctx):
    g = fv.IVFIndex(ctx, n_clusters=3, n_probe=2, train_size=9, max_iterations=10, seed=42)
    g.train(np.array([[0, 0], [0.1, 0.1], [-0.1, 0.1], [5, 5], [5.1, 4.9], [4.9, 5.1], [-5, -5], [-5.1, -4.9], [-4.9, -5.1]],
                     np.float32))
    return g


def test_reference_retrain_circle(fv, ctx):
    g = trained_toy(fv, ctx)
    ang = np.arange(50, dtype=np.float32) * np.float32(2 * np.pi / 50)
    g.batch_insert(np.arange(50, dtype=np.uint64), np.stack([np.cos(ang) * 5, np.sin(ang) * 5], 1).astype(np.float32))
    res = g.retrain(10, n_probe=3, train_size=50, max_iterations=20, seed=42)
    assert (res["old_clusters"], res["new_clusters"], res["vectors_reassigned"]) == (3, 10, 50) and res["converged"]
    assert g.n_clusters == 10 and g.total_vectors() == 50 and int(g.list_sizes().sum()) == 50
    assert g.search(np.zeros((1, 2), np.float32), 5).counts[0] > 0


def test_reference_add_clusters_outliers(fv, ctx):
    g = trained_toy(fv, ctx)
    x = np.stack([10.0 + np.arange(20, dtype=np.float32) * np.float32(0.1), np.full(20, 10.0, np.float32)], 1)
    g.batch_insert(np.arange(20, dtype=np.uint64), x)
    assert g.add_clusters(2) == dict(clusters_added=2, vectors_reassigned=20) and g.n_clusters == 5


def test_reference_optimize_uneven(fv, ctx):
    g = trained_toy(fv, ctx)
    x = np.array([[i * 0.1, i * 0.1] if i < 25 else [20.0, 20.0] for i in range(30)], np.float32)
    g.batch_insert(np.arange(30, dtype=np.uint64), x)
    before = g.get_cluster_stats()
    res = g.optimize_clusters()
    assert res["iterations"] > 0 and res["improvement"] >= 0.0
    assert g.get_cluster_stats()["size_variance"] <= before["size_variance"]


def test_error_cases_and_the_state_they_leave(fv, ctx):
    g = fv.IVFIndex(ctx, n_clusters=3, n_probe=2)
    for call in (lambda: g.retrain(4), lambda: g.add_clusters(1), g.optimize_clusters):
        with pytest.raises(fv.NotTrained):
            call()
    g = trained_toy(fv, ctx)
    with pytest.raises(fv.InvalidConfig):
        g.add_clusters(0)
    x = np.array([[0, 0], [5, 5], [-5, -5], [1, 1], [4, 4]], np.float32)
    g.batch_insert(np.arange(5, dtype=np.uint64), x)
    with pytest.raises(fv.InsufficientTrainingData):
        g.retrain(8, n_probe=2)
    # operations.rs:168-172: the config is replaced and `trained` cleared before train fails; the lists are whole
    assert g.n_clusters == 8 and not g.is_trained() and g.total_vectors() == 5
    with pytest.raises(fv.NotTrained):
        g.search(x[:1], 1)
    assert int(g.list_sizes().sum()) == 5
    g.train(np.vstack([x, x + 0.5]))  # training again builds the index for the new config, empty like the reference's
    assert g.is_trained() and g.total_vectors() == 0 and g.list_sizes().size == 8


# ---- 4. fp16 pool ---------------------------------------------------------------------------------------------------
def test_fp16_pool_retrain(fv, ctx):
    fp16_pool_retrain(fv, ctx, 4000)


def test_fp16_pool_train_from_across_a_tile(fv, ctx):
    # train_from gathers more rows from the fp16 lists than one 8192-element tile of the sequential training sums holds
    fp16_pool_retrain(fv, ctx, 9000)


def fp16_pool_retrain(fv, ctx, n):
    d, old, new = 32, 6, 14
    x = mixture(n, d, n_comp=10, seed=31)
    xh = x.astype(np.float16).astype(np.float32)  # what the pool stores, widened exactly
    ids = np.arange(n, dtype=np.uint64) + 5
    cents = x[:old].copy()
    src = fv.DeviceIVF(ctx, d, old, dtype="f16")
    src.set_centroids(cents)
    cl, pos = src.add(x, ids)
    dead = np.arange(3, 300, 7)
    src.set_deleted(cl[dead], pos[dead])
    order = np.concatenate([np.flatnonzero(cl == c) for c in range(old)])  # sequence order (appends keep row order)
    for c in range(old):
        rows, lid, _ = src.list_export(c)
        assert np.array_equal(lid, ids[order[cl[order] == c]]) and np.array_equal(bits(rows), bits(xh[cl == c]))
    o = orc.IVFIndex(n_clusters=new, n_probe=4, max_iterations=10, seed=5)
    ores = o.train(xh[order])
    o.batch_insert(ids[order], xh[order])
    for i in ids[dead]:
        o.mark_deleted(int(i))
    dst = fv.DeviceIVF(ctx, d, new, dtype="f16")
    res = dst.train_from(src, max_iterations=10, seed=5)
    assert res["iterations"] == ores["iterations"] and res["converged"] == ores["converged"]
    assert np.array_equal(bits(dst.get_centroids()), bits(o.get_centroids()))
    ncl, nids = dst.assign_from(src)
    assert np.array_equal(nids, ids[order]) and np.array_equal(ncl, o.assign(xh[order]))
    dst.refill_from(src)
    dead_ids = set(ids[dead].tolist())
    for c in range(new):
        rows, lid, live = dst.list_export(c)
        assert lid.tolist() == o.list_ids(c).tolist()
        assert live.tolist() == [i not in dead_ids for i in lid.tolist()]
        assert np.array_equal(bits(rows), bits(xh[(lid - 5).astype(np.int64)])), "fp16 rows must move as bit copies"
    q = mixture(32, d, n_comp=10, seed=32)
    for k, npb in ((10, 4), (50, new)):
        gi, gd, gc = dst.search(q, k, npb)
        oi, od, oc = o.batch_search(q, k, npb)
        assert np.array_equal(gc, oc)
        for b in range(q.shape[0]):
            m = int(oc[b])
            assert np.array_equal(gi[b, :m], oi[b, :m]) and np.array_equal(bits(gd[b, :m]), bits(od[b, :m]))
    assert src.total_rows() == n, "the source is left as it was"


# ---- 5. duplicate rule ----------------------------------------------------------------------------------------------
def test_duplicate_id_meeting_in_one_list(fv, ctx):
    g = fv.IVFIndex(ctx, n_clusters=2, n_probe=2, seed=1)
    g.set_trained(np.array([[0, 0], [10, 10]], np.float32))
    # id 7 twice: its first vector lies in list 0, its second in list 1
    x = np.array([[0, 0], [0.5, 0], [0.2, 0.2], [0, 0.5], [10, 10.5], [9, 10]], np.float32)
    ids = np.array([1, 2, 7, 3, 4, 7], np.uint64)
    assert g.batch_insert(ids, x) == (6, 0), "the duplicate check is per list (src/ivf/core.rs:128-134)"
    # sequence order: list 0 = ids 1, 2, 7, 3; list 1 = ids 4, 7.  One cluster: the second 7 repeats (7, list 0).
    with pytest.raises(fv.DuplicateVector):
        g.retrain(1, n_probe=1, max_iterations=5, seed=1)
    assert g.n_clusters == 1 and g.is_trained()
    assert g.export_list(0)[1].tolist() == [1, 2, 7, 3, 4], "rows before the repeat are in place, nothing after it"
    assert g.total_vectors() == 5
    r = g.search(np.array([[10, 10.5]], np.float32), 5, 1)
    assert r.counts[0] == 5 and r.ids[0, 0] == 4 and sorted(r.ids[0].tolist()) == [1, 2, 3, 4, 7]


# ---- 6. vacuum: what it was, and on the chip ---------------------------------------------------------------------------
def test_vacuum_resident_and_unchanged(fv, ctx):
    d, nlist = 24, 5
    # list sizes by construction: centroids far apart, rows right next to them
    sizes = [128, 64, 70, 200, 3]  # ends on a block boundary; emptied completely; drops by one block (70 -> 64); plain; tiny
    cents = (np.eye(nlist, d, dtype=np.float32) * 50).astype(np.float32)
    rng = np.random.default_rng(8)
    cl_of = np.repeat(np.arange(nlist), sizes)
    rng.shuffle(cl_of)
    n = cl_of.size
    x = (cents[cl_of] + rng.standard_normal((n, d)).astype(np.float32) * np.float32(0.3)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64) + 100
    g = fv.IVFIndex(ctx, n_clusters=nlist, n_probe=3)
    o = orc.IVFIndex(n_clusters=nlist, n_probe=3)
    g.set_trained(cents)
    o.set_trained(cents)
    g.batch_insert(ids, x)
    o.batch_insert(ids, x)
    assert g.list_sizes().tolist() == sizes
    members = [ids[cl_of == c] for c in range(nlist)]
    dead = members[1].tolist() + members[2][3:9].tolist() + members[3][::5].tolist() + members[0][-1:].tolist()
    for i in dead:
        g.mark_deleted(int(i))
        o.mark_deleted(int(i))
    q = np.vstack([cents, x[:20]])
    assert_same_results(g.search(q, 10, 3), *o.batch_search(q, 10, 3))
    assert g.vacuum() == len(dead) == o.vacuum()
    info = g.maintenance_info()
    assert info["rows_in"] == n and info["rows_out"] == n - len(dead) and info["move_bytes"] > 0
    assert info["host_bytes"] <= 16 * info["rows_in"], "ids and list tables only: the rows stay in HBM"
    assert g.list_sizes().tolist() == [127, 0, 64, 160, 3] and g.total_vectors() == n - len(dead) == g.active_count()
    for c in range(nlist):
        rows, lid, live = g.export_list(c)
        assert lid.tolist() == o.list_ids(c).tolist() and live.all()
        assert np.array_equal(bits(rows), bits(x[(lid - 100).astype(np.int64)]))
    for k, npb in ((10, 3), (200, 5), (1, 1)):
        assert_same_results(g.search(q, k, npb), *o.batch_search(q, k, npb))
    assert g.vacuum() == 0
    # inserts afterwards land behind the survivors; a delete after the vacuum finds the new positions
    extra = (cents[[1, 2, 0, 1]] + np.float32(0.1)).astype(np.float32)
    eid = np.array([9001, 9002, 9003, 9004], np.uint64)
    g.batch_insert(eid, extra)
    o.batch_insert(eid, extra)
    victim = int(members[3][1])
    g.mark_deleted(victim)
    o.mark_deleted(victim)
    for c in range(nlist):
        assert g.export_list(c)[1].tolist() == o.list_ids(c).tolist()
    assert_same_results(g.search(q, 20, 5), *o.batch_search(q, 20, 5))
    assert g.vacuum() == 1 == o.vacuum()
    assert_same_results(g.search(q, 20, 5), *o.batch_search(q, 20, 5))


# ---- 7. the rank kernels alone, through refill_from --------------------------------------------------------------------
@pytest.mark.parametrize("nlist", [1, 3, 1024, 16384])
def test_stable_ranks_against_numpy(fv, ctx, nlist):
    # rows (c, 0, 0, 0) with centroid c at (c, 0, 0, 0): the nearest centroid of a row is the destination drawn for it
    n, d = 200_000, 4
    rng = np.random.default_rng(nlist)
    dest = rng.integers(0, nlist, n).astype(np.uint32)
    if nlist > 3:
        dest[rng.random(n) < 0.3] = 5  # one crowded list
    x = np.zeros((n, d), np.float32)
    x[:, 0] = dest
    cents = np.zeros((nlist, d), np.float32)
    cents[:, 0] = np.arange(nlist)
    src = fv.DeviceIVF(ctx, d, 2)
    src.set_centroids(np.array([[-1, 0, 0, 0], [-2, 0, 0, 0]], np.float32))
    src.add_assigned(x, np.arange(n, dtype=np.uint64), (np.arange(n) >= 70_001).astype(np.uint32))  # sequence = row order
    dst = fv.DeviceIVF(ctx, d, nlist)
    dst.set_centroids(cents)
    cl, ids = dst.assign_from(src)
    assert np.array_equal(ids, np.arange(n, dtype=np.uint64)) and np.array_equal(cl, dest)
    keep = n - 1234
    pos = dst.refill_from(src, keep)
    order = np.argsort(dest[:keep], kind="stable")
    want = np.empty(keep, np.uint32)
    counts = np.bincount(dest[:keep], minlength=nlist)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    want[order] = (np.arange(keep) - np.repeat(starts, counts)).astype(np.uint32)
    assert np.array_equal(pos, want)
    assert np.array_equal(dst.list_sizes(), counts.astype(np.uint64)) and dst.total_rows() == keep
    for c in (0, 5 % nlist, nlist - 1):
        rows, lid, live = dst.list_export(c)
        assert np.array_equal(lid, np.flatnonzero(dest[:keep] == c).astype(np.uint64)) and live.all()
        assert np.all(rows[:, 0] == c)


def test_more_lists_than_the_lds_form_serves_is_refused(fv, ctx):
    d = 4
    src = fv.DeviceIVF(ctx, d, 1)
    src.set_centroids(np.zeros((1, d), np.float32))
    src.add(np.ones((10, d), np.float32), np.arange(10, dtype=np.uint64))
    dst = fv.DeviceIVF(ctx, d, 16385)
    c = np.zeros((16385, d), np.float32)
    c[:, 0] = np.arange(16385)
    dst.set_centroids(c)
    dst.assign_from(src)
    with pytest.raises(fv.Unsupported):
        dst.refill_from(src)
    assert src.total_rows() == 10 and dst.total_rows() == 0


# ---- 8. hybrid ------------------------------------------------------------------------------------------------------
def test_hybrid_retrain_historical(fv, ctx):
    DAY = 86400.0
    n, d = 900, 16
    x = mixture(n, d, n_comp=8, seed=41)
    now = 1000 * DAY
    ages = np.where(np.random.default_rng(4).random(n) < 0.25, 1 * DAY, 30 * DAY)
    levels = orc.rng_levels(17, n)
    kw = dict(max_connections=8, max_connections_layer_0=16, ef_construction=40, n_clusters=3, n_probe=2)
    h = fv.HybridIndex(ctx, **kw)
    alone = fv.IVFIndex(ctx, n_clusters=3, n_probe=2)
    cents = x[:3].copy()
    h.set_ivf_centroids(cents)
    alone.set_trained(cents)
    for i in range(n):
        h.insert_with_timestamp(i, x[i], now - ages[i], now, int(levels[i]))
    hist = np.flatnonzero(ages >= 7 * DAY)
    alone.batch_insert(hist.astype(np.uint64), x[hist])
    h.delete(int(hist[3]), now)
    alone.mark_deleted(int(hist[3]))
    q = mixture(24, d, n_comp=8, seed=42)
    before = h.search(q, 10, now=now, hnsw_ef=40, ivf_n_probe=3)  # every list probed: the exact historical answer
    qd = ctx.upload(q)
    h.search_dev_begin(0, qd, q.shape[0], 10, now=now, hnsw_ef=40, ivf_n_probe=3, dim=d)
    with pytest.raises(fv.FvdbError):
        h.retrain_historical(12, n_probe=12, max_iterations=10, seed=9)  # a batch is in flight
    h.search_dev_end(0)
    res = h.retrain_historical(12, n_probe=12, max_iterations=10, seed=9)
    assert res["old_clusters"] == 3 and res["new_clusters"] == 12 and res["vectors_reassigned"] == hist.size
    alone.retrain(12, n_probe=12, max_iterations=10, seed=9)
    hi = h.ivf()
    assert hi.n_clusters == 12 and np.array_equal(bits(hi.get_centroids()), bits(alone.get_centroids()))
    for c in range(12):
        a, b = hi.export_list(c), alone.export_list(c)
        assert a[1].tolist() == b[1].tolist() and a[2].tolist() == b[2].tolist()
    after = h.search(q, 10, now=now, hnsw_ef=40, ivf_n_probe=12)
    assert np.array_equal(after.counts, before.counts)
    for b in range(q.shape[0]):
        m = int(before.counts[b])
        assert np.array_equal(bits(after.distances[b, :m]), bits(before.distances[b, :m]))
    ctx.free(qd)
