"""Recall and precision at every n_probe from one search of every list.

fvdb_ivf_quality_curve_dev returns, for p = 1 .. nlist, the sums over the queries of the per-query recall and precision
that evaluate_search_quality computes at n_probe = p; IVFIndex.recall_by_nprobe divides them by B.  The expected values
always come from the oracle through _curve_ref.py (the rule, pinned against the oracle's p-probe searches by
test_nprobe_curve_symbols.py) or expected_quality; every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
import _any_nprobe_data as D
import _curve_ref as R
from _data import bits, mixture

pytestmark = pytest.mark.gpu

E_NOT_TRAINED, E_INVALID, E_UNSUPPORTED = 1, 6, 12
NLIST = D.NLIST
DAY = 86400.0
u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def dev_curve_rc(ctx, h, q, k, chunk=0, mask=None, fill=None):
    """fvdb_ivf_quality_curve_dev: (status, recall sums [nlist], precision sums [nlist])."""
    q = np.ascontiguousarray(q, np.float32)
    nlist = h.nlist
    q_dev = ctx.upload(q if q.size else np.zeros((1, h.d), np.float32))
    start = np.full(2 * nlist, -1.0 if fill is None else fill, np.float32)
    out = ctx.upload(start)
    try:
        rc = ctx.lib.fvdb_ivf_quality_curve_dev(h.h, None, 0, mask, q_dev, q.shape[0], k, chunk, out,
                                                C.c_void_p(out.value + nlist * 4))
        ctx.synchronize()
        both = ctx.download(out, 2 * nlist, np.float32)
        return rc, both[:nlist], both[nlist:]
    finally:
        ctx.free(q_dev)
        ctx.free(out)


def dev_curve(ctx, h, q, k, chunk=0, mask=None):
    rc, recall, precision = dev_curve_rc(ctx, h, q, k, chunk, mask)
    ctx.check(rc)
    return recall, precision


def build_pair(fv, ctx, x, ids, cents, dtype="f32", clusters=None):
    """The device index and the oracle over the same rows in the same lists (the oracle's assignment unless given)."""
    nlist, d = cents.shape
    rows = D.f16_rounded(x) if dtype == "f16" else x  # what the reference would be given
    cpu = orc.IVFIndex(n_clusters=nlist, n_probe=min(4, nlist))
    cpu.set_trained(cents)
    cl = cpu.assign(x) if clusters is None else np.ascontiguousarray(clusters, np.uint32)
    cpu.batch_insert_assigned(ids, rows, cl)
    gpu = fv.DeviceIVF(ctx, d, nlist, dtype=dtype)
    gpu.set_centroids(cents)
    pos = gpu.add_assigned(x, ids, cl)
    return gpu, cpu, cl, pos


def assert_sums(got, want_values, what):
    """got: (recall sums, precision sums) of the device; want_values: per-query (recall, precision) [B][nlist]."""
    for name, g, w in (("recall", got[0], want_values[0]), ("precision", got[1], want_values[1])):
        want = R.curve_sums(w)
        bad = np.flatnonzero(bits(g) != bits(want))
        assert bad.size == 0, f"{what}: {name} sums differ at p = {bad[:5] + 1}: {g[bad[:5]]} vs {want[bad[:5]]}"


def assert_curve(got, want_values, what):
    """got: IVFIndex.recall_by_nprobe's dict; the averages restated in np.float32, column by column and as one fold."""
    B = want_values[0].shape[0]
    assert got["queries_evaluated"] == B and got["avg_query_time_ms"] > 0
    for name, w in (("avg_recall", want_values[0]), ("avg_precision", want_values[1])):
        g = got[name]
        assert g.dtype == np.float32 and g.shape == (w.shape[1],)
        assert np.array_equal(bits(g), bits(R.curve_averages(w))), f"{what}: {name} differs"
        for p in (1, 2, w.shape[1]):
            assert bits(g[p - 1]) == bits(D.averaged(w[:, p - 1])), f"{what}: {name} at p={p} is not the reference's fold"


def expected_values(cpu, q, k, cents, ids, cl, live_ids=None):
    live = R.live_sizes(ids, cl, cents.shape[0], live_ids)
    recall, precision, _ = R.curve_per_query(cpu, q, k, cents, ids, cl, live)
    return recall, precision


# ---- data ------------------------------------------------------------------------------------------------------------------
def small_case():
    """12 lists, 600 rows, d = 20: lists 0..2 hold exactly 64 rows (one full block), list 3 none, the rest 51 each."""
    x = mixture(600, 20, n_comp=12, seed=5100)
    ids = np.arange(600, dtype=np.uint64) * 5 + 3
    cents = mixture(12, 20, n_comp=12, seed=5101)
    cl = np.concatenate([np.repeat(np.arange(3), 64), 4 + np.arange(600 - 192) % 8]).astype(np.uint32)
    order = np.random.default_rng(5102).permutation(600)
    q = mixture(33, 20, n_comp=12, seed=5103)
    return x, ids, cents, np.ascontiguousarray(cl[order]), q


@pytest.fixture(scope="module")
def quality(fv, ctx):
    """quality_case on the device and in the oracle, untouched by the tests that share it."""
    x, ids, cents, q = D.quality_case()
    gpu, cpu, cl, pos = build_pair(fv, ctx, x, ids, cents)
    return dict(x=x, ids=ids, cents=cents, q=q, gpu=gpu, cpu=cpu, cl=cl, pos=pos,
                want={k: expected_values(cpu, q, k, cents, ids, cl) for k in (10, 300)})


# ---- 1. both routes, every p -------------------------------------------------------------------------------------------------
def test_register_route_12_lists(fv, ctx):
    x, ids, cents, cl, q = small_case()
    gpu, cpu, _, _ = build_pair(fv, ctx, x, ids, cents, clusters=cl)
    sizes = gpu.list_sizes()
    assert sizes[:4].tolist() == [64, 64, 64, 0]
    want = expected_values(cpu, q, 10, cents, ids, cl)
    assert_sums(dev_curve(ctx, gpu, q, 10), want, "nlist=12 k=10")
    # the rule against the repeated searches at every p of this index, through the oracle
    for p in range(1, 13):
        recall, precision = D.per_query_quality(cpu.batch_search(q, 10, p), cpu.batch_search(q, 10, 12), 10)
        assert np.array_equal(bits(want[0][:, p - 1]), bits(recall)) and np.array_equal(bits(want[1][:, p - 1]), bits(precision))
    # k = 257: any k above FVDB_MAX_K takes the wide search, which serves 12 lists as it serves 300 — so does the curve
    assert_sums(dev_curve(ctx, gpu, q, 257), expected_values(cpu, q, 257, cents, ids, cl), "nlist=12 k=257")


@pytest.mark.parametrize("k", [10, 300])
def test_wide_route_300_lists(fv, ctx, quality, k):
    w = quality
    assert np.count_nonzero(w["gpu"].list_sizes() == 0) >= 20, "empty lists rank among the probes"
    assert_sums(dev_curve(ctx, w["gpu"], w["q"], k), w["want"][k], f"nlist=300 k={k}")
    g = fv.IVFIndex(ctx, n_clusters=NLIST, n_probe=4)
    g.set_trained(w["cents"])
    g.batch_insert(w["ids"], w["x"])
    got = g.recall_by_nprobe(w["q"], k)
    assert_curve(got, w["want"][k], f"IVFIndex k={k}")
    # monotone sanity: a longer prefix of the ranking never loses a truth row, and every list finds them all
    assert np.all(np.diff(got["avg_recall"]) >= 0) and got["avg_recall"][-1] == 1.0
    # the configured n_probe's figures are one entry of the curve
    one = g.evaluate_search_quality(w["q"], k)
    assert bits(one["avg_recall"]) == bits(got["avg_recall"][3]) and bits(one["avg_precision"]) == bits(got["avg_precision"][3])


def test_256_and_257_lists_over_the_same_rows(fv, ctx):
    # the register route's last index size and the ranking route's first: list 256 of the larger index is empty and its
    # centroid lies far from every query, so it ranks last and the first 256 entries are the smaller index's curve
    d = 20
    x = mixture(2000, d, n_comp=40, seed=5200)
    ids = np.arange(2000, dtype=np.uint64) + 11
    q = mixture(33, d, n_comp=40, seed=5201)
    cents = np.concatenate([x[:256], np.full((1, d), 1000.0, np.float32)])
    cpu256 = orc.IVFIndex(n_clusters=256, n_probe=4)
    cpu256.set_trained(cents[:256])
    cl = cpu256.assign(x)
    curves = {}
    for nlist in (256, 257):
        gpu, cpu, _, _ = build_pair(fv, ctx, x, ids, cents[:nlist].copy(), clusters=cl)
        want = expected_values(cpu, q, 10, cents[:nlist], ids, cl)
        curves[nlist] = dev_curve(ctx, gpu, q, 10)
        assert_sums(curves[nlist], want, f"nlist={nlist}")
    for a, b in zip(curves[256], curves[257]):
        assert np.array_equal(bits(a), bits(b[:256]))
        assert bits(b[256]) == bits(b[255])


# ---- 2. against the existing call ----------------------------------------------------------------------------------------------
def test_equals_search_quality_dev_summed_in_query_order(fv, ctx, quality):
    w = quality
    q, B, k, gpu = w["q"], w["q"].shape[0], 10, w["gpu"]
    recall, precision = dev_curve(ctx, gpu, q, k)
    q_dev, out = ctx.upload(q), ctx.alloc(B * 8)
    for p in (1, 2, 17, 256, 257, 300):
        ctx.check(ctx.lib.fvdb_ivf_search_quality_dev(gpu.h, None, 0, q_dev, B, k, p, out, C.c_void_p(out.value + B * 4)))
        ctx.synchronize()
        per_query = ctx.download(out, 2 * B, np.float32)
        sums = [np.float32(0), np.float32(0)]
        for b in range(B):
            sums = [np.float32(sums[0] + per_query[b]), np.float32(sums[1] + per_query[B + b])]
        assert bits(sums[0]) == bits(recall[p - 1]), f"p={p}: recall {sums[0]} vs {recall[p - 1]}"
        assert bits(sums[1]) == bits(precision[p - 1]), f"p={p}: precision {sums[1]} vs {precision[p - 1]}"
    ctx.free(q_dev)
    ctx.free(out)


# ---- 3. chunk boundaries ---------------------------------------------------------------------------------------------------------
def test_chunk_boundaries_do_not_change_a_bit(fv, ctx, quality):
    w = quality
    whole = dev_curve(ctx, w["gpu"], w["q"], 10, chunk=0)
    assert_sums(whole, w["want"][10], "chunk=0")
    for chunk in (8, 1, 33, 1000):
        got = dev_curve(ctx, w["gpu"], w["q"], 10, chunk=chunk)
        assert np.array_equal(bits(got[0]), bits(whole[0])) and np.array_equal(bits(got[1]), bits(whole[1])), f"chunk={chunk}"
    one = dev_curve(ctx, w["gpu"], w["q"][:1], 10)
    assert_sums(one, (w["want"][10][0][:1], w["want"][10][1][:1]), "B=1")
    x, ids, cents, cl, q = small_case()
    gpu, cpu, _, _ = build_pair(fv, ctx, x, ids, cents, clusters=cl)
    whole = dev_curve(ctx, gpu, q, 10)
    for chunk in (8, 1):
        got = dev_curve(ctx, gpu, q, 10, chunk=chunk)
        assert np.array_equal(bits(got[0]), bits(whole[0])) and np.array_equal(bits(got[1]), bits(whole[1])), f"12 lists chunk={chunk}"
    # B = 0: nothing to do, nothing written
    rc, r0, p0 = dev_curve_rc(ctx, gpu, q[:0], 10, fill=7.0)
    assert rc == 0 and np.all(r0 == 7.0) and np.all(p0 == 7.0)


# ---- 4. liveness -------------------------------------------------------------------------------------------------------------------
def test_deleted_rows_a_dead_list_k_above_the_live_rows_and_nothing_live(fv, ctx):
    x, ids, cents, q = D.quality_case()
    gpu, cpu, cl, pos = build_pair(fv, ctx, x, ids, cents)

    def kill(rows):
        gpu.set_deleted(cl[rows], pos[rows], True)
        for i in ids[rows]:
            cpu.mark_deleted(int(i))

    dead = np.zeros(ids.size, bool)
    dead[::3] = True
    kill(np.flatnonzero(dead))
    for k in (10, 300):
        assert_sums(dev_curve(ctx, gpu, q, k), expected_values(cpu, q, k, cents, ids, cl, ids[~dead]), f"a third deleted k={k}")
    # the nearest list of the first query that still has live rows, wholly deleted
    ranked = np.argsort(orc.l2_batch(q[0], cents), kind="stable")
    r0 = next(r for r, L in enumerate(ranked) if np.any((cl == L) & ~dead))
    rows = np.flatnonzero((cl == ranked[r0]) & ~dead)
    kill(rows)
    dead[rows] = True
    want = expected_values(cpu, q, 10, cents, ids, cl, ids[~dead])
    assert np.all(want[1][0, : r0 + 1] == 0.0) and want[1][0, -1] == 1.0, "the first r0 + 1 lists give the first query nothing"
    assert_sums(dev_curve(ctx, gpu, q, 10), want, "a list wholly deleted")
    # k above the live rows: the truth is every live row, the result at p every live row of p lists
    live = int(np.count_nonzero(~dead))
    assert live < 4096
    want = expected_values(cpu, q[:3], 4096, cents, ids, cl, ids[~dead])
    assert np.all(want[1][:, -1] == 1.0) and np.all(want[0][:, 0] < 1.0)
    assert_sums(dev_curve(ctx, gpu, q[:3], 4096), want, "k=4096")
    # every row deleted: the truth is empty (recall 1) and so is every result (precision 0)
    kill(np.flatnonzero(~dead))
    for k in (10, 300):
        recall, precision = dev_curve(ctx, gpu, q, k)
        B = np.float32(q.shape[0])
        assert np.all(recall == B) and np.all(precision == 0.0)


def test_an_index_with_no_rows_and_after_vacuum(fv, ctx):
    x, ids, cents, q = D.quality_case()
    g = fv.IVFIndex(ctx, n_clusters=NLIST, n_probe=4)
    g.set_trained(cents)
    got = g.recall_by_nprobe(q, 10)
    assert np.all(got["avg_recall"] == 1.0) and np.all(got["avg_precision"] == 0.0) and got["queries_evaluated"] == q.shape[0]
    g.batch_insert(ids, x)
    cpu, cl = D.oracle_index(x, ids, cents)
    gone = ids[1::4]
    for i in gone:
        g.mark_deleted(int(i))
        cpu.mark_deleted(int(i))
    keep = np.ones(ids.size, bool)
    keep[1::4] = False
    want = expected_values(cpu, q, 10, cents, ids, cl, ids[keep])
    assert_curve(g.recall_by_nprobe(q, 10), want, "before vacuum")
    assert g.vacuum() == gone.size
    cpu.vacuum()
    after = expected_values(cpu, q, 10, cents, ids[keep], cl[keep])
    assert np.array_equal(bits(after[0]), bits(want[0])) and np.array_equal(bits(after[1]), bits(want[1]))
    assert_curve(g.recall_by_nprobe(q, 10), after, "after vacuum")


# ---- 5. ties -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 300])
def test_ties_in_rows_and_in_centroids(fv, ctx, k):
    x, ids, cents, cl, q = D.tie_case()
    assert np.unique(ids).size == ids.size, "every copy has an id of its own: no id sits in two lists"
    gpu, cpu, _, _ = build_pair(fv, ctx, x, ids, cents, clusters=cl)
    assert_sums(dev_curve(ctx, gpu, q, k), expected_values(cpu, q, k, cents, ids, cl), f"tie_case k={k}")


# ---- 6. fp16 rows ------------------------------------------------------------------------------------------------------------------
def test_half_precision_rows(fv, ctx):
    x, ids, cents, q = D.quality_case()
    gpu, cpu, cl, _ = build_pair(fv, ctx, x, ids, cents, dtype="f16")  # the oracle holds the rounded rows
    assert_sums(dev_curve(ctx, gpu, q, 10), expected_values(cpu, q, 10, cents, ids, cl), "f16 k=10")
    g = fv.IVFIndex(ctx, n_clusters=NLIST, n_probe=4, row_dtype="f16")
    g.set_trained(cents)
    g.batch_insert(ids, x)
    assert_curve(g.recall_by_nprobe(q, 300), expected_values(cpu, q, 300, cents, ids, cl), "f16 IVFIndex k=300")


def oracle_allowing(w, allowed):
    """The oracle over the shared rows after mark_deleted of every id outside `allowed`."""
    o, _ = D.oracle_index(w["x"], w["ids"], w["cents"])
    keep = set(int(i) for i in allowed)
    for i in w["ids"]:
        if int(i) not in keep:
            o.mark_deleted(int(i))
    return o


# ---- 7. allow-set ------------------------------------------------------------------------------------------------------------------
def test_under_an_allow_set(fv, ctx, quality):
    w = quality
    x, ids, cents, q, cl = w["x"], w["ids"], w["cents"], w["q"], w["cl"]
    g = fv.IVFIndex(ctx, n_clusters=NLIST, n_probe=4)
    g.set_trained(cents)
    g.batch_insert(ids, x)
    half = ids[np.random.default_rng(5300).random(ids.size) < 0.5]
    # the four nearest lists of each of the first queries (the two nearest are a short list and its empty twin), emptied
    # by the allow-set
    near = set()
    for b in range(8):
        near.update(int(c) for c in np.argsort(orc.l2_batch(q[b], cents), kind="stable")[:4])
    away = ids[~np.isin(cl, list(near))]
    for name, allowed in (("half", half), ("nearest lists emptied", away)):
        o = oracle_allowing(w, allowed)
        for k in (10, 300):
            want = expected_values(o, q, k, cents, ids, cl, allowed)
            if name != "half":
                assert np.all(want[1][:8, 0] == 0.0), "the nearest list of the first queries holds no allowed row"
            assert_curve(g.recall_by_nprobe(q, k, allowed=allowed), want, f"{name} k={k}")
    # the same through the C entry point with a mask of the caller's
    mask = C.c_void_p()
    ctx.check(ctx.lib.fvdb_mask_create_ivf(w["gpu"].h, half.ctypes.data_as(u64p), half.size, C.byref(mask)))
    assert_sums(dev_curve(ctx, w["gpu"], q, 10, mask=mask), expected_values(oracle_allowing(w, half), q, 10, cents, ids, cl, half),
                "masked C entry")
    ctx.lib.fvdb_mask_destroy(mask)
    # an allow-set that allows nothing
    got = g.recall_by_nprobe(q, 10, allowed=[])
    assert np.all(got["avg_recall"] == 1.0) and np.all(got["avg_precision"] == 0.0)


# ---- 8. smallest_n_probe -----------------------------------------------------------------------------------------------------------
def test_smallest_n_probe(fv, ctx, quality):
    w = quality
    g = fv.IVFIndex(ctx, n_clusters=NLIST, n_probe=4)
    g.set_trained(w["cents"])
    g.batch_insert(w["ids"], w["x"])
    avg = R.curve_averages(w["want"][10][0])
    assert avg[0] < 0.95 < avg[-1], "the target is met somewhere inside the curve"
    for target in (0.5, 0.95, float(avg[5]), 1.0):
        p, curve = g.smallest_n_probe(w["q"], 10, target)
        first = int(np.flatnonzero(avg >= np.float32(target))[0]) + 1
        assert p == first and 1 <= p <= NLIST, f"target {target}: {p} vs {first}"
        assert np.array_equal(bits(curve["avg_recall"]), bits(avg))
        assert curve["avg_recall"][p - 1] >= np.float32(target) and (p == 1 or curve["avg_recall"][p - 2] < np.float32(target))
    p, curve = g.smallest_n_probe(w["q"], 10, 1.5)
    assert p is None and curve["avg_recall"].max() == 1.0


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(fv, ctx, quality):
    w = quality
    q, d = w["q"], w["q"].shape[1]
    g = fv.IVFIndex(ctx, n_clusters=NLIST, n_probe=4)
    with pytest.raises(fv.NotTrained):
        g.recall_by_nprobe(q, 10)
    with pytest.raises(fv.InvalidConfig):  # the empty batch comes first, as in evaluate_search_quality
        g.recall_by_nprobe(q[:0], 10)
    g.set_trained(w["cents"])
    g.batch_insert(w["ids"], w["x"])
    with pytest.raises(fv.InvalidConfig):
        g.recall_by_nprobe([], 10)
    for k in (0, 4097):
        with pytest.raises(fv.Unsupported):
            g.recall_by_nprobe(q, k)
    with pytest.raises(fv.DimensionMismatch):
        g.recall_by_nprobe(np.zeros((3, d + 1), np.float32), 10)
    bad = q.copy()
    bad[5, 3] = np.inf
    with pytest.raises(fv.NonFiniteInput):
        g.recall_by_nprobe(bad, 10)
    # the C entry point
    gpu = w["gpu"]
    raw = fv.DeviceIVF(ctx, d, NLIST)
    assert dev_curve_rc(ctx, raw, q, 10)[0] == E_NOT_TRAINED
    for k in (0, 4097):
        assert dev_curve_rc(ctx, gpu, q, k)[0] == E_UNSUPPORTED
    q_dev, out = ctx.upload(q), ctx.alloc(NLIST * 4)
    assert ctx.lib.fvdb_ivf_quality_curve_dev(gpu.h, None, 0, None, None, 3, 10, 0, out, out) == E_INVALID
    assert ctx.lib.fvdb_ivf_quality_curve_dev(gpu.h, None, 0, None, q_dev, 3, 10, 0, None, out) == E_INVALID
    assert ctx.lib.fvdb_ivf_quality_curve_dev(gpu.h, None, 0, None, q_dev, 3, 10, 0, out, None) == E_INVALID
    assert ctx.lib.fvdb_ivf_quality_curve_dev(gpu.h, None, 99, None, q_dev, 3, 10, 0, out, out) == E_INVALID
    ctx.free(q_dev)
    ctx.free(out)


def test_a_stale_or_foreign_mask_and_a_shard_are_refused(fv, ctx):
    x, ids, cents, cl, q = small_case()
    gpu, cpu, _, pos = build_pair(fv, ctx, x, ids, cents, clusters=cl)
    other, _, _, _ = build_pair(fv, ctx, x, ids, cents, clusters=cl)
    mask = C.c_void_p()
    ctx.check(ctx.lib.fvdb_mask_create_ivf(gpu.h, ids.ctypes.data_as(u64p), ids.size, C.byref(mask)))
    assert dev_curve_rc(ctx, gpu, q, 10, mask=mask)[0] == 0
    assert dev_curve_rc(ctx, other, q, 10, mask=mask)[0] == E_INVALID
    gpu.set_deleted(cl[:1], pos[:1], True)
    rc = dev_curve_rc(ctx, gpu, q, 10, mask=mask)[0]
    assert rc == E_INVALID and b"stale" in ctx.lib.fvdb_last_error(ctx.h)
    ctx.lib.fvdb_mask_destroy(mask)
    gpu.set_global_list_sizes(gpu.list_sizes())
    rc = dev_curve_rc(ctx, gpu, q, 10)[0]
    assert rc == E_UNSUPPORTED and b"shard" in ctx.lib.fvdb_last_error(ctx.h)


# ---- 10. the hybrid index's historical part ----------------------------------------------------------------------------------------
def test_hybrid_ivf_view_has_the_curve(fv, ctx):
    n, d, now, nlist = 600, 20, 1000 * DAY, 40
    x = mixture(n, d, n_comp=20, seed=5400)
    ids = np.arange(n, dtype=np.uint64) * 2 + 1
    cents = x[:nlist].copy()
    ages = np.where(np.random.default_rng(5401).random(n) < 0.2, 1 * DAY, 3 * DAY)
    levels = orc.rng_levels(5401, n)
    h = fv.HybridIndex(ctx, max_connections=8, max_connections_layer_0=16, ef_construction=40, n_clusters=nlist, n_probe=4)
    h.set_ivf_centroids(cents)
    for i in range(n):
        h.insert_with_timestamp(int(ids[i]), x[i], now - ages[i], now, int(levels[i]))
    assert h.historical_count() == 0
    later = now + 10 * DAY  # everything written so far is older than a week by then
    for _ in range(2 * n // 100 + 2):  # a call copies one migration batch
        if h.recent_count() == 0:
            break
        h.migrate_with_threshold(7 * DAY, later)
    assert h.historical_count() == n and h.recent_count() == 0
    q = mixture(9, d, n_comp=20, seed=5402)
    got = h.ivf().recall_by_nprobe(q, 10)
    # a stand-alone index holding the historical rows, and the oracle over the lists the view reports
    alone = fv.IVFIndex(ctx, n_clusters=nlist, n_probe=4)
    alone.set_trained(cents)
    alone.batch_insert(ids, x)
    same = alone.recall_by_nprobe(q, 10)
    assert np.array_equal(bits(got["avg_recall"]), bits(same["avg_recall"]))
    assert np.array_equal(bits(got["avg_precision"]), bits(same["avg_precision"]))
    cpu, cl = D.oracle_index(x, ids, cents)
    assert_curve(got, expected_values(cpu, q, 10, cents, ids, cl), "h.ivf()")
    assert h.ivf().smallest_n_probe(q, 10, 1.0)[0] <= nlist
