"""Bit parity with the oracle at the ends of the f32 and fp16 ranges (data and preconditions: tests/_range_data.py).

The C ABI admits every finite f32, and the distances are promised bit-identical to the reference for all of them.  The
other parity tests draw unit-scale rows; here the rows sit where f32 arithmetic stops being ordinary:

  2^-70, 2^-74, 1e-40   every squared sum of the fold is subnormal, underflows to equal values, or is zero: the kernels
                        must keep subnormals in v_mul/v_add, sqrt and division, and resolve the ties by scan position
  2^62, 2^64            t * t overflows: +Inf is a real distance, counted and ordered by scan position, while every output
                        stage also pads with +Inf and several stages use +Inf as "nothing here"
  a few 2^64 rows among unit-scale ones, fp16 rows beyond 65504
                        the matrix-core proposal sees Inf - Inf = NaN: such a row must survive the filter and be scored
  fp16 subnormals, +-65504 and finite rows that round to +-Inf in storage

Every case first asserts, on the oracle's answer alone, that it is the case it claims to be (R.assert_oracle and its
kin), then compares ids, counts and distance bits.  The oracle never returns NaN for finite input; where a NaN is the
reference's own answer (cosine of overflowing norms, a k-means error over rows holding Inf) both sides are compared with
isnan, since the sign and payload of a NaN are the processor's."""
import ctypes as C
import warnings

import numpy as np
import pytest

import fvdb_import
import oracle as orc
import _range_data as R
from _data import bits

pytestmark = pytest.mark.gpu

N, NLIST, K, NPROBE = 600, 8, 10, 4
DAY = 86400.0
SHAPES = [(20, 16), (128, 32)]  # (d, B): d = 128 with 32 queries is the smallest batch the matrix-core scan takes


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def same(got, ref, what=""):
    gi, gd, gc = got
    oi, od, oc = ref
    assert np.array_equal(gc, oc), f"{what}: hit counts differ: {gc} vs {oc}"
    for b in range(oi.shape[0]):
        n = int(oc[b])
        assert np.array_equal(gi[b, :n], oi[b, :n]), f"{what}: query {b}: ids differ\n{gi[b, :n]}\n{oi[b, :n]}"
        assert np.array_equal(bits(gd[b, :n]), bits(od[b, :n])), \
            f"{what}: query {b}: distances not bit-identical\n{gd[b, :n]}\n{od[b, :n]}"


def triple(r):
    return r.ids, r.distances, r.counts


def same_f32(a, b):
    """Bit equality of two f32 arrays; where the reference's value is NaN the other must be NaN (any sign or payload)."""
    a, b = np.atleast_1d(np.asarray(a, np.float32)), np.atleast_1d(np.asarray(b, np.float32))
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


_ivf_cases = {}


def ivf_case(kind, d, B, nlist=NLIST, nprobe=NPROBE, k=K):
    """Rows, ids, centroids, queries, the oracle over them, the list of every row and the oracle's answer: made once."""
    key = (kind, d, B, nlist, nprobe, k)
    if key not in _ivf_cases:
        x = R.rows(kind, N, d)
        ids = np.arange(N, dtype=np.uint64) * 3 + 1
        cents = x[:nlist].copy()
        q = R.queries(x, B)
        cpu, cl = R.oracle_ivf(x, ids, cents, nprobe)
        _ivf_cases[key] = (x, ids, cents, q, cpu, cl, cpu.batch_search(q, k, nprobe))
    return _ivf_cases[key]


def device_ivf(fv, ctx, x, ids, cents, cl=None, dtype="f32", coarse_mode=None):
    gpu = fv.DeviceIVF(ctx, cents.shape[1], cents.shape[0], dtype=dtype)
    if coarse_mode is not None:
        gpu.set_coarse_mode(coarse_mode)
    gpu.set_centroids(cents)
    if cl is None:
        return gpu, gpu.add(x, ids)
    return gpu, (cl, gpu.add_assigned(x, ids, cl))


def run_modes(gpu, q, k, nprobe, ref, what):
    """AUTO (the matrix-core scan where the shape admits it), the exact scan and the oracle hold together; how many
    queries the filter handed to the exact rescan may be anything."""
    gpu.set_scan_mode(0)
    same(gpu.search(q, k, nprobe), ref, f"{what}, AUTO")
    gpu.set_scan_mode(1)
    same(gpu.search(q, k, nprobe), ref, f"{what}, exact scan")
    gpu.set_scan_mode(0)


def matrix_core_stage_ran(gpu, B):
    """Survivors per query of the last matrix-core batch; the call is refused if no such batch has run on the index."""
    return gpu.scan_survivors(B)


# ---- 1. IVF list scan and selection, f32 rows -----------------------------------------------------------------------------
@pytest.mark.parametrize("coarse_mode", [0, 1], ids=["proposal", "exact_coarse"])
@pytest.mark.parametrize("d,B", SHAPES)
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_ivf_scan_at_the_ends_of_the_f32_range(fv, ctx, kind, d, B, coarse_mode):
    x, ids, cents, q, cpu, cl, ref = ivf_case(kind, d, B)
    R.assert_oracle(ref, R.KINDS[kind][2])
    gpu, (gcl, _) = device_ivf(fv, ctx, x, ids, cents, coarse_mode=coarse_mode)
    assert np.array_equal(gcl, cl), "the device's nearest centroid is not the oracle's"
    run_modes(gpu, q, K, NPROBE, ref, f"{kind} d={d}")
    if d == 128:
        matrix_core_stage_ran(gpu, B)


@pytest.mark.parametrize("n,d,nlist,B", [(600, 20, 8, 16), (600, 128, 8, 32), (12000, 128, 16, 64)])
def test_a_few_huge_rows_among_normal_ones(fv, ctx, n, d, nlist, B):
    # |x|^2 and the fp16 mirror of six rows are Inf, so their matrix-core value is NaN (or +-Inf) for every query, and the
    # last query, a huge row itself, has NaN against every row: NaN has to survive the filter to be scored exactly.  With
    # such a row in the index the largest norm is Inf and the error bound +Inf: the filter kernel runs (at n = 12000 over
    # lists long enough to give a threshold) but passes every row, and the select stage hands the queries to the exact rescan
    x, ids, cents, cl, q, huge = R.mixed_huge_case(n, d, nlist, B)
    cpu, _ = R.oracle_ivf(x, ids, cents, NPROBE, clusters=cl)
    ref = cpu.batch_search(q, K, NPROBE)
    R.assert_mixed_huge_oracle(ref, ids, huge)
    for coarse_mode in (0, 1):
        gpu, _ = device_ivf(fv, ctx, x, ids, cents, cl=cl, coarse_mode=coarse_mode)
        f0 = gpu.scan_fallbacks()
        run_modes(gpu, q, K, NPROBE, ref, f"n={n} d={d} coarse mode {coarse_mode}")
        if d == 128:
            surv = matrix_core_stage_ran(gpu, B)
            print(f"n={n}: {gpu.scan_fallbacks() - f0} of {B} queries rescanned exactly, survivors {surv.tolist()}")
            assert np.all(surv >= K), surv  # no query lost a row it needs: the huge query keeps every row it probes


ROUTE_KINDS = [("huge", "inf_and_finite"), ("tiny", "distinct_subnormal_sums")]


@pytest.mark.parametrize("kind,what", ROUTE_KINDS)
def test_wide_selection_with_inf_on_both_sides_of_the_cut(fv, ctx, kind, what):
    k = 300
    x, ids, cents, q, cpu, cl, ref10 = ivf_case(kind, 20, 16)
    R.assert_oracle(ref10, what)
    ref = cpu.batch_search(q, k, NLIST)
    everything = cpu.batch_search(q, N, NLIST)
    assert np.all(ref[2] == k) and not np.isnan(ref[1]).any()
    if kind == "huge":  # the cut falls inside the +Inf results: more of them lie beyond it than before it ...
        assert np.isposinf(ref[1][:, -1]).all() and np.isfinite(ref[1][:, 0]).all()
        assert np.all(np.isposinf(everything[1]).sum(axis=1) > np.isposinf(ref[1]).sum(axis=1))
    gpu, _ = device_ivf(fv, ctx, x, ids, cents)
    same(gpu.search_wide(q, k, NLIST), ref, f"wide {kind}")
    same(gpu.search_wide(q, K, NPROBE), ref10, f"wide {kind} k=10")


@pytest.mark.parametrize("kind,what", ROUTE_KINDS)
def test_more_than_256_probes(fv, ctx, kind, what):
    # 300 lists of two rows each, all probed: the smallest shape that ranks the centroid table whole (kernels_rank.h)
    nlist = 300
    x = R.rows(kind, N, 20)
    ids = np.arange(N, dtype=np.uint64) * 3 + 1
    cents, q = x[:nlist].copy(), R.queries(x, 16)
    cl = (np.arange(N) % nlist).astype(np.uint32)
    cpu, _ = R.oracle_ivf(x, ids, cents, nlist, clusters=cl)
    ref = cpu.batch_search(q, K, nlist)
    R.assert_oracle(ref, what)
    gpu, _ = device_ivf(fv, ctx, x, ids, cents, cl=cl)
    same(gpu.search(q, K, nlist), ref, f"nprobe=300 {kind}")
    ref257 = cpu.batch_search(q, K, 257)
    assert np.all(ref257[2] == K) and not np.isnan(ref257[1]).any()
    same(gpu.search(q, K, 257), ref257, f"nprobe=257 {kind}")


@pytest.mark.parametrize("kind,what", ROUTE_KINDS)
def test_search_all(fv, ctx, kind, what):
    x, ids, cents, q, cpu, cl, _ = ivf_case(kind, 20, 16)
    ref = R.list_order_search(x, ids, cl, q, K)  # the scan in list order, not in probe order: ties fall differently
    R.assert_oracle(ref, what)
    gpu, _ = device_ivf(fv, ctx, x, ids, cents)
    same(gpu.search_all(q, K), ref, f"search_all {kind}")


@pytest.mark.parametrize("kind,what", ROUTE_KINDS)
def test_masked_search_admitting_every_other_row(fv, ctx, kind, what):
    x, ids, cents, q, _, _, _ = ivf_case(kind, 20, 16)
    cpu, _ = R.oracle_ivf(x, ids, cents)
    for i in ids[1::2]:
        cpu.mark_deleted(int(i))
    ref = cpu.batch_search(q, K, NPROBE)
    R.assert_oracle(ref, what)
    g = fv.IVFIndex(ctx, n_clusters=NLIST, n_probe=NPROBE)
    g.set_trained(cents)
    assert g.batch_insert(ids, x) == (N, 0)
    for mode in (1, 2, 0):  # exact scan, the filter forced, AUTO
        ctx.check(ctx.lib.fvdb_ivf_set_scan_mode(g._dev(), mode))
        same(triple(g.search_allowed(q, K, ids[::2], NPROBE)), ref, f"masked {kind} scan mode {mode}")


@pytest.mark.parametrize("d,B", SHAPES)
def test_deleted_rows_at_inf_and_at_zero(fv, ctx, d, B):
    x, ids, cents, q, _, cl, ref = ivf_case("huge", d, B)
    q = q.copy()
    q[0] = x[0]  # a query that is a stored row: distance 0.0
    cpu, _ = R.oracle_ivf(x, ids, cents)
    before = cpu.batch_search(q, K, NPROBE)
    R.assert_oracle(before, "inf_and_finite")
    assert before[0][0, 0] == ids[0] and before[1][0, 0] == 0.0
    b_inf = int(np.flatnonzero(np.isposinf(before[1]).any(axis=1))[0])
    at_inf = int(before[0][b_inf][np.isposinf(before[1][b_inf])][0])  # the first +Inf result of some query
    dead = [int(ids[0]), at_inf]
    for i in dead:
        cpu.mark_deleted(i)
    ref = cpu.batch_search(q, K, NPROBE)
    R.assert_oracle(ref, "inf_and_finite")
    assert not np.isin(ref[0], dead).any()
    gpu, (gcl, pos) = device_ivf(fv, ctx, x, ids, cents)
    same(gpu.search(q, K, NPROBE), before, "before the deletes")
    rows = [(i - 1) // 3 for i in dead]
    gpu.set_deleted(gcl[rows], pos[rows], True)
    run_modes(gpu, q, K, NPROBE, ref, f"after the deletes d={d}")


def oracle_coarse(q, cents, nprobe):
    cl = np.empty((q.shape[0], nprobe), np.uint32)
    ds = np.empty((q.shape[0], nprobe), np.float32)
    for i in range(q.shape[0]):
        dist = orc.l2_batch(q[i], cents)
        order = np.argsort(dist, kind="stable")[:nprobe]  # stable: the lowest cluster id wins a tie
        cl[i], ds[i] = order, dist[order]
    return cl, ds


@pytest.mark.parametrize("d,B", SHAPES)
@pytest.mark.parametrize("nlist,nprobe", [(8, 4), (80, 16)])  # the matrix cores propose from 64 lists on (and d % 16 == 0)
@pytest.mark.parametrize("kind", ["huge", "tiny"])
def test_coarse_ranking(fv, ctx, kind, nlist, nprobe, d, B):
    x = R.rows(kind, N, d)
    cents, q = x[:nlist].copy(), R.queries(x, B)
    ocl, ods = oracle_coarse(q, cents, nprobe)
    assert not np.isnan(ods).any()
    if kind == "huge":  # +Inf coarse distances, tied, in cluster order
        tied = np.isposinf(ods)
        assert tied.any() and np.isfinite(ods).any()
        assert all(np.all(np.diff(ocl[b][tied[b]].astype(np.int64)) > 0) for b in range(B))
    else:
        assert np.all(ods > 0) and np.all(ods < np.float32(2.0 ** -63))
    for mode in (0, 1):
        gpu = fv.DeviceIVF(ctx, d, nlist)
        gpu.set_coarse_mode(mode)
        gpu.set_centroids(cents)
        gcl, gds = gpu.coarse(q, nprobe)
        assert np.array_equal(gcl, ocl), f"coarse mode {mode}: centroid order differs"
        assert np.array_equal(bits(gds), bits(ods)), f"coarse mode {mode}: distances not bit-identical"


@pytest.mark.parametrize("d,B", SHAPES)
@pytest.mark.parametrize("kind,what", ROUTE_KINDS)
def test_lists_sharded_over_8_emulated_gpus(fv, ctx, kind, what, d, B):
    G, nlist = 8, 16
    x, ids, cents, q, cpu, cl, ref = ivf_case(kind, d, B, nlist=nlist)
    R.assert_oracle(ref, what)
    sizes = np.bincount(cl, minlength=nlist).astype(np.uint64)
    owner = fv.sharded.plan_list_shards(sizes, G)
    qd = ctx.upload(q)
    keys_all, ids_all = ctx.alloc(G * B * K * 8), ctx.alloc(G * B * K * 8)
    scratch_d, scratch_c = ctx.alloc(B * K * 4), ctx.alloc(B * 4)
    oi, od, oc = ctx.alloc(B * K * 8), ctx.alloc(B * K * 4), ctx.alloc(B * 4)
    shards = []
    try:
        for g in range(G):
            sh = fv.DeviceIVF(ctx, d, nlist)
            sh.set_centroids(cents)
            mine = owner[cl] == g
            if mine.any():
                sh.add_assigned(x[mine], ids[mine], cl[mine])
            sh.set_global_list_sizes(sizes)
            shards.append(sh)
            off = g * B * K * 8
            sh.search_dev(qd, B, K, NPROBE, C.c_void_p(ids_all.value + off), scratch_d, scratch_c,
                          C.c_void_p(keys_all.value + off))
        fv.engine.merge_keys_dev(ctx, keys_all, ids_all, G, B, K, oi, od, oc)
        ctx.synchronize()
        got = (ctx.download(oi, (B, K), np.uint64), ctx.download(od, (B, K), np.float32), ctx.download(oc, B, np.uint32))
    finally:
        for p in (qd, keys_all, ids_all, scratch_d, scratch_c, oi, od, oc):
            ctx.free(p)
    same(got, ref, f"8 shards {kind} d={d}")


@pytest.mark.parametrize("kind,what", ROUTE_KINDS)
def test_host_mirror_ivf_index(fv, ctx, kind, what):
    x, ids, cents, q, _, _, ref = ivf_case(kind, 20, 16)
    R.assert_oracle(ref, what)
    g = fv.IVFIndex(ctx, n_clusters=NLIST, n_probe=NPROBE)
    g.set_trained(cents)
    assert g.batch_insert(ids, x) == (N, 0)
    same(triple(g.search(q, K, NPROBE)), ref, f"IVFIndex {kind}")


@pytest.mark.parametrize("kind", ["huge", "tiny"])
def test_host_mirror_hybrid_index(fv, ctx, kind):
    n, d, B, now = 300, 20, 16, 1000 * DAY
    x = R.rows(kind, n, d)
    cents, q = x[:NLIST].copy(), R.queries(x, B)
    recent = np.arange(n) % 3 == 0  # rows in both parts
    levels = orc.rng_levels(3, n)
    kw = dict(max_connections=6, max_connections_layer_0=12, ef_construction=40, n_clusters=NLIST, n_probe=NPROBE)
    g, o = fv.HybridIndex(ctx, **kw), orc.HybridIndex(**kw)
    g.set_ivf_centroids(cents)
    o.set_ivf_centroids(cents)
    for i in range(n):
        ts = now - (1 if recent[i] else 30) * DAY
        g.insert_with_timestamp(i, x[i], ts, now, int(levels[i]))
        o.insert_with_timestamp(i, x[i], ts, now, int(levels[i]))
    assert o.recent_count() == int(recent.sum()) and o.historical_count() == n - int(recent.sum())
    assert (g.recent_count(), g.historical_count()) == (o.recent_count(), o.historical_count())
    ref = o.batch_search(q, K, now=now, hnsw_ef=50, ivf_n_probe=NPROBE)
    R.assert_oracle(ref, "inf_and_finite" if kind == "huge" else "distinct_subnormal_sums")
    in_recent = np.isin(ref[0], np.flatnonzero(recent).astype(np.uint64))
    assert in_recent.any() and (~in_recent).any(), "results from both parts"
    same(triple(g.search(q, K, now=now, hnsw_ef=50, ivf_n_probe=NPROBE)), ref, f"HybridIndex {kind}")


# ---- 2. fp16 rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,B", [(20, 32), (128, 32)])  # fp16 rows are padded to 32 dimensions: both shapes take the filter
@pytest.mark.parametrize("kind,what", [("f16_subnormal", "distinct"), ("f16_max", "distinct"), ("f16_overflow", "distinct")])
def test_fp16_rows_at_the_ends_of_the_fp16_range(fv, ctx, kind, what, d, B):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # numpy says "overflow in cast" where a row rounds to Inf
        x, r = R.f16_case(kind, N, d)
    ids = np.arange(N, dtype=np.uint64) * 3 + 1
    cents, q = x[:NLIST].copy(), R.queries(x, B)
    cpu, cl = R.oracle_ivf(x, ids, cents, stored=r)  # lists by the f32 rows, contents as stored
    ref = cpu.batch_search(q, K, NPROBE)
    R.assert_oracle(ref, what)
    # every probed row, so that the rows at +Inf are results too, ordered by scan position
    everything = cpu.batch_search(q, N, NLIST)
    assert np.all(everything[2] == N) and not np.isnan(everything[1]).any()
    if kind == "f16_overflow":
        assert np.all(np.isposinf(everything[1]).sum(axis=1) == np.isinf(r).any(axis=1).sum())
    gpu, (gcl, pos) = device_ivf(fv, ctx, x, ids, cents, dtype="f16")
    assert np.array_equal(gcl, cl)
    run_modes(gpu, q, K, NPROBE, ref, f"{kind} d={d}")
    matrix_core_stage_ran(gpu, B)
    # every row comes back as stored: subnormals kept, 65519 as 65504, +-65520 and 70000 as +-Inf
    assert np.array_equal(bits(gpu.get_rows(cl, pos)), bits(r))
    same(gpu.search_wide(q, N, NLIST), everything, f"{kind} d={d}, every row")


def test_fp16_rows_at_inf_among_the_ten_nearest(fv, ctx):
    # a list of four finite rows and 24 rows holding +-Inf, probed alone: six of the ten nearest are at +Inf, and for the
    # matrix cores those rows are NaN or +Inf
    d, B = 20, 32
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        x, r, ids, cents, cl, q = R.f16_short_list_case(d, B)
    cpu, _ = R.oracle_ivf(x, ids, cents, 1, clusters=cl, stored=r)
    ref = cpu.batch_search(q, K, 1)
    R.assert_f16_short_list_oracle(ref)
    for coarse_mode in (0, 1):
        gpu, _ = device_ivf(fv, ctx, x, ids, cents, cl=cl, dtype="f16", coarse_mode=coarse_mode)
        run_modes(gpu, q, K, 1, ref, f"coarse mode {coarse_mode}")
        matrix_core_stage_ran(gpu, B)


def test_fp16_rows_beyond_the_range_through_maintenance(fv, ctx):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        x, r = R.f16_case("f16_overflow", N, 20)
    ids = np.arange(N, dtype=np.uint64) + 5
    old, new = NLIST, 6
    cents, q = x[:old].copy(), R.queries(x, 16)
    _, cl = R.oracle_ivf(x, ids, cents, stored=r)
    order = np.concatenate([np.flatnonzero(cl == c) for c in range(old)])  # sequence order
    # vacuum: a row holding +Inf and a finite row leave; the rest answer as the oracle over the rest
    dead = [40, 100]
    assert np.isinf(r[40]).any() and np.isfinite(r[100]).all()
    keep = order[~np.isin(order, dead)]
    cpu, _ = R.oracle_ivf(x[keep], ids[keep], cents, stored=r[keep])
    ref = cpu.batch_search(q, N, old)
    assert np.all(ref[2] == N - 2) and not np.isnan(R.live(ref)).any() and np.isposinf(R.live(ref)).any()
    # train_from: k-means over rows that hold +-Inf.  The oracle's run is the expected answer: its first error is +Inf,
    # its last NaN (Inf - Inf), it stops after one iteration, and its centroids hold Inf but no NaN
    o = orc.IVFIndex(n_clusters=new, n_probe=new, max_iterations=10, seed=5)
    ores = o.train(r[keep])
    oc = o.get_centroids()
    assert np.isposinf(ores["initial_error"]) and np.isnan(ores["final_error"]) and ores["iterations"] == 1
    assert not np.isnan(oc).any() and np.isinf(oc).any()

    src, (gcl, pos) = device_ivf(fv, ctx, x, ids, cents, dtype="f16")
    assert np.array_equal(gcl, cl)
    for c in range(old):
        rows_c, lid, _ = src.list_export(c)
        assert np.array_equal(lid, ids[cl == c]) and np.array_equal(bits(rows_c), bits(r[cl == c]))
    src.set_deleted(cl[dead], pos[dead])
    removed, kept = src.compact()
    assert removed == 2 and np.array_equal(kept, ids[keep])
    same(src.search_wide(q, N, old), ref, "after the vacuum")
    dst = fv.DeviceIVF(ctx, 20, new, dtype="f16")
    res = dst.train_from(src, max_iterations=10, seed=5)
    assert (res["iterations"], res["converged"]) == (ores["iterations"], ores["converged"]), (res, ores)
    assert same_f32(res["initial_error"], ores["initial_error"]) and same_f32(res["final_error"], ores["final_error"]), (res, ores)
    assert np.array_equal(bits(dst.get_centroids()), bits(oc))


def test_rows_by_id_at_the_ends_of_the_ranges(fv, ctx):
    # the gathers move bits: fp16 rows come back widened (+-Inf where the f32 row was beyond the range), f32 rows of the
    # index come back as they went in, subnormal and 2^64-scale ones included
    x = (R.base(60, 20) * np.float32(100)).astype(np.float32)
    x[7, 3], x[8, 0], x[9, 5] = 65520.0, -65520.0, 70000.0
    x[10], x[11] = R.rows("subnormal_rows", 60, 20)[10], R.rows("over", 60, 20)[11]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        r = R.f16_rounded(x)
    assert np.isposinf(r[7, 3]) and np.isneginf(r[8, 0]) and np.isposinf(r[9, 5]) and np.isfinite(x).all()
    assert np.all(np.abs(x[10]) < np.float32(2.0 ** -126)) and np.any(x[10] != 0) and np.all(np.abs(x[11]) > np.float32(2.0 ** 55))
    ids = np.arange(60, dtype=np.uint64) + 100
    gpu, (cl, pos) = device_ivf(fv, ctx, x, ids, x[:4].copy(), dtype="f16")
    assert np.array_equal(bits(gpu.get_rows(cl, pos)), bits(r))
    g = fv.IVFIndex(ctx, n_clusters=4, n_probe=4)
    g.set_trained(x[:4].copy())
    assert g.batch_insert(ids, x) == (60, 0)
    rows_by_id, found = g.get_vectors(ids)
    assert found.all() and np.array_equal(bits(rows_by_id), bits(x))


# ---- 3. HNSW --------------------------------------------------------------------------------------------------------------
HN, M, M0, EFC, NQ, EF = 240, 6, 12, 40, 25, 50
HNSW_KINDS = {"tiny": "distinct_subnormal_sums", "huge": "inf_and_finite", "over": "mostly_inf", "subnormal_rows": "all_zero"}
_hnsw_cases = {}


def hnsw_case(kind, d):
    if (kind, d) not in _hnsw_cases:
        x = R.rows(kind, HN, d)
        ids = np.arange(HN, dtype=np.uint64) + 7
        levels = orc.rng_levels(d, HN)
        oh = orc.HNSWIndex(M, M0, EFC, seed=d)
        oh.batch_insert(ids, x, levels)
        q = R.queries(x, NQ)
        _hnsw_cases[(kind, d)] = (x, ids, levels, q, oh, oh.batch_search(q, K, EF))
    return _hnsw_cases[(kind, d)]


def same_graph(gh, oh):
    assert gh.entry_point() == oh.entry_point()
    gi, lv, off, nb = gh.export_graph()
    slot = 0
    for r, l in zip(gi.tolist(), lv.tolist()):
        assert l == oh.level(r)
        for layer in range(l + 1):
            assert nb[int(off[slot]):int(off[slot + 1])].tolist() == oh.neighbors(r, layer), (r, layer)
            slot += 1


def same_results(got, want):
    assert np.array_equal(got.counts, want[2]) and np.array_equal(got.ids, want[0])
    assert np.array_equal(bits(got.distances), bits(want[1]))


def hnsw_parity(fv, ctx, kind, d, mode, visited=None):
    x, ids, levels, q, oh, want = hnsw_case(kind, d)
    R.assert_oracle(want, HNSW_KINDS[kind])
    gh = fv.HNSWIndex(ctx, M, M0, EFC, seed=d)
    gh.set_device_insert(True, mode)
    if visited:
        gh.set_insert_visited(visited)
    ok, bad = gh.batch_insert(ids, x, levels)
    assert (ok, bad) == (HN, 0)
    st = gh.insert_stats()
    assert st["host_path_inserts"] == 0
    if visited == "hashed":
        assert st["hashed_inserts"] > 0
    same_graph(gh, oh)
    again = gh.tie_restarts()[1]
    gh.set_device_traversal(True)
    same_results(gh.search(q, K, EF), want)
    if kind == "huge":  # many heap entries equal at +Inf: the register form hands over to the restated heaps
        assert gh.tie_restarts()[1] > again, "no query was searched again with the restated heaps"
    gh.set_device_traversal(False)
    same_results(gh.search(q, K, EF), want)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("d", [20, 128])
@pytest.mark.parametrize("kind", list(HNSW_KINDS))
def test_hnsw_insert_and_traversal_at_the_ends_of_the_f32_range(fv, ctx, kind, d, mode):
    hnsw_parity(fv, ctx, kind, d, mode)


@pytest.mark.parametrize("kind", ["tiny", "huge"])
def test_hnsw_insert_with_the_hashed_visited_set(fv, ctx, kind):
    hnsw_parity(fv, ctx, kind, 20, 1, visited="hashed")


# ---- 4. k-means training ------------------------------------------------------------------------------------------------------
# What the oracle does at each scale (n = 600, d = 20, max_iterations = 10, seed = 5) is the expected answer:
#   2^-70, 4 lists    errors 3.18e-41 -> 1.28e-41 (subnormal), all 10 iterations, not converged
#   2^-70, 80 lists   errors 3.18e-41 -> 7.94e-42, converged after 7 iterations
#   1e-40 rows        every distance is 0.0: both errors 0.0, converged after 1 iteration, two distinct centroids (the
#                     first pick, and the mean of all rows: subnormal sums divided by the count)
#   2^62              both errors +Inf; 4 lists run 10 iterations, 80 lists converge after 8
TRAINING = [("tiny", 4, 10, False), ("tiny", 80, 7, True), ("subnormal_rows", 4, 1, True), ("subnormal_rows", 80, 1, True),
            ("huge", 4, 10, False), ("huge", 80, 8, True)]


@pytest.mark.parametrize("kind,nlist,iterations,converged", TRAINING)
def test_kmeans_training_at_the_ends_of_the_f32_range(fv, ctx, kind, nlist, iterations, converged):
    x = R.rows(kind, N, 20)
    o = orc.IVFIndex(n_clusters=nlist, n_probe=1, max_iterations=10, seed=5)
    ro = o.train(x)
    oc = o.get_centroids()
    assert (ro["iterations"], ro["converged"]) == (iterations, converged), ro
    e0, e1 = np.float32(ro["initial_error"]), np.float32(ro["final_error"])
    assert not np.isnan([e0, e1]).any() and np.isfinite(oc).all()
    if kind == "tiny":
        assert 0 < e1 < e0 < np.float32(2.0 ** -126)
    elif kind == "huge":
        assert np.isposinf(e0) and np.isposinf(e1)
    else:
        assert e0 == 0 and e1 == 0 and np.all(np.abs(oc) < np.float32(2.0 ** -126)) and np.any(oc != 0)
    g = fv.DeviceIVF(ctx, 20, nlist)
    rg = g.train(x, max_iterations=10, seed=5)
    assert (rg["iterations"], rg["converged"]) == (ro["iterations"], ro["converged"]), (rg, ro)
    for key in ("initial_error", "final_error"):
        assert bits(np.float32(rg[key])) == bits(np.float32(ro[key])), (key, rg, ro)
    differ = np.flatnonzero((bits(g.get_centroids()) != bits(oc)).any(axis=1))
    assert differ.size == 0, f"centroids {differ.tolist()} are not bit-equal"
    assert np.array_equal(g.assign(x), o.assign(x))


# ---- 5. utilities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [8, 96, 257])
def test_dot_and_cosine_with_subnormal_and_overflowing_norms(fv, ctx, size):
    pairs = R.cosine_pairs(size)
    for name, a, b, what in pairs:
        c = np.float32(orc.cosine_similarity_scalar(a, b))
        if what == "one":        # norm product and divisor subnormal, the quotient exact
            assert c == 1.0 and 0 < np.float32(orc.dot_product_scalar(a, b)) < np.float32(2.0 ** -126), name
        elif what == "near_one":  # the rounding of the two roots shows: within two ulps of 1 (1.0000001 at 8 dimensions)
            assert abs(float(c) - 1.0) <= 2.0 ** -22 and (size != 8 or c == np.nextafter(np.float32(1), np.float32(2))), name
        elif what == "zero":     # |a|^2 underflows to 0: the reference returns 0.0 for a zero norm
            assert bits(c) == 0, name
        else:                    # Inf / Inf: the reference's answer is NaN, and the engine returns it (it refuses non-finite
            assert np.isnan(c), name  # INPUT only), so both sides are compared with isnan
    qa = np.stack([p[1] for p in pairs])
    xb = np.stack([p[2] for p in pairs])
    with np.errstate(all="ignore"):
        want_dot = np.array([[orc.dot_product_scalar(a, b) for b in xb] for a in qa], np.float32)
    want_cos = np.array([[orc.cosine_similarity_scalar(a, b) for b in xb] for a in qa], np.float32)
    assert not np.isnan(want_dot).any() and np.isnan(want_cos).sum() > 0
    got_dot, got_cos = fv.dot_products(ctx, qa, xb), fv.batch_cosine_similarity(ctx, qa, xb)
    assert same_f32(got_dot, want_dot), f"dot products\n{got_dot}\n{want_dot}"
    assert same_f32(got_cos, want_cos), f"cosines\n{got_cos}\n{want_cos}"


def test_edge_scores_order_is_the_oracles():
    assert orc.top_k_indices(R.EDGE_SCORES, 7) == R.EDGE_ORDER


KS = [3, 7, 63, 64, 65, 255, 256]  # both sides of 64 and up to FVDB_MAX_K = 256; 257 is refused


@pytest.mark.parametrize("n", [7, 65, 300])
def test_top_k_on_signed_zeros_infinities_and_the_extremes(fv, ctx, n):
    s = np.stack([R.edge_scores(n, seed) for seed in (n, n + 1, n + 2)])
    assert orc.top_k_indices(s[0][:7], 7) == R.EDGE_ORDER
    present = set(bits(s).ravel().tolist())
    assert present == set(bits(R.EDGE_SCORES).tolist()) and (n == 7 or all((bits(s) == v).sum() > 3 for v in present))
    for k in KS:
        got_sort, got_heap = fv.top_k_indices(ctx, s, k), fv.top_k_indices_heap(ctx, s, k)
        for b in range(s.shape[0]):
            assert got_sort[b] == orc.top_k_indices(s[b], k), (n, k, b)
            assert got_heap[b] == orc.top_k_indices_heap(s[b], k), (n, k, b)
    with pytest.raises(fv.Unsupported):
        fv.top_k_indices(ctx, s, 257)


@pytest.mark.parametrize("n", [7, 65, 300])
def test_streaming_top_k_and_merge_on_the_same_scores(fv, ctx, n):
    rng = np.random.default_rng(n)
    s = np.stack([R.edge_scores(n, seed) for seed in (n, n + 1)])
    ids = np.stack([rng.permutation(10 * n)[:n], rng.integers(0, n // 2 + 2, n)]).astype(np.uint64)  # row 1: ids repeat
    for k in KS:
        got = fv.streaming_top_k(ctx, ids, s, k)
        for b in range(2):
            want = orc.streaming_top_k(ids[b], s[b], k)
            assert len(want) == min(k, n)
            assert [g[0] for g in got[b]] == [w[0] for w in want], (n, k, b)
            assert np.array_equal(bits(np.asarray([g[1] for g in got[b]], np.float32)),
                                  bits(np.asarray([w[1] for w in want], np.float32))), (n, k, b)
        # the same pairs as result sets of 5: each id keeps its smallest "distance" (-Inf, -0.0 and 0.0 among them)
        for b in range(2):
            sets = [[(int(ids[b, i]), float(s[b, i])) for i in range(j, min(j + 5, n))] for j in range(0, n, 5)]
            want = orc.merge_search_results(sets, k)
            got_m = fv.merge_search_results(ctx, sets, k)
            assert len(want) > 0
            assert [g[0] for g in got_m] == [w[0] for w in want], (n, k, b)
            assert np.array_equal(bits(np.asarray([g[1] for g in got_m], np.float32)),
                                  bits(np.asarray([w[1] for w in want], np.float32))), (n, k, b)
