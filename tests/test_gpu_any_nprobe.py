"""IVF search at any nprobe: above 256 probed lists the centroid table is ranked whole on the
device and the lists go through the wide selection; evaluate_search_quality measures a configured n_probe against the
search of every list.

The result is the one search_with_config defines for any n_probe, so the oracle is the checker and every comparison is
bit for bit: ids, distance bits and counts."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
import _any_nprobe_data as D
from _data import bits, mixture

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = 12
NO_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_LIST = np.uint32(0xFFFFFFFF)
DAY = 86400.0
NLIST = D.NLIST


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def assert_same(gpu_res, cpu_res, what=""):
    gi, gd, gc = gpu_res
    ci, cd, cc = cpu_res
    assert np.array_equal(gc, cc), f"{what}: hit counts differ: {gc[:8]} vs {cc[:8]}"
    for q in range(gi.shape[0]):
        n = int(cc[q])
        assert np.array_equal(gi[q, :n], ci[q, :n]), f"{what}: query {q}: ids differ"
        assert np.array_equal(bits(gd[q, :n]), bits(cd[q, :n])), f"{what}: query {q}: distances not bit-identical"
        assert np.all(gi[q, n:] == NO_ID) and np.all(np.isposinf(gd[q, n:])), f"{what}: query {q}: tail not padded"


def same_as_oracle(g, ref):
    oi, od, oc = ref
    assert np.array_equal(g.counts, oc), f"hit counts differ: {g.counts[:8]} vs {oc[:8]}"
    for b in range(len(g)):
        n = int(oc[b])
        assert np.array_equal(g.ids[b, :n], oi[b, :n]), f"query {b}: ids differ"
        assert np.array_equal(bits(g.distances[b, :n]), bits(od[b, :n])), f"query {b}: distances not bit-identical"


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


class DevBufs:
    """Device-pointer calls: the batch and one block of outputs (ids, distances, counts, keys) in HBM."""

    def __init__(self, ctx, q, k):
        q = np.ascontiguousarray(q, np.float32)
        self.ctx, self.B, self.k = ctx, q.shape[0], k
        self.q = ctx.upload(q)
        n = self.B * k
        self.out = ctx.alloc(n * 20 + self.B * 4)
        at = lambda off: C.c_void_p(self.out.value + off)  # noqa: E731
        self.ids, self.keys, self.dist, self.cnt = at(0), at(n * 8), at(n * 16), at(n * 20)

    def args(self):
        return self.ids, self.dist, self.cnt, self.keys

    def read(self):
        B, k = self.B, self.k
        return (self.ctx.download(self.ids, (B, k), np.uint64), self.ctx.download(self.dist, (B, k), np.float32),
                self.ctx.download(self.cnt, B, np.uint32), self.ctx.download(self.keys, (B, k), np.uint64))

    def free(self):
        self.ctx.free(self.q)
        self.ctx.free(self.out)


def coarse_dev(ctx, gpu, q, nprobe):
    """fvdb_ivf_coarse_dev_slot: [B][min(nprobe, nlist)] cluster ids in probe order."""
    q = np.ascontiguousarray(q, np.float32)
    B, np_ = q.shape[0], min(nprobe, gpu.nlist)
    q_dev, out = ctx.upload(q), ctx.alloc(B * np_ * 4)
    try:
        ctx.check(ctx.lib.fvdb_ivf_coarse_dev_slot(gpu.h, None, 0, q_dev, B, nprobe, out))
        ctx.synchronize()
        return ctx.download(out, (B, np_), np.uint32)
    finally:
        ctx.free(q_dev)
        ctx.free(out)


# ---- 1. the main case --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("d", [20, 64])
def test_any_nprobe_equals_the_oracle(fv, ctx, d, dtype):
    # 300 lists: five centroid blocks, the last partial; d = 20 is padded (to 32 for fp16 rows)
    x, ids, cents = D.main_case(d, seed=4000 + d)
    gpu, cpu, _, _ = build_pair(fv, ctx, x, ids, cents, dtype=dtype)
    for B in (1, 33):
        q = mixture(B, d, n_comp=40, seed=4001 + d + B)
        for nprobe in (257, 299, 300, 1000):
            for k in (10, 300):
                got = gpu.search(q, k, nprobe)
                assert_same(got, cpu.batch_search(q, k, nprobe, threads=8), f"d={d} {dtype} B={B} nprobe={nprobe} k={k}")
                assert_same(gpu.search_wide(q, k, nprobe), got, f"wide entry d={d} {dtype} B={B} nprobe={nprobe} k={k}")


# ---- 2. continuity at the threshold ---------------------------------------------------------------------------------------
def test_ranking_continues_the_register_path(fv, ctx):
    d = 64
    x, ids, cents = D.main_case(d, seed=4010)
    gpu, cpu, _, _ = build_pair(fv, ctx, x, ids, cents)
    q = mixture(33, d, n_comp=40, seed=4011)
    gpu.set_coarse_mode(1)  # FVDB_COARSE_EXACT: every centroid scored by the register path
    cl256, ds256 = gpu.coarse(q, 256)
    full = coarse_dev(ctx, gpu, q, 300)
    assert full.shape == (33, NLIST)
    assert np.array_equal(full[:, :256], cl256), "the first 256 of the full ranking are the register path's 256"
    assert np.array_equal(np.sort(full, axis=1), np.tile(np.arange(NLIST, dtype=np.uint32), (33, 1))), "a permutation"
    for nprobe in (257, 300):
        cl, ds = gpu.coarse(q, nprobe)
        assert np.array_equal(cl, full[:, :nprobe])
        assert np.array_equal(bits(ds[:, :256]), bits(ds256)), "centroid distances are bit-equal"
        assert np.all(ds[:, 1:] >= ds[:, :-1])
    want = orc.l2_batch(q[0], cents)
    cl, ds = gpu.coarse(q[:1], 300)
    assert np.array_equal(bits(ds[0]), bits(want[cl[0]]))
    assert np.array_equal(cl[0], np.argsort(want, kind="stable").astype(np.uint32)), "the reference's stable sort"
    gpu.set_coarse_mode(0)
    for nprobe in (256, 257):
        for k in (10, 256):
            assert_same(gpu.search(q, k, nprobe), cpu.batch_search(q, k, nprobe, threads=8), f"nprobe={nprobe} k={k}")


# ---- 3. ties the ranking decides ------------------------------------------------------------------------------------------
def test_ties_break_by_probe_rank_and_cluster_position(fv, ctx):
    x, ids, cents, cl, q = D.tie_case()
    gpu, cpu, _, _ = build_pair(fv, ctx, x, ids, cents, clusters=cl)
    # identical centroids tie in the coarse order: the lower cluster position first
    full = coarse_dev(ctx, gpu, q, NLIST)
    for b in range(q.shape[0]):
        assert np.array_equal(full[b], np.argsort(orc.l2_batch(q[b], cents), kind="stable").astype(np.uint32))
    assert full[0, 0] == 10 and full[0, 1] == 200 and full[1, 0] == 37 and full[1, 1] == 150
    for nprobe in (257, 299, NLIST):
        for k in (10, 300):
            assert_same(gpu.search(q, k, nprobe), cpu.batch_search(q, k, nprobe), f"nprobe={nprobe} k={k}")
    # the case decides: a scan in list-index order keeps other rows among the equals (test_any_nprobe_symbols.py holds
    # the same against the oracle alone), and so does fvdb_ivf_search_all
    k = 10
    got = gpu.search(q, k, NLIST)
    by_list = D.list_order_answer(x, ids, cl, q, k)
    assert any(not np.array_equal(got[0][b], by_list[b]) for b in range(q.shape[0]))
    assert np.array_equal(gpu.search_all(q, k)[0], by_list)


# ---- 4. empty lists and deleted rows --------------------------------------------------------------------------------------
def test_empty_lists_among_the_probes_and_deleted_rows(fv, ctx):
    x, ids, cents, q = D.quality_case()
    gpu, cpu, cl, pos = build_pair(fv, ctx, x, ids, cents)
    assert np.all(gpu.list_sizes()[280:] == 0)
    dead = np.arange(0, x.shape[0], 10)
    gpu.set_deleted(cl[dead], pos[dead], True)
    for i in ids[dead]:
        cpu.mark_deleted(int(i))
    for nprobe in (257, NLIST):
        for k in (10, 300):
            res = gpu.search(q, k, nprobe)
            assert_same(res, cpu.batch_search(q, k, nprobe), f"nprobe={nprobe} k={k}")
            assert not np.isin(res[0], ids[dead]).any()
    # k above the live rows: every one of them, then padding
    res = gpu.search(q[:3], 4096, NLIST)
    assert_same(res, cpu.batch_search(q[:3], 4096, NLIST), "k=4096")
    assert np.all(res[2] == x.shape[0] - dead.size)


# ---- 5. mask ----------------------------------------------------------------------------------------------------------------
def test_masked_search_at_nprobe_300_equals_the_oracle_after_deleting_the_complement(fv, ctx):
    x, ids, cents, q = D.quality_case()
    g = fv.IVFIndex(ctx, n_clusters=NLIST, n_probe=NLIST)
    g.set_trained(cents)
    g.batch_insert(ids, x)
    rng = np.random.default_rng(43)
    allowed = ids[rng.random(ids.size) < 0.3]
    o, _ = D.oracle_index(x, ids, cents)
    keep = set(int(i) for i in allowed)
    for i in ids:
        if int(i) not in keep:
            o.mark_deleted(int(i))
    for k in (10, 300):
        same_as_oracle(g.search_allowed(q, k, allowed, NLIST), o.batch_search(q, k, NLIST))
    same_as_oracle(g.search_allowed(q, 10, allowed, 257), o.batch_search(q, 10, 257))


# ---- 6. a sort beyond kWideMaxK -------------------------------------------------------------------------------------------
def test_ranking_of_4100_lists(fv, ctx):
    # 65 centroid blocks: 4160 keys padded to 8192 (64 KiB of LDS), more than the wide selection ever sorts
    nlist, d, n, B = 4100, 16, 8200, 4
    x = mixture(n, d, n_comp=64, seed=4300)
    ids = np.arange(n, dtype=np.uint64) + 9
    gpu, cpu, _, _ = build_pair(fv, ctx, x, ids, x[:nlist].copy())
    q = mixture(B, d, n_comp=64, seed=4301)
    assert_same(gpu.search(q, 10, nlist), cpu.batch_search(q, 10, nlist, threads=4), "nprobe=4100")
    cl, ds = gpu.coarse(q, nlist)
    for b in range(B):
        want = orc.l2_batch(q[b], x[:nlist])
        assert np.array_equal(cl[b], np.argsort(want, kind="stable").astype(np.uint32))
        assert np.array_equal(bits(ds[b]), bits(want[cl[b]]))


def test_ranking_of_16384_lists_the_supported_maximum(fv, ctx):
    # centroids only: 256 blocks, 16384 keys in 128 KiB of dynamic LDS, 1024 threads — the largest sort served
    nlist, d, B = 16384, 4, 3
    cents = np.random.default_rng(6).standard_normal((nlist, d)).astype(np.float32)
    gpu = fv.DeviceIVF(ctx, d, nlist)
    gpu.set_centroids(cents)
    q = np.random.default_rng(7).standard_normal((B, d)).astype(np.float32)
    cl, ds = gpu.coarse(q, nlist)
    head = coarse_dev(ctx, gpu, q, 300)
    for b in range(B):
        want = orc.l2_batch(q[b], cents)
        order = np.argsort(want, kind="stable").astype(np.uint32)
        assert np.array_equal(cl[b], order)
        assert np.array_equal(bits(ds[b]), bits(want[order]))
        assert np.array_equal(head[b], order[:300])
    assert gpu.search(q, 10, nlist)[2].tolist() == [0] * B, "no rows: every list probed, nothing found"


def test_given_probes_and_the_device_entry_points_above_256(fv, ctx):
    # the probes of fvdb_ivf_coarse_dev_slot fed back to fvdb_ivf_search_probes_dev_slot(_masked) at nprobe 300, and the
    # other device-pointer calls: one answer, the oracle's, with one set of keys
    x, ids, cents, q = D.quality_case()
    gpu, cpu, cl, pos = build_pair(fv, ctx, x, ids, cents)
    dead = np.arange(0, x.shape[0], 7)
    gpu.set_deleted(cl[dead], pos[dead], True)
    for i in ids[dead]:
        cpu.mark_deleted(int(i))
    lib, B = ctx.lib, q.shape[0]
    mask = C.c_void_p()
    ctx.check(lib.fvdb_mask_create_ivf(gpu.h, ids.ctypes.data_as(C.POINTER(C.c_uint64)), ids.size, C.byref(mask)))
    for nprobe in (257, NLIST):
        p_dev = ctx.upload(coarse_dev(ctx, gpu, q, nprobe))
        for k in (10, 300):
            ref = cpu.batch_search(q, k, nprobe)
            calls = {
                "dev": lambda b: lib.fvdb_ivf_search_dev(gpu.h, b.q, B, k, nprobe, *b.args()),
                "dev_slot": lambda b: lib.fvdb_ivf_search_dev_slot(gpu.h, None, 1, b.q, B, k, nprobe, *b.args()),
                "masked": lambda b: lib.fvdb_ivf_search_dev_slot_masked(gpu.h, None, 0, mask, b.q, B, k, nprobe, *b.args()),
                "probes": lambda b: lib.fvdb_ivf_search_probes_dev_slot(gpu.h, None, 0, b.q, p_dev, B, k, nprobe, *b.args()),
                "probes_masked": lambda b: lib.fvdb_ivf_search_probes_dev_slot_masked(gpu.h, None, 2, mask, b.q, p_dev, B, k,
                                                                                     nprobe, *b.args()),
                "wide": lambda b: lib.fvdb_ivf_search_wide_dev_slot(gpu.h, None, 0, None, b.q, B, k, nprobe, *b.args()),
            }
            keys = None
            for name, call in calls.items():
                b = DevBufs(ctx, q, k)
                ctx.check(call(b))
                ctx.synchronize()
                gi, gd, gc, gk = b.read()
                b.free()
                assert_same((gi, gd, gc), ref, f"nprobe={nprobe} k={k} {name}")
                keys = gk if keys is None else keys
                assert np.array_equal(gk, keys), f"nprobe={nprobe} k={k} {name}: out_keys differ"
        ctx.free(p_dev)
    lib.fvdb_mask_destroy(mask)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_more_than_16384_lists_is_refused_above_256_probes(fv, ctx):
    nlist, d = 16385, 4
    gpu = fv.DeviceIVF(ctx, d, nlist)
    gpu.set_centroids(np.random.default_rng(5).standard_normal((nlist, d)).astype(np.float32))
    q = np.zeros((2, d), np.float32)
    with pytest.raises(fv.Unsupported, match="16384"):
        gpu.search(q, 10, 300)
    with pytest.raises(fv.Unsupported):
        gpu.search_wide(q, 300, 300)
    with pytest.raises(fv.Unsupported):
        gpu.coarse(q, 300)
    bufs = DevBufs(ctx, q, 10)
    assert ctx.lib.fvdb_ivf_search_dev_slot(gpu.h, None, 0, bufs.q, 2, 10, 300, *bufs.args()) == E_UNSUPPORTED
    bufs.free()
    assert gpu.search(q, 10, 256)[2].tolist() == [0, 0], "256 probes of such an index are served as before"
    with pytest.raises(fv.FvdbError):  # nprobe = 0 stays an error
        gpu.search(q, 10, 0)


def test_sharded_search_and_a_shard_keep_their_limit(fv, ctx):
    x, ids, cents = D.main_case(20, seed=4400)
    gpu, _, _, _ = build_pair(fv, ctx, x, ids, cents)
    lib = ctx.lib
    comm = fv.sharded.Comm.rccl(ctx)
    s = C.c_void_p()
    ctx.check(lib.fvdb_sharded_create(gpu.h, comm.h, C.byref(s)))
    bufs = DevBufs(ctx, x[:4], 10)
    rc = lib.fvdb_ivf_search_sharded_begin(s, None, 0, bufs.q, 4, 10, 257, 0, bufs.ids, bufs.dist, bufs.cnt)
    assert rc == E_UNSUPPORTED and b"nprobe" in lib.fvdb_last_error(ctx.h)
    lib.fvdb_sharded_destroy(s)
    comm.close()
    # an index that holds a shard of a larger one: the wide route is refused, 256 probes are served
    gpu.set_global_list_sizes(gpu.list_sizes())
    assert lib.fvdb_ivf_search_dev_slot(gpu.h, None, 0, bufs.q, 4, 10, 257, *bufs.args()) == E_UNSUPPORTED
    ctx.check(lib.fvdb_ivf_search_dev_slot(gpu.h, None, 0, bufs.q, 4, 10, 256, *bufs.args()))
    ctx.synchronize()
    bufs.free()


# ---- 8. existing behaviour --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_up_to_256_probes_every_entry_point_is_unchanged(fv, ctx, dtype):
    n, d, nlist, nprobe, B = 4000, 32, 16, 5, 40
    x = mixture(n, d, n_comp=nlist, seed=4500)
    ids = np.arange(n, dtype=np.uint64) + 100
    gpu, cpu, cl, pos = build_pair(fv, ctx, x, ids, x[:nlist].copy(), dtype=dtype)
    q = mixture(B, d, n_comp=nlist, seed=4501)
    lib = ctx.lib
    mask = C.c_void_p()
    ctx.check(lib.fvdb_mask_create_ivf(gpu.h, ids.ctypes.data_as(C.POINTER(C.c_uint64)), ids.size, C.byref(mask)))
    probes = coarse_dev(ctx, gpu, q, nprobe)
    p_dev = ctx.upload(probes)

    def every_entry_point(k):
        out = {}
        out["host"] = gpu.search(q, k, nprobe) + (None,)
        calls = {
            "dev": lambda b: lib.fvdb_ivf_search_dev(gpu.h, b.q, B, k, nprobe, *b.args()),
            "dev_slot": lambda b: lib.fvdb_ivf_search_dev_slot(gpu.h, None, 1, b.q, B, k, nprobe, *b.args()),
            "masked": lambda b: lib.fvdb_ivf_search_dev_slot_masked(gpu.h, None, 0, mask, b.q, B, k, nprobe, *b.args()),
            "probes": lambda b: lib.fvdb_ivf_search_probes_dev_slot(gpu.h, None, 0, b.q, p_dev, B, k, nprobe, *b.args()),
            "probes_masked": lambda b: lib.fvdb_ivf_search_probes_dev_slot_masked(gpu.h, None, 0, mask, b.q, p_dev, B, k,
                                                                                 nprobe, *b.args()),
            "wide": lambda b: lib.fvdb_ivf_search_wide_dev_slot(gpu.h, None, 0, None, b.q, B, k, nprobe, *b.args()),
        }
        for name, call in calls.items():
            b = DevBufs(ctx, q, k)
            ctx.check(call(b))
            ctx.synchronize()
            out[name] = b.read()
            b.free()
        return out

    for k in (10, 256):
        ref = cpu.batch_search(q, k, nprobe, threads=8)
        lib.fvdb_ivf_set_scan_mode(gpu.h, 1)  # FVDB_SCAN_EXACT: the one definition every path must meet
        exact = every_entry_point(k)
        lib.fvdb_ivf_set_scan_mode(gpu.h, 0)
        auto = every_entry_point(k)
        keys = exact["dev"][3]
        for mode, res in (("exact", exact), ("auto", auto)):
            for name, (gi, gd, gc, gk) in res.items():
                assert_same((gi, gd, gc), ref, f"{dtype} k={k} {mode} {name}")
                if gk is not None:
                    assert np.array_equal(gk, keys), f"{dtype} k={k} {mode} {name}: out_keys differ"
    with pytest.raises(fv.Unsupported):  # the register path keeps its k limit below 257 probes
        gpu.search(q, 257, nprobe)
    ctx.free(p_dev)
    lib.fvdb_mask_destroy(mask)


# ---- 9. the index classes -----------------------------------------------------------------------------------------------------
def test_ivf_index_search_at_n_probe_300(fv, ctx):
    x, ids, cents, q = D.quality_case()
    g = fv.IVFIndex(ctx, n_clusters=NLIST, n_probe=NLIST)
    g.set_trained(cents)
    g.batch_insert(ids, x)
    o, _ = D.oracle_index(x, ids, cents)
    for k in (10, 300):
        same_as_oracle(g.search(q, k), o.batch_search(q, k, NLIST))
        same_as_oracle(g.search(q, k, 257), o.batch_search(q, k, 257))


def test_hybrid_index_search_at_ivf_n_probe_300(fv, ctx):
    n, d, now = 1200, 20, 1000 * DAY
    x, ids, cents = D.main_case(d, seed=4600)
    x, ids = x[:n], ids[:n]
    rng = np.random.default_rng(4601)
    ages = np.where(rng.random(n) < 0.1, 1 * DAY, 30 * DAY)
    levels = orc.rng_levels(4601, n)
    kw = dict(max_connections=8, max_connections_layer_0=16, ef_construction=40, n_clusters=NLIST, n_probe=4)

    def make(cls, *a):
        h = cls(*a, **kw)
        h.set_ivf_centroids(cents)
        for i in range(n):
            h.insert_with_timestamp(int(ids[i]), x[i], now - ages[i], now, int(levels[i]))
        return h

    g, o = make(fv.HybridIndex, ctx), make(orc.HybridIndex)
    q = mixture(12, d, n_comp=40, seed=4602)
    for k in (10, 300):
        got = g.search(q, k, now=now, hnsw_ef=50, ivf_n_probe=300)
        same_as_oracle(got, o.batch_search(q, k, now=now, hnsw_ef=50, ivf_n_probe=300))


# ---- 10. evaluate_search_quality ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quality(fv, ctx):
    x, ids, cents, q = D.quality_case()
    cpu, cl = D.oracle_index(x, ids, cents)
    return x, ids, cents, q, cpu, cl


@pytest.mark.parametrize("n_probe,k", [(2, 10), (2, 200), (NLIST, 10)])
def test_evaluate_search_quality_equals_the_reference_fold(fv, ctx, quality, n_probe, k):
    x, ids, cents, q, cpu, cl = quality
    g = fv.IVFIndex(ctx, n_clusters=NLIST, n_probe=n_probe)
    g.set_trained(cents)
    g.batch_insert(ids, x)
    assert np.count_nonzero(g.list_sizes() == 0) >= 20, "some lists are empty"
    recall, precision, avg_recall, avg_precision = D.expected_quality(cpu, q, k, n_probe)
    got = g.evaluate_search_quality(q, k)
    print(f"n_probe={n_probe} k={k}: avg_recall {got['avg_recall']!r} (expected {avg_recall!r}), "
          f"avg_precision {got['avg_precision']!r} (expected {avg_precision!r})")
    assert got["queries_evaluated"] == q.shape[0]
    assert bits(got["avg_recall"]) == bits(avg_recall)
    assert bits(got["avg_precision"]) == bits(avg_precision)
    assert got["avg_query_time_ms"] > 0
    if n_probe == NLIST:
        assert got["avg_recall"] == 1.0 and got["avg_precision"] == 1.0
    else:
        assert got["avg_recall"] < 1.0
    # the per-query values behind the averages
    B = q.shape[0]
    q_dev, out = ctx.upload(q), ctx.alloc(B * 8)
    at = lambda off: C.c_void_p(out.value + off)  # noqa: E731
    ctx.check(ctx.lib.fvdb_ivf_search_quality_dev(g._dev(), None, 0, q_dev, B, k, n_probe, at(0), at(B * 4)))
    ctx.synchronize()
    assert np.array_equal(bits(ctx.download(at(0), B, np.float32)), bits(recall))
    assert np.array_equal(bits(ctx.download(at(B * 4), B, np.float32)), bits(precision))
    ctx.free(q_dev)
    ctx.free(out)


def test_evaluate_search_quality_refuses_an_empty_batch(fv, ctx, quality):
    x, ids, cents, q, cpu, cl = quality
    g = fv.IVFIndex(ctx, n_clusters=NLIST, n_probe=2)
    with pytest.raises(fv.FvdbError):
        g.evaluate_search_quality(q[:0], 10)
    g.set_trained(cents)
    with pytest.raises(fv.InvalidConfig):
        g.evaluate_search_quality(q[:0], 10)
    with pytest.raises(fv.InvalidConfig):
        g.evaluate_search_quality([], 10)
    # the C API makes the refusal itself (src/ivf/operations.rs:334-338)
    out, n = np.zeros(3, np.float32), C.c_uint64(0)
    f32p = C.POINTER(C.c_float)
    assert g.lib.fvh_ivf_evaluate_search_quality(g.h, q.ctypes.data_as(f32p), 0, q.shape[1], 10, out.ctypes.data_as(f32p),
                                                 C.byref(n)) == 6
    # an index with no rows: truth empty, recall 1, precision 0 (:367-377)
    got = g.evaluate_search_quality(q, 10)
    assert got["avg_recall"] == 1.0 and got["avg_precision"] == 0.0 and got["queries_evaluated"] == q.shape[0]
