"""Search with k up to FVDB_MAX_K_WIDE (4096): the wide selection of the IVF list scan.

The result is the one the exact scan defines for any k — every live row of the probed lists scored with the reference's
f32 fold, ordered by (distance bits, scan position), the k first — so the oracle, which serves any k, is the checker and
every comparison is bit for bit: ids, distance bits and counts."""
import ctypes as C
import inspect
import threading

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture

pytestmark = pytest.mark.gpu

E_INVALID = 6
NO_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
DAY = 86400.0
WIDE_KS = (257, 300, 1000, 4096)


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


def same_results(a, b):
    assert np.array_equal(a.counts, b.counts)
    assert np.array_equal(a.ids, b.ids)
    assert np.array_equal(bits(a.distances), bits(b.distances))


def same_as_oracle(g, ref):
    oi, od, oc = ref
    assert np.array_equal(g.counts, oc), f"hit counts differ: {g.counts[:8]} vs {oc[:8]}"
    for b in range(len(g)):
        n = int(oc[b])
        assert np.array_equal(g.ids[b, :n], oi[b, :n]), f"query {b}: ids differ"
        assert np.array_equal(bits(g.distances[b, :n]), bits(od[b, :n])), f"query {b}: distances not bit-identical"


def build_pair(fv, ctx, x, ids, cents, dtype="f32", clusters=None):
    nlist, d = cents.shape
    gpu = fv.DeviceIVF(ctx, d, nlist, dtype=dtype)
    gpu.set_centroids(cents)
    cpu = orc.IVFIndex(n_clusters=nlist, n_probe=min(4, nlist))
    cpu.set_trained(cents)
    if clusters is None:
        cl, pos = gpu.add(x, ids)
    else:
        cl = np.ascontiguousarray(clusters, np.uint32)
        pos = gpu.add_assigned(x, ids, cl)
    rows = x.astype(np.float16).astype(np.float32) if dtype == "f16" else x  # what the reference would be given
    cpu.batch_insert_assigned(ids, rows, cl)
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


# ---- 1. parity with the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("d", [64, 100, 384])
def test_wide_k_equals_the_oracle(fv, ctx, d, dtype):
    # 20 000 rows in 32 lists: 8 probed lists hold about 5000 rows (more than k for most queries), one list about 600
    # (fewer than k = 1000 and 4096: short results on the way), all 32 everything
    n, nlist = 20_000, 32
    x = mixture(n, d, n_comp=nlist, seed=900 + d)
    ids = np.arange(n, dtype=np.uint64) * 5 + 11
    gpu, cpu, _, _ = build_pair(fv, ctx, x, ids, x[:nlist].copy(), dtype=dtype)
    for B in (1, 33, 257):
        q = mixture(B, d, n_comp=nlist, seed=901 + d + B)
        for nprobe in (1, 8, nlist):
            for k in WIDE_KS:
                got = gpu.search_wide(q, k, nprobe)
                ref = cpu.batch_search(q, k, nprobe, threads=8)
                assert_same(got, ref, f"d={d} {dtype} B={B} nprobe={nprobe} k={k}")
                if nprobe == nlist:
                    assert np.all(got[2] == k), "every list probed: far more than k live rows"


# ---- 2. the wide path at small k is the register path ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_wide_path_at_small_k_equals_the_register_path(fv, ctx, dtype):
    n, d, nlist, nprobe, B = 8000, 48, 16, 5, 70
    x = mixture(n, d, n_comp=nlist, seed=910)
    gpu, _, cl, pos = build_pair(fv, ctx, x, np.arange(n, dtype=np.uint64) + 100, x[:nlist].copy(), dtype=dtype)
    dead = np.arange(0, n, 9)
    gpu.set_deleted(cl[dead], pos[dead], True)
    q = mixture(B, d, n_comp=nlist, seed=911)
    lib = ctx.lib
    lib.fvdb_ivf_set_scan_mode(gpu.h, 1)  # the exact register path: the one definition both must meet
    for k in (1, 10, 256):
        a, b = DevBufs(ctx, q, k), DevBufs(ctx, q, k)
        ctx.check(lib.fvdb_ivf_search_dev_slot(gpu.h, None, 0, a.q, B, k, nprobe, *a.args()))
        ctx.check(lib.fvdb_ivf_search_wide_dev_slot(gpu.h, None, 0, None, b.q, B, k, nprobe, *b.args()))
        ctx.synchronize()
        for name, u, v in zip(("ids", "distances", "counts", "keys"), a.read(), b.read()):
            assert np.array_equal(u.view(np.uint32) if u.dtype == np.float32 else u,
                                  v.view(np.uint32) if v.dtype == np.float32 else v), f"k={k}: {name} differ"
        a.free()
        b.free()
    # and the matrix-core filter path (AUTO) agrees with both at a k it serves
    lib.fvdb_ivf_set_scan_mode(gpu.h, 0)
    ri, rd, rc = gpu.search(q, 10, nprobe)
    wi, wd, wc = gpu.search_wide(q, 10, nprobe)
    assert np.array_equal(ri, wi) and np.array_equal(bits(rd), bits(wd)) and np.array_equal(rc, wc)


# ---- 3. ties ---------------------------------------------------------------------------------------------------------
def test_ties_at_the_cut_keep_scan_order(fv, ctx):
    # 300 copies of one row, 200 of them in list 0 and 100 in list 1, placed between nearer and farther rows: for the
    # k below the k-th place falls inside the copies of one list (nprobe = 1, or k = 300) or between the copies of the
    # two lists (k = 450); equal distances must come out in scan order (probe rank, position in list)
    d, nlist = 8, 4
    rng = np.random.default_rng(12)
    cents = (np.eye(nlist, d, dtype=np.float32) * 0.05).astype(np.float32)
    near = (rng.standard_normal((200, d)) * 0.1).astype(np.float32)
    dup = np.tile(np.full((1, d), 0.75, np.float32), (300, 1))
    far = (rng.standard_normal((400, d)) * 0.1 + 3.0).astype(np.float32)
    x = np.concatenate([near, dup, far])
    cl = np.concatenate([np.where(np.arange(200) < 150, 0, 1), np.where(np.arange(300) % 3 < 2, 0, 1),
                         np.arange(400) % nlist]).astype(np.uint32)
    order = rng.permutation(x.shape[0])  # the copies are spread over the lists' positions
    x, cl = x[order], cl[order]
    ids = np.arange(x.shape[0], dtype=np.uint64) + 5000
    gpu, cpu, _, _ = build_pair(fv, ctx, x, ids, cents, clusters=cl)
    q = (rng.standard_normal((6, d)) * 0.01).astype(np.float32)
    q[0] = 0.0
    for nprobe in (1, 2, nlist):
        for k in (257, 300, 340, 450, 600):
            ref = cpu.batch_search(q, k, nprobe)
            assert_same(gpu.search_wide(q, k, nprobe), ref, f"nprobe={nprobe} k={k}")
    # the case is what it claims: at k = 450 over every list the last row kept and the first one dropped are copies
    ri, rd, rc = cpu.batch_search(q[:1], 451, nlist)
    assert rc[0] == 451 and bits(rd[0, 449:450]) == bits(rd[0, 450:451])
    # small k through the wide path too: ties inside the first block
    for k in (5, 64, 200):
        assert_same(gpu.search_wide(q, k, nlist), cpu.batch_search(q, k, nlist), f"k={k}")


# ---- 4. short results ------------------------------------------------------------------------------------------------
def test_short_results_and_empty_index(fv, ctx):
    cents = np.array([[0.1, 0.0], [5.0, 5.0], [-5.0, -5.0]], np.float32)
    gpu = fv.DeviceIVF(ctx, 2, 3)
    gpu.set_centroids(cents)
    ids, ds, cnt = gpu.search_wide([[1.0, 1.0]], 300, 2)
    assert cnt[0] == 0 and np.all(ids == NO_ID) and np.all(np.isposinf(ds))
    n, d, nlist = 900, 16, 8
    x = mixture(n, d, n_comp=nlist, seed=920)
    gpu, cpu, cl, pos = build_pair(fv, ctx, x, np.arange(n, dtype=np.uint64), x[:nlist].copy())
    q = mixture(9, d, n_comp=nlist, seed=921)
    for k, nprobe in ((1000, nlist), (4096, nlist), (300, 1), (4096, 3)):
        got = gpu.search_wide(q, k, nprobe)
        assert_same(got, cpu.batch_search(q, k, nprobe), f"k={k} nprobe={nprobe}")
        assert np.all(got[2] < k)
    assert np.all(gpu.search_wide(q, 1000, nlist)[2] == n)


# ---- 5. deleted rows and masks ---------------------------------------------------------------------------------------
def test_deleted_rows_are_skipped(fv, ctx):
    n, d, nlist = 12_000, 32, 16
    x = mixture(n, d, n_comp=nlist, seed=930)
    ids = np.arange(n, dtype=np.uint64)
    gpu, cpu, cl, pos = build_pair(fv, ctx, x, ids, x[:nlist].copy())
    dead = np.random.default_rng(3).choice(n, 3000, replace=False)
    gpu.set_deleted(cl[dead], pos[dead], True)
    for i in dead:
        cpu.mark_deleted(int(i))
    q = x[dead[:40]]
    for k, nprobe in ((300, 6), (1000, 8), (4096, nlist)):
        res = gpu.search_wide(q, k, nprobe)
        assert_same(res, cpu.batch_search(q, k, nprobe), f"k={k}")
        assert not np.isin(res[0], dead.astype(np.uint64)).any()


def test_masked_wide_search_equals_the_oracle_after_deleting_the_complement(fv, ctx):
    n, d, nlist, nprobe, B = 9000, 32, 16, 6, 40
    x = mixture(n, d, n_comp=nlist, seed=940)
    ids = np.arange(n, dtype=np.uint64) * 3 + 7
    cents = x[:nlist].copy()
    rng = np.random.default_rng(41)
    deleted = set(int(i) * 3 + 7 for i in rng.choice(n, 300, replace=False))
    g = fv.IVFIndex(ctx, n_clusters=nlist, n_probe=nprobe)
    g.set_trained(cents)
    g.batch_insert(ids, x)
    for i in deleted:
        g.mark_deleted(i)
    q = mixture(B, d, n_comp=nlist, seed=941)
    for name, allowed in (("half", ids[rng.random(n) < 0.5]), ("tenth", ids[rng.random(n) < 0.1]), ("empty", ids[:0]),
                          ("full", ids.copy())):
        o = orc.IVFIndex(n_clusters=nlist, n_probe=nprobe)
        o.set_trained(cents)
        o.batch_insert(ids, x)
        keep = set(int(i) for i in allowed)
        for i in ids:
            if int(i) in deleted or int(i) not in keep:
                o.mark_deleted(int(i))
        for k in (300, 1000):
            same_as_oracle(g.search_allowed(q, k, allowed, nprobe), o.batch_search(q, k, nprobe))
        if name == "full":
            same_results(g.search_allowed(q, 300, allowed, nprobe), g.search(q, 300, nprobe))


def test_stale_mask_is_refused(fv, ctx):
    n, d, nlist, nprobe, B, k = 3000, 16, 8, 4, 8, 300
    x = mixture(n, d, n_comp=nlist, seed=950)
    ids = np.arange(n, dtype=np.uint64)
    gpu, cpu, cl, pos = build_pair(fv, ctx, x, ids, x[:nlist].copy())
    lib = ctx.lib
    allowed = np.ascontiguousarray(ids[::2])
    mask = C.c_void_p()
    ctx.check(lib.fvdb_mask_create_ivf(gpu.h, allowed.ctypes.data_as(C.POINTER(C.c_uint64)), allowed.size, C.byref(mask)))
    q = mixture(B, d, n_comp=nlist, seed=951)
    for i in ids[1::2]:
        cpu.mark_deleted(int(i))
    assert_same(gpu.search_wide(q, k, nprobe, mask=mask), cpu.batch_search(q, k, nprobe), "masked")
    bad = q.copy()
    bad[3, 5] = np.nan
    with pytest.raises(fv.NonFiniteInput):  # host rows are checked under a mask as they are without one
        gpu.search_wide(bad, k, nprobe, mask=mask)
    gpu.set_deleted(cl[:1], pos[:1], True)  # the index changes: the mask is refused
    bufs = DevBufs(ctx, q, k)
    rc = lib.fvdb_ivf_search_wide_dev_slot(gpu.h, None, 0, mask, bufs.q, B, k, nprobe, *bufs.args())
    assert rc == E_INVALID and b"stale mask" in lib.fvdb_last_error(ctx.h)
    bufs.free()
    lib.fvdb_mask_destroy(mask)


# ---- 6. argument errors ----------------------------------------------------------------------------------------------
def test_errors(fv, ctx):
    gpu = fv.DeviceIVF(ctx, 2, 3)
    with pytest.raises(fv.NotTrained):
        gpu.search_wide([[1.0, 2.0]], 300, 1)
    gpu.set_centroids(np.eye(3, 2, dtype=np.float32))
    with pytest.raises(fv.DimensionMismatch):
        gpu.search_wide([[1.0, 2.0, 3.0]], 300, 1)
    with pytest.raises(fv.NonFiniteInput):
        gpu.search_wide([[np.nan, 0.0]], 300, 1)
    for k in (0, 4097):
        with pytest.raises(fv.Unsupported):
            gpu.search_wide([[0.0, 0.0]], k, 1)
        bufs = DevBufs(ctx, np.zeros((1, 2), np.float32), max(k, 1))
        with pytest.raises(fv.Unsupported):
            gpu.search_wide_dev(bufs.q, 1, k, 1, bufs.ids, bufs.dist, bufs.cnt)
        bufs.free()
    with pytest.raises(fv.Unsupported):  # the register path keeps its limit
        gpu.search([[0.0, 0.0]], 257, 1)
    assert gpu.search_wide([[0.0, 0.0]], 4096, 1)[2][0] == 0


# ---- 7. concurrency --------------------------------------------------------------------------------------------------
def test_two_slots_on_two_streams_and_four_host_threads(fv, ctx):
    n, d, nlist, nprobe, k = 12_000, 64, 16, 6, 700
    x = mixture(n, d, n_comp=nlist, seed=960)
    gpu, _, _, _ = build_pair(fv, ctx, x, np.arange(n, dtype=np.uint64), x[:nlist].copy())
    batches = [mixture(48, d, n_comp=nlist, seed=961 + j) for j in range(4)]
    want = [gpu.search_wide(b, k, nprobe) for b in batches]
    other = fv.Context(0)
    lib = ctx.lib
    for _ in range(3):  # slot 0 on the index's stream and slot 1 on another stream, enqueued back to back
        a, b = DevBufs(ctx, batches[0], k), DevBufs(ctx, batches[1], k)
        ctx.synchronize()
        ctx.check(lib.fvdb_ivf_search_wide_dev_slot(gpu.h, None, 0, None, a.q, 48, k, nprobe, *a.args()))
        ctx.check(lib.fvdb_ivf_search_wide_dev_slot(gpu.h, other.h, 1, None, b.q, 48, k, nprobe, *b.args()))
        ctx.synchronize()
        other.synchronize()
        for bufs, ref in ((a, want[0]), (b, want[1])):
            gi, gd, gc, _ = bufs.read()
            assert np.array_equal(gi, ref[0]) and np.array_equal(bits(gd), bits(ref[1])) and np.array_equal(gc, ref[2])
            bufs.free()
    other.close()
    errors = []

    def worker(t):
        try:
            for it in range(6):
                j = (t + it) % len(batches)
                ids, ds, cnt = gpu.search_wide(batches[j], k, nprobe)
                assert np.array_equal(ids, want[j][0]) and np.array_equal(bits(ds), bits(want[j][1])), (t, it)
                assert np.array_equal(cnt, want[j][2])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors[0]


# ---- 8. hybrid and session -------------------------------------------------------------------------------------------
def hybrid_pair(fv, ctx, n, d, nlist, seed, recent_frac=0.1, now=1000 * DAY):
    rng = np.random.default_rng(seed)
    x = mixture(n, d, n_comp=nlist, seed=seed)
    ids = np.arange(n, dtype=np.uint64)
    cents = x[:nlist].copy()
    ages = np.where(rng.random(n) < recent_frac, 1 * DAY, 30 * DAY)
    levels = orc.rng_levels(seed, n)
    kw = dict(max_connections=8, max_connections_layer_0=16, ef_construction=40, n_clusters=nlist, n_probe=4)

    def make(cls, *a):
        h = cls(*a, **kw)
        h.set_ivf_centroids(cents)
        for i in range(n):
            h.insert_with_timestamp(int(ids[i]), x[i], now - ages[i], now, int(levels[i]))
        return h

    return make(fv.HybridIndex, ctx), (lambda: make(orc.HybridIndex)), ids, x


def test_hybrid_search_serves_the_historical_part_above_256(fv, ctx):
    n, d, nlist, now = 4000, 32, 8, 1000 * DAY
    g, make_oracle, ids, x = hybrid_pair(fv, ctx, n, d, nlist, seed=971)
    o = make_oracle()
    q = mixture(24, d, n_comp=nlist, seed=972)
    for k, nprobe in ((300, 4), (1000, 8)):
        got = g.search(q, k, now=now, hnsw_ef=50, ivf_n_probe=nprobe)
        same_as_oracle(got, o.batch_search(q, k, now=now, hnsw_ef=50, ivf_n_probe=nprobe))
        assert np.all(got.counts > 256), "historical rows are part of the answer"

    # search_with_filter(k = 100): 300 candidates with the default config, the first 100 that match
    k = 100
    allowed = set(range(0, n, 3))
    got = g.search_with_filter(q, k, lambda rid: rid in allowed, now=now)
    oi, od, oc = o.batch_search(q, 3 * k, now=now)  # SearchConfig::default with k = 3 k (src/hybrid/core.rs:419-423, 527-531)
    for b in range(q.shape[0]):
        want = [(int(i), dd) for i, dd in zip(oi[b, : oc[b]], od[b, : oc[b]]) if int(i) in allowed][:k]
        assert got.counts[b] == len(want)
        assert got.ids[b, : len(want)].tolist() == [w[0] for w in want]
        assert np.array_equal(bits(got.distances[b, : len(want)]), bits(np.asarray([w[1] for w in want], np.float32)))
    assert got.counts.max() > 256 // 3, "more matches than 256 candidates could hold: the historical part was searched"

    # three batches in flight at k = 300 equal the blocking search
    qs = [mixture(16, d, n_comp=nlist, seed=973 + j) for j in range(3)]
    blocking = [g.search(qq, 300, now=now, hnsw_ef=50, ivf_n_probe=4) for qq in qs]
    q_dev = [ctx.upload(qq) for qq in qs]
    for s in range(3):
        g.search_dev_begin(s, q_dev[s], 16, 300, now=now, hnsw_ef=50, ivf_n_probe=4, dim=d)
    for s in range(3):
        same_results(g.search_dev_end(s), blocking[s])
    for p in q_dev:
        ctx.free(p)

    # above the wide limit: an error, never the recent rows alone
    with pytest.raises(fv.Unsupported):
        g.search(q, 5000, now=now, hnsw_ef=50, ivf_n_probe=4)
    with pytest.raises(fv.Unsupported):
        g.search(q, 10, now=now, hnsw_ef=50, ivf_n_probe=4, historical_k=5000)
    same_results(g.search(qs[0], 300, now=now, hnsw_ef=50, ivf_n_probe=4), blocking[0])  # and nothing is left behind


def test_hybrid_search_allowed_above_256(fv, ctx):
    n, d, nlist, now, k = 4000, 32, 8, 1000 * DAY, 300
    g, make_oracle, ids, x = hybrid_pair(fv, ctx, n, d, nlist, seed=981)
    g.hnsw().scan_cutoff = 0  # the recent part by the masked traversal, as the oracle walks it after the deletes
    rng = np.random.default_rng(9)
    q = mixture(20, d, n_comp=nlist, seed=982)
    allowed = ids[rng.random(n) < 0.5]
    o = make_oracle()
    keep = set(int(i) for i in allowed)
    for i in ids:
        if int(i) not in keep:
            o.delete(int(i), now)
    got = g.search_allowed(q, k, allowed, now=now, hnsw_ef=50, ivf_n_probe=8)
    same_as_oracle(got, o.batch_search(q, k, now=now, hnsw_ef=50, ivf_n_probe=8))
    assert np.all(got.counts == k)
    with pytest.raises(fv.Unsupported):
        g.search_allowed(q, 5000, allowed, now=now, hnsw_ef=50, ivf_n_probe=8)


def test_session_filtered_search_at_k_100_in_both_modes(fv, ctx):
    """k = 100 with a filter asks the index for 300 candidates; before the wide path the historical part of such a search
    was dropped.  Every row is migrated here, and a migrated row lives in both parts (as in the reference), so a row may
    come back twice, and the two modes see different duplicates (the masked graph walk reaches more matching rows than
    the unmasked one).  All three inverted lists are probed, so apart from duplicates both modes must return the true
    ranking of the matching rows: the lists are compared by first occurrence."""
    s = fv.VectorDbSession(ctx, max_connections=8, max_connections_layer_0=16, ef_construction=40)
    n, d = 1500, 8
    x = mixture(n, d, n_comp=6, seed=990)
    s.add_vectors([{"id": f"doc-{i}", "vector": x[i].tolist(), "metadata": {"even": i % 2 == 0}} for i in range(n)])
    s.now = 30 * DAY
    for _ in range(2 * n // 100 + 2):  # every row is due: copy them all to the inverted lists
        if s.index.recent_count() == 0:
            break
        s.index.migrate_with_threshold(7 * DAY, s.now)
    assert s.index.recent_count() == 0 and s.index.historical_count() == n
    # the comparison with the true ranking below holds only while the session's searches probe every list: both filter
    # modes search with the default config (HybridSearchConfig::default, ivf_n_probe = 10)
    default_n_probe = inspect.signature(s.index.search_allowed).parameters["ivf_n_probe"].default
    assert s.index.ivf().n_clusters <= default_n_probe, "the session default no longer probes every inverted list"
    flt = {"even": True}
    even = np.arange(0, n, 2)

    def first_seen(rows):
        return list(dict.fromkeys(r["id"] for r in rows))

    full = 0
    for qi in range(8):
        qv = x[qi * 17]
        truth = [f"doc-{i}" for i in even[np.argsort(orc.l2_batch(qv, x[even]), kind="stable")]]
        over = s.search(qv.tolist(), 100, {"filter": flt})
        pushed = s.search(qv.tolist(), 100, {"filter": flt, "filterMode": "pushdown"})
        assert all(r["metadata"]["even"] is True for r in over + pushed)
        assert len(pushed) == 100
        for rows in (over, pushed):
            assert [r["score"] for r in rows] == sorted((r["score"] for r in rows), reverse=True)
            seen = first_seen(rows)
            assert seen == truth[:len(seen)], "the nearest matching rows, nearest first"
        if len(over) == 100:
            full += 1
            # the graph walk returns at most ef = 50 rows: a hundred matches hold rows of the inverted lists
            m = min(len(first_seen(over)), len(first_seen(pushed)))
            assert first_seen(over)[:m] == first_seen(pushed)[:m]
    assert full >= 4, "half of the rows match: 300 candidates hold 100 matches for most queries"
    s.destroy()
