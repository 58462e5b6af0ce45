"""Filtered search with the allow-set applied on the device.

The contract: a search under an allow-set A returns exactly what the same search returns on an index in which every
row outside A has been soft-deleted — so the oracle is the checker: build it, delete the complement, search.  Where the
HNSW part is scanned exactly instead (scan_cutoff), the checker is a brute force over the allowed live nodes."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture

pytestmark = pytest.mark.gpu

E_INVALID = 6
DAY = 86400.0


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def same(g, ref):
    oi, od, oc = ref
    assert np.array_equal(g.counts, oc), f"hit counts differ: {g.counts[:8]} vs {oc[:8]}"
    for b in range(len(g)):
        n = int(oc[b])
        assert np.array_equal(g.ids[b, :n], oi[b, :n]), f"query {b}: ids differ\n{g.ids[b, :n]}\n{oi[b, :n]}"
        assert np.array_equal(bits(g.distances[b, :n]), bits(od[b, :n])), f"query {b}: distances not bit-identical"


def same_results(a, b):
    assert np.array_equal(a.counts, b.counts)
    assert np.array_equal(a.ids, b.ids)
    assert np.array_equal(bits(a.distances), bits(b.distances))


def allow_sets(ids, rng):
    """50 %, 10 %, 1 %, empty, full, and one with ids the index does not hold."""
    out = {}
    for name, frac in (("half", 0.5), ("tenth", 0.1), ("hundredth", 0.01)):
        out[name] = ids[rng.random(ids.size) < frac]
    out["empty"] = ids[:0]
    out["full"] = ids.copy()
    out["unknown"] = np.concatenate([ids[rng.random(ids.size) < 0.3], np.arange(5, dtype=np.uint64) + 10 ** 12])
    return out


# ---- 1. IVF ------------------------------------------------------------------------------------------
def build_ivf_pair(fv, ctx, n, d, nlist, nprobe, seed, deleted):
    x = mixture(n, d, n_comp=nlist, seed=seed)
    ids = np.arange(n, dtype=np.uint64) * 3 + 7
    cents = x[:nlist].copy()

    def oracle_after(allowed):
        o = orc.IVFIndex(n_clusters=nlist, n_probe=nprobe)
        o.set_trained(cents)
        o.batch_insert(ids, x)
        keep = set(int(i) for i in allowed)
        for i in ids:
            if int(i) in deleted or int(i) not in keep:
                o.mark_deleted(int(i))
        return o

    g = fv.IVFIndex(ctx, n_clusters=nlist, n_probe=nprobe)
    g.set_trained(cents)
    g.batch_insert(ids, x)
    for i in deleted:
        g.mark_deleted(i)
    return g, oracle_after, ids


@pytest.mark.parametrize("d,nlist,nprobe,k,B", [(32, 16, 4, 10, 48), (64, 32, 32, 5, 40), (20, 8, 3, 70, 9)])
def test_ivf_masked_equals_oracle_after_deleting_the_complement(fv, ctx, d, nlist, nprobe, k, B):
    rng = np.random.default_rng(d)
    n = 6000
    deleted = set(int(i) * 3 + 7 for i in rng.choice(n, 200, replace=False))
    g, oracle_after, ids = build_ivf_pair(fv, ctx, n, d, nlist, nprobe, seed=d, deleted=deleted)
    q = mixture(B, d, n_comp=nlist, seed=d + 1)
    h = g._dev()
    unmasked = g.search(q, k, nprobe)
    for name, allowed in allow_sets(ids, rng).items():
        ref = oracle_after(allowed).batch_search(q, k, nprobe)
        for mode in (1, 2, 0):  # exact scan; the matrix-core filter (and its exact rescan where it proves nothing); AUTO
            ctx.check(ctx.lib.fvdb_ivf_set_scan_mode(h, mode))
            same(g.search_allowed(q, k, allowed, nprobe), ref)
        if name == "full":
            same_results(g.search_allowed(q, k, allowed, nprobe), unmasked)
    ctx.check(ctx.lib.fvdb_ivf_set_scan_mode(h, 0))
    same_results(g.search(q, k, nprobe), unmasked)  # the override left nothing behind


def test_ivf_matrix_core_filter_under_dense_and_sparse_masks(fv, ctx):
    n, d, nlist, nprobe, k, B = 20000, 64, 16, 8, 10, 64
    rng = np.random.default_rng(3)
    g, oracle_after, ids = build_ivf_pair(fv, ctx, n, d, nlist, nprobe, seed=11, deleted=set())
    q = mixture(B, d, n_comp=nlist, seed=12)
    h = g._dev()

    def rescans():
        v = C.c_uint64(0)
        ctx.check(ctx.lib.fvdb_ivf_scan_fallbacks(h, C.byref(v)))
        return v.value

    def survivors():
        out = np.zeros(B, np.uint32)
        return ctx.lib.fvdb_ivf_scan_survivors(h, out.ctypes.data_as(C.POINTER(C.c_uint32)), B), out

    ctx.check(ctx.lib.fvdb_ivf_set_scan_mode(h, 2))
    dense = ids[rng.random(n) < 0.5]
    f0 = rescans()
    assert survivors()[0] == E_INVALID  # no matrix-core scan has run on this index yet
    same(g.search_allowed(q, k, dense, nprobe), oracle_after(dense).batch_search(q, k, nprobe))
    f1 = rescans()
    rc, surv = survivors()
    assert rc == 0, "the masked search went through the matrix-core filter"
    assert np.all(surv >= k) and np.all(surv < n * nprobe // nlist // 4), surv  # it kept the top k and discarded most rows
    assert f1 - f0 < B, "and served the dense mask without rescanning everything"
    # too few allowed rows in the sampled blocks for a finite threshold: every allowed row survives to the select stage
    sparse = ids[rng.random(n) < 0.004]
    same(g.search_allowed(q, k, sparse, nprobe), oracle_after(sparse).batch_search(q, k, nprobe))
    ctx.check(ctx.lib.fvdb_ivf_set_scan_mode(h, 0))


def test_ivf_exact_rescan_under_a_mask(fv, ctx):
    # 300 copies of every row: more candidates than the select stage scores, so every query goes to the exact rescan
    # (fallback_scan_kernel) — which must skip the rows the mask does not allow, like every other stage
    d, nlist, nprobe, k = 64, 8, 3, 10
    base = mixture(100, d, seed=501)
    x = np.ascontiguousarray(np.repeat(base, 300, axis=0))
    ids = np.arange(x.shape[0], dtype=np.uint64)
    cents = base[:nlist].copy()
    g = fv.IVFIndex(ctx, n_clusters=nlist, n_probe=nprobe)
    g.set_trained(cents)
    g.batch_insert(ids, x)
    o = orc.IVFIndex(n_clusters=nlist, n_probe=nprobe)
    o.set_trained(cents)
    o.batch_insert(ids, x)
    allowed = ids[np.random.default_rng(4).random(ids.size) < 0.95]
    for i in np.setdiff1d(ids, allowed):
        o.mark_deleted(int(i))
    q = base[:48] + np.float32(0.001)
    h = g._dev()
    v = C.c_uint64(0)
    ctx.check(ctx.lib.fvdb_ivf_set_scan_mode(h, 2))
    ctx.check(ctx.lib.fvdb_ivf_scan_fallbacks(h, C.byref(v)))
    f0 = v.value
    same(g.search_allowed(q, k, allowed, nprobe), o.batch_search(q, k, nprobe))
    ctx.check(ctx.lib.fvdb_ivf_scan_fallbacks(h, C.byref(v)))
    assert v.value - f0 == q.shape[0], "every query was rescanned exactly, under the mask"
    ctx.check(ctx.lib.fvdb_ivf_set_scan_mode(h, 0))


# ---- 2. / 3. HNSW ---------------------------------------------------------------------------------------
def hnsw_pair(fv, ctx, n, d, seed, dup=False):
    x = mixture(n, d, n_comp=6, seed=seed)
    if dup:
        x[n // 2:] = x[:n - n // 2]  # every vector twice: equal distances meet in every result list
    ids = np.arange(n, dtype=np.uint64) + 100
    levels = orc.rng_levels(seed, n)
    g = fv.HNSWIndex(ctx, 6, 12, 40, seed=seed)
    g.batch_insert(ids, x, levels)

    def oracle_after(allowed, deleted=()):
        o = orc.HNSWIndex(6, 12, 40, seed=seed)
        o.batch_insert(ids, x, levels)
        keep = set(int(i) for i in allowed)
        for i in ids:
            if int(i) not in keep or int(i) in deleted:
                o.mark_deleted(int(i))
        return o

    return g, oracle_after, ids, x


@pytest.mark.parametrize("device", [True, False])
def test_hnsw_masked_traversal_equals_oracle_after_deleting_the_complement(fv, ctx, device):
    n, d = 500, 16
    g, oracle_after, ids, x = hnsw_pair(fv, ctx, n, d, seed=21)
    g.scan_cutoff = 0
    g.set_device_traversal(device)
    rng = np.random.default_rng(5)
    q = mixture(24, d, n_comp=6, seed=22)
    entry = g.entry_point()
    g.mark_deleted(int(ids[3]))
    before = g.search(q, 10, 50)
    for name, allowed in allow_sets(ids, rng).items():
        for with_entry in (True, False):
            a = allowed[allowed != entry]
            if with_entry and name != "empty":
                a = np.concatenate([a, [np.uint64(entry)]])
            o = oracle_after(a, deleted={int(ids[3])})
            for k, ef in ((10, 50), (5, 63), (10, 64), (8, 200)):  # both traversal kernels
                same(g.search_allowed(q, k, ef, a), o.batch_search(q, k, ef))
    same_results(g.search(q, 10, 50), before)


def brute_force(x, live_nodes, ids, q, k):
    B = q.shape[0]
    oi = np.full((B, k), np.uint64(2 ** 64 - 1), np.uint64)
    od = np.full((B, k), np.inf, np.float32)
    oc = np.zeros(B, np.uint32)
    for b in range(B):
        if live_nodes.size == 0:
            continue
        dist = orc.l2_batch(q[b], x[live_nodes])
        order = np.lexsort((live_nodes, bits(dist)))[:k]  # distance bits, then node index
        oc[b] = order.size
        oi[b, :order.size] = ids[live_nodes[order]]
        od[b, :order.size] = dist[order]
    return oi, od, oc


@pytest.mark.parametrize("d", [16, 30, 200])
def test_hnsw_exact_scan_equals_brute_force_with_ties_by_node_index(fv, ctx, d):
    n = 700
    g, _, ids, x = hnsw_pair(fv, ctx, n, d, seed=31 + d, dup=True)
    g.scan_cutoff = fv.HNSWIndex.SCAN_ALWAYS
    g.mark_deleted(int(ids[10]))
    rng = np.random.default_rng(6)
    q = np.concatenate([mixture(20, d, n_comp=6, seed=32), x[5:9]])  # some queries ARE stored vectors (distance 0 twice)
    for name, allowed in allow_sets(ids, rng).items():
        nodes = np.array(sorted(set(int(i) - 100 for i in allowed if int(i) - 100 < n) - {10}), np.int64)
        for k in (10, 1, 100, 200):
            same(g.search_allowed(q, k, 50, allowed), brute_force(x, nodes, ids, q, k))
    few = ids[[4, 4 + n // 2, 77]]  # fewer allowed nodes than k, two of them the same vector
    r = g.search_allowed(q, 10, 50, few)
    assert np.all(r.counts == 3)
    same(r, brute_force(x, np.array([4, 77, 4 + n // 2]), ids, q, 10))
    assert np.all(g.search_allowed(q, 10, 50, ids[:0]).counts == 0)
    # the cutoff decides: with more allowed nodes than it, the traversal answers (and finds fewer than the scan may)
    g.scan_cutoff = 2
    assert g.scan_cutoff == 2
    r = g.search_allowed(q, 3, 50, few)
    assert np.all(r.counts <= 3) and np.all(np.isin(r.ids[r.ids != np.uint64(2 ** 64 - 1)], few))


# ---- 4. / 5. hybrid ---------------------------------------------------------------------------------------
def hybrid_pair(fv, ctx, n, d, nlist, seed, recent_frac=0.3, now=1000 * DAY, due_frac=0.05):
    rng = np.random.default_rng(seed)
    x = mixture(n, d, n_comp=nlist, seed=seed)
    ids = np.arange(n, dtype=np.uint64)
    cents = x[:nlist].copy()
    ages = np.where(rng.random(n) < recent_frac, 1 * DAY, 30 * DAY)
    ages[rng.random(n) < due_frac] = 6.5 * DAY  # recent now, due for migration half a day later
    levels = orc.rng_levels(seed, n)
    kw = dict(max_connections=8, max_connections_layer_0=16, ef_construction=40, n_clusters=nlist, n_probe=4)

    def make(cls, *a):
        h = cls(*a, **kw)
        h.set_ivf_centroids(cents)
        for i in range(n):
            h.insert_with_timestamp(int(ids[i]), x[i], now - ages[i], now, int(levels[i]))
        return h

    return make(fv.HybridIndex, ctx), (lambda: make(orc.HybridIndex)), ids, x, ages


def test_hybrid_masked_equals_oracle_after_deleting_the_complement(fv, ctx):
    n, d, nlist, now = 1500, 32, 8, 1000 * DAY
    g, make_oracle, ids, x, ages = hybrid_pair(fv, ctx, n, d, nlist, seed=41)
    g.hnsw().scan_cutoff = 0
    rng = np.random.default_rng(7)
    q = mixture(40, d, n_comp=nlist, seed=42)
    plain = g.search(q, 10, now=now, hnsw_ef=50, ivf_n_probe=4)
    odd = lambda i: i % 2 == 1  # noqa: E731
    filtered = g.search_with_filter(q, 10, odd, now=now)
    for name, allowed in allow_sets(ids, rng).items():
        o = make_oracle()
        keep = set(int(i) for i in allowed)
        for i in ids:
            if int(i) not in keep:
                o.delete(int(i), now)
        same(g.search_allowed(q, 10, allowed, now=now, hnsw_ef=50, ivf_n_probe=4),
             o.batch_search(q, 10, now=now, hnsw_ef=50, ivf_n_probe=4))
    same_results(g.search(q, 10, now=now, hnsw_ef=50, ivf_n_probe=4), plain)
    same_results(g.search_with_filter(q, 10, odd, now=now), filtered)
    # a search whose `now` makes rows due: they migrate first, the masks are built for the rows as they then lie
    # (a migrated row lives in both parts: "deleted" means in both)
    later = now + 1 * DAY
    allowed = ids[rng.random(n) < 0.4]
    o = make_oracle()
    o.batch_search(q[:1], 1, now=later, hnsw_ef=50, ivf_n_probe=4)
    keep = set(int(i) for i in allowed)
    for i in ids:
        if int(i) not in keep:
            for part in (o.hnsw(), o.ivf()):
                try:
                    part.mark_deleted(int(i))
                except orc.VectorNotFound:
                    pass
    hist_before = g.historical_count()
    same(g.search_allowed(q, 10, allowed, now=later, hnsw_ef=50, ivf_n_probe=4),
         o.batch_search(q, 10, now=later, hnsw_ef=50, ivf_n_probe=4))
    assert g.historical_count() > hist_before, "the search migrated rows first"


def test_hybrid_recent_part_scanned_exactly_and_merged(fv, ctx):
    n, d, nlist, now = 1500, 32, 8, 1000 * DAY
    g, make_oracle, ids, x, ages = hybrid_pair(fv, ctx, n, d, nlist, seed=43)
    g.hnsw().scan_cutoff = fv.HNSWIndex.SCAN_ALWAYS
    rng = np.random.default_rng(8)
    q = mixture(33, d, n_comp=nlist, seed=44)
    allowed = ids[rng.random(n) < 0.2]
    k = 10
    got = g.search_allowed(q, k, allowed, now=now, hnsw_ef=50, ivf_n_probe=4)
    # reference lists: the recent part by brute force over the allowed recent nodes (node index = insertion order among
    # the recent rows), the historical part from the oracle's IVF after deleting the complement
    recent_ids = ids[ages < 7 * DAY]
    node_of = {int(i): j for j, i in enumerate(recent_ids)}
    nodes = np.array(sorted(node_of[int(i)] for i in allowed if int(i) in node_of), np.int64)
    ri, rd, rc = brute_force(x[ages < 7 * DAY], nodes, recent_ids, q, k)
    o = make_oracle()
    keep = set(int(i) for i in allowed)
    for i in ids:
        if int(i) not in keep:
            o.delete(int(i), now)
    hi, hd, hc = o.ivf().batch_search(q, k, 4)
    for b in range(q.shape[0]):
        both_i = np.concatenate([ri[b, :rc[b]], hi[b, :hc[b]]])
        both_d = np.concatenate([rd[b, :rc[b]], hd[b, :hc[b]]])
        order = np.argsort(both_d, kind="stable")[:k]  # recent first, stable by distance (src/hybrid/core.rs:476-485)
        assert got.counts[b] == order.size
        assert np.array_equal(got.ids[b, :order.size], both_i[order]), f"query {b}"
        assert np.array_equal(bits(got.distances[b, :order.size]), bits(both_d[order])), f"query {b}"


def test_pushdown_returns_k_where_oversampling_returns_fewer(fv, ctx):
    """The point of the feature: one row in fifty matches, k = 10."""
    n, d, nlist, now, k = 6000, 32, 8, 1000 * DAY, 10
    g, _, ids, x, ages = hybrid_pair(fv, ctx, n, d, nlist, seed=45, recent_frac=0.1)
    allowed = ids[ids % 50 == 0]
    keep = set(int(i) for i in allowed)
    q = mixture(32, d, n_comp=nlist, seed=46)
    pushed = g.search_allowed(q, k, allowed, now=now, ivf_n_probe=8)
    over = g.search_with_filter(q, k, lambda i: i in keep, now=now)
    assert np.all(pushed.counts == k), pushed.counts
    assert np.all(np.isin(pushed.ids, allowed))
    assert np.all(over.counts < k), over.counts
    assert over.counts.mean() < 3


# ---- 6. staleness and sharing ---------------------------------------------------------------------------------------
def test_stale_mask_is_refused_and_one_mask_serves_several_slots(fv, ctx):
    n, d, nlist, nprobe, k, B = 5000, 32, 16, 4, 10, 40
    g, oracle_after, ids = build_ivf_pair(fv, ctx, n, d, nlist, nprobe, seed=51, deleted=set())
    lib, h = ctx.lib, g._dev()
    rng = np.random.default_rng(9)
    allowed = np.ascontiguousarray(ids[rng.random(n) < 0.1])
    q = mixture(B, d, n_comp=nlist, seed=52)
    mask = C.c_void_p()
    ctx.check(lib.fvdb_mask_create_ivf(h, allowed.ctypes.data_as(C.POINTER(C.c_uint64)), allowed.size, C.byref(mask)))
    info = fv._capi.MaskInfo()
    ctx.check(lib.fvdb_mask_info(mask, C.byref(info)))
    assert info.kind == 1 and info.stale == 0 and info.allowed_live == allowed.size
    q_dev = ctx.upload(q)
    ref = oracle_after(allowed).batch_search(q, k, nprobe)
    slots = []
    others = [fv.Context(0) for _ in range(3)]
    for s, on in enumerate([None] + others):  # four searches share the mask, each in its own slot on its own stream
        bufs = (ctx.alloc(B * k * 8), ctx.alloc(B * k * 4), ctx.alloc(B * 4))
        ctx.check(lib.fvdb_ivf_search_dev_slot_masked(h, on.h if on else None, s, mask, q_dev, B, k, nprobe, *bufs, None))
        slots.append(bufs)
    ctx.device_synchronize()
    for bufs in slots:
        r = fv.index.SearchResults(ctx.download(bufs[0], (B, k), np.uint64), ctx.download(bufs[1], (B, k), np.float32),
                                   ctx.download(bufs[2], (B,), np.uint32))
        same(r, ref)
    # the index changes: the mask is refused, by every masked entry
    g.mark_deleted(int(allowed[0]))
    rc = lib.fvdb_ivf_search_dev_slot_masked(h, None, 0, mask, q_dev, B, k, nprobe, *slots[0], None)
    assert rc == E_INVALID and b"stale mask" in lib.fvdb_last_error(ctx.h)
    ctx.check(lib.fvdb_mask_info(mask, C.byref(info)))
    assert info.stale == 1
    lib.fvdb_mask_destroy(mask)
    for bufs in slots:
        for p in bufs:
            ctx.free(p)
    ctx.free(q_dev)
    for c in others:
        c.close()
    # the mirror's cached mask: reused while nothing changed, rebuilt after the delete, and right again
    builds = g.mask_builds()
    same(g.search_allowed(q, k, allowed, nprobe), oracle_after(allowed[1:]).batch_search(q, k, nprobe))
    same(g.search_allowed(q, k, allowed, nprobe), oracle_after(allowed[1:]).batch_search(q, k, nprobe))
    assert g.mask_builds() == builds + 1
    g.insert(10 ** 9, q[0])
    r = g.search_allowed(q[:1], 1, np.concatenate([allowed, [np.uint64(10 ** 9)]]), nlist)
    assert r.ids[0, 0] == 10 ** 9 and r.distances[0, 0] == 0.0
    assert g.mask_builds() == builds + 2


def test_graph_mask_goes_stale_with_the_graph(fv, ctx):
    n, d = 300, 16
    g, oracle_after, ids, x = hnsw_pair(fv, ctx, n, d, seed=61)
    g.scan_cutoff = 0
    q = mixture(16, d, n_comp=6, seed=62)
    allowed = ids[::3]
    same(g.search_allowed(q, 5, 50, allowed), oracle_after(allowed).batch_search(q, 5, 50))
    builds = g.mask_builds()
    same(g.search_allowed(q, 5, 50, allowed), oracle_after(allowed).batch_search(q, 5, 50))
    assert g.mask_builds() == builds
    g.mark_deleted(int(allowed[1]))
    same(g.search_allowed(q, 5, 50, allowed), oracle_after(allowed, deleted={int(allowed[1])}).batch_search(q, 5, 50))
    assert g.mask_builds() == builds + 1


def test_stale_graph_mask_is_refused_by_traversal_and_scan(fv, ctx):
    n, d, B, k = 300, 16, 16, 5
    g, oracle_after, ids, x = hnsw_pair(fv, ctx, n, d, seed=63)
    lib, gh = ctx.lib, g._graph()
    nodes = np.ascontiguousarray(np.arange(0, n, 3, dtype=np.uint32))
    mask = C.c_void_p()
    ctx.check(lib.fvdb_mask_create_graph(gh, nodes.ctypes.data_as(C.POINTER(C.c_uint32)), nodes.size, C.byref(mask)))
    info = fv._capi.MaskInfo()
    ctx.check(lib.fvdb_mask_info(mask, C.byref(info)))
    assert info.kind == 2 and info.stale == 0 and info.allowed_live == nodes.size and info.units == n
    q = mixture(B, d, n_comp=6, seed=64)
    q_dev = ctx.upload(q)
    out = (ctx.alloc(B * k * 4), ctx.alloc(B * k * 4), ctx.alloc(B * 4), ctx.alloc(B * 4))
    ctx.check(lib.fvdb_graph_search_dev_slot_masked(gh, None, 0, mask, q_dev, B, k, 50, *out))
    ctx.synchronize()
    got = fv.index.SearchResults(ids[ctx.download(out[0], (B, k), np.uint32) % n], ctx.download(out[1], (B, k), np.float32),
                                 ctx.download(out[2], (B,), np.uint32))
    assert not ctx.download(out[3], (B,), np.uint32).any()
    same(got, oracle_after(ids[nodes]).batch_search(q, k, 50))
    ctx.check(lib.fvdb_graph_scan_allowed_dev_slot(gh, None, 0, mask, q_dev, B, k, *out[:3]))
    ctx.synchronize()
    got = fv.index.SearchResults(ids[ctx.download(out[0], (B, k), np.uint32) % n], ctx.download(out[1], (B, k), np.float32),
                                 ctx.download(out[2], (B,), np.uint32))
    same(got, brute_force(x, nodes.astype(np.int64), ids, q, k))
    g.mark_deleted(int(ids[1]))  # not even an allowed node: any change of the graph makes the mask stale
    rc = lib.fvdb_graph_search_dev_slot_masked(gh, None, 0, mask, q_dev, B, k, 50, *out)
    assert rc == E_INVALID and b"stale mask" in lib.fvdb_last_error(ctx.h)
    rc = lib.fvdb_graph_scan_allowed_dev_slot(gh, None, 0, mask, q_dev, B, k, *out[:3])
    assert rc == E_INVALID and b"stale mask" in lib.fvdb_last_error(ctx.h)
    ctx.check(lib.fvdb_mask_info(mask, C.byref(info)))
    assert info.stale == 1 and info.reserved == 0
    lib.fvdb_mask_destroy(mask)
    for p in out + (q_dev,):
        ctx.free(p)


def test_queries_handed_back_to_the_host_walk_keep_the_mask(fv, ctx, monkeypatch):
    n, d = 400, 16
    g, oracle_after, ids, x = hnsw_pair(fv, ctx, n, d, seed=65)
    g.scan_cutoff = 0
    q = mixture(20, d, n_comp=6, seed=66)
    allowed = ids[np.random.default_rng(10).random(n) < 0.6]
    want = oracle_after(allowed).batch_search(q, 10, 100)
    same(g.search_allowed(q, 10, 100, allowed), want)
    assert g.device_fallbacks() == 0
    # a candidate heap of 24 slots: ef = 100 queries overflow it and come back with status 1 (not all of them: the mask
    # keeps four nodes in ten out of the heap)
    monkeypatch.setenv("FVDB_GRAPH_CAND_CAP", "24")
    same(g.search_allowed(q, 10, 100, allowed), want)
    assert 0 < g.device_fallbacks() <= q.shape[0]
    monkeypatch.delenv("FVDB_GRAPH_CAND_CAP")
    same(g.search(q, 10, 100), oracle_after(ids).batch_search(q, 10, 100))  # the walk's view was not kept


def test_hybrid_with_an_empty_recent_part(fv, ctx):
    """Only rows older than the recent threshold: the graph has never held a row and has no device store."""
    n, d, nlist, now = 1200, 32, 8, 1000 * DAY
    g, make_oracle, ids, x, ages = hybrid_pair(fv, ctx, n, d, nlist, seed=47, recent_frac=0.0, due_frac=0.0)
    assert g.recent_count() == 0 and g.historical_count() == n
    rng = np.random.default_rng(11)
    q = mixture(36, d, n_comp=nlist, seed=48)
    for cutoff in (0, fv.HNSWIndex.SCAN_ALWAYS):
        g.hnsw().scan_cutoff = cutoff
        for name, allowed in allow_sets(ids, rng).items():
            o = make_oracle()
            keep = set(int(i) for i in allowed)
            for i in ids:
                if int(i) not in keep:
                    o.delete(int(i), now)
            same(g.search_allowed(q, 10, allowed, now=now, hnsw_ef=50, ivf_n_probe=4),
                 o.batch_search(q, 10, now=now, hnsw_ef=50, ivf_n_probe=4))
    # and the first recent row afterwards is seen
    g.insert_with_timestamp(10 ** 6, q[0], now, now, 0)
    r = g.search_allowed(q[:1], 3, np.array([10 ** 6, int(ids[0])], np.uint64), now=now, ivf_n_probe=8)
    assert r.ids[0, 0] == 10 ** 6 and r.distances[0, 0] == 0.0


def test_failed_filtered_search_leaves_no_mask_in_any_slot(fv, ctx):
    n, d, nlist, now, k = 1500, 32, 8, 1000 * DAY, 10
    g, _, ids, x, ages = hybrid_pair(fv, ctx, n, d, nlist, seed=49)
    q = mixture(24, d, n_comp=nlist, seed=50)
    plain = g.search(q, k, now=now, hnsw_ef=50, ivf_n_probe=4)
    allowed = ids[::7]
    ok = g.search_allowed(q, k, allowed, now=now, hnsw_ef=50, ivf_n_probe=4)
    assert np.all(np.isin(ok.ids[ok.ids != np.uint64(2 ** 64 - 1)], allowed))
    bad = q.copy()
    bad[3, 5] = np.nan
    with pytest.raises(Exception) as e:  # refused after the masks were built and a slot was leased
        g.search_allowed(bad, k, allowed, now=now, hnsw_ef=50, ivf_n_probe=4)
    assert e.value.status == 9  # FVDB_E_NONFINITE
    q_dev = ctx.upload(q)
    for slot in range(fv.HybridIndex.SLOTS):  # the explicit pair is an unfiltered search, whichever slot the failure used
        g.search_dev_begin(slot, q_dev, q.shape[0], k, now=now, hnsw_ef=50, ivf_n_probe=4, dim=d)
        same_results(g.search_dev_end(slot), plain)
    ctx.free(q_dev)
    same_results(g.search_allowed(q, k, allowed, now=now, hnsw_ef=50, ivf_n_probe=4), ok)
