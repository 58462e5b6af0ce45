"""Batched filtered search: one allow-set per query in a single call.

The contract: a grouped call takes G allow-sets and a group index per query, and the result for query b is, bit for bit,
what the single-allow-set call returns for query b alone under allow_sets[group[b]] — ids, distance bits, counts, order,
and on the IVF device entry point the selection keys.  So the checkers of section 9c carry over per group: the CPU oracle
after deleting the complement, and for the graph's exact scan a brute force over the group's allowed live nodes.  A group
may be None ("no filter"): its queries get what the unfiltered search returns."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = 6, 12
MAX_K = 256
DAY = 86400.0
NO_ID = np.uint64(2 ** 64 - 1)
u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def rounded(x):
    """The rows of an index with row_dtype="f16" as it stores them: what the reference would be given."""
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def rows_of(res, idx):
    return res.ids[idx], res.distances[idx], res.counts[idx]


def same(got, ref, what):
    """got, ref: (ids, distances, counts); compared over the hits each query has."""
    gi, gd, gc = got
    oi, od, oc = ref
    assert np.array_equal(gc, oc), f"{what}: hit counts differ: {gc[:8]} vs {oc[:8]}"
    for b in range(len(gc)):
        n = int(oc[b])
        assert np.array_equal(gi[b, :n], oi[b, :n]), f"{what}, query {b}: ids differ\n{gi[b, :n]}\n{oi[b, :n]}"
        assert np.array_equal(bits(gd[b, :n]), bits(od[b, :n])), f"{what}, query {b}: distances not bit-identical"


def same_blocks(got, ref, what):
    """Whole result blocks, padding included."""
    for name, u, v in zip(("ids", "distances", "counts", "keys"), got, ref):
        u, v = np.asarray(u), np.asarray(v)
        if u.dtype == np.float32:
            u, v = bits(u), bits(v)
        assert np.array_equal(u, v), f"{what}: {name} differ"


def group_sets(ids, rng):
    """half / tenth / hundredth / empty / full / unknown ids / None."""
    return [ids[rng.random(ids.size) < 0.5], ids[rng.random(ids.size) < 0.1], ids[rng.random(ids.size) < 0.01], ids[:0],
            ids.copy(), np.concatenate([ids[rng.random(ids.size) < 0.3], np.arange(5, dtype=np.uint64) + 10 ** 12]), None]


def ivf_mask(ctx, h, allowed):
    a = np.ascontiguousarray(allowed, np.uint64)
    a = a if a.size else np.zeros(1, np.uint64)[:0]
    m = C.c_void_p()
    ctx.check(ctx.lib.fvdb_mask_create_ivf(h, a.ctypes.data_as(u64p), a.size, C.byref(m)))
    return m


def mask_table(masks):
    return (C.c_void_p * max(len(masks), 1))(*[None if m is None else m.value for m in masks])


def on_device(ctx, q, k, call):
    """call(q_dev, n, ids, dist, counts, keys) on a batch and outputs in HBM -> (ids, distances, counts, keys)."""
    q = np.ascontiguousarray(q, np.float32)
    n = q.shape[0]
    q_dev, out = ctx.upload(q), ctx.alloc(n * k * 20 + n * 4)
    at = lambda off: C.c_void_p(out.value + off)  # noqa: E731
    ids, keys, dist, cnt = at(0), at(n * k * 8), at(n * k * 16), at(n * k * 20)
    try:
        ctx.check(call(q_dev, n, ids, dist, cnt, keys))
        ctx.device_synchronize()
        return (ctx.download(ids, (n, k), np.uint64), ctx.download(dist, (n, k), np.float32),
                ctx.download(cnt, n, np.uint32), ctx.download(keys, (n, k), np.uint64))
    finally:
        ctx.free(q_dev)
        ctx.free(out)


def groups_call(lib, h, table, G, group, k, nprobe, slot=0):
    g = np.ascontiguousarray(group, np.uint32)
    return lambda qd, n, ids, dist, cnt, keys: lib.fvdb_ivf_search_groups_dev_slot(
        h, None, slot, table, G, g.ctypes.data_as(u32p), qd, n, k, nprobe, ids, dist, cnt, keys)


# ---- 1. IVF ---------------------------------------------------------------------------------------------
def build_ivf_pair(fv, ctx, n, d, nlist, nprobe, seed, deleted, row_dtype="f32"):
    """The construction of test_gpu_allowed_search.py: the index, and the oracle after deleting the complement."""
    x = mixture(n, d, n_comp=min(nlist, 32), seed=seed)
    ids = np.arange(n, dtype=np.uint64) * 3 + 7
    cents = x[:nlist].copy()
    rows = rounded(x) if row_dtype == "f16" else x

    def oracle_after(allowed):
        o = orc.IVFIndex(n_clusters=nlist, n_probe=nprobe)
        o.set_trained(cents)
        o.batch_insert(ids, rows)
        keep = set(int(i) for i in allowed)
        for i in ids:
            if int(i) in deleted or int(i) not in keep:
                o.mark_deleted(int(i))
        return o

    g = fv.IVFIndex(ctx, n_clusters=nlist, n_probe=nprobe, row_dtype=row_dtype)
    g.set_trained(cents)
    g.batch_insert(ids, x)
    for i in deleted:
        g.mark_deleted(i)
    return g, oracle_after, ids


IVF_SHAPES = [(32, 16, 4, 10, 48, "f32"),     # every work item of 16 queries mixes seven groups
              (32, 16, 4, 10, 48, "f16"),
              (20, 8, 3, 70, 9, "f32"),       # the d4 tail loop, work items of at most four queries
              (64, 32, 32, 300, 40, "f32"),   # k > 256
              (16, 300, 280, 10, 24, "f32")]  # more than 256 probes: the full centroid ranking


@pytest.mark.parametrize("d,nlist,nprobe,k,B,row_dtype", IVF_SHAPES)
def test_ivf_groups_equal_oracle_and_single_mask_search_per_group(fv, ctx, d, nlist, nprobe, k, B, row_dtype):
    rng = np.random.default_rng(d + k)
    n = 6000
    deleted = set(int(i) * 3 + 7 for i in rng.choice(n, 200, replace=False))
    g, oracle_after, ids = build_ivf_pair(fv, ctx, n, d, nlist, nprobe, seed=d, deleted=deleted, row_dtype=row_dtype)
    q = mixture(B, d, n_comp=min(nlist, 32), seed=d + 1)
    sets = group_sets(ids, rng)
    G = len(sets)
    group = np.arange(B) % G
    builds = g.mask_builds()
    got = g.search_allowed_groups(q, k, sets, group, nprobe)
    assert g.mask_builds() == builds + G - 1, "one mask per filtered group, built for the call"
    lib, h = ctx.lib, g._dev()
    masks = [None if a is None else ivf_mask(ctx, h, a) for a in sets]
    dev = on_device(ctx, q, k, groups_call(lib, h, mask_table(masks), G, group, k, nprobe))
    same_blocks(dev[:3], (got.ids, got.distances, got.counts), "device entry point against the index class")
    for gi, allowed in enumerate(sets):
        idx = np.flatnonzero(group == gi)
        what = f"group {gi}"
        ref = oracle_after(ids if allowed is None else allowed).batch_search(q[idx], k, nprobe)
        same(rows_of(got, idx), ref, what + " against the oracle")
        one = g.search(q[idx], k, nprobe) if allowed is None else g.search_allowed(q[idx], k, allowed, nprobe)
        same_blocks(rows_of(got, idx), (one.ids, one.distances, one.counts), what + " against search_allowed")
        m = masks[gi]
        if k > MAX_K:
            call = lambda qd, nq, *out: lib.fvdb_ivf_search_wide_dev_slot(h, None, 0, m, qd, nq, k, nprobe, *out)  # noqa: E731
        elif m is None:
            call = lambda qd, nq, *out: lib.fvdb_ivf_search_dev_slot(h, None, 0, qd, nq, k, nprobe, *out)  # noqa: E731
        else:
            call = lambda qd, nq, *out: lib.fvdb_ivf_search_dev_slot_masked(h, None, 0, m, qd, nq, k, nprobe, *out)  # noqa: E731
        same_blocks([a[idx] for a in dev], on_device(ctx, q[idx], k, call), what + " against the single-mask entry point, keys too")
    for m in masks:
        if m is not None:
            lib.fvdb_mask_destroy(m)
    plain = g.search(q, k, nprobe)
    none = g.search_allowed_groups(q, k, [None, None], np.arange(B) % 2, nprobe)
    same_blocks((none.ids, none.distances, none.counts), (plain.ids, plain.distances, plain.counts), "every group None")
    assert g.mask_builds() == builds + 2 * (G - 1), "the cached mask of search_allowed was rebuilt per group, nothing else"


# ---- 2. IVF: more queries than one sub-batch ------------------------------------------------------------
SUB, N_SMALL, NLIST_SMALL = 16384, 700, 4


def small_world(fv, ctx):
    """The 700-row, 4-list index of test_gpu_ivf_sub_batches.py, restated: two long lists, two of fewer than k rows that
    are each other's nearest, copies of rows (ties), soft-deleted rows (short counts)."""
    d, B = 8, SUB + 300
    rng = np.random.default_rng(78)
    centres = (np.random.default_rng(8).standard_normal((NLIST_SMALL, d)) * 4).astype(np.float32)
    centres[3] = centres[2] + np.float32(0.8)

    def clustered(per_list):
        comp = np.repeat(np.arange(NLIST_SMALL), per_list)
        return (centres[comp] + np.float32(0.35) * rng.standard_normal((comp.size, d))).astype(np.float32)

    x = clustered([340, 351, 5, 4])
    x[600:650] = x[100:150]
    ids = np.arange(N_SMALL, dtype=np.uint64) * 3 + 5
    gpu = fv.DeviceIVF(ctx, d, NLIST_SMALL)
    gpu.set_centroids(centres)
    cl, pos = gpu.add(x, ids)
    dead = np.concatenate([np.arange(7, N_SMALL, 29), [100, 101, 602, 693]])
    gpu.set_deleted(cl[dead], pos[dead], True)

    def oracle_after(allowed):
        o = orc.IVFIndex(n_clusters=NLIST_SMALL, n_probe=2)
        o.set_trained(centres)
        o.batch_insert_assigned(ids, x, cl)
        keep = set(int(i) for i in allowed)
        for j, i in enumerate(ids):
            if j in set(dead.tolist()) or int(i) not in keep:
                o.mark_deleted(int(i))
        return o

    q = clustered([B // NLIST_SMALL] * NLIST_SMALL)
    q = q[rng.permutation(B)]
    q[5:45] = x[100:140]
    q[SUB + 3:SUB + 13] = x[640:650]
    return gpu, oracle_after, ids, np.ascontiguousarray(q), rng


def test_ivf_groups_across_sub_batches_keep_each_query_with_its_group(fv, ctx):
    gpu, oracle_after, ids, q, rng = small_world(fv, ctx)
    B, k, nprobe = q.shape[0], 10, 2
    sets = [ids[rng.random(ids.size) < 0.5], ids[rng.random(ids.size) < 0.1], None, ids[rng.random(ids.size) < 0.8]]
    G = len(sets)
    group = (np.arange(B) % G).astype(np.uint32)
    lib, h = ctx.lib, gpu.h
    masks = [None if a is None else ivf_mask(ctx, h, a) for a in sets]
    table = mask_table(masks)
    whole = on_device(ctx, q, k, groups_call(lib, h, table, G, group, k, nprobe))
    first = on_device(ctx, q[:SUB], k, groups_call(lib, h, table, G, group[:SUB], k, nprobe))
    rest = on_device(ctx, q[SUB:], k, groups_call(lib, h, table, G, group[SUB:], k, nprobe))
    same_blocks(whole, [np.concatenate([a, b]) for a, b in zip(first, rest)], "one call against two")
    ends = np.concatenate([np.arange(64), np.arange(B - 64, B)])
    for gi, allowed in enumerate(sets):
        idx = ends[group[ends] == gi]
        ref = oracle_after(ids if allowed is None else allowed).batch_search(q[idx], k, nprobe)
        same([a[idx] for a in whole[:3]], ref, f"group {gi}, first and last 64 queries against the oracle")
    for m in masks:
        if m is not None:
            lib.fvdb_mask_destroy(m)
    gpu.close()


# ---- 3. IVF: what is refused, and that nothing was enqueued ---------------------------------------------
def test_ivf_groups_refusals_leave_the_slot_untouched(fv, ctx):
    n, d, nlist, nprobe, k, B = 2000, 16, 8, 3, 10, 20
    x = mixture(n, d, n_comp=nlist, seed=91)
    ids = np.arange(n, dtype=np.uint64) + 1
    q = mixture(B, d, n_comp=nlist, seed=92)
    lib = ctx.lib

    def make():
        ix = fv.DeviceIVF(ctx, d, nlist)
        ix.set_centroids(x[:nlist].copy())
        ix.add(x, ids)
        return ix

    a, b = make(), make()
    plain = lambda ix: on_device(ctx, q, k, lambda qd, nq, *out: lib.fvdb_ivf_search_dev_slot(ix.h, None, 0, qd, nq, k, nprobe, *out))  # noqa: E731
    want = plain(a)
    group = (np.arange(B) % 2).astype(np.uint32)

    def refused(ix, masks, grp, status, text):
        q_dev, out = ctx.upload(q), ctx.alloc(B * k * 20 + B * 4)
        at = lambda off: C.c_void_p(out.value + off)  # noqa: E731
        grp = np.ascontiguousarray(grp, np.uint32)
        rc = lib.fvdb_ivf_search_groups_dev_slot(ix.h, None, 0, mask_table(masks), len(masks), grp.ctypes.data_as(u32p), q_dev, B, k,
                                                 nprobe, at(0), at(B * k * 16), at(B * k * 20), at(B * k * 8))
        assert rc == status, (rc, lib.fvdb_last_error(ctx.h))
        assert text in lib.fvdb_last_error(ctx.h), lib.fvdb_last_error(ctx.h)
        ctx.free(q_dev)
        ctx.free(out)
        same_blocks(plain(ix), want, "an ordinary search on the slot after the refusal")

    ma, mb = ivf_mask(ctx, a.h, ids[::2]), ivf_mask(ctx, b.h, ids[::2])
    bad = group.copy()
    bad[B - 1] = 2
    refused(a, [ma, None], bad, E_INVALID, b"group index")
    refused(a, [ma, mb], group, E_INVALID, b"mask of another index")
    refused(a, [ma, None, mb], group, E_INVALID, b"mask of another index")  # checked though no query names it
    refused(a, [], group, E_INVALID, b"no group")
    ok = on_device(ctx, q, k, groups_call(lib, a.h, mask_table([ma, None]), 2, group, k, nprobe))
    assert np.array_equal(ok[2][1::2], want[2][1::2]) and np.array_equal(ok[0][1::2], want[0][1::2])
    a.add(q[:1], np.array([10 ** 9], np.uint64))  # one more row: the mask is stale
    want = plain(a)
    refused(a, [ma, None], group, E_INVALID, b"stale mask")
    # an index holding a shard of a larger one: its masks are fresh, the grouped search is not served
    b.set_global_list_sizes(b.list_sizes() * 2)
    want = plain(b)
    lib.fvdb_mask_destroy(mb)
    mb = ivf_mask(ctx, b.h, ids[::2])
    refused(b, [mb, None], group, E_UNSUPPORTED, b"shard")
    for m in (ma, mb):
        lib.fvdb_mask_destroy(m)
    # B == 0 with no group is nothing to do
    assert lib.fvdb_ivf_search_groups_dev_slot(a.h, None, 0, mask_table([]), 0, None, None, 0, k, nprobe, None, None, None, None) == 0
    a.close()
    b.close()


# ---- 4. graph: the exact scan with one node list per query ----------------------------------------------
N_GRAPH, D_GRAPH = 3000, 24
GROUP_SIZES = (0, 1, 63, 64, 65, 300, 2500)


class Graph:
    def __init__(self, fv, ctx, row_dtype):
        n, d = N_GRAPH, D_GRAPH
        rng = np.random.default_rng(101)
        x = mixture(n, d, n_comp=6, seed=102)
        src = rng.choice(n - 100, 100, replace=False)
        x[n - 100:] = x[src]  # copies of other rows: equal distances, ordered by node index
        self.ids = np.arange(n, dtype=np.uint64) + 100
        self.levels = orc.rng_levels(103, n)
        self.x = x
        self.rows = rounded(x) if row_dtype == "f16" else x
        self.g = fv.HNSWIndex(ctx, 6, 12, 40, seed=103, row_dtype=row_dtype)
        self.g.batch_insert(self.ids, x, self.levels)
        self.dead = rng.choice(n, 50, replace=False)
        for i in self.dead:
            self.g.mark_deleted(int(self.ids[i]))
        self.q = np.concatenate([mixture(33, d, n_comp=6, seed=104), x[src[:4]]])  # B = 37; four queries ARE stored rows
        # each group: that many allowed LIVE nodes (copies among them), and from 63 up three deleted nodes besides
        live = np.setdiff1d(np.arange(n), self.dead)
        self.sets = [self.ids[np.sort(np.concatenate([rng.choice(live, size, replace=False), self.dead[:3] if size >= 63 else []]).astype(np.int64))]
                     for size in GROUP_SIZES]

    def live_nodes(self, allowed):
        nodes = np.setdiff1d((allowed - np.uint64(100)).astype(np.int64), self.dead)
        return np.sort(nodes)


_graphs = {}


def graph(fv, ctx, row_dtype):
    if row_dtype not in _graphs:
        _graphs[row_dtype] = Graph(fv, ctx, row_dtype)
    return _graphs[row_dtype]


def brute_force(x, live_nodes, ids, q, k):
    B = q.shape[0]
    oi = np.full((B, k), NO_ID, np.uint64)
    od = np.full((B, k), np.inf, np.float32)
    oc = np.zeros(B, np.uint32)
    for b in range(B):
        if live_nodes.size == 0:
            continue
        dist = orc.l2_batch(q[b], x[live_nodes])  # the sequential f32 fold
        order = np.lexsort((live_nodes, bits(dist)))[:k]  # distance bits, then node index
        oc[b] = order.size
        oi[b, :order.size] = ids[live_nodes[order]]
        od[b, :order.size] = dist[order]
    return oi, od, oc


@pytest.mark.parametrize("row_dtype", ["f32", "f16"])
def test_graph_grouped_scan_equals_brute_force_and_search_allowed_per_group(fv, ctx, row_dtype):
    w = graph(fv, ctx, row_dtype)
    g, q = w.g, w.q
    B, G = q.shape[0], len(w.sets)
    g.scan_cutoff = fv.HNSWIndex.SCAN_ALWAYS
    group = np.arange(B) % G  # a workgroup of four waves holds four groups; the last workgroup has absent waves
    for k in (1, 10, 200):
        builds = g.mask_builds()
        got = g.search_allowed_groups(q, k, 50, w.sets, group)
        assert g.mask_builds() == builds + G
        for gi, allowed in enumerate(w.sets):
            idx = np.flatnonzero(group == gi)
            what = f"k {k}, group of {GROUP_SIZES[gi]}"
            same(rows_of(got, idx), brute_force(w.rows, w.live_nodes(allowed), w.ids, q[idx], k), what + " against the brute force")
            one = g.search_allowed(q[idx], k, 50, allowed)
            same_blocks(rows_of(got, idx), (one.ids, one.distances, one.counts), what + " against search_allowed")
    g.scan_cutoff = 8192


def test_graph_grouped_scan_refusals(fv, ctx):
    w = graph(fv, ctx, "f32")
    g, q = w.g, w.q
    lib, gh = ctx.lib, g._graph()
    B, k = q.shape[0], 5
    other = fv.HNSWIndex(ctx, 6, 12, 40, seed=1)
    other.batch_insert(w.ids[:50], w.x[:50], w.levels[:50])

    def gmask(handle, nodes):
        nd = np.ascontiguousarray(nodes, np.uint32)
        m = C.c_void_p()
        ctx.check(lib.fvdb_mask_create_graph(handle, nd.ctypes.data_as(u32p), nd.size, C.byref(m)))
        return m

    m0, m1, mo = gmask(gh, np.arange(0, 500, 2)), gmask(gh, np.arange(40)), gmask(other._graph(), np.arange(10))
    q_dev = ctx.upload(q)
    out = (ctx.alloc(B * k * 4), ctx.alloc(B * k * 4), ctx.alloc(B * 4))
    group = (np.arange(B) % 2).astype(np.uint32)

    def call(masks, grp):
        return lib.fvdb_graph_scan_allowed_groups_dev_slot(gh, None, 0, mask_table(masks), len(masks), grp.ctypes.data_as(u32p), q_dev,
                                                           B, k, *out)

    ctx.check(call([m0, m1], group))
    ctx.synchronize()
    nodes = ctx.download(out[0], (B, k), np.uint32)
    dist = ctx.download(out[1], (B, k), np.float32)
    cnt = ctx.download(out[2], (B,), np.uint32)
    for gi, allowed_nodes in enumerate((np.arange(0, 500, 2), np.arange(40))):
        idx = np.flatnonzero(group == gi)
        live = np.setdiff1d(allowed_nodes, w.dead)
        same((w.ids[nodes[idx] % N_GRAPH], dist[idx], cnt[idx]), brute_force(w.x, live, w.ids, q[idx], k), f"C entry point, group {gi}")
    bad = group.copy()
    bad[0] = 2
    assert call([m0, m1], bad) == E_INVALID and b"group index" in lib.fvdb_last_error(ctx.h)
    assert call([m0, mo], group) == E_INVALID and b"another graph" in lib.fvdb_last_error(ctx.h)
    assert call([m0, None], group) == E_INVALID  # every query names a mask: the unfiltered exact scan is another call
    assert call([], group) == E_INVALID
    for m in (m0, m1, mo):
        lib.fvdb_mask_destroy(m)
    for p in out + (q_dev,):
        ctx.free(p)


# ---- 5. HNSWIndex: scanned, traversed and unfiltered groups in one batch --------------------------------
def test_hnsw_groups_route_each_group_as_search_allowed_would(fv, ctx):
    w = graph(fv, ctx, "f32")
    g, q = w.g, w.q
    B = q.shape[0]
    g.scan_cutoff = 100
    sets = [w.sets[3], w.sets[6], None]  # 64 allowed nodes: scanned; 2500: traversed; no filter
    group = np.arange(B) % 3
    k, ef = 10, 50
    got = g.search_allowed_groups(q, k, ef, sets, group)

    def oracle_after(allowed):
        o = orc.HNSWIndex(6, 12, 40, seed=103)
        o.batch_insert(w.ids, w.x, w.levels)
        keep = set(int(i) for i in allowed)
        dead = set(int(w.ids[i]) for i in w.dead)
        for i in w.ids:
            if int(i) not in keep or int(i) in dead:
                o.mark_deleted(int(i))
        return o

    for gi, allowed in enumerate(sets):
        idx = np.flatnonzero(group == gi)
        if gi == 0:  # below the cutoff the contract of section 9c is the exact scan, not the thinned graph's traversal
            ref = brute_force(w.x, w.live_nodes(allowed), w.ids, q[idx], k)
        else:
            ref = oracle_after(w.ids if allowed is None else allowed).batch_search(q[idx], k, ef)
        same(rows_of(got, idx), ref, f"group {gi}")
        one = g.search(q[idx], k, ef) if allowed is None else g.search_allowed(q[idx], k, ef, allowed)
        same_blocks(rows_of(got, idx), (one.ids, one.distances, one.counts), f"group {gi} against search_allowed")
    g.scan_cutoff = 8192


# ---- 6. hybrid --------------------------------------------------------------------------------------------
def test_hybrid_groups_equal_oracle_and_search_allowed_per_group(fv, ctx):
    n, d, nlist, now = 3000, 32, 8, 1000 * DAY
    rng = np.random.default_rng(111)
    x = mixture(n, d, n_comp=nlist, seed=112)
    ids = np.arange(n, dtype=np.uint64)
    cents = x[:nlist].copy()
    ages = np.where(rng.random(n) < 2 / 3, 1 * DAY, 30 * DAY)  # a third historical
    ages[rng.random(n) < 0.05] = 6.5 * DAY  # recent now, due for migration half a day later
    levels = orc.rng_levels(113, n)
    kw = dict(max_connections=8, max_connections_layer_0=16, ef_construction=40, n_clusters=nlist, n_probe=4)

    def make(cls, *a):
        h = cls(*a, **kw)
        h.set_ivf_centroids(cents)
        for i in range(n):
            h.insert_with_timestamp(int(ids[i]), x[i], now - ages[i], now, int(levels[i]))
        return h

    g = make(fv.HybridIndex, ctx)
    g.hnsw().scan_cutoff = 0  # the recent part by the masked traversal: what the oracle walks after the deletes
    later = now + 1 * DAY  # the first search migrates the due rows; every mask is built for the rows as they then lie
    sets = [ids[rng.random(n) < 0.4], None, ids[:0], ids[rng.random(n) < 0.05]]
    B = 24
    q = mixture(B, d, n_comp=nlist, seed=114)
    group = np.arange(B) % len(sets)
    hist_before = g.historical_count()
    oracles = {}
    for k, ef in ((10, 50), (300, 320)):
        got = g.search_allowed_groups(q, k, sets, group, now=later, hnsw_ef=ef, ivf_n_probe=4)
        assert g.historical_count() > hist_before, "the search migrated rows first"
        for gi, allowed in enumerate(sets):
            idx = np.flatnonzero(group == gi)
            if gi not in oracles:
                o = make(orc.HybridIndex)
                o.batch_search(q[:1], 1, now=later, hnsw_ef=50, ivf_n_probe=4)  # the migration step
                keep = set(int(i) for i in (ids if allowed is None else allowed))
                for i in ids:
                    if int(i) not in keep:
                        for part in (o.hnsw(), o.ivf()):  # a migrated row lives in both parts
                            try:
                                part.mark_deleted(int(i))
                            except orc.VectorNotFound:
                                pass
                oracles[gi] = o
            ref = oracles[gi].batch_search(q[idx], k, now=later, hnsw_ef=ef, ivf_n_probe=4)
            same(rows_of(got, idx), ref, f"k {k}, group {gi} against the oracle")
            one = (g.search(q[idx], k, now=later, hnsw_ef=ef, ivf_n_probe=4) if allowed is None else
                   g.search_allowed(q[idx], k, allowed, now=later, hnsw_ef=ef, ivf_n_probe=4))
            same_blocks(rows_of(got, idx), (one.ids, one.distances, one.counts), f"k {k}, group {gi} against search_allowed")
    # the recent part scanned (the default cutoff): still what search_allowed returns, group by group
    g.hnsw().scan_cutoff = 8192
    got = g.search_allowed_groups(q, 10, sets, group, now=later, hnsw_ef=50, ivf_n_probe=4)
    for gi, allowed in enumerate(sets):
        idx = np.flatnonzero(group == gi)
        one = (g.search(q[idx], 10, now=later, hnsw_ef=50, ivf_n_probe=4) if allowed is None else
               g.search_allowed(q[idx], 10, allowed, now=later, hnsw_ef=50, ivf_n_probe=4))
        same_blocks(rows_of(got, idx), (one.ids, one.distances, one.counts), f"scanned recent part, group {gi}")
