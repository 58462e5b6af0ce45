"""GPU: HNSWIndex(row_dtype="f16") — the graph's row store keeps IEEE fp16.  The index is given the
unrounded rows, rounds them once at the door, and must then be the CPU oracle given `x.astype(float16).astype(float32)`:
the same graph node for node from the device insert, the same ids and bit-identical f32 distances from every search
path, through every kernel instantiation (128-dim block counts 1..8, FULL or bounds-checked, sorted-register and
restated-heap searches, hashed visited set, the exact-heap kernel's own row loaders above 1024 dimensions)."""
import functools

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture
from test_gpu_device_insert import same_graph, same_results

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


def rounded(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def same(g, ref):
    oi, od, oc = ref
    assert np.array_equal(g.counts, oc), f"hit counts differ: {g.counts[:8]} vs {oc[:8]}"
    for b in range(len(g)):
        n = int(oc[b])
        assert np.array_equal(g.ids[b, :n], oi[b, :n]), f"query {b}: ids differ"
        assert np.array_equal(bits(g.distances[b, :n]), bits(od[b, :n])), f"query {b}: distances not bit-identical"


# n, d, M, M0, efc: one per 128-dim block count, FULL (384, 768) or bounds-checked, and the restated-heap insert (efc 300)
CASES = [
    (400, 16, 6, 12, 40),
    (500, 200, 8, 16, 64),
    (400, 300, 8, 16, 64),
    (500, 384, 16, 32, 200),
    (300, 512, 16, 32, 100),
    (300, 700, 8, 16, 64),
    (300, 768, 16, 32, 200),
    (250, 1024, 8, 16, 64),
    (350, 40, 4, 8, 300),
]


@functools.lru_cache(maxsize=None)
def reference(n, d, M, M0, efc):
    """the case's data and the oracle built ONCE on the rounded rows (shared by both insert modes; only searched after)"""
    orc.build()
    seed = d + n
    x = mixture(n, d, n_comp=8, seed=seed)
    xr = rounded(x)
    assert (bits(xr) != bits(x)).any()
    ids = np.arange(n, dtype=np.uint64) + 7
    levels = orc.rng_levels(seed, n)
    oh = orc.HNSWIndex(M, M0, efc, seed=seed)
    oh.batch_insert(ids, xr, levels)
    q = mixture(25, d, n_comp=8, seed=seed + 100)  # queries stay f32: not rounded
    want = {ef: oh.batch_search(q, 10, ef) for ef in (50, 100)}
    return x, xr, ids, levels, oh, q, want


@pytest.mark.parametrize("n,d,M,M0,efc", CASES)
@pytest.mark.parametrize("mode", [1, 2])
def test_device_insert_builds_the_oracles_graph_on_the_rounded_rows(fv, ctx, n, d, M, M0, efc, mode):
    x, xr, ids, levels, oh, q, want = reference(n, d, M, M0, efc)
    gh = fv.HNSWIndex(ctx, M, M0, efc, seed=d + n, row_dtype="f16")
    assert gh.row_dtype == "f16"
    gh.set_device_insert(True, mode)
    assert gh.batch_insert(ids, x, levels) == (n, 0)
    st = gh.insert_stats()
    assert st["host_path_inserts"] == 0 and st["n_done"] == n
    same_graph(gh, oh)
    for device in (True, False):
        gh.set_device_traversal(device)
        for ef in (50, 100):  # the sorted-register kernel, the exact-heap kernel
            same_results(gh.search(q, 10, ef), want[ef])
    assert gh.device_fallbacks() == 0
    assert np.array_equal(bits(gh.get_vector_by_id(int(ids[3]))), bits(xr[3]))
    assert gh.store_bytes() == n * ((d + 3) // 4 * 4) * 2


def test_hashed_visited_set_at_384(fv, ctx):
    n, d, M, M0, efc = CASES[3]
    x, xr, ids, levels, oh, q, want = reference(n, d, M, M0, efc)
    gh = fv.HNSWIndex(ctx, M, M0, efc, seed=d + n, row_dtype="f16")
    gh.set_insert_visited(2, 256)
    gh.set_device_insert(True, 2)
    assert gh.batch_insert(ids, x, levels) == (n, 0)
    st = gh.insert_stats()
    assert st["hashed_inserts"] > 0
    if st["host_path_inserts"]:  # an insert whose search fills the 256 slots is linked by the host algorithm: same graph
        assert st["visited_overflows"] >= st["host_path_inserts"]
    same_graph(gh, oh)
    same_results(gh.search(q, 10, 50), want[50])


def test_above_1024_dimensions_the_exact_heap_kernel_reads_half_rows(fv, ctx):
    # the device insert stops at 1024 dimensions: the host algorithm links (every hop scored on the fp16 store), and the
    # searches run the exact-heap kernel with its own row loaders
    n, d = 250, 1100
    x = mixture(n, d, n_comp=8, seed=1100)
    xr = rounded(x)
    ids = np.arange(n, dtype=np.uint64)
    levels = orc.rng_levels(1100, n)
    gh, oh = fv.HNSWIndex(ctx, 8, 16, 64, seed=1, row_dtype="f16"), orc.HNSWIndex(8, 16, 64, seed=1)
    assert gh.batch_insert(ids, x, levels) == (n, 0)
    oh.batch_insert(ids, xr, levels)
    assert gh.insert_stats()["host_path_inserts"] == n
    same_graph(gh, oh)
    q = mixture(20, d, n_comp=8, seed=1101)
    for device in (True, False):
        gh.set_device_traversal(device)
        for ef in (50, 100):
            same_results(gh.search(q, 10, ef), oh.batch_search(q, 10, ef))
    assert gh.device_fallbacks() == 0


def test_rows_that_are_equal_after_rounding_tie_like_the_reference(fv, ctx):
    # every row three times AFTER rounding: two of the copies differ from the first before it (by less than half a unit
    # in the last place of an fp16), so the index meets the ties only because it rounds
    n, d = 600, 64
    base = rounded(mixture(n // 3, d, n_comp=3, seed=31))
    up, down = base * np.float32(1 + 2.0 ** -13), base * np.float32(1 - 2.0 ** -13)
    up, down = np.where(rounded(up) == base, up, base), np.where(rounded(down) == base, down, base)
    assert (up != base).mean() > 0.9 and (down != base).mean() > 0.9
    x = np.concatenate([base, up, down]).astype(np.float32)
    xr = rounded(x)
    assert np.array_equal(bits(xr), bits(np.tile(base, (3, 1))))
    ids = np.arange(n, dtype=np.uint64)
    levels = orc.rng_levels(31, n)
    gh, oh = fv.HNSWIndex(ctx, 6, 12, 48, seed=31, row_dtype="f16"), orc.HNSWIndex(6, 12, 48, seed=31)
    gh.set_device_insert(True, 1)
    assert gh.batch_insert(ids, x, levels) == (n, 0)
    oh.batch_insert(ids, xr, levels)
    assert gh.insert_stats()["tie_restarts"] > 0
    same_graph(gh, oh)
    q = np.concatenate([mixture(20, d, n_comp=3, seed=32), x[5:9]])  # some queries are stored rows, before rounding
    for device in (True, False):
        gh.set_device_traversal(device)
        same_results(gh.search(q, 10, 50), oh.batch_search(q, 10, 50))
    served, again = gh.tie_restarts()
    assert again > 0, "the sorted-register search met equal distances and ran the restated heaps"


def brute_force(xr, nodes, ids, q, k):
    B = q.shape[0]
    oi = np.full((B, k), np.uint64(2 ** 64 - 1), np.uint64)
    od = np.full((B, k), np.inf, np.float32)
    oc = np.zeros(B, np.uint32)
    for b in range(B):
        dist = orc.l2_batch(q[b], xr[nodes])
        order = np.lexsort((nodes, bits(dist)))[:k]  # distance bits, then node index
        oc[b] = order.size
        oi[b, :order.size] = ids[nodes[order]]
        od[b, :order.size] = dist[order]
    return oi, od, oc


def test_deleted_and_tall_nodes_allowed_search_and_vacuum(fv, ctx):
    n, d, n0 = 500, 20, 440
    x = mixture(n, d, n_comp=4, seed=41)
    xr = rounded(x)
    ids = np.arange(n, dtype=np.uint64) + 100
    levels = orc.rng_levels(41, n).copy()
    levels[300] = 17  # above the layers one workgroup keeps on chip: that node takes the host algorithm
    gh, oh = fv.HNSWIndex(ctx, 6, 12, 40, seed=41, row_dtype="f16"), orc.HNSWIndex(6, 12, 40, seed=41)
    gh.set_device_insert(True, 1)
    gh.batch_insert(ids[:200], x[:200], levels[:200])
    oh.batch_insert(ids[:200], xr[:200], levels[:200])
    dead = list(range(0, 200, 7))
    for i in dead:  # soft-deleted nodes are visited, never scored, never linked (src/hnsw/core.rs:511-513)
        gh.mark_deleted(int(ids[i]))
        oh.mark_deleted(int(ids[i]))
    gh.batch_insert(ids[200:n0], x[200:n0], levels[200:n0])
    oh.batch_insert(ids[200:n0], xr[200:n0], levels[200:n0])
    assert gh.insert_stats()["host_path_inserts"] == 1
    same_graph(gh, oh)
    q = mixture(20, d, n_comp=4, seed=42)
    for device in (True, False):
        gh.set_device_traversal(device)
        got = gh.search(q, 10, 50)
        same_results(got, oh.batch_search(q, 10, 50))
        assert not np.isin(got.ids, ids[dead]).any()
    gh.set_device_traversal(True)

    # search_allowed, on both sides of the scan cutoff
    rng = np.random.default_rng(43)
    allowed = ids[:n0][rng.random(n0) < 0.4]
    o2 = orc.HNSWIndex(6, 12, 40, seed=41)  # the oracle search filtered by the same set: the complement deleted
    o2.batch_insert(ids[:200], xr[:200], levels[:200])
    for i in dead:
        o2.mark_deleted(int(ids[i]))
    o2.batch_insert(ids[200:n0], xr[200:n0], levels[200:n0])
    keep = set(int(i) for i in allowed)
    for i in ids[:n0]:
        if int(i) not in keep and int(i) - 100 not in dead:
            o2.mark_deleted(int(i))
    gh.scan_cutoff = 0  # the masked traversal
    for k, ef in ((10, 50), (10, 100)):
        same(gh.search_allowed(q, k, ef, allowed), o2.batch_search(q, k, ef))
    gh.scan_cutoff = fv.HNSWIndex.SCAN_ALWAYS  # the exact scan of the allowed live nodes
    nodes = np.array(sorted(set(int(i) - 100 for i in allowed) - set(dead)), np.int64)
    for k in (10, 70):
        same(gh.search_allowed(q, k, 50, allowed), brute_force(xr, nodes, ids, q, k))
    gh.scan_cutoff = 8192

    # a resident vacuum: the rows move as halves
    before = gh.store_bytes()
    assert before == n0 * d * 2
    assert gh.vacuum() == oh.vacuum() == len(dead)
    assert gh.vacuum_info()["path"] == "resident"
    info = gh.vacuum_info()
    assert info["move_bytes"] == 2 * (n0 - len(dead)) * d * 2
    assert gh.store_rows() == gh.node_count() == n0 - len(dead)
    assert gh.store_bytes() == (n0 - len(dead)) * d * 2 < before
    same_graph(gh, oh)
    for i in range(n0):
        if i not in dead:
            assert np.array_equal(bits(gh.get_vector_by_id(int(ids[i]))), bits(xr[i])), i
    for device in (True, False):
        gh.set_device_traversal(device)
        same_results(gh.search(q, 10, 50), oh.batch_search(q, 10, 50))
    gh.set_device_traversal(True)
    # the rows in HBM moved whole: the exact scan of the store finds every row at distance zero from its rounded value
    live = np.array([i for i in range(n0) if i not in dead])
    gh.scan_cutoff = fv.HNSWIndex.SCAN_ALWAYS
    own = gh.search_allowed(xr[live], 1, 50, ids[live])
    assert np.array_equal(own.ids[:, 0], ids[live]) and np.all(own.distances[:, 0] == 0)
    gh.scan_cutoff = 8192
    # later inserts link against the moved rows and their edge distances
    assert gh.batch_insert(ids[n0:], x[n0:], levels[n0:]) == (n - n0, 0)
    oh.batch_insert(ids[n0:], xr[n0:], levels[n0:])
    assert gh.insert_stats()["host_path_inserts"] == 1
    same_graph(gh, oh)
    same_results(gh.search(q, 10, 50), oh.batch_search(q, 10, 50))


def test_a_row_that_rounds_to_infinity_is_refused(fv, ctx):
    n, d = 120, 24
    x = mixture(n, d, n_comp=4, seed=51)
    ids = np.arange(n, dtype=np.uint64)
    levels = orc.rng_levels(51, n)
    gh, oh = fv.HNSWIndex(ctx, 5, 10, 50, seed=9, row_dtype="f16"), orc.HNSWIndex(5, 10, 50, seed=9)
    assert gh.batch_insert(ids[:50], x[:50], levels[:50]) == (50, 0)
    bad = x[50].copy()
    bad[7] = 70000.0  # finite as f32, +Inf as fp16
    with pytest.raises(fv.NonFiniteInput) as e:
        gh.insert(int(ids[50]), bad, int(levels[50]))
    assert e.value.status == 9  # FVDB_E_NONFINITE
    assert gh.node_count() == 50 and gh.store_rows() == 50
    rest = x[50:].copy()
    rest[20, 3] = -70000.0
    assert gh.batch_insert(ids[50:], rest, levels[50:]) == (n - 51, 1)  # one failure, the rest linked
    keep = np.array([i for i in range(n) if i != 70])
    oh.batch_insert(ids[keep], rounded(x[keep]), levels[keep])
    same_graph(gh, oh)
    # 65504 is the largest half, and what rounds to it goes in
    top = x[70].copy()
    top[3] = 65519.0
    gh.insert(int(ids[70]), top, int(levels[70]))
    assert gh.get_vector_by_id(int(ids[70]))[3] == np.float32(65504.0)
    # the f32 index takes the same row as it is
    gf = fv.HNSWIndex(ctx, 5, 10, 50, seed=9)
    assert gf.row_dtype == "f32"
    gf.insert(1, bad, 0)
    assert gf.get_vector_by_id(1)[7] == np.float32(70000.0)
