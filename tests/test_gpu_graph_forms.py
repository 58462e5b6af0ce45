"""GPU: the traversal forms the small graphs of the other tests never select (fvdb_graph.cpp, search_plan).

One bit per node as `visited` (hnsw_search_fast_kernel<NB, R, /*BYTES=*/false, RT>: atomicOr, a log clear that zeroes whole
words, its own branch of the whole-map clear) serves a batch whose byte maps would pass 1 GiB: ceil64(n) * max(B, 1024)
> 2^30.  N = 32 832 nodes and B = 32 771 queries cross that; the same graph at B = 1024 stays on the byte map.  A
synthetic adjacency (_graph_forms.py) is restored into the index and into the CPU oracle, and every comparison is bit
for bit — ids, distance bits, counts: the big batch against the same queries in 1024-row batches (the other form), and
both against the oracle.  HNSWIndex.search_info says which form a search takes, so a threshold that moves fails these
tests instead of emptying them.  Also here: f32 rows above 1024 dimensions (the exact-heap kernel's f32 loader)."""
import functools
import gc

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits
from _graph_forms import synthetic_graph
from test_graph_forms_data import B, M, M0, N, N_WIDER, ceil64, queries

pytestmark = pytest.mark.gpu

K, EF = 10, 50
SMALL = 1024
BLOCKS = {100: (1, 16), 200: (2, 16), 384: (3, 16), 500: (4, 12), 768: (6, 8), 1000: (8, 6)}  # d: nb128, rows per round
SAMPLE = np.r_[0:256, B - 256:B]  # oracle rows: the first 256, the last 256 (the stored-row and the nudged queries are in these)


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()
    gc.collect()


def rounded(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=1)
def world(n, d, copies):
    """the graph of (n, d, copies) and its queries per row type, made once and left unchanged"""
    g = synthetic_graph(n, d, M, M0, seed=d + copies, copies=copies)
    x = g[0]
    b = B if n >= N else 200
    q = {"f32": queries(x, d, seed=d + copies, b=b), "f16": queries(rounded(x), d, seed=d + copies, b=b)}
    for a in (x, q["f32"], q["f16"]):
        a.setflags(write=False)
    return g, q


def pair(fv, ctx, n, d, dtype, copies=1):
    """the same graph in the index and in the oracle (which gets the rounded rows of an f16 index)"""
    (x, ids, levels, off, nbrs, entry), q = world(n, d, copies)
    gh, oh = fv.HNSWIndex(ctx, M, M0, 200, seed=1, row_dtype=dtype), orc.HNSWIndex(M, M0, 200, seed=1)
    gh.restore(ids, x, levels, off, nbrs, entry)
    oh.restore(ids, x if dtype == "f32" else rounded(x), levels, off, nbrs, entry)
    return gh, oh, ids, q[dtype]


class Res:
    def __init__(self, ids, distances, counts):
        self.ids, self.distances, self.counts = ids, distances, counts


def in_batches(search, q, size=SMALL):
    parts = [search(q[i:i + size]) for i in range(0, q.shape[0], size)]
    return Res(*(np.concatenate([getattr(p, f) for p in parts]) for f in ("ids", "distances", "counts")))


def same(a, b, rows=slice(None)):
    assert np.array_equal(a.counts[rows], b.counts[rows]), "hit counts differ"
    bad = np.flatnonzero((a.ids[rows] != b.ids[rows]).any(axis=1))
    assert bad.size == 0, f"ids differ in {bad.size} queries, first {bad[:8]}"
    bad = np.flatnonzero((bits(a.distances[rows]) != bits(b.distances[rows])).any(axis=1))
    assert bad.size == 0, f"distance bits differ in {bad.size} queries, first {bad[:8]}"


def same_as_oracle(got, oh, q, k, ef, rows=SAMPLE):
    oi, od, oc = oh.batch_search(q[rows], k, ef)
    assert np.array_equal(got.counts[rows], oc), "hit counts differ from the oracle's"
    for j, b in enumerate(rows):
        c = int(oc[j])
        assert np.array_equal(got.ids[b, :c], oi[j, :c]), f"query {b}: ids differ from the oracle's"
        assert np.array_equal(bits(got.distances[b, :c]), bits(od[j, :c])), f"query {b}: distances not bit-identical"


def three_ways(gh, oh, q, k, ef):
    """the big batch (bit map), the same rows in 1024-row batches (byte map), the oracle on the sample"""
    big = gh.search(q, k, ef)
    same(big, in_batches(lambda part: gh.search(part, k, ef), q))
    same_as_oracle(big, oh, q, k, ef)
    return big


def expect_forms(gh, ef, kernel, nb128, rows_per_round):
    big, small = gh.search_info(B, ef), gh.search_info(SMALL, ef)
    assert big["visited"] == "bits" and small["visited"] == "bytes", (big, small)
    n = gh.node_count()
    assert big["visited_bytes"] == B * ((n + 31) // 32) * 4 and small["visited_bytes"] == SMALL * ceil64(n)
    for info in (big, small):
        assert (info["kernel"], info["nb128"], info["rows_per_round"]) == (kernel, nb128, rows_per_round), info
        assert info["nearest_in_registers"] == (ef <= 63) and info["tcap"] == 8192
        assert info["lds_bytes"] <= 160 * 1024 and info["cand_cap"] == max(1024, 8 * ef) and info["spill_cap"] == 8192


@pytest.mark.parametrize("d,dtype", [(d, t) for d in BLOCKS for t in ("f32", "f16")])
def test_both_visited_forms_at_every_block_count(fv, ctx, d, dtype):
    gh, oh, ids, q = pair(fv, ctx, N, d, dtype)
    nb128, R = BLOCKS[d]
    expect_forms(gh, EF, "sorted_register", nb128, R)
    three_ways(gh, oh, q, K, EF)
    if d in (100, 384):
        expect_forms(gh, 100, "exact_heap", nb128, 0)  # its word stride differs between the two forms
        three_ways(gh, oh, q, K, 100)
        expect_forms(gh, 1, "sorted_register", nb128, R)
        three_ways(gh, oh, q, 1, 1)
        expect_forms(gh, 63, "sorted_register", nb128, R)
        three_ways(gh, oh, q, K, 63)
        dead = ids[np.random.default_rng(d).choice(N, N * 3 // 100, replace=False)]
        for i in dead:  # any_deleted: visited, never scored, and the result is filtered once more at the end
            gh.mark_deleted(int(i))
            oh.mark_deleted(int(i))
        big = three_ways(gh, oh, q, K, EF)
        assert not np.isin(big.ids, dead).any()
    assert gh.device_fallbacks() == 0
    del gh
    gc.collect()


@pytest.mark.parametrize("d,dtype", [(100, "f32"), (384, "f16")])
def test_ties_restart_from_a_clean_bit_map(fv, ctx, d, dtype):
    gh, oh, ids, q = pair(fv, ctx, N, d, dtype, copies=3)
    expect_forms(gh, EF, "sorted_register", *BLOCKS[d])
    small = in_batches(lambda part: gh.search(part, K, EF), q)
    before = gh.tie_restarts()[1]
    big = gh.search(q, K, EF)
    assert gh.tie_restarts()[1] > before, "no query of the big batch met equal distances: the restart did not run"
    same(big, small)
    same_as_oracle(big, oh, q, K, EF)
    same(gh.search(q, K, EF), big)  # the restarts left their maps clean again
    assert gh.device_fallbacks() == 0
    del gh
    gc.collect()


def test_log_overflow_clears_the_whole_bit_map(fv, ctx, monkeypatch):
    d = 100
    gh, oh, ids, q = pair(fv, ctx, N, d, "f32")
    want = {ef: in_batches(lambda part: gh.search(part, K, ef), q) for ef in (EF, 100)}
    monkeypatch.setenv("FVDB_GRAPH_TCAP", "40")  # read per call: a log of 40 nodes, every query outgrows it
    info = gh.search_info(B, EF)
    assert info["tcap"] == 40 and info["visited"] == "bits" and gh.search_info(B, 100)["visited"] == "bits"
    for ef in (EF, 100):
        same(gh.search(q, K, ef), want[ef])
    assert gh.device_fallbacks() == 0
    monkeypatch.delenv("FVDB_GRAPH_TCAP")
    assert gh.search_info(B, EF)["tcap"] == 8192
    for ef in (EF, 100):
        same(gh.search(q, K, ef), want[ef])
    same_as_oracle(want[EF], oh, q, K, EF, rows=SAMPLE[:64])
    del gh
    gc.collect()


def test_changing_form_on_one_graph_and_one_slot(fv, ctx):
    d = 100  # a multiple of 4: slot 1 is allowed
    for n in (N, N_WIDER):  # the second graph has another `words`
        gh, oh, ids, q = pair(fv, ctx, n, d, "f32")
        assert gh.search_info(B, EF)["visited"] == "bits" and gh.search_info(SMALL, EF)["visited"] == "bytes"
        assert gh.search_info(33, EF)["visited"] == "bytes"
        first = {}
        for size in (SMALL, B, SMALL, B, 33):
            got = gh.search(q[:size], K, EF)
            same(got, first.setdefault(size, got))
        same(first[B], first[SMALL], rows=slice(0, SMALL))
        same(first[B], first[33], rows=slice(0, 33))
        same_as_oracle(first[B], oh, q, K, EF, rows=SAMPLE[::4])
        q_dev = ctx.upload(q)
        try:
            for size in (SMALL, B, SMALL, B, 33):
                gh.search_dev_begin(1, q_dev, size, d, K, EF)
                same(gh.search_dev_end(1), first[size])
        finally:
            ctx.free(q_dev)
        assert gh.device_fallbacks() == 0
        del gh
        gc.collect()


def test_allow_set_mask_in_the_bit_map_form(fv, ctx):
    d = 100
    gh, oh, ids, q = pair(fv, ctx, N, d, "f32")
    gh.scan_cutoff = 0  # the masked traversal serves the query, not the scan of the allowed nodes
    allowed = ids[np.random.default_rng(7).random(N) < 0.5]
    assert gh.search_info(B, EF)["visited"] == "bits" and gh.search_info(SMALL, EF)["visited"] == "bytes"
    big = gh.search_allowed(q, K, EF, allowed)
    same(big, in_batches(lambda part: gh.search_allowed(part, K, EF, allowed), q))
    assert np.isin(big.ids[big.counts == K], allowed).all()
    for i in np.setdiff1d(ids, allowed):  # the oracle after deleting the complement
        oh.mark_deleted(int(i))
    same_as_oracle(big, oh, q, K, EF, rows=np.r_[0:128, B - 128:B])
    assert gh.device_fallbacks() == 0
    del gh
    gc.collect()


def test_f32_rows_above_1024_dimensions(fv, ctx):
    n, d = 2000, 1100
    gh, oh, ids, q = pair(fv, ctx, n, d, "f32")
    for ef, in_registers in ((EF, True), (100, False)):
        info = gh.search_info(q.shape[0], ef)
        assert info["kernel"] == "exact_heap" and info["nearest_in_registers"] == in_registers, info
        assert info["nb128"] == 9 and info["rows_per_round"] == 0 and info["visited"] == "bytes"
        want = oh.batch_search(q, K, ef)
        for device in (True, False):
            gh.set_device_traversal(device)
            got = gh.search(q, K, ef)
            assert np.array_equal(got.counts, want[2]) and np.array_equal(got.ids, want[0])
            assert np.array_equal(bits(got.distances), bits(want[1]))
    assert gh.device_fallbacks() == 0
