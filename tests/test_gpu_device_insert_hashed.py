"""The device insert's `visited` set (src/hnsw/core.rs:469-554, visited: HashSet<VectorId>) as a hashed table of node
indices in LDS instead of a bitmap over every node of the graph (kernels_graph_build.h, Visited<true>): graphs beyond the
bitmap's reach stay on the device.  Whatever the form, the graph is the CPU oracle's node for node; a search that fills
the table hands that one insert to the host algorithm."""
import os
import sys

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture

pytestmark = pytest.mark.gpu

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


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


def pair(fv, ctx, M, M0, efc, seed):
    return fv.HNSWIndex(ctx, M, M0, efc, seed=seed), orc.HNSWIndex(M, M0, efc, seed=seed)


CASES = [  # n, d, M, M0, efc, seed: the shapes of test_gpu_device_insert.py
    (400, 16, 6, 12, 40, 1),
    (700, 100, 8, 16, 64, 2),
    (500, 384, 16, 32, 200, 3),
    (300, 768, 16, 32, 200, 4),
    (350, 40, 4, 8, 300, 5),
]


@pytest.mark.parametrize("n,d,M,M0,efc,seed", CASES)
@pytest.mark.parametrize("mode", [1, 2])
def test_hashed_visited_builds_the_oracles_graph(fv, ctx, n, d, M, M0, efc, seed, mode):
    x = mixture(n, d, n_comp=8, seed=seed)
    ids = np.arange(n, dtype=np.uint64) + 7
    levels = orc.rng_levels(seed, n)
    gh, oh = pair(fv, ctx, M, M0, efc, seed)
    gh.set_device_insert(True, mode)
    gh.set_insert_visited(2)
    assert gh.batch_insert(ids, x, levels) == (n, 0)
    oh.batch_insert(ids, x, levels)
    st = gh.insert_stats()
    assert st["host_path_inserts"] == 0 and st["n_done"] == n and st["hashed_inserts"] == n
    assert st["visited_overflows"] == 0 and 0 < st["visited_peak"] <= n
    if mode == 2:
        assert st["speculated_ok"] > 0 and st["commit_stops"] > 0
    same_graph(gh, oh)
    q = mixture(25, d, n_comp=8, seed=seed + 100)
    for device in (True, False):
        gh.set_device_traversal(device)
        same_results(gh.search(q, 10, 50), oh.batch_search(q, 10, 50))


def test_bitmap_and_hashed_agree_on_a_graph_large_enough_to_speculate(fv, ctx):
    # the C1 shape: speculated batches, validation's second looks (which mark whole rows in the visited set) included
    n, d, M, M0, efc, seed = 10000, 384, 16, 32, 200, 91
    x = mixture(n, d, n_comp=4096, seed=seed)
    ids = np.arange(n, dtype=np.uint64)
    levels = orc.rng_levels(seed, n)
    graphs, stats = [], []
    for visited in (1, 2):
        gh = fv.HNSWIndex(ctx, M, M0, efc, seed=seed)
        gh.set_insert_visited(visited)
        assert gh.batch_insert(ids, x, levels) == (n, 0)
        st = gh.insert_stats()
        assert st["host_path_inserts"] == 0 and st["hashed_inserts"] == (n if visited == 2 else 0)
        assert st["speculated_ok"] > n // 4
        graphs.append(gh)
        stats.append(st)
    info = graphs[1].insert_info()
    print(f"[hashed] 10K x 384 ef 200: table {info['table_slots']} slots, entries after a search: largest "
          f"{info['visited_peak']}, mean {info['visited_mean']:.0f}; adopted {stats[0]['speculated_ok']} (bitmap) / "
          f"{stats[1]['speculated_ok']} (hashed)")
    a, b = graphs[0].export_graph(), graphs[1].export_graph()
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert graphs[0].entry_point() == graphs[1].entry_point()
    oh = orc.HNSWIndex(M, M0, efc, seed=seed)
    oh.batch_insert(ids, x, levels)
    same_graph(graphs[1], oh)


def test_auto_switches_to_the_hashed_set_past_the_bitmaps_reach(fv, ctx, monkeypatch):
    n, d = 600, 32
    x = mixture(n, d, n_comp=5, seed=12)
    ids = np.arange(n, dtype=np.uint64)
    levels = orc.rng_levels(12, n)
    gh, oh = pair(fv, ctx, 8, 16, 80, 12)
    gh.batch_insert(ids[:200], x[:200], levels[:200])
    assert gh.insert_info()["representation"] == "bitmap" and gh.insert_stats()["hashed_inserts"] == 0
    monkeypatch.setenv("FVDB_BUILD_BITMAP_MAX_NODES", "256")
    assert gh.insert_info()["bitmap_max_nodes"] == 256     # 200 nodes: still the bitmap's
    assert gh.insert_info()["representation"] == "bitmap"
    gh.batch_insert(ids[200:], x[200:], levels[200:])
    assert gh.insert_info()["representation"] == "hashed"
    monkeypatch.delenv("FVDB_BUILD_BITMAP_MAX_NODES")
    assert gh.insert_info()["representation"] == "bitmap"  # the hook is read at every call
    oh.batch_insert(ids, x, levels)
    st = gh.insert_stats()
    assert st["host_path_inserts"] == 0 and st["hashed_inserts"] == 400 and st["n_done"] == n
    same_graph(gh, oh)
    q = mixture(20, d, n_comp=5, seed=13)
    same_results(gh.search(q, 10, 50), oh.batch_search(q, 10, 50))


def test_appended_but_unlinked_nodes_do_not_push_an_empty_index_onto_the_host(fv, ctx, monkeypatch, capfd):
    # batch_insert appends the whole run before it links: the node count is 600 from the first insert on
    n, d = 600, 32
    x = mixture(n, d, n_comp=5, seed=14)
    ids = np.arange(n, dtype=np.uint64)
    levels = orc.rng_levels(14, n)
    oh = orc.HNSWIndex(8, 16, 80, seed=14)
    oh.batch_insert(ids, x, levels)
    monkeypatch.setenv("FVDB_BUILD_BITMAP_MAX_NODES", "256")
    gh = fv.HNSWIndex(ctx, 8, 16, 80, seed=14)
    assert gh.batch_insert(ids, x, levels) == (n, 0)
    st = gh.insert_stats()
    assert st["host_path_inserts"] == 0 and st["hashed_inserts"] == n
    same_graph(gh, oh)
    # bitmap only: today's behaviour — the call is refused, the host algorithm links every node, and says so once
    capfd.readouterr()
    gb = fv.HNSWIndex(ctx, 8, 16, 80, seed=14)
    gb.set_insert_visited(1)
    assert gb.batch_insert(ids, x, levels) == (n, 0)
    st = gb.insert_stats()
    assert st["host_path_inserts"] == n and st["hashed_inserts"] == 0 and st["n_done"] == 0
    err = capfd.readouterr().err
    assert err.count("linked by the host algorithm") == 1 and "visited bitmap" in err
    assert gb.insert_info()["representation"] is None
    same_graph(gb, oh)


def test_a_visited_set_that_fills_sends_the_insert_to_the_host(fv, ctx):
    n, d = 800, 16
    x = mixture(n, d, n_comp=64, seed=15)   # (a few tight clusters would keep an ef = 100 search below 192 nodes)
    ids = np.arange(n, dtype=np.uint64)
    levels = orc.rng_levels(15, n)
    oh = orc.HNSWIndex(16, 32, 100, seed=15)
    oh.batch_insert(ids, x, levels)
    gh = fv.HNSWIndex(ctx, 16, 32, 100, seed=15)
    gh.set_insert_visited(2, 256)   # 192 entries: an ef = 100 search outgrows that once the graph has a few hundred nodes
    assert gh.batch_insert(ids, x, levels) == (n, 0)
    assert gh.insert_info()["table_slots"] == 256
    st = gh.insert_stats()
    print(f"[hashed] 256 slots, 800 x 16, ef 100: {st['visited_overflows']} of {n} inserts filled the set (host algorithm), "
          f"largest set {st['visited_peak']}")
    assert st["visited_overflows"] > 0 and st["host_path_inserts"] == st["visited_overflows"]
    assert st["hashed_inserts"] + st["host_path_inserts"] == n and 192 < st["visited_peak"] < 256
    same_graph(gh, oh)
    q = mixture(20, d, n_comp=64, seed=16)
    same_results(gh.search(q, 10, 50), oh.batch_search(q, 10, 50))
    g2 = fv.HNSWIndex(ctx, 16, 32, 100, seed=15)
    g2.set_insert_visited(2)        # default table
    assert g2.batch_insert(ids, x, levels) == (n, 0)
    st = g2.insert_stats()
    assert st["visited_overflows"] == 0 and st["host_path_inserts"] == 0 and st["hashed_inserts"] == n
    same_graph(g2, oh)
    with pytest.raises(ValueError):
        g2.set_insert_visited(2, 300)   # not a power of two
    with pytest.raises(ValueError):
        g2.set_insert_visited(3)


def test_hashed_visited_skips_deleted_nodes_and_handles_tall_nodes(fv, ctx):
    n, d = 500, 20
    x = mixture(n, d, n_comp=4, seed=41)
    ids = np.arange(n, dtype=np.uint64)
    levels = orc.rng_levels(41, n).copy()
    levels[300] = 17                 # above the layers one workgroup keeps on chip: that node takes the host algorithm
    gh, oh = pair(fv, ctx, 6, 12, 40, 41)
    gh.set_device_insert(True, 1)
    gh.set_insert_visited(2)
    gh.batch_insert(ids[:200], x[:200], levels[:200])
    oh.batch_insert(ids[:200], x[:200], levels[:200])
    for i in range(0, 200, 7):       # soft-deleted nodes are visited (they take a slot of the table), never scored
        gh.mark_deleted(int(ids[i]))
        oh.mark_deleted(int(ids[i]))
    gh.batch_insert(ids[200:], x[200:], levels[200:])
    oh.batch_insert(ids[200:], x[200:], levels[200:])
    st = gh.insert_stats()
    assert st["host_path_inserts"] == 1 and st["hashed_inserts"] == n - 1 and st["visited_overflows"] == 0
    same_graph(gh, oh)
    q = mixture(20, d, n_comp=4, seed=42)
    same_results(gh.search(q, 10, 50), oh.batch_search(q, 10, 50))


def test_hashed_visited_duplicate_vectors_tie_like_the_reference(fv, ctx):
    # every admission ties: the restated heaps and the hashed set together
    n, d = 600, 64
    base = mixture(60, d, n_comp=3, seed=31)
    x = np.tile(base, (10, 1))
    ids = np.arange(n, dtype=np.uint64)
    levels = orc.rng_levels(31, n)
    gh, oh = pair(fv, ctx, 6, 12, 48, 31)
    gh.set_device_insert(True, 1)
    gh.set_insert_visited(2)
    gh.batch_insert(ids, x, levels)
    oh.batch_insert(ids, x, levels)
    st = gh.insert_stats()
    assert st["tie_restarts"] > 0 and st["hashed_inserts"] == n
    same_graph(gh, oh)


def test_randomised_sequences_with_the_hashed_set_forced(fv, ctx):
    # the case lists of test_gpu_device_insert.py / test_gpu_host_mirror.py's sweeps, `visited` hashed throughout
    sys.path.insert(0, TOOLS)
    import hnsw_ops_fuzz
    import hybrid_ops_fuzz
    import insert_fuzz
    rng = np.random.default_rng(1)
    failed = [("ops", c) for c in range(12)
              if hnsw_ops_fuzz.one_case(fv, orc, ctx, rng, c, c if c in (1, 4, 7, 10, 11) else -2, visited="hashed")]
    rng = np.random.default_rng(1)
    failed += [("hybrid", c) for c in range(12)
               if hybrid_ops_fuzz.one_case(fv, orc, ctx, rng, c, c if c % 3 == 2 else -2, visited="hashed")]
    rng = np.random.default_rng(1)
    failed += [("insert", c) for c in range(24)
               if insert_fuzz.one_case(fv, orc, ctx, rng, c, c if c in (3, 11, 17, 23) else -2, visited="hashed")]
    assert not failed, failed


def test_hybrid_bulk_insert_reaches_the_hashed_set(fv, ctx, monkeypatch):
    # HybridIndex::bulk_insert builds the recent part's graph with sequential device inserts: past the bitmap's reach
    # (hook) they run hashed, not on the host, and leave the graph and the answers of the build that used the bitmap
    n, d, nlist = 900, 24, 8
    x = mixture(n, d, n_comp=6, seed=17)
    ids = np.arange(n, dtype=np.uint64)
    now, day = 1000 * 86400.0, 86400.0
    ts = np.where(np.arange(n) % 3 == 0, now - 30 * day, now - 1 * day).astype(np.float64)
    kw = dict(max_connections=8, max_connections_layer_0=16, ef_construction=60, n_clusters=nlist, n_probe=4, hnsw_seed=5)
    q = mixture(16, d, n_comp=6, seed=18)
    built = []
    for hook in (False, True):
        if hook:
            monkeypatch.setenv("FVDB_BUILD_BITMAP_MAX_NODES", "256")
        gi = fv.HybridIndex(ctx, **kw)
        gi.set_ivf_centroids(x[:nlist].copy())
        gi.bulk_insert(ids, x, ts, now)
        st = gi.hnsw().insert_stats()
        assert gi.recent_count() == 600 and st["host_path_inserts"] == 0
        assert st["hashed_inserts"] == (600 if hook else 0)
        built.append((gi.hnsw().export_graph(), gi.search(q, 10, now=now, hnsw_ef=50, ivf_n_probe=4)))
    for u, v in zip(built[0][0], built[1][0]):
        assert np.array_equal(u, v)
    r0, r1 = built[0][1], built[1][1]
    assert np.array_equal(r0.counts, r1.counts) and np.array_equal(r0.ids, r1.ids)
    assert np.array_equal(bits(r0.distances), bits(r1.distances))


def test_insert_info_names_the_limit_it_switches_at(fv, ctx, monkeypatch):
    n, d = 300, 16
    x = mixture(n, d, n_comp=3, seed=19)
    ids = np.arange(n, dtype=np.uint64)
    levels = orc.rng_levels(19, n)
    gh = fv.HNSWIndex(ctx, 16, 32, 200, seed=19)
    with pytest.raises(RuntimeError):
        gh.insert_info()             # no device graph before the first insert
    gh.batch_insert(ids[:100], x[:100], levels[:100])
    info = gh.insert_info()
    # ef_construction 200: the fixed tables leave the bitmap 63 280 bytes beside the smallest `candidates` heap
    assert info["mode"] == "auto" and info["representation"] == "bitmap" and info["bitmap_max_nodes"] == 63280 * 8
    assert info["table_slots"] == 0 and info["cand_cap"] == 4096 and info["lds_bytes"] <= 160 * 1024
    gh.set_insert_visited("hashed")
    info = gh.insert_info()
    assert info["representation"] == "hashed" and info["table_slots"] == 8192 and info["cand_cap"] == 4096
    assert info["lds_bytes"] <= 160 * 1024
    gh.set_insert_visited("auto")
    # a budget that holds the hashed set with a smaller table, and one that holds nothing
    monkeypatch.setenv("FVDB_BUILD_LDS_LIMIT", str(120 * 1024))
    monkeypatch.setenv("FVDB_BUILD_BITMAP_MAX_NODES", "50")
    info = gh.insert_info()
    assert info["representation"] == "hashed" and 256 <= info["table_slots"] < 8192 and info["cand_cap"] >= 512
    assert info["lds_bytes"] <= 120 * 1024
    gh.batch_insert(ids[100:200], x[100:200], levels[100:200])
    monkeypatch.setenv("FVDB_BUILD_LDS_LIMIT", "4096")
    assert gh.insert_info()["representation"] is None
    monkeypatch.delenv("FVDB_BUILD_LDS_LIMIT")
    monkeypatch.delenv("FVDB_BUILD_BITMAP_MAX_NODES")
    gh.batch_insert(ids[200:], x[200:], levels[200:])
    st = gh.insert_stats()
    assert st["host_path_inserts"] == 0 and st["hashed_inserts"] == 100 and st["n_done"] == n
    oh = orc.HNSWIndex(16, 32, 200, seed=19)
    oh.batch_insert(ids, x, levels)
    same_graph(gh, oh)
