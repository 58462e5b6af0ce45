"""GPU: HNSWIndex.vacuum as one device job on the adjacency in HBM (fvdb_graph_vacuum; src/hnsw/operations.rs:176-200)
against the CPU oracle: lists pruned in order, survivors renumbered densely, store rows given back, edge distances kept.

The oracle has no filtered search: "the oracle with the complement deleted" is a second oracle index with every id
outside the allow-set soft-deleted.  That holds for the masked traversal.  An allow-set at or below scan_cutoff is
answered by the exact scan, which by design is not the traversal's answer: its reference is the
oracle's l2_batch over the allowed live rows, best k by (distance bits, node index) — the order a renumbering that
keeps the survivors' relative order must not disturb."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture

pytestmark = pytest.mark.gpu

N, D, M, M0, EFC = 3000, 32, 8, 16, 40
EXTRA = 400
E_INVALID = 6  # FVDB_E_INVALID (include/fvdb.h)


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


def same_answers(a, b):
    assert np.array_equal(a.counts, b.counts) and np.array_equal(a.ids, b.ids)
    assert np.array_equal(bits(a.distances), bits(b.distances))


def same_graph(g, o):
    """ids in order, levels, every list with the same members in the same order; returns (nodes, edges)."""
    gi, lv, off, nb = g.export_graph()
    assert gi.size == o.node_count() == g.node_count()
    slot = 0
    for r, l in zip(gi.tolist(), lv.tolist()):
        assert o.level(r) == l
        for layer in range(l + 1):
            assert nb[int(off[slot]):int(off[slot + 1])].tolist() == o.neighbors(r, layer), f"node {r} layer {layer}"
            slot += 1
    assert g.entry_point() == o.entry_point()
    return gi, int(nb.size)


def same_searches(g, o, q):
    for dev in (True, False):
        g.set_device_traversal(dev)
        for k, ef in ((5, 5), (10, 50), (10, 64), (20, 120)):
            same(g.search(q, k, ef), o.batch_search(q, k, ef))
    g.set_device_traversal(True)


def dataset(seed, n=N + EXTRA, d=D):
    x = mixture(n, d, n_comp=8, seed=seed)
    ids = np.arange(n, dtype=np.uint64) * 5 + 11
    levels = orc.rng_levels(seed, n).astype(np.int64)
    levels[7::97] = 3  # several nodes on layers 1-3 whatever the draw gave
    levels[5::53] = 2
    levels[3::31] = np.maximum(levels[3::31], 1)
    return x, ids, levels


def pair(fv, ctx, seed, n=N, **kw):
    x, ids, levels = dataset(seed)
    g = fv.HNSWIndex(ctx, M, M0, EFC, seed=seed, **kw)
    o = orc.HNSWIndex(M, M0, EFC, seed=seed)
    assert g.batch_insert(ids[:n], x[:n], levels[:n]) == (n, 0)  # on the device: the host never held these lists
    o.batch_insert(ids[:n], x[:n], levels[:n])
    assert g.insert_stats()["host_path_inserts"] == 0
    return g, o, x, ids, levels


def pick_dead(o, ids, levels, n, seed, frac=0.15, gone=()):
    """~frac of the nodes, upper-layer nodes and the highest row among them, never the entry point (nor a row in `gone`)."""
    rng = np.random.default_rng(seed)
    entry = o.entry_point()
    rows = set(rng.choice(n, int(frac * n), replace=False).tolist())
    rows |= {n - 1}
    rows |= set(np.flatnonzero(levels[:n] >= 1)[::9].tolist())
    rows |= set(np.flatnonzero(levels[:n] >= 3)[:2].tolist())
    dead = sorted(r for r in rows if int(ids[r]) != entry and r not in gone)
    assert entry not in set(int(ids[r]) for r in dead)
    assert gone or (any(levels[r] >= 2 for r in dead) and n - 1 in dead)
    return dead


def delete(g, o, ids, rows):
    for r in rows:
        g.mark_deleted(int(ids[r]))
        o.mark_deleted(int(ids[r]))


# ---- 1. - 3. one resident vacuum: parity, what crossed the host link, what was reclaimed -----------------------------
@pytest.fixture(scope="module")
def vacuumed(fv, ctx):
    g, o, x, ids, levels = pair(fv, ctx, seed=101)
    dead = pick_dead(o, ids, levels, N, seed=1)
    delete(g, o, ids, dead)
    q = mixture(32, D, n_comp=8, seed=102)
    same(g.search(q, 10, 50), o.batch_search(q, 10, 50))  # (also: the device graph is current)
    before = dict(upload=g.insert_stats()["graph_upload_bytes"], store=g.store_rows(), nodes=g.node_count())
    removed = g.vacuum()
    return dict(g=g, o=o, x=x, ids=ids, levels=levels, dead=dead, q=q, before=before, removed=removed,
                o_removed=o.vacuum(), info=g.vacuum_info())


def test_parity_after_a_resident_vacuum(vacuumed):
    v = vacuumed
    g, o, ids = v["g"], v["o"], v["ids"]
    assert v["removed"] == v["o_removed"] == len(v["dead"])
    assert v["info"]["path"] == "resident"
    assert g.node_count() == v["before"]["nodes"] - len(v["dead"]) == g.active_count()
    for r in v["dead"][:20]:
        assert not g.is_deleted(int(ids[r])) and g.level(int(ids[r])) == -1
        with pytest.raises(fv_error()):
            g.get_vector_by_id(int(ids[r]))
    for r in (0, 1, N // 2):
        if r not in v["dead"]:
            assert np.array_equal(g.get_vector_by_id(int(ids[r])), v["x"][r]) and g.level(int(ids[r])) == v["levels"][r]
    same_graph(g, o)
    same_searches(g, o, v["q"])
    info = g.vacuum_info()
    assert g.vacuum() == 0 and o.vacuum() == 0
    assert g.vacuum_info() == info, "a vacuum with nothing to remove runs no job"
    assert g.store_rows() == g.node_count()


def fv_error():
    return fvdb_import.load().FvdbError


def test_only_small_tables_crossed_the_host_link(vacuumed):
    v = vacuumed
    assert v["g"].insert_stats()["graph_upload_bytes"] == v["before"]["upload"]
    assert v["info"]["nodes_in"] == v["before"]["nodes"] == N
    assert v["info"]["host_bytes"] <= 8 * v["info"]["nodes_in"]


def test_rows_reclaimed(vacuumed):
    v = vacuumed
    g, info = v["g"], v["info"]
    assert v["before"]["store"] == N
    assert g.store_rows() == g.node_count() == N - len(v["dead"])
    assert info["rows_reclaimed"] == v["removed"]
    gi, edges = same_graph(g, v["o"])
    assert info["nodes_out"] == gi.size and info["edges_out"] == edges
    assert info["edges_in"] > info["edges_out"]
    assert info["bytes_reclaimed"] > 0 and info["move_bytes"] == 2 * gi.size * D * 4


# ---- 4. life goes on -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("visited", [0, 2])
def test_life_goes_on(fv, ctx, visited):
    g, o, x, ids, levels = pair(fv, ctx, seed=111, n=N - 100)
    g.set_insert_visited(visited)
    q = mixture(24, D, n_comp=8, seed=112)
    at = N - 100
    delete(g, o, ids, pick_dead(o, ids, levels, at, seed=2))
    assert g.vacuum() == o.vacuum()
    sl = slice(at, at + 200)  # misplaced edge distances would show here as different prunes
    assert g.batch_insert(ids[sl], x[sl], levels[sl]) == (200, 0)
    o.batch_insert(ids[sl], x[sl], levels[sl])
    at += 200
    assert g.insert_stats()["host_path_inserts"] == 0
    same_graph(g, o)
    g.set_device_insert(False)
    sl = slice(at, at + 20)
    assert g.batch_insert(ids[sl], x[sl], levels[sl]) == (20, 0)
    o.batch_insert(ids[sl], x[sl], levels[sl])
    at += 20
    assert g.insert_stats()["host_path_inserts"] == 20
    g.set_device_insert(True)
    same_graph(g, o)
    same_searches(g, o, q)
    rng = np.random.default_rng(3)
    for cycle in range(3):
        entry = o.entry_point()
        live = [int(i) for i in g.export_graph()[0] if int(i) != entry]
        for i in rng.choice(live, 60, replace=False).tolist():
            g.mark_deleted(i)
            o.mark_deleted(i)
        assert g.vacuum() == o.vacuum() == 60
        assert g.vacuum_info()["path"] == "resident" and g.store_rows() == g.node_count()
        sl = slice(at, at + 40)
        assert g.batch_insert(ids[sl], x[sl], levels[sl]) == (40, 0)
        o.batch_insert(ids[sl], x[sl], levels[sl])
        at += 40
        same_graph(g, o)
        same(g.search(q, 10, 50), o.batch_search(q, 10, 50))
    assert g.insert_stats()["host_path_inserts"] == 20


# ---- 5. the keep-rows form and the host form agree with the job -----------------------------------------------------------------
def test_keep_rows_form_and_host_form_agree_with_the_job(fv, ctx):
    q = mixture(24, D, n_comp=8, seed=122)
    made = []
    for form in ("resident", "resident_keep_rows", "host"):
        g, o, x, ids, levels = pair(fv, ctx, seed=121, n=1500)
        if form == "resident_keep_rows":
            g._set_vacuum_keep_rows(True)
        if form == "host":
            g.set_resident_vacuum(False)
            assert not g.resident_vacuum()
        at, gone = 1500, []
        for rnd in range(2):
            now_dead = pick_dead(o, ids, levels, 1500, seed=4 + rnd, frac=0.05, gone=gone)
            gone += now_dead
            delete(g, o, ids, now_dead)
            removed = g.vacuum()
            assert removed == o.vacuum() and removed > 0
            assert g.vacuum_info()["path"] == form
            sl = slice(at, at + 80)
            g.batch_insert(ids[sl], x[sl], levels[sl])
            o.batch_insert(ids[sl], x[sl], levels[sl])
            at += 80
        same_graph(g, o)
        made.append((g, g.export_graph(), [g.search(q, k, ef) for k, ef in ((10, 50), (20, 120))]))
    for g, graph, answers in made[1:]:
        for a, b in zip(graph, made[0][1]):
            assert np.array_equal(a, b)
        for a, b in zip(answers, made[0][2]):
            same_answers(a, b)
    assert made[0][0].store_rows() == made[0][0].node_count() < at
    assert made[1][0].store_rows() == at and made[2][0].store_rows() == at, "only the default form shrinks its store"
    # the C entry itself on a graph of its own: KEEP_ROWS, then the reclaiming job drops what it left behind
    g, o, x, ids, levels = pair(fv, ctx, seed=123, n=800)
    dead = pick_dead(o, ids, levels, 800, seed=6, frac=0.1)
    delete(g, o, ids, dead)
    lib, gh = ctx.lib, g._graph()
    removed = C.c_uint64(0)
    ctx.check(lib.fvdb_graph_vacuum(gh, fv._capi.VACUUM_KEEP_ROWS, C.byref(removed)))
    info = fv._capi.GraphMaintenanceInfo()
    ctx.check(lib.fvdb_graph_maintenance_info(gh, C.byref(info)))
    assert removed.value == len(dead) and info.nodes_out == 800 and info.rows_reclaimed == 0 and info.move_bytes == 0
    assert info.edges_in > info.edges_out
    edges_kept = info.edges_out
    ctx.check(lib.fvdb_graph_vacuum(gh, fv._capi.VACUUM_KEEP_ROWS, C.byref(removed)))
    assert removed.value == 0, "the lists are empty already"
    assert lib.fvdb_graph_vacuum(gh, 2, None) == E_INVALID
    ctx.check(lib.fvdb_graph_vacuum(gh, 0, C.byref(removed)))
    ctx.check(lib.fvdb_graph_maintenance_info(gh, C.byref(info)))
    assert removed.value == len(dead) and info.nodes_out == 800 - len(dead) and info.edges_in == info.edges_out == edges_kept
    n_nodes = C.c_uint32(0)
    ctx.check(lib.fvdb_graph_entry(gh, None, C.byref(n_nodes)))
    assert n_nodes.value == 800 - len(dead)
    # (that index's mirror was bypassed: it is not used again)


# ---- 6. masks ---------------------------------------------------------------------------------------------------------------
def brute_force(x, rows, ids, q, k):
    B = q.shape[0]
    oi = np.full((B, k), np.uint64(2 ** 64 - 1), np.uint64)
    od = np.full((B, k), np.inf, np.float32)
    oc = np.zeros(B, np.uint32)
    for b in range(B):
        dist = orc.l2_batch(q[b], x[rows])
        order = np.lexsort((rows, bits(dist)))[:k]  # distance bits, then node index (old or new: the order is the same)
        oc[b] = order.size
        oi[b, :order.size] = ids[rows[order]]
        od[b, :order.size] = dist[order]
    return oi, od, oc


def test_masks_before_and_after(fv, ctx):
    n = 1200
    g, o, x, ids, levels = pair(fv, ctx, seed=131, n=n)
    q = mixture(16, D, n_comp=8, seed=132)
    dead = pick_dead(o, ids, levels, n, seed=7, frac=0.1)
    rng = np.random.default_rng(8)
    entry = o.entry_point()
    wide = ids[:n][rng.random(n) < 0.5]
    wide = np.ascontiguousarray(np.concatenate([wide[wide != entry], [np.uint64(entry)]]))
    narrow = np.ascontiguousarray(ids[:n][rng.random(n) < 0.04])
    g.scan_cutoff = 200  # `wide` is traversed under its mask, `narrow` is scanned exactly

    def oracle_after(allowed, deleted):
        oo = orc.HNSWIndex(M, M0, EFC, seed=131)
        oo.batch_insert(ids[:n], x[:n], levels[:n])
        keep = set(int(i) for i in allowed)
        for r in deleted:
            oo.mark_deleted(int(ids[r]))
        oo.vacuum()
        for i in ids[:n].tolist():
            if i not in keep and i not in set(int(ids[r]) for r in deleted):
                oo.mark_deleted(i)
        return oo

    def narrow_rows(deleted):
        return np.array(sorted(set(((narrow - 11) // 5).tolist()) - set(deleted)), np.int64)

    assert narrow_rows(()).size <= 200 < wide.size - len(dead)
    same(g.search_allowed(q, 10, 50, wide), oracle_after(wide, ()).batch_search(q, 10, 50))
    same(g.search_allowed(q, 10, 50, narrow), brute_force(x, narrow_rows(()), ids, q, 10))
    # a mask made by hand on the device graph before the vacuum
    lib, gh = ctx.lib, g._graph()
    nodes = np.ascontiguousarray(np.arange(0, n, 3, dtype=np.uint32))
    mask = C.c_void_p()
    ctx.check(lib.fvdb_mask_create_graph(gh, nodes.ctypes.data_as(C.POINTER(C.c_uint32)), nodes.size, C.byref(mask)))
    delete(g, o, ids, dead)
    assert g.vacuum() == o.vacuum() == len(dead)
    assert g.vacuum_info()["path"] == "resident"
    same(g.search_allowed(q, 10, 50, wide), oracle_after(wide, dead).batch_search(q, 10, 50))
    same(g.search_allowed(q, 10, 50, narrow), brute_force(x, narrow_rows(dead), ids, q, 10))
    B, k = q.shape[0], 5
    q_dev = ctx.upload(q)
    out = (ctx.alloc(B * k * 4), ctx.alloc(B * k * 4), ctx.alloc(B * 4), ctx.alloc(B * 4))
    rc = lib.fvdb_graph_search_dev_slot_masked(g._graph(), None, 0, mask, q_dev, B, k, 50, *out)
    assert rc == E_INVALID and b"stale mask" in lib.fvdb_last_error(ctx.h)
    rc = lib.fvdb_graph_scan_allowed_dev_slot(g._graph(), None, 0, mask, q_dev, B, k, *out[:3])
    assert rc == E_INVALID and b"stale mask" in lib.fvdb_last_error(ctx.h)
    lib.fvdb_mask_destroy(mask)
    for p in out + (q_dev,):
        ctx.free(p)


# ---- 7. entry point ---------------------------------------------------------------------------------------------------
def test_vacuumed_entry_point_is_not_repaired(fv, ctx):
    g, o, x, ids, levels = pair(fv, ctx, seed=141, n=400)
    q = mixture(4, D, n_comp=8, seed=142)
    entry = g.entry_point()
    assert entry == o.entry_point()
    g.mark_deleted(entry)
    o.mark_deleted(entry)
    g.mark_deleted(int(ids[5]))
    o.mark_deleted(int(ids[5]))
    assert g.vacuum() == o.vacuum() == 2
    assert g.vacuum_info()["path"] == "resident_keep_rows", "the entry-lost state keeps the numbering (fvdb_host.hpp)"
    assert g.entry_point() == o.entry_point() == entry
    for dev in (True, False):
        g.set_device_traversal(dev)
        with pytest.raises(fv.FvdbError):
            g.search(q, 3, 10)
    with pytest.raises(orc.OracleError):
        o.batch_search(q, 3, 10)
    with pytest.raises(fv.FvdbError):
        g.search_allowed(q, 3, 10, ids[:50])
    with pytest.raises(fv.FvdbError):
        g.insert(10 ** 9, x[N], 0)
    g.set_device_insert(False)
    with pytest.raises(fv.FvdbError):
        g.insert(10 ** 9, x[N], 0)
    assert g.node_count() == 398


# ---- 8. hybrid and session ---------------------------------------------------------------------------------------------
DAY = 86400.0


def test_hybrid_and_session(fv, ctx):
    n, d, nlist = 900, 24, 6
    x = mixture(n + 80, d, n_comp=6, seed=151)
    cents = x[:nlist].copy()
    now = 1000 * DAY
    ages = np.where(np.random.default_rng(9).random(n + 80) < 0.4, 1 * DAY, 30 * DAY)
    levels = orc.rng_levels(152, n + 80)
    kw = dict(max_connections=8, max_connections_layer_0=16, ef_construction=40, n_clusters=nlist, n_probe=3)
    g, o = fv.HybridIndex(ctx, **kw), orc.HybridIndex(**kw)
    g.set_ivf_centroids(cents)
    o.set_ivf_centroids(cents)
    for i in range(n):
        g.insert_with_timestamp(i, x[i], now - ages[i], now, int(levels[i]))
        o.insert_with_timestamp(i, x[i], now - ages[i], now, int(levels[i]))
    q = mixture(24, d, n_comp=6, seed=153)

    def check():
        oi, od, oc = o.batch_search(q, 10, now=now, hnsw_ef=30, ivf_n_probe=4)
        same(g.search(q, 10, now=now, hnsw_ef=30, ivf_n_probe=4), (oi, od, oc))

    entry = o.hnsw().entry_point()
    recent = [i for i in range(n) if ages[i] < 7 * DAY and i != entry]
    hist = [i for i in range(n) if ages[i] >= 7 * DAY]
    dead = recent[3:90:2] + hist[10:100:3]
    for i in dead:
        g.delete(i, now)
        o.delete(i, now)
    check()
    rows_before = g.hnsw().store_rows()
    n_recent_dead = len(recent[3:90:2])
    assert g.vacuum() == {"hnsw_removed": n_recent_dead, "ivf_removed": 30, "total_removed": n_recent_dead + 30}
    assert (o.hnsw().vacuum(), o.ivf().vacuum()) == (n_recent_dead, 30)
    assert g.hnsw().vacuum_info()["path"] == "resident"
    assert g.hnsw().store_rows() == rows_before - n_recent_dead == g.hnsw().node_count()
    check()
    same_graph(g.hnsw(), o.hnsw())
    for c in range(nlist):
        assert g.ivf().export_list(c)[1].tolist() == o.ivf().list_ids(c).tolist()
    with pytest.raises(fv.DuplicateVector):  # a vacuumed id is still on record
        g.insert_with_timestamp(dead[0], x[dead[0]], now, now)
    for i in range(n, n + 80):
        g.insert_with_timestamp(i, x[i], now - ages[i], now, int(levels[i]))
        o.insert_with_timestamp(i, x[i], now - ages[i], now, int(levels[i]))
    check()
    later = now + 7 * DAY  # everything recent is due: the inserts that migrate after the vacuum match too
    assert g.migrate_with_threshold(7 * DAY, later) == o.migrate_with_threshold(7 * DAY, later)
    oi, od, oc = o.batch_search(q, 10, now=later, hnsw_ef=30, ivf_n_probe=4)
    same(g.search(q, 10, now=later, hnsw_ef=30, ivf_n_probe=4), (oi, od, oc))

    # the session: the same operations with the resident vacuum on and off answer the same
    answers = []
    for resident in (True, False):
        s = fv.VectorDbSession(ctx, now=now, **kw)
        s.index.hnsw().set_resident_vacuum(resident)
        s.add_vectors({"id": f"doc{i}", "vector": x[i].tolist(), "metadata": {"group": int(i % 5), "n": i}} for i in range(300))
        r = s.delete_by_metadata({"group": 3})
        assert r["deleted_count"] == 60
        stats = s.vacuum()
        assert stats["total_removed"] == 60
        assert s.index.hnsw().vacuum_info()["path"] == ("resident" if resident else "host")
        assert (s.index.hnsw().store_rows() == s.index.hnsw().node_count()) == resident
        s.add_vectors({"id": f"doc{i}", "vector": x[i].tolist(), "metadata": {"group": int(i % 5), "n": i}} for i in range(300, 340))
        answers.append([s.search(q[b].tolist(), 8) for b in range(8)])
        assert all(hit["metadata"]["group"] != 3 or hit["metadata"]["n"] >= 300 for a in answers[-1] for hit in a)
    assert answers[0] == answers[1]


# ---- 9. wide rows -------------------------------------------------------------------------------------------------------------
def wide_graph(n, d, m0, longest, seed):
    """a graph to restore: ring + random links, node 0 with `longest` neighbours on layer 0, all at level 0 but a few"""
    rng = np.random.default_rng(seed)
    x = mixture(n, d, n_comp=4, seed=seed)
    ids = np.arange(n, dtype=np.uint64) + 1000
    levels = np.zeros(n, np.uint32)
    levels[:3] = 1
    lists = []
    for i in range(n):
        deg = longest if i == 0 else int(rng.integers(4, min(m0, 40)))
        nb = [int(v) for v in rng.permutation(n) if v != i][:deg]
        lists.append(nb)
        if levels[i]:
            lists.append([int(v) for v in range(3) if v != i])
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists])
    nbrs = np.array([int(ids[v]) for l in lists for v in l], np.uint64)
    return x, ids, levels, off, nbrs


@pytest.mark.parametrize("longest, path", [(90, "host"), (60, "resident")])
def test_wide_rows(fv, ctx, longest, path):
    """max_connections_layer_0 = 96 makes the layer-0 stride 97 words.  The job walks a row in chunks of 64, so such a
    graph is pruned on the device — if it can be installed there at all: fvdb_graph_upload refuses a LIST longer than
    64 (one lane per neighbour in the traversal), and then the mirror takes the host form."""
    n, d = 300, 16
    x, ids, levels, off, nbrs = wide_graph(n, d, 96, longest, seed=161)
    g = fv.HNSWIndex(ctx, 16, 96, 40, seed=1)
    o = orc.HNSWIndex(16, 96, 40, seed=1)
    g.restore(ids, x, levels, off, nbrs, int(ids[0]))
    o.restore(ids, x, levels, off, nbrs, int(ids[0]))
    installed = bool(g._graph())  # asks for the device graph: installed, or refused
    assert installed == (path == "resident")
    dead = [5, 17, 100, 299] + list(range(30, 60, 2))
    assert int(ids[0]) == o.entry_point()
    for r in dead:
        g.mark_deleted(int(ids[r]))
        o.mark_deleted(int(ids[r]))
    assert g.vacuum() == o.vacuum() == len(dead)
    assert g.vacuum_info()["path"] == path
    same_graph(g, o)
    q = mixture(8, d, n_comp=4, seed=162)
    same(g.search(q, 10, 50), o.batch_search(q, 10, 50))
    assert (g.store_rows() == g.node_count()) == (path == "resident")


# ---- 10. randomised sequences ----------------------------------------------------------------------------------------------
def run_case(seed, oh_cls, gh_cls=None):
    """One sequence of insert / delete / vacuum / search steps, vacuum drawn three times as often as in
    tools/hnsw_ops_fuzz.py.  gh_cls = None runs the oracle alone (seeds are picked on a CPU-only machine that way).
    Returns (mismatches, entry_lost, vacuums that removed something)."""
    r = np.random.default_rng(seed)
    d = int(r.choice([8, 24, 100]))
    Mx = int(r.choice([4, 8, 16]))
    efc = int(r.choice([16, 48, 100]))
    total = 2500
    x = mixture(total, d, n_comp=int(r.choice([1, 8, 64])), sigma=0.4, seed=seed)
    if r.random() < 0.3:
        x[r.integers(0, total, 300)] = x[r.integers(0, total, 300)]  # duplicate vectors: ties
    ids = np.arange(total, dtype=np.uint64) * 7 + 3
    levels = orc.rng_levels(seed, total)
    oh = oh_cls(Mx, 2 * Mx, efc, seed=seed)
    gh = gh_cls(Mx, 2 * Mx, efc, seed=seed) if gh_cls else None
    at, bad, alive, vacuums, lost = 0, 0, [], 0, False

    def outcome(f):
        try:
            return ("ok", f())
        except Exception as e:  # noqa: BLE001
            return ("err", type(e).__name__)

    for step in range(int(r.integers(10, 22))):
        op = r.choice(["batch_dev", "batch_dev", "batch_host", "single", "delete", "delete", "search", "search",
                       "vacuum", "vacuum", "vacuum"])
        if op in ("batch_dev", "batch_host", "single"):
            cnt = min(1 if op == "single" else int(r.integers(2, 400)), total - at)
            if cnt <= 0:
                continue
            sl = slice(at, at + cnt)
            rb = outcome(lambda: oh.batch_insert(ids[sl], x[sl], levels[sl]))
            if gh is not None:
                gh.set_device_insert(op != "batch_host")
                ra = outcome(lambda: gh.batch_insert(ids[sl], x[sl], levels[sl]))
                g_ok = ra[0] == "ok" and ra[1][1] == 0
                g_none = ra[0] != "ok" or ra[1][0] == 0
                if g_ok != (rb[0] == "ok") or (not g_ok and not g_none):  # both succeed, or both fail whole
                    bad += 1
            if rb[0] == "ok":
                alive += list(range(at, at + cnt))
                at += cnt
        elif op == "delete" and alive:
            for i in r.choice(alive, size=min(len(alive), int(r.integers(1, 40))), replace=False).tolist():
                oh.mark_deleted(int(ids[i]))
                alive.remove(i)
                if gh is not None:
                    gh.mark_deleted(int(ids[i]))
        elif op == "vacuum" and at:
            entry = oh.entry_point()
            b = oh.vacuum()
            vacuums += 1 if b else 0
            if gh is not None:
                bad += 0 if gh.vacuum() == b else 1
                bad += 0 if gh.entry_point() == entry else 1
        elif op == "search" and at:
            q = np.ascontiguousarray(np.concatenate([x[r.integers(0, at, 8)], x[r.integers(0, total, 8)]]), np.float32)
            k, ef = (int(v) for v in r.choice([[5, 5], [10, 50], [10, 64], [20, 120]]))
            dev = bool(r.integers(0, 2))
            b = outcome(lambda: oh.batch_search(q, k, ef))
            lost = lost or b[0] == "err"
            if gh is not None:
                gh.set_device_traversal(dev)
                a = outcome(lambda: gh.search(q, k, ef))
                if a[0] != b[0]:  # a failure on one side only is a mismatch, whichever side
                    bad += 1
                elif a[0] == "ok":
                    valid = np.arange(k)[None, :] < np.asarray(b[1][2])[:, None]
                    ok = (np.array_equal(a[1].counts, b[1][2]) and np.array_equal(a[1].ids[valid], b[1][0][valid]) and
                          np.array_equal(bits(a[1].distances)[valid], bits(b[1][1])[valid]))
                    bad += 0 if ok else 1
    if not lost and at:  # (asked once more at the end, so that a case's state is known)
        lost = outcome(lambda: oh.batch_search(x[:2], 1, 5))[0] == "err"
    if gh is not None and at:
        gi, lv, off, nb = gh.export_graph()
        bad += 0 if gi.size == oh.node_count() else 1
        slot = 0
        for node, l in zip(gi.tolist(), lv.tolist()):
            for layer in range(l + 1):
                if nb[int(off[slot]):int(off[slot + 1])].tolist() != oh.neighbors(node, layer):
                    bad += 1
                slot += 1
        bad += 0 if gh.entry_point() == oh.entry_point() else 1
    return bad, lost, vacuums


# picked on the CPU with the oracle alone (run_case(seed, orc.HNSWIndex)): every case vacuums something at least once,
# and 3 of the 14 (at most a quarter) reach the entry-lost state
FUZZ_SEEDS = [1, 2, 3, 4, 5, 8, 10, 11, 12, 13, 17, 27, 32, 38]
FUZZ_ENTRY_LOST = {1, 3, 32}


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_randomised_sequences(fv, ctx, seed):
    bad, lost, vacuums = run_case(seed, orc.HNSWIndex, lambda *a, **kw: fv.HNSWIndex(ctx, *a, **kw))
    assert bad == 0
    assert vacuums >= 1 and lost == (seed in FUZZ_ENTRY_LOST)


def test_the_slice_keeps_exercising_live_graphs():
    assert len(FUZZ_SEEDS) >= 12 and 4 * len(FUZZ_ENTRY_LOST) <= len(FUZZ_SEEDS) and FUZZ_ENTRY_LOST <= set(FUZZ_SEEDS)
