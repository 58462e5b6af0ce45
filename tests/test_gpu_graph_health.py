"""GPU: the graph-health job (fvdb_graph_health, kernels_graph_health.h) on graphs installed with
restore, against the plain Python statement of its definitions (tests/_graph_health_ref.py, pinned by hand-computed
answers in tests/test_graph_health_ref.py) and against the host mirror's own restatement on a second index whose device
traversal is off.  d = 4: the job reads no vector row."""
import numpy as np
import pytest

import _graph_health_ref as ref
import fvdb_import
from _graph_health_check import agrees, raw_nodes, reference_of

pytestmark = pytest.mark.gpu

E_INVALID = 6  # FVDB_E_INVALID (include/fvdb.h)
CASES = ref.hand_built_cases()


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    c = fv.Context(0)
    yield c
    c.close()


def install(fv, ctx, levels, lists, deleted, entry, device, m=16, m0=32):
    """ids = node index + 100"""
    n = len(levels)
    off, nb = ref.csr(levels, lists)
    h = fv.HNSWIndex(ctx, m, m0, 50, seed=1)
    h.set_device_traversal(device)
    vec = (np.arange(n * 4, dtype=np.float32).reshape(n, 4) % 17.0)
    h.restore(np.arange(n, dtype=np.uint64) + 100, vec, np.asarray(levels, np.uint32), np.asarray(off, np.uint64),
              np.asarray(nb, np.uint64) + 100, 100 + entry)
    for d in deleted:
        h.mark_deleted(100 + int(d))
    return h


def both_paths(fv, ctx, levels, lists, deleted, entry, **kw):
    dev = install(fv, ctx, levels, lists, deleted, entry, True, **kw)
    known = reference_of(dev)
    got, f = agrees(fv, dev, "device", known)
    host = install(fv, ctx, levels, lists, deleted, entry, False, **kw)
    for a, b in zip(dev.export_graph(), host.export_graph()):  # the same graph: one reference serves both
        assert np.array_equal(a, b)
    assert dev.entry_point() == host.entry_point() and dev.active_count() == host.active_count()
    agrees(fv, host, "host", known)
    return got, f


def expect_table(got, expect):
    for k in ref.INT_FIELDS:
        assert got[k] == expect[k], (k, got[k], expect[k])
    hist = [0] * 65
    for b, c in expect["hist"].items():
        hist[b] = c
    assert got["degree0_hist"] == hist


@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "entry_lost"))
def test_hand_built_table(fv, ctx, name):
    levels, lists, deleted, entry, expect = CASES[name]
    got, _ = both_paths(fv, ctx, levels, lists, deleted, entry)
    expect_table(got, expect)


@pytest.mark.parametrize("device", [True, False])
def test_hand_built_entry_lost_to_a_vacuum(fv, ctx, device):
    # 0 <-> 1 <-> 2 with the entry 0 deleted and vacuumed away: what is left is the table's case (1 <-> 2, no entry)
    h = install(fv, ctx, [0, 0, 0], [[[1]], [[0, 2]], [[1]]], [0], 0, device)
    if device:
        h.search(np.zeros((1, 4), np.float32), 1, 8)  # the device graph exists: the vacuum is the resident job
    assert h.vacuum() == 1
    if device:
        assert h.vacuum_info()["path"] == "resident_keep_rows"
    got, _ = agrees(fv, h, "device" if device else "host")
    expect_table(got, CASES["entry_lost"][4])
    assert h.unreachable_ids().tolist() == [101, 102]


def ring(n, entry=0):
    return [0] * n, [[[(i + 1) % n]] for i in range(n)], [], entry


def path_graph(n, entry=0):
    """a directed path from the entry: entry = 0 runs upwards, entry = n - 1 downwards"""
    step = 1 if entry == 0 else -1
    return [0] * n, [[[i + step] if 0 <= i + step < n else []] for i in range(n)], [], entry


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_word_and_wave_edges(fv, ctx, n):
    for shape in (ring(n), path_graph(n), path_graph(n, n - 1), ring(n, n - 1)):
        got, f = both_paths(fv, ctx, *shape)
        assert got["reachable_live"] == n and got["components0"] == 1 and got["reach_rounds0"] == n
    # the same path with a node in its middle deleted: everything behind it is unreachable
    levels, lists, _, entry = path_graph(n)
    got, f = both_paths(fv, ctx, levels, lists, [n // 2], entry)
    assert got["reachable_live"] == n // 2 and got["unreachable_live"] == n - 1 - n // 2 and got["components0"] == 2


def test_full_rows_and_narrow_wide_narrow(fv, ctx):
    # a 63-ary tree of depth 2 (1 + 63 + 3969 nodes, rows of 63 entries at stride 64) with a 500-node path hung on the
    # last leaf: the frontier goes 1 -> 63 -> 3969 -> 1 -> 1 ...
    lists = [[list(range(1, 64))]]
    for i in range(63):
        lists.append([list(range(64 + 63 * i, 64 + 63 * (i + 1)))])
    n_tree = 1 + 63 + 3969
    for i in range(3969):
        lists.append([[]])
    lists[n_tree - 1] = [[n_tree]]
    for i in range(500):
        lists.append([[n_tree + i + 1] if i < 499 else []])
    n = n_tree + 500
    assert len(lists) == n
    got, f = both_paths(fv, ctx, [0] * n, lists, [], 0, m0=63)
    assert got["degree0_hist"][63] == 64 and got["reachable_live"] == n and got["components0"] == 1
    assert got["reach_rounds0"] == 3 + 500
    # narrow (1, 63, hands 3969 on), wide (3969), narrow (the path): three launches, not one per step
    assert got["reach_launches"] == 3


def test_a_path_costs_no_launch_per_node(fv, ctx):
    n = 3000
    got, f = both_paths(fv, ctx, *path_graph(n))
    assert got["reachable_live"] == n and got["reach_rounds0"] == n
    # a condition, not a measurement: the narrow loop carries a frontier of one node without a host round trip per node
    assert got["reach_launches"] <= 2 * (got["entry_level"] + 1)


def random_digraph(seed, n=20000, deleted_entry=False):
    """levels drawn with p = 0.4 and capped at 3; out-degree drawn uniformly in 0..32 on layer 0 and 0..16 above (a target
    drawn twice is kept once; a node may name itself); targets among the nodes of sufficient level; 30 % deleted; the
    entry a live node of the top level, or that node deleted"""
    rng = np.random.default_rng(seed)
    levels = np.minimum(rng.geometric(0.6, n) - 1, 3).astype(np.int64)  # P(level >= l) = 0.4 ** l, capped at 3
    levels[int(rng.integers(n))] = 3
    at_least = [np.flatnonzero(levels >= l) for l in range(4)]
    lists = []
    for u in range(n):
        layers = []
        for l in range(int(levels[u]) + 1):
            deg = int(rng.integers(0, 33 if l == 0 else 17))
            pool = at_least[l]
            layers.append(list(dict.fromkeys(pool[rng.integers(0, pool.size, deg)].tolist())))  # distinct, in draw order
        lists.append(layers)
    dead = set(rng.choice(n, int(0.3 * n), replace=False).tolist())
    top = np.flatnonzero(levels == 3)
    alive_top = [int(u) for u in top if int(u) not in dead]
    entry = alive_top[0] if alive_top else int(top[0])
    dead.discard(entry)
    if deleted_entry:
        dead.add(entry)
    return levels.tolist(), lists, sorted(dead), entry


@pytest.mark.parametrize("seed,deleted_entry", [(11, False), (12, True)])
def test_random_digraph(fv, ctx, seed, deleted_entry):
    levels, lists, dead, entry = random_digraph(seed, deleted_entry=deleted_entry)
    got, f = both_paths(fv, ctx, levels, lists, dead, entry)
    assert got["entry_live"] == (0 if deleted_entry else 1) and got["entry_level"] == 3
    assert got["n_live"] == len(levels) - len(dead) and got["dangling"] > 0 and got["reachable_live"] > 0


def test_skipped_parts(fv, ctx):
    levels, lists, deleted, entry, expect = CASES["deleted_bridge"]
    h = install(fv, ctx, levels, lists, deleted, entry, True)
    full = h.graph_health()
    census = [k for k in ref.INT_FIELDS if k not in ref.REACH_FIELDS + ref.COMPONENT_FIELDS]
    no_reach = h.graph_health(reach=False)
    assert all(no_reach[k] == 0 for k in ref.REACH_FIELDS) and no_reach["reach_launches"] == 0
    assert all(no_reach[k] == full[k] for k in census + list(ref.COMPONENT_FIELDS))
    assert no_reach["degree0_hist"] == full["degree0_hist"]
    assert raw_nodes(fv, h, 5, want_label=False)[0] == E_INVALID
    rc, _, label = raw_nodes(fv, h, 5, want_reached=False)
    assert rc == 0 and label.tolist() == expect["label"]
    no_comp = h.graph_health(components=False)
    assert all(no_comp[k] == 0 for k in ref.COMPONENT_FIELDS)
    assert all(no_comp[k] == full[k] for k in census + list(ref.REACH_FIELDS))
    assert raw_nodes(fv, h, 5, want_reached=False)[0] == E_INVALID
    rc, reached, _ = raw_nodes(fv, h, 5, want_label=False)
    assert rc == 0 and reached.tolist() == expect["reached"]
    neither = h.graph_health(reach=False, components=False)
    assert all(neither[k] == 0 for k in ref.REACH_FIELDS + ref.COMPONENT_FIELDS)
    assert all(neither[k] == full[k] for k in census) and neither["scratch_bytes"] < full["scratch_bytes"]
    # a change to the graph makes the per-node results of the job before it unavailable
    h.graph_health()
    assert raw_nodes(fv, h, 5)[0] == 0
    h.mark_deleted(104)
    assert raw_nodes(fv, h, 5)[0] == E_INVALID
    # the host restatement skips the same parts
    host = install(fv, ctx, levels, lists, deleted, entry, False)
    assert {k: v for k, v in host.graph_health(reach=False).items() if k in ref.INT_FIELDS} == \
           {k: no_reach[k] for k in ref.INT_FIELDS}
    assert {k: v for k, v in host.graph_health(components=False).items() if k in ref.INT_FIELDS} == \
           {k: no_comp[k] for k in ref.INT_FIELDS}


def test_reference_known_answers(fv, ctx):
    # tests/hnsw/operations.rs:284-304 of the reference: an empty index, then five inserted 1-d vectors [i]
    h = fv.HNSWIndex(ctx, 16, 32, 200, seed=3)
    s = h.get_graph_stats()
    assert s["total_nodes"] == 0 and s["total_edges"] == 0
    assert s == {"total_nodes": 0, "total_edges": 0, "avg_degree": 0.0, "max_layer": 0, "connected_components": 0}
    assert h.get_level_distribution() == [0] and h.get_max_level() == 0
    empty = h.graph_health()
    assert all(empty[k] == 0 for k in ref.INT_FIELDS) and empty["path"] == "host"
    assert h.unreachable_ids().size == 0 and h.component_labels()[1].size == 0
    for i in range(5):
        h.insert(i, np.array([float(i)], np.float32))
    s = h.get_graph_stats()
    assert s["total_nodes"] == 5 and s["total_edges"] > 0 and s["avg_degree"] > 0 and s["connected_components"] == 1
    dist = h.get_level_distribution()
    assert dist[0] == h.node_count() == 5 and len(dist) == h.get_max_level() + 1
    got, f = agrees(fv, h, "device")
    assert s["total_edges"] == got["edge_slots_live"] // 2 and s["max_layer"] == got["max_level_live"]
    assert s["avg_degree"] == float(np.float32(s["total_edges"] * 2) / np.float32(5))
    # deleted nodes stay in the level figures and leave the stats
    h.mark_deleted(4)
    assert h.get_level_distribution() == dist and h.get_graph_stats()["total_nodes"] == 4
