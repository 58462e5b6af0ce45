"""A plain Python statement of the graph-health definitions (include/fvdb.h, fvdb_graph_health).

Input: what HNSWIndex.export_graph() returns (ids, levels, nbr_offsets, nbrs: CSR over (node, layer) slots in node
order, layer 0 first, neighbours as ids), the set of deleted ids and the entry id (None: no entry, or lost to a vacuum).
Everything is integers; nodes are numbered in export order.  A deque BFS per layer and a union-find, nothing else.
"""
from collections import deque

NONE32 = 0xFFFFFFFF
INT_FIELDS = ("n_nodes", "n_live", "has_entry", "entry_live", "entry_level", "max_level_live", "edge_slots_live", "dangling",
              "dangling0", "reachable_live", "unreachable_live", "reach_rounds0", "components0", "largest_component0",
              "isolated0")
REACH_FIELDS = ("reachable_live", "unreachable_live", "reach_rounds0")
COMPONENT_FIELDS = ("components0", "largest_component0", "isolated0")


def lists_of(ids, levels, nbr_offsets, nbrs):
    """[node][layer] -> list of node indices."""
    index_of = {int(x): i for i, x in enumerate(ids)}
    out, slot = [], 0
    for i in range(len(ids)):
        layers = []
        for _ in range(int(levels[i]) + 1):
            layers.append([index_of[int(x)] for x in nbrs[int(nbr_offsets[slot]):int(nbr_offsets[slot + 1])]])
            slot += 1
        out.append(layers)
    return out


def graph_health(ids, levels, nbr_offsets, nbrs, deleted_ids=(), entry_id=None):
    """-> (figures dict incl. degree0_hist, reached[n] 0/1, label0[n] node index or NONE32)."""
    n = len(ids)
    index_of = {int(x): i for i, x in enumerate(ids)}
    N = lists_of(ids, levels, nbr_offsets, nbrs)
    dead = set(int(x) for x in deleted_ids)
    live = [int(ids[i]) not in dead for i in range(n)]
    entry = index_of.get(int(entry_id)) if entry_id is not None else None
    f = {k: 0 for k in INT_FIELDS}
    hist = [0] * 65
    f["n_nodes"] = n
    for u in range(n):
        if not live[u]:
            continue
        f["n_live"] += 1
        f["max_level_live"] = max(f["max_level_live"], int(levels[u]))
        for l, lst in enumerate(N[u]):
            gone = sum(1 for v in lst if not live[v])
            f["edge_slots_live"] += len(lst)
            f["dangling"] += gone
            if l == 0:
                f["dangling0"] += gone
                hist[min(len(lst), 64)] += 1
    # reach: layer by layer from the entry's level; a step expands what the step before added, the first one all of R
    reached = [0] * n
    if entry is not None:
        f["has_entry"], f["entry_live"], f["entry_level"] = 1, int(live[entry]), int(levels[entry])
        reached[entry] = 1
        R = [entry]
        for l in range(int(levels[entry]), -1, -1):
            frontier = deque(R)
            while frontier:
                if l == 0:
                    f["reach_rounds0"] += 1
                nxt = deque()
                while frontier:
                    u = frontier.popleft()
                    if int(levels[u]) < l or not (live[u] or u == entry):
                        continue
                    for v in N[u][l]:
                        if live[v] and not reached[v]:
                            reached[v] = 1
                            nxt.append(v)
                R.extend(nxt)
                frontier = nxt
    f["reachable_live"] = sum(1 for u in range(n) if reached[u] and live[u])
    f["unreachable_live"] = f["n_live"] - f["reachable_live"]
    # weak components of layer 0 among live nodes
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u in range(n):
        if live[u]:
            for v in N[u][0]:
                if live[v]:
                    a, b = find(u), find(v)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    label = [find(u) if live[u] else NONE32 for u in range(n)]
    sizes = {}
    for u in range(n):
        if live[u]:
            sizes[label[u]] = sizes.get(label[u], 0) + 1
    f["components0"] = len(sizes)
    f["largest_component0"] = max(sizes.values()) if sizes else 0
    f["isolated0"] = sum(1 for s in sizes.values() if s == 1)
    f["degree0_hist"] = hist
    return f, reached, label


def csr(levels, lists):
    """lists[node][layer] of node INDICES -> (nbr_offsets, nbrs) with ids = indices (the tests use ids 0..n-1 or map)."""
    off, nb = [0], []
    for i, lv in enumerate(levels):
        assert len(lists[i]) == lv + 1
        for l in range(lv + 1):
            nb.extend(lists[i][l])
            off.append(len(nb))
    return off, nb


def hand_built_cases():
    """name -> (levels, lists[node][layer] of node indices, deleted nodes, entry or None, expected figures).  ids = node
    index + 100.  The expected figures are worked out by hand, each with its reasoning."""
    cases = {}

    def add(name, levels, lists, deleted, entry, **expect):
        cases[name] = (levels, lists, sorted(deleted), entry, expect)

    # one node, no links: it is the entry, R = {0}, one step at layer 0 that finds nothing
    add("one_node", [0], [[[]]], [], 0,
        n_nodes=1, n_live=1, has_entry=1, entry_live=1, entry_level=0, max_level_live=0, edge_slots_live=0, dangling=0,
        dangling0=0, reachable_live=1, unreachable_live=0, reach_rounds0=1, components0=1, largest_component0=1, isolated0=1,
        hist={0: 1}, reached=[1], label=[0])
    # two nodes linked mutually: step 1 expands {0} and finds 1, step 2 expands {1} and finds nothing
    add("two_mutual", [0, 0], [[[1]], [[0]]], [], 0,
        n_nodes=2, n_live=2, has_entry=1, entry_live=1, entry_level=0, max_level_live=0, edge_slots_live=2, dangling=0,
        dangling0=0, reachable_live=2, unreachable_live=0, reach_rounds0=2, components0=1, largest_component0=2, isolated0=0,
        hist={1: 2}, reached=[1, 1], label=[0, 0])
    # main part 0 <-> 1; island 2 <-> 3 where 3 also points INTO the main part (3 -> 0): weakly one component,
    # but nothing in the main part points at the island: 2 and 3 are unreachable
    add("island_points_in", [0, 0, 0, 0], [[[1]], [[0]], [[3]], [[2, 0]]], [], 0,
        n_nodes=4, n_live=4, has_entry=1, entry_live=1, entry_level=0, max_level_live=0, edge_slots_live=5, dangling=0,
        dangling0=0, reachable_live=2, unreachable_live=2, reach_rounds0=2, components0=1, largest_component0=4, isolated0=0,
        hist={1: 3, 2: 1}, reached=[1, 1, 0, 0], label=[0, 0, 0, 0])
    # main part 0 <-> 1; island 2 <-> 3 reached only through the one-way edge 1 -> 2: all reachable.
    # steps at layer 0: {0} finds 1; {1} finds 2; {2} finds 3; {3} finds nothing = 4
    add("island_one_way_in", [0, 0, 0, 0], [[[1]], [[0, 2]], [[3]], [[2]]], [], 0,
        n_nodes=4, n_live=4, has_entry=1, entry_live=1, entry_level=0, max_level_live=0, edge_slots_live=5, dangling=0,
        dangling0=0, reachable_live=4, unreachable_live=0, reach_rounds0=4, components0=1, largest_component0=4, isolated0=0,
        hist={1: 3, 2: 1}, reached=[1, 1, 1, 1], label=[0, 0, 0, 0])
    # path 0 <-> 1 <-> 2 <-> 3 <-> 4 with the bridge 2 deleted: 3 and 4 are live and unfindable; two components {0,1}, {3,4}
    # slots of live nodes: 0:1, 1:2, 3:2, 4:1 = 6; entries naming the deleted 2: in 1's and 3's lists = 2
    # steps: {0} finds 1; {1} finds nothing (2 is deleted) = 2
    add("deleted_bridge", [0] * 5, [[[1]], [[0, 2]], [[1, 3]], [[2, 4]], [[3]]], [2], 0,
        n_nodes=5, n_live=4, has_entry=1, entry_live=1, entry_level=0, max_level_live=0, edge_slots_live=6, dangling=2,
        dangling0=2, reachable_live=2, unreachable_live=2, reach_rounds0=2, components0=2, largest_component0=2, isolated0=0,
        hist={1: 2, 2: 2}, reached=[1, 1, 0, 0, 0], label=[0, 0, NONE32, 3, 3])
    # deleted entry 0 <-> 1 <-> 2: still seeded and expanded (so 1, 2 are reached), in R but not counted as live.
    # live slots: 1:2, 2:1 = 3; 1's list names the deleted 0 = 1 dangling.  steps: {0} finds 1; {1} finds 2; {2} nothing = 3
    add("deleted_entry", [0, 0, 0], [[[1]], [[0, 2]], [[1]]], [0], 0,
        n_nodes=3, n_live=2, has_entry=1, entry_live=0, entry_level=0, max_level_live=0, edge_slots_live=3, dangling=1,
        dangling0=1, reachable_live=2, unreachable_live=0, reach_rounds0=3, components0=1, largest_component0=2, isolated0=0,
        hist={1: 1, 2: 1}, reached=[1, 1, 1], label=[NONE32, 1, 1])
    # entry 0 (level 1) links to 1 on layer 1 only; on layer 0 nobody names 1 (0's layer-0 list holds 2).  The layered
    # seeding finds 1 on layer 1; a BFS of layer 0 alone from the entry would miss it.  1 -> 3 on layer 0 then finds 3.
    # layer 1: R = {0, 1}.  layer 0: step 1 expands {0, 1}: finds 2 and 3; step 2 expands {2, 3}: nothing = 2
    # live slots: 0: 1 + 1, 1: 1 + 0, 2: 0, 3: 0 = 3.  layer 0 ignoring direction: 0-2, 1-3: components {0,2}, {1,3}
    add("inbound_on_layer_1_only", [1, 1, 0, 0], [[[2], [1]], [[3], []], [[]], [[]]], [], 0,
        n_nodes=4, n_live=4, has_entry=1, entry_live=1, entry_level=1, max_level_live=1, edge_slots_live=3, dangling=0,
        dangling0=0, reachable_live=4, unreachable_live=0, reach_rounds0=2, components0=2, largest_component0=2, isolated0=0,
        hist={0: 2, 1: 2}, reached=[1, 1, 1, 1], label=[0, 1, 0, 1])
    # 0 <-> 1, and 1's layer-1 list names the deleted 2 as well: dangling counts all layers, dangling0 layer 0 only.
    # levels 1, 1, 1; layer 1: 0 -> 1, 1 -> 0, 2;  layer 0: 0 -> 1, 2; 1 -> 0; 2 -> 0
    # live slots: 0: 2 + 1, 1: 1 + 2 = 6; dangling: 0's layer-0 list (2), 1's layer-1 list (2) = 2; dangling0 = 1
    # layer 1: {0} finds 1; {1} nothing.  layer 0: {0, 1} nothing = 1 step
    add("dangling_entries", [1, 1, 1], [[[1, 2], [1]], [[0], [0, 2]], [[0], []]], [2], 0,
        n_nodes=3, n_live=2, has_entry=1, entry_live=1, entry_level=1, max_level_live=1, edge_slots_live=6, dangling=2,
        dangling0=1, reachable_live=2, unreachable_live=0, reach_rounds0=1, components0=1, largest_component0=2, isolated0=0,
        hist={1: 1, 2: 1}, reached=[1, 1, 0], label=[0, 0, NONE32])
    # no live node: the deleted entry is in R, nothing is counted.  step 1 expands {0}: 1 is deleted, nothing = 1
    add("no_live_node", [0, 0], [[[1]], [[0]]], [0, 1], 0,
        n_nodes=2, n_live=0, has_entry=1, entry_live=0, entry_level=0, max_level_live=0, edge_slots_live=0, dangling=0,
        dangling0=0, reachable_live=0, unreachable_live=0, reach_rounds0=1, components0=0, largest_component0=0, isolated0=0,
        hist={}, reached=[1, 0], label=[NONE32, NONE32])
    # the entry was lost to a vacuum: what export_graph() returns no longer holds it.  R is empty, every live node is
    # unreachable.  1 <-> 2 survive.
    add("entry_lost", [0, 0], [[[1]], [[0]]], [], None,
        n_nodes=2, n_live=2, has_entry=0, entry_live=0, entry_level=0, max_level_live=0, edge_slots_live=2, dangling=0,
        dangling0=0, reachable_live=0, unreachable_live=2, reach_rounds0=0, components0=1, largest_component0=2, isolated0=0,
        hist={1: 2}, reached=[0, 0], label=[0, 0])
    return cases
