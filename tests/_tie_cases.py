"""Hand-built HNSW graphs around the tie rules of the sorted-register searches (hnsw_search_fast_kernel,
kernels_graph_fast.h; ef_search_layer<EXACT = false>, kernels_graph_build.h), the rules restated in Python, and the
integer-lattice graphs of the fuzz.  Data only: no GPU, no index.

The rules.  Equal distances end a sorted-register attempt (the query is searched again with the reference's heaps
restated) only where BinaryHeap's layout can decide the outcome:
  twin    two unexpanded candidates share the minimum at a pop: fine while neither expansion admits anything nearer;
          three sharing it, or a second pair inside the first, end the attempt
  amb     two or more members share the maximum when one has to leave: an expanded one is sent away; the attempt ends
          when the survivor is popped, or is read in the result
  result  equal neighbours, or a value equal to `amb`, among the entries that are read: the first min(nN, k + 1) of a
          search (all of them with any soft-deleted node in the graph), the first entry of an upper layer, every entry
          of an insert's search here (select_neighbors takes m = M0 = 8 >= ef of them)

The graphs.  Node i is the row (x_i, y_i, 0, ...), the query is the origin, every coordinate a multiple of 1/8 and every
distance a multiple of 1/8 below 32: exact in f32 and in fp16, so d(q, i) = |(x_i, y_i)| in every arithmetic.
Ids are node + ID_BASE.  `adj` is the layer-0 list ORDER, which is the push order of a walk.  The entry is node 0 unless
the case has an upper layer (`top`): then one more node, far away, sits on level 1 with node 0, and the descent from it
ends at node 0, over the same layer-0 picture.

Each case lists its searches as (k, deleted nodes, restart expected, family); the table is the written rule — whoever
changes the rule edits the table on purpose.  `insert_restart` is the expectation for the device insert of the origin
row at level 0 with (M, M0, ef_construction) = (4, 8, ef): the same walk, but the result is read whole (every list here
is shorter than M0 + 1), so any equal pair that ends in it, and an `amb` equal to the final maximum, end the attempt."""
import collections

import numpy as np

ID_BASE = 1000
INSERT_ID = 5000  # id of the origin row the insert tests add

Case = collections.namedtuple("Case", "name coords adj ef tied ties searches insert_restart top why")
Search = collections.namedtuple("Search", "k deleted restart family")


def _case(name, coords, adj, ef, tied, searches, insert_restart, why, top=False, ties=None):
    """tied: the nodes the mirror exchanges; ties: every group of equal distances among the case's nodes (default: tied
    alone).  A `restart` or `insert_restart` given as a pair is (the case's, its mirror's)."""
    coords = [c if isinstance(c, tuple) else (c, 0) for c in coords]
    return Case(name, coords, [list(a) for a in adj], ef, tuple(tied), [tuple(t) for t in (ties or [tied])],
                [Search(k, tuple(dl), r, f) for k, dl, r, f in searches], insert_restart, top, why)


T1_ADJ = [[1, 2, 3], [0, 4], [0, 5], [0, 6], [1], [2], [3]]
M3_ADJ = [[1, 2, 3], [0, 4], [0, 5], [0], [1], [2]]
M4_ADJ = [[1, 2, 3, 4, 5], [0, 6], [0, 7], [0], [0], [0], [1], [2]]
M5_ADJ = [[1, 2, 3, 4, 5, 6], [0, 7], [0, 8], [0, 9], [0], [0], [0], [1], [2], [3]]
P, Q = (3, 4), (5, 0)  # two vectors at distance 5: tied members that are no mirror images of each other

CASES = [
    # ---- twin pops --------------------------------------------------------------------------------------------------
    _case("T1", [1, 2, 3, -3, 4, 5, 6], T1_ADJ, 8, (2, 3),
          [(1, (), False, "twin"), (2, (), False, "twin"), (3, (), True, "cut"), (4, (), True, "twin")], True,
          "nodes 2 and 3 share the minimum at the third pop; their expansions admit 5 and 6, farther than the pair.  The "
          "pair ends at entries 3 and 4 of the result: past what k = 1, 2 read, across the cut at k = 3, inside at k = 4.  "
          "Insert: the pair is in the result that is read whole"),
    _case("T2", [1, 2, 3, -3, 4, 2.5, 6], T1_ADJ, 8, (2, 3),
          [(1, (), True, "twin"), (2, (), True, "twin")], True,
          "as T1, but node 2's expansion admits node 5 at 2.5 < 3: d < twin_d"),
    _case("T2b", [1, 2, 3, -3, 4, 5, 2.5], T1_ADJ, 8, (2, 3),
          [(1, (), True, "twin"), (2, (), True, "twin")], True,
          "as T2 with the nearer node behind node 3: whichever of the pair a walk expands first, one of T2 and T2b admits "
          "the nearer node in the first expansion and the other in the second"),
    _case("T3", [(1, 0), (3, 0), (-3, 0), (0, 3), 4, 5, 6], T1_ADJ, 8, (1, 2, 3),
          [(1, (), True, "twin")], True,
          "three candidates share the minimum at the second pop: holders > 2"),
    _case("T4", [1, 3, -3, 3.5, (0, 3.5), 6, 7, 8, 9], [[1, 2], [0, 3], [0, 4], [1, 5, 6], [2, 7, 8], [3], [3], [4], [4]], 9, (1, 2),
          [(1, (), False, "twin"), (2, (), True, "cut"), (3, (), True, "twin")], True,
          "two pairs one after the other (1, 2 at 3; then 3, 4 at 3.5, admitted by the first pair's expansions): the second "
          "pair is popped when twin_left is back at 0 and is benign as well", ties=[(1, 2), (3, 4)]),
    _case("T5", [1, 3, -3, (0, 3), 6, 7], [[1, 2], [0, 3], [0, 4], [1, 5], [2], [3]], 8, (1, 2),
          [(1, (), (False, True), "twin"), (2, (), True, "cut")], True,
          "the expansion of node 1 admits node 3 at the pair's own distance (not nearer: no d < twin_d).  The sorted list "
          "holds the later of two equals first, so the case expands 2, then 1, and pops 3 alone afterwards; its mirror "
          "expands 1 first and finds two holders at the pair's second pop: holders != twin_left", ties=[(1, 2, 3)]),
    # ---- a tied maximum ---------------------------------------------------------------------------------------------
    _case("M1", [1, 3, -3, 2], [[1], [0, 2], [1, 3], [2]], 3, (1, 2),
          [(1, (), False, "max"), (2, (), True, "max"), (3, (), True, "max")], True,
          "1 and 2 are both expanded when 3 arrives at the full list: one leaves, the other is never popped again but is "
          "entry 3 of the result — read at k = 2 (the pair at the cut) and k = 3, not at k = 1"),
    _case("M2", [1, 3, -3, 2, 10], [[1], [0, 2, 3], [1, 4], [1], [2]], 3, (1, 2),
          [(1, (), True, "max"), (2, (), True, "max"), (3, (), True, "max")], True,
          "1 is expanded and 2 is not when 3 arrives: the expanded one is sent away, the survivor 2 is popped: dc == amb"),
    _case("M3", [1, 3, -3, 2, 10, 11], M3_ADJ, 3, (1, 2),
          [(1, (), True, "max"), (2, (), True, "max"), (3, (), True, "max")], True,
          "1 and 2 are both unexpanded when 3 arrives: one leaves, the survivor is popped"),
    _case("M4", [1, 3, -3, 2, 1.5, 1.25, 10, 11], M4_ADJ, 3, (1, 2),
          [(1, (), False, "max"), (2, (), False, "max"), (3, (), False, "max")], False,
          "as M3, but 4 and 5 follow in the same list: the survivor leaves too, before any pop.  Insert: the final maximum "
          "is 1.5, not amb = 3"),
    _case("M5", [(1, 0), (3, 0), (-3, 0), (0, 3), 1.5, 1.25, 1.125, 10, 11, 12], M5_ADJ, 4, (1, 2, 3),
          [(1, (), False, "max"), (2, (), False, "max"), (3, (), False, "max")], False,
          "three share the maximum of the full list; 4, 5, 6 send all three away one by one (amb is set twice, to the same "
          "value)"),
    _case("M1p", [1, P, Q, 2], [[1], [0, 2], [1, 3], [2]], 3, (1, 2),
          [(1, (), False, "max"), (2, (), True, "max"), (3, (), True, "max")], True,
          "M1 with the tied members at (3, 4) and (5, 0).  It is also what an M2 where the survivor is read without being "
          "popped comes to: an unexpanded survivor is always popped (dc == amb) or sent away, so a survivor that is only "
          "read is an expanded one"),
    _case("M2p", [1, P, Q, 2, 10], [[1], [0, 2, 3], [1, 4], [1], [2]], 3, (1, 2),
          [(1, (), True, "max"), (2, (), True, "max")], True, "M2 with the tied members at (3, 4) and (5, 0)"),
    _case("M3p", [1, P, Q, 2, 10, 11], M3_ADJ, 3, (1, 2),
          [(2, (), True, "max"), (3, (), True, "max")], True, "M3 with the tied members at (3, 4) and (5, 0)"),
    _case("M4p", [1, P, Q, 2, 1.5, 1.25, 10, 11], M4_ADJ, 3, (1, 2),
          [(1, (), False, "max"), (3, (), False, "max")], False, "M4 with the tied members at (3, 4) and (5, 0)"),
    _case("M6", [1, 3, -3, 2, 2.5, 10], [[1], [0, 2, 3], [1, 5], [1, 4], [3], [2]], 3, (1, 2),
          [(1, (), False, "max"), (2, (), False, "max"), (3, (), False, "max")], False,
          "as M2 (the expanded member 1 is sent away), but the expansion of 3 admits 4 at 2.5 and the survivor 2 leaves "
          "unpopped"),
    # ---- at the cut -------------------------------------------------------------------------------------------------
    _case("E1", [1, 3, -3, 2, 2.5, -2.25], [[1, 2], [0, 3], [0, 4], [1, 5], [2], [3]], 2, (1, 2),
          [(2, (), False, "cut")], False,
          "the list is full when the second of 1, 2 arrives at the maximum's distance: refused (d < worst fails), no two "
          "members ever share the maximum.  List order decides, legitimately: it is the input"),
    _case("D1", [1, 2, 3, -3, 4, 5, 6, 7], [[1, 2, 3], [0, 4], [0, 5], [0, 6], [1, 7], [2], [3], [4]], 8, (2, 3),
          [(1, (), False, "cut"), (1, (7,), True, "cut"), (2, (1,), True, "cut")], True,
          "T1 with one more node: with any node soft-deleted the whole list is read, and the pair 2, 3 is in it"),
    # ---- under an upper layer ---------------------------------------------------------------------------------------
    _case("T1u", [1, 2, 3, -3, 4, 5, 6], T1_ADJ, 8, (2, 3),
          [(1, (), False, "twin"), (2, (), False, "twin"), (3, (), True, "cut"), (4, (), True, "twin")], True,
          "T1 below a level-1 entry point", top=True),
    _case("M4u", [1, 3, -3, 2, 1.5, 1.25, 10, 11], M4_ADJ, 3, (1, 2),
          [(1, (), False, "max"), (3, (), False, "max")], False, "M4 below a level-1 entry point", top=True),
]
BY_NAME = {c.name: c for c in CASES}
TOP_COORD = (20, 0)


def _lists_exchanged(case, lists=None):
    adj = []
    for row in case.adj if lists is None else lists:
        at = [i for i, v in enumerate(row) if v in case.tied]
        row = list(row)
        for i, v in zip(at, [row[i] for i in reversed(at)]):
            row[i] = v
        adj.append(row)
    return adj


def exchanged(case):
    """the mirror: the tied nodes in reversed order among themselves in every list that holds more than one of them; where
    no list does (the chains M1, M2, M6: each tied node is admitted by another list) the tied nodes trade vectors"""
    adj, coords = _lists_exchanged(case), list(case.coords)
    if adj == case.adj:
        for a, b in zip(case.tied, reversed(case.tied)):
            coords[a] = case.coords[b]
    second = lambda r: r[1] if isinstance(r, tuple) else r
    return case._replace(name=case.name + "~", adj=adj, coords=coords, insert_restart=second(case.insert_restart),
                         searches=[s._replace(restart=second(s.restart)) for s in case.searches])


def plain(case):
    """the case itself, pairs of expectations resolved to its own"""
    first = lambda r: r[0] if isinstance(r, tuple) else r
    return case._replace(searches=[s._replace(restart=first(s.restart)) for s in case.searches],
                         insert_restart=first(case.insert_restart))


def both(case):
    return [plain(case), exchanged(case)]


def exchange_lists(case, lists):
    """what exchanged() does to the case's lists, done to `lists` (nothing where the mirror trades vectors instead)"""
    return [list(r) for r in lists] if _lists_exchanged(case) == case.adj else _lists_exchanged(case, lists)


def graph(case, d):
    """x, ids, levels, off, nbrs, entry for restore(), and the origin query"""
    coords = case.coords + ([TOP_COORD] if case.top else [])
    n = len(coords)
    x = np.zeros((n, d), np.float32)
    x[:, :2] = np.asarray(coords, np.float32)
    ids = np.arange(n, dtype=np.uint64) + np.uint64(ID_BASE)
    levels = np.zeros(n, np.int64)
    lists = [list(a) for a in case.adj]
    if case.top:  # slots in node order, layer 0 first: node 0 gets a level-1 list, the top node a layer-0 and a level-1 list
        levels[0] = levels[n - 1] = 1
        lists = [lists[0], [n - 1]] + lists[1:] + [[0], [0]]
    off = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.uint64)
    nbrs = np.asarray([v for a in lists for v in a], np.uint64) + np.uint64(ID_BASE)
    return x, ids, levels, off, nbrs, int(ids[n - 1 if case.top else 0]), np.zeros(d, np.float32)


def distances(case):
    c = np.asarray(case.coords + ([TOP_COORD] if case.top else []), np.float64)
    return np.sqrt((c * c).sum(axis=1))  # exact: see the module's docstring


# ---- the rules restated ------------------------------------------------------------------------------------------------
EVENTS = collections.Counter()  # what the restated walks met: "twin", "amb", "swap" (the sorted list's lane swap), "ended" in a walk


def _layer(dist, lists, deleted, ep, ef, insert_form):
    """one search_layer by the sorted-register rules; (members in ascending order as [d, node, expanded], amb) or None
    where the attempt ends.  insert_form: the register SET of the insert — the member sent away from a tied maximum is the
    first expanded one, else the first in admission order — instead of the sorted list's last lane / lane swap; the two
    forms differ only in which of two equal members stays, which no attempt that goes on depends on."""
    near, visited = [[dist[ep], ep, False]], {ep}
    amb, twin_d, twin_left = None, None, 0
    while True:
        open_ = [m for m in near if not m[2]]
        if not open_:
            return near, amb
        cur = min(open_, key=lambda m: m[0]) if insert_form else open_[0]
        holders = sum(m[0] == cur[0] for m in open_)
        if holders > 2 or cur[0] == amb or (twin_left and (cur[0] != twin_d or holders != twin_left)):
            EVENTS["ended"] += 1
            return None
        if holders == 2 and twin_left == 0:
            twin_d, twin_left = cur[0], 2
            EVENTS["twin"] += 1
        cur[2] = True
        fresh = [v for v in lists[cur[1]] if v not in visited]
        visited.update(fresh)
        for v in fresh:
            if deleted[v]:
                continue
            d = dist[v]
            worst = max(m[0] for m in near)
            if len(near) < ef or d < worst:
                if twin_left and d < twin_d:
                    EVENTS["ended"] += 1
                    return None
                if len(near) == ef:
                    grp = [m for m in near if m[0] == worst]
                    if len(grp) > 1:
                        amb = worst
                        EVENTS["amb"] += 1
                    ex = [m for m in grp if m[2]] if len(grp) > 1 else []
                    if insert_form:
                        near.remove(ex[0] if ex else grp[0])
                    else:  # the last lane leaves; an expanded member trades places with an unexpanded one there first
                        EVENTS["swap"] += bool(ex) and not grp[-1][2]
                        near.remove(grp[-1] if grp[-1][2] or not ex else ex[0])
                if insert_form:
                    near.append([d, v, False])
                else:
                    near.insert(sum(m[0] < d for m in near), [d, v, False])  # before its equals, as the kernel's lanes
        if twin_left:
            twin_left -= 1


def restated_search(case, k, deleted_nodes=()):
    """(restart, [nodes]) of a search of the origin by the traversal's rules; the nodes only where there is no restart"""
    dist = distances(case)
    n = dist.size
    deleted = np.zeros(n, bool)
    deleted[list(deleted_nodes)] = True
    ep = 0
    if case.top:  # level 1, ef = 1: the lists there are top <-> 0; the first entry is read
        upper = {n - 1: [0], 0: [n - 1]}
        got = _layer(dist, upper, deleted, n - 1, 1, False)
        if got is None or got[0][0][0] == got[1]:
            return True, None
        ep = got[0][0][1]
    return restated_walk(dist, case.adj + ([[0]] if case.top else []), deleted, ep, case.ef, k)


def restated_walk(dist, lists, deleted, ep, ef, k):
    """layer 0 of a search by the traversal's rules: (restart, the k nodes where there is none)"""
    got = _layer(dist, lists, deleted, ep, ef, False)
    if got is None:
        return True, None
    near, amb = got
    read = len(near) if deleted.any() else min(len(near), k + 1)
    ds = [m[0] for m in near[:read]]
    if any(a == b for a, b in zip(ds, ds[1:])) or amb in ds:
        return True, None
    return False, [m[1] for m in near if not deleted[m[1]]][:k]


def restated_insert(case):
    """restart or not for the ef search of the device insert of the origin at level 0 (M0 = 8 >= ef: all of it is read)"""
    dist = distances(case)
    n = dist.size
    lists = case.adj + ([[0]] if case.top else [])
    start = n - 1 if case.top else 0
    while True:  # search_layer(ef = 1) on layer 0 from the entry point: the first neighbour holding the smallest distance
        nb = [v for v in lists[start]]
        best = min(nb, key=lambda v: dist[v], default=start)
        if dist[best] >= dist[start]:
            break
        start = best
    got = _layer(dist, lists, np.zeros(n, bool), start, case.ef, True)
    if got is None:
        return True
    near, amb = got
    ds = sorted(m[0] for m in near)  # M0 = 8: an equal pair that begins among the first 9 entries, amb in a list of at most 9
    return any(a == b for a, b in zip(ds[:9], ds[1:])) or (len(near) <= 9 and ds[-1] == amb)


# ---- the lattice fuzz --------------------------------------------------------------------------------------------------
def lattice_graph(seed, d, n=64, span=4):
    """x, ids, levels, off, nbrs, entry, deleted ids, the lists: n nodes on {-span..span}^2 (repeats allowed), all on level 0, lists of
    1-6 distinct random neighbours plus a ring link; on odd seeds an eighth of the nodes is soft-deleted, never node 0"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, d), np.float32)
    x[:, :2] = rng.integers(-span, span + 1, size=(n, 2))
    lists = []
    for i in range(n):
        others = np.delete(np.arange(n), i)
        row = rng.choice(others, size=int(rng.integers(1, 7)), replace=False).tolist()
        if (i + 1) % n not in row:
            row.insert(int(rng.integers(0, len(row) + 1)), (i + 1) % n)
        lists.append(row)
    ids = np.arange(n, dtype=np.uint64) + np.uint64(ID_BASE)
    off = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.uint64)
    nbrs = np.asarray([v for a in lists for v in a], np.uint64) + np.uint64(ID_BASE)
    dead = ids[1 + rng.choice(n - 1, n // 8, replace=False)] if seed % 2 else ids[:0]
    return x, ids, np.zeros(n, np.int64), off, nbrs, int(ids[0]), dead, lists


# The seeds of the traversal fuzz, four of them odd (soft deletes).  3, 4 and 8 are left out: by the restated rule every
# one of their 512 queries ends in a restart at some (k, ef) of the fuzz, and a batch that restarts whole says nothing
# about the branches that go on (test_tie_cases_data.py asserts the prediction for the seeds that are used).
LATTICE_SEEDS = (0, 1, 2, 5, 6, 7, 9, 10)
LATTICE_K_EF = ((1, 1), (1, 3), (2, 3), (3, 4), (5, 5), (3, 8))
LATTICE_B = 512


def lattice_queries(seed, d, b=LATTICE_B, span=4):
    q = np.zeros((b, d), np.float32)
    q[:, :2] = np.random.default_rng(1000 + seed).integers(-span, span + 1, size=(b, 2))
    return q


def lattice_rows(seed, n=300, d=16, span=6):
    x = np.zeros((n, d), np.float32)
    x[:, :2] = np.random.default_rng(2000 + seed).integers(-span, span + 1, size=(n, 2))
    return x
