"""A synthetic HNSW graph to restore (fv.HNSWIndex.restore / orc.HNSWIndex.restore take any adjacency): large enough to
select a traversal form by its node count, made in milliseconds — vectorised numpy, no loop over the nodes."""
import numpy as np

import oracle as orc
from _data import mixture

ID_BASE = 1000  # id of node i is i + ID_BASE: ids and node numbers are never interchangeable by accident


def _offsets(m, ring, cap, rng):
    """(m, w) offsets, each row distinct values in 1..m-1: all of them while m - 1 <= cap, else +-1..+-ring first and
    then one draw from each of cap - 2 * ring equal strata of ring+1 .. m-ring-1 (distinct by construction)."""
    if m - 1 <= cap:
        return np.tile(np.arange(1, m, dtype=np.int64), (m, 1)), m - 1
    steps = np.arange(1, ring + 1, dtype=np.int64)
    fixed = np.concatenate([steps, m - steps])
    r = cap - 2 * ring
    lo, hi = ring + 1, m - ring
    edges = lo + (np.arange(r + 1, dtype=np.int64) * (hi - lo)) // r
    rand = rng.integers(edges[:-1], edges[1:], size=(m, r))
    return np.concatenate([np.tile(fixed, (m, 1)), rand], axis=1), 2 * ring


def _layer(members, ring, cap, rng):
    """lists among `members` (ascending node numbers): per member a row of neighbours and how many of them count; the
    ring links always count, the random ones up to a random degree, and the list order is shuffled"""
    m = members.size
    if m < 2:
        return np.zeros((m, 0), np.int64), np.zeros(m, np.int64)
    off, least = _offsets(m, ring, cap, rng)
    w = off.shape[1]
    deg = rng.integers(least, w + 1, size=m)
    pos = (np.arange(m, dtype=np.int64)[:, None] + off) % m
    key = rng.random((m, w))
    key[np.arange(w)[None, :] >= deg[:, None]] = 2.0  # the columns past the degree sort last
    order = np.argsort(key, axis=1, kind="stable")
    return members[np.take_along_axis(pos, order, axis=1)], deg


def synthetic_graph(n, d, M, M0, seed, copies=1):
    """x, ids, levels, off, nbrs, entry for restore().  Rows: _data.mixture; with copies = c every row is present c times,
    the copies spread over the node numbers by a permutation.  Levels: orc.rng_levels; entry: the first node of the top
    level.  Layer 0: ring links to +-1..+-4 plus random links, up to M0 per node; layer l >= 1: ring links to +-1, +-2
    plus random links among the nodes of that level, up to M.  Every list holds distinct nodes, never the node itself."""
    assert n % copies == 0 and 8 <= M0 <= 63 and 4 <= M <= 63 and n > M0 + 1
    rng = np.random.default_rng(seed)
    base = mixture(n // copies, d, n_comp=8, seed=seed)
    x = base if copies == 1 else np.ascontiguousarray(base[rng.permutation(n) % (n // copies)])
    ids = np.arange(n, dtype=np.uint64) + np.uint64(ID_BASE)
    levels = np.asarray(orc.rng_levels(seed, n), np.int64)
    top = int(levels.max())
    entry = int(ids[np.flatnonzero(levels == top)[0]])
    first_slot = np.concatenate([[0], np.cumsum(levels + 1)])  # lists in node order, layer 0 first
    lens = np.zeros(first_slot[-1], np.int64)
    layers = []
    for layer in range(top + 1):
        members = np.flatnonzero(levels >= layer)
        rows, deg = _layer(members, 4 if layer == 0 else 2, M0 if layer == 0 else M, rng)
        slots = first_slot[members] + layer
        lens[slots] = deg
        layers.append((rows, deg, slots))
    off = np.concatenate([[0], np.cumsum(lens)])
    nbrs = np.zeros(off[-1], np.uint64)
    for rows, deg, slots in layers:
        keep = np.arange(rows.shape[1])[None, :] < deg[:, None]
        within = np.broadcast_to(np.arange(rows.shape[1])[None, :], rows.shape)[keep]
        nbrs[np.repeat(off[slots], deg) + within] = ids[rows[keep]]
    return x, ids, levels, off.astype(np.uint64), nbrs, entry
