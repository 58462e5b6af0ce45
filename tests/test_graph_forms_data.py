"""What test_gpu_graph_forms.py rests on, checked on the CPU: the synthetic graphs of _graph_forms.py are legal HNSW
adjacencies at the sizes used there, the sizes cross the byte-map / bit-map threshold of the traversal as the rule is
written (fvdb_graph.cpp, search_plan), and the oracle's walk over such a graph finds k hits — a graph on which the walk
dies at the entry point would make every parity test pass and test nothing."""
import functools

import numpy as np
import pytest

import oracle as orc
from _data import mixture
from _graph_forms import ID_BASE, synthetic_graph

# the smallest node count and batch that cross 2^30 map bytes with both factors (nearly) equal; B is not a multiple of 4,
# so the last workgroup of the sorted-register kernel (four queries each) is partial
N, B = 32832, 32771
N_WIDER = N + 4096  # another `words`
M, M0 = 16, 32


def ceil64(n):
    return (n + 63) // 64 * 64


def queries(x, d, seed, b=B):
    """b queries: mixture rows around the data's own means, then 64 stored rows (distance 0), then 64 stored rows
    nudged by 1e-3"""
    n = x.shape[0]
    q = mixture(b - 128, d, n_comp=8, seed=seed)  # the seed of the rows: the same means, other draws
    stored = x[(np.arange(64) * 509 + 3) % n]
    nudged = x[(np.arange(64) * 521 + 11) % n] + np.float32(1e-3)
    return np.ascontiguousarray(np.concatenate([q, stored, nudged]), np.float32)


def test_the_sizes_cross_the_threshold_as_the_rule_is_written():
    # one byte per node while ceil64(n) * max(B, 1024) <= 2^30, one bit per node above
    for n in (N, N_WIDER):
        assert ceil64(n) * max(B, 1024) > 2 ** 30
        assert ceil64(n) * max(1024, 1024) <= 2 ** 30
        assert ceil64(n) * max(33, 1024) <= 2 ** 30
    assert B % 4 != 0 and B > 1024
    assert (N + 31) // 32 != (N_WIDER + 31) // 32
    # the graph of the f32 test above 1024 dimensions stays on the byte map at any batch used there
    assert ceil64(2000) * 1024 <= 2 ** 30


def lists_of(levels, off):
    levels = np.asarray(levels, np.int64)
    node = np.repeat(np.arange(levels.size), levels + 1)
    first_slot = np.concatenate([[0], np.cumsum(levels + 1)])[:-1]
    layer = np.arange(node.size) - np.repeat(first_slot, levels + 1)
    return node, layer, np.asarray(off, np.int64)


@pytest.mark.parametrize("n,d,copies", [(N, 8, 1), (N, 8, 3), (N_WIDER, 8, 1), (2000, 1100, 1)])
def test_synthetic_graph_is_a_legal_adjacency(n, d, copies):
    orc.build()
    x, ids, levels, off, nbrs, entry = synthetic_graph(n, d, M, M0, seed=5, copies=copies)
    assert x.shape == (n, d) and x.dtype == np.float32 and np.isfinite(x).all()
    assert np.array_equal(ids, np.arange(n, dtype=np.uint64) + ID_BASE)
    assert np.array_equal(levels, orc.rng_levels(5, n))
    top = int(levels.max())
    assert top >= 1 and entry == int(ids[np.flatnonzero(levels == top)[0]])
    rows, counts = np.unique(x, axis=0, return_counts=True)
    assert rows.shape[0] == n // copies and np.all(counts == copies)
    if copies > 1:  # spread over the node numbers: the copies of a row are not neighbours in the numbering
        order = np.lexsort(x.T[::-1])
        gap = np.abs(np.diff(order.reshape(n // copies, copies), axis=1))
        assert np.median(gap) > n // 20

    node, layer, off = lists_of(levels, off)
    assert off.size == node.size + 1 and off[0] == 0 and off[-1] == nbrs.size
    lens = np.diff(off)
    assert lens.max() <= 63
    alone = np.bincount(layer)[layer] == 1  # a layer with one node: its list is empty, as in a built graph
    assert np.all(lens[~alone] >= 1) and np.all(lens[alone] == 0)
    assert np.all(lens[layer == 0] <= M0) and np.all(lens[layer > 0] <= M)
    assert lens[layer == 0].min() >= 8 and lens[layer == 0].max() > 8  # the ring, and random links beside it
    nb = nbrs.astype(np.int64) - ID_BASE
    assert nb.min() >= 0 and nb.max() < n
    owner = np.repeat(np.arange(node.size), lens)
    assert np.all(nb != node[owner]), "a node in its own list"
    key = owner * n + nb
    assert np.unique(key).size == key.size, "a list holds a node twice"
    assert np.all(levels[nb] >= layer[owner]), "a link on a layer its target does not reach"
    # the ring on layer 0: i +- 1..4 (mod n) are in i's list
    slot0 = np.flatnonzero(layer == 0)
    for step in (1, 2, 3, 4, -1, -2, -3, -4):
        assert np.isin(slot0 * n + (np.arange(n) + step) % n, key).all(), step
    # lists are not sorted copies of each other's order: the order inside a list is shuffled
    first = nb[off[:-1][slot0]]
    assert np.unique((first - np.arange(n)) % n).size > 100


@functools.lru_cache(maxsize=None)
def walked(copies):
    orc.build()
    d = 100
    x, ids, levels, off, nbrs, entry = synthetic_graph(N, d, M, M0, seed=100 + copies, copies=copies)
    o = orc.HNSWIndex(M, M0, 200, seed=1)
    o.restore(ids, x, levels, off, nbrs, entry)
    q = queries(x, d, seed=100 + copies, b=256)
    return x, ids, o, q


@pytest.mark.parametrize("copies", [1, 3])
def test_the_oracle_walks_such_a_graph_and_finds_k_hits(copies):
    x, ids, o, q = walked(copies)
    assert o.entry_point() is not None and o.node_count() == N
    oi, od, oc = o.batch_search(q, 10, 50)
    assert np.all(oc == 10)
    assert np.all(np.diff(od.astype(np.float64), axis=1) >= 0)
    # the walk goes somewhere: the answers differ between queries, and are not the entry point's neighbourhood
    assert np.unique(oi[:, 0]).size > 64
    # a graph of random links is a poor index, but some stored-row queries do find their row at distance 0
    assert np.any(od[128:192, 0] == 0)
    print(f"copies {copies}: {int(np.sum(od[128:192, 0] == 0))} of 64 stored rows found, "
          f"{int(np.sum((od[:, :-1] == od[:, 1:]).any(axis=1)))} of {q.shape[0]} queries return equal distances")
    oi1, od1, oc1 = o.batch_search(q, 1, 1)
    assert np.all(oc1 == 1)
    if copies > 1:  # ties are met: some query returns two hits at the same distance
        assert np.any(od[:, :-1] == od[:, 1:])
