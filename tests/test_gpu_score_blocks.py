"""The register-resident transposed-product scorer (score_fixed, csrc/score_rows.h) at every block count and row count
the other GPU tests do not reach: the device insert (one product tile) and the traversal (two) must build the CPU oracle's
graph and return its results bit for bit at

  d = 128         NB = 1 with dpad == 128: the traversal's path without bounds checks
  d = 200, 260    NB = 2 and NB = 3, bounds-checked
  d = 500         NB = 4 with R = 12
  d = 600         NB = 5: served by the NB = 6 kernel with R = 8, and by the build's 8-row ladder
  d = 1000, 1024  NB = 8 with R = 6, bounds-checked and full (at d = 1000 two of the 250 returned distances are equal:
                  the tie path resolves them as the reference does)
"""
import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture

pytestmark = pytest.mark.gpu

N, M, M0, EFC, NQ, K, EF = 240, 6, 12, 40, 25, 10, 50
DIMS = [128, 200, 260, 500, 600, 1000, 1024]


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle_case(ctx):
    """d -> (rows, ids, levels, queries, the oracle's index, the oracle's results): computed once, read by both modes"""
    cache = {}

    def get(d):
        if d not in cache:
            x = mixture(N, d, n_comp=8, seed=d)
            ids = np.arange(N, dtype=np.uint64) + 7
            levels = orc.rng_levels(d, N)
            oh = orc.HNSWIndex(M, M0, EFC, seed=d)
            oh.batch_insert(ids, x, levels)
            q = mixture(NQ, d, n_comp=8, seed=d + 100)
            cache[d] = (x, ids, levels, q, oh, oh.batch_search(q, K, EF))
        return cache[d]

    return get


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


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("mode", [1, 2])
def test_insert_and_traversal_match_the_oracle_at_every_block_count(fv, ctx, oracle_case, d, mode):
    x, ids, levels, q, oh, want = oracle_case(d)
    assert np.array_equal(want[2], np.full(NQ, K))  # every query has its 10 results: the comparison below is about all of them
    gh = fv.HNSWIndex(ctx, M, M0, EFC, seed=d)
    gh.set_device_insert(True, mode)
    ok, bad = gh.batch_insert(ids, x, levels)
    assert (ok, bad) == (N, 0)
    assert gh.insert_stats()["host_path_inserts"] == 0
    same_graph(gh, oh)
    for device in (True, False):
        gh.set_device_traversal(device)
        same_results(gh.search(q, K, EF), want)
