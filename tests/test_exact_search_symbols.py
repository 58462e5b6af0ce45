"""Exact search and search quality: the new entry points are declared in the header, the export
list and the ctypes tables, and the numpy restatement test_gpu_exact_search.py leans on (_exact_ref.py) gives the
oracle's distance bits and order — proven here, on the CPU, before anything on a GPU is compared with it."""
import os
import re

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture
import _exact_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_SYMBOLS = ["fvdb_graph_search_flat_dev_slot", "fvdb_search_quality_lists_dev"]
HOST_SYMBOLS = ["fvh_hnsw_search_exact", "fvh_hnsw_search_exact_allowed", "fvh_hnsw_evaluate_search_quality",
                "fvh_hybrid_search_exact", "fvh_hybrid_evaluate_search_quality"]


def test_new_symbols_are_declared():
    fv = fvdb_import.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    lib, host = fv._capi.load(), fv.load_host()
    for name in C_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in fv._capi.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in HOST_SYMBOLS:
        assert name in fv.index.HOST_SIGNATURES, name
        assert hasattr(host, name), name
    # the two C entry points take what the header says: ten and nine arguments
    assert len(fv._capi.SIGNATURES["fvdb_graph_search_flat_dev_slot"][1]) == 10
    assert len(fv._capi.SIGNATURES["fvdb_search_quality_lists_dev"][1]) == 9


def test_the_three_index_classes_share_one_vocabulary():
    fv = fvdb_import.load()
    for cls in (fv.IVFIndex, fv.HNSWIndex, fv.HybridIndex):
        assert callable(getattr(cls, "search_exact")), cls.__name__
        assert callable(getattr(cls, "evaluate_search_quality")), cls.__name__
    assert callable(fv.HNSWIndex.search_exact_allowed)


@pytest.mark.parametrize("d", [10, 130, 384])
def test_numpy_restatement_gives_the_oracles_bits_and_order(d):
    """A one-list oracle IVF index searched with every list IS the flat exact search: every row scored with the
    reference's fold, a stable sort by distance over the scan order (= insertion order = row index)."""
    orc.build()
    n, k = 300, 40
    x = mixture(n, d, n_comp=4, seed=900 + d)
    # duplicated rows: pairs, a triple, and copies far apart — equal distances must come out in row order
    x = R.with_duplicates(x, [(5, 6), (20, 40), (20, 250), (100, 299), (0, 150)])
    q = np.concatenate([mixture(6, d, n_comp=4, seed=77 + d), x[[20, 5]]])  # two queries ON duplicated rows: distance 0 ties
    ids = np.arange(n, dtype=np.uint64)
    o = orc.IVFIndex(n_clusters=1, n_probe=1)
    o.set_trained(np.zeros((1, d), np.float32))
    o.batch_insert(ids, x)
    oi, od, oc = o.batch_search(q, k, 1)
    gi, gd, gc = R.exact_topk(R.fold_distances(q, x), k)
    assert np.array_equal(gc, oc) and np.all(gc == k)
    assert np.array_equal(bits(gd), bits(od)), "the numpy fold does not give the oracle's distance bits"
    assert np.array_equal(gi, oi), "lexsort((node, distance bits)) does not give the oracle's order"
    # the ties are really there and really decided by row index
    assert list(oi[6, :3]) == [20, 40, 250] and list(oi[7, :2]) == [5, 6]
    # and on the fp16-rounded rows
    xr = R.rounded(x)
    o2 = orc.IVFIndex(n_clusters=1, n_probe=1)
    o2.set_trained(np.zeros((1, d), np.float32))
    o2.batch_insert(ids, xr)
    oi, od, oc = o2.batch_search(q, k, 1)
    gi, gd, gc = R.exact_topk(R.fold_distances(q, xr), k)
    assert np.array_equal(bits(gd), bits(od)) and np.array_equal(gi, oi)


def test_host_quality_restates_the_reference_formulas():
    class Res:
        def __init__(self, ids, counts):
            self.ids, self.counts = np.asarray(ids, np.uint64), np.asarray(counts, np.uint32)
    # query 0: 2 of 3 match; query 1: empty truth -> recall 1, precision 0; query 2: an id returned twice counts twice
    res = Res([[1, 2, 9], [4, 5, 6], [7, 7, 8]], [3, 3, 3])
    truth = Res([[1, 2, 3], [0, 0, 0], [7, 1, 2]], [3, 0, 3])
    ar, ap = R.host_quality(res, truth, 3)
    f = np.float32
    want_r = f(f(f(f(2) / f(3)) + f(1)) + f(f(2) / f(3))) / f(3)
    want_p = f(f(f(f(2) / f(3)) + f(0)) + f(f(2) / f(3))) / f(3)
    assert ar == want_r and ap == want_p
