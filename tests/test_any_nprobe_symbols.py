"""Search at any nprobe and evaluate_search_quality: the new symbols are declared, and the data
generators of test_gpu_any_nprobe.py meet their conditions — checked through the oracle alone, so a seed that misses one
is caught before anything runs on a GPU."""
import os
import re

import numpy as np

import fvdb_import
import oracle as orc
import _any_nprobe_data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_declared():
    fv = fvdb_import.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    assert re.search(r"\bfvdb_ivf_search_quality_dev\s*\(", header)
    assert "fvdb_ivf_search_quality_dev" in fv._capi.SIGNATURES
    assert "fvh_ivf_evaluate_search_quality" in fv.index.HOST_SIGNATURES
    assert hasattr(fv._capi.load(), "fvdb_ivf_search_quality_dev")
    assert hasattr(fv.load_host(), "fvh_ivf_evaluate_search_quality")
    assert callable(getattr(fv.IVFIndex, "evaluate_search_quality"))


def test_quality_data_separates_recall_from_precision():
    orc.build()
    x, ids, cents, q = D.quality_case()
    cpu, cl = D.oracle_index(x, ids, cents)
    sizes = np.bincount(cl, minlength=D.NLIST)
    assert np.all(sizes[280:] == 0), "the repeated centroids own no rows"
    recall, precision, _, _ = D.expected_quality(cpu, q, 10, 2)
    assert np.count_nonzero(recall < 1) * 4 >= q.shape[0], "n_probe = 2 must miss neighbours for a quarter of the queries"
    assert np.any(recall != precision), "some query's two lists hold fewer than k rows"
    # a k larger than any two lists: every result is short, so no query reaches recall 1 and the two figures part
    assert np.all(cpu.batch_search(q, 200, 2)[2] < 200)
    recall, precision, _, _ = D.expected_quality(cpu, q, 200, 2)
    assert np.all(recall < 1) and np.all(precision > recall)
    # the ground truth against itself
    recall, precision, ar, ap = D.expected_quality(cpu, q, 10, D.NLIST)
    assert ar == 1 and ap == 1


def test_tie_data_orders_by_probe_rank():
    orc.build()
    x, ids, cents, cl, q = D.tie_case()
    cpu, _ = D.oracle_index(x, ids, cents, clusters=cl)
    for k in (10, 300):
        oi, od, oc = cpu.batch_search(q, k, D.NLIST)
        assert np.all(oc == k)
        by_list = D.list_order_answer(x, ids, cl, q, k)
        differ = [b for b in range(q.shape[0]) if not np.array_equal(oi[b], by_list[b])]
        assert differ, f"k={k}: a scan in list order gives the oracle's answer: the case decides nothing"
        # both answers hold rows at the same distances: only the order among equals differs
        row_of = {int(i): r for r, i in enumerate(ids)}
        for b in differ:
            theirs = orc.l2_batch(q[b], x[[row_of[int(i)] for i in by_list[b]]])
            assert np.array_equal(theirs.view(np.uint32), od[b].view(np.uint32))
    # the coarse order has ties too: the query on a twin centroid sees both at distance 0
    d0 = orc.l2_batch(q[0], cents)
    assert d0[10] == 0 and d0[200] == 0
