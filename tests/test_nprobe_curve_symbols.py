"""Recall and precision at every n_probe from one search of every list: the new symbols are
declared, and the rule the device kernels implement is pinned — through the oracle alone — against what it replaces: a
search at n_probe = p compared with the search of every list, for every p."""
import os
import re

import numpy as np
import pytest

import fvdb_import
import oracle as orc
import _any_nprobe_data as D
import _curve_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_declared():
    fv = fvdb_import.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    assert re.search(r"\bfvdb_ivf_quality_curve_dev\s*\(", header)
    assert "fvdb_ivf_quality_curve_dev" in fv._capi.SIGNATURES
    assert len(fv._capi.SIGNATURES["fvdb_ivf_quality_curve_dev"][1]) == 10
    assert "fvh_ivf_quality_curve" in fv.index.HOST_SIGNATURES
    assert hasattr(fv._capi.load(), "fvdb_ivf_quality_curve_dev")
    assert hasattr(fv.load_host(), "fvh_ivf_quality_curve")
    for name in ("recall_by_nprobe", "smallest_n_probe"):
        assert callable(getattr(fv.IVFIndex, name))
        assert not hasattr(fv.HybridIndex, name), "the hybrid index has the curve through h.ivf()"


def cases():
    x, ids, cents, q = D.quality_case()
    yield "quality", x, ids, cents, None, q, ()
    yield "quality_third_deleted", x, ids, cents, None, q, tuple(int(i) for i in ids[::3])
    x, ids, cents, cl, q = D.tie_case()
    yield "tie", x, ids, cents, cl, q, ()


@pytest.mark.parametrize("k", [10, 300])
@pytest.mark.parametrize("case", list(cases()), ids=lambda c: c[0])
def test_the_rule_equals_the_repeated_searches_at_every_p(case, k):
    orc.build()
    _, x, ids, cents, clusters, q, dead = case
    cpu, cl = D.oracle_index(x, ids, cents, clusters=clusters)
    for i in dead:
        cpu.mark_deleted(i)
    live = R.live_sizes(ids, cl, D.NLIST, None if not dead else set(int(i) for i in ids) - set(dead))
    recall, precision, length = R.curve_per_query(cpu, q, k, cents, ids, cl, live)
    truth = cpu.batch_search(q, k, D.NLIST, threads=8)
    for p in range(1, D.NLIST + 1):
        res = cpu.batch_search(q, k, p, threads=8)
        want_recall, want_precision = D.per_query_quality(res, truth, k)
        assert np.array_equal(length[:, p - 1], res[2]), f"p={p}: result lengths"
        assert np.array_equal(recall[:, p - 1].view(np.uint32), want_recall.view(np.uint32)), f"p={p}: recall"
        assert np.array_equal(precision[:, p - 1].view(np.uint32), want_precision.view(np.uint32)), f"p={p}: precision"
    # the averages: column by column the reference's fold
    for p in (1, 2, 17, D.NLIST):
        assert R.curve_averages(recall)[p - 1].view(np.uint32) == D.averaged(recall[:, p - 1]).view(np.uint32)
    assert np.all(recall[:, -1] == 1), "the truth against itself"
