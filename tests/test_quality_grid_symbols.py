"""Search quality over a grid of ef and n_probe: the new symbols are declared, exported and bound,
and the Python methods have the parameter lists the design states.  No GPU."""
import inspect
import os
import re

import numpy as np

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_c_symbol_is_declared_exported_and_bound():
    fv = fvdb_import.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    assert re.search(r"\bfvdb_quality_grid_dev\s*\(", header)
    assert "fvdb_quality_grid_dev" in fv._capi.SIGNATURES
    assert len(fv._capi.SIGNATURES["fvdb_quality_grid_dev"][1]) == 17
    assert hasattr(fv._capi.load(), "fvdb_quality_grid_dev")


def test_the_host_wrappers_are_bound_and_exported():
    fv = fvdb_import.load()
    assert len(fv.index.HOST_SIGNATURES["fvh_hnsw_quality_by_ef"][1]) == 11
    assert len(fv.index.HOST_SIGNATURES["fvh_hybrid_quality_grid"][1]) == 18
    host = fv.load_host()
    for name in ("fvh_hnsw_quality_by_ef", "fvh_hybrid_quality_grid"):
        assert hasattr(host, name)


def test_the_python_methods_and_their_parameters():
    fv = fvdb_import.load()
    want = {
        (fv.HNSWIndex, "recall_by_ef"): ["self", "queries", "k", "efs"],
        (fv.HNSWIndex, "smallest_ef"): ["self", "queries", "k", "target_recall", "efs"],
        (fv.HybridIndex, "quality_grid"): ["self", "queries", "k", "efs", "n_probes", "now", "search_recent", "search_historical"],
        (fv.HybridIndex, "operating_points"): ["self", "queries", "k", "target_recall", "efs", "n_probes", "now"],
        (fv.VectorDbSession, "quality_grid"): ["self", "queries", "k", "efs", "n_probes"],
    }
    for (cls, name), params in want.items():
        sig = inspect.signature(getattr(cls, name))
        assert list(sig.parameters) == params, f"{cls.__name__}.{name}"
    sig = inspect.signature(fv.HybridIndex.quality_grid).parameters
    assert (sig["now"].default, sig["search_recent"].default, sig["search_historical"].default) == (0.0, True, True)
    assert inspect.signature(fv.HybridIndex.operating_points).parameters["now"].default == 0.0
    # evaluate_search_quality's own signature stays as it was
    assert list(inspect.signature(fv.VectorDbSession.evaluate_search_quality).parameters) == ["self", "queries", "k", "options"]


def test_operating_points_on_a_hand_checkable_grid():
    fv = fvdb_import.load()
    f = np.float32
    grid = dict(efs=[40, 10, 20, 10], n_probes=[4, 1, 2],
                avg_recall=np.array([[.99, .95, .96],   # ef 40
                                     [.96, .50, .90],   # ef 10
                                     [.97, .60, .95],   # ef 20
                                     [.96, .50, .90]], f),  # ef 10 again
                avg_precision=np.zeros((4, 3), f))
    pts = fv.index.pareto_points(grid, 0.95)
    # reaching: (40,4) (40,1) (40,2) (10,4) (20,4) (20,2); (40,4), (40,2) fall to (40,1); (20,4) to (20,2) and (10,4)
    assert [(p["ef"], p["n_probe"]) for p in pts] == [(10, 4), (20, 2), (40, 1)]
    assert [p["avg_recall"] for p in pts] == [f(.96), f(.95), f(.95)]
    assert fv.index.pareto_points(grid, 0.995) == []
    # the target is compared in f32: 0.95 as a double is below f32(0.95), and still reaches
    assert f(.95) >= f(0.95) and len(fv.index.pareto_points(grid, 0.95)) == 3
