"""Radius search: the new C entry points are declared, exported and bound with the stated
arguments, the host mirror's wrappers are in HOST_SIGNATURES and exported, and the Python methods exist.  No GPU."""
import inspect
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> number of arguments, as include/fvdb.h declares them
C_SYMBOLS = {"fvdb_graph_search_flat_radius_dev_slot": 12, "fvdb_graph_count_within_dev_slot": 8,
             "fvdb_ivf_search_radius_dev_slot": 13, "fvdb_ivf_search_radius": 10}
HOST_SYMBOLS = {"fvh_hnsw_search_radius": 10, "fvh_hnsw_search_radius_allowed": 12, "fvh_hnsw_count_within": 8,
                "fvh_ivf_search_radius": 13, "fvh_hybrid_search_radius": 16}


def test_the_c_entry_points_are_declared_exported_and_bound():
    fv = fvdb_import.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    lib = fv._capi.load()
    for name, arity in C_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == arity, f"{name}: declared with another number of arguments"
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(fv._capi.SIGNATURES[name][1]) == arity, f"{name}: bound with another number of arguments"
    # the radius forms take their wide sibling's arguments with (radius, max_results) for k, and one more output
    wide = fv._capi.SIGNATURES["fvdb_graph_search_flat_wide_dev_slot"][1]
    assert len(fv._capi.SIGNATURES["fvdb_graph_search_flat_radius_dev_slot"][1]) == len(wide) + 2
    wide = fv._capi.SIGNATURES["fvdb_ivf_search_wide_dev_slot"][1]
    assert len(fv._capi.SIGNATURES["fvdb_ivf_search_radius_dev_slot"][1]) == len(wide) + 1  # + radius + totals - keys
    assert re.search(r"#define\s+FVDB_MAX_K_WIDE\s+4096u", header)


def test_the_host_mirror_exports_the_radius_wrappers():
    fv = fvdb_import.load()
    host = fv.load_host()
    sig = fv.index.HOST_SIGNATURES
    for name, arity in HOST_SYMBOLS.items():
        assert name in sig, name
        assert hasattr(host, name), name
        assert len(sig[name][1]) == arity, name


def test_the_python_methods_exist():
    fv = fvdb_import.load()
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(fv.IVFIndex.search_radius) == ["self", "queries", "radius", "max_results", "n_probe", "allowed"]
    assert params(fv.HNSWIndex.search_radius) == ["self", "queries", "radius", "max_results", "allowed"]
    assert params(fv.HNSWIndex.count_within) == ["self", "queries", "radius", "allowed"]
    assert params(fv.HybridIndex.search_radius)[:8] == ["self", "queries", "radius", "max_results", "now", "ivf_n_probe",
                                                        "search_recent", "search_historical"]
    assert params(fv.VectorDbSession.search_within) == ["self", "query_vector", "threshold", "options"]
    for f in (fv.IVFIndex.search_radius, fv.HNSWIndex.search_radius, fv.HybridIndex.search_radius):
        assert inspect.signature(f).parameters["max_results"].default == 4096
    assert callable(fv.session.radius_of_threshold)
