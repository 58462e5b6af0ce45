"""Exact search at k up to 4096 over the graph and the hybrid index: the new C entry point is
declared, exported and bound, the host mirror's new wrappers are in HOST_SIGNATURES and exported, and the Python
methods exist.  No GPU."""
import inspect
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_SYMBOL = "fvdb_graph_search_flat_wide_dev_slot"
HOST_SYMBOLS = ["fvh_hnsw_search_exact_wide", "fvh_hnsw_search_exact_wide_allowed", "fvh_hnsw_evaluate_search_quality_wide",
                "fvh_hybrid_search_exact_wide", "fvh_hybrid_evaluate_search_quality_wide"]


def test_the_c_entry_point_is_declared_exported_and_bound():
    fv = fvdb_import.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % C_SYMBOL, header)
    assert hasattr(fv._capi.load(), C_SYMBOL)
    # the arguments of the register form, one for one
    assert fv._capi.SIGNATURES[C_SYMBOL] == fv._capi.SIGNATURES["fvdb_graph_search_flat_dev_slot"]
    # and the limit it is documented against
    assert re.search(r"#define\s+FVDB_MAX_K_WIDE\s+4096u", header)


def test_the_host_mirror_exports_the_wide_wrappers():
    fv = fvdb_import.load()
    host = fv.load_host()
    sig = fv.index.HOST_SIGNATURES
    for name in HOST_SYMBOLS:
        assert name in sig, name
        assert hasattr(host, name), name
        assert sig[name] == sig[name.replace("_wide", "")], f"{name} takes what its register form takes"


def test_the_python_methods_exist():
    fv = fvdb_import.load()
    for cls, names in ((fv.HNSWIndex, ["search_exact_wide", "search_exact_wide_allowed", "evaluate_search_quality_wide"]),
                       (fv.HybridIndex, ["search_exact_wide", "evaluate_search_quality_wide"]),
                       (fv.VectorDbSession, ["evaluate_search_quality"])):
        for n in names:
            assert callable(getattr(cls, n)), f"{cls.__name__}.{n}"
    p = list(inspect.signature(fv.HybridIndex.search_exact_wide).parameters)
    assert p == ["self", "queries", "k", "now", "search_recent", "search_historical"]
    p = list(inspect.signature(fv.HybridIndex.evaluate_search_quality_wide).parameters)
    assert p == ["self", "queries", "k", "now", "hnsw_ef", "ivf_n_probe"]
    p = list(inspect.signature(fv.VectorDbSession.evaluate_search_quality).parameters)
    assert p == ["self", "queries", "k", "options"]
