"""No GPU: the filtered exact search (include/fvdb.h) is declared, exported and bound with equal
arity in the engine, and the host mirror and the Python classes carry its entry points."""
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fvdb_graph_search_flat_mfma_dev_slot", "fvdb_graph_flat_mfma_info"]
HOST = ["fvh_hnsw_search_exact_filtered", "fvh_hnsw_search_exact_filtered_allowed", "fvh_hnsw_exact_filter_info",
        "fvh_hybrid_search_exact_filtered"]


def test_filtered_entry_points_declared_exported_bound():
    fv = fvdb_import.load()
    lib = fv._capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fvdb_graph_[a-z0-9_]*flat_mfma[a-z0-9_]*)\s*\(", text))) == sorted(NAMES)
    for n in NAMES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert hasattr(lib, n), f"{n} is not exported"
        assert len(fv._capi.SIGNATURES[n][1]) == len([a for a in args.split(",") if a.strip()]), n
    # the filtered search takes the flat search's arguments
    assert fv._capi.SIGNATURES[NAMES[0]] == fv._capi.SIGNATURES["fvdb_graph_search_flat_dev_slot"]
    fields = [f for f, _ in fv._capi.FlatMfmaInfo._fields_]
    body = re.search(r"typedef struct fvdb_flat_mfma_info \{(.*?)\} fvdb_flat_mfma_info;", text, flags=re.S).group(1)
    declared = [re.sub(r"\[\d+\]", "", w.strip()) for d in re.findall(r"(?:uint64_t|uint32_t|float)\s+([^;]+);", body) for w in d.split(",")]
    assert fields == declared


def test_filtered_host_mirror_and_classes():
    fv = fvdb_import.load()
    host = fv.load_host()
    for n in HOST:
        assert n in fv.index.HOST_SIGNATURES and hasattr(host, n), n
    assert fv.index.HOST_SIGNATURES[HOST[0]] == fv.index.HOST_SIGNATURES["fvh_hnsw_search_exact"]
    assert fv.index.HOST_SIGNATURES[HOST[3]] == fv.index.HOST_SIGNATURES["fvh_hybrid_search_exact"]
    for cls, names in ((fv.HNSWIndex, "search_exact_filtered exact_filter_info"), (fv.HybridIndex, "search_exact_filtered")):
        for name in names.split():
            assert callable(getattr(cls, name))
