"""No GPU needed: the graph-health job is declared, exported and bound at every layer."""
import ctypes
import os

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_carries_the_graph_health_entries():
    fv = fvdb_import.load()
    lib = fv._capi.load()
    header = open(os.path.join(ROOT, "include", "fvdb.h")).read()
    for name in ("fvdb_graph_health", "fvdb_graph_health_nodes"):
        assert name + "(" in header
        assert name in fv._capi.SIGNATURES and hasattr(lib, name)
    assert "FVDB_HEALTH_SKIP_REACH 1u" in header and fv._capi.HEALTH_SKIP_REACH == 1
    assert "FVDB_HEALTH_SKIP_COMPONENTS 2u" in header and fv._capi.HEALTH_SKIP_COMPONENTS == 2
    fields = [n for n, _ in fv._capi.GraphHealth._fields_]
    assert fields == ["n_nodes", "n_live", "has_entry", "entry_live", "entry_level", "max_level_live", "edge_slots_live",
                      "dangling", "dangling0", "degree0_hist", "reachable_live", "unreachable_live", "reach_rounds0",
                      "components0", "largest_component0", "isolated0", "launches", "reach_launches", "host_syncs", "ms",
                      "scratch_bytes"]
    struct = header[header.index("typedef struct fvdb_graph_health_t"):header.index("} fvdb_graph_health_t")]
    at = [struct.index(f) for f in fields]
    assert at == sorted(at)
    # 6 + 65 + 9 words, three 64-bit figures, the float, padding to 8, the 64-bit byte count
    assert ctypes.sizeof(fv._capi.GraphHealth) == 24 + 24 + 260 + 36 + 4 + 4 + 8
    assert fv._capi.GraphHealth.edge_slots_live.offset == 24 and fv._capi.GraphHealth.scratch_bytes.offset == 352


def test_integration_document_lists_the_entries():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fvdb_graph_health(" in text and "fvdb_graph_health_nodes(" in text


def test_host_mirror_and_python_surface_carry_the_health_methods():
    fv = fvdb_import.load()
    host = fv.load_host()
    for name in ("fvh_hnsw_graph_stats", "fvh_hnsw_max_level", "fvh_hnsw_level_distribution", "fvh_hnsw_graph_health",
                 "fvh_hnsw_unreachable", "fvh_hnsw_component_labels"):
        assert name in fv.index.HOST_SIGNATURES and hasattr(host, name)
    for method in ("get_graph_stats", "get_level_distribution", "get_max_level", "graph_health", "unreachable_ids",
                   "component_labels"):
        assert callable(getattr(fv.HNSWIndex, method))
    assert callable(fv.VectorDbSession.graph_health)
