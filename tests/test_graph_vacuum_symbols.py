"""No GPU needed: the resident graph vacuum is declared, exported and bound at every layer."""
import os

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_carries_the_graph_vacuum_entries():
    fv = fvdb_import.load()
    lib = fv._capi.load()
    header = open(os.path.join(ROOT, "include", "fvdb.h")).read()
    for name in ("fvdb_graph_vacuum", "fvdb_graph_maintenance_info"):
        assert name + "(" in header
        assert name in fv._capi.SIGNATURES and hasattr(lib, name)
    assert "FVDB_VACUUM_KEEP_ROWS" in header and fv._capi.VACUUM_KEEP_ROWS == 1
    fields = [n for n, _ in fv._capi.GraphMaintenanceInfo._fields_]
    assert fields == ["nodes_in", "nodes_out", "edges_in", "edges_out", "rows_reclaimed", "bytes_reclaimed", "host_bytes",
                      "move_bytes", "ms_scan", "ms_prune", "ms_move", "ms_total"]
    # the struct in the header names the same fields in the same order
    struct = header[header.index("typedef struct fvdb_graph_maintenance_info_t"):header.index("} fvdb_graph_maintenance_info_t")]
    at = [struct.index(f) for f in fields]
    assert at == sorted(at)


def test_host_mirror_carries_the_vacuum_status_info_and_switch():
    fv = fvdb_import.load()
    host = fv.load_host()
    for name in ("fvh_hnsw_vacuum", "fvh_hnsw_vacuum_ex", "fvh_hnsw_vacuum_info", "fvh_hnsw_set_resident_vacuum",
                 "fvh_hnsw_resident_vacuum", "fvh_hnsw_set_vacuum_keep_rows", "fvh_hnsw_store_rows"):
        assert name in fv.index.HOST_SIGNATURES and hasattr(host, name)
    for method in ("vacuum", "vacuum_info", "store_rows", "set_resident_vacuum", "resident_vacuum"):
        assert callable(getattr(fv.HNSWIndex, method))
