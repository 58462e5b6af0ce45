"""The row gathers (rows by location, migration from a row store in HBM) are declared, exported and bound: header,
library and ctypes table agree; the host mirror exports what index.py binds."""
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {
    "fvdb_ivf_get_rows": 5,                     # ivf, cluster, pos, n, out
    "fvdb_ivf_get_rows_dev": 6,                 # ivf, ctx, cluster, pos, n, out
    "fvdb_ivf_assign_from_store": 5,            # ivf, store, rows, n, out_cluster
    "fvdb_ivf_add_assigned_from_store": 7,      # ivf, store, rows, ids, n, cluster, out_pos
}
HOST = ("fvh_ivf_get_vectors", "fvh_hybrid_get_vectors", "fvh_hybrid_set_resident_migration", "fvh_hybrid_migration_info")


def test_header_declares_the_row_entries():
    text = open(os.path.join(ROOT, "include", "fvdb.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, nargs in ROWS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in include/fvdb.h"
        assert len(m.group(1).split(",")) == nargs, f"{name}: argument count"


def test_ctypes_table_lists_them():
    fv = fvdb_import.load()
    for name, nargs in ROWS.items():
        assert name in fv._capi.SIGNATURES
        assert len(fv._capi.SIGNATURES[name][1]) == nargs, name
    for name in HOST:
        assert name in fv.index.HOST_SIGNATURES


def test_built_libraries_export_them():
    fv = fvdb_import.load()
    lib = fv._capi.load()
    for name in ROWS:
        assert hasattr(lib, name), f"{name} is not exported by libfvdb_hip.so"
    host = fv.load_host()
    for name in HOST:
        assert hasattr(host, name), f"{name} is not exported by libfvdb_host.so"


def test_python_surface_has_the_methods():
    fv = fvdb_import.load()
    for cls, names in ((fv.IVFIndex, ("get_vector_by_id", "get_vectors")),
                       (fv.HybridIndex, ("get_vectors", "set_resident_migration", "migration_info"))):
        for n in names:
            assert callable(getattr(cls, n, None)), f"{cls.__name__}.{n}"
