"""Half-precision rows in the row store and the index classes are declared, exported and bound:
header, both libraries and the ctypes tables agree, and the three index classes take `row_dtype`."""
import inspect
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = {  # name: (return type in the header, argument count)
    "fvdb_store_create_ex": ("int", 5),   # ctx, d, capacity_rows, row_dtype, out
    "fvdb_store_dtype": ("int", 1),       # store
    "fvdb_store_bytes": ("uint64_t", 1),  # store
}
HOST = {
    "fvh_ivf_new_ex": 7,       # fvh_ivf_new's six + row_dtype
    "fvh_hnsw_new_ex": 6,      # fvh_hnsw_new's five + row_dtype
    "fvh_hybrid_new_ex": 16,   # fvh_hybrid_new's fifteen + row_dtype
    "fvh_round_f16": 3,        # in, n, out
    "fvh_ivf_row_dtype": 1,
    "fvh_hnsw_row_dtype": 1,
    "fvh_hnsw_store_bytes": 1,
}


def test_header_declares_the_store_entries():
    text = open(os.path.join(ROOT, "include", "fvdb.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (ret, nargs) in ENGINE.items():
        m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), code)
        assert m, f"{name} is not declared in include/fvdb.h"
        assert len(m.group(1).split(",")) == nargs, f"{name}: argument count"
    assert re.search(r"\bint\s+fvdb_store_create\s*\(", code), "fvdb_store_create stays"


def test_ctypes_tables_list_them():
    fv = fvdb_import.load()
    for name, (_, nargs) in ENGINE.items():
        assert name in fv._capi.SIGNATURES
        assert len(fv._capi.SIGNATURES[name][1]) == nargs, name
    for name, nargs in HOST.items():
        assert name in fv.index.HOST_SIGNATURES
        assert len(fv.index.HOST_SIGNATURES[name][1]) == nargs, name
    # the _ex constructors are the existing ones plus one argument
    for old in ("fvh_ivf_new", "fvh_hnsw_new", "fvh_hybrid_new"):
        assert fv.index.HOST_SIGNATURES[old + "_ex"][1][:-1] == fv.index.HOST_SIGNATURES[old][1]


def test_built_libraries_export_them():
    fv = fvdb_import.load()
    lib = fv._capi.load()
    for name in ENGINE:
        assert hasattr(lib, name), f"{name} is not exported by libfvdb_hip.so"
    host = fv.load_host()
    for name in HOST:
        assert hasattr(host, name), f"{name} is not exported by libfvdb_host.so"
    for old in ("fvh_ivf_new", "fvh_hnsw_new", "fvh_hybrid_new"):
        assert hasattr(host, old), f"{old} stays"


def test_index_classes_take_row_dtype():
    fv = fvdb_import.load()
    for cls in (fv.IVFIndex, fv.HNSWIndex, fv.HybridIndex):
        p = inspect.signature(cls.__init__).parameters
        assert "row_dtype" in p and p["row_dtype"].default == "f32", cls.__name__
    assert callable(getattr(fv.HNSWIndex, "store_bytes", None))
    assert "dtype" in inspect.signature(fv.RowStore.__init__).parameters
