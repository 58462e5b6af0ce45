"""No GPU: the IVF-over-PQ entry points (include/fvdb.h) are declared, exported and bound with
equal arity, and the class and its methods are exported from the package."""
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fvdb_ivfpq_" + n for n in (
    "create destroy train set_centroids get_centroids add set_deleted rows live bytes list_sizes info search "
    "search_dev_slot").split()]


def test_ivfpq_entry_points_declared_exported_bound():
    fv = fvdb_import.load()
    lib = fv._capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fvdb_ivfpq_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NAMES)
    for n in NAMES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert hasattr(lib, n), f"{n} is not exported"
        assert len(fv._capi.SIGNATURES[n][1]) == len([a for a in args.split(",") if a.strip() not in ("", "void")]), n


def test_ivfpq_class_exported():
    fv = fvdb_import.load()
    for name in "train set_centroids centroids add mark_deleted rows live bytes list_sizes info search close".split():
        assert callable(getattr(fv.IVFPQIndex, name))
