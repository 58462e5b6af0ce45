"""No GPU: the binary-quantization entry points (include/fvdb.h) are declared, exported and bound
with equal arity, and the class and the function are exported from the package."""
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fvdb_bq_" + n for n in (
    "encode encode_dev index_create index_destroy index_add index_set_deleted index_rows index_live index_bytes index_info "
    "index_search index_search_dev_slot").split()]


def test_bq_entry_points_declared_exported_bound():
    fv = fvdb_import.load()
    lib = fv._capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fvdb_bq_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(NAMES)
    for n in NAMES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert hasattr(lib, n), f"{n} is not exported"
        assert len(fv._capi.SIGNATURES[n][1]) == len([a for a in args.split(",") if a.strip() not in ("", "void")]), n


def test_bq_classes_exported():
    fv = fvdb_import.load()
    assert callable(fv.binary_quantize)
    for name in "add mark_deleted search rows live bytes info close".split():
        assert callable(getattr(fv.BQIndex, name))
