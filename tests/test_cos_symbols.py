"""No GPU: the cosine-search entry points (include/fvdb.h) are declared, exported and bound with
equal arity, and the class and batch_normalize are exported from the package."""
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fvdb_batch_normalize", "fvdb_batch_normalize_dev"] + ["fvdb_cos_index_" + n for n in (
    "create destroy add set_deleted rows live bytes info search search_dev_slot").split()]


def test_cos_entry_points_declared_exported_bound():
    fv = fvdb_import.load()
    lib = fv._capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fvdb_cos_[a-z0-9_]+|fvdb_batch_normalize[a-z_]*)\s*\(", text)))
    assert declared == sorted(NAMES)
    for n in NAMES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert hasattr(lib, n), f"{n} is not exported"
        assert len(fv._capi.SIGNATURES[n][1]) == len([a for a in args.split(",") if a.strip() not in ("", "void")]), n


def test_cos_classes_exported():
    fv = fvdb_import.load()
    assert callable(fv.batch_normalize)
    for name in "add mark_deleted search rows live bytes info close".split():
        assert callable(getattr(fv.CosineIndex, name))
