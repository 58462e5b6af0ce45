"""No GPU: the residual IVF-PQ surface (include/fvdb.h, "IVF over residual PQ codes") is declared,
exported and bound with equal arity, IVFPQIndex takes `residual`, and ivf_residuals is exported."""
import inspect
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ivfrpq_create_declared_exported_bound():
    fv = fvdb_import.load()
    lib = fv._capi.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    assert re.findall(r"\b(fvdb_ivfrpq_[a-z0-9_]+)\s*\(", text) == ["fvdb_ivfrpq_create"]
    args = re.search(r"\bfvdb_ivfrpq_create\s*\(([^)]*)\)", text).group(1)
    assert hasattr(lib, "fvdb_ivfrpq_create")
    assert len(fv._capi.SIGNATURES["fvdb_ivfrpq_create"][1]) == len(args.split(",")) == 4


def test_python_surface():
    fv = fvdb_import.load()
    p = inspect.signature(fv.IVFPQIndex.__init__).parameters
    assert list(p) == ["self", "ctx", "pq", "nlist", "refine_rows", "residual"] and p["residual"].default is False
    assert callable(fv.ivf_residuals) and fv.ivf_residuals is fv.engine.ivf_residuals
