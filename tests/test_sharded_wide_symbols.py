"""The sharded search at any k and nprobe and under an allow-set: its entry points are declared,
exported and bound.  No GPU needed."""
import inspect
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = {"fvdb_ivf_search_shard_wide_dev_slot": 13, "fvdb_merge_keys_wide_dev": 9, "fvdb_ivf_search_sharded_wide_begin": 12}


def test_engine_symbols_are_declared_exported_and_bound():
    fv = fvdb_import.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    lib = fv._capi.load()
    for name, nargs in ENGINE.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/fvdb.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in fv._capi.SIGNATURES and len(fv._capi.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported by the engine"
    # the entry points whose limits stay are still there, with the arguments they had
    assert len(fv._capi.SIGNATURES["fvdb_ivf_search_sharded_begin"][1]) == 11
    assert len(fv._capi.SIGNATURES["fvdb_merge_keys_dev"][1]) == 9


def test_host_mirror_and_python_surface():
    fv = fvdb_import.load()
    host = fv.load_host()
    assert "fvh_hybrid_search_allowed_sharded_begin" in fv.index.HOST_SIGNATURES
    assert len(fv.index.HOST_SIGNATURES["fvh_hybrid_search_allowed_sharded_begin"][1]) == 16
    assert hasattr(host, "fvh_hybrid_search_allowed_sharded_begin")
    assert callable(fv.DeviceIVF.search_shard_wide_dev) and callable(fv.engine.merge_keys_wide_dev)
    assert callable(fv.HybridIndex.search_allowed_sharded_begin)
    for fn in (fv.sharded.ShardedHybrid.search_dev_begin, fv.sharded.ShardedHybrid.search_dev):
        p = inspect.signature(fn).parameters
        assert "allowed" in p and p["allowed"].default is None
