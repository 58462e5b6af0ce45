"""No GPU needed: the re-partitioning entry points are declared, exported and bound at every layer."""
import fvdb_import


def test_host_signatures_carry_the_repartitioning_entries():
    fv = fvdb_import.load()
    host = fv.load_host()
    for name in ("fvh_ivf_retrain", "fvh_ivf_add_clusters", "fvh_ivf_optimize_clusters", "fvh_ivf_cluster_stats",
                 "fvh_hybrid_retrain_historical"):
        assert name in fv.index.HOST_SIGNATURES and hasattr(host, name)


def test_c_abi_carries_the_resident_maintenance_entries():
    fv = fvdb_import.load()
    lib = fv._capi.load()
    for name in ("fvdb_ivf_compact", "fvdb_ivf_train_from", "fvdb_ivf_assign_from", "fvdb_ivf_refill_from",
                 "fvdb_ivf_maintenance_info"):
        assert name in fv._capi.SIGNATURES and hasattr(lib, name)
    for cls, method in ((fv.IVFIndex, "retrain"), (fv.IVFIndex, "add_clusters"), (fv.IVFIndex, "optimize_clusters"),
                        (fv.IVFIndex, "get_cluster_stats"), (fv.HybridIndex, "retrain_historical"),
                        (fv.DeviceIVF, "compact"), (fv.DeviceIVF, "refill_from")):
        assert callable(getattr(cls, method))
