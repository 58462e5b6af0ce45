"""Python surface of the host mirror (lib/libfvdb_host.so): IVFIndex, HNSWIndex, HybridIndex.

Names, argument meaning and error behaviour follow the reference (src/ivf/core.rs,
src/hnsw/core.rs, src/hybrid/core.rs); vector ids are u64 row ids (the 32-byte BLAKE3
VectorId of src/core/types.rs:9-22 is a host-side mapping outside the hot path).  All
search entry points take a BATCH of queries: the reference's per-query loop
(src/ivf/operations.rs:132-145) is what the GPU batch replaces.
"""
import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import f32p, u32p, u64p
from .engine import (STATUS_TO_EXC, DimensionMismatch, FvdbError, InconsistentDimensions,
                     InsufficientTrainingData, InvalidConfig, Unsupported, _f32, _ptr, row_dtype_code)

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_capi.LIB_DIR, "libfvdb_host.so")
_host = None
i64p = C.POINTER(C.c_int64)
f64p = C.POINTER(C.c_double)
u8p = C.POINTER(C.c_uint8)
vp, u64, u32, i32, i64, dbl, f32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_int64, C.c_double, C.c_float

HOST_SIGNATURES = {
    "fvh_ivf_new": (vp, [vp, u32, u32, u32, u32, u64]),
    "fvh_ivf_free": (None, [vp]),
    "fvh_ivf_train": (i32, [vp, f32p, u64, u32, C.POINTER(_capi.TrainResult)]),
    "fvh_ivf_set_trained": (i32, [vp, f32p, u32]),
    "fvh_ivf_get_centroids": (i32, [vp, f32p]),
    "fvh_ivf_is_trained": (i32, [vp]),
    "fvh_ivf_dimension": (u32, [vp]),
    "fvh_ivf_total_vectors": (u64, [vp]),
    "fvh_ivf_active_count": (u64, [vp]),
    "fvh_ivf_cluster_size": (u64, [vp, u32]),
    "fvh_ivf_export_list": (i32, [vp, u32, f32p, u64p, C.POINTER(C.c_uint8)]),
    "fvh_ivf_insert": (i32, [vp, u64, f32p, u32]),
    "fvh_ivf_batch_insert": (i32, [vp, u64p, f32p, u64, u32, u64p, C.POINTER(i32)]),
    "fvh_ivf_find_cluster": (i32, [vp, f32p, u32, u32p]),
    "fvh_ivf_search": (i32, [vp, f32p, u32, u32, u32, u32, u64p, f32p, u32p]),
    "fvh_ivf_mark_deleted": (i32, [vp, u64]),
    "fvh_ivf_is_deleted": (i32, [vp, u64]),
    "fvh_ivf_device": (vp, [vp]),
    "fvh_ivf_retrain": (i32, [vp, u32, u32, u32, u32, u64, u64p]),
    "fvh_ivf_add_clusters": (i32, [vp, u32, u64p]),
    "fvh_ivf_optimize_clusters": (i32, [vp, u32p, f32p]),
    "fvh_ivf_cluster_stats": (i32, [vp, vp]),
    "fvh_ivf_n_clusters": (u32, [vp]),
    "fvh_ivf_n_probe": (u32, [vp]),
    "fvh_hybrid_retrain_historical": (i32, [vp, u32, u32, u32, u32, u64, u64p]),
    "fvh_hnsw_new": (vp, [vp, u32, u32, u32, u64]),
    "fvh_hnsw_free": (None, [vp]),
    "fvh_hnsw_insert": (i32, [vp, u64, f32p, u32, i64]),
    "fvh_hnsw_batch_insert": (i32, [vp, u64p, f32p, u64, u32, i64p, u64p, C.POINTER(i32)]),
    "fvh_hnsw_search": (i32, [vp, f32p, u32, u32, u32, u32, u64p, f32p, u32p]),
    "fvh_hnsw_node_count": (u64, [vp]),
    "fvh_hnsw_active_count": (u64, [vp]),
    "fvh_hnsw_entry_point": (i32, [vp, u64p]),
    "fvh_hnsw_level": (i64, [vp, u64]),
    "fvh_hnsw_neighbors": (i64, [vp, u64, u32, u64p, u64]),
    "fvh_hnsw_mark_deleted": (i32, [vp, u64]),
    "fvh_hnsw_is_deleted": (i32, [vp, u64]),
    "fvh_hnsw_bulk_build": (i32, [vp, u64p, f32p, u64, u32, i64p]),
    "fvh_hnsw_restore": (i32, [vp, u64p, f32p, u64, u32, u32p, u64p, u64p, u64]),
    "fvh_hnsw_graph_slots": (u64, [vp]),
    "fvh_hnsw_graph_edges": (u64, [vp]),
    "fvh_hnsw_export_graph": (None, [vp, u64p, u32p, u64p, u64p]),
    "fvh_hnsw_get_vector": (i32, [vp, u64, f32p]),
    "fvh_hnsw_dist_evals": (u64, [vp]),
    "fvh_hnsw_hops": (u64, [vp]),
    "fvh_hnsw_set_threads": (None, [vp, i32]),
    "fvh_hnsw_dimension": (u32, [vp]),
    "fvh_hnsw_set_device_traversal": (None, [vp, i32]),
    "fvh_hnsw_set_device_insert": (None, [vp, i32, i32]),
    "fvh_hnsw_device_insert": (i32, [vp]),
    "fvh_hnsw_insert_stats": (None, [vp, vp, u64p, u64p]),
    "fvh_hnsw_set_insert_visited": (i32, [vp, i32, u32]),
    "fvh_hnsw_insert_info": (i32, [vp, vp]),
    "fvh_hnsw_device_traversal": (i32, [vp]),
    "fvh_hnsw_device_fallbacks": (u64, [vp]),
    "fvh_hnsw_graph_kernel_times": (i32, [vp, f32p, u32p, u64p, u64p]),
    "fvh_hnsw_tie_restarts": (i32, [vp, u64p, u64p]),
    "fvh_hybrid_new": (vp, [vp, vp, dbl, u64, i32, u64, u32, u32, u32, u64, u32, u32, u32, u32, u64]),
    "fvh_hybrid_free": (None, [vp]),
    "fvh_hybrid_initialize": (i32, [vp, f32p, u64, u32]),
    "fvh_hybrid_set_ivf_centroids": (i32, [vp, f32p, u32]),
    "fvh_hybrid_insert": (i32, [vp, u64, f32p, u32, dbl, dbl, i64]),
    "fvh_hybrid_bulk_insert": (i32, [vp, u64p, f32p, u64, u32, f64p, dbl]),
    "fvh_hybrid_bulk_insert_sharded": (i32, [vp, u64p, f32p, u64, u32, f64p, dbl, u32, u32, u32p]),
    "fvh_hybrid_search": (i32, [vp, f32p, u32, u32, u64, u64, u64, i32, i32, u64, u64, dbl, u64p, f32p, u32p]),
    "fvh_hybrid_search_with_filter": (i32, [vp, f32p, u32, u32, u64, vp, vp, dbl, u64p, f32p, u32p]),
    # filtered search with the allow-set applied on the device
    "fvh_ivf_search_allowed": (i32, [vp, f32p, u32, u32, u32, u32, u64p, u64, u64p, f32p, u32p]),
    "fvh_ivf_mask_builds": (u64, [vp]),
    "fvh_hnsw_search_allowed": (i32, [vp, f32p, u32, u32, u32, u32, u64p, u64, u64p, f32p, u32p]),
    "fvh_hnsw_set_scan_cutoff": (None, [vp, u64]),
    "fvh_hnsw_scan_cutoff": (u64, [vp]),
    "fvh_hnsw_mask_builds": (u64, [vp]),
    "fvh_hnsw_device_graph": (vp, [vp]),
    "fvh_hybrid_search_allowed": (i32, [vp, f32p, u32, u32, u64, u64, u64, i32, i32, u64, u64, u64p, u64, dbl, u64p, f32p,
                                        u32p]),
    "fvh_hybrid_search_dev": (i32, [vp, vp, u32, u32, u64, u64, u64, i32, i32, u64, u64, dbl, u64p, f32p, u32p]),
    "fvh_hybrid_search_dev_begin": (i32, [vp, u32, vp, u32, u32, u64, u64, u64, i32, i32, u64, u64, dbl]),
    "fvh_hybrid_search_dev_end": (i32, [vp, u32, u64p, f32p, u32p]),
    "fvh_hybrid_attach_comm": (i32, [vp, vp]),
    "fvh_hybrid_search_sharded_begin": (i32, [vp, u32, vp, u32, u32, u64, u64, u64, i32, i32, u64, u64, i32, dbl]),
    "fvh_hybrid_search_allowed_sharded_begin": (i32, [vp, u32, vp, u32, u32, u64, u64, u64, i32, i32, u64, u64, i32, u64p, u64,
                                                      dbl]),
    "fvh_hybrid_search_sharded_end": (i32, [vp, u32, u64p, f32p, u32p]),
    "fvh_hybrid_sharded_rows": (u32, [vp, u32, i32]),
    "fvh_plan_list_owners": (None, [u64p, u32, u32, u32p]),
    "fvh_merge_parts": (None, [u32, u32, u32, u32, u64p, f32p, u32p, u64p, f32p, u32p, u64p, f32p, u32p]),
    "fvh_hnsw_search_dev": (i32, [vp, vp, u32, u32, u32, u32, u64p, f32p, u32p]),
    "fvh_hnsw_search_dev_begin": (i32, [vp, u32, vp, u32, u32, u32, u32]),
    "fvh_hnsw_search_dev_end": (i32, [vp, u32, vp, u32, u32, u32, u32, u64p, f32p, u32p]),
    "fvh_hybrid_delete": (i32, [vp, u64, dbl]),
    "fvh_hybrid_migrate": (u64, [vp, dbl, dbl]),
    "fvh_hybrid_vacuum": (i32, [vp, u64p, u64p]),
    "fvh_ivf_vacuum": (i32, [vp, u64p]),
    "fvh_hnsw_vacuum": (u64, [vp]),
    # resident vacuum
    "fvh_hnsw_vacuum_ex": (i32, [vp, u64p]),
    "fvh_hnsw_set_resident_vacuum": (None, [vp, i32]),
    "fvh_hnsw_resident_vacuum": (i32, [vp]),
    "fvh_hnsw_set_vacuum_keep_rows": (None, [vp, i32]),
    "fvh_hnsw_vacuum_info": (i32, [vp, vp]),
    "fvh_hnsw_store_rows": (u64, [vp]),
    "fvh_hybrid_from_parts": (i32, [vp, u64p, f64p, u64, u64, u64, i32]),
    "fvh_hybrid_timestamp_count": (u64, [vp]),
    "fvh_hybrid_export_timestamps": (None, [vp, u64p, f64p]),
    "fvh_hybrid_recent_count": (u64, [vp]),
    "fvh_hybrid_historical_count": (u64, [vp]),
    "fvh_hybrid_is_initialized": (i32, [vp]),
    "fvh_hybrid_is_ivf_trained": (i32, [vp]),
    "fvh_hybrid_hnsw": (vp, [vp]),
    "fvh_hybrid_set_sequential_graph": (None, [vp, i32]),
    "fvh_hybrid_sequential_graph": (i32, [vp]),
    "fvh_hybrid_recent_build_seconds": (dbl, [vp]),
    "fvh_hybrid_set_blocking_writers": (None, [vp, i32]),
    "fvh_hybrid_blocking_writers": (i32, [vp]),
    "fvh_hybrid_ivf": (vp, [vp]),
    # rows by id and resident migration
    "fvh_ivf_get_vectors": (i32, [vp, u64p, u64, f32p, C.POINTER(C.c_uint8)]),
    "fvh_hybrid_get_vectors": (i32, [vp, u64p, u64, f32p, C.POINTER(C.c_uint8)]),
    "fvh_hybrid_set_resident_migration": (None, [vp, i32]),
    "fvh_hybrid_migration_info": (i32, [vp, vp]),
    # recall self-evaluation at any n_probe
    "fvh_ivf_evaluate_search_quality": (i32, [vp, f32p, u32, u32, u32, f32p, u64p]),
    # recall and precision at every n_probe from one search of every list
    "fvh_ivf_quality_curve": (i32, [vp, f32p, u32, u32, u32, i32, u64p, u64, u32, f32p, f32p, f32p, u64p]),
    # half-precision rows: the constructors with a row_dtype, the doors' rounding routine
    "fvh_ivf_new_ex": (vp, [vp, u32, u32, u32, u32, u64, i32]),
    "fvh_hnsw_new_ex": (vp, [vp, u32, u32, u32, u64, i32]),
    "fvh_hybrid_new_ex": (vp, [vp, vp, dbl, u64, i32, u64, u32, u32, u32, u64, u32, u32, u32, u32, u64, i32]),
    "fvh_ivf_row_dtype": (i32, [vp]),
    "fvh_hnsw_row_dtype": (i32, [vp]),
    "fvh_hnsw_store_bytes": (u64, [vp]),
    "fvh_round_f16": (None, [f32p, u64, f32p]),
    # exact search and search quality
    "fvh_hnsw_search_exact": (i32, [vp, f32p, u32, u32, u32, u64p, f32p, u32p]),
    "fvh_hnsw_search_exact_allowed": (i32, [vp, f32p, u32, u32, u32, u64p, u64, u64p, f32p, u32p]),
    "fvh_hnsw_evaluate_search_quality": (i32, [vp, f32p, u32, u32, u32, u32, f32p, u64p]),
    "fvh_hybrid_search_exact": (i32, [vp, f32p, u32, u32, u64, i32, i32, dbl, u64p, f32p, u32p]),
    "fvh_hybrid_evaluate_search_quality": (i32, [vp, f32p, u32, u32, u64, u64, u64, dbl, f32p, u64p]),
    # the same at k up to 4096
    "fvh_hnsw_search_exact_wide": (i32, [vp, f32p, u32, u32, u32, u64p, f32p, u32p]),
    "fvh_hnsw_search_exact_wide_allowed": (i32, [vp, f32p, u32, u32, u32, u64p, u64, u64p, f32p, u32p]),
    "fvh_hnsw_evaluate_search_quality_wide": (i32, [vp, f32p, u32, u32, u32, u32, f32p, u64p]),
    "fvh_hybrid_search_exact_wide": (i32, [vp, f32p, u32, u32, u64, i32, i32, dbl, u64p, f32p, u32p]),
    "fvh_hybrid_evaluate_search_quality_wide": (i32, [vp, f32p, u32, u32, u64, u64, u64, dbl, f32p, u64p]),
    # radius search
    "fvh_hnsw_search_radius": (i32, [vp, f32p, u32, u32, f32p, u32, u64p, f32p, u32p, u32p]),
    "fvh_hnsw_search_radius_allowed": (i32, [vp, f32p, u32, u32, f32p, u32, u64p, u64, u64p, f32p, u32p, u32p]),
    "fvh_hnsw_count_within": (i32, [vp, f32p, u32, u32, f32p, u64p, u64, u32p]),
    "fvh_ivf_search_radius": (i32, [vp, f32p, u32, u32, f32p, u32, u32, u64p, u64, u64p, f32p, u32p, u32p]),
    "fvh_hybrid_search_radius": (i32, [vp, f32p, u32, u32, f32p, u64, u64, i32, i32, u64p, u64, dbl, u64p, f32p, u32p, u32p]),
    # diverse search
    "fvh_set_diverse_stage_bytes": (None, [u64]),
    "fvh_diverse_stage_bytes": (u64, []),
    "fvh_ivf_search_diverse": (i32, [vp, f32p, u32, u32, u32, u32, f32, i32, u32, u64p, u64, u64p, f32p, u32p, u32p]),
    "fvh_hnsw_search_diverse": (i32, [vp, f32p, u32, u32, u32, u32, f32, i32, u32, u64p, u64, u64p, f32p, u32p, u32p]),
    "fvh_hybrid_search_diverse": (i32, [vp, f32p, u32, u32, u64, u32, f32, i32, u64, u64, i32, i32, u64p, u64, dbl, u64p, f32p, u32p,
                                        u32p]),
    "fvh_hybrid_search_diverse_groups": (i32, [vp, f32p, u32, u32, u64, u32, f32, i32, u64, u64, i32, i32, u64p, u64p, u8p, u32, u32p,
                                               dbl, u64p, f32p, u32p, u32p]),
    # grouped search: index, its context, the metadata table, the column, ...
    "fvh_ivf_search_grouped": (i32, [vp, vp, vp, u32, f32p, u32, u32, u32, u32, u32, i32, i32, u32, u64p, u64, u64p, f32p, u32p,
                                     u32p, u32p, u8p, u64p, u32p, u32p]),
    "fvh_hnsw_search_grouped": (i32, [vp, vp, vp, u32, f32p, u32, u32, u32, u32, u32, i32, i32, u32, u64p, u64, u64p, f32p, u32p,
                                      u32p, u32p, u8p, u64p, u32p, u32p]),
    "fvh_hybrid_search_grouped": (i32, [vp, vp, vp, u32, f32p, u32, u32, u64, u32, u32, i32, i32, u64, u64, i32, i32, u64p, u64,
                                        dbl, u64p, f32p, u32p, u32p, u32p, u8p, u64p, u32p, u32p]),
    # search quality over a grid of ef and n_probe from one exact search
    "fvh_hnsw_quality_by_ef": (i32, [vp, f32p, u32, u32, u32, u32p, u32, f32p, f32p, f32p, u64p]),
    "fvh_hybrid_quality_grid": (i32, [vp, f32p, u32, u32, u64, i32, i32, u64, u64, u32p, u32, u32p, u32, dbl, f32p, f32p, f32p,
                                      u64p]),
    # one allow-set per query
    "fvh_ivf_search_allowed_groups": (i32, [vp, f32p, u32, u32, u32, u32, u64p, u64p, u8p, u32, u32p, u64p, f32p, u32p]),
    "fvh_hnsw_search_allowed_groups": (i32, [vp, f32p, u32, u32, u32, u32, u64p, u64p, u8p, u32, u32p, u64p, f32p, u32p]),
    "fvh_hybrid_search_allowed_groups": (i32, [vp, f32p, u32, u32, u64, u64, u64, i32, i32, u64p, u64p, u8p, u32, u32p, dbl, u64p,
                                               f32p, u32p]),
    # graph stats and health
    "fvh_hnsw_graph_stats": (i32, [vp, u64p]),
    "fvh_hnsw_max_level": (u32, [vp]),
    "fvh_hnsw_level_distribution": (None, [vp, u64p]),
    "fvh_hnsw_graph_health": (i32, [vp, u32, C.POINTER(_capi.GraphHealth), C.POINTER(C.c_int)]),
    "fvh_hnsw_unreachable": (i32, [vp, u64p, u64, u64p]),
    "fvh_hnsw_component_labels": (i32, [vp, u64p]),
}

_ROW_DTYPE_NAMES = ("f32", "f16")


def load_host():
    global _host
    if _host is not None:
        return _host
    _capi.load()  # the engine first: the host mirror links against it
    if not os.path.exists(HOST_LIB_PATH):
        raise ImportError(f"{HOST_LIB_PATH} not found: build it with `make -C fabstir-vectordb_amd`")
    lib = C.CDLL(HOST_LIB_PATH)
    for name, (res, args) in HOST_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _host = lib
    return lib


class SearchResults:
    """B x k ids / distances with per-query hit counts (Vec<Vec<SearchResult>> in the reference)."""

    def __init__(self, ids, distances, counts):
        self.ids, self.distances, self.counts = ids, distances, counts

    def __len__(self):
        return self.ids.shape[0]

    def __getitem__(self, b):
        n = int(self.counts[b])
        return self.ids[b, :n], self.distances[b, :n]

    def scores(self):
        """Node/REST surface score = 1/(1+distance) in f32 (bindings/node/src/session.rs:291, src/api/rest.rs:653)."""
        return (np.float32(1.0) / (np.float32(1.0) + self.distances)).astype(np.float32)


GROUP_MISSING = {"drop": 0, "own": 1}  # FVDB_GROUP_MISSING_*


class GroupedResults:
    """What search_grouped returns, as fvdb_group_select_dev lays it out: ids / distances / ranks
    [B][k][group_size] (tails FVDB_NO_ID / +inf / FVDB_NO_ROW), members / totals / key_tags / key_words [B][k], groups and
    flags [B].  result[b] lists query b's groups as (key tag, key word, ids, distances, ranks, total) in group order."""

    def __init__(self, ids, distances, ranks, members, totals, key_tags, key_words, groups, flags, k, group_size):
        self.ids, self.distances, self.ranks, self.members, self.totals = ids, distances, ranks, members, totals
        self.key_tags, self.key_words, self.groups, self.flags = key_tags, key_words, groups, flags
        self.k, self.group_size = k, group_size

    def __len__(self):
        return self.groups.shape[0]

    def __getitem__(self, b):
        out = []
        for g in range(int(self.groups[b])):
            m = int(self.members[b, g])
            out.append((int(self.key_tags[b, g]), int(self.key_words[b, g]), self.ids[b, g, :m], self.distances[b, g, :m],
                        self.ranks[b, g, :m], int(self.totals[b, g])))
        return out

    def cut(self, b):
        """True when query b's candidate list was full (flag bit 0): a nearer-than-returned row cannot be missing, but
        rows beyond the fetch_k-th were not seen."""
        return bool(int(self.flags[b]) & 1)

    def groups_complete(self, b):
        """The set of groups of query b is exact with respect to the underlying search: k groups were found, or the
        candidate list was not cut."""
        return int(self.groups[b]) == self.k or not self.cut(b)

    def group_complete(self, b, g):
        """Group g of query b holds its best members: it is full, or the candidate list was not cut."""
        return int(self.members[b, g]) == self.group_size or not self.cut(b)


def set_diverse_stage_bytes(nbytes):
    """The cap of search_diverse's staging block of candidate rows in HBM, for the process (default
    256 MiB, or FVDB_DIVERSE_STAGE_BYTES read once): a batch is walked in sub-batches of the queries that fit, at least one.
    0 restores the default.  The results do not depend on it.  Returns the cap now in force."""
    lib = load_host()
    lib.fvh_set_diverse_stage_bytes(int(nbytes))
    return int(lib.fvh_diverse_stage_bytes())


def round_f16(x):
    """The rounding an index with row_dtype="f16" applies at its door: f32 -> IEEE fp16 (nearest, ties to even) -> f32,
    by the host mirror's own routine."""
    x = _f32(x)
    out = np.empty_like(x)
    load_host().fvh_round_f16(_ptr(x, f32p), x.size, _ptr(out, f32p))
    return out


def _rows(x, dim=None):
    x = _f32(x)
    if x.ndim == 1:
        x = x.reshape(1, -1)
    if dim is not None and x.shape[1] != dim:
        raise DimensionMismatch(f"Dimension mismatch: expected {dim}, got {x.shape[1]}")
    return x


def _allowed_ids(allowed):
    """An allow-set as a contiguous 1-d u64 array; an empty one is a zero-length view of a real buffer, so that
    ctypes has an address to pass."""
    a = np.ascontiguousarray(np.fromiter(allowed, np.uint64) if not isinstance(allowed, np.ndarray) else allowed, np.uint64)
    return a.reshape(-1) if a.size else np.zeros(1, np.uint64)[:0]


def _allowed_args(allowed):
    """(pointer, count, array) of an optional allow-set: a null pointer for None ("no filter")."""
    if allowed is None:
        return None, 0, None
    a = _allowed_ids(allowed)
    return _ptr(a, u64p), a.size, a


def _radii(radius, B):
    """The radii of a radius search as f32[B]: one value for every query, or one per query."""
    r = np.asarray(radius, np.float32).reshape(-1)
    if r.size == 1:
        r = np.full(B, r[0], np.float32)
    if r.size != B:
        raise InvalidConfig(f"radius has {r.size} entries for {B} queries")
    return np.ascontiguousarray(r) if B else np.zeros(1, np.float32)[:0]


def _allow_groups(allow_sets, group_of_query, B):
    """The ctypes arguments of a grouped search: the allow-sets laid end to end with their offsets, a flag per set (0 where
    the entry is None: "no filter") and the group of each query.  The arrays are returned too: the caller keeps them
    alive for the call."""
    sets = [None if a is None else _allowed_ids(a) for a in allow_sets]
    off = np.zeros(len(sets) + 1, np.uint64)
    off[1:] = np.cumsum([0 if a is None else a.size for a in sets], dtype=np.uint64)
    flat = np.zeros(max(int(off[-1]), 1), np.uint64)
    for g, a in enumerate(sets):
        if a is not None:
            flat[int(off[g]):int(off[g + 1])] = a
    filtered = np.zeros(max(len(sets), 1), np.uint8)
    filtered[:len(sets)] = [a is not None for a in sets]
    group = np.asarray(group_of_query).reshape(-1)
    if group.size != B:
        raise InvalidConfig(f"group_of_query has {group.size} entries for {B} queries")
    if group.size and (group.min() < 0 or group.max() >= len(sets)):
        raise InvalidConfig(f"group_of_query names a group outside allow_sets (0..{len(sets) - 1})")
    group = np.zeros(1, np.uint32)[:0] if not group.size else np.ascontiguousarray(group, np.uint32)
    keep = (flat, off, filtered, group)
    return (_ptr(flat, u64p), _ptr(off, u64p), filtered.ctypes.data_as(u8p), len(sets), _ptr(group, u32p)), keep


def _get_vectors(self, fn, ids, dim):
    """(rows [n x dim] f32, found [n] bool) for `ids`; a row that was not found is zero."""
    ids = np.ascontiguousarray(np.atleast_1d(ids), np.uint64).reshape(-1)
    out = np.zeros((ids.size, max(int(dim or 0), 1)), np.float32)
    found = np.zeros(max(ids.size, 1), np.uint8)
    if ids.size:
        self._check(fn(self.h, _ptr(ids, u64p), ids.size, _ptr(out, f32p), found.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out, found[:ids.size].astype(bool)


class _Base:
    def _check(self, rc):
        if rc:
            msg = self.ctx.lib.fvdb_last_error(self.ctx.h)
            exc = STATUS_TO_EXC.get(rc, FvdbError)((msg.decode() if msg else "") or f"status {rc}")
            exc.status = rc
            raise exc

    def _search(self, fn, q, k, *mid):
        q = _rows(q)
        B = q.shape[0]
        ids = np.empty((B, max(k, 1)), np.uint64)
        ds = np.empty((B, max(k, 1)), np.float32)
        cnt = np.zeros(B, np.uint32)
        self._check(fn(self.h, _ptr(q, f32p), B, q.shape[1], k, *mid, _ptr(ids, u64p), _ptr(ds, f32p), _ptr(cnt, u32p)))
        return SearchResults(ids, ds, cnt)

    def _search_radius(self, fn, q, radius, max_results, *mid):
        """The radius searches: (SearchResults of [B][max_results], totals uint32[B])."""
        q = _rows(q)
        B, m = q.shape[0], int(max_results)
        r = _radii(radius, B)
        ids = np.empty((B, max(m, 1)), np.uint64)
        ds = np.empty((B, max(m, 1)), np.float32)
        cnt, totals = np.zeros(B, np.uint32), np.zeros(B, np.uint32)
        self._check(fn(self.h, _ptr(q, f32p), B, q.shape[1], _ptr(r, f32p), m, *mid, _ptr(ids, u64p), _ptr(ds, f32p),
                       _ptr(cnt, u32p), _ptr(totals, u32p)))
        return SearchResults(ids, ds, cnt), totals

    def _search_diverse(self, fn, q, k, fetch_k, lam, distinct, *mid):
        """The diverse searches: (SearchResults of [B][k] in pick order, ranks uint32[B][k])."""
        q = _rows(q)
        B, k, fetch_k, lam = q.shape[0], int(k), int(fetch_k), float(lam)
        if not (k >= 0 and 0 <= fetch_k <= 0xFFFFFFFF):
            raise InvalidConfig("Invalid parameter: k and fetch_k are unsigned")
        ids = np.full((B, max(k, 1)), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
        ds = np.full((B, max(k, 1)), np.inf, np.float32)
        ranks = np.full((B, max(k, 1)), 0xFFFFFFFF, np.uint32)
        cnt = np.zeros(B, np.uint32)
        self._check(fn(self.h, _ptr(q, f32p), B, q.shape[1], k, fetch_k, lam, int(bool(distinct)), *mid, _ptr(ids, u64p),
                       _ptr(ds, f32p), _ptr(ranks, u32p), _ptr(cnt, u32p)))
        return SearchResults(ids, ds, cnt), ranks

    def _search_grouped(self, fn, q, k, group_size, fetch_k, columns, path, distinct, missing, metadata, *mid):
        """The grouped searches: GroupedResults.  `columns` is a MetadataColumns; the column of
        `path` is built on first use, as a "resident" filter builds it, from `metadata` (None: the map of the columns'
        last sync_rows) — after the limits have been checked, so a call that is refused builds nothing."""
        q = _rows(q)
        B, k, gs, fetch_k = q.shape[0], int(k), int(group_size), int(fetch_k)
        if missing not in GROUP_MISSING:
            raise InvalidConfig(f'Invalid parameter: missing must be "drop" or "own", got {missing!r}')
        if not (0 <= k <= 0xFFFFFFFF and 0 <= gs <= 0xFFFFFFFF and 0 <= fetch_k <= 0xFFFFFFFF):
            raise InvalidConfig("Invalid parameter: k, group_size and fetch_k are unsigned")
        if fetch_k == 0 or fetch_k > 4096 or k * gs > 4096:  # the engine's refusals, in its order (check_grouped)
            raise Unsupported("search_grouped: fetch_k must be in 1..4096 and k * group_size at most 4096")
        if k == 0 or gs == 0:
            raise InvalidConfig("Invalid parameter: k and group_size must be at least 1")
        column = columns.group_column(path, metadata)
        kk, gg = k, gs
        ids = np.full((B, kk, gg), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
        ds = np.full((B, kk, gg), np.inf, np.float32)
        ranks = np.full((B, kk, gg), 0xFFFFFFFF, np.uint32)
        members, totals = np.zeros((B, kk), np.uint32), np.zeros((B, kk), np.uint32)
        tags, words = np.zeros((B, kk), np.uint8), np.zeros((B, kk), np.uint64)
        groups, flags = np.zeros(B, np.uint32), np.zeros(B, np.uint32)
        table = columns.table
        self._check(fn(self.h, self.ctx.h, table.h, column, _ptr(q, f32p), B, q.shape[1], k, gs, fetch_k,
                       int(bool(distinct)), GROUP_MISSING[missing], *mid, _ptr(ids, u64p), _ptr(ds, f32p), _ptr(ranks, u32p),
                       _ptr(members, u32p), _ptr(totals, u32p), tags.ctypes.data_as(u8p), _ptr(words, u64p), _ptr(groups, u32p),
                       _ptr(flags, u32p)))
        return GroupedResults(ids, ds, ranks, members, totals, tags, words, groups, flags, k, gs)

    def _quality(self, fn, queries, *args):
        """evaluate_search_quality of the graph and hybrid classes: SearchQuality as a dict, as IVFIndex returns it."""
        q = np.asarray(queries, np.float32)
        if q.size == 0:
            raise InvalidConfig("Invalid parameter: No test queries provided")
        q = _rows(q)
        out, n = np.zeros(3, np.float32), C.c_uint64(0)
        self._check(fn(self.h, _ptr(q, f32p), q.shape[0], q.shape[1], *args, _ptr(out, f32p), C.byref(n)))
        return dict(avg_recall=out[0], avg_precision=out[1], avg_query_time_ms=float(out[2]), queries_evaluated=int(n.value))

    def _grid(self, call, queries, efs, n_probes):
        """The grid calls of the graph and hybrid classes: call(q, B, dim, efs, E, n_probes, P, recall,
        precision, ms, done) fills [max(E, 1)][max(P, 1)] f32 arrays."""
        q = np.asarray(queries, np.float32)
        if q.size == 0:
            raise InvalidConfig("Invalid parameter: No test queries provided")
        q = _rows(q)
        e, p = _points(efs), _points(n_probes)
        shape = (max(e.size, 1), max(p.size, 1))
        recall, precision = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        ms, done = C.c_float(0), C.c_uint64(0)
        self._check(call(_ptr(q, f32p), q.shape[0], q.shape[1], _ptr(e, u32p) if e.size else None, e.size,
                         _ptr(p, u32p) if p.size else None, p.size, _ptr(recall, f32p), _ptr(precision, f32p), C.byref(ms),
                         C.byref(done)))
        return recall, precision, float(ms.value), int(done.value), e, p


def pareto_points(grid, target_recall):
    """HybridIndex.operating_points on a grid as quality_grid returns it: the (ef, n_probe) pairs whose avg_recall reaches
    target_recall (compared in f32) and that no other reaching pair dominates (ef' <= ef and n_probe' <= n_probe), as
    dicts sorted by ef.  A pair listed twice is reported once."""
    reach = {}
    for i, ef in enumerate(grid["efs"]):
        for j, p in enumerate(grid["n_probes"]):
            if grid["avg_recall"][i][j] >= np.float32(target_recall):
                reach.setdefault((int(ef), int(p)), (grid["avg_recall"][i][j], grid["avg_precision"][i][j]))
    keep = [pt for pt in reach if not any(o != pt and o[0] <= pt[0] and o[1] <= pt[1] for o in reach)]
    return [dict(ef=ef, n_probe=p, avg_recall=reach[(ef, p)][0], avg_precision=reach[(ef, p)][1]) for ef, p in sorted(keep)]


def _points(values):
    """The listed ef or n_probe values of a grid call as a u32 array (None: no value)."""
    v = np.asarray([] if values is None else values, np.int64).reshape(-1)
    if v.size and (v.min() < 0 or v.max() > 0xFFFFFFFF):
        raise InvalidConfig("Invalid parameter: ef and n_probe values are 32-bit unsigned")
    return np.ascontiguousarray(v, np.uint32)


class IVFIndex(_Base):
    """src/ivf/core.rs IVFIndex (IVFConfig::default :50-60)."""

    def __init__(self, ctx, n_clusters=256, n_probe=16, train_size=10000, max_iterations=25, seed=0, row_dtype="f32",
                 _handle=None):
        """row_dtype "f16": the lists keep their rows as IEEE fp16.  Every inserted row is rounded once (nearest even) and
        the index is the reference algorithm on the rounded rows; training data, centroids and queries stay f32."""
        self.ctx, self.lib = ctx, load_host()
        self.n_clusters, self.n_probe = n_clusters, n_probe
        self._own = _handle is None
        if _handle is None:
            _handle = self.lib.fvh_ivf_new_ex(ctx.h, n_clusters, n_probe, train_size, max_iterations, seed,
                                              row_dtype_code(row_dtype))
            if not _handle:
                raise InvalidConfig("Invalid IVFConfig")
        self.h = _handle
        self.row_dtype = _ROW_DTYPE_NAMES[self.lib.fvh_ivf_row_dtype(self.h)]

    def __del__(self):
        if getattr(self, "_own", False) and getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.fvh_ivf_free(self.h)
            self.h = None

    def is_trained(self):
        return bool(self.lib.fvh_ivf_is_trained(self.h))

    def dimension(self):
        return int(self.lib.fvh_ivf_dimension(self.h)) if self.is_trained() else None

    def total_vectors(self):
        return int(self.lib.fvh_ivf_total_vectors(self.h))

    def active_count(self):
        return int(self.lib.fvh_ivf_active_count(self.h))

    def train(self, training_data):
        rows = [np.asarray(r, np.float32) for r in training_data]
        if len(rows) == 0 or len(rows) < self.n_clusters:  # src/ivf/core.rs:242-254
            raise InsufficientTrainingData(f"Insufficient training data: got {len(rows)}, need at least {self.n_clusters}")
        d = rows[0].size
        if any(r.size != d for r in rows):  # :257-265
            raise InconsistentDimensions("Inconsistent dimensions in training data")
        x = _f32(np.stack(rows))
        res = _capi.TrainResult()
        self._check(self.lib.fvh_ivf_train(self.h, _ptr(x, f32p), x.shape[0], d, C.byref(res)))
        return dict(iterations=res.iterations, converged=bool(res.converged), initial_error=res.initial_error,
                    final_error=res.final_error)

    def set_trained(self, centroids):
        c = _rows(centroids)
        if c.shape[0] != self.n_clusters:
            raise InvalidConfig(f"expected {self.n_clusters} centroids")
        self._check(self.lib.fvh_ivf_set_trained(self.h, _ptr(c, f32p), c.shape[1]))

    def get_centroids(self):
        out = np.empty((self.n_clusters, self.dimension()), np.float32)
        self._check(self.lib.fvh_ivf_get_centroids(self.h, _ptr(out, f32p)))
        return out

    def insert(self, id, vector):
        v = _f32(vector).reshape(-1)
        self._check(self.lib.fvh_ivf_insert(self.h, int(id), _ptr(v, f32p), v.size))

    def batch_insert(self, ids, vectors):
        """Returns (successful, failed) like BatchInsertResult (src/ivf/operations.rs:107-130)."""
        v = _rows(vectors)
        ids = np.ascontiguousarray(ids, np.uint64)
        ok, err = C.c_uint64(0), C.c_int(0)
        self._check(self.lib.fvh_ivf_batch_insert(self.h, _ptr(ids, u64p), _ptr(v, f32p), v.shape[0], v.shape[1],
                                                  C.byref(ok), C.byref(err)))
        return ok.value, v.shape[0] - ok.value

    def find_cluster(self, vector):
        v = _f32(vector).reshape(-1)
        out = C.c_uint32(0)
        self._check(self.lib.fvh_ivf_find_cluster(self.h, _ptr(v, f32p), v.size, C.byref(out)))
        return out.value

    def get_cluster_size(self, c):
        return int(self.lib.fvh_ivf_cluster_size(self.h, c))

    def vacuum(self):
        out = C.c_uint64(0)
        self._check(self.lib.fvh_ivf_vacuum(self.h, C.byref(out)))
        return out.value

    # --- re-partitioning (src/ivf/operations.rs:148-288); the rows stay in HBM ---
    def _sync_config(self):
        # the mirror replaces its config before a retrain's training can fail (operations.rs:168-169): read it back
        self._dev_clusters = max(getattr(self, "_dev_clusters", 0), self.n_clusters)  # list_sizes: room for the old lists
        self.n_clusters = int(self.lib.fvh_ivf_n_clusters(self.h))
        self.n_probe = int(self.lib.fvh_ivf_n_probe(self.h))

    def retrain(self, n_clusters, n_probe=None, train_size=10000, max_iterations=25, seed=0):
        """IVFIndex::retrain (operations.rs:148-193) with the new IVFConfig's fields; returns RetrainResult as a dict."""
        out = np.zeros(4, np.uint64)
        rc = self.lib.fvh_ivf_retrain(self.h, int(n_clusters), int(self.n_probe if n_probe is None else n_probe),
                                      int(train_size), int(max_iterations), int(seed), _ptr(out, u64p))
        self._sync_config()
        self._check(rc)
        return dict(old_clusters=int(out[0]), new_clusters=int(out[1]), vectors_reassigned=int(out[2]), converged=bool(out[3]))

    def add_clusters(self, n_clusters_to_add):
        """IVFIndex::add_clusters (operations.rs:195-220)."""
        out = C.c_uint64(0)
        rc = self.lib.fvh_ivf_add_clusters(self.h, int(n_clusters_to_add), C.byref(out))
        self._sync_config()
        if rc == 6 and int(n_clusters_to_add) == 0:
            raise InvalidConfig("Invalid parameter: Cannot add 0 clusters")
        self._check(rc)
        return dict(clusters_added=int(n_clusters_to_add), vectors_reassigned=out.value)

    def optimize_clusters(self):
        """IVFIndex::optimize_clusters (operations.rs:222-260); total_vectors doubles like the reference's."""
        it, imp = C.c_uint32(0), C.c_float(0)
        self._check(self.lib.fvh_ivf_optimize_clusters(self.h, C.byref(it), C.byref(imp)))
        return dict(iterations=it.value, improvement=imp.value)

    def get_cluster_stats(self):
        """ClusterStats (operations.rs:263-288)."""
        st = _ClusterStats()
        self._check(self.lib.fvh_ivf_cluster_stats(self.h, C.byref(st)))
        return dict(n_clusters=st.n_clusters, total_vectors=st.total_vectors, avg_cluster_size=st.avg_cluster_size,
                    size_variance=st.size_variance, empty_clusters=st.empty_clusters)

    def evaluate_search_quality(self, queries, k):
        """IVFIndex::evaluate_search_quality (operations.rs:329-391): the configured n_probe against the search of every
        list, both on the device.  Returns SearchQuality as a dict; avg_query_time_ms is the call's wall time over the
        number of queries."""
        q = np.asarray(queries, np.float32)
        if q.size == 0:
            raise InvalidConfig("Invalid parameter: No test queries provided")
        q = _rows(q)
        out, n = np.zeros(3, np.float32), C.c_uint64(0)
        self._check(self.lib.fvh_ivf_evaluate_search_quality(self.h, _ptr(q, f32p), q.shape[0], q.shape[1], int(k),
                                                             _ptr(out, f32p), C.byref(n)))
        return dict(avg_recall=out[0], avg_precision=out[1], avg_query_time_ms=float(out[2]), queries_evaluated=int(n.value))

    def recall_by_nprobe(self, queries, k, allowed=None):
        """evaluate_search_quality (operations.rs:329-391) at EVERY n_probe from one search of every list (DESIGN.md
        section 9m).  Returns a dict: avg_recall and avg_precision, f32 arrays of length n_clusters whose entry p - 1 is
        what evaluate_search_quality returns with n_probe = p configured, bit for bit; queries_evaluated;
        avg_query_time_ms (the call's wall time over the number of queries).  The figures are the reference's id-based
        ones when no id is stored in two lists; otherwise they count rows, not ids.  allowed: an allow-set of ids, as
        search_allowed takes it; the curve is then the one of the index with every other id deleted.
        HybridIndex has no call of its own: h.ivf() is an IVFIndex view of the historical part, and this is its curve."""
        q = np.asarray(queries, np.float32)
        if q.size == 0:
            raise InvalidConfig("Invalid parameter: No test queries provided")
        q = _rows(q)
        n = int(self.lib.fvh_ivf_n_clusters(self.h))
        recall, precision = np.zeros(n, np.float32), np.zeros(n, np.float32)
        ms, done = C.c_float(0), C.c_uint64(0)
        a = None if allowed is None else _allowed_ids(allowed)
        self._check(self.lib.fvh_ivf_quality_curve(self.h, _ptr(q, f32p), q.shape[0], q.shape[1], int(k), int(a is not None),
                                                   None if a is None else _ptr(a, u64p), 0 if a is None else a.size, n,
                                                   _ptr(recall, f32p), _ptr(precision, f32p), C.byref(ms), C.byref(done)))
        return dict(avg_recall=recall, avg_precision=precision, avg_query_time_ms=float(ms.value),
                    queries_evaluated=int(done.value))

    def smallest_n_probe(self, queries, k, target_recall, allowed=None):
        """(p, curve): the smallest n_probe whose avg_recall on these queries reaches target_recall (compared in f32), or
        None when none does, and the curve of recall_by_nprobe it was read from."""
        curve = self.recall_by_nprobe(queries, k, allowed)
        hit = np.flatnonzero(curve["avg_recall"] >= np.float32(target_recall))
        return (int(hit[0]) + 1 if hit.size else None), curve

    def maintenance_info(self):
        """Figures of the last resident maintenance job (fvdb_ivf_maintenance_info)."""
        m = _capi.MaintenanceInfo()
        self._check(self.ctx.lib.fvdb_ivf_maintenance_info(self._dev(), C.byref(m)))
        return {name: getattr(m, name) for name, _ in m._fields_}

    def export_list(self, c):
        """Rows (f32), ids and live flags of inverted list `c`, in list-position order (save path)."""
        n = self.get_cluster_size(c)
        rows, ids, live = np.empty((n, max(self.dimension(), 1)), np.float32), np.empty(n, np.uint64), np.empty(n, np.uint8)
        self._check(self.lib.fvh_ivf_export_list(self.h, int(c), _ptr(rows, f32p), _ptr(ids, u64p),
                                                 live.ctypes.data_as(C.POINTER(C.c_uint8))))
        return rows, ids, live.astype(bool)

    def get_vectors(self, ids):
        """Rows of `ids` read back from HBM with one device gather: (rows [n x d] f32, found [n] bool).  A soft-deleted
        id still has its row; of several lists holding one id the lowest (cluster, position) answers."""
        return _get_vectors(self, self.lib.fvh_ivf_get_vectors, ids, self.dimension())

    def get_vector_by_id(self, id):
        """IVFIndex::get_vector_by_id (src/ivf/core.rs:553-562): the row as f32, or None."""
        rows, found = self.get_vectors([int(id)])
        return rows[0] if found[0] else None

    def search(self, queries, k, n_probe=None):
        return self._search(self.lib.fvh_ivf_search, queries, k, self.n_probe if n_probe is None else n_probe)

    def search_exact(self, queries, k):
        """The exact k nearest live rows: the search of every list, search_with_config(q, k, n_clusters) (src/ivf/core.rs
        :626-681).  A spelling of search() that the three index classes share; it adds no engine code."""
        return self.search(queries, k, n_probe=self.n_clusters)

    def search_allowed(self, queries, k, allowed, n_probe=None):
        """search() among the rows whose id is in `allowed`: exactly what search() returns once every other row has been
        mark_deleted.  The allow-set is applied inside the list scan on the device; the last mask is kept for a caller
        that repeats one filter."""
        a = _allowed_ids(allowed)
        return self._search(self.lib.fvh_ivf_search_allowed, queries, k, self.n_probe if n_probe is None else n_probe,
                            _ptr(a, u64p), a.size)

    def search_allowed_groups(self, queries, k, allow_sets, group_of_query, n_probe=None):
        """One allow-set per query in one call: query b gets what search_allowed(queries[b], k, allow_sets[g]) returns for
        g = group_of_query[b], or what search() returns where allow_sets[g] is None.  The masks are built for this call
        (mask_builds counts them) and dropped after it; the mask search_allowed keeps is left alone."""
        q = _rows(queries)
        args, keep = _allow_groups(allow_sets, group_of_query, q.shape[0])
        return self._search(self.lib.fvh_ivf_search_allowed_groups, q, k, self.n_probe if n_probe is None else n_probe, *args)

    def search_radius(self, queries, radius, max_results=4096, n_probe=None, allowed=None):
        """Every live row of the n_probe probed lists within `radius` of its query (a scalar or one value per query; f32,
        >= 0, inf allowed; the boundary is inclusive, on the f32 distance search() reports): (results, totals).
        results[b] is what search(k=max_results) returns on the wide route, cut at the radius; totals[b] (uint32) is the
        exact size of the ball over the probed lists, never capped.  max_results in 1..4096.  allowed: as in
        search_allowed — rows outside it are in neither."""
        ap, an, keep = _allowed_args(allowed)
        return self._search_radius(self.lib.fvh_ivf_search_radius, queries, radius, max_results,
                                   self.n_probe if n_probe is None else n_probe, ap, an)

    def search_diverse(self, queries, k, fetch_k, lam=0.5, distinct=True, n_probe=None, allowed=None):
        """The k best rows that are not copies of each other: (results, ranks).  The candidates are
        exactly what search(fetch_k, n_probe) — search_allowed with `allowed` — returns; on the device, k of them are
        kept greedily by maximal marginal relevance, gain = (1 - lam) * (distance to the nearest pick) - lam * (distance
        to the query) in f32, the first pick being the nearest row; distinct drops every later copy of an id first.
        Results come in PICK order (not sorted by distance); ranks[b, i] (uint32) is the pick's position among the
        candidates.  lam = 1 is the first k (distinct) candidates; lam = 0 a farthest-first traversal.
        1 <= k <= fetch_k <= 256, lam in [0, 1]."""
        ap, an, keep = _allowed_args(allowed)
        return self._search_diverse(self.lib.fvh_ivf_search_diverse, queries, k, fetch_k, lam, distinct,
                                    self.n_probe if n_probe is None else n_probe, ap, an)

    def search_grouped(self, queries, k, group_size, fetch_k, columns, path, distinct=True, missing="drop", n_probe=None,
                       allowed=None, metadata=None):
        """The k best groups by a metadata field: GroupedResults.  The candidates are exactly what
        search(fetch_k, n_probe) — search_allowed with `allowed` — returns; on the device each candidate id is looked up
        in `columns` (a MetadataColumns) and gets the cell of `path` as its key, and walking the candidates in order the
        first k distinct keys are the groups, each with its first group_size members.  Equality is the filters': 1, 1.0,
        "1" and True are four keys, 0.0 and -0.0 one; a row without the field, with an array or an object there, or with
        a NaN has no key and is dropped (missing="drop") or forms a group of its own ("own").  distinct drops every
        later copy of an id first.  1 <= fetch_k <= 4096, k * group_size <= 4096.  metadata: the map the column of `path`
        is built from on first use (None: the one `columns` was last synchronised with)."""
        ap, an, keep = _allowed_args(allowed)
        return self._search_grouped(self.lib.fvh_ivf_search_grouped, queries, k, group_size, fetch_k, columns, path, distinct, missing,
                                    metadata, self.n_probe if n_probe is None else n_probe, ap, an)

    def mask_builds(self):
        return int(self.lib.fvh_ivf_mask_builds(self.h))

    search_with_config = search

    batch_search = search

    def mark_deleted(self, id):
        self._check(self.lib.fvh_ivf_mark_deleted(self.h, int(id)))

    def is_deleted(self, id):
        return bool(self.lib.fvh_ivf_is_deleted(self.h, int(id)))

    # --- views of the device index behind this mirror (accounting, bulk helpers) ---
    def _dev(self):
        return C.c_void_p(self.lib.fvh_ivf_device(self.h))

    def assign(self, vectors):
        """Batched find_nearest_centroid on the GPU (src/ivf/core.rs:373-386)."""
        v = _rows(vectors)
        out = np.empty(v.shape[0], np.uint32)
        self._check(self.ctx.lib.fvdb_ivf_assign(self._dev(), _ptr(v, f32p), v.shape[0], _ptr(out, u32p)))
        return out

    def list_sizes(self):
        # after a retrain whose training failed the device index still has its old lists (see _sync_config)
        out = np.zeros(max(self.n_clusters, getattr(self, "_dev_clusters", 0)), np.uint64)
        self._check(self.ctx.lib.fvdb_ivf_list_sizes(self._dev(), _ptr(out, u64p)))
        return out[:self.n_clusters]

    def stage_times(self):
        ms = np.zeros(8, np.float32)
        n = self.ctx.lib.fvdb_ivf_stage_times(self._dev(), _ptr(ms, f32p))
        return int(n), dict(zip(("coarse_scan", "coarse_merge", "plan", "fine_scan", "fine_merge", "mfma_filter_kernel"), ms.tolist()))

    def last_stats(self):
        st = _capi.SearchStats()
        self._check(self.ctx.lib.fvdb_ivf_last_stats(self._dev(), C.byref(st)))
        return dict(rows_scanned=st.rows_scanned, work_items=st.work_items, list_rows_touched=st.list_rows_touched)


class _ClusterStats(C.Structure):
    """IVFIndex::ClusterStats (host/fvdb_host.hpp)."""
    _fields_ = [("n_clusters", u64), ("total_vectors", u64), ("empty_clusters", u64), ("avg_cluster_size", C.c_float),
                ("size_variance", C.c_float)]


class _InsertInfo(C.Structure):
    """fvdb_graph_insert_info_t (include/fvdb.h)."""
    _fields_ = [(n, C.c_uint32) for n in ("mode", "representation", "table_slots", "cand_cap", "lds_bytes",
                                          "bitmap_max_nodes", "visited_peak", "reserved")] + \
               [(n, C.c_uint64) for n in ("hashed_inserts", "visited_overflows", "visited_searches", "visited_entries")]


class HNSWIndex(_Base):
    """src/hnsw/core.rs HNSWIndex (HNSWConfig::default :37-46)."""

    def __init__(self, ctx, max_connections=16, max_connections_layer_0=32, ef_construction=200, seed=0, row_dtype="f32",
                 _handle=None):
        """row_dtype "f16": the graph's row store keeps IEEE fp16.  Every inserted row is rounded once (nearest even) and
        the index is the reference algorithm on the rounded rows (get_vector_by_id returns them); queries stay f32."""
        self.ctx, self.lib = ctx, load_host()
        self._own = _handle is None
        if _handle is None:
            _handle = self.lib.fvh_hnsw_new_ex(ctx.h, max_connections, max_connections_layer_0, ef_construction, seed,
                                               row_dtype_code(row_dtype))
            if not _handle:
                raise InvalidConfig("Invalid HNSWConfig")
        self.h = _handle
        self.row_dtype = _ROW_DTYPE_NAMES[self.lib.fvh_hnsw_row_dtype(self.h)]

    def __del__(self):
        if getattr(self, "_own", False) and getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.fvh_hnsw_free(self.h)
            self.h = None

    def insert(self, id, vector, level=-1):
        v = _f32(vector).reshape(-1)
        self._check(self.lib.fvh_hnsw_insert(self.h, int(id), _ptr(v, f32p), v.size, level))

    def batch_insert(self, ids, vectors, levels=None):
        v = _rows(vectors)
        ids = np.ascontiguousarray(ids, np.uint64)
        lv = None if levels is None else np.ascontiguousarray(levels, np.int64)
        ok, err = C.c_uint64(0), C.c_int(0)
        self._check(self.lib.fvh_hnsw_batch_insert(self.h, _ptr(ids, u64p), _ptr(v, f32p), v.shape[0], v.shape[1],
                                                   None if lv is None else _ptr(lv, i64p), C.byref(ok), C.byref(err)))
        return ok.value, v.shape[0] - ok.value

    def bulk_build(self, ids, vectors, levels=None):
        v = _rows(vectors)
        ids = np.ascontiguousarray(ids, np.uint64)
        lv = None if levels is None else np.ascontiguousarray(levels, np.int64)
        self._check(self.lib.fvh_hnsw_bulk_build(self.h, _ptr(ids, u64p), _ptr(v, f32p), v.shape[0], v.shape[1],
                                                 None if lv is None else _ptr(lv, i64p)))

    def search(self, queries, k, ef):
        return self._search(self.lib.fvh_hnsw_search, queries, k, ef)

    def search_allowed(self, queries, k, ef, allowed):
        """search() among the nodes whose id is in `allowed`: what search() returns once every other node has been
        mark_deleted — unless at most scan_cutoff allowed live nodes remain: those are scanned exactly (the k best by
        distance bits, then node index)."""
        a = _allowed_ids(allowed)
        return self._search(self.lib.fvh_hnsw_search_allowed, queries, k, ef, _ptr(a, u64p), a.size)

    def search_allowed_groups(self, queries, k, ef, allow_sets, group_of_query):
        """One allow-set per query in one call: query b gets what search_allowed(queries[b], k, ef, allow_sets[g]) returns
        for g = group_of_query[b] (search(), where allow_sets[g] is None).  The queries of every group small enough to be
        scanned (scan_cutoff) share one launch; each larger group is one masked traversal of its own queries."""
        q = _rows(queries)
        args, keep = _allow_groups(allow_sets, group_of_query, q.shape[0])
        return self._search(self.lib.fvh_hnsw_search_allowed_groups, q, k, ef, *args)

    def search_exact(self, queries, k):
        """The k nearest live nodes, exactly: every live row the graph holds is scored where it is stored (as it is
        stored: the rounded rows of an "f16" index) with the reference's f32 distance; the best k by distance bits, then
        node index.  k in 1..256.  No counterpart in the reference: the ground truth recall is measured against."""
        return self._search(self.lib.fvh_hnsw_search_exact, queries, k)

    def search_exact_allowed(self, queries, k, allowed):
        """search_exact() among the nodes whose id is in `allowed` (the cached mask of search_allowed)."""
        a = _allowed_ids(allowed)
        return self._search(self.lib.fvh_hnsw_search_exact_allowed, queries, k, _ptr(a, u64p), a.size)

    def evaluate_search_quality(self, queries, k, ef):
        """search(k, ef) against search_exact(k) with the reference's formulas (src/ivf/operations.rs:357-377): per query
        matches = result entries whose id is among the truth's, recall = matches / min(len(truth), k) (1 if the truth
        is empty), precision = matches / len(result) (0 if the result is empty); compared on the device, averaged in
        f32 in query order."""
        return self._quality(self.lib.fvh_hnsw_evaluate_search_quality, queries, int(k), int(ef))

    def search_exact_wide(self, queries, k):
        """search_exact() with k in 1..4096: the same rows scored by the same fold, the k best
        chosen by the wide selection.  For k <= 256 it returns exactly what search_exact() returns; that call keeps its
        limit and its faster register list."""
        return self._search(self.lib.fvh_hnsw_search_exact_wide, queries, k)

    def search_exact_wide_allowed(self, queries, k, allowed):
        """search_exact_wide() among the nodes whose id is in `allowed` (the cached mask of search_allowed)."""
        a = _allowed_ids(allowed)
        return self._search(self.lib.fvh_hnsw_search_exact_wide_allowed, queries, k, _ptr(a, u64p), a.size)

    def search_radius(self, queries, radius, max_results=4096, allowed=None):
        """Every live node within `radius` of its query (a scalar or one value per query; f32, >= 0, inf allowed; the
        boundary is inclusive, on the f32 distance search_exact_wide() reports): (results, totals).  results[b] is
        search_exact_wide(k=max_results) cut at the radius; totals[b] (uint32) is the exact size of the ball, never
        capped.  max_results in 1..4096.  allowed: as in search_exact_wide_allowed — nodes outside it are in neither."""
        if allowed is None:
            return self._search_radius(self.lib.fvh_hnsw_search_radius, queries, radius, max_results)
        a = _allowed_ids(allowed)
        return self._search_radius(self.lib.fvh_hnsw_search_radius_allowed, queries, radius, max_results, _ptr(a, u64p), a.size)

    def search_diverse(self, queries, k, fetch_k, ef, lam=0.5, distinct=True, allowed=None):
        """IVFIndex.search_diverse over the graph: the candidates are exactly what search(fetch_k, ef) — search_allowed
        with `allowed` — returns.  A graph walk returns at most ef rows, so fetch_k > ef just yields fewer candidates.
        (results, ranks) in pick order; 1 <= k <= fetch_k <= 256, lam in [0, 1]."""
        ap, an, keep = _allowed_args(allowed)
        return self._search_diverse(self.lib.fvh_hnsw_search_diverse, queries, k, fetch_k, lam, distinct, int(ef), ap, an)

    def search_grouped(self, queries, k, group_size, fetch_k, ef, columns, path, distinct=True, missing="drop", allowed=None,
                       metadata=None):
        """IVFIndex.search_grouped over the graph: the candidates are exactly what search(fetch_k, ef) — search_allowed
        with `allowed` — returns.  A graph walk returns at most ef rows, so fetch_k > ef just yields fewer candidates (and
        a list that was not cut)."""
        ap, an, keep = _allowed_args(allowed)
        return self._search_grouped(self.lib.fvh_hnsw_search_grouped, queries, k, group_size, fetch_k, columns, path, distinct, missing,
                                    metadata, int(ef), ap, an)

    def count_within(self, queries, radius, allowed=None):
        """search_radius()'s totals alone (uint32[B]), by a scan that keeps no distances and selects nothing."""
        q = _rows(queries)
        r = _radii(radius, q.shape[0])
        ap, an, keep = _allowed_args(allowed)
        totals = np.zeros(q.shape[0], np.uint32)
        self._check(self.lib.fvh_hnsw_count_within(self.h, _ptr(q, f32p), q.shape[0], q.shape[1], _ptr(r, f32p), ap, an,
                                                   _ptr(totals, u32p)))
        return totals

    def evaluate_search_quality_wide(self, queries, k, ef):
        """evaluate_search_quality() with k in 1..4096: search(k, ef), which returns at most ef rows, against
        search_exact_wide(k); the same formulas."""
        return self._quality(self.lib.fvh_hnsw_evaluate_search_quality_wide, queries, int(k), int(ef))

    def recall_by_ef(self, queries, k, efs):
        """evaluate_search_quality (its wide form above k = 256) at every listed ef from ONE exact search (DESIGN.md section
        9r): one traversal per listed ef, one device job that counts them all.  Returns a dict: efs (the list, as
        given: duplicates and any order are fine), avg_recall and avg_precision (f32 arrays whose entry i is what the
        single call returns at efs[i], bit for bit), queries_evaluated, avg_query_time_ms (the call's wall time over the
        number of queries)."""
        k = int(k)
        recall, precision, ms, done, e, _ = self._grid(
            lambda *a: self.lib.fvh_hnsw_quality_by_ef(self.h, a[0], a[1], a[2], k, a[3], a[4], *a[7:]), queries, efs, None)
        return dict(efs=[int(x) for x in e], avg_recall=recall[:, 0], avg_precision=precision[:, 0], avg_query_time_ms=ms,
                    queries_evaluated=done)

    def smallest_ef(self, queries, k, target_recall, efs):
        """The smallest listed ef whose avg_recall on these queries reaches target_recall (compared in f32), or None when
        none does; read from recall_by_ef."""
        curve = self.recall_by_ef(queries, k, efs)
        reach = [ef for ef, r in zip(curve["efs"], curve["avg_recall"]) if r >= np.float32(target_recall)]
        return min(reach) if reach else None

    @property
    def scan_cutoff(self):
        return int(self.lib.fvh_hnsw_scan_cutoff(self.h))

    @scan_cutoff.setter
    def scan_cutoff(self, nodes):
        """0 = never scan, SCAN_ALWAYS = always.  The default (8192) is a guess nobody has measured."""
        self.lib.fvh_hnsw_set_scan_cutoff(self.h, int(nodes))

    SCAN_ALWAYS = 2 ** 64 - 1

    def mask_builds(self):
        return int(self.lib.fvh_hnsw_mask_builds(self.h))

    def _graph(self):
        """fvdb_graph* of the device graph, up to date (raw C-ABI calls in tests and tools)."""
        return C.c_void_p(self.lib.fvh_hnsw_device_graph(self.h))

    def search_dev(self, q_dev, B, dim, k, ef):
        ids = np.empty((B, max(k, 1)), np.uint64)
        ds = np.empty((B, max(k, 1)), np.float32)
        cnt = np.zeros(B, np.uint32)
        self._check(self.lib.fvh_hnsw_search_dev(self.h, q_dev, B, dim, k, ef, _ptr(ids, u64p), _ptr(ds, f32p),
                                                 _ptr(cnt, u32p)))
        return SearchResults(ids, ds, cnt)

    def search_dev_begin(self, slot, q_dev, B, dim, k, ef):
        """Enqueue the device traversal of a batch in `slot` (0..7); the query buffer must stay valid until
        search_dev_end(slot)."""
        rc = self.lib.fvh_hnsw_search_dev_begin(self.h, slot, q_dev, B, dim, k, ef)
        if rc < 0:
            self._check(-rc)
        self._inflight = getattr(self, "_inflight", {})
        self._inflight[slot] = (q_dev, B, dim, k, ef, rc == 1)

    def search_dev_end(self, slot):
        q_dev, B, dim, k, ef, started = self._inflight.pop(slot)
        if not started:  # not a device-path search (host-walk mode, empty index ...): run it now
            return self.search_dev(q_dev, B, dim, k, ef)
        ids = np.empty((B, max(k, 1)), np.uint64)
        ds = np.empty((B, max(k, 1)), np.float32)
        cnt = np.zeros(B, np.uint32)
        self._check(self.lib.fvh_hnsw_search_dev_end(self.h, slot, q_dev, B, dim, k, ef, _ptr(ids, u64p), _ptr(ds, f32p),
                                                     _ptr(cnt, u32p)))
        return SearchResults(ids, ds, cnt)

    def node_count(self):
        return int(self.lib.fvh_hnsw_node_count(self.h))

    def active_count(self):
        return int(self.lib.fvh_hnsw_active_count(self.h))

    def entry_point(self):
        out = C.c_uint64(0)
        return None if self.lib.fvh_hnsw_entry_point(self.h, C.byref(out)) else out.value

    def level(self, id):
        return int(self.lib.fvh_hnsw_level(self.h, int(id)))

    def neighbors(self, id, layer):
        buf = np.empty(1024, np.uint64)
        n = self.lib.fvh_hnsw_neighbors(self.h, int(id), layer, _ptr(buf, u64p), buf.size)
        if n < 0:
            raise STATUS_TO_EXC[7](f"Vector not found: {id}")
        return [int(x) for x in buf[:n]]

    def mark_deleted(self, id):
        self._check(self.lib.fvh_hnsw_mark_deleted(self.h, int(id)))

    def is_deleted(self, id):
        return bool(self.lib.fvh_hnsw_is_deleted(self.h, int(id)))

    def vacuum(self):
        """Deleted nodes leave every neighbour list and the node map; returns how many.  With a device graph this is one
        device job that also gives their rows back (set_resident_vacuum); a failure raises."""
        out = C.c_uint64(0)
        self._check(self.lib.fvh_hnsw_vacuum_ex(self.h, C.byref(out)))
        return out.value

    def set_resident_vacuum(self, on):
        """True (default): vacuum() runs on the adjacency in HBM and compacts the row store (fvdb_graph_vacuum).  False:
        the host algorithm — lists pulled, filtered and installed whole at the next device use, rows kept.  Same
        graph and same answers either way."""
        self.lib.fvh_hnsw_set_resident_vacuum(self.h, int(bool(on)))

    def resident_vacuum(self):
        return bool(self.lib.fvh_hnsw_resident_vacuum(self.h))

    def _set_vacuum_keep_rows(self, on):
        """A/B and tests: the resident job prunes in place and reclaims nothing (FVDB_VACUUM_KEEP_ROWS)."""
        self.lib.fvh_hnsw_set_vacuum_keep_rows(self.h, int(bool(on)))

    def vacuum_info(self):
        """The last vacuum() that removed something: "path" (None before the first, "resident", "resident_keep_rows" or
        "host") and, for a resident one, the device job's figures (fvdb_graph_maintenance_info_t; zeros otherwise)."""
        m = _capi.GraphMaintenanceInfo()
        path = self.lib.fvh_hnsw_vacuum_info(self.h, C.cast(C.pointer(m), C.c_void_p))
        out = {name: getattr(m, name) for name, _ in m._fields_}
        out["path"] = (None, "resident", "resident_keep_rows", "host")[path]
        return out

    def get_graph_stats(self):
        """The reference's GraphStats over the live nodes (src/hnsw/operations.rs:227-272), "connected_components" being
        its stub: 1 whenever a node is live.  graph_health() has the real figures."""
        out = np.zeros(5, np.uint64)
        self._check(self.lib.fvh_hnsw_graph_stats(self.h, _ptr(out, u64p)))
        return {"total_nodes": int(out[0]), "total_edges": int(out[1]),
                "avg_degree": float(np.array([out[4]], np.uint64).astype(np.uint32).view(np.float32)[0]),
                "max_layer": int(out[2]), "connected_components": int(out[3])}

    def get_max_level(self):
        """The highest level among the nodes the index holds, deleted ones included (src/hnsw/core.rs:667-670)."""
        return int(self.lib.fvh_hnsw_max_level(self.h))

    def get_level_distribution(self):
        """Nodes present on each layer, deleted ones included: get_max_level() + 1 entries (src/hnsw/core.rs:673-684)."""
        out = np.zeros(self.get_max_level() + 1, np.uint64)
        self.lib.fvh_hnsw_level_distribution(self.h, _ptr(out, u64p))
        return [int(x) for x in out]

    def graph_health(self, reach=True, components=True):
        """What deletes and vacuums have done to the graph, computed exactly by one read-only device job on the adjacency in
        HBM (fvdb_graph_health_t, include/fvdb.h): reachable_live / unreachable_live (live nodes any search can / no search
        can admit, whatever the query, ef and k), the weak components of the live layer-0 graph, dangling links and the
        layer-0 degree histogram.  "path": "device", or "host" where the mirror restated the same definitions itself
        (device traversal off, an empty index, a graph the device cannot hold).  A part switched off reads as zeros."""
        m, path = _capi.GraphHealth(), C.c_int(0)
        flags = (0 if reach else _capi.HEALTH_SKIP_REACH) | (0 if components else _capi.HEALTH_SKIP_COMPONENTS)
        self._check(self.lib.fvh_hnsw_graph_health(self.h, flags, C.byref(m), C.byref(path)))
        out = {name: getattr(m, name) for name, _ in m._fields_}
        out["degree0_hist"] = [int(x) for x in m.degree0_hist]
        out["path"] = (None, "device", "host")[path.value]
        return out

    def unreachable_ids(self):
        """Ids of the live nodes no search can return, in node order."""
        buf = np.empty(max(self.active_count(), 1), np.uint64)
        n = C.c_uint64(0)
        self._check(self.lib.fvh_hnsw_unreachable(self.h, _ptr(buf, u64p), buf.size, C.byref(n)))
        return buf[:n.value].copy()

    def component_labels(self):
        """(ids, labels) in export_graph()'s node order: labels[i] is the id of the smallest-index node of the layer-0
        component ids[i] lies in, 2**64 - 1 for a deleted node."""
        n = self.node_count()
        if n == 0:
            return np.empty(0, np.uint64), np.empty(0, np.uint64)
        labels = np.empty(n, np.uint64)
        self._check(self.lib.fvh_hnsw_component_labels(self.h, _ptr(labels, u64p)))
        return self.export_graph()[0], labels

    def store_rows(self):
        """Rows the index's vectors occupy in HBM (equals node_count() after a resident vacuum)."""
        return int(self.lib.fvh_hnsw_store_rows(self.h))

    def store_bytes(self):
        """HBM the index's vectors occupy: store_rows() x the padded row's bytes (half as many with row_dtype "f16")."""
        return int(self.lib.fvh_hnsw_store_bytes(self.h))

    def get_vector_by_id(self, id):
        out = np.empty(int(self.lib.fvh_hnsw_dimension(self.h)), np.float32)
        self._check(self.lib.fvh_hnsw_get_vector(self.h, int(id), _ptr(out, f32p)))
        return out

    def export_graph(self):
        n = int(self.lib.fvh_hnsw_node_count(self.h))
        slots, edges = int(self.lib.fvh_hnsw_graph_slots(self.h)), int(self.lib.fvh_hnsw_graph_edges(self.h))
        ids, lv = np.empty(n, np.uint64), np.empty(n, np.uint32)
        off, nb = np.empty(slots + 1, np.uint64), np.empty(max(edges, 1), np.uint64)
        self.lib.fvh_hnsw_export_graph(self.h, _ptr(ids, u64p), _ptr(lv, u32p), _ptr(off, u64p), _ptr(nb, u64p))
        return ids, lv, off, nb[:edges]

    def restore(self, ids, vectors, levels, nbr_offsets, nbrs, entry):
        v = _rows(vectors)
        ids = np.ascontiguousarray(ids, np.uint64)
        lv = np.ascontiguousarray(levels, np.uint32)
        off = np.ascontiguousarray(nbr_offsets, np.uint64)
        nb = np.ascontiguousarray(nbrs if len(nbrs) else [0], np.uint64)
        self._check(self.lib.fvh_hnsw_restore(self.h, _ptr(ids, u64p), _ptr(v, f32p), v.shape[0], v.shape[1],
                                              _ptr(lv, u32p), _ptr(off, u64p), _ptr(nb, u64p), int(entry)))

    def dist_evals(self):
        return int(self.lib.fvh_hnsw_dist_evals(self.h))

    def hops(self):
        return int(self.lib.fvh_hnsw_hops(self.h))

    def set_threads(self, t):
        self.lib.fvh_hnsw_set_threads(self.h, int(t))

    def set_device_traversal(self, on):
        """True (default): the layered walk runs on the GPU (one launch per batch); False: on the host
        with one scoring launch per hop (the north_star's split).  Results are identical."""
        self.lib.fvh_hnsw_set_device_traversal(self.h, int(bool(on)))

    def device_traversal(self):
        return bool(self.lib.fvh_hnsw_device_traversal(self.h))

    def set_device_insert(self, on, mode=0):
        """True (default): an insert's searches, links and prunes run on the GPU against the adjacency in HBM
        (fvdb_graph_insert_linked); False: the host algorithm with every distance batch scored on the GPU.
        mode 0 = choose, 1 = one insert at a time, 2 = speculate batches.  The graph is identical."""
        self.lib.fvh_hnsw_set_device_insert(self.h, int(bool(on)), int(mode))

    def device_insert(self):
        return bool(self.lib.fvh_hnsw_device_insert(self.h))

    def insert_stats(self):
        """Sums since construction: device-insert counters, inserts that took the host algorithm, and the
        host -> device bytes of graph structure moved (levels, patched rows, whole-graph installs)."""
        st = (C.c_uint32 * 10)()
        host, up = C.c_uint64(0), C.c_uint64(0)
        self.lib.fvh_hnsw_insert_stats(self.h, C.cast(st, C.c_void_p), C.byref(host), C.byref(up))
        names = ("n_done", "needs_host", "speculated_ok", "searched_in_commit", "commit_stops", "rounds", "expanded",
                 "rows_scored", "tie_restarts", "launches")
        out = {k: int(v) for k, v in zip(names, st)}
        out["host_path_inserts"] = host.value
        out["graph_upload_bytes"] = up.value
        info = self._insert_info()
        out["hashed_inserts"] = info.hashed_inserts if info else 0
        out["visited_overflows"] = info.visited_overflows if info else 0
        out["visited_peak"] = info.visited_peak if info else 0
        return out

    def set_insert_visited(self, mode, slots=0):
        """The device insert keeps `visited` on chip.  mode 0 (default) or "auto": a bitmap over all nodes while the
        graph fits it, a hashed set of node indices beyond; 1 / "bitmap": bitmap only (larger graphs are linked by the
        host algorithm); 2 / "hashed": hashed always.  slots: size of the hashed table, a power of two in 256..32768
        (0 = default).  An insert whose search fills the table takes the host algorithm.  The graph is identical."""
        mode = {"auto": 0, "bitmap": 1, "hashed": 2}.get(mode, mode)
        rc = self.lib.fvh_hnsw_set_insert_visited(self.h, int(mode), int(slots))
        if rc:
            raise ValueError(f"set_insert_visited({mode}, {slots}): mode 0..2, slots 0 or a power of two in 256..32768")

    def _insert_info(self):
        info = _InsertInfo()
        rc = self.lib.fvh_hnsw_insert_info(self.h, C.cast(C.pointer(info), C.c_void_p))
        return None if rc else info

    def insert_info(self):
        """What the next device insert would use for the graph as it stands: representation ("bitmap" / "hashed" /
        None when neither fits and the host algorithm links), the hashed table's slots, the `candidates` heap's slots,
        LDS bytes per workgroup, the largest node count the bitmap serves — and what the hashed set has seen so far
        (inserts, overflows, largest and mean number of entries after a search)."""
        info = self._insert_info()
        if info is None:
            raise RuntimeError("insert_info: the index has no device graph yet (insert or search first)")
        return {
            "mode": ("auto", "bitmap", "hashed")[info.mode],
            "representation": (None, "bitmap", "hashed")[info.representation],
            "table_slots": int(info.table_slots), "cand_cap": int(info.cand_cap), "lds_bytes": int(info.lds_bytes),
            "bitmap_max_nodes": int(info.bitmap_max_nodes), "hashed_inserts": int(info.hashed_inserts),
            "visited_overflows": int(info.visited_overflows), "visited_peak": int(info.visited_peak),
            "visited_mean": info.visited_entries / info.visited_searches if info.visited_searches else 0.0,
        }

    def search_info(self, B, ef):
        """What a device search of B queries at ef would run on the graph as it stands (fvdb_graph_search_info: the
        launch's own plan, nothing allocated or launched): "visited" ("bytes" / "bits" per node), "kernel"
        ("sorted_register" / "exact_heap"), "nb128", "rows_per_round" (0 for the exact-heap kernel),
        "nearest_in_registers", "tcap", "cand_cap", "spill_cap", "lds_bytes", "visited_bytes" (the batch's maps)."""
        g = self._graph()
        if not g:
            raise RuntimeError("search_info: the index has no device graph (empty, or a list longer than 64)")
        info = _capi.GraphSearchInfo()
        self._check(_capi.load().fvdb_graph_search_info(g, int(B), int(ef), C.byref(info)))
        out = {name: int(getattr(info, name)) for name, _ in info._fields_ if name != "reserved"}
        out["visited"] = (None, "bytes", "bits")[info.visited]
        out["kernel"] = (None, "sorted_register", "exact_heap")[info.kernel]
        out["nearest_in_registers"] = bool(info.nearest_in_registers)
        return out

    def device_fallbacks(self):
        return int(self.lib.fvh_hnsw_device_fallbacks(self.h))

    def graph_kernel_times(self):
        """(summed ms, launches timed, rows scored, hops) of the device traversal kernel since the last call
        (timings need ctx profiling on; the counters are always kept)."""
        ms, n, rows, hops = C.c_float(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        self.lib.fvh_hnsw_graph_kernel_times(self.h, C.byref(ms), C.byref(n), C.byref(rows), C.byref(hops))
        return float(ms.value), int(n.value), int(rows.value), int(hops.value)


    def tie_restarts(self):
        """(queries served by the device traversal, queries it searched again with the restated heaps) since creation."""
        q, a = C.c_uint64(0), C.c_uint64(0)
        self.lib.fvh_hnsw_tie_restarts(self.h, C.byref(q), C.byref(a))
        return int(q.value), int(a.value)


class HybridIndex(_Base):
    """src/hybrid/core.rs HybridIndex.  Timestamps / `now` are seconds supplied by the caller."""

    WEEK = 7 * 24 * 3600.0

    def __init__(self, ctx, recent_threshold=WEEK, migration_batch_size=100, auto_migrate=True,
                 min_ivf_training_size=10, max_connections=16, max_connections_layer_0=32, ef_construction=200,
                 hnsw_seed=0, n_clusters=3, n_probe=2, train_size=9, max_iterations=25, ivf_seed=0, ctx_hnsw=None,
                 row_dtype="f32"):
        # defaults = HybridConfig::default (src/hybrid/core.rs:69-85); row_dtype "f16": the graph's rows and the lists'
        # rows are IEEE fp16, rounded once at insert (one knob for both parts)
        self.ctx, self.lib = ctx, load_host()
        self.row_dtype = _ROW_DTYPE_NAMES[row_dtype_code(row_dtype)]
        self.ctx_hnsw = ctx_hnsw or ctx
        self.n_clusters, self.n_probe = n_clusters, n_probe
        self.config = dict(recent_threshold=recent_threshold, migration_batch_size=migration_batch_size,
                           auto_migrate=auto_migrate, min_ivf_training_size=min_ivf_training_size,
                           max_connections=max_connections, max_connections_layer_0=max_connections_layer_0,
                           ef_construction=ef_construction, hnsw_seed=hnsw_seed, n_clusters=n_clusters, n_probe=n_probe,
                           train_size=train_size, max_iterations=max_iterations, ivf_seed=ivf_seed,
                           row_dtype=self.row_dtype)
        self.h = self.lib.fvh_hybrid_new_ex(ctx.h, self.ctx_hnsw.h, recent_threshold, migration_batch_size,
                                            int(auto_migrate), min_ivf_training_size, max_connections,
                                            max_connections_layer_0, ef_construction, hnsw_seed, n_clusters, n_probe,
                                            train_size, max_iterations, ivf_seed, row_dtype_code(self.row_dtype))
        if not self.h:
            raise InvalidConfig("Invalid HybridConfig")

    def __del__(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.lib.fvh_hybrid_free(self.h)
            self.h = None

    def is_initialized(self):
        return bool(self.lib.fvh_hybrid_is_initialized(self.h))

    def is_ivf_trained(self):
        return bool(self.lib.fvh_hybrid_is_ivf_trained(self.h))

    def initialize(self, training_data):
        x = _f32(training_data)
        if x.ndim != 2:
            x = x.reshape(len(training_data), -1)
        self._check(self.lib.fvh_hybrid_initialize(self.h, _ptr(x, f32p), x.shape[0], x.shape[1]))

    def set_ivf_centroids(self, centroids):
        c = _rows(centroids)
        self._check(self.lib.fvh_hybrid_set_ivf_centroids(self.h, _ptr(c, f32p), c.shape[1]))

    def insert_with_timestamp(self, id, vector, timestamp, now, level=-1):
        v = _f32(vector).reshape(-1)
        self._check(self.lib.fvh_hybrid_insert(self.h, int(id), _ptr(v, f32p), v.size, float(timestamp), float(now), level))

    def insert(self, id, vector, now=0.0, level=-1):
        self.insert_with_timestamp(id, vector, now, now, level)

    def set_sequential_graph(self, on):
        """How bulk_insert builds the recent part's graph: True (default) = the reference's sequential inserts
        (device-resident), False = HNSWIndex.bulk_build (exact nearest-M per layer: an extension, another graph)."""
        self.lib.fvh_hybrid_set_sequential_graph(self.h, int(bool(on)))

    def sequential_graph(self):
        return bool(self.lib.fvh_hybrid_sequential_graph(self.h))

    def set_blocking_writers(self, on):
        """Mutations while batches begun with search_dev_begin are uncollected: False (default) = FvdbError(INVALID) at once,
        True = wait until they are collected (the reference's write guard; for searches and writes on different threads)."""
        self.lib.fvh_hybrid_set_blocking_writers(self.h, int(bool(on)))

    def recent_build_seconds(self):
        return float(self.lib.fvh_hybrid_recent_build_seconds(self.h))

    def bulk_insert(self, ids, vectors, timestamps, now):
        v = _rows(vectors)
        ids = np.ascontiguousarray(ids, np.uint64)
        ts = np.ascontiguousarray(timestamps, np.float64)
        self._check(self.lib.fvh_hybrid_bulk_insert(self.h, _ptr(ids, u64p), _ptr(v, f32p), v.shape[0], v.shape[1],
                                                    _ptr(ts, f64p), float(now)))

    def bulk_insert_sharded(self, ids, vectors, timestamps, now, rank, world):
        """Multi-GPU placement: HNSW replicated, IVF lists owned by `rank` only.  Returns owner[nlist]."""
        self._refuse_sharded_f16("bulk_insert_sharded")
        v = _rows(vectors)
        ids = np.ascontiguousarray(ids, np.uint64)
        ts = np.ascontiguousarray(timestamps, np.float64)
        owner = np.zeros(self.n_clusters, np.uint32)
        self._sharded = True
        self._check(self.lib.fvh_hybrid_bulk_insert_sharded(self.h, _ptr(ids, u64p), _ptr(v, f32p), v.shape[0],
                                                            v.shape[1], _ptr(ts, f64p), float(now), rank, world,
                                                            _ptr(owner, u32p)))
        return owner

    def search(self, queries, k, now=0.0, hnsw_ef=50, ivf_n_probe=10, search_recent=True, search_historical=True,
               recent_k=0, historical_k=0):
        # HybridSearchConfig::default (src/hybrid/core.rs:184-197)
        return self._search(self.lib.fvh_hybrid_search, queries, k, hnsw_ef, ivf_n_probe, int(search_recent),
                            int(search_historical), recent_k, historical_k, float(now))

    search_with_config = search

    def search_allowed(self, queries, k, allowed, now=0.0, hnsw_ef=50, ivf_n_probe=10, search_recent=True,
                       search_historical=True, recent_k=0, historical_k=0):
        """search() with the allow-set applied inside both parts on the device: what search() returns once every id
        outside `allowed` has been deleted (the recent part scanned exactly below recent().scan_cutoff).  Unlike
        search_with_filter it returns k matches whenever the searched rows hold k."""
        a = _allowed_ids(allowed)
        return self._search(self.lib.fvh_hybrid_search_allowed, queries, k, hnsw_ef, ivf_n_probe, int(search_recent),
                            int(search_historical), recent_k, historical_k, _ptr(a, u64p), a.size, float(now))

    def search_allowed_groups(self, queries, k, allow_sets, group_of_query, now=0.0, hnsw_ef=50, ivf_n_probe=10,
                              search_recent=True, search_historical=True):
        """One allow-set per query in one call: query b gets what search_allowed(queries[b], k, allow_sets[g], ...) returns
        for g = group_of_query[b] (search(), where allow_sets[g] is None).  One auto-migration step; every mask is built
        after it.  Refused (Unsupported) on a sharded index, as search_allowed is."""
        q = _rows(queries)
        args, keep = _allow_groups(allow_sets, group_of_query, q.shape[0])
        return self._search(self.lib.fvh_hybrid_search_allowed_groups, q, k, hnsw_ef, ivf_n_probe, int(search_recent),
                            int(search_historical), *args, float(now))

    def search_exact(self, queries, k, now=0.0, search_recent=True, search_historical=True):
        """search() with both parts exact: the recent part from the flat scan of the graph's rows, the historical part
        from the search of every list, merged as search() merges (no de-duplication: a migrated row that still sits in
        the graph appears twice).  Takes the same auto-migration step and read lock.  k in 1..256.  Refused
        (Unsupported) on a sharded index: each rank holds only the lists it owns, so no rank can answer alone."""
        self._refuse_when_sharded("search_exact")
        return self._search(self.lib.fvh_hybrid_search_exact, queries, k, int(search_recent), int(search_historical),
                            float(now))

    def evaluate_search_quality(self, queries, k, now=0.0, hnsw_ef=50, ivf_n_probe=10):
        """search(k, hnsw_ef, ivf_n_probe) against search_exact(k), both under one hold of the read lock after one
        migration step; the formulas of HNSWIndex.evaluate_search_quality (an id returned twice counts twice).  Refused
        on a sharded index, as search_exact is."""
        self._refuse_when_sharded("evaluate_search_quality")
        return self._quality(self.lib.fvh_hybrid_evaluate_search_quality, queries, int(k), int(hnsw_ef), int(ivf_n_probe),
                             float(now))

    def search_exact_wide(self, queries, k, now=0.0, search_recent=True, search_historical=True):
        """search_exact() with k in 1..4096: the recent part from the graph's wide exact scan, the
        rest — migration step, read lock, every-list search, merge, the sharded refusal — as there."""
        self._refuse_when_sharded("search_exact_wide")
        return self._search(self.lib.fvh_hybrid_search_exact_wide, queries, k, int(search_recent), int(search_historical),
                            float(now))

    def search_radius(self, queries, radius, max_results=4096, now=0.0, ivf_n_probe=10, search_recent=True, search_historical=True,
                      allowed=None):
        """Every resident row within `radius` of its query (a scalar or one value per query; f32, >= 0, inf allowed; the
        boundary is inclusive): (results, totals).  The recent part is the graph's exact radius scan (a walk bounded by ef
        cannot enumerate a ball), the historical part the ball of the ivf_n_probe probed lists (every list at
        ivf_n_probe = n_clusters); each is capped at max_results (1..4096) and the two are merged as search() merges.
        totals[b] (uint32) = recent total + historical total, exact and never capped; like the merge it does not
        de-duplicate, so a migrated row that still sits in the graph counts twice.  One auto-migration step, the read
        lock.  allowed: as in search_allowed.  Refused (Unsupported) on a sharded index."""
        self._refuse_when_sharded("search_radius")
        ap, an, keep = _allowed_args(allowed)
        return self._search_radius(self.lib.fvh_hybrid_search_radius, queries, radius, max_results, int(ivf_n_probe),
                                   int(search_recent), int(search_historical), ap, an, float(now))

    def search_diverse(self, queries, k, fetch_k, lam=0.5, distinct=True, now=0.0, hnsw_ef=50, ivf_n_probe=10,
                       search_recent=True, search_historical=True, allowed=None):
        """IVFIndex.search_diverse over both parts: the candidates are exactly what search(fetch_k, ...) — search_allowed
        with `allowed` — returns at these settings (the walk yields at most hnsw_ef recent rows), after one
        auto-migration step; the search, the id-to-row lookup (the recent part first, as get_vectors) and the gather run
        under one hold of the read lock.  search() returns a migrated row that still sits in the graph twice; with
        distinct it comes once, and lam = 1 with distinct is the de-duplicated search().  (results, ranks) in pick order;
        1 <= k <= fetch_k <= 256, lam in [0, 1].  Refused (Unsupported) on a sharded index."""
        self._refuse_when_sharded("search_diverse")
        ap, an, keep = _allowed_args(allowed)
        return self._search_diverse(self.lib.fvh_hybrid_search_diverse, queries, k, fetch_k, lam, distinct, int(hnsw_ef),
                                    int(ivf_n_probe), int(search_recent), int(search_historical), ap, an, float(now))

    def search_grouped(self, queries, k, group_size, fetch_k, columns, path, distinct=True, missing="drop", now=0.0, hnsw_ef=50,
                       ivf_n_probe=10, search_recent=True, search_historical=True, allowed=None, metadata=None):
        """IVFIndex.search_grouped over both parts: the candidates are exactly what search(fetch_k, ...) — search_allowed
        with `allowed` — returns at these settings, after its auto-migration step.  search() returns a migrated row that
        still sits in the graph twice; with distinct it takes one seat of its group.  Refused (Unsupported) on a sharded
        index."""
        self._refuse_when_sharded("search_grouped")
        ap, an, keep = _allowed_args(allowed)
        return self._search_grouped(self.lib.fvh_hybrid_search_grouped, queries, k, group_size, fetch_k, columns, path, distinct, missing,
                                    metadata, int(hnsw_ef), int(ivf_n_probe), int(search_recent), int(search_historical), ap, an, float(now))

    def search_diverse_groups(self, queries, k, fetch_k, allow_sets, group_of_query, lam=0.5, distinct=True, now=0.0, hnsw_ef=50,
                              ivf_n_probe=10, search_recent=True, search_historical=True):
        """search_diverse() with one allow-set per query: the candidates of query b are what search_allowed_groups(fetch_k,
        allow_sets, group_of_query) returns for it; one selection serves the batch."""
        self._refuse_when_sharded("search_diverse_groups")
        q = _rows(queries)
        args, keep = _allow_groups(allow_sets, group_of_query, q.shape[0])
        return self._search_diverse(self.lib.fvh_hybrid_search_diverse_groups, q, k, fetch_k, lam, distinct, int(hnsw_ef),
                                    int(ivf_n_probe), int(search_recent), int(search_historical), *args, float(now))

    def evaluate_search_quality_wide(self, queries, k, now=0.0, hnsw_ef=50, ivf_n_probe=10):
        """evaluate_search_quality() with k in 1..4096: search() against search_exact_wide() under one hold of the lock."""
        self._refuse_when_sharded("evaluate_search_quality_wide")
        return self._quality(self.lib.fvh_hybrid_evaluate_search_quality_wide, queries, int(k), int(hnsw_ef),
                             int(ivf_n_probe), float(now))

    def quality_grid(self, queries, k, efs, n_probes, now=0.0, search_recent=True, search_historical=True):
        """evaluate_search_quality (its wide form above k = 256) at EVERY pair (efs[i], n_probes[j]) in one call (DESIGN.md
        section 9r): one migration step, one exact search, one traversal per listed ef, one list search per listed
        n_probe, one device job that merges and counts every pair.  Returns a dict: efs and n_probes (the lists, as
        given: duplicates and any order are fine), avg_recall and avg_precision (f32 arrays [E][P] whose entry (i, j) is
        what evaluate_search_quality(queries, k, now, efs[i], n_probes[j]) returns, bit for bit), queries_evaluated,
        avg_query_time_ms (the call's wall time over the number of queries).  A part that is not searched (or lists that
        are untrained) leaves its axis constant; its list may then be empty and the axis has length 1.  Refused on a
        sharded index, as evaluate_search_quality is."""
        self._refuse_when_sharded("quality_grid")
        k, sr, sh, now = int(k), int(bool(search_recent)), int(bool(search_historical)), float(now)
        recall, precision, ms, done, e, p = self._grid(
            lambda *a: self.lib.fvh_hybrid_quality_grid(self.h, a[0], a[1], a[2], k, sr, sh, 0, 0, a[3], a[4], a[5], a[6], now,
                                                        *a[7:]), queries, efs, n_probes)
        return dict(efs=[int(x) for x in e], n_probes=[int(x) for x in p], avg_recall=recall, avg_precision=precision,
                    avg_query_time_ms=ms, queries_evaluated=done)

    def operating_points(self, queries, k, target_recall, efs, n_probes, now=0.0):
        """The cheapest pairs that reach target_recall on these queries (compared in f32), read from quality_grid: every
        listed (ef, n_probe) whose avg_recall reaches the target and that no other reaching pair dominates — none with
        ef' <= ef and n_probe' <= n_probe.  A list of dicts (ef, n_probe, avg_recall, avg_precision) sorted by ef; empty
        when no pair reaches the target.  No timing is involved: which of them is fastest is for the caller to measure."""
        grid = self.quality_grid(queries, k, efs, n_probes, now)
        return pareto_points(grid, target_recall)

    _FILTER_FN =C.CFUNCTYPE(C.c_int, C.c_uint64, C.c_void_p)

    def search_with_filter(self, queries, k, matches=None, now=0.0):
        """HybridIndex::search_with_filter (src/hybrid/core.rs:513-549) in the host mirror: 3 k candidates with the
        default search config, the first k whose id `matches(id)` accepts (None = no filter = plain search).  The
        oversampling, the walk over the candidates and the truncation run below Python; `matches` stands for the
        application's metadata_map lookup + MetadataFilter::matches."""
        q = _rows(queries)
        B = q.shape[0]
        ids = np.empty((B, max(k, 1)), np.uint64)
        ds = np.empty((B, max(k, 1)), np.float32)
        cnt = np.zeros(B, np.uint32)
        failure = []

        def trampoline(rid, _user):
            try:
                return 1 if matches(int(rid)) else 0
            except Exception as e:  # noqa: BLE001 — must not unwind through the C frames
                failure.append(e)
                return 0

        cb = self._FILTER_FN(trampoline) if matches is not None else C.cast(None, self._FILTER_FN)
        self._check(self.lib.fvh_hybrid_search_with_filter(self.h, _ptr(q, f32p), B, q.shape[1], k, C.cast(cb, C.c_void_p),
                                                           None, float(now), _ptr(ids, u64p), _ptr(ds, f32p), _ptr(cnt, u32p)))
        if failure:
            raise failure[0]
        return SearchResults(ids, ds, cnt)

    def search_dev(self, q_dev, B, k, now=0.0, hnsw_ef=50, ivf_n_probe=10, search_recent=True, search_historical=True,
                   recent_k=0, historical_k=0, dim=None):
        """Same search with the B x d query batch already resident in HBM (device pointer)."""
        ids = np.empty((B, max(k, 1)), np.uint64)
        ds = np.empty((B, max(k, 1)), np.float32)
        cnt = np.zeros(B, np.uint32)
        self._check(self.lib.fvh_hybrid_search_dev(self.h, q_dev, B, dim, k, hnsw_ef, ivf_n_probe, int(search_recent),
                                                   int(search_historical), recent_k, historical_k, float(now),
                                                   _ptr(ids, u64p), _ptr(ds, f32p), _ptr(cnt, u32p)))
        return SearchResults(ids, ds, cnt)

    SLOTS = 16

    def search_dev_begin(self, slot, q_dev, B, k, now=0.0, hnsw_ef=50, ivf_n_probe=10, search_recent=True,
                         search_historical=True, recent_k=0, historical_k=0, dim=None):
        """Enqueue a batch search in `slot` (0..SLOTS-1) and return at once; several slots may be in flight together
        (the graph walk of one batch uses one wavefront per SIMD, so a second batch's walk runs beside it).  The
        query buffer must stay valid until search_dev_end(slot).  Inserts, deletes and migrations are refused (status
        INVALID) while any slot is in flight, and so is a begin whose `now` makes an auto-migration due.
        Timing: the graph walk starts now; the IVF part of the batch may start at the NEXT search_dev_begin — one IVF
        chain then serves both batches — or at this batch's own search_dev_end (unsharded index, no allow-set;
        FVDB_HYBRID_PAIR=0 starts every chain at its begin).  Results and error codes are unchanged."""
        self._check(self.lib.fvh_hybrid_search_dev_begin(self.h, slot, q_dev, B, dim, k, hnsw_ef, ivf_n_probe,
                                                         int(search_recent), int(search_historical), recent_k,
                                                         historical_k, float(now)))
        self._inflight = getattr(self, "_inflight", {})
        self._inflight[slot] = (B, k)

    def search_dev_end(self, slot):
        """Wait for the batch of `slot` and return its SearchResults."""
        B, k = self._inflight.pop(slot)
        ids = np.empty((B, max(k, 1)), np.uint64)
        ds = np.empty((B, max(k, 1)), np.float32)
        cnt = np.zeros(B, np.uint32)
        self._check(self.lib.fvh_hybrid_search_dev_end(self.h, slot, _ptr(ids, u64p), _ptr(ds, f32p), _ptr(cnt, u32p)))
        return SearchResults(ids, ds, cnt)

    # ---- multi-GPU (sharded.py is the user-facing wrapper) ----
    def _refuse_when_sharded(self, what):
        # the host mirror refuses the same call with FVDB_E_UNSUPPORTED; it has no message channel of its own
        if getattr(self, "_sharded", False):
            exc = Unsupported(f"{what}: not served on a sharded HybridIndex: each rank holds only the inverted lists it "
                              "owns, so no rank can give the exact answer alone")
            exc.status = 12
            raise exc

    def _refuse_sharded_f16(self, what):
        # the host mirror refuses the same call with FVDB_E_UNSUPPORTED; it has no message channel of its own
        if self.row_dtype == "f16":
            exc = Unsupported(f'{what}: a HybridIndex with row_dtype="f16" cannot be sharded: the sharded step and the '
                              'replicated graph serve f32 rows only')
            exc.status = 12
            raise exc

    def attach_comm(self, comm_handle):
        if comm_handle:
            self._refuse_sharded_f16("attach_comm")
        self._check(self.lib.fvh_hybrid_attach_comm(self.h, comm_handle))
        self._sharded = True

    def sharded_rows(self, B, mode):
        return int(self.lib.fvh_hybrid_sharded_rows(self.h, B, mode))

    def search_sharded_begin(self, slot, q_dev, B, k, mode, hnsw_ef=50, ivf_n_probe=10, search_recent=True,
                             search_historical=True, recent_k=0, historical_k=0, dim=None, now=0.0):
        self._check(self.lib.fvh_hybrid_search_sharded_begin(self.h, slot, q_dev, B, dim, k, hnsw_ef, ivf_n_probe,
                                                             int(search_recent), int(search_historical), recent_k,
                                                             historical_k, mode, float(now)))
        self._inflight = getattr(self, "_inflight", {})
        self._inflight[slot] = (self.sharded_rows(B, mode), k)

    def search_allowed_sharded_begin(self, slot, q_dev, B, k, mode, allowed, hnsw_ef=50, ivf_n_probe=10, search_recent=True,
                                     search_historical=True, recent_k=0, historical_k=0, dim=None, now=0.0):
        """search_sharded_begin under an allow-set (search_allowed's semantics): every rank passes the same `allowed`.
        Collected by search_sharded_end."""
        a = np.ascontiguousarray(allowed, np.uint64).reshape(-1)
        self._check(self.lib.fvh_hybrid_search_allowed_sharded_begin(self.h, slot, q_dev, B, dim, k, hnsw_ef, ivf_n_probe,
                                                                     int(search_recent), int(search_historical), recent_k,
                                                                     historical_k, mode, _ptr(a, u64p), a.size, float(now)))
        self._inflight = getattr(self, "_inflight", {})
        self._inflight[slot] = (self.sharded_rows(B, mode), k)

    def search_sharded_end(self, slot):
        R, k = self._inflight.pop(slot)
        ids = np.empty((max(R, 1), max(k, 1)), np.uint64)
        ds = np.empty((max(R, 1), max(k, 1)), np.float32)
        cnt = np.zeros(max(R, 1), np.uint32)
        self._check(self.lib.fvh_hybrid_search_sharded_end(self.h, slot, _ptr(ids, u64p), _ptr(ds, f32p), _ptr(cnt, u32p)))
        return SearchResults(ids[:R], ds[:R], cnt[:R])

    def delete(self, id, now=0.0):
        self._check(self.lib.fvh_hybrid_delete(self.h, int(id), float(now)))

    def vacuum(self):
        """Physically drop soft-deleted vectors from both indexes (src/hybrid/core.rs:989-1012)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.fvh_hybrid_vacuum(self.h, C.byref(a), C.byref(b)))
        return {"hnsw_removed": a.value, "ivf_removed": b.value, "total_removed": a.value + b.value}

    def retrain_historical(self, n_clusters, n_probe=None, train_size=10000, max_iterations=25, seed=0):
        """IVFIndex::retrain of the historical index (no counterpart in the reference, whose maintenance scheduler only
        simulates one, src/hybrid/maintenance.rs:509-533): the way from the default 3 clusters to a partition that
        suits the data.  Refused while a batch begun with search_dev_begin is uncollected, and once sharded."""
        out = np.zeros(4, np.uint64)
        n_probe = int(self.n_probe if n_probe is None else n_probe)
        rc = self.lib.fvh_hybrid_retrain_historical(self.h, int(n_clusters), n_probe, int(train_size),
                                                    int(max_iterations), int(seed), _ptr(out, u64p))
        ivf = self.lib.fvh_hybrid_ivf(self.h)
        self.n_clusters, self.n_probe = int(self.lib.fvh_ivf_n_clusters(ivf)), int(self.lib.fvh_ivf_n_probe(ivf))
        self._check(rc)
        return dict(old_clusters=int(out[0]), new_clusters=int(out[1]), vectors_reassigned=int(out[2]), converged=bool(out[3]))

    def from_parts(self, ids, timestamps, recent_count, historical_count, ivf_trained):
        """HybridIndex::from_parts (src/hybrid/core.rs:857-877): adopt hnsw() / ivf() as restored by the caller."""
        ids = np.ascontiguousarray(ids, np.uint64)
        ts = np.ascontiguousarray(timestamps, np.float64)
        self._check(self.lib.fvh_hybrid_from_parts(self.h, _ptr(ids, u64p), _ptr(ts, f64p), ids.size, int(recent_count),
                                                   int(historical_count), int(bool(ivf_trained))))

    def export_timestamps(self):
        n = int(self.lib.fvh_hybrid_timestamp_count(self.h))
        ids, ts = np.empty(n, np.uint64), np.empty(n, np.float64)
        self.lib.fvh_hybrid_export_timestamps(self.h, _ptr(ids, u64p), _ptr(ts, f64p))
        return ids, ts

    def migrate_with_threshold(self, threshold, now):
        return int(self.lib.fvh_hybrid_migrate(self.h, float(threshold), float(now)))

    def set_resident_migration(self, on):
        """Where a migration's rows come from: True (default) = the graph's row store in HBM (the due ids go down as
        store row indices), False = the host copy, uploaded.  Same lists either way."""
        self.lib.fvh_hybrid_set_resident_migration(self.h, int(bool(on)))

    def migration_info(self):
        """The last migration that had rows to copy: path ("resident" / "host" / None) and its figures
        (fvdb_maintenance_info_t; the host path reports rows and host_bytes only)."""
        m = _capi.MaintenanceInfo()
        path = self.lib.fvh_hybrid_migration_info(self.h, C.byref(m))
        out = {name: getattr(m, name) for name, _ in m._fields_}
        out["path"] = {1: "resident", 2: "host"}.get(path)
        out["resident"] = path == 1
        return out

    def get_vectors(self, ids):
        """Vectors of `ids` (includeVectors, bindings/node/src/session.rs:266-281): the recent part answers first, the
        historical part (one device gather) for the rest.  Returns (rows [n x d] f32, found [n] bool)."""
        dim = int(self.lib.fvh_hnsw_dimension(self.lib.fvh_hybrid_hnsw(self.h))) or \
            int(self.lib.fvh_ivf_dimension(self.lib.fvh_hybrid_ivf(self.h)))
        return _get_vectors(self, self.lib.fvh_hybrid_get_vectors, ids, dim)

    def recent_count(self):
        return int(self.lib.fvh_hybrid_recent_count(self.h))

    def historical_count(self):
        return int(self.lib.fvh_hybrid_historical_count(self.h))

    def hnsw(self):
        return HNSWIndex(self.ctx_hnsw, _handle=self.lib.fvh_hybrid_hnsw(self.h))

    def store_bytes(self):
        """HBM the recent part's vectors occupy (HNSWIndex.store_bytes)."""
        return self.hnsw().store_bytes()

    def ivf_device_stage_times(self):
        return self.ivf().stage_times()

    def ivf_device_last_stats(self):
        return self.ivf().last_stats()

    def ivf(self):
        return IVFIndex(self.ctx, n_clusters=self.n_clusters, n_probe=self.n_probe, _handle=self.lib.fvh_hybrid_ivf(self.h))
