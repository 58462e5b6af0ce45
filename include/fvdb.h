/* fvdb.h — C ABI of the MI355X-native distance/top-k engine for fabstir-vectordb's
 * hybrid HNSW/IVF hot path.
 *
 * The reference (Rust) has NO FFI seam for distance computation: the L2 loops are called
 * directly (src/ivf/core.rs:351,378,424,650,671; src/hnsw/core.rs:279,434,487,515,573,605,611).
 * This header DEFINES the seam exactly at those call sites; each entry point cites the
 * reference code it replaces.  A Rust host binds it with a plain `extern "C"` block
 * (see INTEGRATION.md); this repo's own host code (C++, fabstir-vectordb_amd/host) and the
 * test harness (Python ctypes) use the same symbols.
 *
 * Conventions
 *  - plain pointers + sizes, row-major, no strides; caller owns host buffers for the
 *    duration of a call; the library owns device memory behind opaque handles.
 *  - `*_dev` variants take DEVICE pointers (HBM-resident inputs/outputs) and only enqueue
 *    work on the context's stream (call fvdb_ctx_synchronize or use the stream).
 *  - every call returns an fvdb_status; nothing throws or aborts across the boundary.
 *    Fewer than k hits is NOT an error (reference returns a short list:
 *    tests/ivf/core.rs:385-398, tests/hnsw/core.rs:300-316): see out_counts.
 *  - distances are the reference's arithmetic bit for bit: sqrt(sum_i (a_i-b_i)^2), f32,
 *    summed left to right, no FMA (src/core/vector_ops.rs:51-57).
 *  - ordering: ascending distance; exact ties keep scan order (probe rank, then position
 *    in the list) = what the reference's stable sort gives (src/ivf/core.rs:655,677).
 *  - threading (reference: searches hold a tokio RwLock READ guard, bindings/node/src/session.rs:253,
 *    src/hybrid/core.rs:457,466 — many at once; inserts/deletes hold the write guard):
 *      * the blocking host-pointer searches (fvdb_ivf_search, fvdb_ivf_search_all, fvdb_ivf_coarse) may be
 *        called on ONE index from any number of host threads at once: each call leases a private scratch
 *        set and stream inside the library and returns it when done;
 *      * the `*_slot` entry points may be called concurrently for DIFFERENT slots (each slot = one scratch
 *        set; the caller supplies the stream through `on`); two calls naming the same slot must use the same
 *        stream and are then ordered by it;
 *      * the stream-ordered `*_dev` entry points without a slot use set 0 on the index's own stream;
 *      * a search never modifies the index object.  Mutations (set_centroids, train, add*, set_deleted,
 *        clear, reserve, graph_upload, store_append) need external exclusion against searches and each other,
 *        as the reference's write guard provides.
 */
#ifndef FVDB_H
#define FVDB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum fvdb_status {
  FVDB_OK = 0,
  FVDB_E_NOT_TRAINED = 1,   /* IVFError::NotTrained            src/ivf/core.rs:16 */
  FVDB_E_DUPLICATE = 2,     /* IVFError/HNSWError::DuplicateVector (raised by host code) */
  FVDB_E_DIM = 3,           /* DimensionMismatch                src/ivf/core.rs:22 */
  FVDB_E_INSUFFICIENT = 4,  /* InsufficientTrainingData         src/ivf/core.rs:25 */
  FVDB_E_INCONSISTENT = 5,  /* InconsistentDimensions           src/ivf/core.rs:28 */
  FVDB_E_INVALID = 6,       /* InvalidConfig / bad argument     src/ivf/core.rs:31 */
  FVDB_E_NOT_FOUND = 7,     /* VectorNotFound                   src/ivf/core.rs:37 */
  FVDB_E_NOT_INITIALIZED = 8, /* HybridError::NotInitialized    src/hybrid/core.rs */
  FVDB_E_NONFINITE = 9,     /* NaN/Inf input (reference panics: partial_cmp().unwrap()) */
  FVDB_E_HIP = 10,          /* HIP runtime error (message via fvdb_last_error) */
  FVDB_E_OOM = 11,          /* device or host allocation failed */
  FVDB_E_UNSUPPORTED = 12,  /* k above the compiled limit of the entry point, or a shape it does not serve */
  FVDB_E_RCCL = 13          /* RCCL missing or a collective failed (message via fvdb_last_error) */
} fvdb_status;

/* Largest k (and nprobe) served by the in-kernel wavefront top-k (64 lanes x 4 registers).  It is the limit of that
 * register path only: an IVF search with a larger k (fvdb_ivf_search_wide*) or with more than this many lists probed
 * (any IVF search entry point) goes through the wide selection below, and its centroids are ranked by a full sort. */
#define FVDB_MAX_K 256u
/* Largest k served by the wide selection of the IVF list scan (fvdb_ivf_search_wide*): the distances of the probed
 * rows go through an arena in HBM and the k best are selected and sorted in LDS.  Equal to the traversal's ef limit. */
#define FVDB_MAX_K_WIDE 4096u
/* Row id meaning "no row" in padded outputs / candidate lists. */
#define FVDB_NO_ROW UINT32_MAX
#define FVDB_NO_ID UINT64_MAX

typedef struct fvdb_ctx fvdb_ctx;     /* one GPU + one HIP stream + scratch arenas */
typedef struct fvdb_ivf fvdb_ivf;     /* IVF-flat index resident in HBM (centroids + paged lists) */
typedef struct fvdb_store fvdb_store; /* row-major vector store for gathered candidate scoring */

/* ---- context ------------------------------------------------------------------------ */
int fvdb_ctx_create(int device, fvdb_ctx** out);
void fvdb_ctx_destroy(fvdb_ctx* ctx);
int fvdb_ctx_synchronize(fvdb_ctx* ctx);
int fvdb_device_synchronize(fvdb_ctx* ctx); /* every stream of ctx's device (hipDeviceSynchronize) */
int fvdb_ctx_device(fvdb_ctx* ctx); /* the device ordinal the context was created on */
/* Batches in flight run on streams of their own; the HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues
 * (default 4), and kernels of streams sharing a queue run one after the other.  fvdb_ctx_create asks for 16 unless the host
 * application set the variable itself — which only works if HIP has not been initialised in the process yet.
 * hw_queues_source: 1 = the host application's setting, 2 = set by this library, 3 = could NOT be applied (HIP was already
 * up; hw_queues then reports the runtime's default and a warning went to stderr: expect ~35 % less overlap). */
typedef struct fvdb_ctx_info_t {
  int device, compute_units, hw_queues, hw_queues_source;
} fvdb_ctx_info_t;
int fvdb_ctx_info(fvdb_ctx* ctx, fvdb_ctx_info_t* out);
void* fvdb_ctx_stream(fvdb_ctx* ctx);          /* hipStream_t, for callers that interleave work */
const char* fvdb_last_error(fvdb_ctx* ctx);    /* message of the last failing call on ctx */
const char* fvdb_version(void);
/* Device memory helpers so a host without a HIP binding can keep inputs resident in HBM. */
int fvdb_dev_alloc(fvdb_ctx* ctx, size_t bytes, void** out);
int fvdb_dev_free(fvdb_ctx* ctx, void* p);
int fvdb_dev_upload(fvdb_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int fvdb_dev_download(fvdb_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* Pieces for keeping more than one batch in flight: pinned host memory, a copy that does not wait, and events
 * recorded on a context's stream (fvdb_event_wait blocks the host until the work recorded before it is done). */
int fvdb_host_alloc(fvdb_ctx* ctx, size_t bytes, void** out);
void fvdb_host_free(fvdb_ctx* ctx, void* p);
int fvdb_dev_download_async(fvdb_ctx* ctx, void* dst_pinned, const void* src_dev, size_t bytes);
/* device to device on ctx's stream, without waiting: the source must stay unchanged until the stream has passed it */
int fvdb_dev_copy_async(fvdb_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);
/* The host mirror's hybrid begin/end pair (HybridIndex::search_dev_begin / search_dev_end, fvh_hybrid_search_dev_begin /
 * _end) is built from these.  Timing rule of that pair: the graph walk of a batch is enqueued by its begin; its IVF part
 * may be enqueued later — by the NEXT begin, which then runs one IVF chain for both batches (their queries copied side
 * by side with fvdb_dev_copy_async), or by the batch's own end.  Results and error codes are what they would be had
 * every chain been enqueued at once; the query buffer must stay valid and unchanged until end, as ever. */
typedef struct fvdb_event fvdb_event;
int fvdb_event_create(fvdb_ctx* ctx, fvdb_event** out);
void fvdb_event_destroy(fvdb_event* e);
int fvdb_event_record(fvdb_ctx* ctx, fvdb_event* e);
int fvdb_event_wait(fvdb_ctx* ctx, fvdb_event* e);
/* Stream-ordered timing of the region between the two calls (HIP events on ctx's stream). */
int fvdb_timer_start(fvdb_ctx* ctx);
int fvdb_timer_stop_ms(fvdb_ctx* ctx, float* out_ms);
/* Per-stage HIP-event timing of searches on this context.  on = 1: each search synchronises the
 * stream and accumulates its stage times; on = 2: events are only recorded, the caller folds them
 * in with fvdb_ivf_profile_collect() after its own synchronisation point (no extra sync). */
int fvdb_ctx_set_profiling(fvdb_ctx* ctx, int on);

/* ---- similarity utilities ------------------------------------------------------------
 * dot_product_scalar / cosine_similarity_scalar / batch_cosine_similarity
 * (src/core/vector_ops.rs:8-10,35-49; Embedding::cosine_similarity src/core/types.rs:79-103):
 * B queries x n rows -> out[B x n], sequential f32 folds (bit-identical to the reference).
 * No index calls these in the reference; they are part of its public vector_ops surface. */
int fvdb_dot_products(fvdb_ctx* ctx, const float* q, uint32_t B, const float* x, uint64_t n, uint32_t d, float* out);
int fvdb_cosine_similarities(fvdb_ctx* ctx, const float* q, uint32_t B, const float* x, uint64_t n, uint32_t d,
                             float* out);

/* ---- IVF-flat ------------------------------------------------------------------------
 * Replaces IVFIndex's arithmetic: find_nearest_centroid (src/ivf/core.rs:373-386), the
 * coarse ranking + list scan + selection of search_with_config (:626-681) and
 * batch_search (src/ivf/operations.rs:132-145).  Row ids are caller-chosen u64.
 */
int fvdb_ivf_create(fvdb_ctx* ctx, uint32_t d, uint32_t nlist, fvdb_ivf** out);
/* Row storage of the inverted lists.  FVDB_F16 (config C5) keeps rows as IEEE fp16 (rounded to nearest
 * even at insert) and widens them to f32 in registers; centroids, queries, the f32 fold and the ordering
 * are unchanged, so results equal the reference algorithm run on the fp16-rounded rows.  A finite row value beyond
 * the fp16 range (|x| >= 65520) is stored as +-Inf and searched as such: the row's distance is +Inf, a result like any
 * other, ordered by scan position, and the row reads back as +-Inf. */
typedef enum fvdb_dtype { FVDB_F32 = 0, FVDB_F16 = 1 } fvdb_dtype;
int fvdb_ivf_create_ex(fvdb_ctx* ctx, uint32_t d, uint32_t nlist, int row_dtype, fvdb_ivf** out);
void fvdb_ivf_destroy(fvdb_ivf* ivf);
/* set_trained (src/ivf/core.rs:509-520): install nlist x d centroids (host), empty the lists. */
int fvdb_ivf_set_centroids(fvdb_ivf* ivf, const float* centroids);
int fvdb_ivf_get_centroids(fvdb_ivf* ivf, float* out /* nlist x d */);
/* k-means++ + Lloyd on the GPU (src/ivf/core.rs:240-429).  Assignment = the coarse kernel;
 * centroid update and error are summed in data order like the reference.  The seeding
 * draws come from SplitMix64(seed) (the reference's StdRng stream is unpinned). */
typedef struct fvdb_train_result {
  uint32_t iterations;
  uint32_t converged;
  float initial_error;
  float final_error;
} fvdb_train_result;
int fvdb_ivf_train(fvdb_ivf* ivf, const float* x, uint64_t n, uint32_t max_iterations, uint64_t seed,
                   fvdb_train_result* out);
/* Batched find_nearest_centroid: strict '<', lowest cluster id wins ties. */
int fvdb_ivf_assign(fvdb_ivf* ivf, const float* x, uint64_t n, uint32_t* out_cluster);
/* insert (src/ivf/core.rs:431-455) for n rows: assign on the GPU, append to the lists in row
 * order.  out_cluster/out_pos (optional) receive each row's list and position in it. */
int fvdb_ivf_add(fvdb_ivf* ivf, const float* x, const uint64_t* ids, uint64_t n, uint32_t* out_cluster,
                 uint32_t* out_pos);
/* Append rows whose cluster is already known (load path, shard placement). */
int fvdb_ivf_add_assigned(fvdb_ivf* ivf, const float* x, const uint64_t* ids, uint64_t n,
                          const uint32_t* cluster, uint32_t* out_pos);
/* Soft delete (src/ivf/operations.rs:569-591 + the skip at src/ivf/core.rs:666-669). */
int fvdb_ivf_set_deleted(fvdb_ivf* ivf, const uint32_t* cluster, const uint32_t* pos, uint64_t n, int deleted);
int fvdb_ivf_list_sizes(fvdb_ivf* ivf, uint64_t* out /* nlist */);
uint64_t fvdb_ivf_total_rows(fvdb_ivf* ivf);
/* Copy list `list` back to the host in list-position order: rows [len x d] as f32 (fp16 rows widened exactly), ids
 * [len], live [len] (0 = soft-deleted).  Any output may be NULL.  len = fvdb_ivf_list_sizes()[list].  Replaces the
 * walk over `InvertedList.vectors` of the reference's save path (src/hybrid/persistence.rs:289-311). */
int fvdb_ivf_list_export(fvdb_ivf* ivf, uint32_t list, float* rows, uint64_t* ids, uint8_t* live);
int fvdb_ivf_reserve(fvdb_ivf* ivf, uint64_t n_rows);

/* ---- Maintenance that re-partitions an index without its rows leaving HBM -------------------------------------------
 * (src/ivf/operations.rs:148-260 retrain / add_clusters / optimize_clusters, :625-645 vacuum).  The SEQUENCE ORDER of
 * an index is: lists in ascending cluster id, each list in list-position order (the order of fvdb_ivf_list_export).
 * Every row keeps its place in that order inside the list it moves to, in every representation the pool keeps; norms
 * and live bits travel with the row (a soft-deleted row stays soft-deleted).  The job builds a second pool beside the
 * first and swaps: FVDB_E_OOM leaves the index as it was.  Destination lists are ranked with one LDS counter per list:
 * up to 16384 lists, FVDB_E_UNSUPPORTED above.  An index with global list sizes set (a shard) is refused with
 * FVDB_E_UNSUPPORTED.  Only ids, cluster numbers, positions and the list tables cross the host link. */
typedef struct fvdb_maintenance_info_t {
  uint64_t rows_in, rows_out;  /* rows of the source sequence; rows in the lists afterwards */
  uint64_t host_bytes;         /* copied to or from the host by the job (ids, clusters, positions, list tables) */
  uint64_t move_bytes;         /* read + written in HBM by the move stage */
  float ms_gather, ms_train, ms_assign, ms_ranks, ms_move;  /* device time per stage, summed over the job's calls */
  float ms_total;
} fvdb_maintenance_info_t;
/* Drop every row whose live bit is clear; survivors keep their order.  removed (optional) = rows dropped.  out_ids
 * (optional, room for fvdb_ivf_total_rows() entries) receives the surviving ids in sequence order: with
 * fvdb_ivf_list_sizes that is every survivor's (list, position). */
int fvdb_ivf_compact(fvdb_ivf* ivf, uint64_t* removed, uint64_t* out_ids);
/* fvdb_ivf_train of dst on src's rows in sequence order (soft-deleted rows included, fp16 rows widened exactly), with
 * no host copy: the result is that of fvdb_ivf_train given the exported rows, bit for bit.  dst and src share d, row
 * dtype and device and are different objects; src is not modified; dst's lists are emptied like fvdb_ivf_train does
 * and dst takes over src's coarse and scan mode. */
int fvdb_ivf_train_from(fvdb_ivf* dst, fvdb_ivf* src, uint32_t max_iterations, uint64_t seed, fvdb_train_result* out);
/* Nearest centroid of dst for each of src's rows in sequence order.  out_cluster / out_ids (optional, host,
 * fvdb_ivf_total_rows(src) entries each): the cluster and the id of every row.  The ranking stays on the device for
 * fvdb_ivf_refill_from. */
int fvdb_ivf_assign_from(fvdb_ivf* dst, fvdb_ivf* src, uint32_t* out_cluster, uint64_t* out_ids);
/* Move the first n_rows rows of src's sequence into dst's lists (which must be empty), each into the list
 * fvdb_ivf_assign_from chose; the rest are left out (the host mirror cuts the sequence where the reference's re-insert
 * stops at a duplicate).  out_pos (optional, host, n_rows entries): each row's position in its list.  src is unchanged. */
int fvdb_ivf_refill_from(fvdb_ivf* dst, fvdb_ivf* src, uint64_t n_rows, uint32_t* out_pos);
/* Figures of the last maintenance job on this index (compact; train_from + assign_from + refill_from as dst). */
int fvdb_ivf_maintenance_info(fvdb_ivf* ivf, fvdb_maintenance_info_t* out);

/* ---- Rows by location ------------------------------------------------------------------------------------------------
 * One device gather serves three things: reading a row back (IVFIndex::get_vector_by_id, src/ivf/core.rs:553-562),
 * returning the hits' vectors (includeVectors, bindings/node/src/session.rs:266-281) and the migration of rows from
 * the graph's row store into the lists without a trip through the host (src/hybrid/core.rs:600-649). */
/* Rows of the inverted lists by location (list, position), as fvdb_ivf_set_deleted names them.  out: n x d f32
 * (fp16 rows widened exactly).  A soft-deleted row is returned like any other (src/ivf/core.rs:553-562 does not look
 * at the deleted set).  FVDB_E_NOT_FOUND if a location is not a row; nothing is written then.  Reads only: does not
 * bump the mutation counter, leaves masks fresh.  Any number of host threads may call it, beside searches in any
 * slot (each call leases a scratch set and its stream, like fvdb_ivf_search); not beside a mutation. */
int fvdb_ivf_get_rows(fvdb_ivf* ivf, const uint32_t* cluster, const uint32_t* pos, uint64_t n, float* out_rows /*host*/);
/* Same, enqueued on `on`'s stream (NULL = the index's) into device memory; no synchronisation. */
int fvdb_ivf_get_rows_dev(fvdb_ivf* ivf, fvdb_ctx* on, const uint32_t* cluster, const uint32_t* pos, uint64_t n,
                          float* out_rows_dev);
/* fvdb_ivf_assign / fvdb_ivf_add_assigned with the rows taken from a row store in HBM instead of the host (the
 * staging vector of HybridIndex::migrate, src/hybrid/core.rs:619-640, never exists): the result is, bit for bit and
 * in every representation the pool keeps (blocked rows, fp16 mirror, row-major copy, norms, largest norm), that of
 * the host form given fvdb_store_get() of those rows.  Store and index share d (FVDB_E_DIM) and the device
 * (FVDB_E_INVALID); a row index >= fvdb_store_rows() is FVDB_E_NOT_FOUND before anything is changed.  The rows are
 * not checked for NaN / Inf again: fvdb_store_append did.  fvdb_ivf_maintenance_info afterwards reports the pair as
 * one job: rows_in = rows_out = n, host_bytes (row indices, clusters, ids, slots: at most 32 n), ms_gather,
 * ms_assign, ms_move. */
int fvdb_ivf_assign_from_store(fvdb_ivf* ivf, fvdb_store* store, const uint32_t* rows, uint64_t n, uint32_t* out_cluster);
int fvdb_ivf_add_assigned_from_store(fvdb_ivf* ivf, fvdb_store* store, const uint32_t* rows, const uint64_t* ids,
                                     uint64_t n, const uint32_t* cluster, uint32_t* out_pos);
int fvdb_ivf_clear(fvdb_ivf* ivf);   /* empties the lists, keeps centroids (hybrid initialize :278-287) */
/* Multi-GPU: sizes of ALL lists of the logical index (this rank may own a subset), so the
 * tie-break position `seq` is identical on every rank.  Default = local sizes. */
int fvdb_ivf_set_global_list_sizes(fvdb_ivf* ivf, const uint64_t* sizes /* nlist */);

/* search_with_config for B queries.  out_ids/out_dist are B x k (unused tail = FVDB_NO_ID /
 * +inf), out_counts[B] the number of hits.  nprobe > nlist probes every list.  Any nprobe >= 1 is served: with
 * min(nprobe, nlist) > FVDB_MAX_K the centroid table is ranked whole (one sort per query, nlist <= 16384, otherwise
 * FVDB_E_UNSUPPORTED) and the lists go through the wide selection, which then also takes any k <= FVDB_MAX_K_WIDE.  The
 * same holds for every IVF search entry point below, the coarse step alone and the masked forms included; not for an
 * index holding a shard of a larger one (fvdb_ivf_set_global_list_sizes) nor for fvdb_ivf_search_sharded_begin: a shard
 * is served by fvdb_ivf_search_shard_wide_dev_slot and the sharded search by fvdb_ivf_search_sharded_wide_begin. */
int fvdb_ivf_search(fvdb_ivf* ivf, const float* q, uint32_t B, uint32_t k, uint32_t nprobe, uint64_t* out_ids,
                    float* out_dist, uint32_t* out_counts);
/* Same with device pointers.  q is B x d row-major f32 in HBM.  out_keys (optional, B x k u64)
 * receives (distance bits << 32 | seq): the total order used for selection; unique per row, so
 * per-GPU partial results can be merged exactly (fvdb_merge_keys_dev). */
int fvdb_ivf_search_dev(fvdb_ivf* ivf, const float* q_dev, uint32_t B, uint32_t k, uint32_t nprobe,
                        uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev,
                        uint64_t* out_keys_dev);
/* Exhaustive scan of every list (exact k-NN; ground truth for recall, and the a7/a8 kernel
 * with no coarse step). */
int fvdb_ivf_search_all(fvdb_ivf* ivf, const float* q, uint32_t B, uint32_t k, uint64_t* out_ids,
                        float* out_dist, uint32_t* out_counts);
/* Same search on the stream of context `on` (NULL = the index's own) with the slot-th (0..15) set of per-search
 * scratch: searches in different slots and on different contexts may be in flight together.  The index must not be
 * modified while any is.  Stage timing (profiling) is only kept for searches on the index's own context. */
int fvdb_ivf_search_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t k,
                             uint32_t nprobe, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev,
                             uint64_t* out_keys_dev);
/* The two stages separately (multi-GPU: each rank ranks the centroids for its own queries only, the probe lists
 * travel with the queries, and every rank scans its lists for all of them).  probes: B x min(nprobe, n_clusters)
 * cluster ids in probe order, device memory. */
int fvdb_ivf_coarse_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t nprobe,
                             uint32_t* out_probes_dev);
int fvdb_ivf_search_probes_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, const float* q_dev,
                                    const uint32_t* probes_dev, uint32_t B, uint32_t k, uint32_t nprobe,
                                    uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev,
                                    uint64_t* out_keys_dev);
int fvdb_ivf_search_all_dev(fvdb_ivf* ivf, const float* q_dev, uint32_t B, uint32_t k, uint64_t* out_ids_dev,
                            float* out_dist_dev, uint32_t* out_counts_dev);
/* Coarse step alone (src/ivf/core.rs:645-656): the nprobe nearest clusters per query in
 * probe order, and their distances. */
int fvdb_ivf_coarse(fvdb_ivf* ivf, const float* q, uint32_t B, uint32_t nprobe, uint32_t* out_clusters,
                    float* out_dist);

/* Coarse-stage implementation.  FVDB_COARSE_AUTO (default): the query x centroid contraction runs on the
 * matrix cores (MFMA) to propose 64 candidate clusters per query, whose distances are then recomputed with
 * the reference's sequential f32 arithmetic; a rounding-error bound proves the proposal contains the true
 * top nprobe, otherwise that query is ranked exactly over the whole table.  Results are identical to
 * FVDB_COARSE_EXACT (every centroid scored with the reference's arithmetic) by construction.  AUTO applies
 * when padded d % 16 == 0, nprobe <= 48 and n_clusters >= 64; other shapes use the exact scan. */
#define FVDB_COARSE_AUTO 0
#define FVDB_COARSE_EXACT 1
int fvdb_ivf_set_coarse_mode(fvdb_ivf* ivf, int mode);
/* Queries (since the centroids were installed) whose proposal could not be proven and were ranked exactly. */
int fvdb_ivf_coarse_fallbacks(fvdb_ivf* ivf, uint64_t* out);

/* Inverted-list scan implementation.  FVDB_SCAN_AUTO (default): fp16 MFMA evaluates |x|^2 - 2 x.q for every
 * (row, query) of the probed lists and discards the rows that provably cannot reach the top k (threshold from an
 * exact scan of the query's nearest lists plus a rounding-error bound); the few survivors are scored with the
 * reference's sequential f32 fold and selected by (distance, scan position).  A query whose k-th result is not
 * strictly below its threshold is rescanned exactly.  Results are identical to FVDB_SCAN_EXACT (every probed
 * row scored with the reference's arithmetic) by construction.  AUTO also watches its own hit rate: when more than
 * one query in eight of the recent batches needed the exact rescan (data the filter cannot separate), the following
 * 64 batches (doubling up to 4096 while that stays so) use the exact scan.  AUTO applies when padded d % 16 == 0,
 * k <= 26, nprobe <= 256 and the batch has 32..16384 queries; other shapes use the exact scan (more than 256 lists
 * probed: the wide selection, whatever the mode). */
#define FVDB_SCAN_AUTO 0
#define FVDB_SCAN_EXACT 1
#define FVDB_SCAN_FILTER 2 /* the matrix-core filter for every batch it can serve (AUTO without the hit-rate back-off) */
int fvdb_ivf_set_scan_mode(fvdb_ivf* ivf, int mode);
/* Queries (since the centroids were installed) that were rescanned exactly. */
int fvdb_ivf_scan_fallbacks(fvdb_ivf* ivf, uint64_t* out);
/* of those, by cause: [0] survivor buffer overflow, [1] more candidates than the select stage scores, [2] the k-th kept
 * distance not strictly below the bound of the unscored rows, [3] no usable threshold; and [4] (not a rescan) queries
 * whose survivors outgrew the buffer and were filtered a second time with a threshold taken from those survivors */
int fvdb_ivf_scan_fallback_reasons(fvdb_ivf* ivf, uint64_t* out5);

/* Diagnostic: rows per query that survived the matrix-core filter in the last (sub-)batch of B queries. */
int fvdb_ivf_scan_survivors(fvdb_ivf* ivf, uint32_t* out, uint32_t B);

/* Diagnostic: the survivors of one query of the last matrix-core (sub-)batch — probe rank, position in that list and
 * the matrix-core value v = |x|^2 - 2 x~.q~ — so that a test can hold v + |q|^2 against the reference's sum and the
 * error bound.  At most max_n entries are written. */
int fvdb_ivf_scan_survivor_dump(fvdb_ivf* ivf, uint32_t query, uint32_t max_n, uint32_t* rank, uint32_t* pos, float* v,
                                uint32_t* n_out);

/* Counters of the last search on this index (for roofline accounting). */
typedef struct fvdb_search_stats {
  uint64_t rows_scanned;      /* sum over queries of rows in probed lists (algorithmic) */
  uint64_t work_items;        /* (list segment, query group) items executed */
  uint64_t list_rows_touched; /* rows of the union of probed lists (physical lower bound) */
} fvdb_search_stats;
int fvdb_ivf_last_stats(fvdb_ivf* ivf, fvdb_search_stats* out);
/* With profiling on: ms[8] = coarse scan, coarse merge, plan, fine scan, fine merge, [5] the matrix-core filter
 * kernel alone (part of fine scan; 0 on the exact path), [6..7] reserved (0) — summed over the searches since
 * the last call; returns how many searches (sub-batches) were accumulated. */
uint64_t fvdb_ivf_stage_times(fvdb_ivf* ivf, float* ms_out);
int fvdb_ivf_profile_collect(fvdb_ivf* ivf);  /* profiling mode 2: fold the last search's events in */

/* ---- merge ---------------------------------------------------------------------------
 * G-way merge of per-shard partial top-k by key (a4/a12 semantics: ascending, keep k).
 * keys/ids: G x B x k (device).  Exact because keys are unique. */
int fvdb_merge_keys_dev(fvdb_ctx* ctx, const uint64_t* keys_dev, const uint64_t* ids_dev, uint32_t G, uint32_t B,
                        uint32_t k, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev);

/* The same merge for 1 <= k <= FVDB_MAX_K_WIDE (same layout, same outputs: tails from the count up are FVDB_NO_ID /
 * +inf, counts = min(k, valid entries)).  Needs what every search here writes: each partial list ascending by key with
 * its "no result" (~0) entries last, and keys unique across the lists.  An entry's place in the result is then its own
 * index plus the number of smaller keys in every other list, so nothing is sorted and nothing is staged on chip.  At
 * k <= FVDB_MAX_K it returns exactly what fvdb_merge_keys_dev returns. */
int fvdb_merge_keys_wide_dev(fvdb_ctx* ctx, const uint64_t* keys_dev, const uint64_t* ids_dev, uint32_t G, uint32_t B,
                             uint32_t k, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev);

/* ---- top-k / merge utilities -----------------------------------------------------------
 * The reference's public vector_ops helpers, batched: B independent rows per call, k <= FVDB_MAX_K.  Outputs are
 * B x k (unused tail = FVDB_NO_ID / 0), out_counts[B] the number of entries.  A NaN score is FVDB_E_NONFINITE in
 * the host-pointer forms (the reference panics in partial_cmp().unwrap()); the *_dev forms take device pointers,
 * run on ctx's stream and do not inspect their input.
 *  - fvdb_top_k_indices: top_k_indices (src/core/vector_ops.rs:12-22) — indices of the k largest scores, ties in
 *    index order (stable sort).
 *  - fvdb_top_k_indices_heap: top_k_indices_heap (:180-201) — BinaryHeap of size k with strict `>` replacement, then
 *    a stable descending sort of the heap's vector: the tie behaviour of that heap is reproduced exactly.
 *  - fvdb_streaming_top_k: StreamingTopK::add for every (id, score) of a row in order, then get_results()
 *    (:204-263).  Heap order is the (reversed score, id) tuple order; u64 ids stand for VectorIds (a host that
 *    needs the reference's tie order passes the first 8 bytes of the VectorId, big-endian).
 *  - fvdb_merge_search_results: merge_search_results (:24-32) + SearchResult::deduplicate (src/core/types.rs:206-223)
 *    — per row the concatenated result sets (id FVDB_NO_ID = padding); per id the smallest distance is kept (the
 *    earliest entry on a tie), survivors ascending by distance, first k.  Where the reference's order among equal
 *    distances comes out of HashMap iteration, first appearance of the id decides. */
int fvdb_top_k_indices(fvdb_ctx* ctx, const float* scores /* B x n */, uint32_t B, uint64_t n, uint32_t k,
                       uint64_t* out_idx, uint32_t* out_counts);
int fvdb_top_k_indices_heap(fvdb_ctx* ctx, const float* scores, uint32_t B, uint64_t n, uint32_t k, uint64_t* out_idx,
                            uint32_t* out_counts);
int fvdb_top_k_indices_dev(fvdb_ctx* ctx, const float* scores_dev, uint32_t B, uint64_t n, uint32_t k, int heap,
                           uint64_t* out_idx_dev, uint32_t* out_counts_dev);
int fvdb_streaming_top_k(fvdb_ctx* ctx, const uint64_t* ids, const float* scores, uint32_t B, uint64_t n, uint32_t k,
                         uint64_t* out_ids, float* out_scores, uint32_t* out_counts);
int fvdb_streaming_top_k_dev(fvdb_ctx* ctx, const uint64_t* ids_dev, const float* scores_dev, uint32_t B, uint64_t n,
                             uint32_t k, uint64_t* out_ids_dev, float* out_scores_dev, uint32_t* out_counts_dev);
int fvdb_merge_search_results(fvdb_ctx* ctx, const uint64_t* ids, const float* dist, uint32_t B, uint64_t n, uint32_t k,
                              uint64_t* out_ids, float* out_dist, uint32_t* out_counts);
int fvdb_merge_search_results_dev(fvdb_ctx* ctx, const uint64_t* ids_dev, const float* dist_dev, uint32_t B, uint64_t n,
                                  uint32_t k, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev);

/* ---- candidate scoring (HNSW) --------------------------------------------------------
 * Replaces euclidean_distance at src/hnsw/core.rs:279,434,487,515 (search_layer) and
 * :573,605,611 (prune): the host walks the graph, each hop's candidate batch is scored here.
 */
int fvdb_store_create(fvdb_ctx* ctx, uint32_t d, uint64_t capacity_rows, fvdb_store** out); /* FVDB_F32 rows */
/* The same with the row element chosen.  An FVDB_F16 store keeps its rows as IEEE fp16, the rule of fvdb_ivf_create_ex:
 * fvdb_store_append rounds each value to nearest even on the device (a value whose rounding overflows is stored as
 * +-Inf; a caller that wants such rows refused checks before it appends) and pads the row with zeros to the same
 * multiple of four elements as an f32 store, fvdb_store_get widens.  Every entry point that takes a store, or a graph
 * built on one, serves either element: fvdb_score_candidates, fvdb_scorer_* (set_query_rows widens the stored rows
 * into the f32 queries), fvdb_graph_* (search, masked search, scan_allowed, insert_linked, edge distances, vacuum),
 * fvdb_ivf_assign_from_store and fvdb_ivf_add_assigned_from_store (the gather widens, so the lists may be of either
 * dtype).  Queries are f32 everywhere.  Widening fp16 is exact and the f32 arithmetic is the f32 store's, so every
 * distance is, bit for bit, what an f32 store holding the rounded values gives. */
int fvdb_store_create_ex(fvdb_ctx* ctx, uint32_t d, uint64_t capacity_rows, int row_dtype, fvdb_store** out);
void fvdb_store_destroy(fvdb_store* s);
int fvdb_store_append(fvdb_store* s, const float* rows, uint64_t n, uint64_t* first_row);
uint64_t fvdb_store_rows(fvdb_store* s);
int fvdb_store_dtype(fvdb_store* s);      /* FVDB_F32 or FVDB_F16 */
uint64_t fvdb_store_bytes(fvdb_store* s); /* HBM held by the stored rows: rows x padded row bytes */
int fvdb_store_get(fvdb_store* s, uint64_t row, float* out /* d */);
/* One-shot: B queries (host), C candidate row indices per query (FVDB_NO_ROW = pad) -> B x C
 * distances (+inf for pads). */
int fvdb_score_candidates(fvdb_store* s, const float* q, uint32_t B, const uint32_t* cand, uint32_t C, float* out);
/* Hop loop: queries stay in HBM, candidates/distances travel through pinned host memory
 * mapped into the GPU (no memcpy calls): one launch + one stream sync per hop. */
typedef struct fvdb_scorer fvdb_scorer;
int fvdb_scorer_create(fvdb_store* s, uint32_t max_B, uint32_t max_C, fvdb_scorer** out);
void fvdb_scorer_destroy(fvdb_scorer* sc);
int fvdb_scorer_set_queries(fvdb_scorer* sc, const float* q, uint32_t B);      /* host rows */
int fvdb_scorer_set_query_rows(fvdb_scorer* sc, const uint32_t* rows, uint32_t B); /* queries = stored rows */
int fvdb_scorer_set_queries_dev(fvdb_scorer* sc, const float* q_dev, uint32_t B); /* B x d rows already in HBM */
uint32_t* fvdb_scorer_cand_buffer(fvdb_scorer* sc);   /* B x max_C, write candidates here */
const float* fvdb_scorer_dist_buffer(fvdb_scorer* sc); /* B x max_C, read distances here */
int fvdb_scorer_run(fvdb_scorer* sc, uint32_t B, uint32_t C); /* scores cand_buffer rows 0..B, columns 0..C; waits */
/* Each scorer owns a HIP stream: several scorers (one per host thread / query group) keep several
 * hops in flight.  launch enqueues the scoring of rows 0..B x columns 0..C, wait blocks until it is done. */
int fvdb_scorer_launch(fvdb_scorer* sc, uint32_t B, uint32_t C);
int fvdb_scorer_wait(fvdb_scorer* sc);

/* ---- device-resident graph traversal --------------------------------------------------------
 * Optional fast path for HNSWIndex::search (src/hnsw/core.rs:398-554): the adjacency lists are
 * mirrored in HBM and one wavefront per query runs the whole layered search in a single launch
 * (same heaps, same visiting order, same distance arithmetic => same results as the host walk that
 * uses fvdb_scorer_*).  Rows are the store's; node index = store row.
 */
typedef struct fvdb_graph fvdb_graph;
int fvdb_graph_create(fvdb_store* s, fvdb_graph** out);
void fvdb_graph_destroy(fvdb_graph* g);
/* Install a whole graph (restore, bulk build, vacuum): levels[n]; deleted[n] (0/1); slot_start[n_slots+1] / adj[]: CSR
 * over (node, layer) slots in node order, layer 0 first (n_slots = sum(level+1)); every list must hold <= 64 neighbours. */
int fvdb_graph_upload(fvdb_graph* g, uint32_t n, const uint32_t* levels, const uint8_t* deleted,
                      const uint32_t* slot_start, const uint32_t* adj, uint32_t entry_node);
int fvdb_graph_set_deleted(fvdb_graph* g, uint32_t node, int deleted);
/* B queries (device, B x d).  out_nodes/out_dist: B x k device buffers, out_counts/out_status: B.
 * status 1 = the query overflowed the on-chip candidate heap and must be searched through the host walk
 * instead (its count is 0). */
int fvdb_graph_search_dev(fvdb_graph* g, const float* q_dev, uint32_t B, uint32_t k, uint32_t ef,
                          uint32_t* out_nodes_dev, float* out_dist_dev, uint32_t* out_counts_dev,
                          uint32_t* out_status_dev);
/* Same on the stream of context `on` (NULL = the store's context), with the slot-th (0..15) set of per-batch
 * traversal state: searches in different slots and on different contexts may be in flight together. */
int fvdb_graph_search_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t k,
                               uint32_t ef, uint32_t* out_nodes_dev, float* out_dist_dev, uint32_t* out_counts_dev,
                               uint32_t* out_status_dev);
/* ---- device-resident graph construction --------------------------------------------------------
 * HNSWIndex::insert (src/hnsw/core.rs:226-378) with the graph resident in HBM: greedy descent, search_layer
 * (ef_construction), select_neighbors (:556-558), back-links and prune_neighbors_with_new_node (:588-624) run in one
 * workgroup per insert against the adjacency rows in HBM, strictly in insert order — the graph is the one the
 * reference's sequential loop builds.  Adjacency rows have a fixed stride per (node, layer), so every mutation —
 * this one, or a host-side insert patched in with fvdb_graph_set_lists — rewrites only the rows it touches.
 *
 * configure: the degree caps (max_connections, max_connections_layer_0; src/hnsw/core.rs:37-46) the row strides
 *   are sized for; before the first node.
 * append_nodes: store rows [first, first + n) become nodes with empty lists (levels[n]); first must equal the
 *   current node count (node index = store row).
 * insert_linked: links the appended, not yet linked nodes [first, first + n) in order.  mode 0 = choose,
 *   1 = one insert at a time, 2 = speculate a batch of searches against the frozen graph and commit in order
 *   (a speculated search is adopted only if it is provably the search the serial algorithm would run at its turn:
 *   the adjacency rows it expanded are unchanged, or what earlier inserts of the batch added to / dropped from them
 *   cannot alter its pops, its expansions or its result — DESIGN.md section 6a).  The result never depends on the
 *   mode.  Environment knobs for A/B runs only: FVDB_BUILD_MODE, FVDB_BUILD_K / FVDB_BUILD_KMAX (batch size),
 *   FVDB_BUILD_STRICT (1 = adopt only when no expanded row changed), FVDB_BUILD_SEQ_BELOW, FVDB_BUILD_EXACT_FIRST,
 *   FVDB_BUILD_DEBUG (per-call diagnostics on stderr).  *n_done < n with stats->needs_host = 1: node first + *n_done needs the host path (level >= 16, an
 *   on-chip heap overflow or a hashed visited set that filled); link it through fvdb_graph_set_lists / fvdb_graph_set_entry and call again.
 * set_lists: overwrite the lists of n_lists (node, layer) rows: offsets[n_lists + 1] into nbrs[].
 * set_entry: entry point + the number of nodes whose links are complete.
 * download: the adjacency in CSR form over (node, layer) slots in node order (slot_start[slots + 1], adj[adj_cap];
 *   either may be NULL), *n_edges = total.  upload_bytes: host -> device bytes of graph STRUCTURE moved so far. */
typedef struct fvdb_graph_insert_stats {
  uint32_t n_done, needs_host;
  uint32_t speculated_ok, searched_in_commit, commit_stops;  /* speculation: adopted / searched by the commit workgroup / early stops */
  uint32_t rounds, expanded, rows_scored, tie_restarts;      /* of the searches run by the commit workgroup; tie_restarts: of the speculated ones too */
  uint32_t launches;
} fvdb_graph_insert_stats;
int fvdb_graph_configure(fvdb_graph* g, uint32_t max_connections, uint32_t max_connections_layer_0);
int fvdb_graph_append_nodes(fvdb_graph* g, uint32_t first, uint32_t n, const uint32_t* levels);
int fvdb_graph_insert_linked(fvdb_graph* g, uint32_t first, uint32_t n, uint32_t ef_construction, int mode, uint32_t* n_done,
                             fvdb_graph_insert_stats* stats);
int fvdb_graph_set_lists(fvdb_graph* g, uint32_t n_lists, const uint32_t* nodes, const uint32_t* layers, const uint32_t* offsets,
                         const uint32_t* nbrs);
int fvdb_graph_set_entry(fvdb_graph* g, uint32_t entry_node, uint32_t n_linked);
int fvdb_graph_entry(fvdb_graph* g, uint32_t* entry_node, uint32_t* n_nodes);
int fvdb_graph_download(fvdb_graph* g, uint32_t* slot_start, uint32_t* adj, uint64_t adj_cap, uint64_t* n_edges);
uint64_t fvdb_graph_upload_bytes(fvdb_graph* g);
/* `visited` of the insert's searches (src/hnsw/core.rs:469-554, visited: HashSet<VectorId>) lives in LDS in one of two
 * forms.  A bitmap over every node index of the graph: one LDS read per test, n / 8 bytes — it fits beside the
 * search's other tables up to bitmap_max_nodes nodes (appended, not yet linked nodes count).  Or a hashed set of node
 * indices (open addressing, full keys: exact like the bitmap) whose size does not depend on the graph; a search that
 * meets more nodes than 3/4 of its slots gives up and that one insert takes the host path (needs_host), like an
 * insert whose `candidates` heap outgrows LDS.  The graph never depends on the form.
 * set_insert_visited: mode 0 = bitmap while the graph fits it, hashed beyond (default); 1 = bitmap only
 *   (insert_linked returns FVDB_E_UNSUPPORTED beyond its reach); 2 = hashed always.  table_slots: 0 = default (the
 *   largest power of two that leaves the `candidates` heap 2048 slots: 8192 at ef_construction 200), else a power of two
 *   in 256..32768.  Test hooks, read at every call: FVDB_BUILD_LDS_LIMIT (LDS budget in bytes),
 *   FVDB_BUILD_BITMAP_MAX_NODES (lowers the node count the bitmap serves).
 * insert_info: what insert_linked(ef_construction) would use for the graph as it stands — representation 1 bitmap,
 *   2 hashed, 0 neither fits (the call would return FVDB_E_UNSUPPORTED) — and, since the graph was created: inserts
 *   linked with the hashed set, inserts it handed to the host because it filled, and the number of entries it held at
 *   the end of a search_layer(ef_construction) (largest; count and sum for the mean). */
typedef struct fvdb_graph_insert_info_t {
  uint32_t mode;              /* the setting */
  uint32_t representation;
  uint32_t table_slots;       /* hashed: slots of the table; bitmap: 0 */
  uint32_t cand_cap;          /* slots of the restated `candidates` heap */
  uint32_t lds_bytes;         /* LDS of one insert workgroup */
  uint32_t bitmap_max_nodes;  /* the largest node count the bitmap serves at this ef_construction */
  uint32_t visited_peak;
  uint32_t reserved;
  uint64_t hashed_inserts, visited_overflows, visited_searches, visited_entries;
} fvdb_graph_insert_info_t;
int fvdb_graph_set_insert_visited(fvdb_graph* g, int mode, uint32_t table_slots);
int fvdb_graph_insert_info(fvdb_graph* g, uint32_t ef_construction, fvdb_graph_insert_info_t* out);
/* search_info: what fvdb_graph_search_dev* would run for B queries at ef on the graph as it stands (node count, row
 *   width and element), from the function the launch itself takes its plan from.  Allocates nothing, launches nothing;
 *   the environment hooks the launch reads are read here too.  Same refusals as the search (graph not uploaded, ef
 *   outside 1..4096, traversal state larger than LDS). */
#define FVDB_GRAPH_VISITED_BYTES 1u   /* `visited` of a query: one byte per node */
#define FVDB_GRAPH_VISITED_BITS 2u    /*                       one bit per node (atomicOr) */
#define FVDB_GRAPH_KERNEL_SORTED 1u   /* hnsw_search_fast_kernel: `nearest` a sorted register array, four queries per workgroup */
#define FVDB_GRAPH_KERNEL_HEAPS 2u    /* hnsw_search_kernel: the reference's heaps restated, one query per workgroup */
typedef struct fvdb_graph_search_info_t {
  uint32_t visited;               /* FVDB_GRAPH_VISITED_* */
  uint32_t kernel;                /* FVDB_GRAPH_KERNEL_* */
  uint32_t nb128;                 /* 128-dimension blocks of a padded row */
  uint32_t rows_per_round;        /* rows one scoring round of the sorted-register kernel holds; 0 for the exact-heap kernel */
  uint32_t nearest_in_registers;  /* exact-heap search (the kernel, or the restart after a tie): `nearest` in registers */
  uint32_t tcap;                  /* entries of a query's visited log */
  uint32_t cand_cap;              /* slots of the restated `candidates` heap in LDS */
  uint32_t spill_cap;             /* slots of its continuation in HBM, per query */
  uint32_t lds_bytes;             /* dynamic LDS of one workgroup */
  uint32_t reserved;
  uint64_t visited_bytes;         /* the batch's visited maps: B x the stride of one query's map */
} fvdb_graph_search_info_t;
int fvdb_graph_search_info(fvdb_graph* g, uint32_t B, uint32_t ef, fvdb_graph_search_info_t* out);

/* ---- device-resident graph maintenance ---------------------------------------------------------
 * HNSWIndex::vacuum (src/hnsw/operations.rs:176-200: deleted nodes leave every neighbour set, then the node map) on
 * the adjacency in HBM, as one device job.  Every node whose deleted flag is set is dropped from every list; a list
 * keeps its survivors in their old order, each with its stored edge distance (so the distances stay valid and no
 * whole-graph recomputation follows).  Rows of any stride are served (a row longer than 64 entries is walked in chunks).
 *
 * flags = 0: the job also RECLAIMS.  The surviving nodes are renumbered densely in their old order (node index = store
 *   row still holds), the row store, the adjacency and distance rows, the stamps and the per-node arrays are written into
 *   fresh buffers sized for the survivors (plus the usual growth slack) and swapped in, and the old ones are freed.  The
 *   job holds two copies for a moment.  Every allocation precedes the first change: FVDB_E_OOM leaves the graph and the
 *   store exactly as they were.  The graph must cover the whole store (FVDB_E_INVALID otherwise).  The entry point is
 *   renumbered; if it was deleted the graph has no entry afterwards and searches are refused (the reference does not
 *   repair it either).  The caller renumbers by the same rule: new index = number of undeleted nodes before it.
 * FVDB_VACUUM_KEEP_ROWS: the lists are pruned in place with the numbering unchanged and nothing allocated or freed; the
 *   lists of the deleted nodes are emptied; the nodes stay (deleted, unreferenced) until a later job reclaims them.
 *
 * removed (optional): flags = 0: nodes dropped; KEEP_ROWS: deleted nodes whose layer-0 list this call emptied.
 * Every mask created before the call is stale afterwards.  fvdb_graph_upload_bytes does not change.  The caller
 * excludes searches and inserts for the duration; the job synchronises the device before it starts and its stream
 * before it returns.  Only totals, counters and the 32-byte construction state cross the host link. */
#define FVDB_VACUUM_KEEP_ROWS 1u
typedef struct fvdb_graph_maintenance_info_t {
  uint64_t nodes_in, nodes_out;   /* nodes before / after */
  uint64_t edges_in, edges_out;   /* stored neighbours before / after, all layers */
  uint64_t rows_reclaimed;        /* store rows given back (0 with KEEP_ROWS) */
  uint64_t bytes_reclaimed;       /* what the dropped nodes held: store row, adjacency + distance rows, stamps, per-node words */
  uint64_t host_bytes;            /* copied to or from the host by the job */
  uint64_t move_bytes;            /* read + written in HBM by the store-row move */
  float ms_scan, ms_prune, ms_move;  /* device time per stage (HIP events) */
  float ms_total;                    /* wall clock of the call, allocations and the final synchronisation included */
} fvdb_graph_maintenance_info_t;
int fvdb_graph_vacuum(fvdb_graph* g, uint32_t flags, uint64_t* removed);
/* Figures of the last fvdb_graph_vacuum on this graph (zeros before the first). */
int fvdb_graph_maintenance_info(fvdb_graph* g, fvdb_graph_maintenance_info_t* out);

/* ---- device-resident graph health ---------------------------------------------------------------
 * A read-only job over the adjacency in HBM, everything in integers.  live(u): the deleted flag of u is clear.  N_l(u):
 * the stored list of u on layer l as stored (entries naming deleted nodes stay in it until a vacuum).
 *   census   n_live; edge_slots_live = the list lengths of live nodes over all their layers and max_level_live — the
 *            inputs of the reference's get_graph_stats (src/hnsw/operations.rs:227-272: total_edges = slots / 2,
 *            avg_degree, max_layer; its connected_components is a stub that answers 1); dangling / dangling0 = entries of
 *            live nodes' lists that name deleted nodes (all layers / layer 0: what fvdb_graph_vacuum would prune);
 *            degree0_hist[b] = live nodes with |N_0(u)| = b, the last bin "64 or more".
 *   reach    R = the nodes some search can admit, for every query, ef and k (src/hnsw/core.rs:398-554: a deleted
 *            neighbour is marked visited and never expanded, :510-513; the entry point is seeded and expanded whether it
 *            is deleted or not).  R = {entry} at l = level(entry); for l down to 0, R is closed under "u in R, live or
 *            the entry, level(u) >= l: every live v in N_l(u) joins"; what a layer leaves seeds the next.  reachable_live
 *            = |R and live|, unreachable_live = n_live - reachable_live, reach_rounds0 = the steps of layer 0's closure
 *            (a step expands what the step before added, the first one all of R; the last one adds nothing).  No entry
 *            point: R is empty.
 *   components  weak components of layer 0 among live nodes (u ~ v when v in N_0(u), both live, direction ignored):
 *            components0, largest_component0, isolated0 (components of one node).  The label of a live node is the
 *            smallest node index of its component, that of a deleted node 0xFFFFFFFF.
 * flags = 0 computes everything; a skipped part leaves its fields zero and its per-node result unavailable.  The job
 * runs on the context's stream, allocates its scratch (about 17 bytes a node) before the first launch — FVDB_E_OOM
 * leaves everything as it was — and gives it back, except the per-node results.  It changes nothing a search, an insert,
 * a mask or a vacuum can see; searches may run beside it, the caller excludes inserts, deletes and vacuums for the
 * duration.  n = 0: FVDB_OK and zeros; a graph that holds no device arrays yet: FVDB_E_INVALID;
 * 2^31 nodes or more: FVDB_E_UNSUPPORTED.  Between launches the host reads 16 bytes of state. */
#define FVDB_HEALTH_SKIP_REACH 1u
#define FVDB_HEALTH_SKIP_COMPONENTS 2u
typedef struct fvdb_graph_health_t {
  uint32_t n_nodes, n_live, has_entry, entry_live, entry_level, max_level_live;
  uint64_t edge_slots_live, dangling, dangling0;
  uint32_t degree0_hist[65];
  uint32_t reachable_live, unreachable_live, reach_rounds0;
  uint32_t components0, largest_component0, isolated0;
  uint32_t launches, reach_launches, host_syncs;   /* how the job ran: kernel launches (of them: reach steps), stream waits */
  float    ms;                                     /* HIP events around the job */
  uint64_t scratch_bytes;
} fvdb_graph_health_t;
int fvdb_graph_health(fvdb_graph* g, uint32_t flags, fvdb_graph_health_t* out);
/* Per-node results of the last fvdb_graph_health: reached[n] (1 = in R), label0[n].  FVDB_E_INVALID if the graph changed
 * since (or the job skipped what is asked for).  Either pointer may be NULL. */
int fvdb_graph_health_nodes(fvdb_graph* g, uint8_t* reached, uint32_t* label0);

/* With profiling on (fvdb_ctx_set_profiling): summed duration (HIP events on the launch stream) of the last
 * <= 64 launches of the traversal kernel since the previous call, and how many were summed; and (always) the
 * rows scored and hops taken by all queries since the previous call (either may be NULL).  Synchronises. */
int fvdb_graph_kernel_times(fvdb_graph* g, float* ms_sum, uint32_t* launches, uint64_t* rows_scored, uint64_t* hops);
/* Since the graph was created: queries the traversal kernel served, and how many of them it searched a second time with
 * the reference's BinaryHeaps restated because equal distances met where the heap layout decides (src/hnsw/core.rs:469-554;
 * such a query is the slowest of its launch).  Synchronises. */
int fvdb_graph_tie_restarts(fvdb_graph* g, uint64_t* queries, uint64_t* searched_again);

/* ---- filtered search: allow-set masks on the device -------------------------------------------------------
 *   The reference filters after the search: search_with_filter asks for
 * 3 k neighbours and keeps those the metadata filter accepts (src/hybrid/core.rs:513-549), so a selective filter
 * returns few results or none.  A masked search applies the allow-set INSIDE the search: it returns exactly what the
 * same search returns on an index in which every row outside the allow-set has been soft-deleted (mark_deleted,
 * src/ivf/operations.rs:569-591, src/hnsw/operations.rs:127-137) — ids and distance bits, in the same order.  Rows
 * already deleted stay excluded; entries of the allow-set the index does not hold are ignored.
 *
 * A mask is immutable and owns its device buffers: any number of searches in different slots may share one.  It is
 * built against the index as it stands; every mutation of the index (add*, set_deleted, clear, reserve, set_centroids,
 * train*, compact, refill_from; graph: upload, append_nodes, insert_linked, set_lists, set_entry, set_deleted) makes it
 * stale, and a masked search with a stale mask returns FVDB_E_INVALID (fvdb_last_error says so), never wrong rows.
 * Creating a mask needs the same exclusion against mutations as a search.  One mask serves a whole batch call of the
 * *_masked entry points; a batch in which every query has an allow-set of its own goes through the grouped entry points
 * (fvdb_ivf_search_groups_dev_slot, fvdb_graph_scan_allowed_groups_dev_slot: a table of masks and one index per query).  The
 * sharded search takes one through fvdb_ivf_search_sharded_wide_begin (fvdb_ivf_search_sharded_begin takes none).
 *  - fvdb_mask_create_ivf: ids[n] = the allowed row ids (host; duplicates and unknown ids are harmless).
 *  - fvdb_mask_create_graph: nodes[n] = the allowed NODE indices (host; the graph holds no ids: node index = store row).
 *  - fvdb_mask_info: allowed_live = rows (nodes) that are live in the index and allowed; stale = 1 once the index changed.
 *  - fvdb_mask_destroy waits for the device before it frees the buffers. */
typedef struct fvdb_mask fvdb_mask;
typedef struct fvdb_mask_info_t {
  uint32_t kind;   /* 1 = IVF index, 2 = graph */
  uint32_t stale;
  uint32_t units;  /* pool blocks (IVF) / nodes (graph) covered */
  uint32_t reserved;
  uint64_t allowed_live;
} fvdb_mask_info_t;
int fvdb_mask_create_ivf(fvdb_ivf* ivf, const uint64_t* ids, uint64_t n, fvdb_mask** out);
int fvdb_mask_create_graph(fvdb_graph* g, const uint32_t* nodes, uint64_t n, fvdb_mask** out);
int fvdb_mask_info(fvdb_mask* mask, fvdb_mask_info_t* out);
void fvdb_mask_destroy(fvdb_mask* mask);
/* fvdb_ivf_search_dev_slot / fvdb_ivf_search_probes_dev_slot under a mask: the skip of deleted rows
 * (src/ivf/core.rs:666-669) also skips the rows the mask does not allow, in every stage of the list scan (exact scan,
 * matrix-core threshold / filter / select / refine, exact rescan).  Under a mask FVDB_SCAN_AUTO always scans exactly
 * (the filter samples its threshold from lists the mask has thinned); FVDB_SCAN_FILTER still forces the filter.  Masked
 * searches are kept out of AUTO's hit-rate watch; fvdb_ivf_scan_fallbacks and _reasons count their rescans too. */
int fvdb_ivf_search_dev_slot_masked(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                    uint32_t k, uint32_t nprobe, uint64_t* out_ids_dev, float* out_dist_dev,
                                    uint32_t* out_counts_dev, uint64_t* out_keys_dev);
int fvdb_ivf_search_probes_dev_slot_masked(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev,
                                           const uint32_t* probes_dev, uint32_t B, uint32_t k, uint32_t nprobe,
                                           uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev,
                                           uint64_t* out_keys_dev);
/* search_with_config (src/ivf/core.rs:626-681) with 1 <= k <= FVDB_MAX_K_WIDE.  Same result definition, outputs,
 * padding and keys as fvdb_ivf_search_dev_slot; mask may be NULL (fvdb_mask_create_ivf otherwise; a stale mask is
 * FVDB_E_INVALID).  Always the exact scan (the matrix-core filter serves k <= 26).  Any nprobe >= 1, as for
 * fvdb_ivf_search.  k = 0 or k > FVDB_MAX_K_WIDE is FVDB_E_UNSUPPORTED, and so is an index holding a
 * shard of a larger one (fvdb_ivf_set_global_list_sizes).  Slot and stream rules are fvdb_ivf_search_dev_slot's. */
int fvdb_ivf_search_wide_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                  uint32_t k, uint32_t nprobe, uint64_t* out_ids_dev, float* out_dist_dev,
                                  uint32_t* out_counts_dev, uint64_t* out_keys_dev);
/* The wide search for an index that may hold a shard of a larger one (fvdb_ivf_set_global_list_sizes; an index
 * without global sizes is its own logical index).  1 <= k <= FVDB_MAX_K_WIDE, any nprobe >= 1 (nlist <= 16384 above
 * FVDB_MAX_K probes), mask may be NULL, given_probes_dev may be NULL (otherwise [B][min(nprobe, nlist)] list ids in
 * probe order, 0xFFFFFFFF = "no list", and the coarse stage is skipped).  The rows are selected as the wide search
 * selects them — by (distance bits, scan position on this rank); lists this rank does not own are empty here, so that
 * order over this rank's rows is the logical index's — and every key is
 *   (distance bits << 32) | (64 x blocks of the earlier-ranked probed lists of the LOGICAL index + position),
 * the key of fvdb_ivf_search_dev_slot: unique across the ranks, so the partial lists merge exactly
 * (fvdb_merge_keys_wide_dev).  The low word is 32 bits wide, on this path as on the register path: a logical index
 * whose probed lists could hold 2^32 scan positions or more (64 x min(nprobe x longest list, all lists) blocks) is
 * refused with FVDB_E_UNSUPPORTED.  Slot and stream rules are fvdb_ivf_search_dev_slot's. */
int fvdb_ivf_search_shard_wide_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev,
                                        uint32_t B, uint32_t k, uint32_t nprobe, const uint32_t* given_probes_dev,
                                        uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev,
                                        uint64_t* out_keys_dev);
/* The wide search with one allow-set per query.  masks[G]: masks of this index, or NULL for "no
 * filter"; group_of_query[B] (HOST memory, read before the call returns): the entry of masks[] query b is searched
 * under.  The result of query b — ids, distance bits, count, order and key — is what fvdb_ivf_search_wide_dev_slot returns
 * for that query alone under masks[group_of_query[b]] (for k <= FVDB_MAX_K also what fvdb_ivf_search_dev_slot_masked
 * returns).  Always the wide route, 1 <= k <= FVDB_MAX_K_WIDE, any nprobe >= 1, with fvdb_ivf_search_wide_dev_slot's
 * limits: an index holding a shard of a larger one is FVDB_E_UNSUPPORTED.  Checked before anything is enqueued, and for
 * every entry of masks[] whether a query names it or not: a mask of another index or a stale one, a group index >= G, and
 * G == 0 with B > 0 are FVDB_E_INVALID.  Counts as a masked search (AUTO's watch does not see it).  Slot and stream rules
 * are fvdb_ivf_search_dev_slot's. */
int fvdb_ivf_search_groups_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* const* masks, uint32_t G,
                                    const uint32_t* group_of_query, const float* q_dev, uint32_t B, uint32_t k, uint32_t nprobe,
                                    uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev, uint64_t* out_keys_dev);
/* The same search (src/ivf/core.rs:626-681), blocking, with host pointers and leased scratch like fvdb_ivf_search: any
 * number of host threads may call it on one index. */
int fvdb_ivf_search_wide(fvdb_ivf* ivf, const float* q, uint32_t B, uint32_t k, uint32_t nprobe, uint64_t* out_ids,
                         float* out_dist, uint32_t* out_counts);
/* evaluate_search_quality's per-query figures (src/ivf/operations.rs:344-377), resident: the search at `nprobe` and
 * the search of every list in centroid-rank order (search_with_config(query, k, n_clusters): the ground truth) run on
 * the slot, both results stay in HBM, and per query
 *   matches   = result entries whose id occurs among the truth's ids,
 *   recall    = truth empty ? 1 : matches / min(len(truth), k),
 *   precision = result empty ? 0 : matches / len(result)        (f32 divisions of exactly representable integers)
 * go to out_recall_dev[B] / out_precision_dev[B] (device memory).  1 <= k <= FVDB_MAX_K_WIDE; slot and stream rules are
 * fvdb_ivf_search_dev_slot's. */
int fvdb_ivf_search_quality_dev(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t k,
                                uint32_t nprobe, float* out_recall_dev, float* out_precision_dev);
/* evaluate_search_quality (src/ivf/operations.rs:329-391) at EVERY nprobe from one search of every list.  The truth
 * of a query is the top k of the search of every list in centroid-rank order, and a search at nprobe = p scans the
 * first p ranked lists at the same scan positions: a truth row whose list ranks below p is in the p-probe result, and
 * a p-probe result row that is in the truth is such a row.  Per query and p = 1 .. nlist
 *   matches(p)   = truth entries whose list has centroid rank < p,
 *   recall(p)    = truth empty ? 1 : matches(p) / min(len(truth), k),
 *   precision(p) = len_result(p) == 0 ? 0 : matches(p) / len_result(p),  len_result(p) = min(k, live rows of the first
 *                  p ranked lists)                                       (the f32 divisions of fvdb_ivf_search_quality_dev)
 * and out_recall_sum_dev[p - 1] / out_precision_sum_dev[p - 1] (device memory, nlist floats each) receive their sums
 * over the B queries, added in query order in f32 as the reference's `total_recall += recall` (:379-387): bit for bit
 * the sums of fvdb_ivf_search_quality_dev's values at nprobe = p.  Uniqueness condition: these figures equal the
 * reference's id-based ones when no id is stored in two lists; otherwise they count rows, not ids.
 * mask: NULL, or an allow-set mask of this index ("live" then means allowed and live; a stale mask is FVDB_E_INVALID).
 * chunk_queries: 0 = as many queries per pass as fit the call's scratch budget, else at most that many (the sums do not
 * depend on it).  1 <= k <= FVDB_MAX_K_WIDE (the every-list search is fvdb_ivf_search_dev_slot's, or the wide one's for
 * k > FVDB_MAX_K), else FVDB_E_UNSUPPORTED; so are an index of more than 16384 lists and one holding a shard of a larger
 * one (fvdb_ivf_set_global_list_sizes).  B = 0 is FVDB_OK and writes nothing.  Slot and stream rules are
 * fvdb_ivf_search_dev_slot's. */
int fvdb_ivf_quality_curve_dev(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                               uint32_t k, uint32_t chunk_queries, float* out_recall_sum_dev, float* out_precision_sum_dev);
/* fvdb_graph_search_dev_slot under a mask: a node the mask does not allow is treated as deleted — never expanded into
 * `candidates`, never returned (src/hnsw/core.rs:511-513, :451-466).  status 1 queries go to the host walk as before;
 * the host must apply the same view there. */
int fvdb_graph_search_dev_slot_masked(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                      uint32_t k, uint32_t ef, uint32_t* out_nodes_dev, float* out_dist_dev,
                                      uint32_t* out_counts_dev, uint32_t* out_status_dev);
/* Exact k-NN over the allowed live nodes of a graph mask (no counterpart in the reference: "as if deleted" thins the
 * graph the traversal walks, so a small allow-set is scanned instead).  Every allowed node is scored with the
 * reference's f32 fold (src/core/vector_ops.rs:51-57); the k best by (distance bits ascending, node index ascending).
 * out_nodes/out_dist: B x k (unused tail = FVDB_NO_ROW / +inf), out_counts[B].  k <= FVDB_MAX_K. */
int fvdb_graph_scan_allowed_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                     uint32_t k, uint32_t* out_nodes_dev, float* out_dist_dev, uint32_t* out_counts_dev);
/* The same scan with one mask per query: masks[G] are masks of this graph, none NULL (the
 * unfiltered exact scan is fvdb_graph_search_flat_dev_slot), group_of_query[B] is HOST memory, read before the call
 * returns.  Query b gets what fvdb_graph_scan_allowed_dev_slot returns for it under masks[group_of_query[b]].
 * k <= FVDB_MAX_K.  Checked before anything is enqueued, every mask whether named or not: a NULL, foreign or stale mask,
 * a group index >= G, and G == 0 with B > 0 are FVDB_E_INVALID. */
int fvdb_graph_scan_allowed_groups_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* const* masks, uint32_t G,
                                            const uint32_t* group_of_query, const float* q_dev, uint32_t B, uint32_t k,
                                            uint32_t* out_nodes_dev, float* out_dist_dev, uint32_t* out_counts_dev);

/* ---- exact search ------------------------------------------------
 * Flat exact k-NN over the rows a graph holds, as they are stored, where they are stored (no counterpart in the
 * reference: the ground truth its recall figures are measured against).  Every live node is scored with the
 * reference's f32 fold (src/core/vector_ops.rs:51-57; an fp16 row widened exactly first) by a coalesced tile scan of
 * the row store; the k best by (distance bits ascending, node index ascending) — the result rule of
 * fvdb_graph_scan_allowed_dev_slot, whose slot, stream and staleness rules also hold here.  mask: NULL = the graph's
 * own deleted flags; else a node the mask does not allow counts as deleted (a mask of another graph or a stale one:
 * FVDB_E_INVALID).  out_nodes/out_dist: B x k (unused tail = FVDB_NO_ROW / +inf), out_counts[q] = min(k, live nodes);
 * an empty graph gives counts of 0.  k == 0 or k > FVDB_MAX_K: FVDB_E_UNSUPPORTED.  Large batches are scanned in
 * sub-batches on the stream so the partial lists in the slot's scratch stay bounded. */
int fvdb_graph_search_flat_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                    uint32_t k, uint32_t* out_nodes_dev, float* out_dist_dev, uint32_t* out_counts_dev);
/* The same search with 1 <= k <= FVDB_MAX_K_WIDE.  Same result definition, arguments, outputs,
 * mask, slot, stream and staleness rules, and the same refusals in the same order; k == 0 or k > FVDB_MAX_K_WIDE is
 * FVDB_E_UNSUPPORTED.  Replaces nothing: fvdb_graph_search_flat_dev_slot keeps its limit and its register list, as
 * fvdb_ivf_search kept its own beside fvdb_ivf_search_wide.  The rows are scored by the same fold; each distance word
 * goes to a per-query arena in the slot's scratch (4 bytes per node, padded to whole 64-row tiles) and the k best are
 * found by the wide selection of fvdb_ivf_search_wide — radix select of the k-th word, ties at the cut in node order —
 * so for k <= FVDB_MAX_K it returns exactly what fvdb_graph_search_flat_dev_slot returns.  Always this route, whatever
 * k.  Queries go in sub-batches whose arena fits 1 GiB (FVDB_FLAT_WIDE_ARENA_BYTES in the environment, read at every
 * call, overrides the figure; a sub-batch holds at least one query), one after the other on the stream. */
int fvdb_graph_search_flat_wide_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev,
                                         uint32_t B, uint32_t k, uint32_t* out_nodes_dev, float* out_dist_dev,
                                         uint32_t* out_counts_dev);
/* ---- radius search -----------------------------------------------
 * "Everything within r" where every search above answers "the k nearest".  For query b with radius r = radius[b]
 * (f32, r >= 0, +inf allowed) the BALL is the set of candidate rows — the rows the corresponding k-search would score,
 * under the same mask — whose distance word satisfies bits(dist) <= bits(r): inclusive, on the reference's own f32
 * distance.  out_totals[b] = the size of the ball, exact and never capped.  The results are its first
 * min(total, max_results) rows by the wide selection's key (distance bits << 32 | scan position): what the wide search
 * at k = max_results returns, cut at the radius.  Outputs are [B][max_results] with the usual tails, out_counts[b] =
 * min(total, max_results).  1 <= max_results <= FVDB_MAX_K_WIDE, else FVDB_E_UNSUPPORTED.  The _dev forms do not
 * inspect device input: there a negative or NaN radius has an empty ball (-0.0 is 0.0).
 *
 * Over a graph's live nodes: fvdb_graph_search_flat_wide_dev_slot's scan, arguments, sub-batches, mask, slot, stream and
 * staleness rules and its refusals in its order; the selection counts the ball in one pass over the arena and, when it
 * fits max_results, gathers and sorts it with no radix pass. */
int fvdb_graph_search_flat_radius_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev,
                                           uint32_t B, const float* radius_dev, uint32_t max_results, uint32_t* out_nodes_dev,
                                           float* out_dist_dev, uint32_t* out_counts_dev, uint32_t* out_totals_dev);
/* out_totals_dev[b] alone: the same scan with no arena and no selection, each wave counting the rows of its slice within
 * each radius (integer adds: the result does not depend on their order).  out_totals_dev is zeroed on the stream first. */
int fvdb_graph_count_within_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                     const float* radius_dev, uint32_t* out_totals_dev);
/* Over the live rows of the nprobe probed lists in probe order: fvdb_ivf_search_wide_dev_slot's lists, score stage,
 * mask, any-nprobe, slot, stream and staleness rules; an index holding a shard of a larger one is FVDB_E_UNSUPPORTED.
 * Totals count the probed lists only. */
int fvdb_ivf_search_radius_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                    const float* radius_dev, uint32_t max_results, uint32_t nprobe, uint64_t* out_ids_dev,
                                    float* out_dist_dev, uint32_t* out_counts_dev, uint32_t* out_totals_dev);
/* The same, blocking, with host pointers and leased scratch like fvdb_ivf_search_wide.  Non-finite queries are
 * FVDB_E_NONFINITE as there; a negative or NaN radius is FVDB_E_INVALID. */
int fvdb_ivf_search_radius(fvdb_ivf* ivf, const float* q, uint32_t B, const float* radius, uint32_t max_results, uint32_t nprobe,
                           uint64_t* out_ids, float* out_dist, uint32_t* out_counts, uint32_t* out_totals);

/* ---- diverse selection -------------------------------------------
 * "The k best rows that are not copies of each other": of the candidates a search of fetch_k returned for a query,
 * keep k by maximal marginal relevance, optionally after dropping every later copy of an id.  Per query, with
 * candidates c = 0 .. n-1 (n = min(counts[b], fetch_k)) in the order given, a = (float)lam, b = 1.0f - a:
 *   1. distinct: c is dropped when some c' < c has the same id;
 *   2. the first pick is the first kept candidate;
 *   3. after every pick s, for each kept unpicked c: t = the reference distance of row c to row s (f32, dimensions
 *      ascending, no FMA, sqrtf), m[c] = min(m[c], t) from +inf, gain[c] = b * m[c] - a * dist[c] (two multiplies and
 *      one subtract, each rounded once); the next pick has the largest gain, the smallest c among equal gains;
 *   4. min(k, kept) picks.
 * Outputs are [B][k] in PICK order: the id, the distance as given, and the rank (the candidate position c); tails are
 * FVDB_NO_ID / +inf / FVDB_NO_ROW; out_counts[b] = the number of picks.  lam = 1 is the first k kept candidates.
 * rows_dev: [B][fetch_k][row_stride] f32, 16-byte aligned, candidate c of query b at (b * fetch_k + c) * row_stride; the
 * whole stride is folded, so every float past the dimension must be zero.  Rows of candidates at or beyond the count
 * are not read.  Everything is device memory; the call is enqueued on ctx's stream and does not synchronise.
 * fetch_k == 0 or > FVDB_MAX_K: FVDB_E_UNSUPPORTED; k == 0, k > fetch_k, lam NaN or outside [0, 1], row_stride == 0 or
 * not a multiple of 4, a NULL buffer with B > 0: FVDB_E_INVALID; B == 0: FVDB_OK, nothing enqueued. */
int fvdb_mmr_select_dev(fvdb_ctx* ctx, const float* rows_dev, uint32_t row_stride, const uint64_t* ids_dev, const float* dist_dev,
                        const uint32_t* counts_dev, uint32_t B, uint32_t fetch_k, uint32_t k, float lam, int distinct,
                        uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_rank_dev, uint32_t* out_counts_dev);
/* The gathers that fill such a block.  fvdb_ivf_get_rows_dev with output row i at out_rows_dev + i * out_stride
 * (out_stride >= d, else FVDB_E_INVALID); dimensions d .. min(out_stride, d rounded up to 4) are written as zeros, and a
 * location whose cluster is FVDB_NO_ROW is skipped (its output row is left as it was).  out_stride == d is
 * fvdb_ivf_get_rows_dev. */
int fvdb_ivf_get_rows_dev_strided(fvdb_ivf* ivf, fvdb_ctx* on, const uint32_t* cluster, const uint32_t* pos, uint64_t n,
                                  float* out_rows_dev, uint32_t out_stride);
/* Rows of a row store by row index, the same output form: rows_dev[n] in DEVICE memory, widened exactly when the store
 * is fp16; an index at or beyond fvdb_store_rows() (FVDB_NO_ROW among them) is skipped.  Enqueued on `on`'s stream
 * (NULL = the store's); no synchronisation.  Reads only. */
int fvdb_store_get_rows_dev(fvdb_store* store, fvdb_ctx* on, const uint32_t* rows_dev, uint64_t n, float* out_rows_dev,
                            uint32_t out_stride);
/* ---- grouped selection --------------------------------------------
 * "The k best groups by a metadata field": of the candidates a search of fetch_k returned for a query, the first k
 * groups by a key, each with its first group_size members.
 *
 * Key of a candidate, under a metadata table and one of its columns.  The key is NONE when the id is FVDB_NO_ID, the id
 * is in no slot of the table, its slot is not present, its cell is MISSING, ARRAY or COMPLEX, or its cell is a FLOAT NaN.
 * Otherwise it is (tag, canon): canon is the cell's word as stored, except that a FLOAT -0.0 is folded onto 0.0 and a NULL
 * is 0.  Two candidates are in the same group iff their tags are equal and their canon words are equal (the equality of
 * the metadata columns: 1, 1.0, "1" and true are four groups, 0.0 and -0.0 are one).
 *
 * Selection, per query, over candidates c = 0 .. n-1 (n = min(counts[b], fetch_k)) IN THE ORDER GIVEN; only positions
 * are compared, never distances:
 *   1. distinct: c is dropped when some c' < c has the same id;
 *   2. a kept candidate whose key is none is dropped (missing = FVDB_GROUP_MISSING_DROP) or forms a group of its own
 *      (FVDB_GROUP_MISSING_OWN);
 *   3. the groups are ordered by the position of their first member;
 *   4. the members of a group are its kept candidates in position order;
 *   5. output is the first k groups, each with its first group_size members.
 * Outputs, all device memory: out_ids / out_dist / out_rank [B][k][group_size] (the id, the distance as given, the
 * candidate position c), out_members[B][k] (members written), out_group_total[B][k] (kept candidates of the n that carry
 * the key, not capped by group_size), out_key_tag / out_key_val [B][k] (the group's tag and canon word; a group made by
 * FVDB_GROUP_MISSING_OWN has tag FVDB_META_MISSING and word 0), out_groups[B] (groups written), out_flags[B] (bit 0 set
 * iff n == fetch_k: the candidate list may have been cut).  Tails are FVDB_NO_ID / +inf / FVDB_NO_ROW / 0.
 *
 * What the flags let a caller conclude.  Walking candidates in ascending distance, the first k distinct keys ARE the k
 * best groups by best member.  So the set of groups is exact with respect to the underlying search iff
 * out_groups[b] == k or bit 0 is clear, and a group's members are its best members iff out_members == group_size or bit 0
 * is clear.  Nothing else is claimed.
 *
 * fvdb_group_keys_of_ids_dev writes one (tag, canon) per id, a none key as (FVDB_META_MISSING, 0); enqueued on the
 * stream of the table's context, no synchronisation.  (Its name carries the feature's prefix, not fvdb_meta_: the set of
 * fvdb_meta_ entry points is the table's own.)  The lookup goes through an open-addressing index in HBM that the table
 * owns: a power of two of cells, at least twice the slots, linear probing; built by a kernel from the slots' ids with a
 * 64-bit compare-and-swap on the id word and an atomic min on the slot word, so of the slots that carry one id the LOWEST
 * answers, whatever the scheduling.  The empty id word is FVDB_NO_ID, whose key is none by definition: such a slot is
 * never entered, and every other id, 0 among them, is an ordinary id.  The index is rebuilt lazily, by the first lookup
 * after fvdb_meta_set_rows has run; presence and cells are read at lookup time, so fvdb_meta_set_present and
 * fvdb_meta_set_cells need no rebuild.  fvdb_meta_info's hbm_bytes counts it.  A column outside the table is
 * FVDB_E_INVALID before anything is enqueued; n >= 2^31 is FVDB_E_UNSUPPORTED; n == 0 is FVDB_OK.  Locks the table.
 *
 * fvdb_group_select_dev takes key_tag_dev / key_val_dev [B][fetch_k] as that call writes them (a tag other than NULL,
 * BOOL, INT, FLOAT or STRING, and any candidate whose id is FVDB_NO_ID, is a none key).  Enqueued on ctx's stream, no
 * synchronisation; two runs over the same inputs write identical bytes.  fetch_k == 0 or > FVDB_MAX_K_WIDE, or
 * k * group_size > FVDB_MAX_K_WIDE: FVDB_E_UNSUPPORTED; k == 0, group_size == 0, an unknown `missing`, a NULL buffer with
 * B > 0: FVDB_E_INVALID; B == 0: FVDB_OK, nothing enqueued. */
#define FVDB_GROUP_MISSING_DROP 0
#define FVDB_GROUP_MISSING_OWN 1
int fvdb_group_select_dev(fvdb_ctx* ctx, const uint64_t* ids_dev, const float* dist_dev, const uint32_t* counts_dev,
                          const uint8_t* key_tag_dev, const uint64_t* key_val_dev, uint32_t B, uint32_t fetch_k, uint32_t k,
                          uint32_t group_size, int distinct, int missing, uint64_t* out_ids_dev, float* out_dist_dev,
                          uint32_t* out_rank_dev, uint32_t* out_members_dev, uint32_t* out_group_total_dev, uint8_t* out_key_tag_dev,
                          uint64_t* out_key_val_dev, uint32_t* out_groups_dev, uint32_t* out_flags_dev);
/* The comparison of fvdb_ivf_search_quality_dev on two id blocks the caller holds in HBM (B x k ids with their hit
 * counts; entries at or beyond a count are not read): per query matches, recall and precision by the formulas stated
 * there — an id the result holds twice counts twice — to out_recall_dev[B] / out_precision_dev[B], enqueued on ctx's
 * stream.  k > 0. */
int fvdb_search_quality_lists_dev(fvdb_ctx* ctx, const uint64_t* res_ids_dev, const uint32_t* res_counts_dev,
                                  const uint64_t* truth_ids_dev, const uint32_t* truth_counts_dev, uint32_t B, uint32_t k,
                                  float* out_recall_dev, float* out_precision_dev);
/* fvdb_search_quality_lists_dev's figures for the hybrid result at EVERY pair (efs[i], n_probes[j]) from the PARTS the
 * caller holds in HBM, without forming any merged result.  Per query
 *   truth    truth_ids_dev[B][k] with truth_counts_dev[B]: the ids of the exact result;
 *   recent   recent_ids_dev / recent_dist_dev [E][B][rk] with recent_counts_dev[E][B]: the recent part at each listed
 *            ef, distances ascending;
 *   hist     hist_ids_dev / hist_dist_dev [P][B][hk] with hist_counts_dev[P][B]: the historical part at each listed
 *            n_probe, distances ascending.
 * Entries at or beyond a count are not read.  The result at (i, j) is the first L = min(k, |G| + |H|) entries of the
 * stable merge of G = recent[i] and H = hist[j], recent first on equal distances (src/hybrid/core.rs:476-485): the
 * first a entries of G and the first L - a of H, a found by a binary search (entry a of G is inside iff
 * a + #{h in H : d_h < d_G[a]} < L).  matches = entries of that result whose id occurs in the truth (an id the
 * result holds twice counts twice), recall = truth empty ? 1 : matches / min(len(truth), k), precision = L == 0 ? 0 :
 * matches / L — bit for bit what fvdb_search_quality_lists_dev writes for the merged result.
 * out_recall_dev / out_precision_dev: [max(E, 1)][max(P, 1)][B] floats, enqueued on ctx's stream.
 * P == 0 (the hist pointers are not read, NULL is fine): the graph-only form, the result is recent[i] cut at k.
 * E == 0 likewise: the list-only form.  E == 0 and P == 0, a NULL block of a part that is present: FVDB_E_INVALID.
 * 1 <= k <= FVDB_MAX_K_WIDE, and so rk / hk of a part that is present; E, P <= 64; B < 2^31 and at most 2^38 (i, j,
 * query) triples: FVDB_E_UNSUPPORTED otherwise.  B == 0 is FVDB_OK and writes nothing.  The lists' prefix counts go to
 * scratch the context owns (4 bytes per list entry), shared by the calls on that context in stream order. */
int fvdb_quality_grid_dev(fvdb_ctx* ctx, const uint64_t* truth_ids_dev, const uint32_t* truth_counts_dev,
                          const uint64_t* recent_ids_dev, const float* recent_dist_dev, const uint32_t* recent_counts_dev,
                          const uint64_t* hist_ids_dev, const float* hist_dist_dev, const uint32_t* hist_counts_dev, uint32_t B,
                          uint32_t k, uint32_t rk, uint32_t hk, uint32_t E, uint32_t P, float* out_recall_dev,
                          float* out_precision_dev);

/* ---- multi-GPU: inverted lists sharded across the GPUs of a node, RCCL over xGMI -------------------------
 * (BASELINE config C4; SURVEY §8e.  The reference has no distributed execution: what is preserved is the result —
 * the merged answer equals the single-index answer bit for bit, because the selection keys are global.)
 * One rank per GPU: a process (torch.distributed-style launch) or a host thread of one process, each with its own
 * fvdb_ctx.  Lists are placed with fvdb_ivf_add_assigned (only the lists the rank owns) + fvdb_ivf_set_global_list_sizes;
 * centroids are replicated.
 *
 * Communicator.  fvdb_comm_unique_id on rank 0 yields 128 bytes (ncclUniqueId) that the host ships to the other
 * ranks out of band (its own rendezvous: TCP store, file, MPI ...); every rank then calls fvdb_comm_create
 * (ncclCommInitRank).  librccl is loaded at that moment (dlopen), never by a single-GPU process.
 * fvdb_comm_create_hosted is the same interface over a caller-supplied exchange of HOST buffers (tests, rehearsals on
 * one GPU, fabrics RCCL does not drive): op 0 = all-gather (send: `bytes`, recv: world blocks of `bytes` in rank
 * order), op 1 = all-to-all (send/recv: world blocks of `bytes`; block p of send goes to rank p); return 0 on success.
 * Collectives of one communicator must be issued in the same order on every rank. */
typedef struct fvdb_comm fvdb_comm;
typedef int (*fvdb_exchange_fn)(void* user, int op, const void* send_host, void* recv_host, size_t bytes);
int fvdb_comm_unique_id(void* out128);
int fvdb_comm_create(fvdb_ctx* ctx, const void* id128, int world, int rank, fvdb_comm** out);
int fvdb_comm_create_hosted(fvdb_ctx* ctx, int world, int rank, fvdb_exchange_fn fn, void* user, fvdb_comm** out);
void fvdb_comm_destroy(fvdb_comm* comm);
int fvdb_comm_rank(fvdb_comm* comm);
int fvdb_comm_world(fvdb_comm* comm);
/* Stream-ordered collectives on `on`'s stream (NULL = the communicator's context): recv_dev holds world blocks. */
int fvdb_comm_all_gather_dev(fvdb_comm* comm, fvdb_ctx* on, const void* send_dev, void* recv_dev, size_t bytes);
int fvdb_comm_all_to_all_dev(fvdb_comm* comm, fvdb_ctx* on, const void* send_dev, void* recv_dev, size_t bytes);

/* Sharded search_with_config.  FVDB_SHARD_WEAK: q_dev = this rank's OWN B queries (global batch world*B); the rank
 * gets the results of its own B queries.  FVDB_SHARD_STRONG: q_dev = the SAME B queries on every rank (global batch
 * B); rank r gets the results of queries [r*per, min(B, (r+1)*per)), per = ceil(B/world) = fvdb_sharded_out_rows().
 * begin enqueues the whole step — centroid ranking, exchange 1 (weak: all-gather of queries + probe lists), scan of
 * the lists this rank owns, exchange 2 (all-to-all of the partial (key, id) lists), world-way merge by key — on
 * `on`'s stream (NULL = the index's own) with the slot-th scratch set; no host synchronisation in between.  Outputs
 * (device, fvdb_sharded_out_rows() x k) are valid after fvdb_ivf_search_sharded_end (or any wait on that stream).
 * Every rank calls begin for the same slots in the same order. */
#define FVDB_SHARD_WEAK 0
#define FVDB_SHARD_STRONG 1
typedef struct fvdb_sharded fvdb_sharded;
int fvdb_sharded_create(fvdb_ivf* ivf, fvdb_comm* comm, fvdb_sharded** out);
void fvdb_sharded_destroy(fvdb_sharded* s);
uint32_t fvdb_sharded_out_rows(fvdb_sharded* s, uint32_t B, int mode);
int fvdb_ivf_search_sharded_begin(fvdb_sharded* s, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t k,
                                  uint32_t nprobe, int mode, uint64_t* out_ids_dev, float* out_dist_dev,
                                  uint32_t* out_counts_dev);
/* The sharded search at any k <= FVDB_MAX_K_WIDE, any nprobe >= 1 (nlist <= 16384 above FVDB_MAX_K probes) and under
 * an optional allow-set mask (NULL = none); collected by fvdb_ivf_search_sharded_end.  Same modes, exchanges, slot
 * buffers and output shapes as fvdb_ivf_search_sharded_begin.  With k > FVDB_MAX_K or more than FVDB_MAX_K lists
 * probed, the lists step is fvdb_ivf_search_shard_wide_dev_slot and the merge fvdb_merge_keys_wide_dev; that route has
 * no matrix-core filter, so it exchanges no thresholds.  Otherwise the step is fvdb_ivf_search_sharded_begin's, under
 * the mask if there is one; a masked step keeps its filter thresholds rank-local.  Which route and which collectives
 * a call takes follows from shapes, mode and whether a mask is given alone, so every rank decides alike.
 * Every rank must pass a mask built from the SAME allow-set (each over its own shard: fvdb_mask_create_ivf), as every
 * rank of a hybrid index passes the same `now`.  A mask of another index, or one built before the index last changed,
 * is FVDB_E_INVALID before anything is exchanged. */
int fvdb_ivf_search_sharded_wide_begin(fvdb_sharded* s, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev,
                                       uint32_t B, uint32_t k, uint32_t nprobe, int mode, uint64_t* out_ids_dev,
                                       float* out_dist_dev, uint32_t* out_counts_dev);
int fvdb_ivf_search_sharded_end(fvdb_sharded* s, fvdb_ctx* on, uint32_t slot);

/* ---- metadata columns: filters evaluated on the device -------------------------------
 * A table of typed metadata columns resident in HBM and one evaluation pass per filter.  Together they replace the
 * walk of MetadataFilter::matches (src/core/metadata_filter.rs:265-338) over every entry of the session's metadata
 * map (bindings/node/src/session.rs:233-247 hands the filter to the search; the allow-set form of that search is
 * fvdb_mask_create_*).  The result is the list of row ids whose metadata match, in slot order, plus the slots the
 * device could not decide.
 *
 * Slots.  A table has slots 0 .. slots-1, never reordered, never reused for another id: per slot a uint64 row id and a
 * `present` byte (the row has an entry in the metadata map).  A slot that is not present matches no filter.
 * Columns.  One per metadata path, as two arrays: tag[slot] (one byte, FVDB_META_*) and val[slot] (eight bytes):
 *   MISSING, NULL, COMPLEX  no payload        BOOL    0 or 1            INT     the int64
 *   FLOAT   the bits of the f64              STRING  the caller's dense code of the string (exact, assigned by the host)
 *   ARRAY   its elements live in the column's element arrays; an element carries any tag but MISSING and ARRAY
 * COMPLEX marks a value the device does not decide (an object compared whole, a nested list, an integer outside
 * int64); a leaf that needs a comparison with one is "unknown" on that slot.  A new column is MISSING everywhere.
 *
 * Program.  Postfix, over three-valued results (true, false, unknown); n_instrs instructions of four uint32 each:
 *   { FVDB_META_OP_EQUALS,               column, c, 0 }   cell (or any element of an ARRAY cell) equals constant c
 *   { FVDB_META_OP_IN | flags << 8,      column, c, n }   a scalar cell equals one of the constants c .. c+n-1, which are
 *                                                          sorted ascending by (tag, key), distinct, none COMPLEX or NEVER;
 *                                                          flags: FVDB_META_IN_HAS_COMPLEX (the list also held a COMPLEX
 *                                                          constant), FVDB_META_IN_HAS_ANY (the list was not empty)
 *   { FVDB_META_OP_RANGE | flags << 8,   column, c, 0 }   constants c (lower) and c+1 (upper): FLOAT, key = the f64's bits;
 *                                                          flags FVDB_META_RANGE_*; INT cells go to f64 to nearest even
 *   { FVDB_META_OP_AND / _OR,            n, 0, 0 }        pops n results, pushes their Kleene AND / OR (n = 0: true / false)
 * Constants are (tag, key) pairs.  key: NULL 0; BOOL 0 / 1; STRING the code; INT the int64 with its sign bit flipped;
 * FLOAT the f64's bits with -0.0 folded onto 0.0, then all bits flipped if negative, else the sign bit set (so that key
 * order is value order).  FVDB_META_NEVER is a constant that equals nothing (a NaN, a string without a code);
 * FVDB_META_COMPLEX one that only the host can compare.  Equality needs equal tags (INT never equals FLOAT, BOOL is no
 * number, NULL equals NULL, a NaN equals nothing, 0.0 equals -0.0).  The program must leave exactly one result.
 *
 * Limits (FVDB_E_UNSUPPORTED beyond them): FVDB_META_MAX_PROGRAM instructions, FVDB_META_MAX_STACK results on the stack
 * at once (so also operands of one AND / OR), FVDB_META_MAX_CONSTS constants, fewer than 2^32 slots, fewer than 2^32
 * elements in one column.  Malformed arguments (a column, constant or slot out of range, an unknown tag or op, unsorted
 * IN constants, a stack underflow, more or less than one result left) are FVDB_E_INVALID before anything is enqueued.
 * Every entry point locks the table: evaluations and mutations of one table are serialised. */
#define FVDB_META_MISSING 0u
#define FVDB_META_NULL 1u
#define FVDB_META_BOOL 2u
#define FVDB_META_INT 3u
#define FVDB_META_FLOAT 4u
#define FVDB_META_STRING 5u
#define FVDB_META_ARRAY 6u
#define FVDB_META_COMPLEX 7u
#define FVDB_META_NEVER 15u
#define FVDB_META_OP_EQUALS 1u
#define FVDB_META_OP_IN 2u
#define FVDB_META_OP_RANGE 3u
#define FVDB_META_OP_AND 4u
#define FVDB_META_OP_OR 5u
#define FVDB_META_IN_HAS_COMPLEX 1u
#define FVDB_META_IN_HAS_ANY 2u
#define FVDB_META_RANGE_HAS_MIN 1u
#define FVDB_META_RANGE_MIN_INCLUSIVE 2u
#define FVDB_META_RANGE_HAS_MAX 4u
#define FVDB_META_RANGE_MAX_INCLUSIVE 8u
#define FVDB_META_MAX_PROGRAM 1024u
#define FVDB_META_MAX_STACK 16u
#define FVDB_META_MAX_CONSTS 65536u
typedef struct fvdb_meta fvdb_meta;
typedef struct fvdb_meta_info_t {
  uint64_t slots, present, columns;
  uint64_t live_elements, dead_elements; /* elements of ARRAY cells in use / left behind by rewritten cells, all columns */
  uint64_t hbm_bytes;                    /* device memory the table holds, result buffers included */
} fvdb_meta_info_t;
/* The table itself: replaces the session's `metadata: HashMap<String, Value>` (bindings/node/src/session.rs:69) as
 * what a filter is evaluated over. */
int fvdb_meta_create(fvdb_ctx* ctx, fvdb_meta** out);
void fvdb_meta_destroy(fvdb_meta* t);
int fvdb_meta_info(fvdb_meta* t, fvdb_meta_info_t* out);
/* Slots first .. first+n-1 get ids[i] and present[i] (session.rs:394-415: an entry of the metadata map per added
 * vector).  first <= slots: a run may rewrite slots, extend the table, or both; new slots are MISSING in every column.
 * A run over existing slots stores the ids it is given: that a slot is never reused for another id is the caller's
 * rule to keep, the table does not check it. */
int fvdb_meta_set_rows(fvdb_meta* t, uint64_t first, uint64_t n, const uint64_t* ids, const uint8_t* present);
/* present[i] for the listed slots, strictly ascending (session.rs:464-467: delete_vector drops the entry). */
int fvdb_meta_set_present(fvdb_meta* t, const uint32_t* slots, const uint8_t* present, uint64_t n);
/* A new column, MISSING everywhere; its index to *out_column (metadata_filter.rs:360-375: one per dotted path). */
int fvdb_meta_add_column(fvdb_meta* t, uint32_t* out_column);
/* Cells of one column at the listed slots (strictly ascending): tags[i], vals[i] (session.rs:581-632 update_metadata;
 * the value a path reaches, metadata_filter.rs:360-375).  For an ARRAY cell vals[i] is its LENGTH and its elements are
 * the next vals[i] entries of elem_tags / elem_vals, taken in cell order; n_elems is their total.  A BOOL payload other
 * than 0 or 1 (cell or element) is FVDB_E_INVALID.  Rewriting an ARRAY
 * cell appends its elements and leaves the old ones dead (fvdb_meta_info counts them). */
int fvdb_meta_set_cells(fvdb_meta* t, uint32_t column, const uint32_t* slots, const uint8_t* tags, const uint64_t* vals, uint64_t n,
                        const uint8_t* elem_tags, const uint64_t* elem_vals, uint64_t n_elems);
/* Runs a program over every slot (metadata_filter.rs:265-338 for every row at once).  The matching row ids and the
 * unknown slots stay in buffers the table owns, both in ascending slot order, until the next evaluation;
 * *out_matches / *out_unknown are their counts.  An unknown slot is in neither list of matches: the caller decides it
 * and merges it in.  Returns after the pass has completed. */
int fvdb_meta_eval(fvdb_meta* t, const uint32_t* instrs, uint32_t n_instrs, const uint32_t* const_tags, const uint64_t* const_keys,
                   uint32_t n_consts, uint64_t* out_matches, uint64_t* out_unknown);
/* The last evaluation's results to host memory: ids[matches], unknown_slots[unknown], and unknown_ranks[unknown] = the
 * number of matching slots in front of each unknown slot, which is where a decided one is merged in.  A NULL pointer
 * skips that array.  FVDB_E_INVALID when nothing has been evaluated. */
int fvdb_meta_eval_fetch(fvdb_meta* t, uint64_t* ids, uint32_t* unknown_slots, uint32_t* unknown_ranks);
/* The same three arrays where they are, in HBM, with their counts (any pointer may be NULL): for building a mask
 * without the ids visiting the host.  Valid until the table's next evaluation, growth or destruction. */
int fvdb_meta_eval_dev(fvdb_meta* t, const uint64_t** ids_dev, const uint32_t** unknown_slots_dev, const uint32_t** unknown_ranks_dev,
                       uint64_t* out_matches, uint64_t* out_unknown);
/* The keys of n candidate ids under one column, for fvdb_group_select_dev ("grouped selection" above states the key
 * rule, the id index and the refusals). */
int fvdb_group_keys_of_ids_dev(fvdb_meta* t, uint32_t column, const uint64_t* ids_dev, uint64_t n, uint8_t* out_tag_dev,
                               uint64_t* out_key_dev);
/* The context whose stream carries that lookup (the one the table was made on; NULL for a NULL table): a caller that
 * runs the selection on another stream waits for this one first. */
fvdb_ctx* fvdb_group_keys_ctx(fvdb_meta* t);

#ifdef __cplusplus
}
#endif
#endif /* FVDB_H */
