// fvdb_host.hpp — host-side mirror of the reference's index classes for the hot path.
//
// The reference's host code is Rust (src/ivf/core.rs, src/hnsw/core.rs, src/hybrid/core.rs);
// no Rust toolchain exists here, so the mirror is C++ above the C ABI (include/fvdb.h), with
// the same names, argument meaning and error behaviour.  It owns the index STRUCTURES (lists
// bookkeeping, HNSW graph, heaps, visited sets, routing, timestamps); every distance comes
// from the GPU through the C ABI.  Nothing in here computes a vector distance on the CPU.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/fvdb.h"

namespace fvdbh {

// Documented PRNG for this build's own draws (HNSW levels, k-means++): SplitMix64.
// The reference uses rand 0.8 StdRng whose stream cannot be reproduced here.
struct SplitMix64 {
  uint64_t s;
  explicit SplitMix64(uint64_t seed) : s(seed) {}
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double gen_f64() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

struct Cand {
  uint32_t node;   // node index (HNSW) — ids are resolved at the API boundary
  float distance;
};

// std::collections::BinaryHeap restated (sift_up / sift_down_to_bottom), so exact distance
// ties resolve like the reference's heaps.  Ordering: SearchCandidate::cmp, src/hnsw/core.rs:126-137.
struct RustHeap {
  std::vector<Cand> data;
  static bool le(const Cand& a, const Cand& b) { return a.distance >= b.distance; }
  size_t len() const { return data.size(); }
  bool empty() const { return data.empty(); }
  const Cand& peek() const { return data[0]; }
  void clear() { data.clear(); }
  void sift_up(size_t start, size_t pos);
  void push(Cand c);
  Cand pop();
};

// Open-addressing visited set with O(1) reset.
struct Visited {
  std::vector<uint32_t> keys, stamp;
  uint32_t epoch = 0, used = 0;
  void reset(size_t expect);
  bool insert(uint32_t v);  // true if newly inserted
 private:
  void grow();
};

// "no result" rows of a batch: counts 0, ids FVDB_NO_ID, distances +inf
inline void fill_empty(uint64_t* ids, float* dist, uint32_t* counts, uint32_t B, uint32_t k) {
  for (uint32_t b = 0; b < B; ++b) counts[b] = 0;
  for (size_t i = 0; i < (size_t)B * k; ++i) {
    ids[i] = FVDB_NO_ID;
    dist[i] = __builtin_huge_valf();
  }
}

// the radii of a radius search: each >= 0, +inf allowed; a negative or NaN one is FVDB_E_INVALID
inline int check_radius(const float* radius, uint32_t B) {
  if (B && !radius) return FVDB_E_INVALID;
  for (uint32_t b = 0; b < B; ++b)
    if (!(radius[b] >= 0.0f)) return FVDB_E_INVALID;
  return FVDB_OK;
}

// Grow-only device block and, where the owner asks for one, its pinned host twin of the same size.  reserve() frees and
// reallocates when the block is too small (contents are not kept); the owner's destructor calls release().
struct DevBuf {
  fvdb_ctx* ctx = nullptr;  // the context of the last allocation
  void *dev = nullptr, *host = nullptr;
  uint64_t cap = 0;  // bytes
  int reserve(fvdb_ctx* c, uint64_t bytes, bool pinned) {
    if (bytes <= cap) return FVDB_OK;
    release();
    ctx = c;
    if (fvdb_dev_alloc(c, bytes, &dev) || (pinned && fvdb_host_alloc(c, bytes, &host))) return FVDB_E_OOM;
    cap = bytes;
    return FVDB_OK;
  }
  void release() {
    if (dev) fvdb_dev_free(ctx, dev);
    if (host) fvdb_host_free(ctx, host);
    dev = host = nullptr;
    cap = 0;
  }
};

// Filtered search (include/fvdb.h "allow-set masks"): a device mask shared by the searches that
// use it.  An index keeps the last one it built, keyed by the id list; it is rebuilt when the list differs or the
// device index has changed since (fvdb_mask_info stale).  A search holds its own reference while it runs.
typedef std::shared_ptr<fvdb_mask> MaskRef;
inline MaskRef adopt_mask(fvdb_mask* m) { return MaskRef(m, [](fvdb_mask* p) { fvdb_mask_destroy(p); }); }
inline bool mask_fresh(const MaskRef& m) {
  fvdb_mask_info_t info;
  return m && fvdb_mask_info(m.get(), &info) == FVDB_OK && !info.stale;
}

// The context (stream) of one in-flight slot, made on first use: borrowed from the index (slot 0) or created.
// The allow-sets of one grouped search: G sets laid end to end, set g = ids[off[g] .. off[g + 1]);
// filtered[g] == 0: group g is "no filter" (its range is not read).  group_of_query[B]: the set each query is searched
// under; an entry >= G is FVDB_E_INVALID.
struct AllowGroups {
  const uint64_t* ids;
  const uint64_t* off;      // [G + 1]
  const uint8_t* filtered;  // [G]
  uint32_t G;
  const uint32_t* group_of_query;
  const uint64_t* set(uint32_t g) const { return ids + off[g]; }
  uint64_t size(uint32_t g) const { return off[g + 1] - off[g]; }
  bool valid(uint32_t B) const {
    if (B && !group_of_query) return false;
    if (G && (!off || !filtered)) return false;
    for (uint32_t g = 0; g < G; ++g)
      if (off[g + 1] < off[g] || (filtered[g] && off[g + 1] > off[g] && !ids)) return false;
    for (uint32_t b = 0; b < B; ++b)
      if (group_of_query[b] >= G) return false;
    return true;
  }
};

inline int slot_ctx(fvdb_ctx* base, bool borrow, fvdb_ctx** ctx) {
  if (*ctx) return FVDB_OK;
  if (!borrow) return fvdb_ctx_create(fvdb_ctx_device(base), ctx);
  *ctx = base;
  return FVDB_OK;
}

// Half-precision rows (row_dtype = FVDB_F16 in a config).  An index created with it rounds every
// incoming row to IEEE binary16, to nearest even, ONCE, at the door — insert, batch_insert*, bulk_insert, bulk_build,
// restore, insert_with_timestamp — and is from then on the reference algorithm given the rounded rows: the device
// stores them as fp16 and widens exactly, the host copy holds the same values as f32.  Queries, training data and
// centroids stay f32.  A value whose rounding overflows becomes +-Inf, which the entry point refuses as it refuses any
// non-finite row (FVDB_E_NONFINITE).
//
// round_f16: out[i] = in[i] rounded to binary16 (nearest, ties to even) and widened back; integer arithmetic on the bit
// patterns only.  The doors use it and nothing else does.
void round_f16(const float* in, uint64_t n, float* out);
// the rows as the index keeps them: v itself (FVDB_F32), or the rounded copy in `keep`
inline const float* rows_at_the_door(int row_dtype, const float* v, uint64_t count, std::vector<float>& keep) {
  if (row_dtype != FVDB_F16 || !v || count == 0) return v;
  keep.resize(count);
  round_f16(v, count, keep.data());
  return keep.data();
}

// Exact search and search quality.  SearchQuality: src/ivf/operations.rs SearchQuality.
struct SearchQuality {
  float avg_recall, avg_precision, avg_query_time_ms;
  uint64_t queries_evaluated;
};
// from the sums over B queries; avg_query_time_ms is the wall time since `start` over B
inline SearchQuality quality_of(float total_recall, float total_precision, uint32_t B, std::chrono::steady_clock::time_point start) {
  const std::chrono::duration<float, std::milli> elapsed = std::chrono::steady_clock::now() - start;
  return {total_recall / (float)B, total_precision / (float)B, elapsed.count() / (float)B, B};
}
// Two B x k id blocks with their hit counts compared per query on the device (fvdb_search_quality_lists_dev: the
// reference's matches / recall / precision, src/ivf/operations.rs:357-377); the per-query f32 values are summed here in
// query order, as IVFIndex::evaluate_search_quality sums them.  The node -> id mapping and the hybrid merge live in
// this mirror, so the two blocks go down to `stage` first (16 B k + 8 B bytes).
int compare_id_blocks(fvdb_ctx* ctx, DevBuf& stage, uint32_t B, uint32_t k, const uint64_t* res_ids, const uint32_t* res_counts,
                      const uint64_t* truth_ids, const uint32_t* truth_counts, float* total_recall, float* total_precision);

// Search quality over a grid of (ef, n_probe) from one exact search.  avg_recall / avg_precision:
// [rows][cols] row-major, entry (i, j) what evaluate_search_quality returns at (efs[i], n_probes[j]), bit for bit.
struct QualityGrid {
  uint32_t rows = 0, cols = 0;
  std::vector<float> avg_recall, avg_precision;
  float avg_query_time_ms = 0.0f;  // wall time of the call over B
  uint64_t queries_evaluated = 0;
};
// The parts of a grid on the host, as the searches returned them: the truth's ids [B][k], the recent parts
// [E][B][rk] and the historical parts [P][B][hk] (distances ascending), each with its hit counts.  E == 0 or P == 0:
// that part is absent and its pointers are not read (not both).
struct GridParts {
  uint32_t B, k;
  const uint64_t* tid;
  const uint32_t* tcn;
  uint32_t E, rk;
  const uint64_t* rid;
  const float* rd;
  const uint32_t* rcn;
  uint32_t P, hk;
  const uint64_t* hid;
  const float* hd;
  const uint32_t* hcn;
  uint32_t rows() const { return E ? E : 1; }
  uint32_t cols() const { return P ? P : 1; }
  // bytes one query adds to a sub-batch: its staged lists with their counts, its rows() x cols() pairs of figures, and
  // the prefix counts the engine keeps per list entry (fvdb_quality_grid_dev)
  uint64_t bytes_per_query() const {
    return (uint64_t)k * 8 + 4 + (uint64_t)E * ((uint64_t)rk * 16 + 8) + (uint64_t)P * ((uint64_t)hk * 16 + 8) +
           (uint64_t)rows() * cols() * 8;
  }
};
constexpr uint64_t kQualityGridBytes = 256ull << 20;
// the budget of a call: kQualityGridBytes unless FVDB_QUALITY_GRID_BYTES says otherwise (read at every call)
uint64_t quality_grid_budget();
// queries of a sub-batch: as many as fit the budget, at least one, at most B
inline uint32_t quality_grid_step(uint64_t budget, const GridParts& p) {
  const uint64_t fit = budget / p.bytes_per_query();
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(fit, 1), p.B);
}
// The parts go down to `stage` in sub-batches of quality_grid_step queries, one fvdb_quality_grid_dev call each; the
// per-query figures come back and are added to total_recall / total_precision [rows() * cols()] in query order, in f32,
// as compare_id_blocks adds them: the totals do not depend on the budget.
int quality_grid_totals(fvdb_ctx* ctx, DevBuf& stage, const GridParts& p, float* total_recall, float* total_precision);

// Diverse search (fvdb_mmr_select_dev): the candidates of an ordinary search of fetch_k, their rows
// gathered in HBM into a staging block, k of them selected per query by maximal marginal relevance.
// check_diverse: the refusals every search_diverse makes first, in fvdb_mmr_select_dev's order.
inline int check_diverse(uint32_t k, uint32_t fetch_k, float lam) {
  if (fetch_k == 0 || fetch_k > FVDB_MAX_K) return FVDB_E_UNSUPPORTED;
  if (k == 0 || k > fetch_k || !(lam >= 0.0f && lam <= 1.0f)) return FVDB_E_INVALID;
  return FVDB_OK;
}
// "no result" rows of a diverse search: fill_empty and ranks of FVDB_NO_ROW
inline void fill_empty_diverse(uint64_t* ids, float* dist, uint32_t* ranks, uint32_t* counts, uint32_t B, uint32_t k) {
  fill_empty(ids, dist, counts, B, k);
  for (size_t i = 0; i < (size_t)B * k; ++i) ranks[i] = FVDB_NO_ROW;
}
// The staging block [queries][fetch_k][dim rounded up to 4] f32 is capped at kDiverseStageBytes (FVDB_DIVERSE_STAGE_BYTES,
// read once, says otherwise): a batch is walked in sub-batches of as many queries as fit, at least one.
// set_diverse_stage_budget(bytes) overrides both for the process (0: back to the environment's value or the default).
constexpr uint64_t kDiverseStageBytes = 256ull << 20;
uint64_t diverse_stage_budget();
void set_diverse_stage_budget(uint64_t bytes);
struct DiverseStage {
  std::mutex mu;  // one block per index: selections take turns
  DevBuf rows;    // the staging block
  DevBuf io;      // per sub-batch: candidate ids, distances, counts and row locations in; picks out (pinned twin)
  void release() {
    rows.release();
    io.release();
  }
};
// Fills staging rows [0, n) of a sub-batch on ctx's stream: candidate i (ids[i], wanted where want[i] != 0) goes to
// rows_dev + i * stride; `loc_dev` is room for n uint32_t in device memory, `want` is cleared where a row was found.
struct RowSource {
  virtual int gather(fvdb_ctx* ctx, const uint64_t* ids, uint8_t* want, uint64_t n, uint32_t* loc_dev, float* rows_dev,
                     uint32_t stride) = 0;
  virtual ~RowSource() {}
};
// cid / cd [B][fetch_k] and cc[B]: what the search of fetch_k returned (host memory).  Results [B][k] in pick order.
// FVDB_E_NOT_FOUND when a candidate's row is in no source.
int select_diverse(fvdb_ctx* ctx, DiverseStage& st, RowSource& src, uint32_t dim, uint32_t B, uint32_t fetch_k, uint32_t k,
                   float lam, bool distinct, const uint64_t* cid, const float* cd, const uint32_t* cc, uint64_t* ids, float* dist,
                   uint32_t* ranks, uint32_t* counts);

// Grouped search (fvdb_group_keys_of_ids_dev, fvdb_group_select_dev): the candidates of an ordinary
// search of fetch_k, their keys under one column of a metadata table looked up in HBM, the first k groups with
// group_size members each selected per query.  The class searches hand their candidates back in host memory, so one
// upload of ids, distances and counts per sub-batch goes down; keys never visit the host.
struct GroupBy {
  fvdb_meta* table;      // the metadata table and the column whose cells are the keys
  uint32_t column;
};
struct GroupedOut {      // host arrays, as fvdb_group_select_dev lays them out
  uint64_t* ids;         // [B][k][group_size]
  float* dist;
  uint32_t* ranks;
  uint32_t* members;     // [B][k]
  uint32_t* totals;
  uint8_t* key_tags;
  uint64_t* key_vals;
  uint32_t* groups;      // [B]
  uint32_t* flags;
};
constexpr uint64_t kGroupedStageBytes = 64ull << 20;  // device block of one sub-batch: as many queries as fit, at least one
// the refusals every search_grouped makes first, in fvdb_group_select_dev's order
inline int check_grouped(uint32_t fetch_k, uint32_t k, uint32_t group_size, int missing) {
  if (fetch_k == 0 || fetch_k > FVDB_MAX_K_WIDE) return FVDB_E_UNSUPPORTED;
  if (k == 0 || group_size == 0) return FVDB_E_INVALID;
  if ((uint64_t)k * group_size > FVDB_MAX_K_WIDE) return FVDB_E_UNSUPPORTED;
  if (missing != FVDB_GROUP_MISSING_DROP && missing != FVDB_GROUP_MISSING_OWN) return FVDB_E_INVALID;
  return FVDB_OK;
}
void fill_empty_grouped(const GroupedOut& out, uint32_t B, uint32_t k, uint32_t group_size);
// cid / cd [B][fetch_k] and cc[B]: what the search of fetch_k returned (host memory)
int select_grouped(fvdb_ctx* ctx, const GroupBy& by, uint32_t B, uint32_t fetch_k, uint32_t k, uint32_t group_size, bool distinct,
                   int missing, const uint64_t* cid, const float* cd, const uint32_t* cc, const GroupedOut& out);

// ------------------------------------------------------------------------------------------
// IVFIndex — src/ivf/core.rs, src/ivf/operations.rs
// ------------------------------------------------------------------------------------------
struct IVFConfig {
  uint32_t n_clusters = 256, n_probe = 16, train_size = 10000, max_iterations = 25;  // :50-60
  uint64_t seed = 0;
  int row_dtype = FVDB_F32;  // storage of the lists' rows (no counterpart in the reference)
  bool is_valid() const { return n_clusters > 0 && n_probe > 0 && n_probe <= n_clusters && train_size > 0 && max_iterations > 0; }
};

class IVFIndex {
 public:
  IVFIndex(fvdb_ctx* ctx, const IVFConfig& cfg);
  ~IVFIndex();
  const IVFConfig& config() const { return cfg_; }
  bool is_trained() const { return trained_; }
  uint32_t dimension() const { return dim_; }
  uint64_t total_vectors() const { return total_; }
  int train(const float* data, uint64_t n, uint32_t dim, fvdb_train_result* out);  // :240
  int set_trained(const float* centroids, uint32_t dim);                          // :509
  int get_centroids(float* out) const;
  int insert(uint64_t id, const float* v, uint32_t dim);                          // :431
  // batch_insert (operations.rs:107-130): sequential semantics, one GPU assignment pass.
  int batch_insert(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, uint64_t* n_ok, int* first_error);
  // rows whose list is already known (load path / shard placement)
  int batch_insert_assigned(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const uint32_t* clusters,
                            uint64_t* n_ok, int* first_error);
  // batch_insert with the rows taken from a row store in HBM (rows[i] = store row of ids[i]) instead of the host: the
  // same per-row outcome (the duplicate checks of place(), live_again_), the same lists.  Only the kept rows' indices,
  // ids and clusters cross the host link (fvdb_ivf_assign_from_store / fvdb_ivf_add_assigned_from_store).
  int batch_insert_from_store(const uint64_t* ids, fvdb_store* store, const uint32_t* rows, uint64_t n, uint64_t* n_ok,
                              int* first_error);
  int assign(const float* v, uint64_t n, uint32_t dim, uint32_t* out);
  // Rows by id (get_vector_by_id, src/ivf/core.rs:553-562), read back from HBM with one device gather for the whole
  // batch (fvdb_ivf_get_rows).  An id may sit in several lists (the duplicate check is per list): the LOWEST (cluster,
  // position) is taken.  The reference walks a HashMap of lists and returns the first copy it meets, so any of them
  // is one of its outcomes.  A soft-deleted id still returns its row (:553-562 do not look at the deleted set).
  int get_vector_by_id(uint64_t id, float* out);  // FVDB_E_NOT_FOUND when no list holds the id
  // found[i] = 1 and out row i (dimension() floats) filled, or found[i] = 0 and the row untouched
  int get_vectors(const uint64_t* ids, uint64_t n, float* out, uint8_t* found);
  int find_cluster(const float* v, uint32_t dim, uint32_t* out);                  // :493
  int search(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t n_probe, uint64_t* ids, float* dist,
             uint32_t* counts);                                                   // :626, operations.rs:132
  // same with the queries already resident in HBM (B x d row-major); outputs are device pointers
  // `on` / `slot`: run on another context's stream with that slot's scratch set (several searches in flight)
  int search_dev(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, uint32_t n_probe, uint64_t* ids_dev,
                 float* dist_dev, uint32_t* counts_dev, fvdb_ctx* on = nullptr, uint32_t slot = 0);
  // search under an allow-set: what search() returns after mark_deleted of every id outside allowed[n_allowed]
  int search_allowed(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t n_probe, const uint64_t* allowed,
                     uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts);
  // one allow-set per query: query b gets what search_allowed returns for it under the set of
  // group_of_query[b], or what search returns where that group is "no filter".  One device call
  // (fvdb_ivf_search_groups_dev_slot); the masks are built for this call, counted by mask_builds, and dropped when the
  // results are in — the cached mask of search_allowed is left alone.
  int search_allowed_groups(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t n_probe, const AllowGroups& groups,
                            uint64_t* ids, float* dist, uint32_t* counts);
  // Radius search (fvdb_ivf_search_radius): per query the live rows of the n_probe probed lists
  // whose distance word is <= bits(radius[b]), the first min(total, max_results) of them in the wide search's order —
  // search(k = max_results, n_probe) on the wide route, cut at the radius — and totals[b] = their exact number, over
  // the probed lists only.  radius[B] in host memory, each >= 0 (+inf allowed), else FVDB_E_INVALID; max_results in
  // 1..FVDB_MAX_K_WIDE.  allowed != nullptr: under that allow-set (the cached mask of search_allowed), rows outside it in
  // neither results nor totals.
  int search_radius(const float* q, uint32_t B, uint32_t dim, const float* radius, uint32_t max_results, uint32_t n_probe,
                    const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts, uint32_t* totals);
  // Diverse search: the candidates are exactly what search(fetch_k, n_probe) — search_allowed when
  // allowed != nullptr — returns; k of them per query by fvdb_mmr_select_dev, in pick order, ranks[B][k] = each pick's
  // position among the candidates.  1 <= k <= fetch_k <= FVDB_MAX_K, lam in [0, 1].
  int search_diverse(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t fetch_k, float lam, bool distinct,
                     uint32_t n_probe, const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* ranks,
                     uint32_t* counts);
  // the rows of ids[n] (where want[i]) by the lowest location of each, gathered on ctx's stream (RowSource::gather)
  int gather_rows_dev(fvdb_ctx* ctx, const uint64_t* ids, uint8_t* want, uint64_t n, float* rows_dev, uint32_t stride);
  // the device mask for that allow-set (cached); search_dev under it
  int allowed_mask(const uint64_t* allowed, uint64_t n_allowed, MaskRef* out);
  int search_dev_masked(const MaskRef& mask, const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, uint32_t n_probe,
                        uint64_t* ids_dev, float* dist_dev, uint32_t* counts_dev, fvdb_ctx* on = nullptr, uint32_t slot = 0);
  uint64_t mask_builds() const { return mask_builds_; }
  int mark_deleted(uint64_t id);                                                  // operations.rs:569
  bool is_deleted(uint64_t id) const { return deleted_.count(id) > 0; }
  uint64_t active_count() const { return total_ - deleted_.size(); }
  uint64_t deleted_count() const { return deleted_.size(); }
  int vacuum(uint64_t* removed);                                                  // operations.rs:625
  // Re-partitioning (operations.rs:148-260).  The rows stay in HBM: a new device index is trained on the old one's
  // rows in sequence order (lists ascending, list-position order inside: this project's outcome of the reference's
  // walk over `inverted_lists.values()`), every row is re-inserted in that order, and the old device index is destroyed.
  struct RetrainResult {  // operations.rs RetrainResult
    uint64_t old_clusters, new_clusters, vectors_reassigned, converged;
  };
  struct ClusterStats {  // operations.rs:263-288
    uint64_t n_clusters, total_vectors, empty_clusters;
    float avg_cluster_size, size_variance;
  };
  int retrain(const IVFConfig& new_config, RetrainResult* out);                   // operations.rs:148-193
  int add_clusters(uint32_t n_clusters_to_add, uint64_t* vectors_reassigned);     // operations.rs:195-220
  int optimize_clusters(uint32_t* iterations, float* improvement);                // operations.rs:222-260
  ClusterStats get_cluster_stats() const;                                         // operations.rs:263-288
  // evaluate_search_quality (operations.rs:329-391): the configured n_probe against the search of every list in
  // centroid-rank order, per query on the device (fvdb_ivf_search_quality_dev); the per-query values are summed here
  // in query order, in f32, as the reference's `total_recall += recall`.  avg_query_time_ms is the wall time of the
  // call over B (the reference times each query by itself).  B == 0 is FVDB_E_INVALID (:334-338).
  typedef fvdbh::SearchQuality SearchQuality;  // operations.rs SearchQuality
  int evaluate_search_quality(const float* q, uint32_t B, uint32_t dim, uint32_t k, SearchQuality* out);
  // The same figures at every n_probe = 1 .. n_clusters from ONE search of every list (fvdb_ivf_quality_curve_dev,
  // DESIGN.md section 9m): avg_recall[p - 1] / avg_precision[p - 1] are what evaluate_search_quality would return with
  // n_probe = p configured, bit for bit, provided no id is stored in two lists (otherwise rows are counted, not ids).
  // allowed != nullptr: under that allow-set (the cached mask of search_allowed), "live" meaning allowed and live.
  // evaluate_search_quality's refusals in its order.
  struct QualityCurve {
    std::vector<float> avg_recall, avg_precision;  // [n_clusters]
    float avg_query_time_ms = 0.0f;                // wall time of the call over B
    uint64_t queries_evaluated = 0;
  };
  int quality_curve(const float* q, uint32_t B, uint32_t dim, uint32_t k, const uint64_t* allowed, uint64_t n_allowed,
                    QualityCurve* out);
  uint64_t cluster_size(uint32_t c) const;
  // list `c` in list-position order, copied back from HBM (save path, src/hybrid/persistence.rs:289-311)
  int export_list(uint32_t c, float* rows, uint64_t* ids, uint8_t* live) const;
  void clear_lists();                                                             // hybrid initialize :278-287
  fvdb_ivf* device() { return dev_; }

 private:
  struct Loc {
    uint32_t cluster, pos;
  };
  int ensure_device(uint32_t dim);
  float size_variance() const;                                                    // operations.rs:552-563
  // the shared body of retrain and optimize_clusters: train a new device index of `n_clusters` lists on the rows of
  // the present one and re-insert them; `reinserted` counts the rows that went in (all, or those before a duplicate)
  int rebuild(uint32_t n_clusters, uint32_t max_iterations, uint64_t seed, fvdb_train_result* tr, uint64_t* reinserted);
  int place(const uint64_t* ids, const float* v, uint64_t n, const uint32_t* clusters, uint64_t* n_ok, int* first_error);
  // the per-list duplicate check of place(): the indices of the rows that go in, in order (live_again_ noted)
  std::vector<uint64_t> accept(const uint64_t* ids, uint64_t n, const uint32_t* clusters, int* first_error);
  fvdb_ctx* ctx_;
  IVFConfig cfg_;
  fvdb_ivf* dev_ = nullptr;
  uint32_t dev_clusters_ = 0;  // lists of dev_; differs from cfg_.n_clusters only after a retrain whose training failed
  uint32_t dim_ = 0;
  bool trained_ = false;
  bool live_again_ = false;    // a row was inserted under an id that is in deleted_: its live bit is set (vacuum)
  uint64_t total_ = 0;
  std::unordered_multimap<uint64_t, Loc> where_;  // id -> every list position holding it
  std::unordered_set<uint64_t> deleted_;
  std::mutex mask_mu_;  // the cached mask: several search threads may ask at once
  std::vector<uint64_t> mask_key_;
  MaskRef mask_;
  uint64_t mask_builds_ = 0;
  std::mutex allowed_mu_;           // search_allowed's staging blocks
  // search_allowed: staged queries, result block and its pinned copy; evaluate_search_quality stages its queries and
  // its per-query figures in the same pair, under the same mutex
  DevBuf allowed_q_, allowed_out_;
  DiverseStage diverse_;
  void drop_mask() {
    mask_.reset();
    mask_key_.clear();
  }
};

// ------------------------------------------------------------------------------------------
// HNSWIndex — src/hnsw/core.rs, src/hnsw/operations.rs
// ------------------------------------------------------------------------------------------
struct HNSWConfig {
  uint32_t max_connections = 16, max_connections_layer_0 = 32, ef_construction = 200;  // :37-46
  uint64_t seed = 0;
  int row_dtype = FVDB_F32;  // storage of the graph's rows (no counterpart in the reference)
};

class HNSWIndex {
 public:
  // Filtered search.  AllowView = the allow-set as this index sees it: the device mask over node indices and the host
  // copy of the same flags (deleted | not allowed, per node) for the queries the traversal hands back to the host walk.
  struct AllowView {
    MaskRef mask;
    std::vector<uint8_t> eff;
    uint64_t allowed_live = 0;
  };
  typedef std::shared_ptr<const AllowView> ViewRef;
  HNSWIndex(fvdb_ctx* ctx, const HNSWConfig& cfg);
  ~HNSWIndex();
  const HNSWConfig& config() const { return cfg_; }
  uint64_t node_count() const { return n_registered_; }
  bool entry_point(uint64_t* id) const;
  uint32_t dimension() const { return dim_; }
  size_t assign_level();                                                           // :211
  int insert(uint64_t id, const float* v, uint32_t dim, int64_t forced_level);     // :226
  // batch_insert (src/hnsw/operations.rs:74-94): the reference's sequential loop, keeps going after a failure.
  // levels[i] < 0 (or levels == nullptr): drawn with assign_level() in order, like the loop would.  The inserts that
  // pass the reference's checks are linked on the device in one call (fvdb_graph_insert_linked), strictly in order.
  int batch_insert(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const int64_t* levels, uint64_t* n_ok,
                   int* first_error);
  // Where an insert's searches, links and prunes run: true (default) = on the device against the adjacency in HBM
  // (kernels_graph_build.h); false = the host algorithm with every distance batch scored on the GPU (fvdb_scorer_*).
  // Same graph either way.  mode: fvdb_graph_insert_linked's (0 choose, 1 one at a time, 2 speculate batches).
  void set_device_insert(bool on, int mode = 0) {
    device_insert_ = on;
    insert_mode_ = mode;
  }
  bool device_insert() const { return device_insert_; }
  // `visited` of the device insert's searches (src/hnsw/core.rs:469-554): fvdb_graph_set_insert_visited's mode (0 = a
  // bitmap over all nodes while the graph fits it, a hashed set beyond; 1 = bitmap only; 2 = hashed always) and table size.
  // Same graph whichever form.  insert_info: fvdb_graph_insert_info for this index's ef_construction (FVDB_E_NOT_FOUND
  // before the device graph exists, i.e. before the first insert or search).
  int set_insert_visited(int mode, uint32_t table_slots = 0);
  int insert_info(fvdb_graph_insert_info_t* out);
  const fvdb_graph_insert_stats& insert_stats() const { return insert_stats_; }  // sums since construction
  uint64_t host_path_inserts() const { return n_host_inserts_; }
  uint64_t graph_upload_bytes() const { return graph_ ? fvdb_graph_upload_bytes(graph_) : 0; }
  // the device graph as the searches see it (brought up to date first), for callers that drive the C ABI themselves
  fvdb_graph* device_graph() { return sync_graph() == FVDB_OK ? graph_ : nullptr; }
  // ---- search ----
  // One graph search, stated once: every entry point below fills one in and hands it on.  Where two entry points
  // differ, they differ in these fields.
  struct Search {
    enum Kind { kTraversal, kExact } kind;  // the layered walk (src/hnsw/core.rs:398-467) / the flat scan of every live row
    const float* q;                         // B x dim queries, row-major ...
    bool q_on_device;                       // ... in HBM, or in host memory
    uint32_t B, dim, k, ef;
    uint64_t* ids;                          // B x k results to host memory (null at a begin, which delivers nothing)
    float* dist;
    uint32_t* counts;
    const AllowView* view = nullptr;        // under this allow-set, or (by_list) under allowed[n_allowed]: admit() gets the view
    bool by_list = false;
    const uint64_t* allowed = nullptr;
    uint64_t n_allowed = 0;
    uint32_t slot = 0;                      // stream, scratch set and result block
    bool wide = false;                      // kExact only: k up to FVDB_MAX_K_WIDE, fvdb_graph_search_flat_wide_dev_slot
    bool owns_slot = false;                // the caller holds `slot` for the call (HybridIndex's lease): run() takes no lock
    // kExact + wide, radius search: the rows within radius[b] (host memory, checked by the entry
    // point), at most k of them, and the size of each ball to totals[B]; count_only: the sizes alone (k = 1, no ids)
    const float* radius = nullptr;
    uint32_t* totals = nullptr;
    bool count_only = false;
    // filled in by admit() and stage()
    ViewRef held = nullptr;                 // keeps a by_list view alive
    enum Route { kAnswered, kHostWalk, kDevice } route = kAnswered;
    bool scanned = false;                   // kDevice by a scan: the result block carries no status words
    const float* q_dev = nullptr;           // the queries in HBM
  };
  // Blocking searches, results to host memory.  They run in slot 0 and take turns (search_mu_); what each answers
  // before it reaches the device is the table in DESIGN.md section 9l.
  int search(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, uint64_t* ids, float* dist,
             uint32_t* counts);                                                    // :398 (batched, lock-step hops)
  int search_dev(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, uint64_t* ids, float* dist,
                 uint32_t* counts);  // the queries resident in HBM
  // search under an allow-set: what search() returns after mark_deleted of every id outside it — unless the allowed
  // live nodes number at most scan_cutoff(): then they are scanned exactly (best k by distance bits, then node index)
  int search_allowed(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, const uint64_t* allowed,
                     uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts);
  int allowed_view(const uint64_t* allowed, uint64_t n_allowed, ViewRef* out);  // cached like IVFIndex::allowed_mask
  // One allow-set per query: query b gets what search_allowed returns for it under the set of
  // group_of_query[b] (search, where that group is "no filter").  The views are built for this call and dropped after
  // it; the cached one is left alone.  The queries of every group that scans(view, k) share ONE grouped scan
  // (fvdb_graph_scan_allowed_groups_dev_slot); each other group is one masked traversal of its own queries, the
  // unfiltered ones one plain traversal.  Blocking, in slot 0 under search_mu_ — or, owns_slot, in a slot the caller holds.
  int search_allowed_groups(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, const AllowGroups& groups,
                            uint64_t* ids, float* dist, uint32_t* counts, uint32_t slot = 0, bool owns_slot = false);
  // The split form, so that several batches can be in flight: begin enqueues the launch and the result copy on the
  // slot's own stream (slot < kSlots) and returns whether it did; the slot remembers.  end, given the same arguments,
  // waits for that slot and finishes on the host — or, when nothing was enqueued (the checks answered the search, it
  // has to use the host walk, the launch failed: *rc), runs the blocking search now, in slot 0.  A caller that makes
  // the blocking call itself after a begin that returned false gets the same.  `view` (optional): masked traversal, or
  // the scan of the allowed nodes when scans(view, k) — a device kernel whatever set_device_traversal says.
  static constexpr uint32_t kSlots = 16;
  bool search_dev_begin(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, int* rc, uint32_t slot = 0,
                        const AllowView* view = nullptr);
  int search_dev_end(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, uint64_t* ids, float* dist,
                     uint32_t* counts, uint32_t slot = 0, const AllowView* view = nullptr);
  // Exact search (no counterpart in the reference): the k nearest live nodes by (distance bits,
  // node index), every live row of the store scored by the flat scan (fvdb_graph_search_flat_dev_slot); node indices
  // map to ids as search() maps them.  _allowed: under that allow-set, through the cached view.
  // k in 1..FVDB_MAX_K (FVDB_E_UNSUPPORTED otherwise).  It still answers after the entry point was vacuumed away.
  int search_exact(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint64_t* ids, float* dist, uint32_t* counts);
  int search_exact_allowed(const float* q, uint32_t B, uint32_t dim, uint32_t k, const uint64_t* allowed, uint64_t n_allowed,
                           uint64_t* ids, float* dist, uint32_t* counts);
  // the same with the queries in HBM and the slot chosen by the caller, who owns that slot for the call (HybridIndex)
  int search_exact_dev(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, const AllowView* view, uint64_t* ids,
                       float* dist, uint32_t* counts, uint32_t slot);
  // search(k, ef) against search_exact(k): the reference's recall / precision (src/ivf/operations.rs:329-391 applied
  // to the graph).  B == 0 is FVDB_E_INVALID.
  int evaluate_search_quality(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, SearchQuality* out);
  // The same four with k in 1..FVDB_MAX_K_WIDE: the rows scored by the same fold, the k best
  // chosen by the wide selection (fvdb_graph_search_flat_wide_dev_slot) — at k <= FVDB_MAX_K exactly what the calls
  // above return.  They replace nothing above: search_exact and its kin keep their limit, as fvdb_ivf_search kept its
  // own when fvdb_ivf_search_wide arrived.  evaluate_search_quality_wide: search(k, ef) returns at most ef rows.
  int search_exact_wide(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint64_t* ids, float* dist, uint32_t* counts);
  int search_exact_wide_allowed(const float* q, uint32_t B, uint32_t dim, uint32_t k, const uint64_t* allowed, uint64_t n_allowed,
                                uint64_t* ids, float* dist, uint32_t* counts);
  int search_exact_wide_dev(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, const AllowView* view, uint64_t* ids,
                            float* dist, uint32_t* counts, uint32_t slot);
  int evaluate_search_quality_wide(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, SearchQuality* out);
  int quality_impl(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, SearchQuality* out, bool wide);  // both forms
  // Radius search (fvdb_graph_search_flat_radius_dev_slot): per query the live nodes whose distance
  // word is <= bits(radius[b]) — radius[B] in host memory, each >= 0, +inf allowed; a negative or NaN one is
  // FVDB_E_INVALID — the first min(total, max_results) of them by (distance bits, node index), which is
  // search_exact_wide(k = max_results) cut at the radius, and totals[b] = their exact number.  Nodes map to ids as
  // search_exact_wide maps them.  max_results in 1..FVDB_MAX_K_WIDE.  _allowed: under that allow-set (the cached view),
  // rows outside it in neither results nor totals.  count_within: totals alone, by a scan that keeps no distances
  // (fvdb_graph_count_within_dev_slot); allowed == nullptr: no filter.  _dev: queries in HBM, the caller's slot.
  int search_radius(const float* q, uint32_t B, uint32_t dim, const float* radius, uint32_t max_results, uint64_t* ids, float* dist,
                    uint32_t* counts, uint32_t* totals);
  int search_radius_allowed(const float* q, uint32_t B, uint32_t dim, const float* radius, uint32_t max_results,
                            const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts, uint32_t* totals);
  int count_within(const float* q, uint32_t B, uint32_t dim, const float* radius, const uint64_t* allowed, uint64_t n_allowed,
                   uint32_t* totals);
  int search_radius_dev(const float* q_dev, uint32_t B, uint32_t dim, const float* radius, uint32_t max_results, const AllowView* view,
                        uint64_t* ids, float* dist, uint32_t* counts, uint32_t* totals, uint32_t slot);
  // Diverse search: the candidates are exactly what search(fetch_k, ef) — search_allowed when
  // allowed != nullptr — returns.  A graph walk returns at most ef rows, so fetch_k > ef just yields fewer candidates.
  // k of them per query by fvdb_mmr_select_dev, in pick order; 1 <= k <= fetch_k <= FVDB_MAX_K, lam in [0, 1].
  int search_diverse(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t fetch_k, float lam, bool distinct, uint32_t ef,
                     const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* ranks, uint32_t* counts);
  // the rows of ids[n] (where want[i]) from the row store, gathered on ctx's stream (RowSource::gather)
  int gather_rows_dev(fvdb_ctx* ctx, const uint64_t* ids, uint8_t* want, uint64_t n, uint32_t* loc_dev, float* rows_dev,
                      uint32_t stride);
  // evaluate_search_quality (its wide form above k = FVDB_MAX_K) at every listed ef from ONE exact search (DESIGN.md
  // section 9r): one search(k, efs[i]) each, one fvdb_quality_grid_dev call per sub-batch.  out: E x 1, entry i what
  // the single call returns at efs[i], bit for bit; duplicates and any order are fine.  Refused before any search
  // runs, in this order: B == 0, a null pointer or E == 0 FVDB_E_INVALID; k == 0, k > FVDB_MAX_K_WIDE or E > 64
  // FVDB_E_UNSUPPORTED; a dimension mismatch FVDB_E_DIM.  An ef the search refuses: that search's code.
  int quality_by_ef(const float* q, uint32_t B, uint32_t dim, uint32_t k, const uint32_t* efs, uint32_t E, QualityGrid* out);
  // 0 = never scan, UINT64_MAX = always.  The default is a guess nobody has measured.
  void set_scan_cutoff(uint64_t nodes) { scan_cutoff_ = nodes; }
  uint64_t scan_cutoff() const { return scan_cutoff_; }
  bool scans(const AllowView& v, uint32_t k) const { return v.allowed_live <= scan_cutoff_ && k <= FVDB_MAX_K; }
  uint64_t mask_builds() const { return mask_builds_; }
  int mark_deleted(uint64_t id);                                                   // operations.rs:127
  bool is_deleted(uint64_t id) const;
  uint64_t active_count() const;
  // vacuum (operations.rs:176): deleted nodes leave every neighbour list and the node map.  With a device graph the
  // whole operation is one device job (fvdb_graph_vacuum) that also renumbers the survivors densely, in their old
  // order, and gives the dropped nodes' store rows and adjacency back; this mirror compacts its own arrays by the same
  // rule.  The host algorithm (pull the lists, filter, install the whole graph at the next device use; rows kept)
  // serves an index that has no device graph yet, set_resident_vacuum(false), and a graph the device cannot hold
  // (a list longer than 64).  If the compacted copy cannot be allocated, or the entry point is among the deleted (the
  // index then stays in the reference's entry-lost state, entry_point() still naming the removed id), the job prunes in
  // place and keeps the rows (FVDB_VACUUM_KEEP_ROWS); a later vacuum reclaims them.  *removed: the reference's count.
  int vacuum(uint64_t* removed);
  uint64_t vacuum() {  // the reference's signature; a failure reads as 0
    uint64_t r = 0;
    return vacuum(&r) == FVDB_OK ? r : 0;
  }
  void set_resident_vacuum(bool on) { resident_vacuum_ = on; }
  bool resident_vacuum() const { return resident_vacuum_; }
  void set_vacuum_keep_rows(bool on) { vacuum_keep_rows_ = on; }  // A/B and tests: the resident job without the reclaim
  // the last vacuum that removed something: which path it took and, for a resident one, the job's figures
  enum VacuumPath : int { VACUUM_NONE = 0, VACUUM_RESIDENT = 1, VACUUM_RESIDENT_KEEP_ROWS = 2, VACUUM_HOST = 3 };
  int vacuum_info(fvdb_graph_maintenance_info_t* out) const {
    *out = vacuum_info_;
    return vacuum_path_;
  }
  // ---- graph stats and health ----
  // get_graph_stats (operations.rs:227-272) over the live nodes, its stub component count included ("assume 1
  // component"); get_max_level / get_level_distribution (core.rs:667-684) over every node the map holds, deleted or not.
  struct GraphStats {
    uint64_t total_nodes = 0, total_edges = 0;
    float avg_degree = 0.0f;
    uint64_t max_layer = 0, connected_components = 0;
  };
  int get_graph_stats(GraphStats* out);
  uint32_t get_max_level() const;
  void get_level_distribution(uint64_t* out) const;  // get_max_level() + 1 entries
  // What the stub does not say (definitions: include/fvdb.h, fvdb_graph_health): which live nodes a search can still
  // reach, the weak components of the live layer-0 graph, degree and dangling-link figures.  One device job on the
  // adjacency in HBM (brought up to date first); the same definitions restated on the host over nbrs_ when device
  // traversal is off, the index is empty or the device cannot hold the graph (a list longer than 64).  flags:
  // FVDB_HEALTH_SKIP_*.  A node the map no longer holds (a vacuum that kept its rows) is no node for any figure; an entry
  // point lost to a vacuum leaves R empty.  Returns the job's or the pull's error; *path: which form ran.
  enum HealthPath : int { HEALTH_NONE = 0, HEALTH_DEVICE = 1, HEALTH_HOST = 2 };
  int graph_health(fvdb_graph_health_t* out, uint32_t flags = 0, int* path = nullptr);
  // ids of the live nodes outside R, in node order; runs the reach part
  int unreachable(std::vector<uint64_t>* ids_out);
  // per node the map holds, in export_graph's order: the id of the smallest-index node of its layer-0 component
  // (UINT64_MAX for a deleted node); runs the components part.  Room for node_count() entries.
  int component_labels(uint64_t* labels_out);
  uint64_t store_rows() const { return store_ ? fvdb_store_rows(store_) : 0; }  // rows the vectors occupy in HBM
  uint64_t store_bytes() const { return store_ ? fvdb_store_bytes(store_) : 0; }  // and their bytes
  int64_t level_of(uint64_t id) const;
  int64_t neighbors(uint64_t id, uint32_t layer, uint64_t* out, uint64_t cap);
  const float* vector_of(uint64_t id) const;  // host copy (migration, get_vector_by_id)
  // batch form of vector_of: found[i] = 1 and out row i filled, or found[i] = 0 and the row untouched
  void get_vectors(const uint64_t* ids, uint64_t n, float* out, uint8_t* found) const;
  // The row store behind the graph, and the row of a node in it: the node index (resident migration).  false when the
  // id is not a node or the store does not hold its row.
  fvdb_store* store() const { return store_; }
  bool store_row_of(uint64_t id, uint32_t* row) const;
  bool contains(uint64_t id) const { return index_of_.count(id) > 0; }
  // Extension (not in the reference): build the graph for n vectors at once.  Levels from the PRNG
  // (or given); per layer every member links to its exact nearest M (M0 on layer 0) members, found
  // with the GPU flat scan — the graph nearest-M selection (:556-558, :588-624) converges to.
  int bulk_build(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const int64_t* levels);
  // Install / export a graph (identical structures for parity runs).
  int restore(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const uint32_t* levels,
              const uint64_t* nbr_offsets, const uint64_t* nbrs, uint64_t entry_id);
  uint64_t graph_slots() const;
  uint64_t graph_edges();
  void export_graph(uint64_t* ids, uint32_t* levels, uint64_t* nbr_offsets, uint64_t* nbrs);
  uint64_t dist_evals() const { return n_dist_; }
  uint64_t hops() const { return n_hops_; }
  void set_threads(int t) { threads_ = t; }
  // Where the layered walk runs for batch searches: false = on the host, every hop's candidates scored
  // by one GPU launch (fvdb_scorer_*); true (default) = entirely on the GPU (fvdb_graph_search_dev), the
  // graph mirrored in HBM.  Same results; inserts always use the host walk.
  void set_device_traversal(bool on) { device_traversal_ = on; }
  bool device_traversal() const { return device_traversal_; }
  uint64_t device_fallbacks() const { return n_fallback_.load(); }
  // profiling on: summed HIP-event duration of the traversal kernel's launches since the last call
  int graph_kernel_times(float* ms_sum, uint32_t* launches, uint64_t* rows_scored, uint64_t* hops) {
    *ms_sum = 0.0f;
    *launches = 0;
    *rows_scored = *hops = 0;
    return graph_ ? fvdb_graph_kernel_times(graph_, ms_sum, launches, rows_scored, hops) : 0;
  }
  // queries served by the traversal kernel / searched a second time with the restated heaps (equal distances)
  int tie_restarts(uint64_t* queries, uint64_t* again) {
    *queries = *again = 0;
    return graph_ ? fvdb_graph_tie_restarts(graph_, queries, again) : 0;
  }

 private:
  struct Query {
    RustHeap candidates, nearest;
    Visited visited;
    std::vector<uint32_t> pending;  // candidates sent to the GPU this hop
    std::vector<Cand> cur;          // search_layer: [0] = the layer's entry going in; the layer's nearest, ascending, coming out
    bool active = false;
  };
  // Working state of one lock-step walk: the scorer (one HIP stream; candidate and distance rows in pinned memory) and
  // the per-query heaps.  There are two, never used by the same caller: search_walk_ serves the host walk of the
  // searches (under walk_mu_ — finish() runs it from search threads that hold the index only for reading),
  // insert_walk_ the host algorithm of an insert (B = 1, under the caller's write exclusion).
  struct Walk {
    fvdb_scorer* sc = nullptr;
    uint32_t cap_B = 0, cap_C = 0;
    std::vector<Query> qs;
    std::vector<uint32_t> prev_cnt;  // candidates each scorer row holds from the hop before: what the next hop blanks
    const uint8_t* del = nullptr;    // the deleted flags this walk sees: nullptr = deleted_, else an AllowView's
  };
  Walk search_walk_, insert_walk_;
  uint32_t cap(uint32_t layer) const { return layer == 0 ? cfg_.max_connections_layer_0 : cfg_.max_connections; }
  int ensure_store(uint32_t dim);
  // a walk of B queries with up to C candidates per hop: scorer large enough, every candidate row counted as dirty
  int walk_begin(Walk& w, uint32_t B, uint32_t C);
  // search_layer (:469-554) for the B queries loaded into w's scorer, in lock step; entries and results in Query::cur
  int search_layer(Walk& w, uint32_t B, uint32_t ef, uint32_t layer);
  int score_pairs_from_row(uint32_t base_row, const std::vector<uint32_t>& cands, std::vector<float>& out);
  int sync_graph();
  // The five steps of a search (hnsw_index.cpp).  admit: the checks made before the device is reached; stage: host
  // queries to d_q_; launch: enqueue in the slot and mark it; finish: collect a marked slot, or run the search now;
  // run: all of it, blocking — in slot 0 under search_mu_, or in a slot its caller owns.
  int admit(Search& s);
  int stage(Search& s);
  int launch(Search& s);
  int finish(Search& s);
  int run(Search& s);
  // a view of the synced graph, not cached; scan_k > 0: without the host flags where scans(view, scan_k)
  int make_view(const uint64_t* allowed, uint64_t n_allowed, ViewRef* out, uint32_t scan_k = 0);
  // queries [0, B) of q_dev, already in HBM and ordered so that local[b] indexes masks[]: one grouped scan in `slot`
  int scan_groups(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, const std::vector<fvdb_mask*>& masks,
                  const std::vector<uint32_t>& local, uint32_t slot, uint64_t* ids, float* dist, uint32_t* counts);
  int search_host_walk(const float* q, bool q_on_device, uint32_t B, uint32_t k, uint32_t ef, uint64_t* ids,
                       float* dist, uint32_t* counts, const AllowView* view = nullptr);
  // The adjacency lists exist twice: nbrs_ (host) and the fixed-stride rows in HBM (graph_).  host_ahead_: nbrs_ holds
  // changes the device has not seen (restore, bulk build, vacuum, inserts made before the device graph existed) — the
  // next device use installs the whole graph once.  dev_ahead_: device inserts have linked nodes whose lists nbrs_
  // does not hold yet (a resident vacuum leaves it set too) — whoever needs nbrs_ (export, neighbours, host walk, the host
  // form of vacuum, a host-path insert) pulls them.
  // A host-path insert made while the two agree patches the rows it changed (fvdb_graph_set_lists): no whole-graph
  // upload follows an insert or a delete.
  fvdb_graph* graph_ = nullptr;
  bool host_ahead_ = true, dev_ahead_ = false, device_traversal_ = true, device_insert_ = true;
  int insert_mode_ = 0;
  int visited_mode_ = 0;
  uint32_t visited_slots_ = 0;
  bool resident_vacuum_ = true, vacuum_keep_rows_ = false;
  int vacuum_path_ = VACUUM_NONE;
  fvdb_graph_maintenance_info_t vacuum_info_{};
  uint64_t vacuum_host(const std::vector<uint8_t>& dead, uint64_t removed);  // the host algorithm; the lists are pulled
  void vacuum_adopt(bool reclaimed, const std::vector<uint8_t>& dead);        // bookkeeping after the device job
  // graph_health and the per-node results behind it: reached[node] (1 = in R), label[node] (0xFFFFFFFF: not live)
  int health_run(uint32_t flags, fvdb_graph_health_t* out, int* path, std::vector<uint8_t>* reached, std::vector<uint32_t>* label);
  void health_host(uint32_t flags, fvdb_graph_health_t* out, std::vector<uint8_t>* reached, std::vector<uint32_t>* label) const;
  bool host_link_reported_ = false;  // the stderr line "device insert refused, linking on the host" was written
  fvdb_graph_insert_stats insert_stats_{};
  uint64_t n_host_inserts_ = 0;
  void add_insert_stats(const fvdb_graph_insert_stats& st);  // one fvdb_graph_insert_linked call into the sums
  int ensure_graph_handle();
  int ensure_host_graph();
  bool device_insert_ok() const;
  int check_insert(uint64_t id, const float* v, uint32_t dim) const;
  int insert_host(uint64_t id, const float* v, uint32_t dim, int64_t forced_level);
  // m inserts in progress: vectors into the store and host_vecs_, bookkeeping with registered = 0 ("not yet in the nodes
  // map" while the links are being made, :370); *first = the first of their rows
  int append_nodes(const uint64_t* ids, const uint32_t* levels, const float* v, uint32_t m, uint32_t* first);
  // a whole pre-built graph's nodes into the empty index, registered (restore, bulk_build); levels == nullptr: drawn
  template <class L>
  int adopt_nodes(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const L* levels);
  // Links the appended row by the host algorithm, registers it and brings the device graph up to date by the rules
  // above: rows patched while the two copies agree, host_ahead_ otherwise.  on_device: the device graph holds the node
  // already (fvdb_graph_append_nodes).  The caller has pulled nbrs_ (ensure_host_graph).
  int link_and_publish(uint32_t row, bool on_device);
  // the host algorithm's links for node `row` (bookkeeping and vector already in place); the (node, layer) lists it
  // changed are appended to `touched`
  int link_host(uint32_t row, std::vector<std::pair<uint32_t, uint32_t>>* touched);
  void finalize_insert(uint32_t row);
  struct DevSlot {  // per in-flight batch: stream (context), device result block and its pinned host copy
    fvdb_ctx* ctx = nullptr;  // slot 0 borrows ctx_, the others own theirs
    DevBuf buf;               // WalkBlock layout
    DevBuf gq;                // search_allowed_groups: the queries in group order
    bool enqueued = false;    // launch() to finish(): a batch is in flight here ...
    bool scanned = false;     // ... whose block came from a scan, which writes no status words
  };
  DevSlot slots_[kSlots];
  DevBuf d_q_;  // stage(): host-resident query batches
  DevBuf qual_;  // evaluate_search_quality: the two id blocks and the per-query figures
  DiverseStage diverse_;
  std::atomic<uint64_t> n_fallback_{0};
  // Searches may come from several host threads (HybridIndex leases a slot per call): the graph mirror is synced by
  // one of them, the rare host-walk fallback and the standalone search()/search_dev() entry points are serialised.
  std::mutex sync_mu_, walk_mu_, search_mu_;
  uint64_t scan_cutoff_ = 8192;
  std::mutex view_mu_;  // the cached allow view
  std::vector<uint64_t> view_key_;
  ViewRef view_;
  uint64_t mask_builds_ = 0;

  fvdb_ctx* ctx_;
  HNSWConfig cfg_;
  SplitMix64 rng_;
  fvdb_store* store_ = nullptr;
  uint32_t dim_ = 0;
  bool has_dim_ = false, has_entry_ = false, entry_lost_ = false;
  uint32_t entry_ = 0;
  uint64_t n_registered_ = 0;
  std::vector<uint64_t> ids_;
  std::vector<uint32_t> level_;
  std::vector<uint8_t> deleted_, registered_;
  std::vector<std::vector<std::vector<uint32_t>>> nbrs_;  // [node][layer] insertion-ordered sets
  std::unordered_map<uint64_t, uint32_t> index_of_;
  std::vector<float> host_vecs_;
  uint64_t n_dist_ = 0, n_hops_ = 0;
  int threads_ = 0;
};

// ------------------------------------------------------------------------------------------
// HybridIndex — src/hybrid/core.rs.  `now` / timestamps are seconds passed in by the caller
// (the reference reads Utc::now() at the same points).
// ------------------------------------------------------------------------------------------
struct HybridConfig {
  double recent_threshold_s = 7.0 * 24 * 3600;  // :77
  HNSWConfig hnsw;
  IVFConfig ivf;  // default() below sets 3 clusters / n_probe 2 / train_size 9 like :69-74
  uint64_t migration_batch_size = 100;
  bool auto_migrate = true;
  uint64_t min_ivf_training_size = 10;
  // one knob for both parts: set_row_dtype writes hnsw.row_dtype and ivf.row_dtype together
  void set_row_dtype(int dt) { hnsw.row_dtype = ivf.row_dtype = dt; }
  int row_dtype() const { return hnsw.row_dtype; }
  static HybridConfig defaults() {
    HybridConfig c;
    c.ivf.train_size = 9;
    c.ivf.n_clusters = 3;
    c.ivf.n_probe = 2;
    return c;
  }
};

struct HybridSearchConfig {  // :172-197
  bool search_recent = true, search_historical = true;
  uint64_t recent_k = 0, historical_k = 0;
  uint64_t k = 10, hnsw_ef = 50, ivf_n_probe = 10;
  // results asked of each part: its own k where one is given, k otherwise
  uint32_t rk() const { return (uint32_t)(recent_k > 0 ? recent_k : k); }
  uint32_t hk() const { return (uint32_t)(historical_k > 0 ? historical_k : k); }
};

class HybridIndex {
 public:
  HybridIndex(fvdb_ctx* ctx_ivf, fvdb_ctx* ctx_hnsw, const HybridConfig& cfg);
  ~HybridIndex();
  bool is_initialized() const { return initialized_; }
  bool is_ivf_trained() const { return ivf_trained_; }
  int initialize(const float* data, uint64_t n, uint32_t dim);                                    // :262
  int set_ivf_centroids(const float* c, uint32_t dim);  // install a trained quantizer (parity runs)
  int insert_with_timestamp(uint64_t id, const float* v, uint32_t dim, double ts, double now, int64_t level);  // :357
  int search(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now, uint64_t* ids,
             float* dist, uint32_t* counts);                                                       // :425
  // queries resident in HBM: the IVF scan runs asynchronously on its own stream while the host walks
  // the HNSW graph (hop scoring on the second stream); results come back to host memory
  int search_dev(const float* q_dev, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now,
                 uint64_t* ids, float* dist, uint32_t* counts);
  // The same search split in two, so that `kSlots` batches can be in flight at once (the graph walk of one
  // batch occupies one wavefront per SIMD: a second batch's walk runs beside it almost for free).  begin
  // enqueues everything for the batch (traversal kernel on the slot's stream, IVF chain and its result copies on
  // the IVF stream) and returns; end waits for that slot only and merges on the host.  The query buffer must stay
  // valid and unchanged until end.  Mutations between a begin and its end are not allowed.
  // Timing of the IVF part (unsharded, no allow-set; see Pair below): begin enqueues the graph walk at once, the IVF chain
  // of the batch may start at the NEXT begin — one chain then serves both batches — or at its own end.  Results and
  // error codes are unchanged; an error of a chain enqueued after begin returned comes back from that batch's end.
  static constexpr uint32_t kSlots = HNSWIndex::kSlots;
  int search_dev_begin(uint32_t slot, const float* q_dev, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg,
                       double now);
  int search_dev_end(uint32_t slot, uint64_t* ids, float* dist, uint32_t* counts);
  // Multi-GPU (no counterpart in the reference): this rank's HybridIndex holds the inverted lists it owns
  // (bulk_insert_sharded) and a replica of the graph.  attach_comm binds a communicator (fvdb_comm_create / _hosted);
  // search_sharded_begin enqueues one step in `slot` — the IVF part through fvdb_ivf_search_sharded_begin (both
  // exchanges and the merge by key on the slot's stream), the graph walk of this rank's own queries beside it — and
  // search_sharded_end waits for the slot and applies the reference's hybrid merge.  mode FVDB_SHARD_WEAK: q_dev is
  // this rank's own B queries, B result rows; FVDB_SHARD_STRONG: q_dev is the global batch (same on every rank),
  // result rows = this rank's slice [r*per, min(B,(r+1)*per)) (sharded_rows()).  Every rank makes the same sequence
  // of begin/end calls WITH THE SAME `now`: the per-search auto-migration (src/hybrid/core.rs:437-439) runs on every
  // rank — the same due ids in the same order, assigned by the same centroids; the rank that owns a list appends the
  // row, every rank counts it into the logical list sizes (migrate_locked).
  int attach_comm(fvdb_comm* comm);
  int search_sharded_begin(uint32_t slot, const float* q_dev, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg,
                           int mode, double now = 0.0);
  int search_sharded_end(uint32_t slot, uint64_t* ids, float* dist, uint32_t* counts) {
    return search_dev_end(slot, ids, dist, counts);
  }
  // A step whose historical_k or ivf_n_probe exceeds FVDB_MAX_K goes through fvdb_ivf_search_sharded_wide_begin.
  // search_allowed_sharded_begin is the same step under an allow-set (search_allowed's semantics), collected by
  // search_sharded_end: the masks are built after the migration step, under the read lock, and stay referenced until
  // the slot is collected; the recent part is the masked traversal / allowed scan of this rank's own queries, the
  // historical part the masked sharded step.  Every rank passes the SAME allow-set, as it passes the same `now`.
  int search_allowed_sharded_begin(uint32_t slot, const float* q_dev, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg,
                                   int mode, const uint64_t* allowed, uint64_t n_allowed, double now = 0.0);
  uint32_t sharded_rows(uint32_t B, int mode) const;  // rows search_sharded_end writes on this rank
  // search_with_filter (src/hybrid/core.rs:513-549): ask for 3 k neighbours, keep the first k whose id the host
  // application's metadata filter accepts.  `matches(id, user)` stands for `metadata_map.get(id)` +
  // `MetadataFilter::matches` (an id without metadata does not match); NULL = no filter = plain search.
  typedef int (*FilterFn)(uint64_t id, void* user);
  int search_with_filter(const float* q, uint32_t B, uint32_t dim, uint64_t k, FilterFn matches, void* user, double now,
                         uint64_t* ids, float* dist, uint32_t* counts);
  // Filtered search with the allow-set applied inside both parts (no counterpart in the reference): what search()
  // search_allowed_groups: one allow-set per query — per query what search_allowed returns under
  // the set of its group, or what search returns where the group is "no filter".  One migration step, every mask built
  // after it under the read lock, the two parts by IVFIndex / HNSWIndex::search_allowed_groups, the usual merge.
  int search_allowed_groups(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, const AllowGroups& groups,
                            double now, uint64_t* ids, float* dist, uint32_t* counts);
  // returns after remove() of every id outside allowed[n_allowed]; the recent part is scanned exactly instead when
  // its allowed live nodes number at most recent().scan_cutoff().  The masks are built after the auto-migration step
  // and under the same read lock as the search, so they match the rows searched; the last pair is kept for a caller
  // that repeats one filter.  FVDB_E_UNSUPPORTED once the index is sharded (search_allowed_sharded_begin serves that).
  int search_allowed(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, const uint64_t* allowed,
                     uint64_t n_allowed, double now, uint64_t* ids, float* dist, uint32_t* counts);
  // Exact search: search()'s migration step and read lock, then the recent part from the flat
  // scan of the graph's rows and the historical part from the search of every list (search_with_config(q, k,
  // n_clusters), src/ivf/core.rs:626-681), merged by the usual merge — no de-duplication: a migrated row that still
  // sits in the graph appears twice, as in search().  cfg: k, search_recent, search_historical (recent_k /
  // historical_k as in search()); k in 1..FVDB_MAX_K.  FVDB_E_UNSUPPORTED once the index is sharded: a rank holds
  // only the lists it owns.
  int search_exact(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now, uint64_t* ids,
                   float* dist, uint32_t* counts);
  // search(cfg) against search_exact(cfg) under ONE hold of the read lock, after one migration step: both see the same
  // rows.  B == 0 is FVDB_E_INVALID.
  int evaluate_search_quality(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now,
                              SearchQuality* out);
  // The same two with k in 1..FVDB_MAX_K_WIDE: the recent part from the graph's wide exact scan
  // (recent_k and historical_k up to FVDB_MAX_K_WIDE as well, else FVDB_E_UNSUPPORTED); migration step, read lock,
  // merge and the sharded refusal are search_exact's.  At k <= FVDB_MAX_K they return what the two above return.
  int search_exact_wide(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now, uint64_t* ids,
                        float* dist, uint32_t* counts);
  int evaluate_search_quality_wide(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now,
                                   SearchQuality* out);
  // Radius search: search_exact_wide's migration step, read lock and sharded refusal; cfg.k is
  // max_results (1..FVDB_MAX_K_WIDE) for each part and for the result.  The recent part is the graph's flat radius scan
  // (HNSWIndex::search_radius_dev) and NOT a walk: a walk bounded by ef visits what its frontier reaches and cannot
  // enumerate a ball, so the recent total is exact over every live node.  The historical part is
  // IVFIndex::search_radius over the cfg.ivf_n_probe probed lists — every list when ivf_n_probe = n_clusters, the ball of
  // the probed lists only below that.  The two capped lists go through the usual merge with k = max_results, and
  // totals[b] = recent total + historical total: like that merge it does not de-duplicate, so an id that both parts hold
  // within the radius counts twice.  allowed != nullptr: both parts under that allow-set (the cached view and mask).
  int search_radius(const float* q, uint32_t B, uint32_t dim, const float* radius, const HybridSearchConfig& cfg, double now,
                    const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts, uint32_t* totals);
  // Diverse search: one auto-migration step; then, under ONE hold of the read lock, search(cfg with
  // k = fetch_k) — search_allowed when allowed != nullptr — the id-to-location lookup (the recent part first, then the
  // historical part, as get_vectors) and the gather.  cfg.k is k; recent_k / historical_k are not read (each part is asked
  // for fetch_k).  With distinct a migrated row that still sits in the graph is returned once; lam = 1 and distinct is
  // the de-duplicated search.  FVDB_E_UNSUPPORTED once the index is sharded.
  int search_diverse(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, uint32_t fetch_k, float lam,
                     bool distinct, double now, const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist,
                     uint32_t* ranks, uint32_t* counts);
  // the same with one allow-set per query: the candidates are what search_allowed_groups(cfg with k = fetch_k) returns
  int search_diverse_groups(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, uint32_t fetch_k, float lam,
                            bool distinct, const AllowGroups& groups, double now, uint64_t* ids, float* dist, uint32_t* ranks,
                            uint32_t* counts);
  int diverse_impl(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, uint32_t fetch_k, float lam, bool distinct,
                   double now, const uint64_t* allowed, uint64_t n_allowed, const AllowGroups* groups, uint64_t* ids, float* dist,
                   uint32_t* ranks, uint32_t* counts);  // both forms
  // evaluate_search_quality (its wide form above k = FVDB_MAX_K) at every pair (efs[i], n_probes[j]) in one call
  // (DESIGN.md section 9r): one migration step; under ONE hold of the read lock one exact search, one traversal per
  // listed ef and one list search per listed n_probe, the PARTS kept; then fvdb_quality_grid_dev merges and counts
  // every pair.  cfg: k, recent_k, historical_k, search_recent, search_historical (hnsw_ef and ivf_n_probe are not
  // read).  out: E x P (E or P counting as 1 when it is 0).  When the historical part is not searched or the lists are
  // untrained every column holds the recent-only value, and every row the historical-only one when the recent part is
  // not searched.  Duplicates and any order in efs / n_probes are fine.  Refused before any search runs, in this order:
  // a sharded index FVDB_E_UNSUPPORTED; B == 0, a null pointer, E == 0 (P == 0) with the recent (historical) part
  // searched FVDB_E_INVALID; k == 0, k > FVDB_MAX_K_WIDE, E or P > 64 FVDB_E_UNSUPPORTED; an index never initialised
  // FVDB_E_INVALID; a dimension mismatch FVDB_E_DIM.  An ef or n_probe the underlying search refuses: that search's code.
  int quality_grid(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, const uint32_t* efs, uint32_t E,
                   const uint32_t* n_probes, uint32_t P, double now, QualityGrid* out);
  // Concurrency (reference: tokio RwLock, searches = readers, src/hybrid/core.rs:457,466): search() / search_dev() /
  // search_with_filter() may be called from any number of host threads; each call leases a free slot (stream,
  // traversal state, IVF scratch set, result blocks) and returns it.  Mutations wait for those calls to finish.
  // The explicit search_dev_begin/_end pair is for ONE thread keeping several batches in flight; while such a batch
  // is uncollected, mutations are refused (INVALID) rather than waited for.
  // What a mutation (insert, delete, migrate, vacuum) does while batches begun with search_dev_begin are uncollected:
  // false (default) = returns FVDB_E_INVALID at once; true = waits for them to be collected, like the reference's write
  // guard waits for its readers (src/hybrid/core.rs:457,466) — for hosts whose searches and writes run on different
  // threads (a thread that waits for its OWN uncollected batch would wait for ever).
  void set_blocking_writers(bool on) { writers_wait_ = on; }
  bool blocking_writers() const { return writers_wait_; }
  bool busy() const {  // some batch is in flight: inserts / deletes are refused (or wait) until it is collected
    std::lock_guard<std::mutex> lk(slot_mu_);
    for (const Slot& s : slots_)
      if (s.active) return true;
    return false;
  }
  bool migration_due(double threshold_s, double now) const {
    return !pending_migration_.empty() && age_of(now, pending_min_ts_) >= threshold_s;
  }
  uint64_t migrate_with_threshold(double threshold_s, double now);                                // :600
  // Where a migration's rows come from (the non-sharded branch): true (default) = the graph's row store in HBM, the due
  // ids go down as store row indices (IVFIndex::batch_insert_from_store); false = the host copy, uploaded by
  // IVFIndex::batch_insert.  Same lists either way.  A due id whose row the store does not hold sends the whole job down
  // the host path.
  void set_resident_migration(bool on) { resident_migration_ = on; }
  bool resident_migration() const { return resident_migration_; }
  // the last migration that had rows to copy: which path it took and its figures (resident: fvdb_ivf_maintenance_info;
  // host: rows and the bytes batch_insert copies, no stage times)
  enum MigrationPath : int { MIGRATION_NONE = 0, MIGRATION_RESIDENT = 1, MIGRATION_HOST = 2 };
  int migration_info(fvdb_maintenance_info_t* out) const {
    *out = migration_info_;
    return migration_path_;
  }
  // Vectors by id (includeVectors, bindings/node/src/session.rs:266-281): the recent part is asked first, then the
  // historical part; found[i] = 0 and the row untouched when neither holds the id.  Runs under the read side of the
  // lock, beside searches.
  int get_vectors(const uint64_t* ids, uint64_t n, float* out, uint8_t* found);
  int remove(uint64_t id, double now);                                                             // delete :904
  uint64_t recent_count() const { return recent_count_; }
  uint64_t historical_count() const { return historical_count_; }
  // from_parts (src/hybrid/core.rs:857-877): adopt the two indexes as they now are (the caller has restored the
  // graph into recent() and set_trained + inserted the lists of historical()) together with the saved timestamp
  // table and counters; the index becomes initialised.  Only valid while the timestamp table is empty.
  int from_parts(const uint64_t* ids, const double* ts, uint64_t n, uint64_t recent_count, uint64_t historical_count,
                 bool ivf_trained);
  // vacuum (src/hybrid/core.rs:989-1012): both indexes; refused while a batch is in flight
  int vacuum(uint64_t* hnsw_removed, uint64_t* ivf_removed);
  // IVFIndex::retrain of the historical index, under vacuum's rule (refused while a batch begun with search_dev_begin
  // is uncollected); FVDB_E_UNSUPPORTED once the index is sharded.  The reference has no real counterpart: its
  // maintenance scheduler only simulates a retrain (src/hybrid/maintenance.rs:509-533).  This is the way out of the
  // default configuration's 3 clusters (src/hybrid/core.rs:69).
  int retrain_historical(const IVFConfig& new_ivf_config, IVFIndex::RetrainResult* out);
  uint64_t timestamp_count() const { return ts_order_.size(); }
  void export_timestamps(uint64_t* ids, double* ts) const;  // insertion order
  HNSWIndex& recent() { return *recent_; }
  IVFIndex& historical() { return *historical_; }
  // How the bulk loaders build the graph of the recent part: true (default) = the reference's own build, sequential
  // inserts in id order (HNSWIndex::batch_insert, on the device); false = HNSWIndex::bulk_build (exact nearest-M
  // per layer — a different graph, an extension).
  void set_sequential_graph(bool on) { sequential_graph_ = on; }
  bool sequential_graph() const { return sequential_graph_; }
  double recent_build_seconds() const { return recent_build_s_; }  // wall time of the last bulk load's graph build
  // bulk loaders for scale runs: route by age like insert_with_timestamp, batched on the GPU
  int bulk_insert(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const double* ts, double now);
  // Multi-GPU placement: the same, but of the historical rows only those whose IVF list is owned by
  // `rank` (owner[list] == rank) are stored on this GPU; the logical list sizes are installed so the
  // tie-break position is global.  With owner == nullptr, lists are dealt largest-first to the least
  // loaded of `world` ranks (deterministic, identical on every rank).  The HNSW part is replicated.
  int bulk_insert_sharded(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const double* ts, double now,
                          uint32_t rank, uint32_t world, uint32_t* owner_out /* nlist, optional */);

 private:
  static double age_of(double now, double ts) { return now - ts < 0 ? 0.0 : now - ts; }
  int search_impl(const float* q, bool q_on_device, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg,
                  double now, uint64_t* ids, float* dist, uint32_t* counts, const uint64_t* allowed = nullptr,
                  uint64_t n_allowed = 0, bool masked = false);
  // search_impl / search_exact after the migration step, the caller holding the read side of rw_
  int search_locked(const float* q, bool q_on_device, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, uint64_t* ids,
                    float* dist, uint32_t* counts, const uint64_t* allowed, uint64_t n_allowed, bool masked);
  // search_allowed_groups after the migration step, the caller holding the read side of rw_
  int groups_locked(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, const AllowGroups& groups, uint64_t* ids,
                    float* dist, uint32_t* counts);
  // wide: the graph's wide exact scan, part sizes up to FVDB_MAX_K_WIDE
  int exact_locked(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, uint64_t* ids, float* dist,
                   uint32_t* counts, bool wide = false);
  // search_exact / search_exact_wide and evaluate_search_quality / _wide: one body each, `wide` choosing the limit of k
  int exact_impl(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now, uint64_t* ids, float* dist,
                 uint32_t* counts, bool wide);
  int quality_impl(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now, SearchQuality* out,
                   bool wide);
  std::mutex qual_mu_;  // evaluate_search_quality's staging block
  DevBuf qual_;
  DiverseStage diverse_;
  // the explicit pair's begin, plain (shard_mode -1) or sharded: migration check, slot marked active, begin_impl
  int begin_explicit(uint32_t slot, const float* q_dev, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg,
                     int shard_mode, double now, const uint64_t* allowed = nullptr, uint64_t n_allowed = 0,
                     bool masked = false);
  // may_pair: the caller is the explicit pair's begin, whose IVF chain may wait for a partner (Pair below)
  int begin_impl(uint32_t slot, const float* q_dev, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg,
                 int shard_mode = -1, bool may_pair = false);
  int build_masks(const HybridSearchConfig& cfg, const uint64_t* allowed, uint64_t n_allowed, HNSWIndex::ViewRef* view,
                  MaskRef* ivf_mask);
  // The per-search auto-migration (src/hybrid/core.rs:437-439).  A due migration moves rows between the two indexes (and
  // may grow the list pool), so it is refused with FVDB_E_INVALID while batches begun with search_dev_begin are
  // uncollected — now, or (`in_flight_before`) when the caller looked before it came here.
  int migrate_if_due(double now, bool in_flight_before);
  struct Slice {  // FVDB_SHARD_STRONG: this rank's rows [lo, hi) of a global batch, `per` rows to every rank
    uint32_t per, lo, hi;
  };
  Slice strong_slice(uint32_t B) const;
  int build_recent(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim);
  // first half of both bulk loaders: timestamps, routing by age like insert_with_timestamp, the graph of the recent rows
  // and their migration queue; the historical rows come back in hid / hv
  int bulk_route(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const double* ts, double now,
                 std::vector<uint64_t>& hid, std::vector<float>& hv);
  bool sequential_graph_ = true;
  bool resident_migration_ = true;
  int migration_path_ = MIGRATION_NONE;
  fvdb_maintenance_info_t migration_info_{};
  std::atomic<bool> writers_wait_{false};
  // exclusive access for a mutation: with no batch in flight, or FVDB_E_INVALID / after waiting (set_blocking_writers)
  int write_lock(std::unique_lock<std::shared_mutex>& w);
  double recent_build_s_ = 0.0;
  fvdb_comm* comm_ = nullptr;
  fvdb_sharded* sharded_ = nullptr;
  // list placement of bulk_insert_sharded (world 0 = not sharded): owner rank and logical size of every list
  uint32_t shard_rank_ = 0, shard_world_ = 0;
  std::vector<uint32_t> shard_owner_;
  std::vector<uint64_t> shard_sizes_;
  uint64_t migrate_locked(double threshold_s, double now);
  bool busy_unlocked() const {
    for (const Slot& s : slots_)
      if (s.active) return true;
    return false;
  }
  mutable std::shared_mutex rw_;   // searches of the blocking entry points: shared; mutations: unique
  mutable std::mutex slot_mu_;     // Slot::active
  std::condition_variable slot_cv_;
  fvdb_ctx* ctx_ivf_;
  struct Pair;
  struct Slot {  // one batch in flight
    DevBuf ivf;             // results of the IVF part (IvfBlock layout): device block and its pinned host copy
    uint32_t ivf_rows = 0;  // rows the IVF part writes into it for this batch
    fvdb_event* ivf_done = nullptr;
    fvdb_ctx* ivf_ctx = nullptr;  // slot 0 borrows ctx_ivf_, the others own a context (stream) each
    bool active = false, ivf_in_flight = false, hnsw_in_flight = false, recent = false;
    DevBuf d_q;  // staging for host-resident query batches of the blocking entry points
    const float* q = nullptr;
    uint32_t B = 0, dim = 0, k = 0, rk = 0, hk = 0, ef = 0;
    // a search under an allow-set holds its masks here from begin to end
    MaskRef ivf_mask;
    HNSWIndex::ViewRef view;
    // paired IVF chains (below): all four under pair_mu_
    bool ivf_waiting = false;  // the IVF chain of this batch is not enqueued yet (q, B, dim, hk, n_probe say what it is)
    uint32_t n_probe = 0;
    int ivf_rc = FVDB_OK;      // status of an enqueue that happened after this batch's begin returned; search_dev_end's
    Pair* pair = nullptr;      // the joint chain this batch's IVF rows come from, starting at row pair_off
    uint32_t pair_off = 0;
  };
  Slot slots_[kSlots];
  // One IVF chain for two batches in flight.  A batch begun with search_dev_begin on an unsharded
  // index without an allow-set does not enqueue its IVF chain: it waits (waiting_) for the next such begin, which
  // enqueues ONE chain for the queries of both on its own slot's stream and scratch set, or for its own end, a blocking
  // search or a writer, which enqueue it alone (flush_waiting).
  // Lifetime: the joint query block, the result blocks and the event belong to the Pair, never to a slot — the slot that
  // launched may be collected and begun again (its event re-recorded, its block rewritten) before its partner is
  // collected.  A Pair is held by the slots that read from it (refs) and free again after the second search_dev_end.
  struct Pair {
    DevBuf q;    // [B1 + B2][dim], the waiting batch first
    DevBuf res;  // IvfBlock layout over rows = B1 + B2, with its pinned host copy
    fvdb_event* done = nullptr;
    fvdb_ctx* ctx = nullptr;  // the context whose stream carries the chain (the launching slot's)
    uint32_t rows = 0, hk = 0, refs = 0;
  };
  static constexpr uint32_t kPairs = kSlots / 2;
  static constexpr uint32_t kPairRowsMax = 16384;  // B1 + B2 of a joint chain: the largest batch the engine's parity tests run
  // pairs can outnumber kPairs only when partners are collected far apart; a begin that finds none free does not pair
  Pair pairs_[kPairs];
  std::mutex pair_mu_;  // waiting_, the pool, the Slot fields above, and every enqueue of an IVF chain of the explicit pair
  int waiting_ = -1;
  static bool pairing_enabled();  // FVDB_HYBRID_PAIR=0 (read once) restores one chain per batch, enqueued at begin
  // one batch alone: chain, result copy and event on the slot's own stream
  int enqueue_ivf(uint32_t slot, const float* q_dev, uint32_t B_in, uint32_t ivf_rows, uint32_t dim, uint64_t n_probe,
                  int shard_mode);
  int enqueue_ivf_pair(Slot& first, uint32_t launcher, Pair& p);  // pair_mu_ held
  int begin_ivf_paired(uint32_t slot);                            // takes pair_mu_
  void flush_waiting_locked();                                    // pair_mu_ held: the waiting batch's chain, alone
  void flush_waiting() {
    std::lock_guard<std::mutex> lk(pair_mu_);
    flush_waiting_locked();
  }
  void release_pair(Slot& sl);  // takes pair_mu_
  int stage_finite(Slot& sl, const float* q, uint32_t B, uint32_t dim);
  // A slot keeps a filtered search's masks only while that search runs: dropped at scope exit, whichever way it
  // returns, so that the next user of the slot finds none.  sl = nullptr: handed on to the search_dev_end that collects.
  struct DropMasks {
    Slot* sl;
    ~DropMasks() {
      if (sl) sl->ivf_mask.reset(), sl->view.reset();
    }
  };
  // Slot::active held for a scope: set under slot_mu_, cleared on release with the waiting writers and searches woken.
  // hand_over() leaves the mark in place for the search_dev_end that collects the batch, which adopts it.
  struct Lease {
    static constexpr uint32_t kAnyFree = ~0u;  // wait for a free slot and take the highest
    enum How { kTake, kAdopt };                // mark a slot that is not active / take over the mark of one that is
    Lease(HybridIndex* h, uint32_t slot, How how);
    ~Lease();
    Lease(const Lease&) = delete;
    Lease& operator=(const Lease&) = delete;
    void hand_over() { sl = nullptr; }
    uint32_t index() const { return (uint32_t)(sl - h->slots_); }
    HybridIndex* h;
    Slot* sl = nullptr;  // nullptr: nothing held (the slot was not in the state asked for, or handed over)
  };
  HybridConfig cfg_;
  HNSWIndex* recent_;
  IVFIndex* historical_;
  bool initialized_ = false, ivf_trained_ = false;
  std::vector<uint64_t> ts_order_;
  std::unordered_map<uint64_t, double> timestamps_;
  struct Pending {
    uint64_t id;
    double ts;
  };
  std::vector<Pending> pending_migration_;  // (insertion order) ids living in HNSW not yet copied into IVF
  double pending_min_ts_ = 1e300;           // oldest timestamp among them: O(1) "nothing is due" test
  uint64_t recent_count_ = 0, historical_count_ = 0;
};

// Pure host pieces of the multi-GPU path (also called by the CPU tests through the C wrappers):
// greedy "largest list to the least loaded rank" placement, identical on every rank ...
void plan_list_owners_host(const uint64_t* sizes, uint32_t nlist, uint32_t world, uint32_t* owner);
// ... and HybridIndex::search_with_config's merge (src/hybrid/core.rs:476-485): recent results then historical ones,
// stable sort by distance, truncate(k); B queries, rid/rd are B x rk, hid/hd B x hk (either part may be NULL)
void merge_parts_host(uint32_t B, uint32_t k, uint32_t rk, uint32_t hk, const uint64_t* rid, const float* rd,
                      const uint32_t* rc, const uint64_t* hid, const float* hd, const uint32_t* hc, uint64_t* ids,
                      float* dist, uint32_t* counts);

// Grouped search of the three classes: the candidates are exactly what the class's search(fetch_k)
// — search_allowed when `allowed` is given — returns at these settings, so the register route up to FVDB_MAX_K and the
// wide route above it; `ctx` carries the upload, the selection and the download.  For the hybrid index cfg.k counts
// groups and the candidate search runs with k = fetch_k, recent_k = historical_k = 0; it takes search()'s migration step.
int search_grouped(IVFIndex& ix, fvdb_ctx* ctx, const GroupBy& by, const float* q, uint32_t B, uint32_t dim, uint32_t k,
                   uint32_t group_size, uint32_t fetch_k, bool distinct, int missing, uint32_t n_probe, const uint64_t* allowed,
                   uint64_t n_allowed, const GroupedOut& out);
int search_grouped(HNSWIndex& ix, fvdb_ctx* ctx, const GroupBy& by, const float* q, uint32_t B, uint32_t dim, uint32_t k,
                   uint32_t group_size, uint32_t fetch_k, bool distinct, int missing, uint32_t ef, const uint64_t* allowed,
                   uint64_t n_allowed, const GroupedOut& out);
int search_grouped(HybridIndex& ix, fvdb_ctx* ctx, const GroupBy& by, const float* q, uint32_t B, uint32_t dim,
                   const HybridSearchConfig& cfg, uint32_t group_size, uint32_t fetch_k, bool distinct, int missing, double now,
                   const uint64_t* allowed, uint64_t n_allowed, const GroupedOut& out);

}  // namespace fvdbh
