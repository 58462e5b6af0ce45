// capi.cpp — flat C view of the host mirror for ctypes (fvh_* symbols).
#include <cstring>
#include <new>

#include "fvdb_host.hpp"

using namespace fvdbh;

extern "C" {

// ---- IVFIndex ----
static bool row_dtype_ok(int row_dtype) { return row_dtype == FVDB_F32 || row_dtype == FVDB_F16; }

// fp16 rows: bit-exact round-to-nearest-even f32 -> binary16 -> f32, the doors' routine
void fvh_round_f16(const float* in, uint64_t n, float* out) { round_f16(in, n, out); }

// the constructors with the rows' storage chosen (FVDB_F32 / FVDB_F16); anything else is an invalid config
void* fvh_ivf_new_ex(fvdb_ctx* ctx, uint32_t n_clusters, uint32_t n_probe, uint32_t train_size, uint32_t max_iterations,
                     uint64_t seed, int row_dtype) {
  IVFConfig c;
  c.n_clusters = n_clusters;
  c.n_probe = n_probe;
  c.train_size = train_size;
  c.max_iterations = max_iterations;
  c.seed = seed;
  c.row_dtype = row_dtype;
  if (!c.is_valid() || !row_dtype_ok(row_dtype)) return nullptr;
  return new (std::nothrow) IVFIndex(ctx, c);
}
int fvh_ivf_row_dtype(void* p) { return ((IVFIndex*)p)->config().row_dtype; }

void* fvh_ivf_new(fvdb_ctx* ctx, uint32_t n_clusters, uint32_t n_probe, uint32_t train_size, uint32_t max_iterations,
                  uint64_t seed) {
  IVFConfig c;
  c.n_clusters = n_clusters;
  c.n_probe = n_probe;
  c.train_size = train_size;
  c.max_iterations = max_iterations;
  c.seed = seed;
  if (!c.is_valid()) return nullptr;  // IVFIndex::new panics on an invalid config (:171-174)
  return new (std::nothrow) IVFIndex(ctx, c);
}
void fvh_ivf_free(void* p) { delete (IVFIndex*)p; }
int fvh_ivf_train(void* p, const float* x, uint64_t n, uint32_t d, fvdb_train_result* out) {
  return ((IVFIndex*)p)->train(x, n, d, out);
}
int fvh_ivf_set_trained(void* p, const float* c, uint32_t d) { return ((IVFIndex*)p)->set_trained(c, d); }
int fvh_ivf_get_centroids(void* p, float* out) { return ((IVFIndex*)p)->get_centroids(out); }
int fvh_ivf_is_trained(void* p) { return ((IVFIndex*)p)->is_trained(); }
uint32_t fvh_ivf_dimension(void* p) { return ((IVFIndex*)p)->dimension(); }
uint64_t fvh_ivf_total_vectors(void* p) { return ((IVFIndex*)p)->total_vectors(); }
uint64_t fvh_ivf_active_count(void* p) { return ((IVFIndex*)p)->active_count(); }
uint64_t fvh_ivf_cluster_size(void* p, uint32_t c) { return ((IVFIndex*)p)->cluster_size(c); }
int fvh_ivf_export_list(void* p, uint32_t c, float* rows, uint64_t* ids, uint8_t* live) {
  return ((IVFIndex*)p)->export_list(c, rows, ids, live);
}
int fvh_ivf_insert(void* p, uint64_t id, const float* v, uint32_t d) { return ((IVFIndex*)p)->insert(id, v, d); }
int fvh_ivf_batch_insert(void* p, const uint64_t* ids, const float* v, uint64_t n, uint32_t d, uint64_t* n_ok,
                         int* first_error) {
  return ((IVFIndex*)p)->batch_insert(ids, v, n, d, n_ok, first_error);
}
int fvh_ivf_find_cluster(void* p, const float* v, uint32_t d, uint32_t* out) {
  return ((IVFIndex*)p)->find_cluster(v, d, out);
}
int fvh_ivf_search(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, uint32_t n_probe, uint64_t* ids,
                   float* dist, uint32_t* counts) {
  return ((IVFIndex*)p)->search(q, B, d, k, n_probe, ids, dist, counts);
}
// filtered search: the allow-set is applied inside the search
int fvh_ivf_search_allowed(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, uint32_t n_probe, const uint64_t* allowed,
                           uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts) {
  return ((IVFIndex*)p)->search_allowed(q, B, d, k, n_probe, allowed, n_allowed, ids, dist, counts);
}
// one allow-set per query: set g = allowed[off[g] .. off[g + 1]), filtered[g] == 0 = "no filter"
int fvh_ivf_search_allowed_groups(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, uint32_t n_probe,
                                  const uint64_t* allowed, const uint64_t* off, const uint8_t* filtered, uint32_t G,
                                  const uint32_t* group_of_query, uint64_t* ids, float* dist, uint32_t* counts) {
  return ((IVFIndex*)p)->search_allowed_groups(q, B, d, k, n_probe, AllowGroups{allowed, off, filtered, G, group_of_query}, ids, dist,
                                               counts);
}
uint64_t fvh_ivf_mask_builds(void* p) { return ((IVFIndex*)p)->mask_builds(); }
int fvh_ivf_mark_deleted(void* p, uint64_t id) { return ((IVFIndex*)p)->mark_deleted(id); }
int fvh_ivf_is_deleted(void* p, uint64_t id) { return ((IVFIndex*)p)->is_deleted(id); }
void* fvh_ivf_device(void* p) { return ((IVFIndex*)p)->device(); }
// retrain / add_clusters / optimize_clusters / get_cluster_stats (src/ivf/operations.rs:148-288).  out4 = old_clusters,
// new_clusters, vectors_reassigned, converged.  An invalid config is refused here (IVFIndex::new would have panicked).
static int retrain_config(uint32_t n_clusters, uint32_t n_probe, uint32_t train_size, uint32_t max_iterations, uint64_t seed,
                          IVFConfig* c) {
  c->n_clusters = n_clusters;
  c->n_probe = n_probe;
  c->train_size = train_size;
  c->max_iterations = max_iterations;
  c->seed = seed;
  return c->is_valid() ? FVDB_OK : FVDB_E_INVALID;
}
int fvh_ivf_retrain(void* p, uint32_t n_clusters, uint32_t n_probe, uint32_t train_size, uint32_t max_iterations,
                    uint64_t seed, uint64_t* out4) {
  IVFConfig c;
  if (int rc = retrain_config(n_clusters, n_probe, train_size, max_iterations, seed, &c)) return rc;
  IVFIndex::RetrainResult r{};
  const int rc = ((IVFIndex*)p)->retrain(c, &r);
  if (!rc && out4) std::memcpy(out4, &r, sizeof r);
  return rc;
}
int fvh_ivf_add_clusters(void* p, uint32_t n_clusters_to_add, uint64_t* vectors_reassigned) {
  return ((IVFIndex*)p)->add_clusters(n_clusters_to_add, vectors_reassigned);
}
int fvh_ivf_optimize_clusters(void* p, uint32_t* iterations, float* improvement) {
  return ((IVFIndex*)p)->optimize_clusters(iterations, improvement);
}
int fvh_ivf_cluster_stats(void* p, IVFIndex::ClusterStats* out) {
  *out = ((IVFIndex*)p)->get_cluster_stats();
  return FVDB_OK;
}
// evaluate_search_quality (src/ivf/operations.rs:329-391) at the configured n_probe.  out3 = avg_recall, avg_precision,
// avg_query_time_ms; B = 0 is FVDB_E_INVALID ("No test queries provided")
int fvh_ivf_evaluate_search_quality(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, float* out3,
                                    uint64_t* queries_evaluated) {
  IVFIndex::SearchQuality s{};
  const int rc = ((IVFIndex*)p)->evaluate_search_quality(q, B, d, k, &s);
  if (rc) return rc;
  out3[0] = s.avg_recall;
  out3[1] = s.avg_precision;
  out3[2] = s.avg_query_time_ms;
  if (queries_evaluated) *queries_evaluated = s.queries_evaluated;
  return FVDB_OK;
}
// evaluate_search_quality at every n_probe = 1 .. n_clusters from one search of every list (IVFIndex::quality_curve).
// out_recall / out_precision: n_out floats each, n_out = the index's lists (else FVDB_E_INVALID); out_ms: the wall time
// per query.  use_allowed != 0: under the allow-set allowed[n_allowed] (an empty one allows nothing).
int fvh_ivf_quality_curve(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, int use_allowed, const uint64_t* allowed,
                          uint64_t n_allowed, uint32_t n_out, float* out_recall, float* out_precision, float* out_ms,
                          uint64_t* queries_evaluated) {
  static const uint64_t none = 0;
  if (!out_recall || !out_precision) return FVDB_E_INVALID;
  if (use_allowed && n_allowed && !allowed) return FVDB_E_INVALID;
  IVFIndex::QualityCurve c;
  const int rc = ((IVFIndex*)p)->quality_curve(q, B, d, k, use_allowed ? (n_allowed ? allowed : &none) : nullptr,
                                               use_allowed ? n_allowed : 0, &c);
  if (rc) return rc;
  if (c.avg_recall.size() != n_out) return FVDB_E_INVALID;
  std::memcpy(out_recall, c.avg_recall.data(), (size_t)n_out * 4);
  std::memcpy(out_precision, c.avg_precision.data(), (size_t)n_out * 4);
  if (out_ms) *out_ms = c.avg_query_time_ms;
  if (queries_evaluated) *queries_evaluated = c.queries_evaluated;
  return FVDB_OK;
}
// rows by id, read back from HBM (src/ivf/core.rs:553-562); found[i] = 0 leaves row i of out untouched
int fvh_ivf_get_vectors(void* p, const uint64_t* ids, uint64_t n, float* out, uint8_t* found) {
  return ((IVFIndex*)p)->get_vectors(ids, n, out, found);
}
uint32_t fvh_ivf_n_clusters(void* p) { return ((IVFIndex*)p)->config().n_clusters; }
uint32_t fvh_ivf_n_probe(void* p) { return ((IVFIndex*)p)->config().n_probe; }

// ---- HNSWIndex ----
void* fvh_hnsw_new(fvdb_ctx* ctx, uint32_t M, uint32_t M0, uint32_t efc, uint64_t seed) {
  HNSWConfig c;
  c.max_connections = M;
  c.max_connections_layer_0 = M0;
  c.ef_construction = efc;
  c.seed = seed;
  return new (std::nothrow) HNSWIndex(ctx, c);
}
void* fvh_hnsw_new_ex(fvdb_ctx* ctx, uint32_t M, uint32_t M0, uint32_t efc, uint64_t seed, int row_dtype) {
  if (!row_dtype_ok(row_dtype)) return nullptr;
  HNSWConfig c;
  c.max_connections = M;
  c.max_connections_layer_0 = M0;
  c.ef_construction = efc;
  c.seed = seed;
  c.row_dtype = row_dtype;
  return new (std::nothrow) HNSWIndex(ctx, c);
}
int fvh_hnsw_row_dtype(void* p) { return ((HNSWIndex*)p)->config().row_dtype; }
uint64_t fvh_hnsw_store_bytes(void* p) { return ((HNSWIndex*)p)->store_bytes(); }
void fvh_hnsw_free(void* p) { delete (HNSWIndex*)p; }
int fvh_hnsw_insert(void* p, uint64_t id, const float* v, uint32_t d, int64_t level) {
  return ((HNSWIndex*)p)->insert(id, v, d, level);
}
// batch_insert (src/hnsw/operations.rs:74-94): sequential loop, keeps going after a failure
int fvh_hnsw_batch_insert(void* p, const uint64_t* ids, const float* v, uint64_t n, uint32_t d, const int64_t* levels,
                          uint64_t* n_ok, int* first_error) {
  return ((HNSWIndex*)p)->batch_insert(ids, v, n, d, levels, n_ok, first_error);
}
void fvh_hnsw_set_device_insert(void* p, int on, int mode) { ((HNSWIndex*)p)->set_device_insert(on != 0, mode); }
int fvh_hnsw_device_insert(void* p) { return ((HNSWIndex*)p)->device_insert(); }
int fvh_hnsw_set_insert_visited(void* p, int mode, uint32_t table_slots) { return ((HNSWIndex*)p)->set_insert_visited(mode, table_slots); }
int fvh_hnsw_insert_info(void* p, fvdb_graph_insert_info_t* out) { return ((HNSWIndex*)p)->insert_info(out); }
void fvh_hnsw_insert_stats(void* p, fvdb_graph_insert_stats* out, uint64_t* host_path_inserts, uint64_t* upload_bytes) {
  HNSWIndex* h = (HNSWIndex*)p;
  if (out) *out = h->insert_stats();
  if (host_path_inserts) *host_path_inserts = h->host_path_inserts();
  if (upload_bytes) *upload_bytes = h->graph_upload_bytes();
}
int fvh_hnsw_search(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, uint32_t ef, uint64_t* ids,
                    float* dist, uint32_t* counts) {
  return ((HNSWIndex*)p)->search(q, B, d, k, ef, ids, dist, counts);
}
int fvh_hnsw_search_allowed(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, uint32_t ef, const uint64_t* allowed,
                            uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts) {
  return ((HNSWIndex*)p)->search_allowed(q, B, d, k, ef, allowed, n_allowed, ids, dist, counts);
}
// exact search and search quality.  out3 = avg_recall, avg_precision, avg_query_time_ms
int fvh_hnsw_search_exact(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, uint64_t* ids, float* dist, uint32_t* counts) {
  return ((HNSWIndex*)p)->search_exact(q, B, d, k, ids, dist, counts);
}
int fvh_hnsw_search_exact_allowed(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, const uint64_t* allowed,
                                  uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts) {
  return ((HNSWIndex*)p)->search_exact_allowed(q, B, d, k, allowed, n_allowed, ids, dist, counts);
}
int fvh_hnsw_evaluate_search_quality(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, uint32_t ef, float* out3,
                                     uint64_t* queries_evaluated) {
  SearchQuality s{};
  const int rc = ((HNSWIndex*)p)->evaluate_search_quality(q, B, d, k, ef, &s);
  if (rc) return rc;
  out3[0] = s.avg_recall;
  out3[1] = s.avg_precision;
  out3[2] = s.avg_query_time_ms;
  if (queries_evaluated) *queries_evaluated = s.queries_evaluated;
  return FVDB_OK;
}
// the same three at k up to FVDB_MAX_K_WIDE
int fvh_hnsw_search_exact_wide(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, uint64_t* ids, float* dist, uint32_t* counts) {
  return ((HNSWIndex*)p)->search_exact_wide(q, B, d, k, ids, dist, counts);
}
int fvh_hnsw_search_exact_wide_allowed(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, const uint64_t* allowed,
                                       uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts) {
  return ((HNSWIndex*)p)->search_exact_wide_allowed(q, B, d, k, allowed, n_allowed, ids, dist, counts);
}
// radius search: radius[B]; ids / dist [B][max_results], counts[B], totals[B].  allowed == NULL: no filter
int fvh_hnsw_search_radius(void* p, const float* q, uint32_t B, uint32_t d, const float* radius, uint32_t max_results, uint64_t* ids,
                           float* dist, uint32_t* counts, uint32_t* totals) {
  return ((HNSWIndex*)p)->search_radius(q, B, d, radius, max_results, ids, dist, counts, totals);
}
int fvh_hnsw_search_radius_allowed(void* p, const float* q, uint32_t B, uint32_t d, const float* radius, uint32_t max_results,
                                   const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts,
                                   uint32_t* totals) {
  return ((HNSWIndex*)p)->search_radius_allowed(q, B, d, radius, max_results, allowed, n_allowed, ids, dist, counts, totals);
}
int fvh_hnsw_count_within(void* p, const float* q, uint32_t B, uint32_t d, const float* radius, const uint64_t* allowed,
                          uint64_t n_allowed, uint32_t* totals) {
  return ((HNSWIndex*)p)->count_within(q, B, d, radius, allowed, n_allowed, totals);
}
int fvh_ivf_search_radius(void* p, const float* q, uint32_t B, uint32_t d, const float* radius, uint32_t max_results, uint32_t n_probe,
                          const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts, uint32_t* totals) {
  return ((IVFIndex*)p)->search_radius(q, B, d, radius, max_results, n_probe, allowed, n_allowed, ids, dist, counts, totals);
}
int fvh_hybrid_search_radius(void* p, const float* q, uint32_t B, uint32_t d, const float* radius, uint64_t max_results,
                             uint64_t ivf_n_probe, int search_recent, int search_historical, const uint64_t* allowed, uint64_t n_allowed,
                             double now, uint64_t* ids, float* dist, uint32_t* counts, uint32_t* totals) {
  HybridSearchConfig c;
  c.k = max_results;
  c.ivf_n_probe = ivf_n_probe;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  return ((HybridIndex*)p)->search_radius(q, B, d, radius, c, now, allowed, n_allowed, ids, dist, counts, totals);
}
// diverse search: ids / dist / ranks [B][k] in pick order, counts[B].  allowed == NULL: no filter
void fvh_set_diverse_stage_bytes(uint64_t bytes) { set_diverse_stage_budget(bytes); }  // 0: the default again
uint64_t fvh_diverse_stage_bytes() { return diverse_stage_budget(); }
int fvh_ivf_search_diverse(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, uint32_t fetch_k, float lam, int distinct,
                           uint32_t n_probe, const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* ranks,
                           uint32_t* counts) {
  return ((IVFIndex*)p)->search_diverse(q, B, d, k, fetch_k, lam, distinct != 0, n_probe, allowed, n_allowed, ids, dist, ranks, counts);
}
int fvh_hnsw_search_diverse(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, uint32_t fetch_k, float lam, int distinct,
                            uint32_t ef, const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* ranks,
                            uint32_t* counts) {
  return ((HNSWIndex*)p)->search_diverse(q, B, d, k, fetch_k, lam, distinct != 0, ef, allowed, n_allowed, ids, dist, ranks, counts);
}
int fvh_hybrid_search_diverse(void* p, const float* q, uint32_t B, uint32_t d, uint64_t k, uint32_t fetch_k, float lam, int distinct,
                              uint64_t hnsw_ef, uint64_t ivf_n_probe, int search_recent, int search_historical, const uint64_t* allowed,
                              uint64_t n_allowed, double now, uint64_t* ids, float* dist, uint32_t* ranks, uint32_t* counts) {
  HybridSearchConfig c;
  c.k = k;
  c.hnsw_ef = hnsw_ef;
  c.ivf_n_probe = ivf_n_probe;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  return ((HybridIndex*)p)->search_diverse(q, B, d, c, fetch_k, lam, distinct != 0, now, allowed, n_allowed, ids, dist, ranks, counts);
}
int fvh_hybrid_search_diverse_groups(void* p, const float* q, uint32_t B, uint32_t d, uint64_t k, uint32_t fetch_k, float lam,
                                     int distinct, uint64_t hnsw_ef, uint64_t ivf_n_probe, int search_recent, int search_historical,
                                     const uint64_t* allow_ids, const uint64_t* allow_off, const uint8_t* filtered, uint32_t G,
                                     const uint32_t* group_of_query, double now, uint64_t* ids, float* dist, uint32_t* ranks,
                                     uint32_t* counts) {
  HybridSearchConfig c;
  c.k = k;
  c.hnsw_ef = hnsw_ef;
  c.ivf_n_probe = ivf_n_probe;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  const AllowGroups groups{allow_ids, allow_off, filtered, G, group_of_query};
  return ((HybridIndex*)p)->search_diverse_groups(q, B, d, c, fetch_k, lam, distinct != 0, groups, now, ids, dist, ranks, counts);
}
// grouped search: k groups of up to group_size members by the cells of column `column` of the
// metadata table `meta`; ctx = the context of the index.  ids / dist / ranks [B][k][group_size], members /
// totals / key_tags / key_vals [B][k], groups / flags [B].  allowed == NULL: no filter
int fvh_ivf_search_grouped(void* p, fvdb_ctx* ctx, fvdb_meta* meta, uint32_t column, const float* q, uint32_t B,
                           uint32_t d, uint32_t k, uint32_t group_size, uint32_t fetch_k, int distinct, int missing, uint32_t n_probe,
                           const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* ranks, uint32_t* members,
                           uint32_t* totals, uint8_t* key_tags, uint64_t* key_vals, uint32_t* groups, uint32_t* flags) {
  return search_grouped(*(IVFIndex*)p, ctx, GroupBy{meta, column}, q, B, d, k, group_size, fetch_k, distinct != 0, missing, n_probe,
                        allowed, n_allowed, GroupedOut{ids, dist, ranks, members, totals, key_tags, key_vals, groups, flags});
}
int fvh_hnsw_search_grouped(void* p, fvdb_ctx* ctx, fvdb_meta* meta, uint32_t column, const float* q, uint32_t B,
                            uint32_t d, uint32_t k, uint32_t group_size, uint32_t fetch_k, int distinct, int missing, uint32_t ef,
                            const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* ranks, uint32_t* members,
                            uint32_t* totals, uint8_t* key_tags, uint64_t* key_vals, uint32_t* groups, uint32_t* flags) {
  return search_grouped(*(HNSWIndex*)p, ctx, GroupBy{meta, column}, q, B, d, k, group_size, fetch_k, distinct != 0, missing, ef,
                        allowed, n_allowed, GroupedOut{ids, dist, ranks, members, totals, key_tags, key_vals, groups, flags});
}
int fvh_hybrid_search_grouped(void* p, fvdb_ctx* ctx, fvdb_meta* meta, uint32_t column, const float* q, uint32_t B,
                              uint32_t d, uint64_t k, uint32_t group_size, uint32_t fetch_k, int distinct, int missing, uint64_t hnsw_ef,
                              uint64_t ivf_n_probe, int search_recent, int search_historical, const uint64_t* allowed,
                              uint64_t n_allowed, double now, uint64_t* ids, float* dist, uint32_t* ranks, uint32_t* members,
                              uint32_t* totals, uint8_t* key_tags, uint64_t* key_vals, uint32_t* groups, uint32_t* flags) {
  HybridSearchConfig c;
  c.k = k;
  c.hnsw_ef = hnsw_ef;
  c.ivf_n_probe = ivf_n_probe;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  return search_grouped(*(HybridIndex*)p, ctx, GroupBy{meta, column}, q, B, d, c, group_size, fetch_k, distinct != 0, missing, now,
                        allowed, n_allowed, GroupedOut{ids, dist, ranks, members, totals, key_tags, key_vals, groups, flags});
}
int fvh_hnsw_evaluate_search_quality_wide(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, uint32_t ef, float* out3,
                                          uint64_t* queries_evaluated) {
  SearchQuality s{};
  const int rc = ((HNSWIndex*)p)->evaluate_search_quality_wide(q, B, d, k, ef, &s);
  if (rc) return rc;
  out3[0] = s.avg_recall;
  out3[1] = s.avg_precision;
  out3[2] = s.avg_query_time_ms;
  if (queries_evaluated) *queries_evaluated = s.queries_evaluated;
  return FVDB_OK;
}
// search quality over a grid: the figures of `g` into the caller's arrays, rows x cols floats each
static int grid_out(const QualityGrid& g, float* out_recall, float* out_precision, float* out_ms, uint64_t* queries_evaluated) {
  std::memcpy(out_recall, g.avg_recall.data(), g.avg_recall.size() * 4);
  std::memcpy(out_precision, g.avg_precision.data(), g.avg_precision.size() * 4);
  if (out_ms) *out_ms = g.avg_query_time_ms;
  if (queries_evaluated) *queries_evaluated = g.queries_evaluated;
  return FVDB_OK;
}
// evaluate_search_quality (_wide above k = FVDB_MAX_K) at every listed ef from one exact search; out_recall /
// out_precision: E floats each
int fvh_hnsw_quality_by_ef(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, const uint32_t* efs, uint32_t E,
                           float* out_recall, float* out_precision, float* out_ms, uint64_t* queries_evaluated) {
  QualityGrid g;
  const int rc = ((HNSWIndex*)p)->quality_by_ef(q, B, d, k, efs, E, out_recall && out_precision ? &g : nullptr);
  return rc ? rc : grid_out(g, out_recall, out_precision, out_ms, queries_evaluated);
}
void fvh_hnsw_set_scan_cutoff(void* p, uint64_t nodes) { ((HNSWIndex*)p)->set_scan_cutoff(nodes); }
uint64_t fvh_hnsw_scan_cutoff(void* p) { return ((HNSWIndex*)p)->scan_cutoff(); }
void* fvh_hnsw_device_graph(void* p) { return ((HNSWIndex*)p)->device_graph(); }
int fvh_hnsw_search_allowed_groups(void* p, const float* q, uint32_t B, uint32_t d, uint32_t k, uint32_t ef, const uint64_t* allowed,
                                   const uint64_t* off, const uint8_t* filtered, uint32_t G, const uint32_t* group_of_query,
                                   uint64_t* ids, float* dist, uint32_t* counts) {
  return ((HNSWIndex*)p)->search_allowed_groups(q, B, d, k, ef, AllowGroups{allowed, off, filtered, G, group_of_query}, ids, dist, counts);
}
uint64_t fvh_hnsw_mask_builds(void* p) { return ((HNSWIndex*)p)->mask_builds(); }
uint64_t fvh_hnsw_node_count(void* p) { return ((HNSWIndex*)p)->node_count(); }
uint64_t fvh_hnsw_active_count(void* p) { return ((HNSWIndex*)p)->active_count(); }
int fvh_hnsw_entry_point(void* p, uint64_t* out) { return ((HNSWIndex*)p)->entry_point(out) ? 0 : FVDB_E_NOT_FOUND; }
int64_t fvh_hnsw_level(void* p, uint64_t id) { return ((HNSWIndex*)p)->level_of(id); }
int64_t fvh_hnsw_neighbors(void* p, uint64_t id, uint32_t layer, uint64_t* out, uint64_t cap) {
  return ((HNSWIndex*)p)->neighbors(id, layer, out, cap);
}
int fvh_hnsw_mark_deleted(void* p, uint64_t id) { return ((HNSWIndex*)p)->mark_deleted(id); }
int fvh_hnsw_is_deleted(void* p, uint64_t id) { return ((HNSWIndex*)p)->is_deleted(id); }
int fvh_hnsw_bulk_build(void* p, const uint64_t* ids, const float* v, uint64_t n, uint32_t d, const int64_t* levels) {
  return ((HNSWIndex*)p)->bulk_build(ids, v, n, d, levels);
}
int fvh_hnsw_restore(void* p, const uint64_t* ids, const float* v, uint64_t n, uint32_t d, const uint32_t* levels,
                     const uint64_t* off, const uint64_t* nbrs, uint64_t entry) {
  return ((HNSWIndex*)p)->restore(ids, v, n, d, levels, off, nbrs, entry);
}
uint64_t fvh_hnsw_graph_slots(void* p) { return ((HNSWIndex*)p)->graph_slots(); }
uint64_t fvh_hnsw_graph_edges(void* p) { return ((HNSWIndex*)p)->graph_edges(); }
void fvh_hnsw_export_graph(void* p, uint64_t* ids, uint32_t* levels, uint64_t* off, uint64_t* nbrs) {
  ((HNSWIndex*)p)->export_graph(ids, levels, off, nbrs);
}
int fvh_hnsw_get_vector(void* p, uint64_t id, float* out) {
  HNSWIndex* h = (HNSWIndex*)p;
  const float* v = h->vector_of(id);
  if (!v) return FVDB_E_NOT_FOUND;
  std::memcpy(out, v, h->dimension() * sizeof(float));
  return 0;
}
uint64_t fvh_hnsw_dist_evals(void* p) { return ((HNSWIndex*)p)->dist_evals(); }
uint64_t fvh_hnsw_hops(void* p) { return ((HNSWIndex*)p)->hops(); }
void fvh_hnsw_set_threads(void* p, int t) { ((HNSWIndex*)p)->set_threads(t); }
void fvh_hnsw_set_device_traversal(void* p, int on) { ((HNSWIndex*)p)->set_device_traversal(on != 0); }
int fvh_hnsw_device_traversal(void* p) { return ((HNSWIndex*)p)->device_traversal(); }
uint64_t fvh_hnsw_device_fallbacks(void* p) { return ((HNSWIndex*)p)->device_fallbacks(); }
int fvh_hnsw_tie_restarts(void* p, uint64_t* queries, uint64_t* again) { return ((HNSWIndex*)p)->tie_restarts(queries, again); }
int fvh_hnsw_graph_kernel_times(void* p, float* ms_sum, uint32_t* launches, uint64_t* rows_scored, uint64_t* hops) {
  return ((HNSWIndex*)p)->graph_kernel_times(ms_sum, launches, rows_scored, hops);
}
uint32_t fvh_hnsw_dimension(void* p) { return ((HNSWIndex*)p)->dimension(); }

// ---- HybridIndex ----
// one row_dtype for the graph and the lists
void* fvh_hybrid_new_ex(fvdb_ctx* ctx_ivf, fvdb_ctx* ctx_hnsw, double recent_threshold_s, uint64_t migration_batch_size,
                        int auto_migrate, uint64_t min_ivf_training_size, uint32_t M, uint32_t M0, uint32_t efc,
                        uint64_t hseed, uint32_t n_clusters, uint32_t n_probe, uint32_t train_size, uint32_t max_iter,
                        uint64_t iseed, int row_dtype) {
  HybridConfig c;
  c.recent_threshold_s = recent_threshold_s;
  c.migration_batch_size = migration_batch_size;
  c.auto_migrate = auto_migrate != 0;
  c.min_ivf_training_size = min_ivf_training_size;
  c.hnsw.max_connections = M;
  c.hnsw.max_connections_layer_0 = M0;
  c.hnsw.ef_construction = efc;
  c.hnsw.seed = hseed;
  c.ivf.n_clusters = n_clusters;
  c.ivf.n_probe = n_probe;
  c.ivf.train_size = train_size;
  c.ivf.max_iterations = max_iter;
  c.ivf.seed = iseed;
  c.set_row_dtype(row_dtype);
  if (!c.ivf.is_valid() || !(recent_threshold_s > 0) || migration_batch_size == 0 || !row_dtype_ok(row_dtype)) return nullptr;
  return new (std::nothrow) HybridIndex(ctx_ivf, ctx_hnsw, c);
}

void* fvh_hybrid_new(fvdb_ctx* ctx_ivf, fvdb_ctx* ctx_hnsw, double recent_threshold_s, uint64_t migration_batch_size,
                     int auto_migrate, uint64_t min_ivf_training_size, uint32_t M, uint32_t M0, uint32_t efc,
                     uint64_t hseed, uint32_t n_clusters, uint32_t n_probe, uint32_t train_size, uint32_t max_iter,
                     uint64_t iseed) {
  HybridConfig c;
  c.recent_threshold_s = recent_threshold_s;
  c.migration_batch_size = migration_batch_size;
  c.auto_migrate = auto_migrate != 0;
  c.min_ivf_training_size = min_ivf_training_size;
  c.hnsw.max_connections = M;
  c.hnsw.max_connections_layer_0 = M0;
  c.hnsw.ef_construction = efc;
  c.hnsw.seed = hseed;
  c.ivf.n_clusters = n_clusters;
  c.ivf.n_probe = n_probe;
  c.ivf.train_size = train_size;
  c.ivf.max_iterations = max_iter;
  c.ivf.seed = iseed;
  if (!c.ivf.is_valid() || !(recent_threshold_s > 0) || migration_batch_size == 0) return nullptr;
  return new (std::nothrow) HybridIndex(ctx_ivf, ctx_hnsw, c);
}
void fvh_hybrid_free(void* p) { delete (HybridIndex*)p; }
int fvh_hybrid_initialize(void* p, const float* x, uint64_t n, uint32_t d) {
  return ((HybridIndex*)p)->initialize(x, n, d);
}
int fvh_hybrid_set_ivf_centroids(void* p, const float* c, uint32_t d) {
  return ((HybridIndex*)p)->set_ivf_centroids(c, d);
}
int fvh_hybrid_insert(void* p, uint64_t id, const float* v, uint32_t d, double ts, double now, int64_t level) {
  return ((HybridIndex*)p)->insert_with_timestamp(id, v, d, ts, now, level);
}
int fvh_hybrid_bulk_insert(void* p, const uint64_t* ids, const float* v, uint64_t n, uint32_t d, const double* ts,
                           double now) {
  return ((HybridIndex*)p)->bulk_insert(ids, v, n, d, ts, now);
}
int fvh_hybrid_bulk_insert_sharded(void* p, const uint64_t* ids, const float* v, uint64_t n, uint32_t d,
                                   const double* ts, double now, uint32_t rank, uint32_t world, uint32_t* owner_out) {
  return ((HybridIndex*)p)->bulk_insert_sharded(ids, v, n, d, ts, now, rank, world, owner_out);
}
int fvh_hybrid_search(void* p, const float* q, uint32_t B, uint32_t d, uint64_t k, uint64_t ef, uint64_t nprobe,
                      int search_recent, int search_historical, uint64_t recent_k, uint64_t historical_k, double now,
                      uint64_t* ids, float* dist, uint32_t* counts) {
  HybridSearchConfig c;
  c.k = k;
  c.hnsw_ef = ef;
  c.ivf_n_probe = nprobe;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  c.recent_k = recent_k;
  c.historical_k = historical_k;
  return ((HybridIndex*)p)->search(q, B, d, c, now, ids, dist, counts);
}
int fvh_hybrid_search_exact(void* p, const float* q, uint32_t B, uint32_t d, uint64_t k, int search_recent, int search_historical,
                            double now, uint64_t* ids, float* dist, uint32_t* counts) {
  HybridSearchConfig c;
  c.k = k;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  return ((HybridIndex*)p)->search_exact(q, B, d, c, now, ids, dist, counts);
}
int fvh_hybrid_evaluate_search_quality(void* p, const float* q, uint32_t B, uint32_t d, uint64_t k, uint64_t ef, uint64_t nprobe,
                                       double now, float* out3, uint64_t* queries_evaluated) {
  HybridSearchConfig c;
  c.k = k;
  c.hnsw_ef = ef;
  c.ivf_n_probe = nprobe;
  SearchQuality s{};
  const int rc = ((HybridIndex*)p)->evaluate_search_quality(q, B, d, c, now, &s);
  if (rc) return rc;
  out3[0] = s.avg_recall;
  out3[1] = s.avg_precision;
  out3[2] = s.avg_query_time_ms;
  if (queries_evaluated) *queries_evaluated = s.queries_evaluated;
  return FVDB_OK;
}
// the same two at k up to FVDB_MAX_K_WIDE
int fvh_hybrid_search_exact_wide(void* p, const float* q, uint32_t B, uint32_t d, uint64_t k, int search_recent, int search_historical,
                                 double now, uint64_t* ids, float* dist, uint32_t* counts) {
  HybridSearchConfig c;
  c.k = k;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  return ((HybridIndex*)p)->search_exact_wide(q, B, d, c, now, ids, dist, counts);
}
int fvh_hybrid_evaluate_search_quality_wide(void* p, const float* q, uint32_t B, uint32_t d, uint64_t k, uint64_t ef, uint64_t nprobe,
                                            double now, float* out3, uint64_t* queries_evaluated) {
  HybridSearchConfig c;
  c.k = k;
  c.hnsw_ef = ef;
  c.ivf_n_probe = nprobe;
  SearchQuality s{};
  const int rc = ((HybridIndex*)p)->evaluate_search_quality_wide(q, B, d, c, now, &s);
  if (rc) return rc;
  out3[0] = s.avg_recall;
  out3[1] = s.avg_precision;
  out3[2] = s.avg_query_time_ms;
  if (queries_evaluated) *queries_evaluated = s.queries_evaluated;
  return FVDB_OK;
}
// evaluate_search_quality (_wide above k = FVDB_MAX_K) at every pair (efs[i], n_probes[j]) in one call (DESIGN.md section
// 9r); out_recall / out_precision: max(E, 1) x max(P, 1) floats each, row-major
int fvh_hybrid_quality_grid(void* p, const float* q, uint32_t B, uint32_t d, uint64_t k, int search_recent, int search_historical,
                            uint64_t recent_k, uint64_t historical_k, const uint32_t* efs, uint32_t E, const uint32_t* n_probes,
                            uint32_t P, double now, float* out_recall, float* out_precision, float* out_ms,
                            uint64_t* queries_evaluated) {
  HybridSearchConfig c;
  c.k = k;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  c.recent_k = recent_k;
  c.historical_k = historical_k;
  QualityGrid g;
  const int rc = ((HybridIndex*)p)->quality_grid(q, B, d, c, efs, E, n_probes, P, now, out_recall && out_precision ? &g : nullptr);
  return rc ? rc : grid_out(g, out_recall, out_precision, out_ms, queries_evaluated);
}
int fvh_hybrid_search_allowed(void* p, const float* q, uint32_t B, uint32_t d, uint64_t k, uint64_t ef, uint64_t nprobe,
                              int search_recent, int search_historical, uint64_t recent_k, uint64_t historical_k,
                              const uint64_t* allowed, uint64_t n_allowed, double now, uint64_t* ids, float* dist,
                              uint32_t* counts) {
  HybridSearchConfig c;
  c.k = k;
  c.hnsw_ef = ef;
  c.ivf_n_probe = nprobe;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  c.recent_k = recent_k;
  c.historical_k = historical_k;
  return ((HybridIndex*)p)->search_allowed(q, B, d, c, allowed, n_allowed, now, ids, dist, counts);
}
int fvh_hybrid_search_allowed_groups(void* p, const float* q, uint32_t B, uint32_t d, uint64_t k, uint64_t ef, uint64_t nprobe,
                                     int search_recent, int search_historical, const uint64_t* allowed, const uint64_t* off,
                                     const uint8_t* filtered, uint32_t G, const uint32_t* group_of_query, double now,
                                     uint64_t* ids, float* dist, uint32_t* counts) {
  HybridSearchConfig c;
  c.k = k;
  c.hnsw_ef = ef;
  c.ivf_n_probe = nprobe;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  return ((HybridIndex*)p)->search_allowed_groups(q, B, d, c, AllowGroups{allowed, off, filtered, G, group_of_query}, now, ids, dist,
                                                  counts);
}
// search_with_filter (src/hybrid/core.rs:513-549): `matches(id, user)` is the host application's metadata lookup +
// MetadataFilter::matches (0 = no metadata or no match); NULL = no filter.
int fvh_hybrid_search_with_filter(void* p, const float* q, uint32_t B, uint32_t d, uint64_t k,
                                  int (*matches)(uint64_t, void*), void* user, double now, uint64_t* ids, float* dist,
                                  uint32_t* counts) {
  return ((HybridIndex*)p)->search_with_filter(q, B, d, k, matches, user, now, ids, dist, counts);
}
int fvh_hybrid_search_dev(void* p, const float* q_dev, uint32_t B, uint32_t d, uint64_t k, uint64_t ef, uint64_t nprobe,
                          int search_recent, int search_historical, uint64_t recent_k, uint64_t historical_k,
                          double now, uint64_t* ids, float* dist, uint32_t* counts) {
  HybridSearchConfig c;
  c.k = k;
  c.hnsw_ef = ef;
  c.ivf_n_probe = nprobe;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  c.recent_k = recent_k;
  c.historical_k = historical_k;
  return ((HybridIndex*)p)->search_dev(q_dev, B, d, c, now, ids, dist, counts);
}
int fvh_hybrid_search_dev_begin(void* p, uint32_t slot, const float* q_dev, uint32_t B, uint32_t d, uint64_t k, uint64_t ef,
                                uint64_t nprobe, int search_recent, int search_historical, uint64_t recent_k,
                                uint64_t historical_k, double now) {
  HybridSearchConfig c;
  c.k = k;
  c.hnsw_ef = ef;
  c.ivf_n_probe = nprobe;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  c.recent_k = recent_k;
  c.historical_k = historical_k;
  return ((HybridIndex*)p)->search_dev_begin(slot, q_dev, B, d, c, now);
}
// multi-GPU: see HybridIndex::attach_comm / search_sharded_begin in fvdb_host.hpp
int fvh_hybrid_attach_comm(void* p, fvdb_comm* comm) { return ((HybridIndex*)p)->attach_comm(comm); }
int fvh_hybrid_search_sharded_begin(void* p, uint32_t slot, const float* q_dev, uint32_t B, uint32_t d, uint64_t k,
                                    uint64_t ef, uint64_t nprobe, int search_recent, int search_historical,
                                    uint64_t recent_k, uint64_t historical_k, int mode, double now) {
  HybridSearchConfig c;
  c.k = k;
  c.hnsw_ef = ef;
  c.ivf_n_probe = nprobe;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  c.recent_k = recent_k;
  c.historical_k = historical_k;
  return ((HybridIndex*)p)->search_sharded_begin(slot, q_dev, B, d, c, mode, now);
}
int fvh_hybrid_search_allowed_sharded_begin(void* p, uint32_t slot, const float* q_dev, uint32_t B, uint32_t d, uint64_t k,
                                            uint64_t ef, uint64_t nprobe, int search_recent, int search_historical,
                                            uint64_t recent_k, uint64_t historical_k, int mode, const uint64_t* allowed,
                                            uint64_t n_allowed, double now) {
  HybridSearchConfig c;
  c.k = k;
  c.hnsw_ef = ef;
  c.ivf_n_probe = nprobe;
  c.search_recent = search_recent != 0;
  c.search_historical = search_historical != 0;
  c.recent_k = recent_k;
  c.historical_k = historical_k;
  return ((HybridIndex*)p)->search_allowed_sharded_begin(slot, q_dev, B, d, c, mode, allowed, n_allowed, now);
}
int fvh_hybrid_search_sharded_end(void* p, uint32_t slot, uint64_t* ids, float* dist, uint32_t* counts) {
  return ((HybridIndex*)p)->search_sharded_end(slot, ids, dist, counts);
}
uint32_t fvh_hybrid_sharded_rows(void* p, uint32_t B, int mode) { return ((HybridIndex*)p)->sharded_rows(B, mode); }
// pure host logic of the multi-GPU path, callable without a GPU (CPU tests): list placement and the hybrid merge
void fvh_plan_list_owners(const uint64_t* sizes, uint32_t nlist, uint32_t world, uint32_t* owner) {
  fvdbh::plan_list_owners_host(sizes, nlist, world, owner);
}
void fvh_merge_parts(uint32_t B, uint32_t k, uint32_t rk, uint32_t hk, const uint64_t* rid, const float* rd,
                     const uint32_t* rc, const uint64_t* hid, const float* hd, const uint32_t* hc, uint64_t* ids,
                     float* dist, uint32_t* counts) {
  fvdbh::merge_parts_host(B, k, rk, hk, rid, rd, rc, hid, hd, hc, ids, dist, counts);
}
int fvh_hybrid_search_dev_end(void* p, uint32_t slot, uint64_t* ids, float* dist, uint32_t* counts) {
  return ((HybridIndex*)p)->search_dev_end(slot, ids, dist, counts);
}
// device traversal split in two (several batches in flight): begin returns 1 when the launch is in flight in `slot`,
// 0 when this search cannot run on the device path (call fvh_hnsw_search_dev instead of _end), < 0 on error
int fvh_hnsw_search_dev_begin(void* p, uint32_t slot, const float* q_dev, uint32_t B, uint32_t d, uint32_t k, uint32_t ef) {
  int rc = 0;
  const bool started = ((HNSWIndex*)p)->search_dev_begin(q_dev, B, d, k, ef, &rc, slot);
  if (rc) return rc < 0 ? rc : -rc;
  return started ? 1 : 0;
}
int fvh_hnsw_search_dev_end(void* p, uint32_t slot, const float* q_dev, uint32_t B, uint32_t d, uint32_t k, uint32_t ef,
                            uint64_t* ids, float* dist, uint32_t* counts) {
  return ((HNSWIndex*)p)->search_dev_end(q_dev, B, d, k, ef, ids, dist, counts, slot);
}
int fvh_hnsw_search_dev(void* p, const float* q_dev, uint32_t B, uint32_t d, uint32_t k, uint32_t ef, uint64_t* ids,
                        float* dist, uint32_t* counts) {
  return ((HNSWIndex*)p)->search_dev(q_dev, B, d, k, ef, ids, dist, counts);
}
int fvh_hybrid_delete(void* p, uint64_t id, double now) { return ((HybridIndex*)p)->remove(id, now); }
uint64_t fvh_hybrid_migrate(void* p, double thr, double now) {
  return ((HybridIndex*)p)->migrate_with_threshold(thr, now);
}
int fvh_hybrid_from_parts(void* p, const uint64_t* ids, const double* ts, uint64_t n, uint64_t recent_count,
                          uint64_t historical_count, int ivf_trained) {
  return ((HybridIndex*)p)->from_parts(ids, ts, n, recent_count, historical_count, ivf_trained != 0);
}
int fvh_hybrid_vacuum(void* p, uint64_t* hnsw_removed, uint64_t* ivf_removed) {
  return ((HybridIndex*)p)->vacuum(hnsw_removed, ivf_removed);
}
int fvh_hybrid_retrain_historical(void* p, uint32_t n_clusters, uint32_t n_probe, uint32_t train_size,
                                  uint32_t max_iterations, uint64_t seed, uint64_t* out4) {
  IVFConfig c;
  if (int rc = retrain_config(n_clusters, n_probe, train_size, max_iterations, seed, &c)) return rc;
  IVFIndex::RetrainResult r{};
  const int rc = ((HybridIndex*)p)->retrain_historical(c, &r);
  if (!rc && out4) std::memcpy(out4, &r, sizeof r);
  return rc;
}
int fvh_ivf_vacuum(void* p, uint64_t* removed) { return ((IVFIndex*)p)->vacuum(removed); }
uint64_t fvh_hnsw_vacuum(void* p) { return ((HNSWIndex*)p)->vacuum(); }
int fvh_hnsw_vacuum_ex(void* p, uint64_t* removed) { return ((HNSWIndex*)p)->vacuum(removed); }
void fvh_hnsw_set_resident_vacuum(void* p, int on) { ((HNSWIndex*)p)->set_resident_vacuum(on != 0); }
int fvh_hnsw_resident_vacuum(void* p) { return ((HNSWIndex*)p)->resident_vacuum(); }
void fvh_hnsw_set_vacuum_keep_rows(void* p, int on) { ((HNSWIndex*)p)->set_vacuum_keep_rows(on != 0); }
// returns HNSWIndex::VacuumPath of the last vacuum that removed something
int fvh_hnsw_vacuum_info(void* p, fvdb_graph_maintenance_info_t* out) { return ((HNSWIndex*)p)->vacuum_info(out); }
uint64_t fvh_hnsw_store_rows(void* p) { return ((HNSWIndex*)p)->store_rows(); }
// graph stats and health.  out5: total_nodes, total_edges, max_layer, connected_components, and
// avg_degree's f32 bits in the low half of the fifth word
int fvh_hnsw_graph_stats(void* p, uint64_t* out5) {
  HNSWIndex::GraphStats s;
  const int rc = ((HNSWIndex*)p)->get_graph_stats(&s);
  uint32_t bits;
  std::memcpy(&bits, &s.avg_degree, 4);
  out5[0] = s.total_nodes;
  out5[1] = s.total_edges;
  out5[2] = s.max_layer;
  out5[3] = s.connected_components;
  out5[4] = bits;
  return rc;
}
uint32_t fvh_hnsw_max_level(void* p) { return ((HNSWIndex*)p)->get_max_level(); }
void fvh_hnsw_level_distribution(void* p, uint64_t* out) { ((HNSWIndex*)p)->get_level_distribution(out); }
// *path: HNSWIndex::HealthPath of the form that ran
int fvh_hnsw_graph_health(void* p, uint32_t flags, fvdb_graph_health_t* out, int* path) {
  return ((HNSWIndex*)p)->graph_health(out, flags, path);
}
// out: room for active_count() ids
int fvh_hnsw_unreachable(void* p, uint64_t* out, uint64_t cap, uint64_t* n_out) {
  std::vector<uint64_t> ids;
  const int rc = ((HNSWIndex*)p)->unreachable(&ids);
  *n_out = ids.size();
  if (!rc && ids.size() <= cap && !ids.empty()) std::memcpy(out, ids.data(), ids.size() * 8);
  return rc ? rc : (ids.size() <= cap ? FVDB_OK : FVDB_E_INVALID);
}
// labels: room for node_count() entries, in export_graph's node order
int fvh_hnsw_component_labels(void* p, uint64_t* labels) { return ((HNSWIndex*)p)->component_labels(labels); }
// vectors of search hits (includeVectors, bindings/node/src/session.rs:266-281): recent part first, then historical
int fvh_hybrid_get_vectors(void* p, const uint64_t* ids, uint64_t n, float* out, uint8_t* found) {
  return ((HybridIndex*)p)->get_vectors(ids, n, out, found);
}
void fvh_hybrid_set_resident_migration(void* p, int on) { ((HybridIndex*)p)->set_resident_migration(on != 0); }
// returns HybridIndex::MigrationPath of the last migration that had rows to copy
int fvh_hybrid_migration_info(void* p, fvdb_maintenance_info_t* out) { return ((HybridIndex*)p)->migration_info(out); }
uint64_t fvh_hybrid_timestamp_count(void* p) { return ((HybridIndex*)p)->timestamp_count(); }
void fvh_hybrid_export_timestamps(void* p, uint64_t* ids, double* ts) { ((HybridIndex*)p)->export_timestamps(ids, ts); }
uint64_t fvh_hybrid_recent_count(void* p) { return ((HybridIndex*)p)->recent_count(); }
uint64_t fvh_hybrid_historical_count(void* p) { return ((HybridIndex*)p)->historical_count(); }
int fvh_hybrid_is_initialized(void* p) { return ((HybridIndex*)p)->is_initialized(); }
int fvh_hybrid_is_ivf_trained(void* p) { return ((HybridIndex*)p)->is_ivf_trained(); }
void* fvh_hybrid_hnsw(void* p) { return &((HybridIndex*)p)->recent(); }
void fvh_hybrid_set_sequential_graph(void* p, int on) { ((HybridIndex*)p)->set_sequential_graph(on != 0); }
int fvh_hybrid_sequential_graph(void* p) { return ((HybridIndex*)p)->sequential_graph(); }
double fvh_hybrid_recent_build_seconds(void* p) { return ((HybridIndex*)p)->recent_build_seconds(); }
void fvh_hybrid_set_blocking_writers(void* p, int on) { ((HybridIndex*)p)->set_blocking_writers(on != 0); }
int fvh_hybrid_blocking_writers(void* p) { return ((HybridIndex*)p)->blocking_writers(); }
void* fvh_hybrid_ivf(void* p) { return &((HybridIndex*)p)->historical(); }

}  // extern "C"
