// ivf_index.cpp — IVFIndex mirror (src/ivf/core.rs, src/ivf/operations.rs) over the C ABI.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "fvdb_host.hpp"

namespace fvdbh {

IVFIndex::IVFIndex(fvdb_ctx* ctx, const IVFConfig& cfg) : ctx_(ctx), cfg_(cfg) {}

IVFIndex::~IVFIndex() {
  drop_mask();  // before the device index it points into
  allowed_q_.release();
  allowed_out_.release();
  diverse_.release();
  if (dev_) fvdb_ivf_destroy(dev_);
}

int IVFIndex::ensure_device(uint32_t dim) {
  if (dev_ && dim_ == dim && dev_clusters_ == cfg_.n_clusters) return FVDB_OK;
  if (dev_) {
    drop_mask();
    fvdb_ivf_destroy(dev_);
    dev_ = nullptr;
  }
  int rc = fvdb_ivf_create_ex(ctx_, dim, cfg_.n_clusters, cfg_.row_dtype, &dev_);
  if (rc) return rc;
  dim_ = dim;
  dev_clusters_ = cfg_.n_clusters;
  return FVDB_OK;
}

// src/ivf/core.rs:240-334
int IVFIndex::train(const float* data, uint64_t n, uint32_t dim, fvdb_train_result* out) {
  if (n == 0 || n < cfg_.n_clusters) return FVDB_E_INSUFFICIENT;
  int rc = ensure_device(dim);
  if (rc) return rc;
  rc = fvdb_ivf_train(dev_, data, n, cfg_.max_iterations, cfg_.seed, out);
  if (rc) return rc;
  trained_ = true;
  where_.clear();
  deleted_.clear();
  total_ = 0;
  return FVDB_OK;
}

// src/ivf/core.rs:509-520
int IVFIndex::set_trained(const float* centroids, uint32_t dim) {
  int rc = ensure_device(dim);
  if (rc) return rc;
  rc = fvdb_ivf_set_centroids(dev_, centroids);
  if (rc) return rc;
  trained_ = true;
  where_.clear();
  deleted_.clear();
  total_ = 0;
  return FVDB_OK;
}

int IVFIndex::get_centroids(float* out) const {
  if (!trained_) return FVDB_E_NOT_TRAINED;
  return fvdb_ivf_get_centroids(dev_, out);
}

void IVFIndex::clear_lists() {
  if (dev_) fvdb_ivf_clear(dev_);
  where_.clear();
  deleted_.clear();
  total_ = 0;
}

// src/ivf/operations.rs:625-645: every row of a soft-deleted id leaves its list, the survivors keep their order.
// The rows never leave HBM (fvdb_ivf_compact drops the rows whose live bit is clear); the ids of the survivors come
// back in sequence order, and with the new list sizes that is every survivor's (list, position).
int IVFIndex::vacuum(uint64_t* removed_out) {
  const uint64_t removed = deleted_.size();
  if (removed_out) *removed_out = removed;
  if (removed == 0) return FVDB_OK;
  if (dev_) {
    if (live_again_) {  // rows inserted under an id deleted earlier carry a live bit: the reference drops them by id
      std::vector<uint32_t> cl, ps;
      for (uint64_t id : deleted_) {
        auto r = where_.equal_range(id);
        for (auto it = r.first; it != r.second; ++it) {
          cl.push_back(it->second.cluster);
          ps.push_back(it->second.pos);
        }
      }
      int rc = fvdb_ivf_set_deleted(dev_, cl.data(), ps.data(), cl.size(), 1);
      if (rc) return rc;
    }
    std::vector<uint64_t> ids(fvdb_ivf_total_rows(dev_)), sizes(dev_clusters_);
    int rc = fvdb_ivf_compact(dev_, nullptr, ids.data());
    if (rc) return rc;
    rc = fvdb_ivf_list_sizes(dev_, sizes.data());
    if (rc) return rc;
    where_.clear();
    size_t i = 0;
    for (uint32_t c = 0; c < dev_clusters_; ++c)
      for (uint32_t p = 0; p < sizes[c]; ++p) where_.emplace(ids[i++], Loc{c, p});
  }
  total_ -= removed;  // "total_vectors -= removed_count" (:638), counted in ids like the reference
  deleted_.clear();
  live_again_ = false;
  return FVDB_OK;
}

float IVFIndex::size_variance() const {  // operations.rs:552-563, f32 sums in cluster order
  const uint32_t nc = cfg_.n_clusters;
  std::vector<uint64_t> sizes(std::max(nc, dev_clusters_), 0);
  if (dev_) fvdb_ivf_list_sizes(dev_, sizes.data());
  float sum = 0.0f;
  for (uint32_t c = 0; c < nc; ++c) sum += (float)sizes[c];
  const float mean = sum / (float)nc;
  float acc = 0.0f;
  for (uint32_t c = 0; c < nc; ++c) {
    const float t = (float)sizes[c] - mean;
    acc += t * t;
  }
  return acc / (float)nc;
}

// src/ivf/operations.rs:263-288
IVFIndex::ClusterStats IVFIndex::get_cluster_stats() const {
  ClusterStats st{};
  st.n_clusters = cfg_.n_clusters;
  st.total_vectors = total_;
  st.avg_cluster_size = cfg_.n_clusters ? (float)total_ / (float)cfg_.n_clusters : 0.0f;
  st.size_variance = size_variance();
  std::vector<uint64_t> sizes(std::max(cfg_.n_clusters, dev_clusters_), 0);
  if (dev_) fvdb_ivf_list_sizes(dev_, sizes.data());
  for (uint32_t c = 0; c < cfg_.n_clusters; ++c) st.empty_clusters += sizes[c] == 0;
  return st;
}

// src/ivf/operations.rs:329-391
int IVFIndex::evaluate_search_quality(const float* q, uint32_t B, uint32_t dim, uint32_t k, SearchQuality* out) {
  if (B == 0) return FVDB_E_INVALID;  // "No test queries provided"
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  if (!q || !out) return FVDB_E_INVALID;
  if (k == 0 || k > FVDB_MAX_K_WIDE) return FVDB_E_UNSUPPORTED;
  for (uint64_t i = 0; i < (uint64_t)B * dim; ++i)
    if (!(q[i] - q[i] == 0.0f)) return FVDB_E_NONFINITE;
  const auto start = std::chrono::steady_clock::now();
  std::lock_guard<std::mutex> lk(allowed_mu_);  // search_allowed's staging blocks: calls take turns
  const uint64_t bytes = (uint64_t)B * 8;  // recall[B], precision[B]
  int rc;
  if ((rc = allowed_q_.reserve(ctx_, (uint64_t)B * dim * 4, false)) || (rc = allowed_out_.reserve(ctx_, bytes, true))) return rc;
  if ((rc = fvdb_dev_upload(ctx_, allowed_q_.dev, q, (size_t)B * dim * 4))) return rc;
  float* d = (float*)allowed_out_.dev;
  rc = fvdb_ivf_search_quality_dev(dev_, nullptr, 0, (const float*)allowed_q_.dev, B, k, cfg_.n_probe, d, d + B);
  if (rc) return rc;
  if ((rc = fvdb_dev_download_async(ctx_, allowed_out_.host, allowed_out_.dev, (size_t)bytes)) || (rc = fvdb_ctx_synchronize(ctx_)))
    return rc;
  const float* h = (const float*)allowed_out_.host;
  float total_recall = 0.0f, total_precision = 0.0f;
  for (uint32_t b = 0; b < B; ++b) {
    total_recall += h[b];
    total_precision += h[B + b];
  }
  *out = quality_of(total_recall, total_precision, B, start);
  return FVDB_OK;
}

// evaluate_search_quality (operations.rs:329-391) for every n_probe at once: the sums over the queries come from the
// device in query order (fvdb_ivf_quality_curve_dev), the division by B is the reference's (:386-387).
int IVFIndex::quality_curve(const float* q, uint32_t B, uint32_t dim, uint32_t k, const uint64_t* allowed, uint64_t n_allowed,
                            QualityCurve* out) {
  if (B == 0) return FVDB_E_INVALID;  // "No test queries provided"
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  if (!q || !out) return FVDB_E_INVALID;
  if (k == 0 || k > FVDB_MAX_K_WIDE) return FVDB_E_UNSUPPORTED;
  for (uint64_t i = 0; i < (uint64_t)B * dim; ++i)
    if (!(q[i] - q[i] == 0.0f)) return FVDB_E_NONFINITE;
  const auto start = std::chrono::steady_clock::now();
  MaskRef mask;
  int rc;
  if (allowed && (rc = allowed_mask(allowed, n_allowed, &mask))) return rc;
  std::lock_guard<std::mutex> lk(allowed_mu_);  // search_allowed's staging blocks: calls take turns
  const uint32_t nlist = dev_clusters_;
  const uint64_t bytes = (uint64_t)nlist * 8;  // recall sums [nlist], precision sums [nlist]
  if ((rc = allowed_q_.reserve(ctx_, (uint64_t)B * dim * 4, false)) || (rc = allowed_out_.reserve(ctx_, bytes, true))) return rc;
  if ((rc = fvdb_dev_upload(ctx_, allowed_q_.dev, q, (size_t)B * dim * 4))) return rc;
  float* d = (float*)allowed_out_.dev;
  rc = fvdb_ivf_quality_curve_dev(dev_, nullptr, 0, mask.get(), (const float*)allowed_q_.dev, B, k, 0, d, d + nlist);
  if (rc) return rc;
  if ((rc = fvdb_dev_download_async(ctx_, allowed_out_.host, allowed_out_.dev, (size_t)bytes)) || (rc = fvdb_ctx_synchronize(ctx_)))
    return rc;
  const float* h = (const float*)allowed_out_.host;
  out->avg_recall.resize(nlist);
  out->avg_precision.resize(nlist);
  for (uint32_t p = 0; p < nlist; ++p) {
    out->avg_recall[p] = h[p] / (float)B;
    out->avg_precision[p] = h[nlist + p] / (float)B;
  }
  const std::chrono::duration<float, std::milli> elapsed = std::chrono::steady_clock::now() - start;
  out->avg_query_time_ms = elapsed.count() / (float)B;
  out->queries_evaluated = B;
  return FVDB_OK;
}

// "Collect all existing vectors ... train ... clear ... reinsert" (operations.rs:158-186, :231-250) without the rows
// leaving HBM.  The reference's re-insert loop stops at the first DuplicateVector (`?` at :185 / :249): an id stored in
// two lists (the duplicate check is per list, src/ivf/core.rs:128-134) whose copies now meet in one list.  The rows
// before that repeat are in place and the rest are gone; same here, and FVDB_E_DUPLICATE is returned after the swap.
int IVFIndex::rebuild(uint32_t n_clusters, uint32_t max_iterations, uint64_t seed, fvdb_train_result* tr,
                      uint64_t* reinserted) {
  fvdb_ivf* nd = nullptr;
  int rc = fvdb_ivf_create_ex(ctx_, dim_, n_clusters, cfg_.row_dtype, &nd);
  if (rc) return rc;
  rc = fvdb_ivf_train_from(nd, dev_, max_iterations, seed, tr);
  const uint64_t n = fvdb_ivf_total_rows(dev_);
  std::vector<uint32_t> cl(n), pos(n);
  std::vector<uint64_t> ids(n);
  if (!rc) rc = fvdb_ivf_assign_from(nd, dev_, cl.data(), ids.data());
  uint64_t keep = n;
  if (!rc) {
    std::unordered_multimap<uint64_t, uint32_t> seen;  // only ids stored more than once can repeat
    for (uint64_t i = 0; i < n && keep == n; ++i) {
      if (where_.count(ids[i]) < 2) continue;
      auto r = seen.equal_range(ids[i]);
      for (auto it = r.first; it != r.second; ++it)
        if (it->second == cl[i]) keep = i;
      seen.emplace(ids[i], cl[i]);
    }
    rc = fvdb_ivf_refill_from(nd, dev_, keep, pos.data());
  }
  if (rc) {  // the old device index is untouched
    fvdb_ivf_destroy(nd);
    return rc;
  }
  drop_mask();
  fvdb_ivf_destroy(dev_);
  dev_ = nd;
  dev_clusters_ = n_clusters;
  where_.clear();
  for (uint64_t i = 0; i < keep; ++i) where_.emplace(ids[i], Loc{cl[i], pos[i]});
  *reinserted = keep;
  return keep == n ? FVDB_OK : FVDB_E_DUPLICATE;
}

// src/ivf/operations.rs:148-193.  deleted_ is keyed by id and not touched (:148-193 never mention it): a soft-deleted
// row moves with its live bit clear.
int IVFIndex::retrain(const IVFConfig& new_config, RetrainResult* out) {
  if (!trained_) return FVDB_E_NOT_TRAINED;
  const IVFConfig old_config = cfg_;
  const uint64_t old_vectors = total_;
  // :168-169 replace the config and clear `trained` BEFORE train can fail; when it fails for want of rows (or on
  // degenerate data) the reference is left with the new config, untrained, its lists whole.  Mirrored: the old device
  // index stays (dev_clusters_ lists) until a later train() builds one for the new config.
  cfg_ = new_config;
  cfg_.row_dtype = old_config.row_dtype;  // the rows stay where and as they are: a retrain does not change their storage
  trained_ = false;
  const uint64_t n = dev_ ? fvdb_ivf_total_rows(dev_) : 0;
  if (n == 0 || n < cfg_.n_clusters) return FVDB_E_INSUFFICIENT;
  fvdb_train_result tr{};
  uint64_t reinserted = 0;
  const int rc = rebuild(cfg_.n_clusters, cfg_.max_iterations, cfg_.seed, &tr, &reinserted);
  if (rc && rc != FVDB_E_DUPLICATE) {
    if (rc != FVDB_E_INSUFFICIENT && rc != FVDB_E_INVALID) {  // the device's failure, not the reference's: nothing changed
      cfg_ = old_config;
      trained_ = true;
    }
    return rc;
  }
  trained_ = true;
  total_ = reinserted;  // :176 resets the counter, each re-insert counts one
  if (rc) return rc;
  if (out) *out = RetrainResult{old_config.n_clusters, cfg_.n_clusters, old_vectors, tr.converged};
  return FVDB_OK;
}

// src/ivf/operations.rs:195-220
int IVFIndex::add_clusters(uint32_t n_clusters_to_add, uint64_t* vectors_reassigned) {
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (n_clusters_to_add == 0) return FVDB_E_INVALID;  // "Cannot add 0 clusters"
  IVFConfig nc = cfg_;
  nc.n_clusters += n_clusters_to_add;
  RetrainResult r{};
  const int rc = retrain(nc, &r);
  if (rc) return rc;
  if (vectors_reassigned) *vectors_reassigned = r.vectors_reassigned;
  return FVDB_OK;
}

// src/ivf/operations.rs:222-260.  total_vectors is NOT reset before the re-inserts (:243-250), so it doubles: kept.
int IVFIndex::optimize_clusters(uint32_t* iterations, float* improvement) {
  if (!trained_) return FVDB_E_NOT_TRAINED;
  const float initial_variance = size_variance();
  const uint64_t n = dev_ ? fvdb_ivf_total_rows(dev_) : 0;
  if (n == 0 || n < cfg_.n_clusters) return FVDB_E_INSUFFICIENT;  // train fails first (:240), nothing has changed
  fvdb_train_result tr{};
  uint64_t reinserted = 0;
  const int rc = rebuild(cfg_.n_clusters, cfg_.max_iterations, cfg_.seed, &tr, &reinserted);
  if (rc && rc != FVDB_E_DUPLICATE) return rc;
  total_ += reinserted;
  if (rc) return rc;
  if (iterations) *iterations = tr.iterations;
  if (improvement) *improvement = std::max(initial_variance - size_variance(), 0.0f);
  return FVDB_OK;
}

int IVFIndex::export_list(uint32_t c, float* rows, uint64_t* ids, uint8_t* live) const {
  if (c >= cfg_.n_clusters) return FVDB_E_INVALID;
  if (!dev_ || c >= dev_clusters_) return FVDB_OK;  // nothing stored yet
  return fvdb_ivf_list_export(dev_, c, rows, ids, live);
}

uint64_t IVFIndex::cluster_size(uint32_t c) const {
  if (!dev_ || c >= cfg_.n_clusters || c >= dev_clusters_) return 0;
  std::vector<uint64_t> sizes(dev_clusters_);
  fvdb_ivf_list_sizes(dev_, sizes.data());
  return sizes[c];
}

// src/ivf/core.rs:493-499
int IVFIndex::find_cluster(const float* v, uint32_t dim, uint32_t* out) {
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  return fvdb_ivf_assign(dev_, v, 1, out);
}

// the per-list duplicate check (InvertedList::insert :128-134) over a batch, in order
std::vector<uint64_t> IVFIndex::accept(const uint64_t* ids, uint64_t n, const uint32_t* clusters, int* first_error) {
  std::vector<uint64_t> keep;
  keep.reserve(n);
  std::unordered_multimap<uint64_t, uint32_t> batch_seen;  // (id -> cluster) accepted earlier in this batch
  for (uint64_t i = 0; i < n; ++i) {
    bool dup = false;
    auto r = where_.equal_range(ids[i]);
    for (auto it = r.first; it != r.second && !dup; ++it) dup = it->second.cluster == clusters[i];
    auto r2 = batch_seen.equal_range(ids[i]);
    for (auto it = r2.first; it != r2.second && !dup; ++it) dup = it->second == clusters[i];
    if (dup) {
      if (first_error && *first_error == 0) *first_error = FVDB_E_DUPLICATE;
      continue;
    }
    batch_seen.emplace(ids[i], clusters[i]);
    keep.push_back(i);
    if (!deleted_.empty() && deleted_.count(ids[i])) live_again_ = true;
  }
  return keep;
}

// rows whose cluster is known: per-list duplicate check, then append
int IVFIndex::place(const uint64_t* ids, const float* v, uint64_t n, const uint32_t* clusters, uint64_t* n_ok,
                    int* first_error) {
  const std::vector<uint64_t> keep = accept(ids, n, clusters, first_error);
  if (n_ok) *n_ok = keep.size();
  if (keep.empty()) return FVDB_OK;
  std::vector<uint32_t> pos(keep.size());
  int rc;
  if (keep.size() == n) {
    rc = fvdb_ivf_add_assigned(dev_, v, ids, n, clusters, pos.data());
  } else {
    std::vector<float> xv(keep.size() * (size_t)dim_);
    std::vector<uint64_t> xi(keep.size());
    std::vector<uint32_t> xc(keep.size());
    for (size_t j = 0; j < keep.size(); ++j) {
      std::memcpy(&xv[j * dim_], v + keep[j] * dim_, dim_ * sizeof(float));
      xi[j] = ids[keep[j]];
      xc[j] = clusters[keep[j]];
    }
    rc = fvdb_ivf_add_assigned(dev_, xv.data(), xi.data(), keep.size(), xc.data(), pos.data());
  }
  if (rc) return rc;
  for (size_t j = 0; j < keep.size(); ++j) where_.emplace(ids[keep[j]], Loc{clusters[keep[j]], pos[j]});
  total_ += keep.size();
  return FVDB_OK;
}

// batch_insert (operations.rs:107-130) with the rows read from a row store in HBM: the assignment pass and the append
// gather them there (fvdb_ivf_assign_from_store, fvdb_ivf_add_assigned_from_store); place()'s checks run in between
int IVFIndex::batch_insert_from_store(const uint64_t* ids, fvdb_store* store, const uint32_t* rows, uint64_t n,
                                      uint64_t* n_ok, int* first_error) {
  if (n_ok) *n_ok = 0;
  if (first_error) *first_error = 0;
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (!store) return FVDB_E_INVALID;
  if (n == 0) return FVDB_OK;
  std::vector<uint32_t> clusters(n);
  int rc = fvdb_ivf_assign_from_store(dev_, store, rows, n, clusters.data());
  if (rc) return rc;
  const std::vector<uint64_t> keep = accept(ids, n, clusters.data(), first_error);
  if (n_ok) *n_ok = keep.size();
  if (keep.empty()) return FVDB_OK;
  std::vector<uint32_t> pos(keep.size());
  if (keep.size() == n) {
    rc = fvdb_ivf_add_assigned_from_store(dev_, store, rows, ids, n, clusters.data(), pos.data());
  } else {  // only the kept rows' indices go down
    std::vector<uint32_t> xr(keep.size()), xc(keep.size());
    std::vector<uint64_t> xi(keep.size());
    for (size_t j = 0; j < keep.size(); ++j) {
      xr[j] = rows[keep[j]];
      xi[j] = ids[keep[j]];
      xc[j] = clusters[keep[j]];
    }
    rc = fvdb_ivf_add_assigned_from_store(dev_, store, xr.data(), xi.data(), keep.size(), xc.data(), pos.data());
  }
  if (rc) return rc;
  for (size_t j = 0; j < keep.size(); ++j) where_.emplace(ids[keep[j]], Loc{clusters[keep[j]], pos[j]});
  total_ += keep.size();
  return FVDB_OK;
}

// src/ivf/core.rs:553-562.  Of the lists that hold the id, the lowest (cluster, position) answers (fvdb_host.hpp).
int IVFIndex::get_vectors(const uint64_t* ids, uint64_t n, float* out, uint8_t* found) {
  if (n == 0) return FVDB_OK;
  if (!ids || !out || !found) return FVDB_E_INVALID;
  std::vector<uint32_t> cl, ps;
  std::vector<uint64_t> at;  // which of the n each location answers
  for (uint64_t i = 0; i < n; ++i) {
    found[i] = 0;
    auto r = where_.equal_range(ids[i]);
    if (r.first == r.second) continue;
    Loc best = r.first->second;
    for (auto it = r.first; it != r.second; ++it)
      if (it->second.cluster < best.cluster || (it->second.cluster == best.cluster && it->second.pos < best.pos)) best = it->second;
    found[i] = 1;
    cl.push_back(best.cluster);
    ps.push_back(best.pos);
    at.push_back(i);
  }
  if (at.empty()) return FVDB_OK;
  if (!dev_) return FVDB_E_NOT_TRAINED;
  if (at.size() == n) return fvdb_ivf_get_rows(dev_, cl.data(), ps.data(), n, out);
  std::vector<float> rows(at.size() * (size_t)dim_);
  const int rc = fvdb_ivf_get_rows(dev_, cl.data(), ps.data(), at.size(), rows.data());
  if (rc) {
    for (uint64_t i : at) found[i] = 0;
    return rc;
  }
  for (size_t j = 0; j < at.size(); ++j) std::memcpy(out + at[j] * dim_, &rows[j * dim_], dim_ * sizeof(float));
  return FVDB_OK;
}

int IVFIndex::get_vector_by_id(uint64_t id, float* out) {
  uint8_t found = 0;
  const int rc = get_vectors(&id, 1, out, &found);
  return rc ? rc : (found ? FVDB_OK : FVDB_E_NOT_FOUND);
}

// src/ivf/core.rs:431-455
int IVFIndex::insert(uint64_t id, const float* v, uint32_t dim) {
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  std::vector<float> rounded;
  v = rows_at_the_door(cfg_.row_dtype, v, dim, rounded);
  uint32_t c = 0;
  int rc = fvdb_ivf_assign(dev_, v, 1, &c);
  if (rc) return rc;
  uint64_t ok = 0;
  int err = 0;
  rc = place(&id, v, 1, &c, &ok, &err);
  if (rc) return rc;
  return ok == 1 ? FVDB_OK : err;
}

// src/ivf/operations.rs:107-130 — per-row outcome like a loop of insert(); one GPU assignment pass
int IVFIndex::batch_insert(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, uint64_t* n_ok,
                           int* first_error) {
  if (n_ok) *n_ok = 0;
  if (first_error) *first_error = 0;
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  if (n == 0) return FVDB_OK;
  std::vector<float> rounded;
  v = rows_at_the_door(cfg_.row_dtype, v, n * dim, rounded);
  std::vector<uint32_t> clusters(n);
  int rc = fvdb_ivf_assign(dev_, v, n, clusters.data());
  if (rc) return rc;
  return place(ids, v, n, clusters.data(), n_ok, first_error);
}

int IVFIndex::batch_insert_assigned(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim,
                                    const uint32_t* clusters, uint64_t* n_ok, int* first_error) {
  if (n_ok) *n_ok = 0;
  if (first_error) *first_error = 0;
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  if (n == 0) return FVDB_OK;
  std::vector<float> rounded;
  v = rows_at_the_door(cfg_.row_dtype, v, n * dim, rounded);
  return place(ids, v, n, clusters, n_ok, first_error);
}

int IVFIndex::assign(const float* v, uint64_t n, uint32_t dim, uint32_t* out) {
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  return fvdb_ivf_assign(dev_, v, n, out);
}

// src/ivf/core.rs:626-681 for a batch (src/ivf/operations.rs:132-145).  k <= FVDB_MAX_K goes through the register
// top-k, a larger k (up to FVDB_MAX_K_WIDE) through the wide selection; the engine refuses anything above that.  Any
// n_probe is served: above FVDB_MAX_K probed lists the engine takes the wide selection by itself.
int IVFIndex::search(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t n_probe, uint64_t* ids,
                     float* dist, uint32_t* counts) {
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  if (k > FVDB_MAX_K) return fvdb_ivf_search_wide(dev_, q, B, k, n_probe, ids, dist, counts);
  return fvdb_ivf_search(dev_, q, B, k, n_probe, ids, dist, counts);
}

int IVFIndex::search_dev(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, uint32_t n_probe, uint64_t* ids_dev,
                         float* dist_dev, uint32_t* counts_dev, fvdb_ctx* on, uint32_t slot) {
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  if (k > FVDB_MAX_K)
    return fvdb_ivf_search_wide_dev_slot(dev_, on, slot, nullptr, q_dev, B, k, n_probe, ids_dev, dist_dev, counts_dev, nullptr);
  return fvdb_ivf_search_dev_slot(dev_, on, slot, q_dev, B, k, n_probe, ids_dev, dist_dev, counts_dev, nullptr);
}

// ---- filtered search ----
int IVFIndex::allowed_mask(const uint64_t* allowed, uint64_t n_allowed, MaskRef* out) {
  if (!trained_ || !dev_) return FVDB_E_NOT_TRAINED;
  if (n_allowed && !allowed) return FVDB_E_INVALID;
  std::lock_guard<std::mutex> lk(mask_mu_);
  const bool same = mask_ && mask_key_.size() == n_allowed &&
                    (n_allowed == 0 || std::memcmp(mask_key_.data(), allowed, n_allowed * 8) == 0);
  if (!same || !mask_fresh(mask_)) {
    drop_mask();
    fvdb_mask* m = nullptr;
    const int rc = fvdb_mask_create_ivf(dev_, allowed, n_allowed, &m);
    if (rc) return rc;
    mask_ = adopt_mask(m);
    mask_key_.assign(allowed, allowed + n_allowed);
    mask_builds_ += 1;
  }
  *out = mask_;
  return FVDB_OK;
}

int IVFIndex::search_dev_masked(const MaskRef& mask, const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, uint32_t n_probe,
                                uint64_t* ids_dev, float* dist_dev, uint32_t* counts_dev, fvdb_ctx* on, uint32_t slot) {
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  if (k > FVDB_MAX_K)
    return fvdb_ivf_search_wide_dev_slot(dev_, on, slot, mask.get(), q_dev, B, k, n_probe, ids_dev, dist_dev, counts_dev, nullptr);
  return fvdb_ivf_search_dev_slot_masked(dev_, on, slot, mask.get(), q_dev, B, k, n_probe, ids_dev, dist_dev, counts_dev, nullptr);
}

int IVFIndex::search_allowed(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t n_probe, const uint64_t* allowed,
                             uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts) {
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  if (B == 0) return FVDB_OK;
  if (k == 0 || k > FVDB_MAX_K_WIDE) return FVDB_E_UNSUPPORTED;
  for (uint64_t i = 0; i < (uint64_t)B * dim; ++i)
    if (!(q[i] - q[i] == 0.0f)) return FVDB_E_NONFINITE;
  MaskRef mask;
  int rc = allowed_mask(allowed, n_allowed, &mask);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(allowed_mu_);  // one staging block: calls take turns
  const uint64_t need = (uint64_t)B * k, bytes = need * 12 + (uint64_t)B * 4;
  if ((rc = allowed_q_.reserve(ctx_, (uint64_t)B * dim * 4, false)) || (rc = allowed_out_.reserve(ctx_, bytes, true))) return rc;
  if ((rc = fvdb_dev_upload(ctx_, allowed_q_.dev, q, (size_t)B * dim * 4))) return rc;
  char* d = (char*)allowed_out_.dev;
  rc = search_dev_masked(mask, (const float*)allowed_q_.dev, B, dim, k, n_probe, (uint64_t*)d, (float*)(d + need * 8),
                         (uint32_t*)(d + need * 12));
  if (rc) return rc;
  if ((rc = fvdb_dev_download_async(ctx_, allowed_out_.host, allowed_out_.dev, (size_t)bytes)) || (rc = fvdb_ctx_synchronize(ctx_)))
    return rc;
  const char* h = (const char*)allowed_out_.host;
  std::memcpy(ids, h, need * 8);
  std::memcpy(dist, h + need * 8, need * 4);
  std::memcpy(counts, h + need * 12, (size_t)B * 4);
  return FVDB_OK;
}

// ---- radius search ----
int IVFIndex::search_radius(const float* q, uint32_t B, uint32_t dim, const float* radius, uint32_t max_results, uint32_t n_probe,
                            const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts,
                            uint32_t* totals) {
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  if (!allowed) return fvdb_ivf_search_radius(dev_, q, B, radius, max_results, n_probe, ids, dist, counts, totals);
  // under an allow-set: search_allowed's refusals, staging block and turn-taking
  if (B == 0) return FVDB_OK;
  const uint32_t k = max_results;
  if (k == 0 || k > FVDB_MAX_K_WIDE) return FVDB_E_UNSUPPORTED;
  for (uint64_t i = 0; i < (uint64_t)B * dim; ++i)
    if (!(q[i] - q[i] == 0.0f)) return FVDB_E_NONFINITE;
  int rc = check_radius(radius, B);
  if (rc) return rc;
  MaskRef mask;
  if ((rc = allowed_mask(allowed, n_allowed, &mask))) return rc;
  std::lock_guard<std::mutex> lk(allowed_mu_);
  const uint64_t need = (uint64_t)B * k, bytes = need * 12 + (uint64_t)B * 8, q_bytes = (uint64_t)B * dim * 4;
  if ((rc = allowed_q_.reserve(ctx_, q_bytes + (uint64_t)B * 4, false)) || (rc = allowed_out_.reserve(ctx_, bytes, true))) return rc;
  char* dq = (char*)allowed_q_.dev;
  if ((rc = fvdb_dev_upload(ctx_, dq, q, (size_t)q_bytes)) || (rc = fvdb_dev_upload(ctx_, dq + q_bytes, radius, (size_t)B * 4))) return rc;
  char* d = (char*)allowed_out_.dev;
  rc = fvdb_ivf_search_radius_dev_slot(dev_, nullptr, 0, mask.get(), (const float*)dq, B, (const float*)(dq + q_bytes), k, n_probe,
                                       (uint64_t*)d, (float*)(d + need * 8), (uint32_t*)(d + need * 12), (uint32_t*)(d + need * 12) + B);
  if (rc) return rc;
  if ((rc = fvdb_dev_download_async(ctx_, allowed_out_.host, allowed_out_.dev, (size_t)bytes)) || (rc = fvdb_ctx_synchronize(ctx_)))
    return rc;
  const char* h = (const char*)allowed_out_.host;
  std::memcpy(ids, h, need * 8);
  std::memcpy(dist, h + need * 8, need * 4);
  std::memcpy(counts, h + need * 12, (size_t)B * 4);
  std::memcpy(totals, h + need * 12 + (size_t)B * 4, (size_t)B * 4);
  return FVDB_OK;
}

// ---- one allow-set per query ----
int IVFIndex::search_allowed_groups(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t n_probe, const AllowGroups& groups,
                                    uint64_t* ids, float* dist, uint32_t* counts) {
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  if (B == 0) return FVDB_OK;
  if (k == 0 || k > FVDB_MAX_K_WIDE) return FVDB_E_UNSUPPORTED;
  if (!groups.valid(B)) return FVDB_E_INVALID;
  for (uint64_t i = 0; i < (uint64_t)B * dim; ++i)
    if (!(q[i] - q[i] == 0.0f)) return FVDB_E_NONFINITE;
  // the masks of this call: held until the results are in, dropped at return
  std::vector<MaskRef> held(groups.G);
  std::vector<fvdb_mask*> masks(groups.G, nullptr);
  int rc;
  for (uint32_t g = 0; g < groups.G; ++g) {
    if (!groups.filtered[g]) continue;
    fvdb_mask* m = nullptr;
    if ((rc = fvdb_mask_create_ivf(dev_, groups.set(g), groups.size(g), &m))) return rc;
    held[g] = adopt_mask(m);
    masks[g] = m;
    std::lock_guard<std::mutex> lk(mask_mu_);
    mask_builds_ += 1;
  }
  std::lock_guard<std::mutex> lk(allowed_mu_);  // one staging block: calls take turns
  const uint64_t need = (uint64_t)B * k, bytes = need * 12 + (uint64_t)B * 4;
  if ((rc = allowed_q_.reserve(ctx_, (uint64_t)B * dim * 4, false)) || (rc = allowed_out_.reserve(ctx_, bytes, true))) return rc;
  if ((rc = fvdb_dev_upload(ctx_, allowed_q_.dev, q, (size_t)B * dim * 4))) return rc;
  char* d = (char*)allowed_out_.dev;
  rc = fvdb_ivf_search_groups_dev_slot(dev_, nullptr, 0, masks.data(), groups.G, groups.group_of_query, (const float*)allowed_q_.dev, B,
                                       k, n_probe, (uint64_t*)d, (float*)(d + need * 8), (uint32_t*)(d + need * 12), nullptr);
  if (rc) return rc;
  if ((rc = fvdb_dev_download_async(ctx_, allowed_out_.host, allowed_out_.dev, (size_t)bytes)) || (rc = fvdb_ctx_synchronize(ctx_)))
    return rc;
  const char* h = (const char*)allowed_out_.host;
  std::memcpy(ids, h, need * 8);
  std::memcpy(dist, h + need * 8, need * 4);
  std::memcpy(counts, h + need * 12, (size_t)B * 4);
  return FVDB_OK;
}

// src/ivf/operations.rs:569-591
int IVFIndex::mark_deleted(uint64_t id) {
  auto r = where_.equal_range(id);
  if (r.first == r.second) return FVDB_E_NOT_FOUND;
  deleted_.insert(id);
  std::vector<uint32_t> cl, ps;
  for (auto it = r.first; it != r.second; ++it) {
    cl.push_back(it->second.cluster);
    ps.push_back(it->second.pos);
  }
  return fvdb_ivf_set_deleted(dev_, cl.data(), ps.data(), cl.size(), 1);
}

}  // namespace fvdbh
