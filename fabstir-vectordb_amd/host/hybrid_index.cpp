// hybrid_index.cpp — HybridIndex mirror (src/hybrid/core.rs): age routing, per-search
// auto-migration, HNSW + IVF search and the stable merge.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fvdb_host.hpp"

namespace fvdbh {

HybridIndex::HybridIndex(fvdb_ctx* ctx_ivf, fvdb_ctx* ctx_hnsw, const HybridConfig& cfg) : ctx_ivf_(ctx_ivf), cfg_(cfg) {
  recent_ = new HNSWIndex(ctx_hnsw, cfg.hnsw);
  historical_ = new IVFIndex(ctx_ivf, cfg.ivf);
}

HybridIndex::~HybridIndex() {
  qual_.release();
  diverse_.release();
  // a batch that still waits for a partner has nothing enqueued for its IVF part; joint chains in flight end with the
  // release of their blocks, as the slots' own do
  for (Pair& p : pairs_) {
    p.q.release();
    p.res.release();
    if (p.done) fvdb_event_destroy(p.done);
  }
  for (Slot& sl : slots_) {
    sl.ivf.release();
    if (sl.ivf_done) fvdb_event_destroy(sl.ivf_done);
    sl.d_q.release();
    if (sl.ivf_ctx && sl.ivf_ctx != ctx_ivf_) fvdb_ctx_destroy(sl.ivf_ctx);
  }
  if (sharded_) fvdb_sharded_destroy(sharded_);
  delete recent_;
  delete historical_;
}

// src/hybrid/core.rs:262-290
int HybridIndex::initialize(const float* data, uint64_t n, uint32_t dim) {
  if (n < cfg_.min_ivf_training_size) {  // HNSW-only mode
    ivf_trained_ = false;
    initialized_ = true;
    return FVDB_OK;
  }
  int rc = historical_->train(data, n, dim, nullptr);
  if (rc) return rc;
  historical_->clear_lists();  // :278-287
  ivf_trained_ = true;
  initialized_ = true;
  return FVDB_OK;
}

int HybridIndex::set_ivf_centroids(const float* c, uint32_t dim) {
  int rc = historical_->set_trained(c, dim);
  if (rc) return rc;
  ivf_trained_ = true;
  initialized_ = true;
  return FVDB_OK;
}

// The write guard.  Waiting happens WITHOUT holding rw_ (a searcher that is about to collect its batches may need the
// read side first), and a begin takes the read side while it marks its slot active, so no batch can start under a
// mutation.
int HybridIndex::write_lock(std::unique_lock<std::shared_mutex>& w) {
  for (;;) {
    w.lock();  // the blocking searches of other threads hold the read side for their whole duration: waited for here
    flush_waiting();  // a batch whose IVF chain still waits for a partner: enqueued now, so that its collector only waits
    if (!busy()) return FVDB_OK;
    w.unlock();  // what is left in flight was begun with search_dev_begin and not collected yet
    if (!writers_wait_) return FVDB_E_INVALID;
    std::unique_lock<std::mutex> lk(slot_mu_);
    slot_cv_.wait(lk, [&] { return !busy_unlocked(); });
  }
}

HybridIndex::Lease::Lease(HybridIndex* h_, uint32_t slot, How how) : h(h_) {
  std::unique_lock<std::mutex> lk(h->slot_mu_);
  if (slot == kAnyFree) {
    h->slot_cv_.wait(lk, [&] {
      for (const Slot& s : h->slots_)
        if (!s.active) return true;
      return false;
    });
    for (uint32_t i = kSlots; i-- > 0;)  // from the top: the low slots are the ones a pipelining caller names
      if (!h->slots_[i].active) {
        slot = i;
        break;
      }
  }
  Slot& s = h->slots_[slot];
  if (s.active != (how == kAdopt)) return;
  s.active = true;
  sl = &s;
}

HybridIndex::Lease::~Lease() {
  if (!sl) return;
  {
    std::lock_guard<std::mutex> lk(h->slot_mu_);
    sl->active = false;
  }
  h->slot_cv_.notify_all();
}

// src/hybrid/core.rs:357-417
int HybridIndex::insert_with_timestamp(uint64_t id, const float* v, uint32_t dim, double ts, double now,
                                       int64_t level) {
  if (!initialized_) return FVDB_E_NOT_INITIALIZED;
  std::unique_lock<std::shared_mutex> w(rw_, std::defer_lock);  // waits for the blocking searches of other threads (write guard)
  if (int rc = write_lock(w)) return rc;
  if (timestamps_.count(id)) return FVDB_E_DUPLICATE;
  bool to_recent = !ivf_trained_ || age_of(now, ts) < cfg_.recent_threshold_s;
  if (to_recent) {
    int rc = recent_->insert(id, v, dim, level);
    if (rc) return rc;
    recent_count_ += 1;
    pending_migration_.push_back({id, ts});
    pending_min_ts_ = std::min(pending_min_ts_, ts);
  } else {
    int rc = historical_->insert(id, v, dim);
    if (rc) return rc;
    historical_count_ += 1;
  }
  timestamps_[id] = ts;
  ts_order_.push_back(id);
  return FVDB_OK;
}

// the recent part of a bulk load: the reference's sequential inserts (levels drawn in order), or the exact nearest-M graph
int HybridIndex::build_recent(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim) {
  const auto t0 = std::chrono::steady_clock::now();
  int rc, err = 0;
  if (!sequential_graph_) {
    rc = recent_->bulk_build(ids, v, n, dim, nullptr);
  } else {
    uint64_t ok = 0;
    rc = recent_->batch_insert(ids, v, n, dim, nullptr, &ok, &err);
  }
  recent_build_s_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rc ? rc : err;
}

int HybridIndex::bulk_route(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const double* ts, double now,
                            std::vector<uint64_t>& hid, std::vector<float>& hv) {
  std::vector<uint64_t> rid;
  std::vector<float> rv;
  std::vector<Pending> queue;
  for (uint64_t i = 0; i < n; ++i) {
    if (timestamps_.count(ids[i])) return FVDB_E_DUPLICATE;
    timestamps_[ids[i]] = ts[i];
    const bool to_recent = !ivf_trained_ || age_of(now, ts[i]) < cfg_.recent_threshold_s;
    auto& I = to_recent ? rid : hid;
    auto& V = to_recent ? rv : hv;
    I.push_back(ids[i]);
    V.insert(V.end(), v + i * dim, v + (i + 1) * dim);
    if (to_recent) queue.push_back({ids[i], ts[i]});
  }
  ts_order_.assign(ids, ids + n);
  if (rid.empty()) return FVDB_OK;
  int rc = build_recent(rid.data(), rv.data(), rid.size(), dim);  // sharded: a replica, every rank builds the same graph
  if (rc) return rc;
  recent_count_ = rid.size();
  for (const Pending& p : queue) {
    pending_migration_.push_back(p);
    pending_min_ts_ = std::min(pending_min_ts_, p.ts);
  }
  return FVDB_OK;
}

// Scale loader: same routing as insert_with_timestamp, but the HNSW part is built in one call (build_recent) and the
// IVF part is assigned/appended in one GPU pass.  Only valid on an index with no vectors yet.
int HybridIndex::bulk_insert(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const double* ts,
                             double now) {
  if (!initialized_) return FVDB_E_NOT_INITIALIZED;
  std::unique_lock<std::shared_mutex> w(rw_);
  if (!ts_order_.empty() || busy()) return FVDB_E_INVALID;
  std::vector<uint64_t> hid;
  std::vector<float> hv;
  int rc = bulk_route(ids, v, n, dim, ts, now, hid, hv);
  if (rc) return rc;
  if (!hid.empty()) {
    uint64_t ok = 0;
    int err = 0;
    rc = historical_->batch_insert(hid.data(), hv.data(), hid.size(), dim, &ok, &err);
    if (rc) return rc;
    if (err) return err;
    historical_count_ = ok;
  }
  return FVDB_OK;
}

// Greedy "largest list to the least loaded rank" placement; ties -> lower rank.
static void plan_list_owners(const std::vector<uint64_t>& sizes, uint32_t world, std::vector<uint32_t>& owner) {
  const size_t nlist = sizes.size();
  std::vector<uint32_t> order(nlist);
  for (size_t i = 0; i < nlist; ++i) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return sizes[a] > sizes[b]; });
  std::vector<uint64_t> load(world, 0);
  owner.assign(nlist, 0);
  for (uint32_t L : order) {
    uint32_t best = 0;
    for (uint32_t r = 1; r < world; ++r)
      if (load[r] < load[best]) best = r;
    owner[L] = best;
    load[best] += sizes[L];
  }
}

// of the rows (ids, v, cl = the list of each) those whose list `owner` gives to `rank`
namespace {
struct Rows {
  std::vector<uint64_t> ids;
  std::vector<float> v;
  std::vector<uint32_t> cl;
};
Rows owned_rows(const std::vector<uint64_t>& ids, const std::vector<float>& v, const std::vector<uint32_t>& cl, uint32_t dim,
                const std::vector<uint32_t>& owner, uint32_t rank) {
  Rows r;
  for (size_t i = 0; i < ids.size(); ++i)
    if (owner[cl[i]] == rank) {
      r.ids.push_back(ids[i]);
      r.cl.push_back(cl[i]);
      r.v.insert(r.v.end(), v.begin() + i * dim, v.begin() + (i + 1) * dim);
    }
  return r;
}
}  // namespace

int HybridIndex::bulk_insert_sharded(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const double* ts,
                                     double now, uint32_t rank, uint32_t world, uint32_t* owner_out) {
  if (cfg_.row_dtype() == FVDB_F16) return FVDB_E_UNSUPPORTED;  // a sharded fp16 hybrid is not served (attach_comm)
  if (!initialized_) return FVDB_E_NOT_INITIALIZED;
  std::unique_lock<std::shared_mutex> w(rw_);
  if (!ts_order_.empty() || world == 0 || rank >= world || busy()) return FVDB_E_INVALID;
  std::vector<uint64_t> hid;
  std::vector<float> hv;
  int rc = bulk_route(ids, v, n, dim, ts, now, hid, hv);
  if (rc) return rc;
  shard_rank_ = rank;
  shard_world_ = world;
  if (ivf_trained_) {
    const uint32_t nlist = historical_->config().n_clusters;
    shard_sizes_.assign(nlist, 0);
    plan_list_owners(shard_sizes_, world, shard_owner_);  // (replaced below when rows go to the lists now)
  }
  if (!hid.empty()) {
    const uint32_t nlist = historical_->config().n_clusters;
    std::vector<uint32_t> cl(hid.size());
    rc = historical_->assign(hv.data(), hid.size(), dim, cl.data());
    if (rc) return rc;
    std::vector<uint64_t> sizes(nlist, 0);
    for (uint32_t c : cl) sizes[c]++;
    std::vector<uint32_t> owner;
    plan_list_owners(sizes, world, owner);
    shard_owner_ = owner;
    shard_sizes_ = sizes;
    if (owner_out) std::memcpy(owner_out, owner.data(), nlist * sizeof(uint32_t));
    const Rows mine = owned_rows(hid, hv, cl, dim, owner, rank);
    uint64_t ok = 0;
    int err = 0;
    rc = historical_->batch_insert_assigned(mine.ids.data(), mine.v.data(), mine.ids.size(), dim, mine.cl.data(), &ok, &err);
    if (rc) return rc;
    if (err) return err;
    rc = fvdb_ivf_set_global_list_sizes(historical_->device(), sizes.data());
    if (rc) return rc;
    historical_count_ = hid.size();  // logical count; this rank stores `ok` of them
  }
  return FVDB_OK;
}

void plan_list_owners_host(const uint64_t* sizes, uint32_t nlist, uint32_t world, uint32_t* owner) {
  std::vector<uint64_t> sz(sizes, sizes + nlist);
  std::vector<uint32_t> ow;
  plan_list_owners(sz, world ? world : 1, ow);
  std::memcpy(owner, ow.data(), (size_t)nlist * sizeof(uint32_t));
}

// src/hybrid/core.rs:857-877
int HybridIndex::from_parts(const uint64_t* ids, const double* ts, uint64_t n, uint64_t recent_count,
                            uint64_t historical_count, bool ivf_trained) {
  std::unique_lock<std::shared_mutex> w(rw_);
  if (!ts_order_.empty() || busy()) return FVDB_E_INVALID;
  if (ivf_trained && !historical_->is_trained()) return FVDB_E_NOT_TRAINED;
  for (uint64_t i = 0; i < n; ++i) {
    if (!timestamps_.emplace(ids[i], ts[i]).second) continue;  // a map on disk holds each key once; keep the first
    ts_order_.push_back(ids[i]);
    // ids with a node in the graph are what migrate_with_threshold can still copy into IVF (:626 get_node); one
    // already in a list fails there as a duplicate and leaves the queue, as on every search of the reference
    if (recent_->vector_of(ids[i])) {
      pending_migration_.push_back({ids[i], ts[i]});
      pending_min_ts_ = std::min(pending_min_ts_, ts[i]);
    }
  }
  recent_count_ = recent_count;
  historical_count_ = historical_count;
  ivf_trained_ = ivf_trained;
  initialized_ = true;
  return FVDB_OK;
}

// src/hybrid/core.rs:989-1012
int HybridIndex::vacuum(uint64_t* hnsw_removed, uint64_t* ivf_removed) {
  std::unique_lock<std::shared_mutex> w(rw_, std::defer_lock);
  if (int rc = write_lock(w)) return rc;
  if (int rc = recent_->vacuum(hnsw_removed)) return rc;
  return historical_->vacuum(ivf_removed);
}

int HybridIndex::retrain_historical(const IVFConfig& new_ivf_config, IVFIndex::RetrainResult* out) {
  std::unique_lock<std::shared_mutex> w(rw_, std::defer_lock);
  if (int rc = write_lock(w)) return rc;
  if (sharded_ || comm_ || shard_world_ > 0) return FVDB_E_UNSUPPORTED;  // the ranks would have to agree on the new lists
  if (!ivf_trained_) return FVDB_E_NOT_TRAINED;
  const int rc = historical_->retrain(new_ivf_config, out);
  ivf_trained_ = historical_->is_trained();
  if (historical_->config().n_clusters == new_ivf_config.n_clusters) cfg_.ivf = historical_->config();  // (row_dtype kept)
  return rc;
}

void HybridIndex::export_timestamps(uint64_t* ids, double* ts) const {
  for (size_t i = 0; i < ts_order_.size(); ++i) {
    ids[i] = ts_order_[i];
    ts[i] = timestamps_.at(ts_order_[i]);
  }
}

// src/hybrid/core.rs:600-649 — copies into IVF, never removes from HNSW (:577-581)
uint64_t HybridIndex::migrate_with_threshold(double threshold_s, double now) {
  std::unique_lock<std::shared_mutex> w(rw_, std::defer_lock);
  if (write_lock(w)) return 0;
  return migrate_locked(threshold_s, now);
}

// the caller holds rw_ exclusively and no batch is in flight
uint64_t HybridIndex::migrate_locked(double threshold_s, double now) {
  // The reference walks the whole timestamps map on every search (:606-617).  Same outcome, O(1) when
  // nothing is due: only ids still living in HNSW alone can migrate, and none is due while the oldest
  // of them is younger than the threshold.
  if (!migration_due(threshold_s, now)) return 0;
  std::vector<Pending> keep;
  std::vector<uint64_t> due;
  double min_ts = 1e300;
  for (const Pending& p : pending_migration_) {
    if (age_of(now, p.ts) >= threshold_s) {
      due.push_back(p.id);
    } else {
      keep.push_back(p);
      min_ts = std::min(min_ts, p.ts);
    }
  }
  if (due.empty()) return 0;
  uint64_t migrated = 0;
  const uint32_t dim = recent_->dimension();
  const bool sharded = shard_world_ > 0 && !shard_owner_.empty();
  // Resident form (non-sharded): the rows already sit in HBM in the graph's row store, so the due ids go down as store
  // row indices and nothing of the vectors crosses the host link.  A due id whose row the store does not hold (there is
  // none today) sends the whole job down the host path: one job, one path.
  if (resident_migration_ && !sharded && recent_->store()) {
    std::vector<uint64_t> ri;
    std::vector<uint32_t> rr;
    bool all = true;
    for (uint64_t id : due) {
      if (!recent_->vector_of(id)) continue;  // get_node(id) == None
      uint32_t row = 0;
      if (!recent_->store_row_of(id, &row)) {
        all = false;
        break;
      }
      ri.push_back(id);
      rr.push_back(row);
    }
    if (all) {
      if (!ri.empty()) {
        int err = 0;
        if (historical_->batch_insert_from_store(ri.data(), recent_->store(), rr.data(), ri.size(), &migrated, &err)) return 0;
        migration_path_ = MIGRATION_RESIDENT;
        fvdb_ivf_maintenance_info(historical_->device(), &migration_info_);
      }
      pending_migration_.swap(keep);
      pending_min_ts_ = min_ts;
      if (migrated) {
        recent_count_ = recent_count_ >= migrated ? recent_count_ - migrated : 0;
        historical_count_ += migrated;
      }
      return migrated;
    }
  }
  std::vector<float> xv;
  std::vector<uint64_t> xi;
  for (uint64_t id : due) {
    const float* vec = recent_->vector_of(id);
    if (!vec) continue;  // get_node(id) == None
    xi.push_back(id);
    xv.insert(xv.end(), vec, vec + dim);
  }
  if (!xi.empty() && shard_world_ > 0 && !shard_owner_.empty()) {
    // lists live on their owner ranks (bulk_insert_sharded): every rank runs this with the same due ids in the same
    // order and the same centroids — the owner of a row's list appends it, every rank counts it into the logical list
    // sizes, so list order and the selection keys' positions are what the unsharded index would have.  (An id that
    // is already in a list of ANOTHER rank cannot be seen here; ids that are still pending were never copied.)
    std::vector<uint32_t> cl(xi.size());
    if (historical_->assign(xv.data(), xi.size(), dim, cl.data())) return 0;
    for (uint32_t c : cl) shard_sizes_[c] += 1;
    const Rows mine = owned_rows(xi, xv, cl, dim, shard_owner_, shard_rank_);
    uint64_t ok = 0;
    int err = 0;
    if (!mine.ids.empty() &&
        historical_->batch_insert_assigned(mine.ids.data(), mine.v.data(), mine.ids.size(), dim, mine.cl.data(), &ok, &err))
      return 0;
    if (fvdb_ivf_set_global_list_sizes(historical_->device(), shard_sizes_.data())) return 0;
    migrated = xi.size();
  } else if (!xi.empty()) {
    int err = 0;
    int rc = historical_->batch_insert(xi.data(), xv.data(), xi.size(), dim, &migrated, &err);
    if (rc) return 0;  // IVF untrained / dimension mismatch: every insert fails; ids stay pending
    // what batch_insert copied: the rows up twice (assign, append), clusters down, ids and slots of the kept rows up
    migration_path_ = MIGRATION_HOST;
    migration_info_ = fvdb_maintenance_info_t{};
    migration_info_.rows_in = xi.size();
    migration_info_.rows_out = migrated;
    migration_info_.host_bytes = (uint64_t)xi.size() * (dim * 4ull + 4) + migrated * (dim * 4ull + 12);
  }
  // A copy that failed as a duplicate fails the same way on every later search (the reference
  // retries it each time with no effect), so due ids leave the queue either way.
  pending_migration_.swap(keep);
  pending_min_ts_ = min_ts;
  if (migrated) {
    recent_count_ = recent_count_ >= migrated ? recent_count_ - migrated : 0;
    historical_count_ += migrated;
  }
  return migrated;
}

// bindings/node/src/session.rs:272-279: the recent index answers first, the historical one for the rest
int HybridIndex::get_vectors(const uint64_t* ids, uint64_t n, float* out, uint8_t* found) {
  if (n == 0) return FVDB_OK;
  if (!ids || !out || !found) return FVDB_E_INVALID;
  std::shared_lock<std::shared_mutex> r(rw_);
  recent_->get_vectors(ids, n, out, found);
  std::vector<uint64_t> rest, at;
  for (uint64_t i = 0; i < n; ++i)
    if (!found[i]) {
      rest.push_back(ids[i]);
      at.push_back(i);
    }
  if (rest.empty()) return FVDB_OK;
  const uint32_t dim = historical_->dimension();
  std::vector<float> rows(rest.size() * (size_t)dim);
  std::vector<uint8_t> f(rest.size(), 0);
  if (int rc = historical_->get_vectors(rest.data(), rest.size(), rows.data(), f.data())) return rc;
  for (size_t j = 0; j < rest.size(); ++j)
    if (f[j]) {
      found[at[j]] = 1;
      std::memcpy(out + at[j] * dim, &rows[j * dim], (size_t)dim * sizeof(float));
    }
  return FVDB_OK;
}

// src/hybrid/core.rs:425-486 for a batch of queries
int HybridIndex::search(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now,
                        uint64_t* ids, float* dist, uint32_t* counts) {
  return search_impl(q, false, B, dim, cfg, now, ids, dist, counts);
}
int HybridIndex::search_dev(const float* q_dev, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now,
                            uint64_t* ids, float* dist, uint32_t* counts) {
  return search_impl(q_dev, true, B, dim, cfg, now, ids, dist, counts);
}

// stable merge of the two parts (:476-485): concatenate recent then historical, stable sort by distance, take k
static void merge_parts(uint32_t B, uint32_t k, uint32_t rk, uint32_t hk, bool have_r, const uint64_t* rid, const float* rd,
                        const uint32_t* rc, bool have_h, const uint64_t* hid, const float* hd, const uint32_t* hc,
                        uint64_t* ids, float* dist, uint32_t* counts) {
  struct R {
    uint64_t id;
    float d;
  };
  std::vector<R> all;
  for (uint32_t b = 0; b < B; ++b) {
    all.clear();
    if (have_r)
      for (uint32_t i = 0; i < rc[b]; ++i) all.push_back({rid[(size_t)b * rk + i], rd[(size_t)b * rk + i]});
    if (have_h)
      for (uint32_t i = 0; i < hc[b]; ++i) all.push_back({hid[(size_t)b * hk + i], hd[(size_t)b * hk + i]});
    std::stable_sort(all.begin(), all.end(), [](const R& a, const R& c) { return a.d < c.d; });  // :482
    if (all.size() > k) all.resize(k);
    for (size_t i = 0; i < all.size(); ++i) {
      ids[(size_t)b * k + i] = all[i].id;
      dist[(size_t)b * k + i] = all[i].d;
    }
    counts[b] = (uint32_t)all.size();
  }
}

void merge_parts_host(uint32_t B, uint32_t k, uint32_t rk, uint32_t hk, const uint64_t* rid, const float* rd,
                      const uint32_t* rc, const uint64_t* hid, const float* hd, const uint32_t* hc, uint64_t* ids,
                      float* dist, uint32_t* counts) {
  fill_empty(ids, dist, counts, B, k);
  merge_parts(B, k, rk, hk, rid != nullptr, rid, rd, rc, hid != nullptr, hid, hd, hc, ids, dist, counts);
}

int HybridIndex::migrate_if_due(double now, bool in_flight_before) {
  if (!cfg_.auto_migrate) return FVDB_OK;
  {
    std::shared_lock<std::shared_mutex> r(rw_);
    if (!migration_due(cfg_.recent_threshold_s, now)) return FVDB_OK;
  }
  std::unique_lock<std::shared_mutex> w(rw_);  // the reference takes its write locks here too (:621-622)
  if (!migration_due(cfg_.recent_threshold_s, now)) return FVDB_OK;
  if (in_flight_before || busy()) return FVDB_E_INVALID;  // the caller collects its batches and searches again
  migrate_locked(cfg_.recent_threshold_s, now);
  return FVDB_OK;
}

// Explicit pair for ONE thread that keeps several batches in flight (bench, pipelined servers).
int HybridIndex::search_dev_begin(uint32_t slot, const float* q_dev, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg,
                                  double now) {
  if (slot >= kSlots) return FVDB_E_INVALID;
  return begin_explicit(slot, q_dev, B, dim, cfg, -1, now);
}

int HybridIndex::begin_explicit(uint32_t slot, const float* q_dev, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg,
                                int shard_mode, double now, const uint64_t* allowed, uint64_t n_allowed, bool masked) {
  bool others = false;
  {
    std::lock_guard<std::mutex> lk(slot_mu_);
    if (slots_[slot].active) return FVDB_E_INVALID;  // the previous batch of this slot was never collected
    others = busy_unlocked();
  }
  // the migration check comes before this batch counts as in flight.  Sharded: `now` is the same on every rank, so every
  // rank migrates the same rows at the same step — also a rank that has no query of its own in it
  if (initialized_ && cfg.k != 0 && (B != 0 || shard_mode >= 0))
    if (int rc = migrate_if_due(now, others)) return rc;
  std::shared_lock<std::shared_mutex> r(rw_);  // no mutation is under way while the batch is enqueued
  Lease lease(this, slot, Lease::kTake);
  if (!lease.sl) return FVDB_E_INVALID;
  lease.hand_over();  // whatever begin_impl returns, the slot stays the caller's until search_dev_end
  slots_[slot].ivf_mask.reset();  // the explicit pair is an unfiltered search, unless it names an allow-set
  slots_[slot].view.reset();
  if (masked && initialized_ && cfg.k != 0)  // search_dev_end drops them
    if (int rc = build_masks(cfg, allowed, n_allowed, &slots_[slot].view, &slots_[slot].ivf_mask)) return rc;
  return begin_impl(slot, q_dev, B, dim, cfg, shard_mode, shard_mode < 0 && !masked);
}

// The masks of a filtered search, one per part that is searched.  Every caller builds them after the migration step and
// under the read lock that keeps the rows where they are until the search has its results.
int HybridIndex::build_masks(const HybridSearchConfig& cfg, const uint64_t* allowed, uint64_t n_allowed, HNSWIndex::ViewRef* view,
                             MaskRef* ivf_mask) {
  if (cfg.search_recent)
    if (int rc = recent_->allowed_view(allowed, n_allowed, view)) return rc;
  if (cfg.search_historical && ivf_trained_)
    if (int rc = historical_->allowed_mask(allowed, n_allowed, ivf_mask)) return rc;
  return FVDB_OK;
}

// NaN / Inf in a query: the reference panics in partial_cmp().unwrap()
static int check_finite(const float* q, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (!(q[i] - q[i] == 0.0f)) return FVDB_E_NONFINITE;
  return FVDB_OK;
}
// host queries, checked, into the slot's staging block; both parts read them from there
int HybridIndex::stage_finite(Slot& sl, const float* q, uint32_t B, uint32_t dim) {
  const uint64_t bytes = (uint64_t)B * dim * 4;
  if (int rc = check_finite(q, (uint64_t)B * dim)) return rc;
  if (int rc = sl.d_q.reserve(ctx_ivf_, bytes, false)) return rc;
  if (slot_ctx(ctx_ivf_, &sl == slots_, &sl.ivf_ctx)) return FVDB_E_HIP;
  return fvdb_dev_upload(sl.ivf_ctx, sl.d_q.dev, q, bytes);  // waits on the slot's own stream only
}

int HybridIndex::attach_comm(fvdb_comm* comm) {
  // fp16 rows: the sharded step and the replicated graph have not been taken through half-width rows yet
  if (comm && cfg_.row_dtype() == FVDB_F16) return FVDB_E_UNSUPPORTED;
  std::unique_lock<std::shared_mutex> w(rw_);
  flush_waiting();  // no chain is left to be enqueued under another communicator
  if (busy()) return FVDB_E_INVALID;
  if (sharded_) fvdb_sharded_destroy(sharded_);
  sharded_ = nullptr;
  comm_ = comm;
  if (!comm) return FVDB_OK;
  if (!ivf_trained_ || !historical_->device()) return FVDB_E_NOT_TRAINED;
  return fvdb_sharded_create(historical_->device(), comm, &sharded_);
}

HybridIndex::Slice HybridIndex::strong_slice(uint32_t B) const {
  const uint32_t W = (uint32_t)fvdb_comm_world(comm_), r = (uint32_t)fvdb_comm_rank(comm_);
  const uint32_t per = (B + W - 1) / W;
  return {per, std::min(B, r * per), std::min(B, (r + 1) * per)};
}

uint32_t HybridIndex::sharded_rows(uint32_t B, int mode) const {
  if (!comm_ || mode != FVDB_SHARD_STRONG) return B;
  const Slice s = strong_slice(B);
  return s.hi - s.lo;
}

int HybridIndex::search_sharded_begin(uint32_t slot, const float* q_dev, uint32_t B, uint32_t dim,
                                      const HybridSearchConfig& cfg, int mode, double now) {
  if (slot >= kSlots || !sharded_ || (mode != FVDB_SHARD_WEAK && mode != FVDB_SHARD_STRONG)) return FVDB_E_INVALID;
  return begin_explicit(slot, q_dev, B, dim, cfg, mode, now);
}

int HybridIndex::search_allowed_sharded_begin(uint32_t slot, const float* q_dev, uint32_t B, uint32_t dim,
                                              const HybridSearchConfig& cfg, int mode, const uint64_t* allowed,
                                              uint64_t n_allowed, double now) {
  if (slot >= kSlots || !sharded_ || (mode != FVDB_SHARD_WEAK && mode != FVDB_SHARD_STRONG)) return FVDB_E_INVALID;
  if (n_allowed && !allowed) return FVDB_E_INVALID;
  return begin_explicit(slot, q_dev, B, dim, cfg, mode, now, allowed, n_allowed, true);
}

// one block per slot for the IVF part's results, [ids R*hk u64 | dist R*hk f32 | counts R u32] -> a single copy
// (R = rows the IVF part writes: B, or the padded slice length in strong sharded mode)
namespace {
struct IvfBlock {
  uint64_t* ids = nullptr;
  float* dist = nullptr;
  uint32_t* counts = nullptr;
  static uint64_t bytes(uint32_t rows, uint32_t hk) { return (uint64_t)rows * hk * 12 + (uint64_t)rows * 4; }
  IvfBlock() = default;
  IvfBlock(void* base, uint32_t rows, uint32_t hk) {
    const uint64_t need = (uint64_t)rows * hk;
    ids = (uint64_t*)base;
    dist = (float*)((char*)base + need * 8);
    counts = (uint32_t*)((char*)base + need * 12);
  }
};
}  // namespace

static bool ivf_one_stream() {
  static const bool on = getenv("FVDB_IVF_ONE_STREAM") != nullptr;  // tuning aid
  return on;
}

bool HybridIndex::pairing_enabled() {
  static const bool on = [] {
    const char* v = getenv("FVDB_HYBRID_PAIR");  // A/B switch, read once
    return !(v && std::strcmp(v, "0") == 0);
  }();
  return on;
}

// The IVF chain of one batch on the slot's own stream with its own scratch set, the result copy right behind it, then
// the event.
int HybridIndex::enqueue_ivf(uint32_t slot, const float* q_dev, uint32_t B_in, uint32_t ivf_rows, uint32_t dim, uint64_t n_probe,
                             int shard_mode) {
  Slot& sl = slots_[slot];
  const uint64_t bytes = IvfBlock::bytes(ivf_rows, sl.hk);
  if (int rc = sl.ivf.reserve(ctx_ivf_, bytes, true)) return rc;
  sl.ivf_rows = ivf_rows;
  const IvfBlock d(sl.ivf.dev, ivf_rows, sl.hk);
  // each slot's IVF chain runs on its own stream with its own scratch set, so the chains of consecutive batches
  // overlap (a chain is ~20 dependent launches with gaps between them)
  if (slot_ctx(ctx_ivf_, slot == 0 || ivf_one_stream(), &sl.ivf_ctx)) return FVDB_E_HIP;
  fvdb_ctx* on = sl.ivf_ctx == ctx_ivf_ ? nullptr : sl.ivf_ctx;
  if (!sl.ivf_done && fvdb_event_create(sl.ivf_ctx, &sl.ivf_done)) return FVDB_E_HIP;
  if (shard_mode >= 0) {
    // every rank must take part in the step's collectives even when its own slice is empty
    if (dim != historical_->dimension()) return FVDB_E_DIM;
    // k or nprobe beyond the register path, or an allow-set: the wide sharded step; otherwise the call as ever
    const bool beyond = sl.hk > FVDB_MAX_K || n_probe > FVDB_MAX_K || sl.ivf_mask;
    const int rcs = beyond ? fvdb_ivf_search_sharded_wide_begin(sharded_, on, on ? slot : 0, sl.ivf_mask.get(), q_dev, B_in,
                                                                sl.hk, (uint32_t)std::min<uint64_t>(n_probe, 0xFFFFFFFFu),
                                                                shard_mode, d.ids, d.dist, d.counts)
                           : fvdb_ivf_search_sharded_begin(sharded_, on, on ? slot : 0, q_dev, B_in, sl.hk, (uint32_t)n_probe,
                                                           shard_mode, d.ids, d.dist, d.counts);
    if (rcs) return rcs;
  } else {
    // a historical part the engine refuses (historical_k above FVDB_MAX_K_WIDE, say) fails the search: the result
    // must never quietly be the recent rows alone
    const int rch = sl.ivf_mask ? historical_->search_dev_masked(sl.ivf_mask, q_dev, B_in, dim, sl.hk, (uint32_t)n_probe, d.ids,
                                                                 d.dist, d.counts, on, on ? slot : 0)
                                : historical_->search_dev(q_dev, B_in, dim, sl.hk, (uint32_t)n_probe, d.ids, d.dist, d.counts, on,
                                                          on ? slot : 0);
    if (rch) return rch;
  }
  sl.ivf_in_flight = true;
  // result copy rides the slot's stream right behind the chain, then the event
  if (fvdb_dev_download_async(sl.ivf_ctx, sl.ivf.host, sl.ivf.dev, (size_t)bytes) || fvdb_event_record(sl.ivf_ctx, sl.ivf_done))
    return FVDB_E_HIP;
  return FVDB_OK;
}

// One chain for the waiting batch `first` and the batch of slot `launcher`, on the launcher's stream with its scratch
// set, into the Pair's own blocks.  pair_mu_ held.
int HybridIndex::enqueue_ivf_pair(Slot& first, uint32_t launcher, Pair& p) {
  Slot& sl = slots_[launcher];
  const uint32_t rows = first.B + sl.B, dim = sl.dim;
  const uint64_t bytes = IvfBlock::bytes(rows, sl.hk);
  if (int rc = p.q.reserve(ctx_ivf_, (uint64_t)rows * dim * 4, false)) return rc;
  if (int rc = p.res.reserve(ctx_ivf_, bytes, true)) return rc;
  if (slot_ctx(ctx_ivf_, launcher == 0 || ivf_one_stream(), &sl.ivf_ctx)) return FVDB_E_HIP;
  fvdb_ctx* on = sl.ivf_ctx == ctx_ivf_ ? nullptr : sl.ivf_ctx;
  if (!p.done && fvdb_event_create(sl.ivf_ctx, &p.done)) return FVDB_E_HIP;
  float* q = (float*)p.q.dev;
  if (fvdb_dev_copy_async(sl.ivf_ctx, q, first.q, (size_t)first.B * dim * 4) ||
      fvdb_dev_copy_async(sl.ivf_ctx, q + (size_t)first.B * dim, sl.q, (size_t)sl.B * dim * 4))
    return FVDB_E_HIP;
  const IvfBlock d(p.res.dev, rows, sl.hk);
  if (int rc = historical_->search_dev(q, rows, dim, sl.hk, sl.n_probe, d.ids, d.dist, d.counts, on, on ? launcher : 0)) return rc;
  if (fvdb_dev_download_async(sl.ivf_ctx, p.res.host, p.res.dev, (size_t)bytes) || fvdb_event_record(sl.ivf_ctx, p.done))
    return FVDB_E_HIP;
  p.ctx = sl.ivf_ctx;
  p.rows = rows;
  p.hk = sl.hk;
  p.refs = 2;
  first.pair = sl.pair = &p;
  first.pair_off = 0;
  sl.pair_off = first.B;
  first.ivf_in_flight = sl.ivf_in_flight = true;
  return FVDB_OK;
}

// pair_mu_ held: the waiting batch goes alone, on its own slot's stream; what that returns is its search_dev_end's
void HybridIndex::flush_waiting_locked() {
  if (waiting_ < 0) return;
  Slot& w = slots_[waiting_];
  w.ivf_waiting = false;
  w.ivf_rc = enqueue_ivf((uint32_t)waiting_, w.q, w.B, w.B, w.dim, w.n_probe, -1);
  waiting_ = -1;
}

// The IVF part of an explicit begin that may share its chain: with the waiting batch if there is a compatible one (same
// dim, historical k and n_probe; the index cannot have changed, both slots being in flight), else this batch waits.
int HybridIndex::begin_ivf_paired(uint32_t slot) {
  Slot& sl = slots_[slot];
  std::lock_guard<std::mutex> lk(pair_mu_);
  if (waiting_ >= 0) {
    Slot& w = slots_[waiting_];
    Pair* p = nullptr;
    if (w.dim == sl.dim && w.hk == sl.hk && w.n_probe == sl.n_probe && (uint64_t)w.B + sl.B <= kPairRowsMax)
      for (Pair& c : pairs_)
        if (c.refs == 0) {
          p = &c;
          break;
        }
    if (p) {
      w.ivf_waiting = false;
      waiting_ = -1;
      const int rc = enqueue_ivf_pair(w, slot, *p);
      if (rc) w.ivf_rc = rc;  // nothing of a joint chain that failed is collected, and each batch reports the status
      return rc;
    }
    flush_waiting_locked();
  }
  sl.ivf_waiting = true;
  waiting_ = (int)slot;
  return FVDB_OK;
}

void HybridIndex::release_pair(Slot& sl) {
  std::lock_guard<std::mutex> lk(pair_mu_);
  if (!sl.pair) return;
  sl.pair->refs -= 1;
  sl.pair = nullptr;
}

// enqueue everything for the batch; the slot is already marked active by the caller
int HybridIndex::begin_impl(uint32_t slot, const float* q_dev, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg,
                            int shard_mode, bool may_pair) {
  Slot& sl = slots_[slot];
  sl.ivf_in_flight = sl.hnsw_in_flight = false;
  sl.ivf_rc = FVDB_OK;
  // sharded: `q_own` / `Bown` are the queries whose final results this rank produces (the graph is replicated, so each
  // rank walks it for those only); the IVF part is handed the batch as the mode defines it
  const float* q_own = q_dev;
  uint32_t Bown = B, ivf_rows = B;
  if (shard_mode == FVDB_SHARD_STRONG) {
    const Slice s = strong_slice(B);
    q_own = q_dev + (size_t)s.lo * dim;
    Bown = s.hi - s.lo;
    ivf_rows = s.per;
  }
  const uint32_t B_ivf_in = B;
  B = Bown;
  sl.q = q_own;
  sl.B = B;
  sl.dim = dim;
  sl.k = (uint32_t)cfg.k;
  sl.rk = cfg.rk();
  sl.hk = cfg.hk();
  sl.ef = (uint32_t)cfg.hnsw_ef;
  sl.recent = cfg.search_recent;
  if (!initialized_ || sl.k == 0 || (B == 0 && shard_mode < 0)) return FVDB_OK;
  if (cfg.search_recent && B > 0) {
    // the graph walk is latency-bound (one wave per query): enqueue it FIRST so that the list scan launched
    // next fills the rest of every SIMD and the two run concurrently
    int rcb = 0;
    sl.hnsw_in_flight = recent_->search_dev_begin(q_own, B, dim, sl.rk, sl.ef, &rcb, slot, sl.view.get());
  }
  if (cfg.search_historical && ivf_trained_) {
    sl.n_probe = (uint32_t)cfg.ivf_n_probe;
    // The explicit pair on an unsharded index without an allow-set, inside the register path's k and n_probe (the route
    // every batch size takes alike): the chain may be shared with the next batch begun.  A dimension the engine would
    // refuse is refused now, as ever; what is left to fail later is the enqueue itself.
    const bool pairable = may_pair && pairing_enabled() && shard_mode < 0 && !sharded_ && !sl.ivf_mask && B > 0 &&
                          sl.hk <= FVDB_MAX_K && cfg.ivf_n_probe > 0 &&
                          std::min<uint64_t>(cfg.ivf_n_probe, historical_->config().n_clusters) <= FVDB_MAX_K;
    if (pairable) {
      if (dim != historical_->dimension()) return FVDB_E_DIM;
      return begin_ivf_paired(slot);
    }
    std::unique_lock<std::mutex> lk(pair_mu_, std::defer_lock);
    if (may_pair) {  // an explicit begin that cannot share: the chains still start in the order their batches were begun
      lk.lock();
      flush_waiting_locked();
    }
    return enqueue_ivf(slot, q_dev, B_ivf_in, ivf_rows, dim, cfg.ivf_n_probe, shard_mode);
  }
  return FVDB_OK;
}

int HybridIndex::search_dev_end(uint32_t slot, uint64_t* ids, float* dist, uint32_t* counts) {
  if (slot >= kSlots) return FVDB_E_INVALID;
  Lease lease(this, slot, Lease::kAdopt);  // released at return: the slot is free again only when its buffers have been read
  if (!lease.sl) return FVDB_E_INVALID;
  Slot& sl = *lease.sl;
  const uint32_t B = sl.B, k = sl.k;
  // a filtered search's masks stay referenced until its results are in, whichever way this returns
  DropMasks drop_masks{&sl};
  fill_empty(ids, dist, counts, B, k);
  if (!initialized_ || B == 0 || k == 0) return FVDB_OK;
  {
    // still waiting for a partner: its chain goes alone now, on its own slot's stream
    std::lock_guard<std::mutex> lk(pair_mu_);
    if (sl.ivf_waiting) flush_waiting_locked();
  }
  // the joint chain's blocks are the Pair's: given up when this batch has read its rows, whichever way this returns
  struct DropPair {
    HybridIndex* h;
    Slot* sl;
    ~DropPair() { h->release_pair(*sl); }
  } drop_pair{this, &sl};
  std::vector<uint64_t> rid;
  std::vector<float> rd;
  std::vector<uint32_t> rc_(B, 0);
  bool have_r = false, have_h = false;
  if (sl.recent) {
    rid.resize((size_t)B * sl.rk);
    rd.resize((size_t)B * sl.rk);
    // the graph's slot remembers whether the begin enqueued anything; if not, this is the blocking search
    have_r = recent_->search_dev_end(sl.q, B, sl.dim, sl.rk, sl.ef, rid.data(), rd.data(), rc_.data(), slot, sl.view.get()) == FVDB_OK;
  }
  IvfBlock h;
  if (sl.ivf_in_flight) {
    if (const Pair* p = sl.pair) {  // this batch's rows of the joint block
      have_h = fvdb_event_wait(p->ctx, p->done) == FVDB_OK;
      const IvfBlock all(p->res.host, p->rows, p->hk);
      h.ids = all.ids + (size_t)sl.pair_off * p->hk;
      h.dist = all.dist + (size_t)sl.pair_off * p->hk;
      h.counts = all.counts + sl.pair_off;
    } else {
      have_h = fvdb_event_wait(sl.ivf_ctx, sl.ivf_done) == FVDB_OK;
      h = IvfBlock(sl.ivf.host, sl.ivf_rows, sl.hk);
    }
    bool others = false;
    {
      std::lock_guard<std::mutex> lk(slot_mu_);
      for (const Slot& o : slots_) others = others || (o.active && &o != &sl);
    }
    if (!others) fvdb_ivf_profile_collect(historical_->device());  // stage timing only makes sense one batch at a time
  }
  merge_parts(B, k, sl.rk, sl.hk, have_r, rid.data(), rd.data(), rc_.data(), have_h, h.ids, h.dist, h.counts, ids, dist,
              counts);
  const int late = sl.ivf_rc;  // of a chain enqueued after this batch's begin had returned; FVDB_OK otherwise
  sl.ivf_rc = FVDB_OK;
  return late;
}

// The blocking entry points: any number of host threads.  A call holds the read side of rw_ from after its migration
// check to its merge and works in a slot leased for its duration.
int HybridIndex::search_impl(const float* q, bool q_on_device, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg,
                             double now, uint64_t* ids, float* dist, uint32_t* counts, const uint64_t* allowed,
                             uint64_t n_allowed, bool masked) {
  const uint32_t k = (uint32_t)cfg.k;
  fill_empty(ids, dist, counts, B, k);
  if (!initialized_ || B == 0 || k == 0) return FVDB_OK;
  if (int rc = migrate_if_due(now, false)) return rc;
  std::shared_lock<std::shared_mutex> r(rw_);
  return search_locked(q, q_on_device, B, dim, cfg, ids, dist, counts, allowed, n_allowed, masked);
}

int HybridIndex::search_locked(const float* q, bool q_on_device, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg,
                               uint64_t* ids, float* dist, uint32_t* counts, const uint64_t* allowed, uint64_t n_allowed,
                               bool masked) {
  const uint32_t k = (uint32_t)cfg.k;
  // filtered search: the masks are built here — after the migration, under the lock that keeps the rows where they
  // are until this search has its results
  MaskRef ivf_mask;
  HNSWIndex::ViewRef view;
  if (masked)
    if (int rc = build_masks(cfg, allowed, n_allowed, &view, &ivf_mask)) return rc;
  Lease lease(this, Lease::kAnyFree, Lease::kTake);  // given back at every return, until search_dev_end takes it over
  Slot& sl = *lease.sl;
  const uint32_t slot = lease.index();
  sl.ivf_mask = ivf_mask;
  sl.view = view;
  // the slot keeps them only while this search runs: search_dev_end drops them when it collects the batch, and every
  // return before the slot is handed to it drops them here — the next user of the slot must find none
  DropMasks drop_masks{&sl};
  const float* qd = q;
  if (!q_on_device) {  // stage the batch in HBM once; both parts read it from there
    if (int rc = stage_finite(sl, q, B, dim)) return rc;
    qd = (const float*)sl.d_q.dev;
  }
  flush_waiting();  // a chain that waits for a partner starts before this search's, as it would have without pairing
  const int rc0 = begin_impl(slot, qd, B, dim, cfg);
  if (rc0 && !sl.hnsw_in_flight && !sl.ivf_in_flight) return rc0;
  lease.hand_over();
  drop_masks.sl = nullptr;  // search_dev_end's turn
  if (rc0) {  // drain what was enqueued before the failure
    std::vector<uint64_t> ti((size_t)B * k);
    std::vector<float> td((size_t)B * k);
    std::vector<uint32_t> tc(B);
    (void)search_dev_end(slot, ti.data(), td.data(), tc.data());
    return rc0;
  }
  return search_dev_end(slot, ids, dist, counts);
}

// ---- exact search and search quality ----
// The two exact parts and the usual merge; the caller holds the read side of rw_.  The graph's scan runs in a slot leased
// for the call (its stream, its scratch, its result block), the every-list search in a scratch set the engine leases.
int HybridIndex::exact_locked(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, uint64_t* ids, float* dist,
                              uint32_t* counts, bool wide) {
  const uint32_t k = (uint32_t)cfg.k;
  const uint32_t rk = cfg.rk(), hk = cfg.hk();
  if (int rc = check_finite(q, (uint64_t)B * dim)) return rc;  // whichever parts are searched, and before any other refusal
  std::vector<uint64_t> rid, hid;
  std::vector<float> rd, hd;
  std::vector<uint32_t> rc_(B, 0), hc(B, 0);
  const bool have_r = cfg.search_recent, have_h = cfg.search_historical && ivf_trained_;
  if (have_r) {
    if (rk > (wide ? FVDB_MAX_K_WIDE : FVDB_MAX_K)) return FVDB_E_UNSUPPORTED;
    rid.resize((size_t)B * rk);
    rd.resize((size_t)B * rk);
    Lease lease(this, Lease::kAnyFree, Lease::kTake);
    Slot& sl = *lease.sl;
    int rc;
    if ((rc = stage_finite(sl, q, B, dim))) return rc;
    const float* qd = (const float*)sl.d_q.dev;
    if ((rc = wide ? recent_->search_exact_wide_dev(qd, B, dim, rk, nullptr, rid.data(), rd.data(), rc_.data(), lease.index())
                   : recent_->search_exact_dev(qd, B, dim, rk, nullptr, rid.data(), rd.data(), rc_.data(), lease.index())))
      return rc;
  }
  if (have_h) {
    if (wide && hk > FVDB_MAX_K_WIDE) return FVDB_E_UNSUPPORTED;
    hid.resize((size_t)B * hk);
    hd.resize((size_t)B * hk);
    // search_with_config(q, k, n_clusters): every list, in centroid-rank order (the any-nprobe route where it applies)
    if (int rc = historical_->search(q, B, dim, hk, historical_->config().n_clusters, hid.data(), hd.data(), hc.data())) return rc;
  }
  merge_parts(B, k, rk, hk, have_r, rid.data(), rd.data(), rc_.data(), have_h, hid.data(), hd.data(), hc.data(), ids, dist, counts);
  return FVDB_OK;
}

int HybridIndex::search_exact(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now, uint64_t* ids,
                              float* dist, uint32_t* counts) {
  return exact_impl(q, B, dim, cfg, now, ids, dist, counts, false);
}

// the same search with the recent part from the graph's wide exact scan
int HybridIndex::search_exact_wide(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now, uint64_t* ids,
                                   float* dist, uint32_t* counts) {
  return exact_impl(q, B, dim, cfg, now, ids, dist, counts, true);
}

int HybridIndex::exact_impl(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now, uint64_t* ids,
                            float* dist, uint32_t* counts, bool wide) {
  if (sharded_ || shard_world_) return FVDB_E_UNSUPPORTED;  // a rank holds only the lists it owns
  const uint32_t k = (uint32_t)cfg.k;
  if (cfg.k == 0 || cfg.k > (wide ? FVDB_MAX_K_WIDE : FVDB_MAX_K)) return FVDB_E_UNSUPPORTED;
  fill_empty(ids, dist, counts, B, k);
  if (!initialized_ || B == 0) return FVDB_OK;
  if (int rc = migrate_if_due(now, false)) return rc;
  std::shared_lock<std::shared_mutex> r(rw_);
  return exact_locked(q, B, dim, cfg, ids, dist, counts, wide);
}

// ---- radius search: two radius parts, the usual merge, the sum of the two totals ----
int HybridIndex::search_radius(const float* q, uint32_t B, uint32_t dim, const float* radius, const HybridSearchConfig& cfg, double now,
                               const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts,
                               uint32_t* totals) {
  if (sharded_ || shard_world_) return FVDB_E_UNSUPPORTED;  // a rank holds only the lists it owns
  const uint32_t k = (uint32_t)cfg.k;
  if (cfg.k == 0 || cfg.k > FVDB_MAX_K_WIDE) return FVDB_E_UNSUPPORTED;
  if (int rc = check_radius(radius, B)) return rc;
  fill_empty(ids, dist, counts, B, k);
  std::fill(totals, totals + B, 0u);
  if (!initialized_ || B == 0) return FVDB_OK;
  if (int rc = migrate_if_due(now, false)) return rc;
  std::shared_lock<std::shared_mutex> r(rw_);
  if (int rc = check_finite(q, (uint64_t)B * dim)) return rc;
  std::vector<uint64_t> rid, hid;
  std::vector<float> rd, hd;
  std::vector<uint32_t> rc_(B, 0), hc(B, 0), rt(B, 0), ht(B, 0);
  const bool have_r = cfg.search_recent, have_h = cfg.search_historical && ivf_trained_;
  if (have_r) {
    rid.resize((size_t)B * k);
    rd.resize((size_t)B * k);
    HNSWIndex::ViewRef view;
    int rc;
    if (allowed && (rc = recent_->allowed_view(allowed, n_allowed, &view))) return rc;
    Lease lease(this, Lease::kAnyFree, Lease::kTake);
    Slot& sl = *lease.sl;
    if ((rc = stage_finite(sl, q, B, dim))) return rc;
    if ((rc = recent_->search_radius_dev((const float*)sl.d_q.dev, B, dim, radius, k, allowed ? view.get() : nullptr, rid.data(),
                                         rd.data(), rc_.data(), rt.data(), lease.index())))
      return rc;
  }
  if (have_h) {
    hid.resize((size_t)B * k);
    hd.resize((size_t)B * k);
    if (int rc = historical_->search_radius(q, B, dim, radius, k, (uint32_t)std::min<uint64_t>(cfg.ivf_n_probe, 0xFFFFFFFFu), allowed,
                                            n_allowed, hid.data(), hd.data(), hc.data(), ht.data()))
      return rc;
  }
  merge_parts(B, k, k, k, have_r, rid.data(), rd.data(), rc_.data(), have_h, hid.data(), hd.data(), hc.data(), ids, dist, counts);
  for (uint32_t b = 0; b < B; ++b) totals[b] = rt[b] + ht[b];
  return FVDB_OK;
}

int HybridIndex::evaluate_search_quality(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now,
                                         SearchQuality* out) {
  return quality_impl(q, B, dim, cfg, now, out, false);
}

int HybridIndex::evaluate_search_quality_wide(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now,
                                              SearchQuality* out) {
  return quality_impl(q, B, dim, cfg, now, out, true);
}

int HybridIndex::quality_impl(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, double now, SearchQuality* out,
                              bool wide) {
  if (sharded_ || shard_world_) return FVDB_E_UNSUPPORTED;
  if (B == 0 || !q || !out) return FVDB_E_INVALID;  // "No test queries provided" (src/ivf/operations.rs:334-338)
  if (cfg.k == 0 || cfg.k > (wide ? FVDB_MAX_K_WIDE : FVDB_MAX_K)) return FVDB_E_UNSUPPORTED;
  if (!initialized_) return FVDB_E_INVALID;
  const uint32_t k = (uint32_t)cfg.k;
  const auto start = std::chrono::steady_clock::now();
  const size_t n = (size_t)B * k;
  std::vector<uint64_t> rid(n), tid(n);
  std::vector<float> rd(n), td(n);
  std::vector<uint32_t> rcn(B), tcn(B);
  if (int rc = migrate_if_due(now, false)) return rc;
  float tr = 0.0f, tp = 0.0f;
  {
    std::shared_lock<std::shared_mutex> r(rw_);  // one hold for both searches: they see the same rows
    fill_empty(rid.data(), rd.data(), rcn.data(), B, k);
    fill_empty(tid.data(), td.data(), tcn.data(), B, k);
    int rc;
    if ((rc = search_locked(q, false, B, dim, cfg, rid.data(), rd.data(), rcn.data(), nullptr, 0, false))) return rc;
    if ((rc = exact_locked(q, B, dim, cfg, tid.data(), td.data(), tcn.data(), wide))) return rc;
    std::lock_guard<std::mutex> lk(qual_mu_);
    if ((rc = compare_id_blocks(ctx_ivf_, qual_, B, k, rid.data(), rcn.data(), tid.data(), tcn.data(), &tr, &tp))) return rc;
  }
  *out = quality_of(tr, tp, B, start);
  return FVDB_OK;
}

// quality_impl at every pair (efs[i], n_probes[j]).  The parts are the blocking searches of the
// two index classes — what search_locked's begin / end pair returns for them — kept apart; the merge of every pair
// happens on the device, inside the count.
int HybridIndex::quality_grid(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, const uint32_t* efs, uint32_t E,
                              const uint32_t* n_probes, uint32_t P, double now, QualityGrid* out) {
  if (sharded_ || shard_world_) return FVDB_E_UNSUPPORTED;
  if (B == 0 || !q || !out) return FVDB_E_INVALID;  // "No test queries provided" (src/ivf/operations.rs:334-338)
  if (cfg.search_recent && (E == 0 || !efs)) return FVDB_E_INVALID;
  if (cfg.search_historical && (P == 0 || !n_probes)) return FVDB_E_INVALID;
  if (cfg.k == 0 || cfg.k > FVDB_MAX_K_WIDE || E > 64 || P > 64) return FVDB_E_UNSUPPORTED;
  if (!initialized_) return FVDB_E_INVALID;
  if (cfg.search_recent && recent_->dimension() != 0 && dim != recent_->dimension()) return FVDB_E_DIM;
  if (cfg.search_historical && ivf_trained_ && dim != historical_->dimension()) return FVDB_E_DIM;
  const uint32_t k = (uint32_t)cfg.k, rk = cfg.rk(), hk = cfg.hk();
  const bool wide = k > FVDB_MAX_K;  // the two exact forms agree for k <= FVDB_MAX_K (section 9q)
  const auto start = std::chrono::steady_clock::now();
  if (int rc = migrate_if_due(now, false)) return rc;
  const bool have_r = cfg.search_recent, have_h = cfg.search_historical && ivf_trained_;
  // a part that is not searched leaves the grid: one row (column) stands for all of them
  const uint32_t Eg = have_r ? E : 0, Pg = have_h ? P : 0;
  const size_t nt = (size_t)B * k, nr = (size_t)B * rk, nh = (size_t)B * hk;
  std::vector<uint64_t> tid(nt), rid(nr * Eg), hid(nh * Pg);
  std::vector<float> td(nt), rd(nr * Eg), hd(nh * Pg);
  std::vector<uint32_t> tcn(B), rcn((size_t)B * Eg), hcn((size_t)B * Pg);
  GridParts p{B, k, tid.data(), tcn.data(), Eg, rk, rid.data(), rd.data(), rcn.data(), Pg, hk, hid.data(), hd.data(), hcn.data()};
  // neither part: every result is empty.  One historical list of no entries says so to the device.
  const uint64_t no_id = FVDB_NO_ID;
  const float no_dist = __builtin_huge_valf();
  const std::vector<uint32_t> none(B, 0);
  std::vector<uint64_t> none_ids;
  std::vector<float> none_dist;
  if (!Eg && !Pg) {
    none_ids.assign(B, no_id);
    none_dist.assign(B, no_dist);
    p.P = 1, p.hk = 1, p.hid = none_ids.data(), p.hd = none_dist.data(), p.hcn = none.data();
  }
  std::vector<float> tr((size_t)p.rows() * p.cols()), tp(tr.size());
  {
    std::shared_lock<std::shared_mutex> r(rw_);  // one hold for every search: they see the same rows
    fill_empty(tid.data(), td.data(), tcn.data(), B, k);
    int rc;
    if ((rc = exact_locked(q, B, dim, cfg, tid.data(), td.data(), tcn.data(), wide))) return rc;
    if (Eg) {
      // search_locked's recent part, one ef after the other: the batch staged once in a slot leased for the call, the
      // traversal begun and collected there (a search the checks answer, or one for the host walk, runs in the end)
      Lease lease(this, Lease::kAnyFree, Lease::kTake);
      Slot& sl = *lease.sl;
      if ((rc = stage_finite(sl, q, B, dim))) return rc;
      const float* qd = (const float*)sl.d_q.dev;
      for (uint32_t e = 0; e < Eg; ++e) {
        int rcb = 0;
        recent_->search_dev_begin(qd, B, dim, rk, efs[e], &rcb, lease.index(), nullptr);
        if ((rc = recent_->search_dev_end(qd, B, dim, rk, efs[e], &rid[e * nr], &rd[e * nr], &rcn[(size_t)e * B], lease.index(), nullptr)))
          return rc;
      }
    }
    for (uint32_t j = 0; j < Pg; ++j)
      if ((rc = historical_->search(q, B, dim, hk, n_probes[j], &hid[j * nh], &hd[j * nh], &hcn[(size_t)j * B]))) return rc;
    std::lock_guard<std::mutex> lk(qual_mu_);
    if ((rc = quality_grid_totals(ctx_ivf_, qual_, p, tr.data(), tp.data()))) return rc;
  }
  const uint32_t rows = E ? E : 1, cols = P ? P : 1;
  out->rows = rows, out->cols = cols;
  out->avg_recall.resize((size_t)rows * cols);
  out->avg_precision.resize((size_t)rows * cols);
  for (uint32_t i = 0; i < rows; ++i)
    for (uint32_t j = 0; j < cols; ++j) {
      const size_t at = (size_t)(Eg ? i : 0) * p.cols() + (Pg ? j : 0);
      const SearchQuality s = quality_of(tr[at], tp[at], B, start);
      out->avg_recall[(size_t)i * cols + j] = s.avg_recall;
      out->avg_precision[(size_t)i * cols + j] = s.avg_precision;
      out->avg_query_time_ms = s.avg_query_time_ms;
    }
  out->queries_evaluated = B;
  return FVDB_OK;
}

int HybridIndex::search_allowed(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, const uint64_t* allowed,
                                uint64_t n_allowed, double now, uint64_t* ids, float* dist, uint32_t* counts) {
  if (sharded_ || shard_world_) return FVDB_E_UNSUPPORTED;  // the sharded IVF step takes no mask
  if (n_allowed && !allowed) return FVDB_E_INVALID;
  return search_impl(q, false, B, dim, cfg, now, ids, dist, counts, allowed, n_allowed, true);
}

// One allow-set per query.  The parts run one after the other, as exact_locked's do: the grouped
// calls of the two index classes are blocking.
int HybridIndex::search_allowed_groups(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg,
                                       const AllowGroups& groups, double now, uint64_t* ids, float* dist, uint32_t* counts) {
  if (sharded_ || shard_world_) return FVDB_E_UNSUPPORTED;  // the sharded IVF step takes no mask table
  if (!groups.valid(B)) return FVDB_E_INVALID;
  const uint32_t k = (uint32_t)cfg.k;
  fill_empty(ids, dist, counts, B, k);
  if (!initialized_ || B == 0 || k == 0) return FVDB_OK;
  if (int rc = migrate_if_due(now, false)) return rc;
  std::shared_lock<std::shared_mutex> r(rw_);  // every mask below is built under it, after the migration
  return groups_locked(q, B, dim, cfg, groups, ids, dist, counts);
}

int HybridIndex::groups_locked(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, const AllowGroups& groups,
                               uint64_t* ids, float* dist, uint32_t* counts) {
  const uint32_t k = (uint32_t)cfg.k;
  if (int rc = check_finite(q, (uint64_t)B * dim)) return rc;
  const uint32_t rk = cfg.rk(), hk = cfg.hk();
  std::vector<uint64_t> rid, hid;
  std::vector<float> rd, hd;
  std::vector<uint32_t> rc_(B, 0), hc(B, 0);
  const bool have_r = cfg.search_recent, have_h = cfg.search_historical && ivf_trained_;
  if (have_r) {
    rid.resize((size_t)B * rk);
    rd.resize((size_t)B * rk);
    Lease lease(this, Lease::kAnyFree, Lease::kTake);  // the graph's slot of the same index is this call's
    if (int rc = recent_->search_allowed_groups(q, B, dim, rk, (uint32_t)cfg.hnsw_ef, groups, rid.data(), rd.data(), rc_.data(),
                                                lease.index(), true))
      return rc;
  }
  if (have_h) {
    hid.resize((size_t)B * hk);
    hd.resize((size_t)B * hk);
    if (int rc = historical_->search_allowed_groups(q, B, dim, hk, (uint32_t)cfg.ivf_n_probe, groups, hid.data(), hd.data(), hc.data()))
      return rc;
  }
  merge_parts(B, k, rk, hk, have_r, rid.data(), rd.data(), rc_.data(), have_h, hid.data(), hd.data(), hc.data(), ids, dist, counts);
  return FVDB_OK;
}

// src/hybrid/core.rs:513-549
int HybridIndex::search_with_filter(const float* q, uint32_t B, uint32_t dim, uint64_t k, FilterFn matches, void* user,
                                    double now, uint64_t* ids, float* dist, uint32_t* counts) {
  HybridSearchConfig cfg;  // SearchConfig::default() with k (:419-423)
  cfg.k = k;
  if (!matches) return search_impl(q, false, B, dim, cfg, now, ids, dist, counts);
  const uint64_t k3 = k * 3;  // k-oversampling, multiplier 3 (:527-529)
  cfg.k = k3;
  std::vector<uint64_t> ci((size_t)B * k3);
  std::vector<float> cd((size_t)B * k3);
  std::vector<uint32_t> cc(B, 0);
  const int rc = search_impl(q, false, B, dim, cfg, now, ci.data(), cd.data(), cc.data());
  if (rc) return rc;
  for (uint32_t b = 0; b < B; ++b) {
    uint32_t w = 0;
    for (uint32_t i = 0; i < cc[b] && w < k; ++i) {  // candidates are sorted by distance already; truncate(k) (:543-546)
      const uint64_t id = ci[(size_t)b * k3 + i];
      if (!matches(id, user)) continue;
      ids[(size_t)b * k + w] = id;
      dist[(size_t)b * k + w] = cd[(size_t)b * k3 + i];
      ++w;
    }
    counts[b] = w;
    for (uint32_t i = w; i < k; ++i) {
      ids[(size_t)b * k + i] = FVDB_NO_ID;
      dist[(size_t)b * k + i] = __builtin_huge_valf();
    }
  }
  return FVDB_OK;
}

// delete: src/hybrid/core.rs:904-937
int HybridIndex::remove(uint64_t id, double now) {
  std::unique_lock<std::shared_mutex> w(rw_, std::defer_lock);
  if (int rc = write_lock(w)) return rc;
  auto it = timestamps_.find(id);
  if (it == timestamps_.end()) return FVDB_E_NOT_FOUND;
  if (age_of(now, it->second) < cfg_.recent_threshold_s) return recent_->mark_deleted(id);
  return historical_->mark_deleted(id);
}

}  // namespace fvdbh
