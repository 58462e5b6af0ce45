// diverse.cpp — diverse search of the three index classes: the ordinary search of fetch_k, the
// candidates' rows gathered in HBM by location, and fvdb_mmr_select_dev.  No row and no distance is computed or
// copied on the host: ids, the search's distances, counts and row locations go down, the picks come back.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "fvdb_host.hpp"

namespace fvdbh {

static std::atomic<uint64_t> g_stage_budget{0};  // set_diverse_stage_budget's value; 0: the environment's, or the default
void set_diverse_stage_budget(uint64_t bytes) { g_stage_budget.store(bytes); }

uint64_t diverse_stage_budget() {
  if (const uint64_t set = g_stage_budget.load()) return set;
  static const uint64_t budget = [] {
    const char* e = std::getenv("FVDB_DIVERSE_STAGE_BYTES");
    const unsigned long long v = e ? std::strtoull(e, nullptr, 10) : 0ull;
    return v ? (uint64_t)v : kDiverseStageBytes;
  }();
  return budget;
}

int select_diverse(fvdb_ctx* ctx, DiverseStage& st, RowSource& src, uint32_t dim, uint32_t B, uint32_t fetch_k, uint32_t k,
                   float lam, bool distinct, const uint64_t* cid, const float* cd, const uint32_t* cc, uint64_t* ids, float* dist,
                   uint32_t* ranks, uint32_t* counts) {
  const uint32_t dpad = (dim + 3u) & ~3u;
  const uint64_t per_query = (uint64_t)fetch_k * dpad * 4;
  const uint32_t step = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(diverse_stage_budget() / per_query, 1), B);
  std::lock_guard<std::mutex> lk(st.mu);
  // io block of a sub-batch: ids, distances, counts and locations in; picks (ids, distances, ranks, counts) out
  const uint64_t nc = (uint64_t)step * fetch_k, nk = (uint64_t)step * k;
  const uint64_t o_cd = nc * 8, o_cc = o_cd + nc * 4, o_loc = o_cc + (uint64_t)step * 4, o_out = (o_loc + nc * 4 + 7) & ~7ull;
  const uint64_t o_od = o_out + nk * 8, o_or = o_od + nk * 4, o_oc = o_or + nk * 4, bytes = o_oc + (uint64_t)step * 4;
  int rc;
  if ((rc = st.rows.reserve(ctx, (uint64_t)step * per_query, false)) || (rc = st.io.reserve(ctx, bytes, true))) return rc;
  char* d = (char*)st.io.dev;
  char* h = (char*)st.io.host;
  std::vector<uint8_t> want;
  for (uint32_t b0 = 0; b0 < B; b0 += step) {
    const uint32_t nb = std::min(step, B - b0);
    const uint64_t n = (uint64_t)nb * fetch_k;
    const uint64_t* sid = cid + (size_t)b0 * fetch_k;
    want.assign(n, 0);
    for (uint32_t b = 0; b < nb; ++b)
      for (uint32_t c = 0; c < std::min(cc[b0 + b], fetch_k); ++c) want[(size_t)b * fetch_k + c] = 1;
    std::memcpy(h, sid, n * 8);
    std::memcpy(h + o_cd, cd + (size_t)b0 * fetch_k, n * 4);
    std::memcpy(h + o_cc, cc + b0, (size_t)nb * 4);
    if ((rc = fvdb_dev_upload(ctx, d, h, (size_t)o_loc))) return rc;
    if ((rc = src.gather(ctx, sid, want.data(), n, (uint32_t*)(d + o_loc), (float*)st.rows.dev, dpad))) return rc;
    for (uint64_t i = 0; i < n; ++i)
      if (want[i]) return FVDB_E_NOT_FOUND;
    if ((rc = fvdb_mmr_select_dev(ctx, (const float*)st.rows.dev, dpad, (const uint64_t*)d, (const float*)(d + o_cd),
                                  (const uint32_t*)(d + o_cc), nb, fetch_k, k, lam, distinct ? 1 : 0, (uint64_t*)(d + o_out),
                                  (float*)(d + o_od), (uint32_t*)(d + o_or), (uint32_t*)(d + o_oc))))
      return rc;
    if ((rc = fvdb_dev_download_async(ctx, h + o_out, d + o_out, (size_t)(bytes - o_out))) || (rc = fvdb_ctx_synchronize(ctx))) return rc;
    const uint64_t m = (uint64_t)nb * k;
    std::memcpy(ids + (size_t)b0 * k, h + o_out, m * 8);
    std::memcpy(dist + (size_t)b0 * k, h + o_od, m * 4);
    std::memcpy(ranks + (size_t)b0 * k, h + o_or, m * 4);
    std::memcpy(counts + b0, h + o_oc, (size_t)nb * 4);
  }
  return FVDB_OK;
}

// ---- IVFIndex ----
int IVFIndex::gather_rows_dev(fvdb_ctx* ctx, const uint64_t* ids, uint8_t* want, uint64_t n, float* rows_dev, uint32_t stride) {
  if (!dev_) return FVDB_E_NOT_TRAINED;
  std::vector<uint32_t> cl(n, FVDB_NO_ROW), ps(n, 0);
  bool any = false;
  for (uint64_t i = 0; i < n; ++i) {
    if (!want[i]) continue;
    auto r = where_.equal_range(ids[i]);
    if (r.first == r.second) continue;
    Loc best = r.first->second;  // the lowest (cluster, position), as get_vectors
    for (auto it = r.first; it != r.second; ++it)
      if (it->second.cluster < best.cluster || (it->second.cluster == best.cluster && it->second.pos < best.pos)) best = it->second;
    cl[i] = best.cluster;
    ps[i] = best.pos;
    want[i] = 0;
    any = true;
  }
  return any ? fvdb_ivf_get_rows_dev_strided(dev_, ctx, cl.data(), ps.data(), n, rows_dev, stride) : FVDB_OK;
}

namespace {
struct IvfRows : RowSource {
  IVFIndex* ix;
  explicit IvfRows(IVFIndex* i) : ix(i) {}
  int gather(fvdb_ctx* ctx, const uint64_t* ids, uint8_t* want, uint64_t n, uint32_t*, float* rows_dev, uint32_t stride) override {
    return ix->gather_rows_dev(ctx, ids, want, n, rows_dev, stride);
  }
};
struct GraphRows : RowSource {
  HNSWIndex* ix;
  explicit GraphRows(HNSWIndex* i) : ix(i) {}
  int gather(fvdb_ctx* ctx, const uint64_t* ids, uint8_t* want, uint64_t n, uint32_t* loc_dev, float* rows_dev, uint32_t stride) override {
    return ix->gather_rows_dev(ctx, ids, want, n, loc_dev, rows_dev, stride);
  }
};
struct HybridRows : RowSource {  // the recent part answers first, the historical one for the rest
  HNSWIndex* recent;
  IVFIndex* historical;
  bool have_h;
  int gather(fvdb_ctx* ctx, const uint64_t* ids, uint8_t* want, uint64_t n, uint32_t* loc_dev, float* rows_dev, uint32_t stride) override {
    if (int rc = recent->gather_rows_dev(ctx, ids, want, n, loc_dev, rows_dev, stride)) return rc;
    if (!have_h || std::find(want, want + n, (uint8_t)1) == want + n) return FVDB_OK;
    return historical->gather_rows_dev(ctx, ids, want, n, rows_dev, stride);
  }
};
}  // namespace

int IVFIndex::search_diverse(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t fetch_k, float lam, bool distinct,
                             uint32_t n_probe, const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist,
                             uint32_t* ranks, uint32_t* counts) {
  if (int rc = check_diverse(k, fetch_k, lam)) return rc;
  if (!trained_) return FVDB_E_NOT_TRAINED;
  if (dim != dim_) return FVDB_E_DIM;
  if (B == 0) return FVDB_OK;
  std::vector<uint64_t> cid((size_t)B * fetch_k);
  std::vector<float> cd((size_t)B * fetch_k);
  std::vector<uint32_t> cc(B, 0);
  if (int rc = allowed ? search_allowed(q, B, dim, fetch_k, n_probe, allowed, n_allowed, cid.data(), cd.data(), cc.data())
                       : search(q, B, dim, fetch_k, n_probe, cid.data(), cd.data(), cc.data()))
    return rc;
  IvfRows src(this);
  return select_diverse(ctx_, diverse_, src, dim, B, fetch_k, k, lam, distinct, cid.data(), cd.data(), cc.data(), ids, dist, ranks,
                        counts);
}

// ---- HNSWIndex ----
int HNSWIndex::gather_rows_dev(fvdb_ctx* ctx, const uint64_t* ids, uint8_t* want, uint64_t n, uint32_t* loc_dev, float* rows_dev,
                               uint32_t stride) {
  std::vector<uint32_t> rows(n, FVDB_NO_ROW);
  bool any = false;
  for (uint64_t i = 0; i < n; ++i)
    if (want[i] && store_row_of(ids[i], &rows[i])) {
      want[i] = 0;
      any = true;
    }
  if (!any) return FVDB_OK;
  if (int rc = fvdb_dev_upload(ctx, loc_dev, rows.data(), (size_t)n * 4)) return rc;
  return fvdb_store_get_rows_dev(store_, ctx, loc_dev, n, rows_dev, stride);
}

int HNSWIndex::search_diverse(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t fetch_k, float lam, bool distinct,
                              uint32_t ef, const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* ranks,
                              uint32_t* counts) {
  if (int rc = check_diverse(k, fetch_k, lam)) return rc;
  fill_empty_diverse(ids, dist, ranks, counts, B, k);
  if (B == 0) return FVDB_OK;
  std::vector<uint64_t> cid((size_t)B * fetch_k);
  std::vector<float> cd((size_t)B * fetch_k);
  std::vector<uint32_t> cc(B, 0);
  if (int rc = allowed ? search_allowed(q, B, dim, fetch_k, ef, allowed, n_allowed, cid.data(), cd.data(), cc.data())
                       : search(q, B, dim, fetch_k, ef, cid.data(), cd.data(), cc.data()))
    return rc;
  if (!store_ || std::all_of(cc.begin(), cc.end(), [](uint32_t c) { return c == 0; })) return FVDB_OK;  // nothing to choose from
  GraphRows src(this);
  return select_diverse(ctx_, diverse_, src, dim, B, fetch_k, k, lam, distinct, cid.data(), cd.data(), cc.data(), ids, dist, ranks,
                        counts);
}

// ---- HybridIndex ----
int HybridIndex::search_diverse(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, uint32_t fetch_k, float lam,
                                bool distinct, double now, const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist,
                                uint32_t* ranks, uint32_t* counts) {
  return diverse_impl(q, B, dim, cfg, fetch_k, lam, distinct, now, allowed, n_allowed, nullptr, ids, dist, ranks, counts);
}

int HybridIndex::search_diverse_groups(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, uint32_t fetch_k,
                                       float lam, bool distinct, const AllowGroups& groups, double now, uint64_t* ids, float* dist,
                                       uint32_t* ranks, uint32_t* counts) {
  return diverse_impl(q, B, dim, cfg, fetch_k, lam, distinct, now, nullptr, 0, &groups, ids, dist, ranks, counts);
}

int HybridIndex::diverse_impl(const float* q, uint32_t B, uint32_t dim, const HybridSearchConfig& cfg, uint32_t fetch_k, float lam,
                              bool distinct, double now, const uint64_t* allowed, uint64_t n_allowed, const AllowGroups* groups,
                              uint64_t* ids, float* dist, uint32_t* ranks, uint32_t* counts) {
  if (sharded_ || shard_world_) return FVDB_E_UNSUPPORTED;  // a rank holds only the lists it owns
  if (groups && !groups->valid(B)) return FVDB_E_INVALID;
  const uint32_t k = (uint32_t)std::min<uint64_t>(cfg.k, 0xFFFFFFFFu);
  if (int rc = check_diverse(k, fetch_k, lam)) return rc;
  if (n_allowed && !allowed) return FVDB_E_INVALID;
  fill_empty_diverse(ids, dist, ranks, counts, B, k);
  if (!initialized_ || B == 0) return FVDB_OK;
  if (int rc = migrate_if_due(now, false)) return rc;
  std::shared_lock<std::shared_mutex> r(rw_);  // the search, the lookup and the gather see the same rows
  HybridSearchConfig c = cfg;
  c.k = fetch_k;
  c.recent_k = c.historical_k = 0;
  std::vector<uint64_t> cid((size_t)B * fetch_k);
  std::vector<float> cd((size_t)B * fetch_k);
  std::vector<uint32_t> cc(B, 0);
  fill_empty(cid.data(), cd.data(), cc.data(), B, fetch_k);
  if (int rc = groups ? groups_locked(q, B, dim, c, *groups, cid.data(), cd.data(), cc.data())
                      : search_locked(q, false, B, dim, c, cid.data(), cd.data(), cc.data(), allowed, n_allowed, allowed != nullptr))
    return rc;
  if (std::all_of(cc.begin(), cc.end(), [](uint32_t n) { return n == 0; })) return FVDB_OK;
  HybridRows src;
  src.recent = recent_;
  src.historical = historical_;
  src.have_h = ivf_trained_;
  return select_diverse(ctx_ivf_, diverse_, src, dim, B, fetch_k, k, lam, distinct, cid.data(), cd.data(), cc.data(), ids, dist, ranks,
                        counts);
}

}  // namespace fvdbh
