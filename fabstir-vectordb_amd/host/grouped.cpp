// grouped.cpp — grouped search of the three index classes: the ordinary search of fetch_k, the
// candidates' keys looked up in HBM under one column of a metadata table (fvdb_group_keys_of_ids_dev), and
// fvdb_group_select_dev.  Ids, the search's distances and counts go down in one copy per sub-batch and the groups come
// back in one.  No key, no metadata value and no distance is computed or compared on the host.
#include <algorithm>
#include <cstring>
#include <vector>

#include "fvdb_host.hpp"

namespace fvdbh {

void fill_empty_grouped(const GroupedOut& out, uint32_t B, uint32_t k, uint32_t group_size) {
  const size_t cells = (size_t)B * k * group_size, rows = (size_t)B * k;
  for (size_t i = 0; i < cells; ++i) {
    out.ids[i] = FVDB_NO_ID;
    out.dist[i] = __builtin_huge_valf();
    out.ranks[i] = FVDB_NO_ROW;
  }
  for (size_t i = 0; i < rows; ++i) {
    out.members[i] = out.totals[i] = 0;
    out.key_tags[i] = 0;
    out.key_vals[i] = 0;
  }
  for (uint32_t b = 0; b < B; ++b) out.groups[b] = out.flags[b] = 0;
}

namespace {
struct StageBlock : DevBuf {  // the device block of a call and its pinned twin, freed on every way out
  ~StageBlock() { release(); }
};
inline uint64_t up8(uint64_t x) { return (x + 7) & ~7ull; }
}  // namespace

int select_grouped(fvdb_ctx* ctx, const GroupBy& by, uint32_t B, uint32_t fetch_k, uint32_t k, uint32_t group_size, bool distinct,
                   int missing, const uint64_t* cid, const float* cd, const uint32_t* cc, const GroupedOut& out) {
  fvdb_ctx* table_ctx = fvdb_group_keys_ctx(by.table);  // the lookup runs on its stream, whatever the caller believes
  if (!table_ctx) return FVDB_E_INVALID;
  const uint64_t cells = (uint64_t)k * group_size;
  const uint64_t per_query = (uint64_t)fetch_k * (8 + 4 + 1 + 8) + 4 + cells * 16 + (uint64_t)k * (4 + 4 + 1 + 8) + 8;
  const uint32_t step = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(kGroupedStageBytes / per_query, 1), B);
  // the block of a sub-batch, every array 8-byte aligned: the candidates (one upload), their keys, the outputs (one download)
  const uint64_t nc = (uint64_t)step * fetch_k, ng = (uint64_t)step * k, no = (uint64_t)step * cells;
  const uint64_t o_cd = nc * 8, o_cc = up8(o_cd + nc * 4), o_kt = up8(o_cc + (uint64_t)step * 4), o_kv = up8(o_kt + nc);
  const uint64_t o_oi = o_kv + nc * 8, o_od = o_oi + no * 8, o_or = up8(o_od + no * 4), o_om = up8(o_or + no * 4);
  const uint64_t o_ot = up8(o_om + ng * 4), o_okt = up8(o_ot + ng * 4), o_okv = up8(o_okt + ng), o_og = o_okv + ng * 8;
  const uint64_t o_of = up8(o_og + (uint64_t)step * 4), bytes = o_of + (uint64_t)step * 4;
  StageBlock blk;
  if (int rc = blk.reserve(ctx, bytes, true)) return rc;
  char* d = (char*)blk.dev;
  char* h = (char*)blk.host;
  for (uint32_t b0 = 0; b0 < B; b0 += step) {
    const uint32_t nb = std::min(step, B - b0);
    const uint64_t n = (uint64_t)nb * fetch_k, g = (uint64_t)nb * k, o = (uint64_t)nb * cells;
    int rc;
    std::memcpy(h, cid + (size_t)b0 * fetch_k, (size_t)n * 8);
    std::memcpy(h + o_cd, cd + (size_t)b0 * fetch_k, (size_t)n * 4);
    std::memcpy(h + o_cc, cc + b0, (size_t)nb * 4);
    if ((rc = fvdb_dev_upload(ctx, d, h, (size_t)o_kt))) return rc;  // returns when the bytes have arrived
    if ((rc = fvdb_group_keys_of_ids_dev(by.table, by.column, (const uint64_t*)d, n, (uint8_t*)(d + o_kt), (uint64_t*)(d + o_kv)))) return rc;
    if (table_ctx != ctx && (rc = fvdb_ctx_synchronize(table_ctx))) return rc;  // another stream: the selection waits for the keys
    if ((rc = fvdb_group_select_dev(ctx, (const uint64_t*)d, (const float*)(d + o_cd), (const uint32_t*)(d + o_cc),
                                    (const uint8_t*)(d + o_kt), (const uint64_t*)(d + o_kv), nb, fetch_k, k, group_size, distinct ? 1 : 0,
                                    missing, (uint64_t*)(d + o_oi), (float*)(d + o_od), (uint32_t*)(d + o_or), (uint32_t*)(d + o_om),
                                    (uint32_t*)(d + o_ot), (uint8_t*)(d + o_okt), (uint64_t*)(d + o_okv), (uint32_t*)(d + o_og),
                                    (uint32_t*)(d + o_of))))
      return rc;
    // one copy of the nine output arrays, ordered behind the selection on ctx's stream
    if ((rc = fvdb_dev_download(ctx, h + o_oi, d + o_oi, (size_t)(bytes - o_oi)))) return rc;
    std::memcpy(out.ids + (size_t)b0 * cells, h + o_oi, (size_t)o * 8);
    std::memcpy(out.dist + (size_t)b0 * cells, h + o_od, (size_t)o * 4);
    std::memcpy(out.ranks + (size_t)b0 * cells, h + o_or, (size_t)o * 4);
    std::memcpy(out.members + (size_t)b0 * k, h + o_om, (size_t)g * 4);
    std::memcpy(out.totals + (size_t)b0 * k, h + o_ot, (size_t)g * 4);
    std::memcpy(out.key_tags + (size_t)b0 * k, h + o_okt, (size_t)g);
    std::memcpy(out.key_vals + (size_t)b0 * k, h + o_okv, (size_t)g * 8);
    std::memcpy(out.groups + b0, h + o_og, (size_t)nb * 4);
    std::memcpy(out.flags + b0, h + o_of, (size_t)nb * 4);
  }
  return FVDB_OK;
}

namespace {
// the shape the three classes share: refusals, empty outputs, the class's own search of fetch_k, the selection
template <class Search>
int grouped_impl(fvdb_ctx* ctx, const GroupBy& by, uint32_t B, uint32_t fetch_k, uint32_t k, uint32_t group_size, bool distinct,
                 int missing, const GroupedOut& out, Search search) {
  if (int rc = check_grouped(fetch_k, k, group_size, missing)) return rc;
  if (B == 0) return FVDB_OK;
  fill_empty_grouped(out, B, k, group_size);
  std::vector<uint64_t> cid((size_t)B * fetch_k);
  std::vector<float> cd((size_t)B * fetch_k);
  std::vector<uint32_t> cc(B, 0);
  fill_empty(cid.data(), cd.data(), cc.data(), B, fetch_k);
  if (int rc = search(cid.data(), cd.data(), cc.data())) return rc;
  return select_grouped(ctx, by, B, fetch_k, k, group_size, distinct, missing, cid.data(), cd.data(), cc.data(), out);
}
}  // namespace

int search_grouped(IVFIndex& ix, fvdb_ctx* ctx, const GroupBy& by, const float* q, uint32_t B, uint32_t dim, uint32_t k,
                   uint32_t group_size, uint32_t fetch_k, bool distinct, int missing, uint32_t n_probe, const uint64_t* allowed,
                   uint64_t n_allowed, const GroupedOut& out) {
  return grouped_impl(ctx, by, B, fetch_k, k, group_size, distinct, missing, out, [&](uint64_t* cid, float* cd, uint32_t* cc) {
    return allowed ? ix.search_allowed(q, B, dim, fetch_k, n_probe, allowed, n_allowed, cid, cd, cc)
                   : ix.search(q, B, dim, fetch_k, n_probe, cid, cd, cc);
  });
}

int search_grouped(HNSWIndex& ix, fvdb_ctx* ctx, const GroupBy& by, const float* q, uint32_t B, uint32_t dim, uint32_t k,
                   uint32_t group_size, uint32_t fetch_k, bool distinct, int missing, uint32_t ef, const uint64_t* allowed,
                   uint64_t n_allowed, const GroupedOut& out) {
  return grouped_impl(ctx, by, B, fetch_k, k, group_size, distinct, missing, out, [&](uint64_t* cid, float* cd, uint32_t* cc) {
    return allowed ? ix.search_allowed(q, B, dim, fetch_k, ef, allowed, n_allowed, cid, cd, cc)
                   : ix.search(q, B, dim, fetch_k, ef, cid, cd, cc);
  });
}

int search_grouped(HybridIndex& ix, fvdb_ctx* ctx, const GroupBy& by, const float* q, uint32_t B, uint32_t dim,
                   const HybridSearchConfig& cfg, uint32_t group_size, uint32_t fetch_k, bool distinct, int missing, double now,
                   const uint64_t* allowed, uint64_t n_allowed, const GroupedOut& out) {
  const uint32_t k = (uint32_t)std::min<uint64_t>(cfg.k, 0xFFFFFFFFu);
  HybridSearchConfig c = cfg;  // the candidates: search() at k = fetch_k with the caller's other settings
  c.k = fetch_k;
  c.recent_k = c.historical_k = 0;
  return grouped_impl(ctx, by, B, fetch_k, k, group_size, distinct, missing, out, [&](uint64_t* cid, float* cd, uint32_t* cc) {
    return allowed ? ix.search_allowed(q, B, dim, c, allowed, n_allowed, now, cid, cd, cc) : ix.search(q, B, dim, c, now, cid, cd, cc);
  });
}

}  // namespace fvdbh
