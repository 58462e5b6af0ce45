// flat_search.h — exact search of the C ABI (include/fvdb.h, "exact search"): the flat scan of a
// graph's row store, its form for k up to FVDB_MAX_K_WIDE (section 9q), radius search and count (section 9t), the comparison of two resident id blocks and
// the quality grid over the parts of a hybrid search (section 9r).
// Included at the end of fvdb_hip.cpp, after allow_masks.h, for the same reason: the kernels lean on kernels_scan.h,
// which lives in this translation unit, and what they need of the graph comes through graph_mask_source /
// graph_scan_inputs (fvdb_internal.h).
#pragma once
#include "kernels_flat.h"
#include "kernels_flat_wide.h"
#include "kernels_grid.h"
#include "kernels_range.h"

namespace {

// queries of one launch pair: bounds the partial lists ((4096 Q + B) * k keys at the most, 84 MB at k = 256)
constexpr uint32_t kFlatSubBatch = 8192;

template <int Q, int KR>
void launch_flat_scan(fvdb_ctx* ctx, const FlatScanArgs& a, bool f16 /* the store's rows */, uint32_t* out_nodes, float* out_dist, uint32_t* out_counts) {
  if (a.slices)
    hipLaunchKernelGGL((f16 ? flat_scan_kernel<Q, KR, half_t> : flat_scan_kernel<Q, KR, float>), dim3(cdiv(a.B, Q), cdiv(a.slices, 4)),
                       dim3(256), 0, ctx->stream, a);
  hipLaunchKernelGGL((flat_merge_kernel<KR>), dim3(cdiv(a.B, 4)), dim3(256), 0, ctx->stream, a.part, a.slices, a.B, a.k, out_nodes,
                     out_dist, out_counts);
}

// the wide form's arena budget, kWideArenaBytes unless FVDB_FLAT_WIDE_ARENA_BYTES says otherwise (read at every call: a
// test hook that forces several sub-batches on a small graph)
uint64_t flat_wide_arena_bytes() {
  const char* e = getenv("FVDB_FLAT_WIDE_ARENA_BYTES");
  return e ? strtoull(e, nullptr, 10) : kWideArenaBytes;
}

constexpr int kFlatWideQ = 8;  // queries of a score group (DESIGN.md section 9q has the figures of 8 and 16)

// the argument checks of the two flat entry points, in the C ABI's order and with its messages; the k limit and its
// message are the caller's.  FVDB_OK: *src and *ctx are set.
int flat_check_args(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, uint32_t k, uint32_t k_max, const char* k_msg,
                    bool have_buffers, GraphMaskSource* src, fvdb_ctx** ctx_out) {
  if (!g) return FVDB_E_INVALID;
  int rc = graph_mask_source(g, src);
  if (rc) return rc;
  fvdb_ctx* ctx = *ctx_out = on ? on : src->store->ctx;
  if (slot >= kGraphSlots) FAIL(ctx, FVDB_E_INVALID, "slot out of range");
  if (on && on->device != src->store->ctx->device) FAIL(ctx, FVDB_E_INVALID, "context of another device");
  if (mask && mask->graph != g) FAIL(ctx, FVDB_E_INVALID, "mask of another graph");
  if (mask && mask->stamp != src->mutations) FAIL(ctx, FVDB_E_INVALID, "stale mask: the graph changed after the mask was created");
  if (k == 0 || k > k_max) FAIL(ctx, FVDB_E_UNSUPPORTED, k_msg);
  if (!have_buffers) FAIL(ctx, FVDB_E_INVALID, "null argument");
  return FVDB_OK;
}

// the slices of n rows for a sub-batch of Bs queries in groups of Q: enough (group, slice) waves to fill the device at a
// small batch, a slice no shorter than four tiles of 64 rows; n == 0: no slice
void flat_slice_plan(uint32_t n, uint32_t Bs, uint32_t Q, uint32_t* slices, uint32_t* slice_tiles) {
  const uint32_t tiles = cdiv(n, 64);
  *slices = *slice_tiles = 0;
  if (!n) return;
  *slice_tiles = cdiv(tiles, std::max<uint32_t>(1, std::min<uint32_t>(cdiv(tiles, 4), cdiv(4096, cdiv(Bs, Q)))));
  *slices = cdiv(tiles, *slice_tiles);
}

}  // namespace

extern "C" {

int fvdb_graph_search_flat_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                    uint32_t k, uint32_t* out_nodes_dev, float* out_dist_dev, uint32_t* out_counts_dev) {
  GraphMaskSource src{};
  fvdb_ctx* ctx = nullptr;
  int rc = flat_check_args(g, on, slot, mask, k, FVDB_MAX_K, "exact scan: k must be in 1..FVDB_MAX_K",
                           q_dev && out_nodes_dev && out_dist_dev && out_counts_dev, &src, &ctx);
  if (rc) return rc;
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  fvdb_store* s = src.store;
  const int kr = k <= 64 ? 1 : (k <= 128 ? 2 : 4);
  const uint32_t Q = kr == 4 ? 4 : 8;  // queries of a group: the wider lists leave registers for fewer
  // sub-batches run one after the other on the stream and share the slot's scratch
  for (uint32_t b0 = 0; b0 < B; b0 += kFlatSubBatch) {
    const uint32_t Bs = std::min(kFlatSubBatch, B - b0);
    FlatScanArgs a{};
    a.rows = s->data;
    a.dead = mask ? mask->flags.as<uint32_t>() : src.deleted;
    a.dpad = s->dpad;
    a.n = src.n;
    a.B = Bs;
    a.k = k;
    flat_slice_plan(src.n, Bs, Q, &a.slices, &a.slice_tiles);
    rc = graph_scan_inputs(g, ctx, slot, q_dev + (size_t)b0 * s->d, Bs, (size_t)a.slices * Bs * k * 8, &a.queries, &a.part);
    if (rc) return rc;
    uint32_t* on_ = out_nodes_dev + (size_t)b0 * k;
    float* od_ = out_dist_dev + (size_t)b0 * k;
    uint32_t* oc_ = out_counts_dev + b0;
    switch (kr) {
      case 1: launch_flat_scan<8, 1>(ctx, a, s->f16(), on_, od_, oc_); break;
      case 2: launch_flat_scan<8, 2>(ctx, a, s->f16(), on_, od_, oc_); break;
      default: launch_flat_scan<4, 4>(ctx, a, s->f16(), on_, od_, oc_); break;
    }
    HIPCHK(ctx, hipGetLastError());
  }
  return FVDB_OK;
}

// The arena form of the flat scan, behind the checks of its two entry points: every (query, row) distance word to the
// arena, then one workgroup per query selects — the k nearest (radius_dev null), or the ball of radius_dev[b] capped at k
// with its size to out_totals_dev.
static int flat_arena_search(fvdb_graph* g, fvdb_ctx* ctx, const GraphMaskSource& src, uint32_t slot, fvdb_mask* mask,
                             const float* q_dev, uint32_t B, uint32_t k, uint32_t* out_nodes_dev, float* out_dist_dev,
                             uint32_t* out_counts_dev, const float* radius_dev, uint32_t* out_totals_dev) {
  int rc = FVDB_OK;
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  fvdb_store* s = src.store;
  constexpr uint32_t Q = kFlatWideQ;
  const uint64_t stride = (uint64_t)cdiv(src.n, 64) * 64;  // arena words of a query: whole tiles; < 2^32 whatever n
  // queries of a sub-batch: their arena fits the budget, at least one; sub-batches run one after the other on the
  // stream and share the slot's scratch
  const uint64_t fit = std::max<uint64_t>(flat_wide_arena_bytes() / std::max<uint64_t>(stride * 4, 1), 1);
  const uint32_t step = (uint32_t)std::min<uint64_t>(fit, kFlatSubBatch);
  for (uint32_t b0 = 0; b0 < B; b0 += step) {
    const uint32_t Bs = std::min(step, B - b0);
    FlatScoreArgs a{};
    a.rows = s->data;
    a.dead = mask ? mask->flags.as<uint32_t>() : src.deleted;
    a.dpad = s->dpad;
    a.n = src.n;
    a.B = Bs;
    flat_slice_plan(src.n, Bs, Q, &a.slices, &a.slice_tiles);
    a.stride = stride;
    uint64_t* part = nullptr;
    rc = graph_scan_inputs(g, ctx, slot, q_dev + (size_t)b0 * s->d, Bs, (size_t)(Bs * stride * 4), &a.queries, &part);
    if (rc) return rc;
    a.arena = (uint32_t*)part;
    if (a.slices)
      hipLaunchKernelGGL((s->f16() ? flat_score_kernel<Q, half_t> : flat_score_kernel<Q, float>), dim3(cdiv(Bs, Q), cdiv(a.slices, 4)),
                         dim3(256), 0, ctx->stream, a);
    FlatSelectArgs sel{};
    sel.arena = a.arena;
    sel.stride = stride;
    sel.n_words = (uint32_t)stride;  // n == 0: no word is read and every row comes out empty
    sel.k = k;
    sel.out_nodes = out_nodes_dev + (size_t)b0 * k;
    sel.out_dist = out_dist_dev + (size_t)b0 * k;
    sel.out_counts = out_counts_dev + b0;
    if (radius_dev)
      hipLaunchKernelGGL(range_flat_select_kernel, dim3(Bs), dim3(kWideSelThreads), 0, ctx->stream,
                         RangeFlatArgs{sel, radius_dev + b0, out_totals_dev + b0});
    else
      hipLaunchKernelGGL(flat_select_kernel, dim3(Bs), dim3(kWideSelThreads), 0, ctx->stream, sel);
    HIPCHK(ctx, hipGetLastError());
  }
  return FVDB_OK;
}

int fvdb_graph_search_flat_wide_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                         uint32_t k, uint32_t* out_nodes_dev, float* out_dist_dev, uint32_t* out_counts_dev) {
  GraphMaskSource src{};
  fvdb_ctx* ctx = nullptr;
  int rc = flat_check_args(g, on, slot, mask, k, FVDB_MAX_K_WIDE, "exact scan: k must be in 1..FVDB_MAX_K_WIDE",
                           q_dev && out_nodes_dev && out_dist_dev && out_counts_dev, &src, &ctx);
  if (rc) return rc;
  return flat_arena_search(g, ctx, src, slot, mask, q_dev, B, k, out_nodes_dev, out_dist_dev, out_counts_dev, nullptr, nullptr);
}

// ---- radius search ----
int fvdb_graph_search_flat_radius_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                           const float* radius_dev, uint32_t max_results, uint32_t* out_nodes_dev, float* out_dist_dev,
                                           uint32_t* out_counts_dev, uint32_t* out_totals_dev) {
  GraphMaskSource src{};
  fvdb_ctx* ctx = nullptr;
  int rc = flat_check_args(g, on, slot, mask, max_results, FVDB_MAX_K_WIDE, "radius search: max_results must be in 1..FVDB_MAX_K_WIDE",
                           q_dev && radius_dev && out_nodes_dev && out_dist_dev && out_counts_dev && out_totals_dev, &src, &ctx);
  if (rc) return rc;
  return flat_arena_search(g, ctx, src, slot, mask, q_dev, B, max_results, out_nodes_dev, out_dist_dev, out_counts_dev, radius_dev,
                           out_totals_dev);
}

// The size of every ball and nothing else: no arena.  Sub-batches only bound the grid and the padded queries' scratch.
int fvdb_graph_count_within_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                     const float* radius_dev, uint32_t* out_totals_dev) {
  GraphMaskSource src{};
  fvdb_ctx* ctx = nullptr;
  int rc = flat_check_args(g, on, slot, mask, 1, 1, "", q_dev && radius_dev && out_totals_dev, &src, &ctx);
  if (rc) return rc;
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  fvdb_store* s = src.store;
  constexpr uint32_t Q = kFlatWideQ;
  HIPCHK(ctx, hipMemsetAsync(out_totals_dev, 0, (size_t)B * 4, ctx->stream));
  for (uint32_t b0 = 0; b0 < B; b0 += kFlatSubBatch) {
    const uint32_t Bs = std::min(kFlatSubBatch, B - b0);
    FlatCountArgs a{};
    a.rows = s->data;
    a.dead = mask ? mask->flags.as<uint32_t>() : src.deleted;
    a.dpad = s->dpad;
    a.n = src.n;
    a.B = Bs;
    flat_slice_plan(src.n, Bs, Q, &a.slices, &a.slice_tiles);
    uint64_t* part = nullptr;
    rc = graph_scan_inputs(g, ctx, slot, q_dev + (size_t)b0 * s->d, Bs, 0, &a.queries, &part);
    if (rc) return rc;
    a.radius = radius_dev + b0;
    a.counts = out_totals_dev + b0;
    if (a.slices)
      hipLaunchKernelGGL((s->f16() ? flat_count_kernel<Q, half_t> : flat_count_kernel<Q, float>), dim3(cdiv(Bs, Q), cdiv(a.slices, 4)),
                         dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
  }
  return FVDB_OK;
}

int fvdb_search_quality_lists_dev(fvdb_ctx* ctx, const uint64_t* res_ids_dev, const uint32_t* res_counts_dev,
                                  const uint64_t* truth_ids_dev, const uint32_t* truth_counts_dev, uint32_t B, uint32_t k,
                                  float* out_recall_dev, float* out_precision_dev) {
  if (!ctx) return FVDB_E_INVALID;
  if (!res_ids_dev || !res_counts_dev || !truth_ids_dev || !truth_counts_dev || !out_recall_dev || !out_precision_dev)
    FAIL(ctx, FVDB_E_INVALID, "null buffer");
  if (k == 0) FAIL(ctx, FVDB_E_UNSUPPORTED, "k must be > 0");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(search_quality_kernel, dim3(cdiv(B, 4)), dim3(256), 0, ctx->stream, res_ids_dev, res_counts_dev, truth_ids_dev,
                     truth_counts_dev, B, k, out_recall_dev, out_precision_dev);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// kernels_grid.h: the flags of every list against the truth, then one lane per (ef, n_probe, query).  The lists'
// prefix counts live in the context's own scratch: calls on one context take turns here and run in stream order.
int fvdb_quality_grid_dev(fvdb_ctx* ctx, const uint64_t* truth_ids_dev, const uint32_t* truth_counts_dev,
                          const uint64_t* recent_ids_dev, const float* recent_dist_dev, const uint32_t* recent_counts_dev,
                          const uint64_t* hist_ids_dev, const float* hist_dist_dev, const uint32_t* hist_counts_dev, uint32_t B,
                          uint32_t k, uint32_t rk, uint32_t hk, uint32_t E, uint32_t P, float* out_recall_dev,
                          float* out_precision_dev) {
  if (!ctx) return FVDB_E_INVALID;
  if (!truth_ids_dev || !truth_counts_dev || !out_recall_dev || !out_precision_dev) FAIL(ctx, FVDB_E_INVALID, "null buffer");
  if (E == 0 && P == 0) FAIL(ctx, FVDB_E_INVALID, "quality grid: no recent and no historical lists");
  if (E && (!recent_ids_dev || !recent_dist_dev || !recent_counts_dev)) FAIL(ctx, FVDB_E_INVALID, "null recent block");
  if (P && (!hist_ids_dev || !hist_dist_dev || !hist_counts_dev)) FAIL(ctx, FVDB_E_INVALID, "null historical block");
  if (E > kGridMaxPoints || P > kGridMaxPoints) FAIL(ctx, FVDB_E_UNSUPPORTED, "quality grid: at most 64 ef and 64 n_probe values");
  if (k == 0 || k > FVDB_MAX_K_WIDE) FAIL(ctx, FVDB_E_UNSUPPORTED, "quality grid: k must be in 1..FVDB_MAX_K_WIDE");
  if (E && (rk == 0 || rk > FVDB_MAX_K_WIDE)) FAIL(ctx, FVDB_E_UNSUPPORTED, "quality grid: recent k must be in 1..FVDB_MAX_K_WIDE");
  if (P && (hk == 0 || hk > FVDB_MAX_K_WIDE)) FAIL(ctx, FVDB_E_UNSUPPORTED, "quality grid: historical k must be in 1..FVDB_MAX_K_WIDE");
  if (B == 0) return FVDB_OK;
  const uint64_t pairs = (uint64_t)std::max(E, 1u) * std::max(P, 1u) * B;
  if (B > 0x7FFFFFFFu || pairs > (1ull << 38)) FAIL(ctx, FVDB_E_UNSUPPORTED, "quality grid: batch too large for one call");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t g_words = (size_t)E * B * (rk + 1), h_words = (size_t)P * B * (hk + 1);
  std::lock_guard<std::mutex> lk(ctx->grid_mu);  // both kernels are on the stream before another call may grow the block
  HIPCHK(ctx, ctx->s_grid.ensure((g_words + h_words) * 4));
  GridArgs a{};
  a.t_ids = truth_ids_dev;
  a.t_cnt = truth_counts_dev;
  a.g_ids = E ? recent_ids_dev : nullptr;
  a.g_dist = E ? recent_dist_dev : nullptr;
  a.g_cnt = E ? recent_counts_dev : nullptr;
  a.h_ids = P ? hist_ids_dev : nullptr;
  a.h_dist = P ? hist_dist_dev : nullptr;
  a.h_cnt = P ? hist_counts_dev : nullptr;
  a.B = B, a.k = k, a.rk = rk, a.hk = hk, a.E = E, a.P = P;
  a.g_pfx = ctx->s_grid.as<uint32_t>();
  a.h_pfx = a.g_pfx + g_words;
  a.recall = out_recall_dev;
  a.precision = out_precision_dev;
  hipLaunchKernelGGL(grid_flags_kernel, dim3(B), dim3(kGridThreads), 0, ctx->stream, a);
  hipLaunchKernelGGL(grid_pairs_kernel, dim3(cdiv(pairs, 256)), dim3(256), 0, ctx->stream, a);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

}  // extern "C"
