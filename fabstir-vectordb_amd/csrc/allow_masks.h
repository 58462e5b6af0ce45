// allow_masks.h — allow-set masks of the C ABI (include/fvdb.h, "filtered search"): building a mask for an IVF index
// or a graph, and the exact scan of a graph's allowed nodes.  Included at the end of fvdb_hip.cpp.  The masked searches
// themselves live beside the searches they extend (fvdb_hip.cpp, fvdb_graph.cpp): the same code, handed the mask's
// words / flags instead of the index's.
#pragma once
#include "kernels_allow.h"

namespace {

// a device buffer of this call only, filled from the host
int upload_temp(fvdb_ctx* ctx, DBuf& t, const void* host, size_t bytes) {
  HIPCHK(ctx, t.exact(std::max<size_t>(bytes, 8)));
  if (bytes) HIPCHK(ctx, hipMemcpyAsync(t.p, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  return FVDB_OK;
}

struct IvfMaskSource {
  fvdb_ctx* ctx;
  const uint64_t* ids;    // [blocks][64]
  const uint64_t* valid;  // [blocks]
  uint32_t blocks;
};

int build_ivf_mask(fvdb_mask* m, const IvfMaskSource& src, const uint64_t* ids, uint64_t n) {
  fvdb_ctx* ctx = src.ctx;
  m->units = src.blocks;
  HIPCHK(ctx, m->words.ensure(std::max<size_t>((size_t)src.blocks * 8, 8)));
  if (src.blocks == 0) return FVDB_OK;
  if (n == 0) {  // nothing is allowed
    HIPCHK(ctx, hipMemsetAsync(m->words.p, 0, (size_t)src.blocks * 8, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FVDB_OK;
  }
  uint64_t slots = 1024;
  while (slots < 2 * n) slots <<= 1;
  if (slots > (1ull << 31)) FAIL(ctx, FVDB_E_UNSUPPORTED, "allow-set of more than 2^30 ids");
  DBuf d_ids, d_table, d_count;
  int rc = upload_temp(ctx, d_ids, ids, (size_t)n * 8);
  if (rc) return rc;
  HIPCHK(ctx, d_table.exact((size_t)slots * 8));
  HIPCHK(ctx, d_count.exact(8));
  HIPCHK(ctx, hipMemsetAsync(d_table.p, 0xFF, (size_t)slots * 8, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_count.p, 0, 8, ctx->stream));
  hipLaunchKernelGGL(allow_set_build_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, (const uint64_t*)d_ids.p, n,
                     (unsigned long long*)d_table.p, (uint32_t)(slots - 1));
  hipLaunchKernelGGL(allow_pool_words_kernel, dim3(cdiv(src.blocks, 4)), dim3(256), 0, ctx->stream, src.ids, src.valid, src.blocks,
                     (const unsigned long long*)d_table.p, (uint32_t)(slots - 1), m->words.as<uint64_t>(),
                     (unsigned long long*)d_count.p);
  HIPCHK(ctx, hipGetLastError());
  unsigned long long count = 0;
  HIPCHK(ctx, hipMemcpyAsync(&count, d_count.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  m->allowed_live = count;
  return FVDB_OK;
}

int build_graph_mask(fvdb_mask* m, const GraphMaskSource& src, const uint32_t* nodes, uint64_t n_in) {
  fvdb_ctx* ctx = src.store->ctx;
  const uint32_t n = src.n;
  m->units = n;
  HIPCHK(ctx, m->flags.ensure(std::max<size_t>((size_t)n * 4, 4)));
  HIPCHK(ctx, m->nodes.ensure(std::max<size_t>((size_t)std::min<uint64_t>(n, n_in) * 4, 4)));
  if (n == 0) return FVDB_OK;
  const uint32_t n_wg = cdiv(n, 256);
  DBuf d_in, d_wg, d_total;
  int rc = upload_temp(ctx, d_in, nodes, (size_t)n_in * 4);
  if (rc) return rc;
  HIPCHK(ctx, d_wg.exact((size_t)n_wg * 4));
  HIPCHK(ctx, d_total.exact(8));
  HIPCHK(ctx, hipMemsetAsync(m->flags.p, 0x01, (size_t)n * 4, ctx->stream));  // every word non-zero: not allowed
  if (n_in)
    hipLaunchKernelGGL(allow_graph_mark_kernel, dim3(cdiv(n_in, 256)), dim3(256), 0, ctx->stream, (const uint32_t*)d_in.p, n_in, n,
                       m->flags.as<uint32_t>());
  hipLaunchKernelGGL(allow_graph_count_kernel, dim3(n_wg), dim3(256), 0, ctx->stream, m->flags.as<uint32_t>(), src.deleted, n,
                     (uint32_t*)d_wg.p);
  hipLaunchKernelGGL(block_excl_scan_kernel<unsigned long long>, dim3(1), dim3(1024), 0, ctx->stream, (uint32_t*)d_wg.p, n_wg,
                     (unsigned long long*)d_total.p);
  hipLaunchKernelGGL(allow_graph_write_kernel, dim3(n_wg), dim3(256), 0, ctx->stream, m->flags.as<uint32_t>(), n,
                     (const uint32_t*)d_wg.p, m->nodes.as<uint32_t>());
  HIPCHK(ctx, hipGetLastError());
  unsigned long long total = 0;
  HIPCHK(ctx, hipMemcpyAsync(&total, d_total.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  m->allowed_live = total;
  return FVDB_OK;
}

template <int KR, bool GR = false>
void launch_allow_scan(fvdb_ctx* ctx, const AllowScanArgs& a, bool f16 /* the store's rows */, uint32_t* out_nodes, float* out_dist, uint32_t* out_counts) {
  if (a.slices)
    hipLaunchKernelGGL((f16 ? allow_scan_kernel<KR, half_t, GR> : allow_scan_kernel<KR, float, GR>), dim3(cdiv(a.B, 4), a.slices), dim3(256), 0,
                       ctx->stream, a);
  hipLaunchKernelGGL((allow_merge_kernel<KR, GR>), dim3(cdiv(a.B, 4)), dim3(256), 0, ctx->stream, a.part, a.nodes, a.slices, a.B, a.k,
                     out_nodes, out_dist, out_counts, a.groups, a.group);
}

// the slices of a scan whose longest node list has n_nodes entries: enough (query, slice) waves to fill the device, a
// slice no shorter than four rounds of 64
void allow_scan_slices(AllowScanArgs& a, uint32_t n_nodes) {
  a.slices = n_nodes ? std::max<uint32_t>(1, std::min<uint32_t>(cdiv(n_nodes, 256), cdiv(8192, a.B))) : 0;
  a.slice_len = a.slices ? cdiv(n_nodes, a.slices) : 0;
  if (a.slices) a.slices = cdiv(n_nodes, a.slice_len);
}

}  // namespace

extern "C" {

int fvdb_mask_create_ivf(fvdb_ivf* ivf, const uint64_t* ids, uint64_t n, fvdb_mask** out) {
  if (!ivf || !out) return FVDB_E_INVALID;
  *out = nullptr;
  const IvfMaskSource src{ivf->ctx, ivf->pool.ids(), ivf->pool.valid(), ivf->pool.used_blocks};
  int rc;
  if (n && !ids) FAIL(src.ctx, FVDB_E_INVALID, "allow-set: null ids");
  HIPCHK(src.ctx, hipSetDevice(src.ctx->device));
  fvdb_mask* m = new (std::nothrow) fvdb_mask();
  if (!m) return FVDB_E_OOM;
  m->ctx = src.ctx;
  m->ivf = ivf;
  m->stamp = ivf->mutations;
  rc = build_ivf_mask(m, src, ids, n);
  if (rc) {
    fvdb_mask_destroy(m);
    return rc;
  }
  *out = m;
  return FVDB_OK;
}

int fvdb_mask_create_graph(fvdb_graph* g, const uint32_t* nodes, uint64_t n, fvdb_mask** out) {
  if (!g || !out) return FVDB_E_INVALID;
  *out = nullptr;
  GraphMaskSource src{};
  int rc = graph_mask_source(g, &src);
  if (rc) return rc;
  fvdb_ctx* ctx = src.store->ctx;
  if (n && !nodes) FAIL(ctx, FVDB_E_INVALID, "allow-set: null node list");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  fvdb_mask* m = new (std::nothrow) fvdb_mask();
  if (!m) return FVDB_E_OOM;
  m->ctx = ctx;
  m->graph = g;
  m->stamp = src.mutations;
  rc = build_graph_mask(m, src, nodes, n);
  if (rc) {
    fvdb_mask_destroy(m);
    return rc;
  }
  *out = m;
  return FVDB_OK;
}

int fvdb_mask_info(fvdb_mask* m, fvdb_mask_info_t* out) {
  if (!m || !out) return FVDB_E_INVALID;
  out->kind = m->ivf ? 1u : 2u;
  out->reserved = 0;
  out->units = m->units;
  out->allowed_live = m->allowed_live;
  uint64_t now = 0;
  if (m->ivf) {
    now = m->ivf->mutations;
  } else {
    GraphMaskSource src{};
    if (graph_mask_source(m->graph, &src) == FVDB_OK) now = src.mutations;
  }
  out->stale = now != m->stamp ? 1u : 0u;
  return FVDB_OK;
}

void fvdb_mask_destroy(fvdb_mask* m) {
  if (!m) return;
  (void)hipSetDevice(m->ctx->device);
  (void)hipDeviceSynchronize();  // searches in any slot may still be reading it
  delete m;
}

int fvdb_graph_scan_allowed_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                     uint32_t k, uint32_t* out_nodes_dev, float* out_dist_dev, uint32_t* out_counts_dev) {
  if (!g) return FVDB_E_INVALID;
  GraphMaskSource src{};
  int rc = graph_mask_source(g, &src);
  if (rc) return rc;
  fvdb_store* s = src.store;
  fvdb_ctx* ctx = on ? on : s->ctx;
  if (slot >= kGraphSlots) FAIL(ctx, FVDB_E_INVALID, "slot out of range");
  if (on && on->device != s->ctx->device) FAIL(ctx, FVDB_E_INVALID, "context of another device");
  if (!mask || mask->graph != g) FAIL(ctx, FVDB_E_INVALID, "mask of another graph");
  if (mask->stamp != src.mutations) FAIL(ctx, FVDB_E_INVALID, "stale mask: the graph changed after the mask was created");
  if (k == 0 || k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "exact scan: k must be in 1..FVDB_MAX_K");
  if (!q_dev || !out_nodes_dev || !out_dist_dev || !out_counts_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint32_t n_nodes = (uint32_t)mask->allowed_live;
  AllowScanArgs a{};
  a.rows = s->data;
  a.nodes = mask->nodes.as<uint32_t>();
  a.dpad = s->dpad;
  a.n_nodes = n_nodes;
  a.B = B;
  a.k = k;
  allow_scan_slices(a, n_nodes);
  // the slot's scratch: the queries padded to the store's row stride where d is not a multiple of 4, the partial lists
  rc = graph_scan_inputs(g, ctx, slot, q_dev, B, (size_t)a.slices * B * k * 8, &a.queries, &a.part);
  if (rc) return rc;
  switch (k <= 64 ? 1 : (k <= 128 ? 2 : 4)) {
    case 1: launch_allow_scan<1>(ctx, a, s->f16(), out_nodes_dev, out_dist_dev, out_counts_dev); break;
    case 2: launch_allow_scan<2>(ctx, a, s->f16(), out_nodes_dev, out_dist_dev, out_counts_dev); break;
    default: launch_allow_scan<4>(ctx, a, s->f16(), out_nodes_dev, out_dist_dev, out_counts_dev); break;
  }
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// The same scan, each query over the node list of its own mask.
int fvdb_graph_scan_allowed_groups_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* const* masks, uint32_t G,
                                            const uint32_t* group_of_query, const float* q_dev, uint32_t B, uint32_t k,
                                            uint32_t* out_nodes_dev, float* out_dist_dev, uint32_t* out_counts_dev) {
  if (!g) return FVDB_E_INVALID;
  GraphMaskSource src{};
  int rc = graph_mask_source(g, &src);
  if (rc) return rc;
  fvdb_store* s = src.store;
  fvdb_ctx* ctx = on ? on : s->ctx;
  if (slot >= kGraphSlots) FAIL(ctx, FVDB_E_INVALID, "slot out of range");
  if (on && on->device != s->ctx->device) FAIL(ctx, FVDB_E_INVALID, "context of another device");
  if (G && !masks) FAIL(ctx, FVDB_E_INVALID, "null mask table");
  if (B && !group_of_query) FAIL(ctx, FVDB_E_INVALID, "null group array");
  if (B && G == 0) FAIL(ctx, FVDB_E_INVALID, "queries but no group");
  // every mask, named by a query or not, before anything is enqueued
  std::vector<AllowGroup> groups(G);
  uint32_t longest = 0;
  for (uint32_t i = 0; i < G; ++i) {
    const fvdb_mask* m = masks[i];
    if (!m || m->graph != g) FAIL(ctx, FVDB_E_INVALID, "mask of another graph");
    if (m->stamp != src.mutations) FAIL(ctx, FVDB_E_INVALID, "stale mask: the graph changed after the mask was created");
    groups[i] = AllowGroup{m->nodes.as<uint32_t>(), (uint32_t)m->allowed_live, 0u};
    longest = std::max(longest, groups[i].n_nodes);
  }
  for (uint32_t b = 0; b < B; ++b)
    if (group_of_query[b] >= G) FAIL(ctx, FVDB_E_INVALID, "group index out of range");
  if (k == 0 || k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "exact scan: k must be in 1..FVDB_MAX_K");
  if (!q_dev || !out_nodes_dev || !out_dist_dev || !out_counts_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  AllowScanArgs a{};
  a.rows = s->data;
  a.dpad = s->dpad;
  a.B = B;
  a.k = k;
  allow_scan_slices(a, longest);  // laid out for the longest list
  // the slot's scratch: padded queries, the partial lists, then the group table and the group of each query
  const size_t part_bytes = ((size_t)a.slices * B * k * 8 + 15) & ~(size_t)15;
  const size_t table_bytes = (size_t)G * sizeof(AllowGroup);
  rc = graph_scan_inputs(g, ctx, slot, q_dev, B, part_bytes + table_bytes + (size_t)B * 4, &a.queries, &a.part);
  if (rc) return rc;
  char* tail = (char*)a.part + part_bytes;
  HIPCHK(ctx, hipMemcpyAsync(tail, groups.data(), table_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(tail + table_bytes, group_of_query, (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the table and the caller's array are host memory of this call
  a.groups = (const AllowGroup*)tail;
  a.group = (const uint32_t*)(tail + table_bytes);
  switch (k <= 64 ? 1 : (k <= 128 ? 2 : 4)) {
    case 1: launch_allow_scan<1, true>(ctx, a, s->f16(), out_nodes_dev, out_dist_dev, out_counts_dev); break;
    case 2: launch_allow_scan<2, true>(ctx, a, s->f16(), out_nodes_dev, out_dist_dev, out_counts_dev); break;
    default: launch_allow_scan<4, true>(ctx, a, s->f16(), out_nodes_dev, out_dist_dev, out_counts_dev); break;
  }
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

}  // extern "C"
