// flat_mfma_search.h — the filtered exact search of the C ABI (include/fvdb.h, "exact search, filtered"; DESIGN.md
// section 9z): fvdb_graph_search_flat_dev_slot's answer by a matrix-core filter over an fp16 operand mirror of the
// graph's rows and an exact re-score of the survivors (kernels_flat_mfma.h).  Included by fvdb_hip.cpp after
// flat_search.h, whose argument checks and sub-batch size it shares.
#pragma once
#include <chrono>

#include "kernels_flat_mfma.h"

namespace {

constexpr uint32_t kFmMinSliceBlocks = 16;    // 512 rows: a shorter slice emits its first k rows for too little filtering
constexpr size_t kFmArenaBytes = 512u << 20;  // survivor arenas of one launch chain
constexpr uint32_t kFmMaxExactWaves = 32;     // exact-stage waves (and lists to merge) a query

uint32_t fm_lds_limit(fvdb_ctx* ctx) {
  int lds = 0;
  if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device) != hipSuccess) lds = 65536;
  return (uint32_t)lds;
}
// the query operands go to LDS when they fit beside the buffers of the k class, else they are read from HBM
bool fm_qlds(uint32_t kr, uint32_t ksteps, uint32_t lds_limit) { return flat_mfma_scan_lds(kr, ksteps, true) <= lds_limit; }

// Rows [0, n) of the store in the mirror on return: nothing to do, an extension by the rows appended since, or a whole
// build after a reset.  The kernels run on ctx's stream, which is waited for before the mirror is published: a search
// in another slot reads it from a stream of its own.
int fm_sync_mirror(fvdb_ctx* ctx, GraphFlatMirror* m, const fvdb_store* s, uint32_t n) {
  std::lock_guard<std::mutex> lk(m->mu);
  if (m->built >= n) return FVDB_OK;
  const uint32_t ksteps = cdiv(s->d, 16);
  const uint64_t blocks = cdiv(n, 32), old_blocks = cdiv(m->built, 32);
  const size_t wb = (size_t)ksteps * 1024;
  const auto t0 = std::chrono::steady_clock::now();
  if (!m->xmax.p) HIPCHK(ctx, m->xmax.exact(256));
  if (blocks > m->cap_blocks) {
    const uint64_t nb = std::max<uint64_t>(blocks, m->cap_blocks + m->cap_blocks / 2);
    HIPCHK(ctx, grow_keeping(m->ops, nb * wb, old_blocks * wb, /*zero_rest=*/false, ctx->stream));
    HIPCHK(ctx, grow_keeping(m->xn, nb * 32 * 4, m->built * 4, /*zero_rest=*/false, ctx->stream));
    m->cap_blocks = nb;
  }
  if (m->built == 0) {
    hipLaunchKernelGGL(flat_mfma_clear_kernel, dim3(1), dim3(64), 0, ctx->stream, m->xmax.as<uint32_t>(), (uint64_t)1);
    m->builds += 1;
  }
  FlatMirrorArgs a{};
  a.rows = s->data;
  a.d = s->d;
  a.dpad = s->dpad;
  a.ksteps = ksteps;
  a.first = m->built;
  a.n = n;
  a.n_pad = blocks * 32;
  a.ops = m->ops.as<uint4>();
  a.xn = m->xn.as<float>();
  a.xmax_bits = m->xmax.as<uint32_t>();
  hipLaunchKernelGGL((s->f16() ? flat_mfma_mirror_kernel<half_t> : flat_mfma_mirror_kernel<float>), dim3(cdiv(a.n_pad - a.first, 4)),
                     dim3(256), 0, ctx->stream, a);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  m->build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  m->build_rows = n - m->built;
  m->built = n;
  return FVDB_OK;
}

template <int KR, bool QLDS>
int fm_launch_scan(fvdb_ctx* ctx, const FlatMfmaScanArgs& a, uint32_t slices) {
  const uint32_t lds = flat_mfma_scan_lds(KR, a.ksteps, QLDS);
  // the attribute belongs to the function; every call sets what it needs
  HIPCHK(ctx, hipFuncSetAttribute((const void*)flat_mfma_scan_kernel<KR, QLDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((flat_mfma_scan_kernel<KR, QLDS>), dim3(cdiv(a.B, kFmTile), slices), dim3(256), lds, ctx->stream, a);
  return FVDB_OK;
}

// the scan, the two exact passes (n > 0), the merge
template <int KR, typename RT>
int fm_launch_chain(fvdb_ctx* ctx, bool qlds, const FlatMfmaScanArgs& s, uint32_t slices, const FlatMfmaExactArgs& e, uint32_t* out_nodes,
                    float* out_dist, uint32_t* out_counts) {
  if (e.n) {
    const int rc = qlds ? fm_launch_scan<KR, true>(ctx, s, slices) : fm_launch_scan<KR, false>(ctx, s, slices);
    if (rc) return rc;
    hipLaunchKernelGGL((flat_mfma_exact_kernel<KR, 0, RT>), dim3(cdiv(e.W, 4), e.B), dim3(256), 0, ctx->stream, e);
    hipLaunchKernelGGL((flat_mfma_exact_kernel<KR, 1, RT>), dim3(cdiv(e.W, 4), e.B), dim3(256), 0, ctx->stream, e);
  }
  hipLaunchKernelGGL((flat_merge_kernel<KR>), dim3(cdiv(e.B, 4)), dim3(256), 0, ctx->stream, e.part, e.n ? e.W : 0u, e.B, e.k, out_nodes,
                     out_dist, out_counts);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

size_t fm_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int fvdb_graph_search_flat_mfma_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                         uint32_t k, uint32_t* out_nodes_dev, float* out_dist_dev, uint32_t* out_counts_dev) {
  GraphMaskSource src{};
  fvdb_ctx* ctx = nullptr;
  int rc = flat_check_args(g, on, slot, mask, k, FVDB_MAX_K, "exact scan: k must be in 1..FVDB_MAX_K",
                           q_dev && out_nodes_dev && out_dist_dev && out_counts_dev, &src, &ctx);
  if (rc) return rc;
  fvdb_store* s = src.store;
  if (s->d > kFmMaxDims) FAIL(ctx, FVDB_E_UNSUPPORTED, "filtered exact scan: d must be <= 2048");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  GraphFlatMirror* m = graph_flat_mirror(g);
  const uint32_t n = src.n, blocks = cdiv(n, 32), ksteps = cdiv(s->d, 16);
  if (n && (rc = fm_sync_mirror(ctx, m, s, n))) return rc;
  const uint32_t kr = k <= 64 ? 1 : (k <= 128 ? 2 : 4);
  // Enough (tile, slice) workgroups to fill the device at a small batch, no slice under kFmMinSliceBlocks.  Every slice
  // emits its first k rows and then what passes its own running threshold: the arena holds four times 2 k + 64 rows a
  // slice, and never needs more than n.
  uint32_t slice_blocks = 0, slices = 0, cap = 1;
  if (n) {
    const uint32_t tiles = cdiv(std::min(B, kFlatSubBatch), kFmTile);
    const uint32_t want = std::max<uint32_t>(1, std::min<uint32_t>(cdiv(blocks, kFmMinSliceBlocks), cdiv(4 * (uint32_t)ctx->num_cus, tiles)));
    slice_blocks = (cdiv(blocks, want) + 3u) & ~3u;  // whole rounds
    slices = cdiv(blocks, slice_blocks);
    cap = (uint32_t)std::min<uint64_t>(n, (uint64_t)slices * 4u * (2u * k + 64u));
  }
  const uint32_t sub = std::max<uint32_t>(32, (uint32_t)std::min<size_t>(kFlatSubBatch, kFmArenaBytes / ((size_t)cap * 4)) & ~31u);
  const bool qlds = fm_qlds(kr, ksteps, fm_lds_limit(ctx));
  DBuf& ctr_buf = m->ctr[slot];
  HIPCHK(ctx, ctr_buf.ensure(16));
  uint32_t* ctr = ctr_buf.as<uint32_t>();  // pairs (two words), fallbacks, unbounded
  hipLaunchKernelGGL(flat_mfma_clear_kernel, dim3(1), dim3(64), 0, ctx->stream, ctr, (uint64_t)4);
  // sub-batches run one after the other on the stream and share the slot's scratch
  for (uint32_t b0 = 0; b0 < B; b0 += sub) {
    const uint32_t Bs = std::min(sub, B - b0), tiles = cdiv(Bs, kFmTile);
    const uint32_t W = std::max<uint32_t>(1, std::min<uint32_t>(kFmMaxExactWaves, cdiv(16 * (uint32_t)ctx->num_cus, Bs)));
    // the slot's scratch behind the padded queries: partial lists, query operands, margins, arena counts, flags, arenas
    const size_t o_qops = fm_align((size_t)W * Bs * k * 8), o_mar = o_qops + fm_align((size_t)tiles * ksteps * 1024);
    const size_t o_cnt = o_mar + fm_align((size_t)Bs * 4), o_arena = o_cnt + fm_align((size_t)Bs * 8);
    const float* queries = nullptr;
    uint64_t* part = nullptr;
    rc = graph_scan_inputs(g, ctx, slot, q_dev + (size_t)b0 * s->d, Bs, o_arena + (size_t)Bs * cap * 4, &queries, &part);
    if (rc) return rc;
    char* base = (char*)part;
    uint32_t* arena_cnt = (uint32_t*)(base + o_cnt);
    hipLaunchKernelGGL(flat_mfma_clear_kernel, dim3(cdiv(2ull * Bs, 256)), dim3(256), 0, ctx->stream, arena_cnt, 2ull * Bs);

    FlatMfmaQueryArgs p{};
    p.queries = queries;
    p.d = s->d;
    p.dpad = s->dpad;
    p.ksteps = ksteps;
    p.B = Bs;
    p.B_pad = tiles * kFmTile;
    p.xmax_bits = m->xmax.as<uint32_t>();
    p.x_rounded = s->f16() ? 0 : 1;
    p.qops = (uint4*)(base + o_qops);
    p.margin = (float*)(base + o_mar);
    p.flags = arena_cnt + Bs;
    p.unbounded = ctr + 3;
    if (n) hipLaunchKernelGGL(flat_mfma_query_kernel, dim3(cdiv(p.B_pad, 4)), dim3(256), 0, ctx->stream, p);

    FlatMfmaScanArgs sc{};
    sc.ops = m->ops.as<uint4>();
    sc.xn = m->xn.as<float>();
    sc.dead = mask ? mask->flags.as<uint32_t>() : src.deleted;
    sc.qops = p.qops;
    sc.margin = p.margin;
    sc.arena = (uint32_t*)(base + o_arena);
    sc.arena_cnt = arena_cnt;
    sc.flags = p.flags;
    sc.n = n;
    sc.ksteps = ksteps;
    sc.B = Bs;
    sc.k = k;
    sc.cap = cap;
    sc.slice_blocks = slice_blocks;

    FlatMfmaExactArgs e{};
    e.rows = s->data;
    e.queries = queries;
    e.dead = sc.dead;
    e.arena = sc.arena;
    e.arena_cnt = arena_cnt;
    e.flags = p.flags;
    e.part = part;
    e.pairs = (unsigned long long*)ctr;
    e.fallbacks = ctr + 2;
    e.n = n;
    e.dpad = s->dpad;
    e.B = Bs;
    e.k = k;
    e.cap = cap;
    e.W = W;

    uint32_t* on_ = out_nodes_dev + (size_t)b0 * k;
    float* od_ = out_dist_dev + (size_t)b0 * k;
    uint32_t* oc_ = out_counts_dev + b0;
    const bool f16 = s->f16();
    switch (kr) {
      case 1: rc = f16 ? fm_launch_chain<1, half_t>(ctx, qlds, sc, slices, e, on_, od_, oc_) : fm_launch_chain<1, float>(ctx, qlds, sc, slices, e, on_, od_, oc_); break;
      case 2: rc = f16 ? fm_launch_chain<2, half_t>(ctx, qlds, sc, slices, e, on_, od_, oc_) : fm_launch_chain<2, float>(ctx, qlds, sc, slices, e, on_, od_, oc_); break;
      default: rc = f16 ? fm_launch_chain<4, half_t>(ctx, qlds, sc, slices, e, on_, od_, oc_) : fm_launch_chain<4, float>(ctx, qlds, sc, slices, e, on_, od_, oc_); break;
    }
    if (rc) return rc;
  }
  {
    std::lock_guard<std::mutex> lk(m->mu);
    m->last_slot = slot;
    m->searched = true;
  }
  return FVDB_OK;
}

int fvdb_graph_flat_mfma_info(fvdb_graph* g, fvdb_flat_mfma_info* out) {
  if (!g || !out) return FVDB_E_INVALID;
  GraphMaskSource src{};
  int rc = graph_mask_source(g, &src);
  if (rc) return rc;
  fvdb_ctx* ctx = src.store->ctx;
  GraphFlatMirror* m = graph_flat_mirror(g);
  memset(out, 0, sizeof(*out));
  const uint32_t ksteps = cdiv(src.store->d, 16);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> lk(m->mu);
  out->mirror_rows = m->built;
  out->mirror_bytes = m->built ? (uint64_t)cdiv(m->built, 32) * ksteps * 1024 + m->built * 4 : 0;
  out->rebuilds = m->builds ? m->builds - 1 : 0;
  out->build_rows = m->build_rows;
  out->build_ms = m->build_ms;
  out->block_rows = kFmTile;
  out->queries_per_workgroup = kFmTile;
  out->round_rows = kFmRoundRows;
  out->words_in_flight = kFmAhead;
  out->min_slice_rows = kFmMinSliceBlocks * kFmTile;
  out->lds_limit = fm_lds_limit(ctx);
  const uint32_t krs[3] = {1, 2, 4};
  for (int i = 0; i < 3; ++i) {
    out->queries_in_lds[i] = fm_qlds(krs[i], ksteps, out->lds_limit);
    out->lds_bytes[i] = flat_mfma_scan_lds(krs[i], ksteps, out->queries_in_lds[i] != 0);
  }
  out->max_d = kFmMaxDims;
  out->max_k = FVDB_MAX_K;
  if (m->searched) {  // the counters of the last search, wherever it was enqueued
    HIPCHK(ctx, hipDeviceSynchronize());
    uint32_t w[4];
    HIPCHK(ctx, hipMemcpy(w, m->ctr[m->last_slot].p, 16, hipMemcpyDeviceToHost));
    out->exact_pairs = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    out->fallback_queries = w[2];
    out->unbounded_queries = w[3];
  }
  return FVDB_OK;
}

}  // extern "C"
