// fvdb_cos.cpp — cosine k-NN search and batch_normalize behind the C ABI (include/fvdb.h, "cosine search"; DESIGN.md
// section 9y).  A translation unit of its own: the kernels are kernels_cos.h; WaveTopK, the scalar-path loads and the
// tile fences come from their headers unchanged.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "fvdb_internal.h"
#include "common.h"
#include "kernels_cos.h"

using namespace fvdb;

namespace {

constexpr uint32_t kCosSlots = 16;
constexpr uint32_t kCosSubBatch = 8192;        // queries of one launch chain, a multiple of the 32-query tile
constexpr uint32_t kCosMinSliceBlocks = 16;    // 512 rows: a shorter slice emits its first k rows for too little filtering
constexpr size_t kCosArenaBytes = 512u << 20;  // survivor arenas of one launch chain
constexpr uint32_t kCosMaxExactWaves = 32;     // exact-stage waves (and lists to merge) a query

// What add and the host search refuse before anything is written: a non-finite element or a sum of squares that
// overflows (FVDB_E_NONFINITE), and a magnitude, by the reference's fold, that is neither zero nor inside the window
// DESIGN 9y's bound assumes (FVDB_E_UNSUPPORTED).
int cos_check_rows(fvdb_ctx* ctx, const float* x, uint64_t n, uint32_t d) {
  for (uint64_t r = 0; r < n; ++r) {
    const float* row = x + r * d;
    float s = 0.0f;
    for (uint32_t i = 0; i < d; ++i) {
      if (!std::isfinite(row[i])) FAIL(ctx, FVDB_E_NONFINITE, "non-finite input value");
      s = s + row[i] * row[i];
    }
    if (!std::isfinite(s)) FAIL(ctx, FVDB_E_NONFINITE, "a row's sum of squares overflows f32");
    const float m = std::sqrt(s);
    if (m != 0.0f && (m < kCosMagMin || m > kCosMagMax))
      FAIL(ctx, FVDB_E_UNSUPPORTED, "cosine search: a magnitude must be 0 or within [2^-40, 2^40]");
  }
  return FVDB_OK;
}

// host memory to the device on the stream, complete on return (the source may be pageable and short-lived)
hipError_t upload(fvdb_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!bytes) return hipSuccess;
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream);
  return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
}
hipError_t download(fvdb_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!bytes) return hipSuccess;
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
  return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
}

int check_dims(fvdb_ctx* ctx, uint32_t d) {
  if (d == 0) FAIL(ctx, FVDB_E_INVALID, "d must be > 0");
  if (d > kCosMaxDims) FAIL(ctx, FVDB_E_UNSUPPORTED, "cosine search: d must be <= 2048");
  return FVDB_OK;
}

void launch_prepare(fvdb_ctx* on, const CosPrepArgs& a) {
  hipLaunchKernelGGL(cos_prepare_kernel, dim3(cdiv(a.n_pad, 4)), dim3(256), 0, on->stream, a);
}

}  // namespace

struct CosSlot {
  DBuf q, qops, qmag, qpad, ctr, arena, part, dead, out;
};

struct fvdb_cos_index {
  fvdb_ctx* ctx = nullptr;
  uint32_t d = 0, ksteps = 0, dpad = 0, dq = 0, lds_limit = 0, last_slot = 0;
  bool searched = false;
  DBuf rows, mag, ops, ids, dead, s_in, s_rows;
  uint64_t n = 0, cap_blocks = 0, live = 0;
  std::unordered_map<uint64_t, uint32_t> row_of;
  std::vector<uint8_t> h_dead;
  CosSlot slots[kCosSlots];
  // the query operands go to LDS when they fit beside the buffers of the k class, else they are read from HBM
  bool qlds(uint32_t kr) const { return cos_scan_lds(kr, ksteps, true) <= lds_limit; }
};

namespace {

template <int KR, bool QLDS>
int launch_scan(fvdb_ctx* on, const CosScanArgs& a, uint32_t slices) {
  const uint32_t lds = cos_scan_lds(KR, a.ksteps, QLDS);
  // the attribute belongs to the function; every call sets what it needs
  HIPCHK(on, hipFuncSetAttribute((const void*)cos_scan_kernel<KR, QLDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((cos_scan_kernel<KR, QLDS>), dim3(cdiv(a.B, kCosTile), slices), dim3(256), lds, on->stream, a);
  return FVDB_OK;
}

// scan (filter mode, n > 0), the two exact passes, the merge
template <int KR>
int launch_chain(fvdb_ctx* on, bool qlds, bool filter, const CosScanArgs& s, uint32_t slices, const CosExactArgs& e, const uint64_t* ids,
                 uint64_t* out_ids, float* out_sim, uint32_t* out_counts) {
  if (e.n) {
    if (filter) {
      const int rc = qlds ? launch_scan<KR, true>(on, s, slices) : launch_scan<KR, false>(on, s, slices);
      if (rc) return rc;
      hipLaunchKernelGGL((cos_exact_kernel<KR, 0>), dim3(cdiv(e.W, 4), e.B), dim3(256), 0, on->stream, e);
    }
    hipLaunchKernelGGL((cos_exact_kernel<KR, 1>), dim3(cdiv(e.W, 4), e.B), dim3(256), 0, on->stream, e);
  }
  hipLaunchKernelGGL((cos_merge_kernel<KR>), dim3(cdiv(e.B, 4)), dim3(256), 0, on->stream, e.part, e.n ? e.W : 0u, e.B, e.k, ids, out_ids, out_sim,
                     out_counts);
  HIPCHK(on, hipGetLastError());
  return FVDB_OK;
}

int check_search(fvdb_ctx* ctx, uint32_t k, int mode) {
  if (k == 0 || k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "cosine search: k must be in 1..FVDB_MAX_K");
  if (mode != FVDB_COS_FILTER && mode != FVDB_COS_EXACT) FAIL(ctx, FVDB_E_INVALID, "mode must be FVDB_COS_FILTER or FVDB_COS_EXACT");
  return FVDB_OK;
}

}  // namespace

extern "C" {

// ---- batch_normalize -------------------------------------------------------------------------------------------------
int fvdb_batch_normalize_dev(fvdb_ctx* ctx, const float* rows_dev, uint64_t n, uint32_t d, float* out_dev) {
  if (!ctx) return FVDB_E_INVALID;
  if (d == 0) FAIL(ctx, FVDB_E_INVALID, "d must be > 0");
  if (n == 0) return FVDB_OK;
  if (!rows_dev || !out_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "a call is limited to 2^32-1 rows");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  CosPrepArgs a{};
  a.rows = rows_dev;
  a.d = d;
  a.n = a.n_pad = n;
  a.unit = out_dev;
  launch_prepare(ctx, a);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int fvdb_batch_normalize(fvdb_ctx* ctx, const float* rows, uint64_t n, uint32_t d, float* out) {
  if (!ctx) return FVDB_E_INVALID;
  if (d == 0) FAIL(ctx, FVDB_E_INVALID, "d must be > 0");
  if (n == 0) return FVDB_OK;
  if (!rows || !out) FAIL(ctx, FVDB_E_INVALID, "null argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DBuf in, res;
  HIPCHK(ctx, in.exact(n * d * 4));
  HIPCHK(ctx, res.exact(n * d * 4));
  HIPCHK(ctx, upload(ctx, in.p, rows, n * d * 4));
  const int rc = fvdb_batch_normalize_dev(ctx, in.as<float>(), n, d, res.as<float>());
  if (rc) return rc;
  HIPCHK(ctx, download(ctx, out, res.p, n * d * 4));
  return FVDB_OK;
}

// ---- the index -------------------------------------------------------------------------------------------------------
int fvdb_cos_index_create(fvdb_ctx* ctx, uint32_t d, fvdb_cos_index** out) {
  if (!ctx || !out) return FVDB_E_INVALID;
  *out = nullptr;
  const int rc = check_dims(ctx, d);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int lds = 0;
  HIPCHK(ctx, hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  fvdb_cos_index* ix = new (std::nothrow) fvdb_cos_index();
  if (!ix) return FVDB_E_OOM;
  ix->ctx = ctx;
  ix->d = d;
  ix->ksteps = (d + 15u) / 16u;
  ix->dpad = (d + 3u) & ~3u;
  ix->dq = (d + 31u) & ~31u;
  ix->lds_limit = (uint32_t)lds;
  *out = ix;
  return FVDB_OK;
}

void fvdb_cos_index_destroy(fvdb_cos_index* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->ctx->device);
  (void)hipDeviceSynchronize();  // searches may be in flight on other contexts' streams
  delete ix;
}

uint64_t fvdb_cos_index_rows(fvdb_cos_index* ix) { return ix ? ix->n : 0; }
uint64_t fvdb_cos_index_live(fvdb_cos_index* ix) { return ix ? ix->live : 0; }
uint64_t fvdb_cos_index_bytes(fvdb_cos_index* ix) {
  if (!ix) return 0;
  return (uint64_t)cdiv(ix->n, 32) * ix->ksteps * 1024 + ix->n * ((uint64_t)ix->dpad * 4 + 16);
}

int fvdb_cos_index_info(fvdb_cos_index* ix, fvdb_cos_info_t* out) {
  if (!ix || !out) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->ctx;
  memset(out, 0, sizeof(*out));
  out->d = ix->d;
  out->d_padded = ix->ksteps * 16;
  out->block_rows = kCosTile;
  out->queries_per_workgroup = kCosTile;
  out->round_rows = kCosRoundRows;
  out->words_in_flight = kCosAhead;
  out->min_slice_rows = kCosMinSliceBlocks * kCosTile;
  out->lds_limit = ix->lds_limit;
  const uint32_t krs[3] = {1, 2, 4};
  for (int i = 0; i < 3; ++i) {
    out->queries_in_lds[i] = ix->qlds(krs[i]);
    out->lds_bytes[i] = cos_scan_lds(krs[i], ix->ksteps, ix->qlds(krs[i]));
  }
  out->max_d = kCosMaxDims;
  out->max_k = FVDB_MAX_K;
  out->E = kCosE;
  out->mag_min = kCosMagMin;
  out->mag_max = kCosMagMax;
  if (ix->searched) {  // the counters of the last search, wherever it was enqueued
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());
    uint32_t w[4];
    HIPCHK(ctx, download(ctx, w, ix->slots[ix->last_slot].ctr.p, 16));
    out->exact_pairs = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    out->fallback_queries = w[2];
  }
  return FVDB_OK;
}

int fvdb_cos_index_add(fvdb_cos_index* ix, const uint64_t* ids, const float* rows, uint64_t n) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->ctx;
  if (n == 0) return FVDB_OK;
  if (!ids || !rows) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (ix->n + n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "index limited to 2^32-1 rows");
  const int rc = cos_check_rows(ctx, rows, n, ix->d);
  if (rc) return rc;
  {
    std::unordered_set<uint64_t> seen;
    for (uint64_t i = 0; i < n; ++i)
      if (ix->row_of.count(ids[i]) || !seen.insert(ids[i]).second) FAIL(ctx, FVDB_E_DUPLICATE, "Vector already exists");
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint64_t blocks = cdiv(ix->n + n, 32);
  if (blocks > ix->cap_blocks) {  // operand blocks and flags come zeroed
    const uint64_t nb = std::max<uint64_t>(blocks, ix->cap_blocks + ix->cap_blocks / 2), ob = cdiv(ix->n, 32);
    const size_t wb = (size_t)ix->ksteps * 1024;
    HIPCHK(ctx, grow_keeping(ix->ops, nb * wb, ob * wb, /*zero_rest=*/true, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->rows, nb * 32 * ix->dpad * 4, ix->n * ix->dpad * 4, /*zero_rest=*/false, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->mag, nb * 32 * 4, ix->n * 4, /*zero_rest=*/false, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->ids, nb * 32 * 8, ix->n * 8, /*zero_rest=*/false, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->dead, nb * 32 * 4, ix->n * 4, /*zero_rest=*/true, ctx->stream));
    ix->cap_blocks = nb;
  }
  HIPCHK(ctx, ix->s_in.ensure(n * ix->d * 4));
  HIPCHK(ctx, upload(ctx, ix->s_in.p, rows, n * ix->d * 4));
  CosPrepArgs a{};
  a.rows = ix->s_in.as<float>();
  a.d = ix->d;
  a.ksteps = ix->ksteps;
  a.cpad = ix->dpad;
  a.n = a.n_pad = n;
  a.first = ix->n;
  a.copy = ix->rows.as<float>();
  a.mag = ix->mag.as<float>();
  a.ops = ix->ops.as<uint4>();
  launch_prepare(ctx, a);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, upload(ctx, ix->ids.as<uint64_t>() + ix->n, ids, n * 8));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (uint64_t i = 0; i < n; ++i) ix->row_of.emplace(ids[i], (uint32_t)(ix->n + i));
  ix->h_dead.resize(ix->n + n, 0);
  ix->n += n;
  ix->live += n;
  return FVDB_OK;
}

int fvdb_cos_index_set_deleted(fvdb_cos_index* ix, const uint64_t* ids, uint64_t n, int flag) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->ctx;
  if (n == 0) return FVDB_OK;
  if (!ids) FAIL(ctx, FVDB_E_INVALID, "null argument");
  std::vector<uint32_t> rows(n);
  for (uint64_t i = 0; i < n; ++i) {
    const auto it = ix->row_of.find(ids[i]);
    if (it == ix->row_of.end()) FAIL(ctx, FVDB_E_NOT_FOUND, "Vector not found");
    rows[i] = it->second;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, ix->s_rows.ensure(n * 4));
  HIPCHK(ctx, upload(ctx, ix->s_rows.p, rows.data(), n * 4));
  hipLaunchKernelGGL(cos_set_flags_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, ix->s_rows.as<uint32_t>(), n, flag ? 1u : 0u,
                     ix->dead.as<uint32_t>());
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const uint8_t f = flag ? 1 : 0;
  for (uint32_t r : rows) {
    if (ix->h_dead[r] != f) ix->live += f ? (uint64_t)-1 : 1;
    ix->h_dead[r] = f;
  }
  return FVDB_OK;
}

int fvdb_cos_index_search_dev_slot(fvdb_cos_index* ix, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t k, int mode,
                                   const uint32_t* dead_dev, uint64_t* out_ids_dev, float* out_sim_dev, uint32_t* out_counts_dev) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = on ? on : ix->ctx;
  if (slot >= kCosSlots) FAIL(ctx, FVDB_E_INVALID, "slot out of range");
  if (ctx->device != ix->ctx->device) FAIL(ctx, FVDB_E_INVALID, "context of another device");
  int rc = check_search(ctx, k, mode);
  if (rc) return rc;
  if (!q_dev || !out_ids_dev || !out_sim_dev || !out_counts_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  CosSlot& S = ix->slots[slot];
  const uint32_t d = ix->d, ksteps = ix->ksteps;
  const uint32_t kr = k <= 64 ? 1 : (k <= 128 ? 2 : 4);
  const uint32_t n = (uint32_t)ix->n, blocks = cdiv(n, 32);
  const bool filter = mode == FVDB_COS_FILTER;
  // Enough (tile, slice) workgroups to fill the device at a small batch, no slice under kCosMinSliceBlocks.  Every
  // slice emits its first k rows and then what passes its own running threshold: the arena holds four times
  // 2 k + 64 rows a slice, and never needs more than n.
  uint32_t slice_blocks = 0, slices = 0, cap = 1;
  if (n && filter) {
    const uint32_t tiles = cdiv(std::min(B, kCosSubBatch), kCosTile);
    const uint32_t want = std::max<uint32_t>(1, std::min<uint32_t>(cdiv(blocks, kCosMinSliceBlocks), cdiv(4 * (uint32_t)ctx->num_cus, tiles)));
    slice_blocks = (cdiv(blocks, want) + 3u) & ~3u;  // whole rounds
    slices = cdiv(blocks, slice_blocks);
    cap = (uint32_t)std::min<uint64_t>(n, (uint64_t)slices * 4u * (2u * k + 64u));
  }
  const uint32_t sub = std::max<uint32_t>(32, (uint32_t)std::min<size_t>(kCosSubBatch, kCosArenaBytes / ((size_t)cap * 4)) & ~31u);
  for (uint32_t b0 = 0; b0 < B; b0 += sub) {
    const uint32_t Bs = std::min(sub, B - b0), tiles = cdiv(Bs, kCosTile);
    HIPCHK(ctx, S.ctr.ensure(16 + (size_t)sub * 8));
    HIPCHK(ctx, S.qops.ensure((size_t)tiles * ksteps * 1024));
    HIPCHK(ctx, S.qmag.ensure((size_t)Bs * 4));
    HIPCHK(ctx, S.qpad.ensure((size_t)Bs * ix->dq * 4));
    HIPCHK(ctx, S.arena.ensure((size_t)Bs * cap * 4));
    uint32_t* ctr = S.ctr.as<uint32_t>();
    {  // the search's counters once, the sub-batch's arena counts and overflow flags every time (no memset: a kernel)
      const uint32_t skip = b0 ? 4u : 0u;
      const uint64_t words = 4u + 2ull * Bs - skip;
      hipLaunchKernelGGL(cos_clear_kernel, dim3(cdiv(words, 256)), dim3(256), 0, ctx->stream, ctr + skip, words);
    }
    CosPrepArgs p{};
    p.rows = q_dev + (size_t)b0 * d;
    p.d = d;
    p.ksteps = ksteps;
    p.cpad = ix->dq;
    p.n = Bs;
    p.n_pad = (uint64_t)tiles * kCosTile;
    p.copy = S.qpad.as<float>();
    p.mag = S.qmag.as<float>();
    p.ops = S.qops.as<uint4>();
    launch_prepare(ctx, p);

    CosScanArgs s{};
    s.ops = ix->ops.as<uint4>();
    s.dead = dead_dev ? dead_dev : ix->dead.as<uint32_t>();
    s.qops = S.qops.as<uint4>();
    s.arena = S.arena.as<uint32_t>();
    s.arena_cnt = ctr + 4;
    s.overflow = ctr + 4 + Bs;
    s.n = n;
    s.ksteps = ksteps;
    s.B = Bs;
    s.k = k;
    s.cap = cap;
    s.slice_blocks = slice_blocks;

    CosExactArgs e{};
    e.rows = ix->rows.as<float>();
    e.mag = ix->mag.as<float>();
    e.dead = s.dead;
    e.queries = S.qpad.as<float>();
    e.qmag = S.qmag.as<float>();
    e.arena = s.arena;
    e.arena_cnt = s.arena_cnt;
    e.overflow = s.overflow;
    e.pairs = (unsigned long long*)ctr;
    e.fallbacks = ctr + 2;
    e.n = n;
    e.dpad = ix->dpad;
    e.dq = ix->dq;
    e.B = Bs;
    e.k = k;
    e.cap = cap;
    e.W = std::max<uint32_t>(1, std::min<uint32_t>(kCosMaxExactWaves, cdiv(16 * (uint32_t)ctx->num_cus, Bs)));
    e.all = filter ? 0u : 1u;
    HIPCHK(ctx, S.part.ensure((size_t)e.W * Bs * k * 8));
    e.part = S.part.as<uint64_t>();

    uint64_t* oi = out_ids_dev + (size_t)b0 * k;
    float* os = out_sim_dev + (size_t)b0 * k;
    uint32_t* oc = out_counts_dev + b0;
    const bool qlds = ix->qlds(kr);
    switch (kr) {
      case 1: rc = launch_chain<1>(ctx, qlds, filter, s, slices, e, ix->ids.as<uint64_t>(), oi, os, oc); break;
      case 2: rc = launch_chain<2>(ctx, qlds, filter, s, slices, e, ix->ids.as<uint64_t>(), oi, os, oc); break;
      default: rc = launch_chain<4>(ctx, qlds, filter, s, slices, e, ix->ids.as<uint64_t>(), oi, os, oc); break;
    }
    if (rc) return rc;
  }
  ix->last_slot = slot;
  ix->searched = true;
  return FVDB_OK;
}

int fvdb_cos_index_search(fvdb_cos_index* ix, const float* q, uint32_t B, uint32_t k, int mode, const uint64_t* allowed_ids,
                          uint64_t n_allowed, uint64_t* out_ids, float* out_sim, uint32_t* out_counts) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->ctx;
  if (B == 0) return FVDB_OK;
  if (!q || !out_ids || !out_sim || !out_counts) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (n_allowed && !allowed_ids) FAIL(ctx, FVDB_E_INVALID, "null allow-set");
  int rc = check_search(ctx, k, mode);
  if (rc) return rc;
  rc = cos_check_rows(ctx, q, B, ix->d);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  CosSlot& S = ix->slots[0];
  HIPCHK(ctx, S.q.ensure((size_t)B * ix->d * 4));
  HIPCHK(ctx, S.out.ensure((size_t)B * k * 16 + (size_t)B * 4));
  HIPCHK(ctx, upload(ctx, S.q.p, q, (size_t)B * ix->d * 4));
  const uint32_t* dead_dev = nullptr;
  if (allowed_ids && ix->n) {  // the allow-set as the scan's "dead" words: deleted, or not allowed
    std::vector<uint32_t> dw(ix->n, 1u);
    for (uint64_t i = 0; i < n_allowed; ++i) {
      const auto it = ix->row_of.find(allowed_ids[i]);
      if (it != ix->row_of.end()) dw[it->second] = ix->h_dead[it->second];
    }
    HIPCHK(ctx, S.dead.ensure(ix->n * 4));
    HIPCHK(ctx, upload(ctx, S.dead.p, dw.data(), ix->n * 4));
    dead_dev = S.dead.as<uint32_t>();
  }
  uint64_t* oi = S.out.as<uint64_t>();
  float* os = (float*)(oi + (size_t)B * k);
  uint32_t* oc = (uint32_t*)(os + (size_t)B * k);
  rc = fvdb_cos_index_search_dev_slot(ix, ctx, 0, S.q.as<float>(), B, k, mode, dead_dev, oi, os, oc);
  if (rc) return rc;
  HIPCHK(ctx, download(ctx, out_ids, oi, (size_t)B * k * 8));
  HIPCHK(ctx, download(ctx, out_sim, os, (size_t)B * k * 4));
  HIPCHK(ctx, download(ctx, out_counts, oc, (size_t)B * 4));
  return FVDB_OK;
}

}  // extern "C"
