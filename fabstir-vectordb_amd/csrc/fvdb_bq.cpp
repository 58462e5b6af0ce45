// fvdb_bq.cpp — binary quantization behind the C ABI (include/fvdb.h, "binary quantization"):
// the sign-bit codec, the codes index and its Hamming and refined search.  A translation unit of its own: the kernels
// are kernels_bq.h, the shared pieces (WaveTopK, flat_merge_kernel, the refine wave and the row scorer) come from their
// headers unchanged, and the refine rows live in an fvdb_store reached through the C ABI.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <new>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "fvdb_internal.h"
#include "common.h"
#include "kernels_bq.h"

using namespace fvdb;

namespace {

constexpr uint32_t kBqSlots = 16;
constexpr uint32_t kBqSubBatch = 8192;          // queries of one launch chain, a multiple of the 64-query tile
constexpr uint32_t kBqMinSliceBlocks = 16;      // 1024 rows: a slice shorter than this does not pay for its partial list
constexpr size_t kBqScratchBytes = 256u << 20;  // partial lists of one launch chain

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
  if (d > kBqMaxDims) FAIL(ctx, FVDB_E_UNSUPPORTED, "binary quantization: d must be <= 2048");
  return FVDB_OK;
}

// what the host forms refuse before anything is written
int check_finite(fvdb_ctx* ctx, const float* x, uint64_t count, const char* what) {
  for (uint64_t i = 0; i < count; ++i)
    if (!std::isfinite(x[i])) FAIL(ctx, FVDB_E_NONFINITE, what);
  return FVDB_OK;
}

void launch_encode(fvdb_ctx* on, const BqEncodeArgs& a) {
  hipLaunchKernelGGL(bq_encode_kernel, dim3(cdiv(a.n, 4)), dim3(256), 0, on->stream, a);
}

}  // namespace

struct BqSlot {
  DBuf q, qcodes, qpad, part, nodes, dist, counts, dead, out;
};

struct fvdb_bq_index {
  fvdb_ctx* ctx = nullptr;
  uint32_t d = 0, chunks = 0, lds_limit = 0;
  fvdb_store* store = nullptr;
  DBuf centre, codes, ids, dead, s_in, s_rows;  // centre: null pointer = zeros
  uint64_t n = 0, cap_blocks = 0, live = 0;
  std::unordered_map<uint64_t, uint32_t> row_of;
  std::vector<uint8_t> h_dead;
  std::atomic<uint32_t> last_slices{0};
  std::atomic<uint64_t> last_pairs{0};
  BqSlot slots[kBqSlots];
};

namespace {

template <int KR, int C>
int launch_scan_c(fvdb_ctx* on, const BqScanArgs& a) {
  const uint32_t lds = bq_scan_lds(KR);
  // the attribute belongs to the function; every call sets what it needs
  HIPCHK(on, hipFuncSetAttribute((const void*)bq_scan_kernel<KR, C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((bq_scan_kernel<KR, C>), dim3(cdiv(a.B, kBqTile), a.slices), dim3(256), lds, on->stream, a);
  return FVDB_OK;
}

// the scan of the index's chunk count (bq_chunks: 1, 2, 3, 4, 8 or 16), then the merge of the slices' lists
template <int KR>
int launch_scan(fvdb_ctx* on, uint32_t chunks, const BqScanArgs& a, uint32_t* out_nodes, float* out_dist, uint32_t* out_counts) {
  if (a.slices) {
    int rc;
    switch (chunks) {
      case 1: rc = launch_scan_c<KR, 1>(on, a); break;
      case 2: rc = launch_scan_c<KR, 2>(on, a); break;
      case 3: rc = launch_scan_c<KR, 3>(on, a); break;
      case 4: rc = launch_scan_c<KR, 4>(on, a); break;
      case 8: rc = launch_scan_c<KR, 8>(on, a); break;
      default: rc = launch_scan_c<KR, 16>(on, a); break;
    }
    if (rc) return rc;
  }
  hipLaunchKernelGGL((flat_merge_kernel<KR>), dim3(cdiv(a.B, 4)), dim3(256), 0, on->stream, a.part, a.slices, a.B, a.k, out_nodes, out_dist,
                     out_counts);
  HIPCHK(on, hipGetLastError());
  return FVDB_OK;
}

template <typename RT>
void launch_refine(fvdb_ctx* on, const RefineArgs& r) {
  const dim3 grid(cdiv(r.B, 4)), block(256);
  if (r.k <= 64) hipLaunchKernelGGL((bq_refine_kernel<1, RT>), grid, block, 0, on->stream, r);
  else if (r.k <= 128) hipLaunchKernelGGL((bq_refine_kernel<2, RT>), grid, block, 0, on->stream, r);
  else hipLaunchKernelGGL((bq_refine_kernel<4, RT>), grid, block, 0, on->stream, r);
}

int check_search(fvdb_bq_index* ix, fvdb_ctx* ctx, uint32_t k, uint32_t fetch_k) {
  if (k == 0 || k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "Hamming search: k must be in 1..FVDB_MAX_K");
  if (fetch_k) {
    if (fetch_k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "refined search: fetch_k must be <= FVDB_MAX_K");
    if (k > fetch_k) FAIL(ctx, FVDB_E_INVALID, "refined search: k must be <= fetch_k");
    if (!ix->store) FAIL(ctx, FVDB_E_INVALID, "refined search needs an index created with refine rows");
  }
  return FVDB_OK;
}

}  // namespace

extern "C" {

// ---- the codec -------------------------------------------------------------------------------------------------------
int fvdb_bq_encode_dev(fvdb_ctx* ctx, const float* rows_dev, uint64_t n, uint32_t d, const float* centre_dev, uint8_t* out_codes_dev) {
  if (!ctx) return FVDB_E_INVALID;
  int rc = check_dims(ctx, d);
  if (rc) return rc;
  if (n == 0) return FVDB_OK;
  if (!rows_dev || !out_codes_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "a call is limited to 2^32-1 rows");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  BqEncodeArgs a{};
  a.rows = rows_dev;
  a.centre = centre_dev;
  a.d = d;
  a.chunks = bq_chunks(d);
  a.n = n;
  a.flat = out_codes_dev;
  launch_encode(ctx, a);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int fvdb_bq_encode(fvdb_ctx* ctx, const float* rows, uint64_t n, uint32_t d, const float* centre, uint8_t* out_codes) {
  if (!ctx) return FVDB_E_INVALID;
  int rc = check_dims(ctx, d);
  if (rc) return rc;
  if (n == 0) return FVDB_OK;
  if (!rows || !out_codes) FAIL(ctx, FVDB_E_INVALID, "null argument");
  rc = check_finite(ctx, rows, n * d, "non-finite input value");
  if (!rc && centre) rc = check_finite(ctx, centre, d, "non-finite centre value");
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t nbytes = (d + 7u) / 8u;
  DBuf in, cen, codes;
  HIPCHK(ctx, in.exact(n * d * 4));
  HIPCHK(ctx, codes.exact(n * nbytes));
  HIPCHK(ctx, upload(ctx, in.p, rows, n * d * 4));
  if (centre) {
    HIPCHK(ctx, cen.exact((size_t)d * 4));
    HIPCHK(ctx, upload(ctx, cen.p, centre, (size_t)d * 4));
  }
  rc = fvdb_bq_encode_dev(ctx, in.as<float>(), n, d, cen.as<float>(), codes.as<uint8_t>());
  if (rc) return rc;
  HIPCHK(ctx, download(ctx, out_codes, codes.p, n * nbytes));
  return FVDB_OK;
}

// ---- the codes index -------------------------------------------------------------------------------------------------
int fvdb_bq_index_create(fvdb_ctx* ctx, uint32_t d, int refine_dtype, const float* centre, fvdb_bq_index** out) {
  if (!ctx || !out) return FVDB_E_INVALID;
  *out = nullptr;
  int rc = check_dims(ctx, d);
  if (rc) return rc;
  if (refine_dtype != FVDB_BQ_NO_REFINE && refine_dtype != FVDB_F32 && refine_dtype != FVDB_F16)
    FAIL(ctx, FVDB_E_INVALID, "refine_dtype must be FVDB_BQ_NO_REFINE, FVDB_F32 or FVDB_F16");
  if (centre) {
    rc = check_finite(ctx, centre, d, "non-finite centre value");
    if (rc) return rc;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int lds = 0;
  HIPCHK(ctx, hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  fvdb_bq_index* ix = new (std::nothrow) fvdb_bq_index();
  if (!ix) return FVDB_E_OOM;
  ix->ctx = ctx;
  ix->d = d;
  ix->chunks = bq_chunks(d);
  ix->lds_limit = (uint32_t)lds;
  hipError_t e = hipSuccess;
  if (centre) {
    e = ix->centre.exact((size_t)d * 4);
    if (e == hipSuccess) e = upload(ctx, ix->centre.p, centre, (size_t)d * 4);
  }
  if (e != hipSuccess) {
    delete ix;
    HIPCHK(ctx, e);
  }
  if (refine_dtype != FVDB_BQ_NO_REFINE) {
    rc = fvdb_store_create_ex(ctx, d, 1024, refine_dtype, &ix->store);
    if (rc) {
      delete ix;
      return rc;
    }
  }
  *out = ix;
  return FVDB_OK;
}

void fvdb_bq_index_destroy(fvdb_bq_index* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->ctx->device);
  (void)hipDeviceSynchronize();  // searches may be in flight on other contexts' streams
  if (ix->store) fvdb_store_destroy(ix->store);
  delete ix;
}

uint64_t fvdb_bq_index_rows(fvdb_bq_index* ix) { return ix ? ix->n : 0; }
uint64_t fvdb_bq_index_live(fvdb_bq_index* ix) { return ix ? ix->live : 0; }
uint64_t fvdb_bq_index_bytes(fvdb_bq_index* ix) {
  if (!ix) return 0;
  return (uint64_t)cdiv(ix->n, 64) * ix->chunks * 1024 + ix->n * 12 + (ix->store ? fvdb_store_bytes(ix->store) : 0);
}

int fvdb_bq_index_info(fvdb_bq_index* ix, fvdb_bq_info_t* out) {
  if (!ix || !out) return FVDB_E_INVALID;
  memset(out, 0, sizeof(*out));
  out->d = ix->d;
  out->words = bq_words(ix->d);
  out->chunks = ix->chunks;
  out->block_rows = 64;
  out->queries_per_workgroup = kBqTile;
  out->round_rows = kBqRoundRows;
  out->min_slice_rows = kBqMinSliceBlocks * 64;
  out->max_slice_rows = kBqMaxSliceBlocks * 64;
  out->lds_limit = ix->lds_limit;
  const uint32_t krs[3] = {1, 2, 4};
  for (int i = 0; i < 3; ++i) out->lds_bytes[i] = bq_scan_lds(krs[i]);
  out->max_d = kBqMaxDims;
  out->max_k = FVDB_MAX_K;
  out->last_slices = ix->last_slices.load();
  out->last_pairs = ix->last_pairs.load();
  return FVDB_OK;
}

int fvdb_bq_index_add(fvdb_bq_index* ix, const uint64_t* ids, const float* rows, uint64_t n) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->ctx;
  if (n == 0) return FVDB_OK;
  if (!ids || !rows) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (ix->n + n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "index limited to 2^32-1 rows");
  int rc = check_finite(ctx, rows, n * ix->d, "non-finite input value");
  if (rc) return rc;
  {
    std::unordered_set<uint64_t> seen;
    for (uint64_t i = 0; i < n; ++i)
      if (ix->row_of.count(ids[i]) || !seen.insert(ids[i]).second) FAIL(ctx, FVDB_E_DUPLICATE, "Vector already exists");
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint64_t blocks = cdiv(ix->n + n, 64);
  if (blocks > ix->cap_blocks) {  // code blocks and flags come zeroed
    const uint64_t nb = std::max<uint64_t>(blocks, ix->cap_blocks + ix->cap_blocks / 2), ob = cdiv(ix->n, 64);
    const size_t wb = (size_t)ix->chunks * 1024;
    HIPCHK(ctx, grow_keeping(ix->codes, nb * wb, ob * wb, /*zero_rest=*/true, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->ids, nb * 64 * 8, ix->n * 8, /*zero_rest=*/false, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->dead, nb * 64 * 4, ix->n * 4, /*zero_rest=*/true, ctx->stream));
    ix->cap_blocks = nb;
  }
  HIPCHK(ctx, ix->s_in.ensure(n * ix->d * 4));
  HIPCHK(ctx, upload(ctx, ix->s_in.p, rows, n * ix->d * 4));
  BqEncodeArgs a{};
  a.rows = ix->s_in.as<float>();
  a.centre = ix->centre.as<float>();
  a.d = ix->d;
  a.chunks = ix->chunks;
  a.n = n;
  a.first = ix->n;
  a.blocks = ix->codes.as<uint32_t>();
  launch_encode(ctx, a);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, upload(ctx, ix->ids.as<uint64_t>() + ix->n, ids, n * 8));
  if (ix->store) {
    uint64_t first = 0;
    rc = fvdb_store_append(ix->store, rows, n, &first);
    if (rc) return rc;
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (uint64_t i = 0; i < n; ++i) ix->row_of.emplace(ids[i], (uint32_t)(ix->n + i));
  ix->h_dead.resize(ix->n + n, 0);
  ix->n += n;
  ix->live += n;
  return FVDB_OK;
}

int fvdb_bq_index_set_deleted(fvdb_bq_index* ix, const uint64_t* ids, uint64_t n, int flag) {
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
  hipLaunchKernelGGL(bq_set_flags_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, ix->s_rows.as<uint32_t>(), n, flag ? 1u : 0u,
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

int fvdb_bq_index_search_dev_slot(fvdb_bq_index* ix, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t k,
                                  uint32_t fetch_k, const uint32_t* dead_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                                  uint32_t* out_counts_dev) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = on ? on : ix->ctx;
  if (slot >= kBqSlots) FAIL(ctx, FVDB_E_INVALID, "slot out of range");
  if (ctx->device != ix->ctx->device) FAIL(ctx, FVDB_E_INVALID, "context of another device");
  int rc = check_search(ix, ctx, k, fetch_k);
  if (rc) return rc;
  if (!q_dev || !out_ids_dev || !out_dist_dev || !out_counts_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  BqSlot& S = ix->slots[slot];
  const uint32_t d = ix->d, chunks = ix->chunks;
  const uint32_t kk = fetch_k ? fetch_k : k;
  const uint32_t kr = kk <= 64 ? 1 : (kk <= 128 ? 2 : 4);
  const uint32_t n = (uint32_t)ix->n, blocks = cdiv(n, 64);
  const uint32_t rpad = fetch_k ? ix->store->dpad : 0;  // row stride of the refine source
  // Slices: enough (tile, slice) workgroups for six a CU (two turns of the three that fit one at k <= 64), none under
  // kBqMinSliceBlocks, none over what an in-slice key can number.  The launch chain is halved, down to one tile, until
  // its partial lists fit.
  uint32_t sub = kBqSubBatch, slice_blocks = 0, slices = 0;
  while (n) {
    const uint32_t Bs = std::min(sub, B), tiles = cdiv(Bs, kBqTile);
    uint32_t want = std::max<uint32_t>(1, std::min<uint32_t>(cdiv(blocks, kBqMinSliceBlocks), cdiv(6 * (uint32_t)ctx->num_cus, tiles)));
    want = std::max(want, cdiv(blocks, kBqMaxSliceBlocks));
    slice_blocks = (cdiv(blocks, want) + 3u) & ~3u;  // whole rounds; kBqMaxSliceBlocks is a multiple of 4
    slices = cdiv(blocks, slice_blocks);
    if ((size_t)slices * Bs * kk * 8 <= kBqScratchBytes || sub <= kBqTile) break;
    sub = std::max(kBqTile, (sub / 2) & ~(kBqTile - 1u));
  }
  ix->last_slices.store(slices);
  ix->last_pairs.store((uint64_t)B * n);
  for (uint32_t b0 = 0; b0 < B; b0 += sub) {
    const uint32_t Bs = std::min(sub, B - b0);
    const float* qs = q_dev + (size_t)b0 * d;
    BqScanArgs a{};
    a.codes = ix->codes.as<uint4>();
    a.dead = dead_dev ? dead_dev : ix->dead.as<uint32_t>();
    a.n = n;
    a.B = Bs;
    a.k = kk;
    a.slices = slices;
    a.slice_blocks = slice_blocks;
    if (n) {  // the queries by the rows' rule, a query's words together
      HIPCHK(ctx, S.qcodes.ensure((size_t)Bs * chunks * 16));
      BqEncodeArgs e{};
      e.rows = qs;
      e.centre = ix->centre.as<float>();
      e.d = d;
      e.chunks = chunks;
      e.n = Bs;
      e.per_row = S.qcodes.as<uint32_t>();
      launch_encode(ctx, e);
    }
    a.qcodes = S.qcodes.as<uint32_t>();
    HIPCHK(ctx, S.part.ensure(std::max<size_t>((size_t)slices * Bs * kk * 8, 8)));
    a.part = S.part.as<uint64_t>();
    HIPCHK(ctx, S.nodes.ensure((size_t)Bs * kk * 4));
    uint32_t* nodes = S.nodes.as<uint32_t>();
    float* dist = out_dist_dev + (size_t)b0 * k;
    uint32_t* counts = out_counts_dev + b0;
    if (fetch_k) {
      HIPCHK(ctx, S.dist.ensure((size_t)Bs * kk * 4));
      HIPCHK(ctx, S.counts.ensure((size_t)Bs * 4));
      dist = S.dist.as<float>();
      counts = S.counts.as<uint32_t>();
    }
    switch (kr) {
      case 1: rc = launch_scan<1>(ctx, chunks, a, nodes, dist, counts); break;
      case 2: rc = launch_scan<2>(ctx, chunks, a, nodes, dist, counts); break;
      default: rc = launch_scan<4>(ctx, chunks, a, nodes, dist, counts); break;
    }
    if (rc) return rc;
    uint64_t* oi = out_ids_dev + (size_t)b0 * k;
    if (!fetch_k) {
      hipLaunchKernelGGL(bq_map_ids_kernel, dim3(cdiv((uint64_t)Bs * k, 256)), dim3(256), 0, ctx->stream, nodes, ix->ids.as<uint64_t>(),
                         (uint64_t)Bs * k, oi);
    } else {
      RefineArgs r{};
      r.queries = qs;
      if (rpad != d) {
        HIPCHK(ctx, S.qpad.ensure((size_t)Bs * rpad * 4));
        hipLaunchKernelGGL(bq_pad_queries_kernel, dim3(cdiv((uint64_t)Bs * rpad, 256)), dim3(256), 0, ctx->stream, qs, d, rpad, (uint64_t)Bs,
                           S.qpad.as<float>());
        r.queries = S.qpad.as<float>();
      }
      r.rows = ix->store->data;
      r.cand = nodes;
      r.cand_cnt = counts;
      r.ids = ix->ids.as<uint64_t>();
      r.dpad = rpad;
      r.B = Bs;
      r.fk = kk;
      r.k = k;
      r.out_ids = oi;
      r.out_dist = out_dist_dev + (size_t)b0 * k;
      r.out_counts = out_counts_dev + b0;
      if (ix->store->f16()) launch_refine<half_t>(ctx, r);
      else launch_refine<float>(ctx, r);
    }
    HIPCHK(ctx, hipGetLastError());
  }
  return FVDB_OK;
}

int fvdb_bq_index_search(fvdb_bq_index* ix, const float* q, uint32_t B, uint32_t k, uint32_t fetch_k, const uint64_t* allowed_ids,
                         uint64_t n_allowed, uint64_t* out_ids, float* out_dist, uint32_t* out_counts) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->ctx;
  if (B == 0) return FVDB_OK;
  if (!q || !out_ids || !out_dist || !out_counts) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (n_allowed && !allowed_ids) FAIL(ctx, FVDB_E_INVALID, "null allow-set");
  int rc = check_search(ix, ctx, k, fetch_k);
  if (rc) return rc;
  rc = check_finite(ctx, q, (uint64_t)B * ix->d, "non-finite query value");
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  BqSlot& S = ix->slots[0];
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
  float* od = (float*)(oi + (size_t)B * k);
  uint32_t* oc = (uint32_t*)(od + (size_t)B * k);
  rc = fvdb_bq_index_search_dev_slot(ix, ctx, 0, S.q.as<float>(), B, k, fetch_k, dead_dev, oi, od, oc);
  if (rc) return rc;
  HIPCHK(ctx, download(ctx, out_ids, oi, (size_t)B * k * 8));
  HIPCHK(ctx, download(ctx, out_dist, od, (size_t)B * k * 4));
  HIPCHK(ctx, download(ctx, out_counts, oc, (size_t)B * 4));
  return FVDB_OK;
}

}  // extern "C"
