// fvdb_sq8.cpp — scalar quantization to u8 behind the C ABI (include/fvdb.h, "scalar quantization"; DESIGN.md section
// 9x): the codec, the codes index and its symmetric and refined search.  A translation unit of its own: the kernels are
// kernels_sq8.h, the shared pieces (WaveTopK, flat_merge_kernel, the refine wave and the row scorer) come from their
// headers unchanged, and the refine rows live in an fvdb_store reached through the C ABI.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "fvdb_internal.h"
#include "common.h"
#include "kernels_sq8.h"

using namespace fvdb;

// every element finite and every row's hi - lo finite in f32: what encode refuses before anything is written
// (declared in fvdb_internal.h: the probed index, fvdb_ivfsq8.cpp, refuses the same rows)
int sq8_check_rows(fvdb_ctx* ctx, const float* x, uint64_t n, uint32_t d) {
  for (uint64_t r = 0; r < n; ++r) {
    const float* row = x + r * d;
    float mn = row[0], mx = row[0];
    for (uint32_t i = 0; i < d; ++i) {
      if (!std::isfinite(row[i])) FAIL(ctx, FVDB_E_NONFINITE, "non-finite input value");
      mn = std::min(mn, row[i]);
      mx = std::max(mx, row[i]);
    }
    if (!std::isfinite(mx - mn)) FAIL(ctx, FVDB_E_NONFINITE, "a row's range (max - min) overflows f32");
  }
  return FVDB_OK;
}

namespace {

constexpr uint32_t kSq8Slots = 16;
constexpr uint32_t kSq8SubBatch = 8192;        // queries of one launch chain, a multiple of the 32-query tile
constexpr uint32_t kSq8MinSliceBlocks = 16;    // 512 rows: a slice shorter than this does not pay for its partial list
constexpr size_t kSq8DecodedBytes = 256u << 20;  // decoded candidate rows of one launch chain

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
  if (d > kSq8MaxDims) FAIL(ctx, FVDB_E_UNSUPPORTED, "scalar quantization: d must be <= 2048");
  return FVDB_OK;
}

}  // namespace

struct Sq8Slot {
  DBuf q, qcodes, qinfo, qpad, part, nodes, dist, counts, dead, decoded, out;
};

struct fvdb_sq8_index {
  fvdb_ctx* ctx = nullptr;
  uint32_t d = 0, ksteps = 0, lds_limit = 0;
  int refine = FVDB_SQ8_NO_REFINE;
  fvdb_store* store = nullptr;
  DBuf codes, info, ids, dead, s_in, s_rows;
  uint64_t n = 0, cap_blocks = 0, live = 0;
  std::unordered_map<uint64_t, uint32_t> row_of;
  std::vector<uint8_t> h_dead;
  Sq8Slot slots[kSq8Slots];
  uint32_t dpad4() const { return (d + 3u) & ~3u; }
  // the query operands go to LDS when they fit beside the survivor buffers of the k class, else they are read from HBM
  bool qlds(uint32_t kr) const { return sq8_scan_lds(kr, ksteps, true) <= lds_limit; }
};

namespace {

void launch_encode(fvdb_ctx* on, const Sq8EncodeArgs& a) {
  hipLaunchKernelGGL(sq8_encode_kernel, dim3(cdiv(a.n, 4)), dim3(256), 0, on->stream, a);
}

template <int KR, bool QLDS>
int launch_scan(fvdb_ctx* on, const Sq8ScanArgs& a, uint32_t* out_nodes, float* out_dist, uint32_t* out_counts) {
  if (a.slices) {
    const uint32_t lds = sq8_scan_lds(KR, a.ksteps, QLDS);
    // the attribute belongs to the function; every call sets what it needs
    HIPCHK(on, hipFuncSetAttribute((const void*)sq8_scan_kernel<KR, QLDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((sq8_scan_kernel<KR, QLDS>), dim3(cdiv(a.B, kSq8Tile), a.slices), dim3(256), lds, on->stream, a);
  }
  hipLaunchKernelGGL((flat_merge_kernel<KR>), dim3(cdiv(a.B, 4)), dim3(256), 0, on->stream, a.part, a.slices, a.B, a.k, out_nodes, out_dist,
                     out_counts);
  HIPCHK(on, hipGetLastError());
  return FVDB_OK;
}

template <int KR>
int launch_scan_q(bool qlds, fvdb_ctx* on, const Sq8ScanArgs& a, uint32_t* out_nodes, float* out_dist, uint32_t* out_counts) {
  return qlds ? launch_scan<KR, true>(on, a, out_nodes, out_dist, out_counts) : launch_scan<KR, false>(on, a, out_nodes, out_dist, out_counts);
}

template <typename RT>
void launch_refine(fvdb_ctx* on, const RefineArgs& r) {
  const dim3 grid(cdiv(r.B, 4)), block(256);
  if (r.k <= 64) hipLaunchKernelGGL((sq8_refine_kernel<1, RT>), grid, block, 0, on->stream, r);
  else if (r.k <= 128) hipLaunchKernelGGL((sq8_refine_kernel<2, RT>), grid, block, 0, on->stream, r);
  else hipLaunchKernelGGL((sq8_refine_kernel<4, RT>), grid, block, 0, on->stream, r);
}

int check_search(fvdb_sq8_index* ix, fvdb_ctx* ctx, uint32_t k, uint32_t fetch_k, int refine_mode) {
  if (k == 0 || k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "SQ8 search: k must be in 1..FVDB_MAX_K");
  if (fetch_k) {
    if (fetch_k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "refined search: fetch_k must be <= FVDB_MAX_K");
    if (k > fetch_k) FAIL(ctx, FVDB_E_INVALID, "refined search: k must be <= fetch_k");
    if (refine_mode != FVDB_SQ8_REFINE_DECODED && refine_mode != FVDB_SQ8_REFINE_ROWS)
      FAIL(ctx, FVDB_E_INVALID, "refine_mode must be FVDB_SQ8_REFINE_DECODED or FVDB_SQ8_REFINE_ROWS");
    if (refine_mode == FVDB_SQ8_REFINE_ROWS && !ix->store) FAIL(ctx, FVDB_E_INVALID, "FVDB_SQ8_REFINE_ROWS needs an index created with refine rows");
  }
  return FVDB_OK;
}

}  // namespace

extern "C" {

// ---- the codec -------------------------------------------------------------------------------------------------------
int fvdb_sq8_encode_dev(fvdb_ctx* ctx, const float* rows_dev, uint64_t n, uint32_t d, uint8_t* out_codes_dev, float* out_lo_dev,
                        float* out_hi_dev) {
  if (!ctx) return FVDB_E_INVALID;
  int rc = check_dims(ctx, d);
  if (rc) return rc;
  if (n == 0) return FVDB_OK;
  if (!rows_dev || !out_codes_dev || !out_lo_dev || !out_hi_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "a call is limited to 2^32-1 rows");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Sq8EncodeArgs a{};
  a.rows = rows_dev;
  a.d = d;
  a.n = n;
  a.flat = out_codes_dev;
  a.flat_lo = out_lo_dev;
  a.flat_hi = out_hi_dev;
  launch_encode(ctx, a);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int fvdb_sq8_decode_dev(fvdb_ctx* ctx, const uint8_t* codes_dev, const float* lo_dev, const float* hi_dev, uint64_t n, uint32_t d,
                        float* out_rows_dev) {
  if (!ctx) return FVDB_E_INVALID;
  int rc = check_dims(ctx, d);
  if (rc) return rc;
  if (n == 0) return FVDB_OK;
  if (!codes_dev || !lo_dev || !hi_dev || !out_rows_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "a call is limited to 2^32-1 rows");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(sq8_decode_kernel, dim3(cdiv(n * d, 256)), dim3(256), 0, ctx->stream, codes_dev, lo_dev, hi_dev, d, n, out_rows_dev);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int fvdb_sq8_encode(fvdb_ctx* ctx, const float* rows, uint64_t n, uint32_t d, uint8_t* out_codes, float* out_lo, float* out_hi) {
  if (!ctx) return FVDB_E_INVALID;
  int rc = check_dims(ctx, d);
  if (rc) return rc;
  if (n == 0) return FVDB_OK;
  if (!rows || !out_codes || !out_lo || !out_hi) FAIL(ctx, FVDB_E_INVALID, "null argument");
  rc = sq8_check_rows(ctx, rows, n, d);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DBuf in, codes, lohi;
  HIPCHK(ctx, in.exact(n * d * 4));
  HIPCHK(ctx, codes.exact(n * d));
  HIPCHK(ctx, lohi.exact(n * 8));
  HIPCHK(ctx, upload(ctx, in.p, rows, n * d * 4));
  rc = fvdb_sq8_encode_dev(ctx, in.as<float>(), n, d, codes.as<uint8_t>(), lohi.as<float>(), lohi.as<float>() + n);
  if (rc) return rc;
  HIPCHK(ctx, download(ctx, out_codes, codes.p, n * d));
  HIPCHK(ctx, download(ctx, out_lo, lohi.p, n * 4));
  HIPCHK(ctx, download(ctx, out_hi, lohi.as<float>() + n, n * 4));
  return FVDB_OK;
}

int fvdb_sq8_decode(fvdb_ctx* ctx, const uint8_t* codes, const float* lo, const float* hi, uint64_t n, uint32_t d, float* out_rows) {
  if (!ctx) return FVDB_E_INVALID;
  int rc = check_dims(ctx, d);
  if (rc) return rc;
  if (n == 0) return FVDB_OK;
  if (!codes || !lo || !hi || !out_rows) FAIL(ctx, FVDB_E_INVALID, "null argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DBuf in, lohi, out;
  HIPCHK(ctx, in.exact(n * d));
  HIPCHK(ctx, lohi.exact(n * 8));
  HIPCHK(ctx, out.exact(n * d * 4));
  HIPCHK(ctx, upload(ctx, in.p, codes, n * d));
  HIPCHK(ctx, upload(ctx, lohi.p, lo, n * 4));
  HIPCHK(ctx, upload(ctx, lohi.as<float>() + n, hi, n * 4));
  rc = fvdb_sq8_decode_dev(ctx, in.as<uint8_t>(), lohi.as<float>(), lohi.as<float>() + n, n, d, out.as<float>());
  if (rc) return rc;
  HIPCHK(ctx, download(ctx, out_rows, out.p, n * d * 4));
  return FVDB_OK;
}

// ---- the codes index -------------------------------------------------------------------------------------------------
int fvdb_sq8_index_create(fvdb_ctx* ctx, uint32_t d, int refine_dtype, fvdb_sq8_index** out) {
  if (!ctx || !out) return FVDB_E_INVALID;
  *out = nullptr;
  int rc = check_dims(ctx, d);
  if (rc) return rc;
  if (refine_dtype != FVDB_SQ8_NO_REFINE && refine_dtype != FVDB_F32 && refine_dtype != FVDB_F16)
    FAIL(ctx, FVDB_E_INVALID, "refine_dtype must be FVDB_SQ8_NO_REFINE, FVDB_F32 or FVDB_F16");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int lds = 0;
  HIPCHK(ctx, hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  fvdb_sq8_index* ix = new (std::nothrow) fvdb_sq8_index();
  if (!ix) return FVDB_E_OOM;
  ix->ctx = ctx;
  ix->d = d;
  ix->ksteps = (d + 31u) / 32u;
  ix->lds_limit = (uint32_t)lds;
  ix->refine = refine_dtype;
  if (refine_dtype != FVDB_SQ8_NO_REFINE) {
    rc = fvdb_store_create_ex(ctx, d, 1024, refine_dtype, &ix->store);
    if (rc) {
      delete ix;
      return rc;
    }
  }
  *out = ix;
  return FVDB_OK;
}

void fvdb_sq8_index_destroy(fvdb_sq8_index* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->ctx->device);
  (void)hipDeviceSynchronize();  // searches may be in flight on other contexts' streams
  if (ix->store) fvdb_store_destroy(ix->store);
  delete ix;
}

uint64_t fvdb_sq8_index_rows(fvdb_sq8_index* ix) { return ix ? ix->n : 0; }
uint64_t fvdb_sq8_index_live(fvdb_sq8_index* ix) { return ix ? ix->live : 0; }
uint64_t fvdb_sq8_index_bytes(fvdb_sq8_index* ix) {
  if (!ix) return 0;
  return (uint64_t)cdiv(ix->n, 32) * ix->ksteps * 1024 + ix->n * 28 + (ix->store ? fvdb_store_bytes(ix->store) : 0);
}

int fvdb_sq8_index_info(fvdb_sq8_index* ix, fvdb_sq8_info_t* out) {
  if (!ix || !out) return FVDB_E_INVALID;
  memset(out, 0, sizeof(*out));
  out->d = ix->d;
  out->d_padded = ix->ksteps * 32;
  out->block_rows = kSq8Tile;
  out->queries_per_workgroup = kSq8Tile;
  out->round_rows = kSq8RoundRows;
  out->words_in_flight = kSq8Ahead;
  out->min_slice_rows = kSq8MinSliceBlocks * kSq8Tile;
  out->lds_limit = ix->lds_limit;
  const uint32_t krs[3] = {1, 2, 4};
  for (int i = 0; i < 3; ++i) {
    out->queries_in_lds[i] = ix->qlds(krs[i]);
    out->lds_bytes[i] = sq8_scan_lds(krs[i], ix->ksteps, ix->qlds(krs[i]));
  }
  out->max_d = kSq8MaxDims;
  out->max_k = FVDB_MAX_K;
  return FVDB_OK;
}

int fvdb_sq8_index_add(fvdb_sq8_index* ix, const uint64_t* ids, const float* rows, uint64_t n) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->ctx;
  if (n == 0) return FVDB_OK;
  if (!ids || !rows) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (ix->n + n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "index limited to 2^32-1 rows");
  int rc = sq8_check_rows(ctx, rows, n, ix->d);
  if (rc) return rc;
  {
    std::unordered_set<uint64_t> seen;
    for (uint64_t i = 0; i < n; ++i)
      if (ix->row_of.count(ids[i]) || !seen.insert(ids[i]).second) FAIL(ctx, FVDB_E_DUPLICATE, "Vector already exists");
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint64_t blocks = cdiv(ix->n + n, 32);
  if (blocks > ix->cap_blocks) {  // code blocks and flags come zeroed
    const uint64_t nb = std::max<uint64_t>(blocks, ix->cap_blocks + ix->cap_blocks / 2), ob = cdiv(ix->n, 32);
    const size_t wb = (size_t)ix->ksteps * 1024;
    HIPCHK(ctx, grow_keeping(ix->codes, nb * wb, ob * wb, /*zero_rest=*/true, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->info, nb * 32 * 16, ix->n * 16, /*zero_rest=*/true, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->ids, nb * 32 * 8, ix->n * 8, /*zero_rest=*/false, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->dead, nb * 32 * 4, ix->n * 4, /*zero_rest=*/true, ctx->stream));
    ix->cap_blocks = nb;
  }
  HIPCHK(ctx, ix->s_in.ensure(n * ix->d * 4));
  HIPCHK(ctx, upload(ctx, ix->s_in.p, rows, n * ix->d * 4));
  Sq8EncodeArgs a{};
  a.rows = ix->s_in.as<float>();
  a.d = ix->d;
  a.ksteps = ix->ksteps;
  a.n = n;
  a.first = ix->n;
  a.blocks = ix->codes.as<uint4>();
  a.info = ix->info.as<uint4>();
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

int fvdb_sq8_index_set_deleted(fvdb_sq8_index* ix, const uint64_t* ids, uint64_t n, int flag) {
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
  hipLaunchKernelGGL(sq8_set_flags_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, ix->s_rows.as<uint32_t>(), n, flag ? 1u : 0u,
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

int fvdb_sq8_index_search_dev_slot(fvdb_sq8_index* ix, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t k,
                                   uint32_t fetch_k, int refine_mode, const uint32_t* dead_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                                   uint32_t* out_counts_dev) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = on ? on : ix->ctx;
  if (slot >= kSq8Slots) FAIL(ctx, FVDB_E_INVALID, "slot out of range");
  if (ctx->device != ix->ctx->device) FAIL(ctx, FVDB_E_INVALID, "context of another device");
  int rc = check_search(ix, ctx, k, fetch_k, refine_mode);
  if (rc) return rc;
  if (!q_dev || !out_ids_dev || !out_dist_dev || !out_counts_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Sq8Slot& S = ix->slots[slot];
  const uint32_t d = ix->d, ksteps = ix->ksteps;
  const uint32_t kk = fetch_k ? fetch_k : k;
  const uint32_t kr = kk <= 64 ? 1 : (kk <= 128 ? 2 : 4);
  const uint32_t n = (uint32_t)ix->n, blocks = cdiv(n, 32);
  const bool decoded = fetch_k && refine_mode == FVDB_SQ8_REFINE_DECODED;
  const uint32_t rpad = decoded ? ix->dpad4() : (fetch_k ? ix->store->dpad : 0);  // row stride of the refine source
  uint32_t sub = kSq8SubBatch;
  if (decoded) sub = std::max<uint32_t>(32, std::min<size_t>(sub, kSq8DecodedBytes / ((size_t)kk * rpad * 4)) & ~31u);
  for (uint32_t b0 = 0; b0 < B; b0 += sub) {
    const uint32_t Bs = std::min(sub, B - b0), tiles = cdiv(Bs, kSq8Tile);
    const float* qs = q_dev + (size_t)b0 * d;
    Sq8ScanArgs a{};
    a.codes = ix->codes.as<uint4>();
    a.info = ix->info.as<uint4>();
    a.dead = dead_dev ? dead_dev : ix->dead.as<uint32_t>();
    a.n = n;
    a.d = d;
    a.ksteps = ksteps;
    a.B = Bs;
    a.k = kk;
    if (n) {  // enough (tile, slice) workgroups to fill the device at a small batch, no slice under kSq8MinSliceBlocks
      const uint32_t want = std::max<uint32_t>(1, std::min<uint32_t>(cdiv(blocks, kSq8MinSliceBlocks), cdiv(4 * (uint32_t)ctx->num_cus, tiles)));
      a.slice_blocks = (cdiv(blocks, want) + 3u) & ~3u;  // whole rounds
      a.slices = cdiv(blocks, a.slice_blocks);
      HIPCHK(ctx, S.qcodes.ensure((size_t)tiles * ksteps * 1024));
      HIPCHK(ctx, S.qinfo.ensure((size_t)tiles * 32 * 16));
      Sq8EncodeArgs e{};
      e.rows = qs;
      e.d = d;
      e.ksteps = ksteps;
      e.n = Bs;
      e.blocks = S.qcodes.as<uint4>();
      e.info = S.qinfo.as<uint4>();
      launch_encode(ctx, e);
    }
    a.qcodes = S.qcodes.as<uint4>();
    a.qinfo = S.qinfo.as<uint4>();
    HIPCHK(ctx, S.part.ensure(std::max<size_t>((size_t)a.slices * Bs * kk * 8, 8)));
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
    const bool qlds = ix->qlds(kr);
    switch (kr) {
      case 1: rc = launch_scan_q<1>(qlds, ctx, a, nodes, dist, counts); break;
      case 2: rc = launch_scan_q<2>(qlds, ctx, a, nodes, dist, counts); break;
      default: rc = launch_scan_q<4>(qlds, ctx, a, nodes, dist, counts); break;
    }
    if (rc) return rc;
    uint64_t* oi = out_ids_dev + (size_t)b0 * k;
    if (!fetch_k) {
      hipLaunchKernelGGL(sq8_map_ids_kernel, dim3(cdiv((uint64_t)Bs * k, 256)), dim3(256), 0, ctx->stream, nodes, ix->ids.as<uint64_t>(),
                         (uint64_t)Bs * k, oi);
    } else {
      RefineArgs r{};
      r.queries = qs;
      if (rpad != d) {
        HIPCHK(ctx, S.qpad.ensure((size_t)Bs * rpad * 4));
        hipLaunchKernelGGL(sq8_pad_queries_kernel, dim3(cdiv((uint64_t)Bs * rpad, 256)), dim3(256), 0, ctx->stream, qs, d, rpad, (uint64_t)Bs,
                           S.qpad.as<float>());
        r.queries = S.qpad.as<float>();
      }
      if (decoded) {
        HIPCHK(ctx, S.decoded.ensure((size_t)Bs * kk * rpad * 4));
        hipLaunchKernelGGL(sq8_decode_cand_kernel, dim3(cdiv((uint64_t)Bs * kk * rpad, 256)), dim3(256), 0, ctx->stream, ix->codes.as<uint4>(),
                           ix->info.as<uint4>(), ksteps, d, rpad, nodes, counts, Bs, kk, S.decoded.as<float>());
        r.rows = S.decoded.p;
        r.local = 1;
      } else {
        r.rows = ix->store->data;
      }
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
      if (!decoded && ix->store->f16()) launch_refine<half_t>(ctx, r);
      else launch_refine<float>(ctx, r);
    }
    HIPCHK(ctx, hipGetLastError());
  }
  return FVDB_OK;
}

int fvdb_sq8_index_search(fvdb_sq8_index* ix, const float* q, uint32_t B, uint32_t k, uint32_t fetch_k, int refine_mode,
                          const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t* out_ids, float* out_dist, uint32_t* out_counts) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->ctx;
  if (B == 0) return FVDB_OK;
  if (!q || !out_ids || !out_dist || !out_counts) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (n_allowed && !allowed_ids) FAIL(ctx, FVDB_E_INVALID, "null allow-set");
  int rc = check_search(ix, ctx, k, fetch_k, refine_mode);
  if (rc) return rc;
  rc = sq8_check_rows(ctx, q, B, ix->d);  // a query is encoded by the rows' rule
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Sq8Slot& S = ix->slots[0];
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
  rc = fvdb_sq8_index_search_dev_slot(ix, ctx, 0, S.q.as<float>(), B, k, fetch_k, refine_mode, dead_dev, oi, od, oc);
  if (rc) return rc;
  HIPCHK(ctx, download(ctx, out_ids, oi, (size_t)B * k * 8));
  HIPCHK(ctx, download(ctx, out_dist, od, (size_t)B * k * 4));
  HIPCHK(ctx, download(ctx, out_counts, oc, (size_t)B * 4));
  return FVDB_OK;
}

}  // extern "C"
