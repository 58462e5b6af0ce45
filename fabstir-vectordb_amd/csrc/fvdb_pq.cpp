// fvdb_pq.cpp — product quantization behind the C ABI (include/fvdb.h, "product quantization"):
// the quantizer (train, encode, decode), the codes-only index and its ADC and refined search.  A translation unit of its
// own: the kernels are kernels_pq.h, the shared pieces (WaveTopK, flat_merge_kernel, the row scorer) come from their
// headers unchanged, and the refine rows live in an fvdb_store reached through the C ABI.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "fvdb_internal.h"
#include "common.h"
#include "kernels_pq.h"

using namespace fvdb;

namespace {

constexpr uint32_t kPqSlots = 16;
constexpr uint32_t kPqSubBatch = 8192;      // queries of one launch chain (bounds the tables and the partial lists)
constexpr uint32_t kPqMinSliceBlocks = 8;   // 512 rows: a slice shorter than this does not pay for its partial list

uint64_t sm64(uint64_t x) {  // one output of SplitMix64 from state x
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int pq_check_finite(fvdb_ctx* ctx, const float* x, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (!std::isfinite(x[i])) FAIL(ctx, FVDB_E_NONFINITE, "non-finite input value");
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

}  // namespace

struct PqSlot {
  DBuf q, qpad, tables, part, nodes, dist, counts, dead, out_ids;
};

struct fvdb_pq_index {
  fvdb_pq* pq = nullptr;
  uint64_t version = 0;
  int refine = FVDB_PQ_NO_REFINE;
  fvdb_store* store = nullptr;
  DBuf codes, ids, dead, s_in, s_rows;
  uint64_t n = 0, cap_blocks = 0, live = 0;
  std::unordered_map<uint64_t, uint32_t> row_of;
  std::vector<uint8_t> h_dead;
  PqSlot slots[kPqSlots];
};

namespace {

void launch_encode(fvdb_pq* pq, fvdb_ctx* on, const PqEncodeArgs& a, uint32_t tiles) {
  const dim3 grid(cdiv(tiles, 4)), block(256);
  switch (pq->dmax) {
    case 8: hipLaunchKernelGGL(pq_encode_kernel<8>, grid, block, 0, on->stream, a); break;
    case 32: hipLaunchKernelGGL(pq_encode_kernel<32>, grid, block, 0, on->stream, a); break;
    default: hipLaunchKernelGGL(pq_encode_kernel<128>, grid, block, 0, on->stream, a); break;
  }
}

// rows already in HBM to [n][m] codes
int encode_flat_dev(fvdb_pq* pq, fvdb_ctx* on, const float* rows_dev, uint64_t n, uint8_t* out_codes_dev) {
  PqEncodeArgs a{};
  a.rows = rows_dev;
  a.books = pq->books.as<float>();
  a.g = pq->g;
  a.n = n;
  a.first = 0;
  a.flat = out_codes_dev;
  a.m16 = pq->m16();
  launch_encode(pq, on, a, cdiv(n, 64));
  HIPCHK(on, hipGetLastError());
  return FVDB_OK;
}

size_t book_floats(const PqGeom& g) { return (size_t)g.ka * g.d; }

int set_books(fvdb_pq* pq, const float* books, uint32_t ka) {
  fvdb_ctx* ctx = pq->ctx;
  pq->g.ka = ka;
  HIPCHK(ctx, upload(ctx, pq->books.p, books, book_floats(pq->g) * 4));
  pq->trained = true;
  ++pq->version;
  return FVDB_OK;
}

template <int QT, int KR>
int launch_scan(fvdb_ctx* on, const PqScanArgs& a, uint32_t lds, uint32_t* out_nodes, float* out_dist, uint32_t* out_counts) {
  if (a.slices) {
    // the attribute belongs to the function; every call sets what it needs
    HIPCHK(on, hipFuncSetAttribute((const void*)pq_adc_scan_kernel<QT, KR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((pq_adc_scan_kernel<QT, KR>), dim3(cdiv(a.B, QT), cdiv(a.slices, 4)), dim3(256), lds, on->stream, a);
  }
  hipLaunchKernelGGL((flat_merge_kernel<KR>), dim3(cdiv(a.B, 4)), dim3(256), 0, on->stream, a.part, a.slices, a.B, a.k, out_nodes, out_dist,
                     out_counts);
  HIPCHK(on, hipGetLastError());
  return FVDB_OK;
}

template <int KR>
int launch_scan_qt(uint32_t qt, fvdb_ctx* on, const PqScanArgs& a, uint32_t lds, uint32_t* out_nodes, float* out_dist, uint32_t* out_counts) {
  switch (qt) {
    case 4: return launch_scan<4, KR>(on, a, lds, out_nodes, out_dist, out_counts);
    case 2: return launch_scan<2, KR>(on, a, lds, out_nodes, out_dist, out_counts);
    default: return launch_scan<1, KR>(on, a, lds, out_nodes, out_dist, out_counts);
  }
}

template <typename RT>
void launch_refine(fvdb_ctx* on, const PqRefineArgs& r) {
  const dim3 grid(cdiv(r.B, 4)), block(256);
  if (r.k <= 64) hipLaunchKernelGGL((pq_refine_kernel<1, RT>), grid, block, 0, on->stream, r);
  else if (r.k <= 128) hipLaunchKernelGGL((pq_refine_kernel<2, RT>), grid, block, 0, on->stream, r);
  else hipLaunchKernelGGL((pq_refine_kernel<4, RT>), grid, block, 0, on->stream, r);
}

int index_usable(fvdb_pq_index* ix) {
  if (!ix) return FVDB_E_INVALID;
  if (ix->version != ix->pq->version) FAIL(ix->pq->ctx, FVDB_E_INVALID, "the quantizer's codebooks changed after the index was created");
  return FVDB_OK;
}

}  // namespace

extern "C" {

int fvdb_pq_create(fvdb_ctx* ctx, uint32_t d, uint32_t m, uint32_t ksub, fvdb_pq** out) {
  if (!ctx || !out) return FVDB_E_INVALID;
  *out = nullptr;
  if (d == 0 || m == 0 || ksub == 0) FAIL(ctx, FVDB_E_INVALID, "d, num_subspaces and num_centroids must be > 0");
  if (m > d) FAIL(ctx, FVDB_E_INVALID, "num_subspaces must not exceed the dimension");
  if (ksub > 256) FAIL(ctx, FVDB_E_UNSUPPORTED, "num_centroids must be <= 256: a code is one byte");
  if (d > kPqMaxDims) FAIL(ctx, FVDB_E_UNSUPPORTED, "product quantizer: d must be <= 2048");
  const uint32_t dsub = d / m, dlast = d - (m - 1) * dsub;
  if (dlast > kPqMaxSubDims) FAIL(ctx, FVDB_E_UNSUPPORTED, "product quantizer: a subspace holds at most 128 dims");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int lds = 0;
  HIPCHK(ctx, hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  fvdb_pq* pq = new (std::nothrow) fvdb_pq();
  if (!pq) return FVDB_E_OOM;
  pq->ctx = ctx;
  pq->g = PqGeom{d, m, dsub, 0};
  pq->ksub = ksub;
  pq->dmax = dlast <= 8 ? 8 : (dlast <= 32 ? 32 : 128);
  const char* e = getenv("FVDB_PQ_TABLE_PAD");  // the measured alternative of DESIGN.md section 9w
  pq->pad = e && atoi(e) ? 1 : 0;
  pq->lds_limit = (uint32_t)lds;
  if (pq->books.exact((size_t)ksub * d * 4) != hipSuccess) {
    delete pq;
    FAIL(ctx, FVDB_E_OOM, "codebook allocation failed");
  }
  *out = pq;
  return FVDB_OK;
}

void fvdb_pq_destroy(fvdb_pq* pq) {
  if (!pq) return;
  (void)hipSetDevice(pq->ctx->device);
  (void)hipStreamSynchronize(pq->ctx->stream);
  delete pq;
}

int fvdb_pq_info(fvdb_pq* pq, fvdb_pq_info_t* out) {
  if (!pq || !out) return FVDB_E_INVALID;
  memset(out, 0, sizeof(*out));
  out->d = pq->g.d;
  out->m = pq->g.m;
  out->ksub = pq->ksub;
  out->ksub_actual = pq->g.ka;
  out->trained = pq->trained;
  out->dsub = pq->g.dsub;
  out->dsub_last = pq->g.dims(pq->g.m - 1);
  out->m_padded = pq->m16() * 16;
  out->table_stride = pq->trained ? pq->ts() : 0;
  out->queries_per_workgroup = pq->trained ? pq->qt() : 0;
  out->lds_bytes = out->queries_per_workgroup * pq->g.m * out->table_stride * 4;
  out->lds_limit = pq->lds_limit;
  out->min_slice_rows = kPqMinSliceBlocks * 64;
  out->max_d = kPqMaxDims;
  out->max_sub_dims = kPqMaxSubDims;
  return FVDB_OK;
}

int fvdb_pq_set_codebooks(fvdb_pq* pq, const float* books, uint32_t ksub_actual) {
  if (!pq) return FVDB_E_INVALID;
  fvdb_ctx* ctx = pq->ctx;
  if (!books) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (ksub_actual == 0 || ksub_actual > pq->ksub) FAIL(ctx, FVDB_E_INVALID, "ksub_actual must be in 1..num_centroids");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return set_books(pq, books, ksub_actual);
}

int fvdb_pq_get_codebooks(fvdb_pq* pq, float* out_books) {
  if (!pq) return FVDB_E_INVALID;
  fvdb_ctx* ctx = pq->ctx;
  if (!pq->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "Index not trained");
  if (!out_books) FAIL(ctx, FVDB_E_INVALID, "null argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, download(ctx, out_books, pq->books.p, book_floats(pq->g) * 4));
  return FVDB_OK;
}

int fvdb_pq_train(fvdb_pq* pq, const float* rows, uint64_t n, uint32_t iterations, const uint32_t* init_rows, uint64_t seed) {
  if (!pq) return FVDB_E_INVALID;
  fvdb_ctx* ctx = pq->ctx;
  if (!rows) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (n == 0) FAIL(ctx, FVDB_E_INSUFFICIENT, "no training rows");
  if (n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "training set limited to 2^32-1 rows");
  const PqGeom g0 = pq->g;
  int rc = pq_check_finite(ctx, rows, n * g0.d);
  if (rc) return rc;
  const uint32_t ka = (uint32_t)std::min<uint64_t>(pq->ksub, n);
  const uint32_t m = g0.m;
  std::vector<uint32_t> picks((size_t)m * ka);
  if (init_rows) {
    for (size_t i = 0; i < picks.size(); ++i) {
      if (init_rows[i] >= n) FAIL(ctx, FVDB_E_INVALID, "init_rows names a row beyond the training set");
      picks[i] = init_rows[i];
    }
  } else {
    uint64_t t = 0;
    for (uint32_t j = 0; j < m; ++j) {
      std::unordered_set<uint32_t> seen;
      for (uint32_t c = 0; c < ka;) {
        const uint32_t r = (uint32_t)(sm64(seed + t++ * 0x9E3779B97F4A7C15ull) % n);
        if (seen.insert(r).second) picks[(size_t)j * ka + c++] = r;
      }
    }
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // the initial centroids: bit copies of the picked sub-vectors
  PqGeom g = g0;
  g.ka = ka;
  std::vector<float> books(book_floats(g));
  for (uint32_t j = 0; j < m; ++j)
    for (uint32_t c = 0; c < ka; ++c)
      memcpy(&books[g.book(j) + (size_t)c * g.dims(j)], rows + (size_t)picks[(size_t)j * ka + c] * g.d + g.off(j), g.dims(j) * 4);
  if (iterations) {
    HIPCHK(ctx, pq->s_rows.ensure(n * g.d * 4));
    HIPCHK(ctx, pq->s_codes.ensure(n * m));
    HIPCHK(ctx, pq->s_refill.ensure((size_t)m * ka * 4));
    HIPCHK(ctx, upload(ctx, pq->s_rows.p, rows, n * g.d * 4));
  }
  rc = set_books(pq, books.data(), ka);
  if (rc) return rc;
  std::vector<uint32_t> refill((size_t)m * ka);
  for (uint32_t it = 0; it < iterations; ++it) {
    for (uint32_t j = 0; j < m; ++j)
      for (uint32_t c = 0; c < ka; ++c)
        refill[(size_t)j * ka + c] = (uint32_t)(sm64(seed + (((uint64_t)it * m + j) * 256 + c)) % n);
    HIPCHK(ctx, upload(ctx, pq->s_refill.p, refill.data(), refill.size() * 4));
    rc = encode_flat_dev(pq, ctx, pq->s_rows.as<float>(), n, pq->s_codes.as<uint8_t>());
    if (rc) return rc;
    PqUpdateArgs u{};
    u.rows = pq->s_rows.as<float>();
    u.codes = pq->s_codes.as<uint8_t>();
    u.books = pq->books.as<float>();
    u.refill = pq->s_refill.as<uint32_t>();
    u.g = pq->g;
    u.n = n;
    hipLaunchKernelGGL(pq_update_kernel, dim3(ka, m), dim3(128), 0, ctx->stream, u);
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}

int fvdb_pq_encode_dev(fvdb_pq* pq, fvdb_ctx* on, const float* rows_dev, uint64_t n, uint8_t* out_codes_dev) {
  if (!pq) return FVDB_E_INVALID;
  fvdb_ctx* ctx = on ? on : pq->ctx;
  if (!pq->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "Index not trained");
  if (ctx->device != pq->ctx->device) FAIL(ctx, FVDB_E_INVALID, "context of another device");
  if (n == 0) return FVDB_OK;
  if (!rows_dev || !out_codes_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return encode_flat_dev(pq, ctx, rows_dev, n, out_codes_dev);
}

int fvdb_pq_decode_dev(fvdb_pq* pq, fvdb_ctx* on, const uint8_t* codes_dev, uint64_t n, float* out_rows_dev) {
  if (!pq) return FVDB_E_INVALID;
  fvdb_ctx* ctx = on ? on : pq->ctx;
  if (!pq->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "Index not trained");
  if (ctx->device != pq->ctx->device) FAIL(ctx, FVDB_E_INVALID, "context of another device");
  if (n == 0) return FVDB_OK;
  if (!codes_dev || !out_rows_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(pq_decode_kernel, dim3(cdiv(n * pq->g.d, 256)), dim3(256), 0, ctx->stream, codes_dev, pq->books.as<float>(), pq->g, n,
                     out_rows_dev);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int fvdb_pq_encode(fvdb_pq* pq, const float* rows, uint64_t n, uint8_t* out_codes) {
  if (!pq) return FVDB_E_INVALID;
  fvdb_ctx* ctx = pq->ctx;
  if (!pq->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "Index not trained");
  if (n == 0) return FVDB_OK;
  if (!rows || !out_codes) FAIL(ctx, FVDB_E_INVALID, "null argument");
  int rc = pq_check_finite(ctx, rows, n * pq->g.d);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, pq->s_rows.ensure(n * pq->g.d * 4));
  HIPCHK(ctx, pq->s_codes.ensure(n * pq->g.m));
  HIPCHK(ctx, upload(ctx, pq->s_rows.p, rows, n * pq->g.d * 4));
  rc = encode_flat_dev(pq, ctx, pq->s_rows.as<float>(), n, pq->s_codes.as<uint8_t>());
  if (rc) return rc;
  HIPCHK(ctx, download(ctx, out_codes, pq->s_codes.p, n * pq->g.m));
  return FVDB_OK;
}

int fvdb_pq_decode(fvdb_pq* pq, const uint8_t* codes, uint64_t n, float* out_rows) {
  if (!pq) return FVDB_E_INVALID;
  fvdb_ctx* ctx = pq->ctx;
  if (!pq->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "Index not trained");
  if (n == 0) return FVDB_OK;
  if (!codes || !out_rows) FAIL(ctx, FVDB_E_INVALID, "null argument");
  for (uint64_t i = 0; i < n * pq->g.m; ++i)
    if (codes[i] >= pq->g.ka) FAIL(ctx, FVDB_E_INVALID, "a code names a centroid the codebook does not hold");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, pq->s_codes.ensure(n * pq->g.m));
  HIPCHK(ctx, pq->s_rows.ensure(n * pq->g.d * 4));
  HIPCHK(ctx, upload(ctx, pq->s_codes.p, codes, n * pq->g.m));
  int rc = fvdb_pq_decode_dev(pq, ctx, pq->s_codes.as<uint8_t>(), n, pq->s_rows.as<float>());
  if (rc) return rc;
  HIPCHK(ctx, download(ctx, out_rows, pq->s_rows.p, n * pq->g.d * 4));
  return FVDB_OK;
}

// ---- the codes-only index --------------------------------------------------------------------------------------------
int fvdb_pq_index_create(fvdb_pq* pq, int refine_dtype, fvdb_pq_index** out) {
  if (!pq || !out) return FVDB_E_INVALID;
  *out = nullptr;
  fvdb_ctx* ctx = pq->ctx;
  if (!pq->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "Index not trained");
  if (refine_dtype != FVDB_PQ_NO_REFINE && refine_dtype != FVDB_F32 && refine_dtype != FVDB_F16)
    FAIL(ctx, FVDB_E_INVALID, "refine_dtype must be FVDB_PQ_NO_REFINE, FVDB_F32 or FVDB_F16");
  fvdb_pq_index* ix = new (std::nothrow) fvdb_pq_index();
  if (!ix) return FVDB_E_OOM;
  ix->pq = pq;
  ix->version = pq->version;
  ix->refine = refine_dtype;
  if (refine_dtype != FVDB_PQ_NO_REFINE) {
    const int rc = fvdb_store_create_ex(ctx, pq->g.d, 1024, refine_dtype, &ix->store);
    if (rc) {
      delete ix;
      return rc;
    }
  }
  *out = ix;
  return FVDB_OK;
}

void fvdb_pq_index_destroy(fvdb_pq_index* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->pq->ctx->device);
  (void)hipDeviceSynchronize();  // searches may be in flight on other contexts' streams
  if (ix->store) fvdb_store_destroy(ix->store);
  delete ix;
}

uint64_t fvdb_pq_index_rows(fvdb_pq_index* ix) { return ix ? ix->n : 0; }
uint64_t fvdb_pq_index_live(fvdb_pq_index* ix) { return ix ? ix->live : 0; }
uint64_t fvdb_pq_index_bytes(fvdb_pq_index* ix) {
  if (!ix) return 0;
  return (uint64_t)cdiv(ix->n, 64) * ix->pq->m16() * 1024 + ix->n * 12 + (ix->store ? fvdb_store_bytes(ix->store) : 0);
}

int fvdb_pq_index_add(fvdb_pq_index* ix, const uint64_t* ids, const float* rows, uint64_t n) {
  int rc = index_usable(ix);
  if (rc) return rc;
  fvdb_pq* pq = ix->pq;
  fvdb_ctx* ctx = pq->ctx;
  if (n == 0) return FVDB_OK;
  if (!ids || !rows) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (ix->n + n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "index limited to 2^32-1 rows");
  rc = pq_check_finite(ctx, rows, n * pq->g.d);
  if (rc) return rc;
  {
    std::unordered_set<uint64_t> seen;
    for (uint64_t i = 0; i < n; ++i)
      if (ix->row_of.count(ids[i]) || !seen.insert(ids[i]).second) FAIL(ctx, FVDB_E_DUPLICATE, "Vector already exists");
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint64_t blocks = cdiv(ix->n + n, 64);
  if (blocks > ix->cap_blocks) {  // code blocks and flags come zeroed: a lane beyond the last row reads code 0
    const uint64_t nb = std::max<uint64_t>(blocks, ix->cap_blocks + ix->cap_blocks / 2), ob = cdiv(ix->n, 64);
    const size_t wb = (size_t)pq->m16() * 1024;
    HIPCHK(ctx, grow_keeping(ix->codes, nb * wb, ob * wb, /*zero_rest=*/true, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->ids, nb * 64 * 8, ix->n * 8, /*zero_rest=*/false, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->dead, nb * 64 * 4, ix->n * 4, /*zero_rest=*/true, ctx->stream));
    ix->cap_blocks = nb;
  }
  HIPCHK(ctx, ix->s_in.ensure(n * pq->g.d * 4));
  HIPCHK(ctx, upload(ctx, ix->s_in.p, rows, n * pq->g.d * 4));
  PqEncodeArgs a{};
  a.rows = ix->s_in.as<float>();
  a.books = pq->books.as<float>();
  a.g = pq->g;
  a.n = n;
  a.first = ix->n;
  a.blocks = ix->codes.as<uint4>();
  a.m16 = pq->m16();
  launch_encode(pq, ctx, a, (uint32_t)(blocks - ix->n / 64));
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

int fvdb_pq_index_set_deleted(fvdb_pq_index* ix, const uint64_t* ids, uint64_t n, int flag) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->pq->ctx;
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
  hipLaunchKernelGGL(pq_set_flags_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, ix->s_rows.as<uint32_t>(), n, flag ? 1u : 0u,
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

int fvdb_pq_index_search_dev_slot(fvdb_pq_index* ix, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t k,
                                  uint32_t fetch_k, const uint32_t* dead_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                                  uint32_t* out_counts_dev) {
  int rc = index_usable(ix);
  if (rc) return rc;
  fvdb_pq* pq = ix->pq;
  fvdb_ctx* ctx = on ? on : pq->ctx;
  if (slot >= kPqSlots) FAIL(ctx, FVDB_E_INVALID, "slot out of range");
  if (ctx->device != pq->ctx->device) FAIL(ctx, FVDB_E_INVALID, "context of another device");
  if (k == 0 || k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "ADC search: k must be in 1..FVDB_MAX_K");
  if (fetch_k) {
    if (!ix->store) FAIL(ctx, FVDB_E_INVALID, "fetch_k needs an index created with refine rows");
    if (fetch_k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "refined search: fetch_k must be <= FVDB_MAX_K");
    if (k > fetch_k) FAIL(ctx, FVDB_E_INVALID, "refined search: k must be <= fetch_k");
  }
  const uint32_t qt = pq->qt();
  if (!qt) FAIL(ctx, FVDB_E_UNSUPPORTED, "ADC search: one query's tables (m x table_stride x 4 bytes) exceed the device's LDS");
  if (!q_dev || !out_ids_dev || !out_dist_dev || !out_counts_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  PqSlot& S = ix->slots[slot];
  const PqGeom g = pq->g;
  const uint32_t kk = fetch_k ? fetch_k : k;
  const uint32_t n = (uint32_t)ix->n, blocks = cdiv(n, 64);
  const uint32_t lds = qt * g.m * pq->ts() * 4;
  for (uint32_t b0 = 0; b0 < B; b0 += kPqSubBatch) {
    const uint32_t Bs = std::min(kPqSubBatch, B - b0);
    const float* qs = q_dev + (size_t)b0 * g.d;
    PqScanArgs a{};
    a.codes = ix->codes.as<uint4>();
    a.dead = dead_dev ? dead_dev : ix->dead.as<uint32_t>();
    a.n = n;
    a.m = g.m;
    a.m16 = pq->m16();
    a.ka = g.ka;
    a.ts = pq->ts();
    a.B = Bs;
    a.k = kk;
    if (n) {  // enough (group, slice) waves to fill the device at a small batch, no slice under kPqMinSliceBlocks
      const uint32_t groups = cdiv(Bs, qt);
      const uint32_t want = std::max<uint32_t>(1, std::min<uint32_t>(cdiv(blocks, kPqMinSliceBlocks), 4 * cdiv(2 * (uint32_t)ctx->num_cus, groups)));
      a.slice_blocks = cdiv(blocks, want);
      a.slices = cdiv(blocks, a.slice_blocks);
      HIPCHK(ctx, S.tables.ensure((size_t)Bs * g.m * g.ka * 4));
      hipLaunchKernelGGL(pq_table_kernel, dim3(g.m, Bs), dim3(256), 0, ctx->stream, qs, pq->books.as<float>(), g, S.tables.as<float>());
    }
    a.tables = S.tables.as<float>();
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
    const int kr = kk <= 64 ? 1 : (kk <= 128 ? 2 : 4);
    switch (kr) {
      case 1: rc = launch_scan_qt<1>(qt, ctx, a, lds, nodes, dist, counts); break;
      case 2: rc = launch_scan_qt<2>(qt, ctx, a, lds, nodes, dist, counts); break;
      default: rc = launch_scan_qt<4>(qt, ctx, a, lds, nodes, dist, counts); break;
    }
    if (rc) return rc;
    uint64_t* oi = out_ids_dev + (size_t)b0 * k;
    if (!fetch_k) {
      hipLaunchKernelGGL(pq_map_ids_kernel, dim3(cdiv((uint64_t)Bs * k, 256)), dim3(256), 0, ctx->stream, nodes, ix->ids.as<uint64_t>(),
                         (uint64_t)Bs * k, oi);
    } else {
      fvdb_store* st = ix->store;
      PqRefineArgs r{};
      r.rows = st->data;
      r.queries = qs;
      if (st->dpad != g.d) {
        HIPCHK(ctx, S.qpad.ensure((size_t)Bs * st->dpad * 4));
        hipLaunchKernelGGL(pq_pad_queries_kernel, dim3(cdiv((uint64_t)Bs * st->dpad, 256)), dim3(256), 0, ctx->stream, qs, g.d, st->dpad,
                           (uint64_t)Bs, S.qpad.as<float>());
        r.queries = S.qpad.as<float>();
      }
      r.cand = nodes;
      r.cand_cnt = counts;
      r.ids = ix->ids.as<uint64_t>();
      r.dpad = st->dpad;
      r.B = Bs;
      r.fk = kk;
      r.k = k;
      r.out_ids = oi;
      r.out_dist = out_dist_dev + (size_t)b0 * k;
      r.out_counts = out_counts_dev + b0;
      if (st->f16()) launch_refine<half_t>(ctx, r);
      else launch_refine<float>(ctx, r);
    }
    HIPCHK(ctx, hipGetLastError());
  }
  return FVDB_OK;
}

int fvdb_pq_index_search(fvdb_pq_index* ix, const float* q, uint32_t B, uint32_t k, uint32_t fetch_k, const uint64_t* allowed_ids,
                         uint64_t n_allowed, uint64_t* out_ids, float* out_dist, uint32_t* out_counts) {
  int rc = index_usable(ix);
  if (rc) return rc;
  fvdb_pq* pq = ix->pq;
  fvdb_ctx* ctx = pq->ctx;
  if (B == 0) return FVDB_OK;
  if (!q || !out_ids || !out_dist || !out_counts) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (n_allowed && !allowed_ids) FAIL(ctx, FVDB_E_INVALID, "null allow-set");
  if (k == 0 || k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "ADC search: k must be in 1..FVDB_MAX_K");
  rc = pq_check_finite(ctx, q, (uint64_t)B * pq->g.d);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  PqSlot& S = ix->slots[0];
  HIPCHK(ctx, S.q.ensure((size_t)B * pq->g.d * 4));
  HIPCHK(ctx, S.out_ids.ensure((size_t)B * k * 16 + (size_t)B * 4));
  HIPCHK(ctx, upload(ctx, S.q.p, q, (size_t)B * pq->g.d * 4));
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
  uint64_t* oi = S.out_ids.as<uint64_t>();
  float* od = (float*)(oi + (size_t)B * k);
  uint32_t* oc = (uint32_t*)(od + (size_t)B * k);
  rc = fvdb_pq_index_search_dev_slot(ix, ctx, 0, S.q.as<float>(), B, k, fetch_k, dead_dev, oi, od, oc);
  if (rc) return rc;
  HIPCHK(ctx, download(ctx, out_ids, oi, (size_t)B * k * 8));
  HIPCHK(ctx, download(ctx, out_dist, od, (size_t)B * k * 4));
  HIPCHK(ctx, download(ctx, out_counts, oc, (size_t)B * 4));
  return FVDB_OK;
}

}  // extern "C"
