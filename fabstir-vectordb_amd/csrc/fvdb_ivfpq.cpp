// fvdb_ivfpq.cpp — the inverted file over PQ codes behind the C ABI (include/fvdb.h, "IVF over PQ codes"; DESIGN.md
// section 9zc).  A translation unit of its own: the scan is kernels_ivfpq.h, the tables, the fold, the refine and the id
// map are kernels_pq.h's and the merge kernels_flat.h's, all unchanged.  The codebooks belong to an fvdb_pq the caller
// owns; centroids, assignment and the coarse ranking to an fvdb_ivf without rows, reached through the C ABI like the
// refine rows' fvdb_store.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "fvdb_internal.h"
#include "common.h"
#include "kernels_ivfpq.h"
#include "kernels_ivfrpq.h"  // residual codes: the fused encode, the inner-product tables, the base

using namespace fvdb;

namespace {

constexpr uint32_t kSlots = 16;
constexpr size_t kArenaBytes = 256u << 20;  // partial lists of one launch chain
constexpr size_t kTableBytes = 64u << 20;   // ADC tables of one launch chain
constexpr uint32_t kMaxSubBatch = 8192;     // queries of one launch chain whatever the arenas allow (the grids' second dimension)

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

void launch_fill(fvdb_ctx* on, void* p, uint64_t words, uint32_t v) {
  if (words) hipLaunchKernelGGL(ivfpq_fill_kernel, dim3(cdiv(words, 256)), dim3(256), 0, on->stream, (uint32_t*)p, words, v);
}

int check_finite(fvdb_ctx* ctx, const float* x, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (!std::isfinite(x[i])) FAIL(ctx, FVDB_E_NONFINITE, "non-finite input value");
  return FVDB_OK;
}

}  // namespace

struct IvfPqSlot {
  DBuf q, qpad, probes, tables, part, nodes, dist, counts, dead, out, stats;
  DBuf base, qres;  // residual codes: base[Bs][np]; the queries at the centroid copy's row stride where it is not d
  uint32_t last_S = 0;
};

struct fvdb_ivfpq {
  fvdb_ctx* ctx = nullptr;
  fvdb_pq* pq = nullptr;
  uint64_t version = 0;  // the quantizer's at creation
  uint32_t nlist = 0;
  int refine = FVDB_PQ_NO_REFINE;
  bool trained = false;         // centroids are set
  fvdb_ivf* ivf = nullptr;      // centroids only: it never receives rows
  fvdb_store* store = nullptr;  // refine rows, store row = seq
  DBuf codes, dead, seq_of_row;  // per pool block / pool row
  DBuf row_of_seq, ids;          // per seq
  DBuf list_off, list_len, list_blocks, s_in, s_flat, s_rows;
  // Residual codes (fvdb_ivfrpq_create; section 9zd): a row's codes encode row - centroid, and the pool carries one f32
  // row term beside dead and seq_of_row.  The encode and the base kernel read the index's own copy of the centroids,
  // [nlist][dpad] with dpad = d rounded up to 4 and zeros beyond d (the fvdb_ivf's table is behind the C ABI).
  bool residual = false;
  uint32_t dpad = 0;
  DBuf term_of_row, cent, s_cluster, s_term;
  uint64_t n = 0, live = 0, blocks = 0, cap_blocks = 0, cap_seq = 0;
  std::vector<std::vector<uint32_t>> h_blocks;  // per list, in fill order
  std::vector<uint32_t> h_len, h_row_of_seq;
  std::vector<uint8_t> h_dead;                  // per seq
  std::unordered_map<uint64_t, uint32_t> seq_of;
  IvfPqSlot slots[kSlots];
  int last_slot = -1;
  fvdb_ctx* last_ctx = nullptr;
  // Queries of a scan workgroup.  A wave scans for ONE query, so a larger QT buys nothing but fewer table loads a
  // workgroup, and costs resident waves: the largest of 4, 2, 1 whose tables take at most half of lds_limit, which is the
  // largest LDS block of ONE workgroup (hipDeviceAttributeMaxSharedMemoryPerBlock), not the CU's LDS; on gfx950 the two
  // are equal, so there two workgroups fit a CU.  Where none does, section 9w's rule: the largest whose tables fit once.
  uint32_t qt() const {
    const uint64_t per = (uint64_t)pq->g.m * pq->ts() * 4;
    for (uint32_t q = 4; q; q >>= 1)
      if (2 * per * q <= pq->lds_limit) return q;
    return pq->qt();
  }
};

namespace {

template <int QT, int KR, bool RES>
int launch_scan(fvdb_ctx* on, const IvfPqScanArgs& a, uint32_t lds, uint32_t* out_nodes, float* out_dist, uint32_t* out_counts) {
  // the attribute belongs to the function; every call sets what it needs
  HIPCHK(on, hipFuncSetAttribute((const void*)ivfpq_scan_kernel<QT, KR, kIvfPqChains, RES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((ivfpq_scan_kernel<QT, KR, kIvfPqChains, RES>), dim3(cdiv(a.B, QT), cdiv(a.S, 4 / QT)), dim3(256), lds, on->stream, a);
  hipLaunchKernelGGL((flat_merge_kernel<KR>), dim3(cdiv(a.B, 4)), dim3(256), 0, on->stream, a.part, a.S, a.B, a.k, out_nodes, out_dist, out_counts);
  HIPCHK(on, hipGetLastError());
  return FVDB_OK;
}

// a.base set = residual codes: the RES instantiation
template <int KR>
int launch_scan_qt(uint32_t qt, fvdb_ctx* on, const IvfPqScanArgs& a, uint32_t lds, uint32_t* out_nodes, float* out_dist, uint32_t* out_counts) {
  if (a.base) {
    switch (qt) {
      case 4: return launch_scan<4, KR, true>(on, a, lds, out_nodes, out_dist, out_counts);
      case 2: return launch_scan<2, KR, true>(on, a, lds, out_nodes, out_dist, out_counts);
      default: return launch_scan<1, KR, true>(on, a, lds, out_nodes, out_dist, out_counts);
    }
  }
  switch (qt) {
    case 4: return launch_scan<4, KR, false>(on, a, lds, out_nodes, out_dist, out_counts);
    case 2: return launch_scan<2, KR, false>(on, a, lds, out_nodes, out_dist, out_counts);
    default: return launch_scan<1, KR, false>(on, a, lds, out_nodes, out_dist, out_counts);
  }
}

// add, residual codes: rows (in HBM) and their lists to flat codes and row terms
void launch_residual_encode(fvdb_pq* pq, fvdb_ctx* on, const IvfRpqEncodeArgs& a) {
  const dim3 grid(cdiv(cdiv(a.n, 64), 4)), block(256);
  switch (pq->dmax) {
    case 8: hipLaunchKernelGGL(ivfrpq_encode_kernel<8>, grid, block, 0, on->stream, a); break;
    case 32: hipLaunchKernelGGL(ivfrpq_encode_kernel<32>, grid, block, 0, on->stream, a); break;
    default: hipLaunchKernelGGL(ivfrpq_encode_kernel<128>, grid, block, 0, on->stream, a); break;
  }
}

// search, residual codes: base[Bs][np] and the inner-product tables of a sub-batch (probes: the sub-batch's rows)
int launch_residual_tables(fvdb_ivfpq* ix, fvdb_ctx* ctx, IvfPqSlot& S, const float* qs, uint32_t Bs, uint32_t np, const uint32_t* probes) {
  const PqGeom g = ix->pq->g;
  const float* qp = qs;
  if (ix->dpad != g.d) {
    HIPCHK(ctx, S.qres.ensure((size_t)Bs * ix->dpad * 4));
    hipLaunchKernelGGL(pq_pad_queries_kernel, dim3(cdiv((uint64_t)Bs * ix->dpad, 256)), dim3(256), 0, ctx->stream, qs, g.d, ix->dpad, (uint64_t)Bs,
                       S.qres.as<float>());
    qp = S.qres.as<float>();
  }
  HIPCHK(ctx, S.base.ensure((size_t)Bs * np * 4));
  hipLaunchKernelGGL(ivfrpq_base_kernel, dim3(cdiv(cdiv(np, 16), 4), Bs), dim3(256), 0, ctx->stream, qp, ix->cent.as<float>(), ix->dpad, probes, Bs,
                     np, ix->nlist, S.base.as<float>());
  hipLaunchKernelGGL(ivfrpq_table_kernel<(int)kIvfRpqTableQueries>, dim3(g.m, cdiv(Bs, kIvfRpqTableQueries)), dim3(256), 0, ctx->stream, qs,
                     ix->pq->books.as<float>(), g, Bs, S.tables.as<float>());
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// residual codes: the index's own padded copy of the centroids, after they were trained or set
int copy_centroids(fvdb_ivfpq* ix) {
  fvdb_ctx* ctx = ix->ctx;
  const uint32_t d = ix->pq->g.d;
  std::vector<float> c((size_t)ix->nlist * d), padded((size_t)ix->nlist * ix->dpad, 0.0f);
  const int rc = fvdb_ivf_get_centroids(ix->ivf, c.data());
  if (rc) return rc;
  for (uint32_t L = 0; L < ix->nlist; ++L) memcpy(&padded[(size_t)L * ix->dpad], &c[(size_t)L * d], (size_t)d * 4);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, upload(ctx, ix->cent.p, padded.data(), padded.size() * 4));
  return FVDB_OK;
}

template <typename RT>
void launch_refine(fvdb_ctx* on, const PqRefineArgs& r) {
  const dim3 grid(cdiv(r.B, 4)), block(256);
  if (r.k <= 64) hipLaunchKernelGGL((pq_refine_kernel<1, RT>), grid, block, 0, on->stream, r);
  else if (r.k <= 128) hipLaunchKernelGGL((pq_refine_kernel<2, RT>), grid, block, 0, on->stream, r);
  else hipLaunchKernelGGL((pq_refine_kernel<4, RT>), grid, block, 0, on->stream, r);
}

// S: slices of a query's probe ranks, so that (groups x S) covers about twice the CUs; a multiple of the slices a
// workgroup's own waves take, at most np
uint32_t slices_for(uint32_t groups, uint32_t qt, uint32_t np, uint32_t cus) {
  const uint32_t spw = 4 / qt;
  const uint32_t want = cdiv(cdiv(2 * cus, groups), spw) * spw;
  return std::max<uint32_t>(1, std::min(np, want));
}

int index_usable(fvdb_ivfpq* ix, fvdb_ctx* ctx) {
  if (!ix->pq->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "Index not trained");
  if (ix->version != ix->pq->version) FAIL(ctx, FVDB_E_INVALID, "the quantizer's codebooks changed after the index was created");
  return FVDB_OK;
}

int check_search(fvdb_ivfpq* ix, fvdb_ctx* ctx, uint32_t k, uint32_t nprobe, uint32_t fetch_k) {
  int rc = index_usable(ix, ctx);
  if (rc) return rc;
  if (!ix->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "index not trained");
  if (k == 0 || k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "IVF-PQ search: k must be in 1..FVDB_MAX_K");
  if (fetch_k) {
    if (!ix->store) FAIL(ctx, FVDB_E_INVALID, "fetch_k needs an index created with refine rows");
    if (fetch_k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "refined search: fetch_k must be <= FVDB_MAX_K");
    if (k > fetch_k) FAIL(ctx, FVDB_E_INVALID, "refined search: k must be <= fetch_k");
  }
  if (nprobe == 0) FAIL(ctx, FVDB_E_INVALID, "nprobe must be > 0");
  if (!ix->qt()) FAIL(ctx, FVDB_E_UNSUPPORTED, "ADC search: one query's tables (m x table_stride x 4 bytes) exceed the device's LDS");
  return FVDB_OK;
}

// the list table of the rows present, rebuilt whole: n / 64 words
int upload_lists(fvdb_ivfpq* ix) {
  fvdb_ctx* ctx = ix->ctx;
  std::vector<uint32_t> off(ix->nlist + 1, 0), flat;
  flat.reserve(ix->blocks);
  for (uint32_t L = 0; L < ix->nlist; ++L) {
    flat.insert(flat.end(), ix->h_blocks[L].begin(), ix->h_blocks[L].end());
    off[L + 1] = (uint32_t)flat.size();
  }
  HIPCHK(ctx, ix->list_blocks.ensure(std::max<size_t>(flat.size() * 4, 4)));
  HIPCHK(ctx, upload(ctx, ix->list_off.p, off.data(), off.size() * 4));
  HIPCHK(ctx, upload(ctx, ix->list_len.p, ix->h_len.data(), (size_t)ix->nlist * 4));
  HIPCHK(ctx, upload(ctx, ix->list_blocks.p, flat.data(), flat.size() * 4));
  return FVDB_OK;
}

// both kinds of index: fvdb_ivfpq_create and fvdb_ivfrpq_create
int create_index(fvdb_pq* pq, uint32_t nlist, int refine_dtype, bool residual, fvdb_ivfpq** out) {
  if (!pq || !out) return FVDB_E_INVALID;
  *out = nullptr;
  fvdb_ctx* ctx = pq->ctx;
  if (!pq->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "Index not trained");
  if (nlist == 0) FAIL(ctx, FVDB_E_INVALID, "nlist must be > 0");
  if (nlist > kIvfPqMaxLists) FAIL(ctx, FVDB_E_UNSUPPORTED, "IVF-PQ: nlist must be <= 16384");
  if (refine_dtype != FVDB_PQ_NO_REFINE && refine_dtype != FVDB_F32 && refine_dtype != FVDB_F16)
    FAIL(ctx, FVDB_E_INVALID, "refine_dtype must be FVDB_PQ_NO_REFINE, FVDB_F32 or FVDB_F16");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  fvdb_ivfpq* ix = new (std::nothrow) fvdb_ivfpq();
  if (!ix) return FVDB_E_OOM;
  ix->ctx = ctx;
  ix->pq = pq;
  ix->version = pq->version;
  ix->nlist = nlist;
  ix->refine = refine_dtype;
  ix->h_blocks.assign(nlist, {});
  ix->h_len.assign(nlist, 0);
  int rc = fvdb_ivf_create(ctx, pq->g.d, nlist, &ix->ivf);
  if (!rc && refine_dtype != FVDB_PQ_NO_REFINE) rc = fvdb_store_create_ex(ctx, pq->g.d, 1024, refine_dtype, &ix->store);
  if (!rc && (ix->list_off.exact((size_t)(nlist + 1) * 4) != hipSuccess || ix->list_len.exact((size_t)nlist * 4) != hipSuccess)) rc = FVDB_E_OOM;
  ix->residual = residual;
  ix->dpad = (pq->g.d + 3u) & ~3u;
  if (!rc && residual && ix->cent.exact((size_t)nlist * ix->dpad * 4) != hipSuccess) rc = FVDB_E_OOM;
  if (!rc) rc = upload_lists(ix);
  if (rc) {
    fvdb_ivfpq_destroy(ix);
    return rc;
  }
  *out = ix;
  return FVDB_OK;
}

}  // namespace

extern "C" {

int fvdb_ivfpq_create(fvdb_pq* pq, uint32_t nlist, int refine_dtype, fvdb_ivfpq** out) {
  return create_index(pq, nlist, refine_dtype, /*residual=*/false, out);
}

int fvdb_ivfrpq_create(fvdb_pq* pq, uint32_t nlist, int refine_dtype, fvdb_ivfpq** out) {
  return create_index(pq, nlist, refine_dtype, /*residual=*/true, out);
}

void fvdb_ivfpq_destroy(fvdb_ivfpq* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->ctx->device);
  (void)hipDeviceSynchronize();  // searches may be in flight on other contexts' streams
  if (ix->store) fvdb_store_destroy(ix->store);
  if (ix->ivf) fvdb_ivf_destroy(ix->ivf);
  delete ix;
}

int fvdb_ivfpq_train(fvdb_ivfpq* ix, const float* x, uint64_t n, uint32_t max_iterations, uint64_t seed, fvdb_train_result* out) {
  if (!ix) return FVDB_E_INVALID;
  if (ix->n) FAIL(ix->ctx, FVDB_E_UNSUPPORTED, "IVF-PQ: the centroids of an index with rows cannot be replaced");
  int rc = fvdb_ivf_train(ix->ivf, x, n, max_iterations, seed, out);
  if (!rc && ix->residual) rc = copy_centroids(ix);
  if (!rc) ix->trained = true;
  return rc;
}

int fvdb_ivfpq_set_centroids(fvdb_ivfpq* ix, const float* centroids) {
  if (!ix) return FVDB_E_INVALID;
  if (ix->n) FAIL(ix->ctx, FVDB_E_UNSUPPORTED, "IVF-PQ: the centroids of an index with rows cannot be replaced");
  int rc = fvdb_ivf_set_centroids(ix->ivf, centroids);
  if (!rc && ix->residual) rc = copy_centroids(ix);
  if (!rc) ix->trained = true;
  return rc;
}

int fvdb_ivfpq_get_centroids(fvdb_ivfpq* ix, float* out) {
  if (!ix) return FVDB_E_INVALID;
  if (!out) FAIL(ix->ctx, FVDB_E_INVALID, "null argument");
  return fvdb_ivf_get_centroids(ix->ivf, out);
}

uint64_t fvdb_ivfpq_rows(fvdb_ivfpq* ix) { return ix ? ix->n : 0; }
uint64_t fvdb_ivfpq_live(fvdb_ivfpq* ix) { return ix ? ix->live : 0; }
uint64_t fvdb_ivfpq_bytes(fvdb_ivfpq* ix) {
  if (!ix) return 0;
  return ix->blocks * ((uint64_t)ix->pq->m16() * 1024 + 64 * 8 + 4 + (ix->residual ? 64 * 4 : 0)) + ix->n * 12 +
         (uint64_t)(2 * ix->nlist + 1) * 4 + (ix->store ? fvdb_store_bytes(ix->store) : 0);
}

int fvdb_ivfpq_list_sizes(fvdb_ivfpq* ix, uint64_t* out) {
  if (!ix) return FVDB_E_INVALID;
  if (!out) FAIL(ix->ctx, FVDB_E_INVALID, "null argument");
  for (uint32_t L = 0; L < ix->nlist; ++L) out[L] = ix->h_len[L];
  return FVDB_OK;
}

int fvdb_ivfpq_info(fvdb_ivfpq* ix, fvdb_ivfpq_info_t* out) {
  if (!ix || !out) return FVDB_E_INVALID;
  memset(out, 0, sizeof(*out));
  const fvdb_pq* pq = ix->pq;
  out->d = pq->g.d;
  out->m = pq->g.m;
  out->ksub_actual = pq->g.ka;
  out->nlist = ix->nlist;
  out->block_rows = 64;
  out->queries_per_workgroup = pq->trained ? ix->qt() : 0;
  out->lds_bytes = out->queries_per_workgroup * pq->g.m * pq->ts() * 4;
  out->lds_limit = pq->lds_limit;
  out->words_in_flight = kIvfPqAhead;
  out->max_k = FVDB_MAX_K;
  out->max_nlist = kIvfPqMaxLists;
  out->pool_blocks = ix->blocks;
  if (ix->last_slot >= 0) {
    fvdb_ctx* ctx = ix->last_ctx;
    const IvfPqSlot& S = ix->slots[ix->last_slot];
    unsigned long long w[2] = {0, 0};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, download(ctx, w, S.stats.p, sizeof(w)));
    out->last_slices = S.last_S;
    out->rows_scored = w[0];
    out->pairs = w[1];
  }
  return FVDB_OK;
}

int fvdb_ivfpq_add(fvdb_ivfpq* ix, const uint64_t* ids, const float* rows, uint64_t n) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->ctx;
  fvdb_pq* pq = ix->pq;
  int rc = index_usable(ix, ctx);
  if (rc) return rc;
  if (n == 0) return FVDB_OK;
  if (!ids || !rows) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (!ix->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "index not trained");
  if (ix->n + n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "index limited to 2^32-1 rows");
  const uint32_t d = pq->g.d, m = pq->g.m, m16 = pq->m16();
  rc = check_finite(ctx, rows, n * d);
  if (rc) return rc;
  {
    std::unordered_set<uint64_t> seen;
    for (uint64_t i = 0; i < n; ++i)
      if (ix->seq_of.count(ids[i]) || !seen.insert(ids[i]).second) FAIL(ctx, FVDB_E_DUPLICATE, "Vector already exists");
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> cluster(n), dest(n);
  rc = fvdb_ivf_assign(ix->ivf, rows, n, cluster.data());
  if (rc) return rc;
  // destinations in add order: a list's last partial block first, then fresh blocks; committed once everything is in HBM
  std::vector<uint32_t> len = ix->h_len;
  std::vector<std::pair<uint32_t, uint32_t>> fresh;  // (list, block) in the order taken
  std::vector<uint32_t> tail(ix->nlist);             // the block a list is filling
  for (uint32_t L = 0; L < ix->nlist; ++L) tail[L] = ix->h_blocks[L].empty() ? 0u : ix->h_blocks[L].back();
  uint64_t blocks = ix->blocks;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t L = cluster[i], pos = len[L]++;
    if ((pos & 63u) == 0) {
      tail[L] = (uint32_t)blocks++;
      fresh.emplace_back(L, tail[L]);
    }
    dest[i] = tail[L] * 64u + (pos & 63u);
  }
  if (blocks * 64 >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "pool limited to 2^32-1 rows");
  if (blocks > ix->cap_blocks) {  // code blocks come zeroed (a lane without a row reads code 0), the new blocks' rows dead until placed
    const uint64_t nb = std::max<uint64_t>(blocks, ix->cap_blocks + ix->cap_blocks / 2), ob = ix->blocks;
    const size_t wb = (size_t)m16 * 1024;
    HIPCHK(ctx, grow_keeping(ix->codes, nb * wb, ob * wb, /*zero_rest=*/true, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->seq_of_row, nb * 64 * 4, ob * 64 * 4, /*zero_rest=*/true, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->dead, nb * 64 * 4, ob * 64 * 4, /*zero_rest=*/false, ctx->stream));
    launch_fill(ctx, ix->dead.as<uint32_t>() + ob * 64, (nb - ob) * 64, 1u);
    if (ix->residual) HIPCHK(ctx, grow_keeping(ix->term_of_row, nb * 64 * 4, ob * 64 * 4, /*zero_rest=*/true, ctx->stream));
    ix->cap_blocks = nb;
  }
  if (ix->n + n > ix->cap_seq) {
    const uint64_t ns = std::max<uint64_t>(ix->n + n, ix->cap_seq + ix->cap_seq / 2);
    HIPCHK(ctx, grow_keeping(ix->row_of_seq, ns * 4, ix->n * 4, /*zero_rest=*/false, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->ids, ns * 8, ix->n * 8, /*zero_rest=*/false, ctx->stream));
    ix->cap_seq = ns;
  }
  HIPCHK(ctx, ix->s_in.ensure(n * d * 4));
  HIPCHK(ctx, ix->s_flat.ensure(n * m));
  HIPCHK(ctx, ix->s_rows.ensure(n * 4));
  HIPCHK(ctx, upload(ctx, ix->s_in.p, rows, n * d * 4));
  HIPCHK(ctx, upload(ctx, ix->s_rows.p, dest.data(), n * 4));
  // the quantizer's own encode to flat codes (residual codes: of row - centroid, with the row terms, in one kernel), then
  // the place kernel packs them into the destination blocks
  if (ix->residual) {
    HIPCHK(ctx, ix->s_cluster.ensure(n * 4));
    HIPCHK(ctx, ix->s_term.ensure(n * 4));
    HIPCHK(ctx, upload(ctx, ix->s_cluster.p, cluster.data(), n * 4));
    IvfRpqEncodeArgs e{};
    e.rows = ix->s_in.as<float>();
    e.cluster = ix->s_cluster.as<uint32_t>();
    e.cent = ix->cent.as<float>();
    e.books = pq->books.as<float>();
    e.g = pq->g;
    e.n = n;
    e.nlist = ix->nlist;
    e.dpad = ix->dpad;
    e.flat = ix->s_flat.as<uint8_t>();
    e.term = ix->s_term.as<float>();
    launch_residual_encode(pq, ctx, e);
    HIPCHK(ctx, hipGetLastError());
  } else {
    rc = fvdb_pq_encode_dev(pq, ctx, ix->s_in.as<float>(), n, ix->s_flat.as<uint8_t>());
    if (rc) return rc;
  }
  hipLaunchKernelGGL(ivfpq_place_kernel, dim3(cdiv(n * m16, 256)), dim3(256), 0, ctx->stream, ix->s_flat.as<uint8_t>(), ix->s_rows.as<uint32_t>(),
                     n, m, m16, (uint32_t)ix->n, ix->codes.as<uint4>(), ix->seq_of_row.as<uint32_t>(), ix->row_of_seq.as<uint32_t>(),
                     ix->residual ? ix->s_term.as<float>() : (const float*)nullptr, ix->term_of_row.as<float>());
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, upload(ctx, ix->ids.as<uint64_t>() + ix->n, ids, n * 8));
  if (ix->store) {
    uint64_t first = 0;
    rc = fvdb_store_append(ix->store, rows, n, &first);
    if (rc) return rc;
  }
  // the rows become candidates last: a call that failed above leaves their slots dead, as an unfilled slot is
  hipLaunchKernelGGL(ivfpq_live_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, ix->s_rows.as<uint32_t>(), n, ix->dead.as<uint32_t>());
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (const auto& f : fresh) ix->h_blocks[f.first].push_back(f.second);
  ix->h_len = std::move(len);
  ix->blocks = blocks;
  for (uint64_t i = 0; i < n; ++i) ix->seq_of.emplace(ids[i], (uint32_t)(ix->n + i));
  ix->h_row_of_seq.insert(ix->h_row_of_seq.end(), dest.begin(), dest.end());
  ix->h_dead.resize(ix->n + n, 0);
  ix->n += n;
  ix->live += n;
  return upload_lists(ix);
}

int fvdb_ivfpq_set_deleted(fvdb_ivfpq* ix, const uint64_t* ids, uint64_t n, int flag) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->ctx;
  if (n == 0) return FVDB_OK;
  if (!ids) FAIL(ctx, FVDB_E_INVALID, "null argument");
  std::vector<uint32_t> seqs(n);
  for (uint64_t i = 0; i < n; ++i) {
    const auto it = ix->seq_of.find(ids[i]);
    if (it == ix->seq_of.end()) FAIL(ctx, FVDB_E_NOT_FOUND, "Vector not found");
    seqs[i] = it->second;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, ix->s_rows.ensure(n * 4));
  HIPCHK(ctx, upload(ctx, ix->s_rows.p, seqs.data(), n * 4));
  hipLaunchKernelGGL(ivfpq_set_flags_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, ix->s_rows.as<uint32_t>(), n, flag ? 1u : 0u,
                     ix->row_of_seq.as<uint32_t>(), ix->dead.as<uint32_t>());
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const uint8_t f = flag ? 1 : 0;
  for (uint32_t s : seqs) {
    if (ix->h_dead[s] != f) ix->live += f ? (uint64_t)-1 : 1;
    ix->h_dead[s] = f;
  }
  return FVDB_OK;
}

int fvdb_ivfpq_search_dev_slot(fvdb_ivfpq* ix, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t k, uint32_t nprobe,
                               uint32_t fetch_k, const uint32_t* dead_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                               uint32_t* out_counts_dev) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = on ? on : ix->ctx;
  if (slot >= kSlots) FAIL(ctx, FVDB_E_INVALID, "slot out of range");
  if (ctx->device != ix->ctx->device) FAIL(ctx, FVDB_E_INVALID, "context of another device");
  int rc = check_search(ix, ctx, k, nprobe, fetch_k);
  if (rc) return rc;
  if (!q_dev || !out_ids_dev || !out_dist_dev || !out_counts_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  IvfPqSlot& S = ix->slots[slot];
  fvdb_pq* pq = ix->pq;
  const PqGeom g = pq->g;
  const uint32_t np = std::min(nprobe, ix->nlist);
  const uint32_t qt = ix->qt(), lds = qt * g.m * pq->ts() * 4;
  const uint32_t kk = fetch_k ? fetch_k : k;
  // the probe lists of the whole batch, by the IVF-flat index's own coarse stage; what it refuses is refused here
  HIPCHK(ctx, S.probes.ensure((size_t)B * np * 4));
  rc = fvdb_ivf_coarse_dev_slot(ix->ivf, ctx, slot, q_dev, B, np, S.probes.as<uint32_t>());
  if (rc) return rc;
  HIPCHK(ctx, S.stats.ensure(16));
  launch_fill(ctx, S.stats.p, 4, 0u);
  // arenas for the tables and for the partial lists cut a large batch into sub-batches; the second is a target, not a
  // bound: a shorter last sub-batch has fewer groups and may take a larger S, and part grows to what it needs
  uint32_t sub = (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min(B, kMaxSubBatch), kTableBytes / ((size_t)g.m * g.ka * 4)));
  {
    const uint32_t s0 = slices_for(cdiv(sub, qt), qt, np, (uint32_t)ctx->num_cus);
    sub = (uint32_t)std::max<size_t>(1, std::min<size_t>(sub, kArenaBytes / ((size_t)s0 * kk * 8)));
  }
  for (uint32_t b0 = 0; b0 < B; b0 += sub) {
    const uint32_t Bs = std::min(sub, B - b0);
    const float* qs = q_dev + (size_t)b0 * g.d;
    IvfPqScanArgs a{};
    a.S = slices_for(cdiv(Bs, qt), qt, np, (uint32_t)ctx->num_cus);
    S.last_S = a.S;
    HIPCHK(ctx, S.tables.ensure((size_t)Bs * g.m * g.ka * 4));
    if (ix->residual) {
      rc = launch_residual_tables(ix, ctx, S, qs, Bs, np, S.probes.as<uint32_t>() + (size_t)b0 * np);
      if (rc) return rc;
      a.term_of_row = ix->term_of_row.as<float>();
      a.base = S.base.as<float>();
    } else {
      hipLaunchKernelGGL(pq_table_kernel, dim3(g.m, Bs), dim3(256), 0, ctx->stream, qs, pq->books.as<float>(), g, S.tables.as<float>());
    }
    HIPCHK(ctx, S.part.ensure((size_t)a.S * Bs * kk * 8));
    a.codes = ix->codes.as<uint4>();
    a.dead = dead_dev ? dead_dev : ix->dead.as<uint32_t>();
    a.seq_of_row = ix->seq_of_row.as<uint32_t>();
    a.list_off = ix->list_off.as<uint32_t>();
    a.list_len = ix->list_len.as<uint32_t>();
    a.list_blocks = ix->list_blocks.as<uint32_t>();
    a.probes = S.probes.as<uint32_t>() + (size_t)b0 * np;
    a.tables = S.tables.as<float>();
    a.part = S.part.as<uint64_t>();
    a.stats = S.stats.as<unsigned long long>();
    a.nlist = ix->nlist;
    a.np = np;
    a.m = g.m;
    a.m16 = pq->m16();
    a.ka = g.ka;
    a.ts = pq->ts();
    a.B = Bs;
    a.k = kk;
    HIPCHK(ctx, S.nodes.ensure((size_t)Bs * kk * 4));
    uint32_t* nodes = S.nodes.as<uint32_t>();  // seqs
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
  ix->last_slot = (int)slot;
  ix->last_ctx = ctx;
  return FVDB_OK;
}

int fvdb_ivfpq_search(fvdb_ivfpq* ix, const float* q, uint32_t B, uint32_t k, uint32_t nprobe, uint32_t fetch_k, const uint64_t* allowed_ids,
                      uint64_t n_allowed, uint64_t* out_ids, float* out_dist, uint32_t* out_counts) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->ctx;
  if (B == 0) return FVDB_OK;
  if (!q || !out_ids || !out_dist || !out_counts) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (n_allowed && !allowed_ids) FAIL(ctx, FVDB_E_INVALID, "null allow-set");
  int rc = check_search(ix, ctx, k, nprobe, fetch_k);
  if (rc) return rc;
  const uint32_t d = ix->pq->g.d;
  rc = check_finite(ctx, q, (uint64_t)B * d);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  IvfPqSlot& S = ix->slots[0];
  HIPCHK(ctx, S.q.ensure((size_t)B * d * 4));
  HIPCHK(ctx, S.out.ensure((size_t)B * k * 16 + (size_t)B * 4));
  HIPCHK(ctx, upload(ctx, S.q.p, q, (size_t)B * d * 4));
  const uint32_t* dead_dev = nullptr;
  if (allowed_ids && ix->blocks) {  // the allow-set as the scan's "dead" words: unfilled, deleted, or not allowed
    std::vector<uint32_t> dw(ix->blocks * 64, 1u);
    for (uint64_t i = 0; i < n_allowed; ++i) {
      const auto it = ix->seq_of.find(allowed_ids[i]);
      if (it != ix->seq_of.end()) dw[ix->h_row_of_seq[it->second]] = ix->h_dead[it->second];
    }
    HIPCHK(ctx, S.dead.ensure(dw.size() * 4));
    HIPCHK(ctx, upload(ctx, S.dead.p, dw.data(), dw.size() * 4));
    dead_dev = S.dead.as<uint32_t>();
  }
  uint64_t* oi = S.out.as<uint64_t>();
  float* od = (float*)(oi + (size_t)B * k);
  uint32_t* oc = (uint32_t*)(od + (size_t)B * k);
  rc = fvdb_ivfpq_search_dev_slot(ix, ctx, 0, S.q.as<float>(), B, k, nprobe, fetch_k, dead_dev, oi, od, oc);
  if (rc) return rc;
  HIPCHK(ctx, download(ctx, out_ids, oi, (size_t)B * k * 8));
  HIPCHK(ctx, download(ctx, out_dist, od, (size_t)B * k * 4));
  HIPCHK(ctx, download(ctx, out_counts, oc, (size_t)B * 4));
  return FVDB_OK;
}

}  // extern "C"
