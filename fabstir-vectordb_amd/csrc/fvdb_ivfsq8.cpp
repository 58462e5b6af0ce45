// fvdb_ivfsq8.cpp — the inverted file over SQ8 codes behind the C ABI (include/fvdb.h, "IVF over SQ8 codes"; DESIGN.md
// section 9za).  A translation unit of its own: the scan is kernels_ivfsq8.h, the codec, score and selection are
// kernels_sq8.h's, the plan kernels kernels_scan.h's and the merge kernels_flat.h's, all unchanged.  Centroids,
// assignment and the coarse ranking belong to an fvdb_ivf without rows, reached through the C ABI like the refine
// rows' fvdb_store.
#include <algorithm>
#include <cstring>
#include <new>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "fvdb_internal.h"
#include "common.h"
#include "kernels_ivfsq8.h"

using namespace fvdb;

namespace {

constexpr uint32_t kSlots = 16;
constexpr size_t kArenaBytes = 256u << 20;    // partial lists of one launch chain
constexpr size_t kDecodedBytes = 256u << 20;  // decoded candidate rows of one launch chain

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
  if (words) hipLaunchKernelGGL(ivfsq8_fill_kernel, dim3(cdiv(words, 256)), dim3(256), 0, on->stream, (uint32_t*)p, words, v);
}

// what the plan kernels write besides their tables: stats[3] (rows scored, items, rows touched), the item count, a head
struct PlanWords {
  unsigned long long stats[3];
  uint32_t n_items, head;
};

}  // namespace

struct IvfSq8Slot {
  DBuf q, probes, qwords, qinfo, qpad, cnt, fill, eoff, ioff, entries, words, part, nodes, dist, counts, dead, decoded, out;
  uint32_t cnt_lists = 0;   // cnt[] is zero for this many lists (the plan leaves it so)
  uint32_t item_bound = 0;  // of the last launch chain
};

struct fvdb_ivfsq8 {
  fvdb_ctx* ctx = nullptr;
  uint32_t d = 0, ksteps = 0, nlist = 0, lds_limit = 0;
  int refine = FVDB_SQ8_NO_REFINE;
  bool trained = false;
  fvdb_ivf* ivf = nullptr;      // centroids only: it never receives rows
  fvdb_store* store = nullptr;  // refine rows, store row = seq
  DBuf codes, info, dead, seq_of_row;  // per pool block / pool row
  DBuf row_of_seq, ids;                // per seq
  DBuf list_off, list_len, list_blocks, s_in, s_rows;
  uint64_t n = 0, live = 0, blocks = 0, cap_blocks = 0, cap_seq = 0;
  uint32_t max_list_blocks = 0;
  std::vector<std::vector<uint32_t>> h_blocks;  // per list, in fill order
  std::vector<uint32_t> h_len, h_row_of_seq;
  std::vector<uint8_t> h_dead;                  // per seq
  std::unordered_map<uint64_t, uint32_t> seq_of;
  IvfSq8Slot slots[kSlots];
  int last_slot = -1;
  fvdb_ctx* last_ctx = nullptr;
  uint32_t dpad4() const { return (d + 3u) & ~3u; }
  // no list in more than kIvfSq8MaxSegments segments, no segment under kIvfSq8MinSegBlocks blocks
  uint32_t segb() const { return std::max<uint32_t>(kIvfSq8MinSegBlocks, cdiv(max_list_blocks, kIvfSq8MaxSegments)); }
  uint32_t segments() const { return std::max<uint32_t>(1, cdiv(max_list_blocks, segb())); }
  // the gathered operands go to LDS when they fit beside the survivor buffers of the k class, else they are read from HBM
  bool qlds(uint32_t kr) const { return ivfsq8_scan_lds(kr, ksteps, true) <= lds_limit; }
};

namespace {

template <int KR, bool QLDS>
int launch_scan(fvdb_ctx* on, const IvfSq8ScanArgs& a, uint32_t grid, uint32_t slices, uint32_t* out_nodes, float* out_dist, uint32_t* out_counts) {
  if (grid) {
    const uint32_t lds = ivfsq8_scan_lds(KR, a.ksteps, QLDS);
    // the attribute belongs to the function; every call sets what it needs
    HIPCHK(on, hipFuncSetAttribute((const void*)ivfsq8_scan_kernel<KR, QLDS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((ivfsq8_scan_kernel<KR, QLDS>), dim3(grid), dim3(256), lds, on->stream, a);
  }
  hipLaunchKernelGGL((flat_merge_kernel<KR>), dim3(cdiv(a.B, 4)), dim3(256), 0, on->stream, a.part, slices, a.B, a.k, out_nodes, out_dist,
                     out_counts);
  HIPCHK(on, hipGetLastError());
  return FVDB_OK;
}

template <int KR>
int launch_scan_q(bool qlds, fvdb_ctx* on, const IvfSq8ScanArgs& a, uint32_t grid, uint32_t slices, uint32_t* out_nodes, float* out_dist,
                  uint32_t* out_counts) {
  return qlds ? launch_scan<KR, true>(on, a, grid, slices, out_nodes, out_dist, out_counts)
              : launch_scan<KR, false>(on, a, grid, slices, out_nodes, out_dist, out_counts);
}

template <typename RT>
void launch_refine(fvdb_ctx* on, const RefineArgs& r) {
  const dim3 grid(cdiv(r.B, 4)), block(256);
  if (r.k <= 64) hipLaunchKernelGGL((sq8_refine_kernel<1, RT>), grid, block, 0, on->stream, r);
  else if (r.k <= 128) hipLaunchKernelGGL((sq8_refine_kernel<2, RT>), grid, block, 0, on->stream, r);
  else hipLaunchKernelGGL((sq8_refine_kernel<4, RT>), grid, block, 0, on->stream, r);
}

int check_search(fvdb_ivfsq8* ix, fvdb_ctx* ctx, uint32_t k, uint32_t nprobe, uint32_t fetch_k, int refine_mode) {
  if (k == 0 || k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "IVF-SQ8 search: k must be in 1..FVDB_MAX_K");
  if (fetch_k) {
    if (fetch_k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "refined search: fetch_k must be <= FVDB_MAX_K");
    if (k > fetch_k) FAIL(ctx, FVDB_E_INVALID, "refined search: k must be <= fetch_k");
    if (refine_mode != FVDB_SQ8_REFINE_DECODED && refine_mode != FVDB_SQ8_REFINE_ROWS)
      FAIL(ctx, FVDB_E_INVALID, "refine_mode must be FVDB_SQ8_REFINE_DECODED or FVDB_SQ8_REFINE_ROWS");
    if (refine_mode == FVDB_SQ8_REFINE_ROWS && !ix->store) FAIL(ctx, FVDB_E_INVALID, "FVDB_SQ8_REFINE_ROWS needs an index created with refine rows");
  }
  if (nprobe == 0) FAIL(ctx, FVDB_E_INVALID, "nprobe must be > 0");
  if (std::min(nprobe, ix->nlist) > kIvfSq8MaxProbe) FAIL(ctx, FVDB_E_UNSUPPORTED, "IVF-SQ8 search: at most 256 probed lists");
  if (!ix->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "index not trained");
  return FVDB_OK;
}

// the list table of the rows present, rebuilt whole: n / 32 words
int upload_lists(fvdb_ivfsq8* ix) {
  fvdb_ctx* ctx = ix->ctx;
  std::vector<uint32_t> off(ix->nlist + 1, 0), flat;
  flat.reserve(ix->blocks);
  ix->max_list_blocks = 0;
  for (uint32_t L = 0; L < ix->nlist; ++L) {
    flat.insert(flat.end(), ix->h_blocks[L].begin(), ix->h_blocks[L].end());
    off[L + 1] = (uint32_t)flat.size();
    ix->max_list_blocks = std::max<uint32_t>(ix->max_list_blocks, (uint32_t)ix->h_blocks[L].size());
  }
  HIPCHK(ctx, ix->list_blocks.ensure(std::max<size_t>(flat.size() * 4, 4)));
  HIPCHK(ctx, upload(ctx, ix->list_off.p, off.data(), off.size() * 4));
  HIPCHK(ctx, upload(ctx, ix->list_len.p, ix->h_len.data(), (size_t)ix->nlist * 4));
  HIPCHK(ctx, upload(ctx, ix->list_blocks.p, flat.data(), flat.size() * 4));
  return FVDB_OK;
}

}  // namespace

extern "C" {

int fvdb_ivfsq8_create(fvdb_ctx* ctx, uint32_t d, uint32_t nlist, int refine_dtype, fvdb_ivfsq8** out) {
  if (!ctx || !out) return FVDB_E_INVALID;
  *out = nullptr;
  if (d == 0 || nlist == 0) FAIL(ctx, FVDB_E_INVALID, "d and nlist must be > 0");
  if (d > kSq8MaxDims) FAIL(ctx, FVDB_E_UNSUPPORTED, "scalar quantization: d must be <= 2048");
  if (nlist > kIvfSq8MaxLists) FAIL(ctx, FVDB_E_UNSUPPORTED, "IVF-SQ8: nlist must be <= 16384");
  if (refine_dtype != FVDB_SQ8_NO_REFINE && refine_dtype != FVDB_F32 && refine_dtype != FVDB_F16)
    FAIL(ctx, FVDB_E_INVALID, "refine_dtype must be FVDB_SQ8_NO_REFINE, FVDB_F32 or FVDB_F16");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int lds = 0;
  HIPCHK(ctx, hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  fvdb_ivfsq8* ix = new (std::nothrow) fvdb_ivfsq8();
  if (!ix) return FVDB_E_OOM;
  ix->ctx = ctx;
  ix->d = d;
  ix->ksteps = (d + 31u) / 32u;
  ix->nlist = nlist;
  ix->lds_limit = (uint32_t)lds;
  ix->refine = refine_dtype;
  ix->h_blocks.assign(nlist, {});
  ix->h_len.assign(nlist, 0);
  int rc = fvdb_ivf_create(ctx, d, nlist, &ix->ivf);
  if (!rc && refine_dtype != FVDB_SQ8_NO_REFINE) rc = fvdb_store_create_ex(ctx, d, 1024, refine_dtype, &ix->store);
  if (!rc && (ix->list_off.exact((size_t)(nlist + 1) * 4) != hipSuccess || ix->list_len.exact((size_t)nlist * 4) != hipSuccess)) rc = FVDB_E_OOM;
  if (!rc) rc = upload_lists(ix);
  if (rc) {
    fvdb_ivfsq8_destroy(ix);
    return rc;
  }
  *out = ix;
  return FVDB_OK;
}

void fvdb_ivfsq8_destroy(fvdb_ivfsq8* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->ctx->device);
  (void)hipDeviceSynchronize();  // searches may be in flight on other contexts' streams
  if (ix->store) fvdb_store_destroy(ix->store);
  if (ix->ivf) fvdb_ivf_destroy(ix->ivf);
  delete ix;
}

int fvdb_ivfsq8_train(fvdb_ivfsq8* ix, const float* x, uint64_t n, uint32_t max_iterations, uint64_t seed, fvdb_train_result* out) {
  if (!ix) return FVDB_E_INVALID;
  if (ix->n) FAIL(ix->ctx, FVDB_E_UNSUPPORTED, "IVF-SQ8: the centroids of an index with rows cannot be replaced");
  const int rc = fvdb_ivf_train(ix->ivf, x, n, max_iterations, seed, out);
  if (!rc) ix->trained = true;
  return rc;
}

int fvdb_ivfsq8_set_centroids(fvdb_ivfsq8* ix, const float* centroids) {
  if (!ix) return FVDB_E_INVALID;
  if (ix->n) FAIL(ix->ctx, FVDB_E_UNSUPPORTED, "IVF-SQ8: the centroids of an index with rows cannot be replaced");
  const int rc = fvdb_ivf_set_centroids(ix->ivf, centroids);
  if (!rc) ix->trained = true;
  return rc;
}

int fvdb_ivfsq8_get_centroids(fvdb_ivfsq8* ix, float* out) {
  if (!ix) return FVDB_E_INVALID;
  if (!out) FAIL(ix->ctx, FVDB_E_INVALID, "null argument");
  return fvdb_ivf_get_centroids(ix->ivf, out);
}

uint64_t fvdb_ivfsq8_rows(fvdb_ivfsq8* ix) { return ix ? ix->n : 0; }
uint64_t fvdb_ivfsq8_live(fvdb_ivfsq8* ix) { return ix ? ix->live : 0; }
uint64_t fvdb_ivfsq8_bytes(fvdb_ivfsq8* ix) {
  if (!ix) return 0;
  return ix->blocks * ((uint64_t)ix->ksteps * 1024 + 32 * 24 + 4) + ix->n * 12 + (uint64_t)(2 * ix->nlist + 1) * 4 +
         (ix->store ? fvdb_store_bytes(ix->store) : 0);
}

int fvdb_ivfsq8_list_sizes(fvdb_ivfsq8* ix, uint64_t* out) {
  if (!ix) return FVDB_E_INVALID;
  if (!out) FAIL(ix->ctx, FVDB_E_INVALID, "null argument");
  for (uint32_t L = 0; L < ix->nlist; ++L) out[L] = ix->h_len[L];
  return FVDB_OK;
}

int fvdb_ivfsq8_info(fvdb_ivfsq8* ix, fvdb_ivfsq8_info_t* out) {
  if (!ix || !out) return FVDB_E_INVALID;
  memset(out, 0, sizeof(*out));
  out->d = ix->d;
  out->d_padded = ix->ksteps * 32;
  out->nlist = ix->nlist;
  out->block_rows = kSq8Tile;
  out->queries_per_item = kSq8Tile;
  out->round_rows = kSq8RoundRows;
  out->words_in_flight = kSq8Ahead;
  out->max_segments = kIvfSq8MaxSegments;
  out->segb = ix->segb();
  out->segments = ix->segments();
  out->max_list_blocks = ix->max_list_blocks;
  out->lds_limit = ix->lds_limit;
  const uint32_t krs[3] = {1, 2, 4};
  for (int i = 0; i < 3; ++i) {
    out->queries_in_lds[i] = ix->qlds(krs[i]);
    out->lds_bytes[i] = ivfsq8_scan_lds(krs[i], ix->ksteps, ix->qlds(krs[i]));
  }
  out->max_d = kSq8MaxDims;
  out->max_k = FVDB_MAX_K;
  out->max_nprobe = kIvfSq8MaxProbe;
  out->max_nlist = kIvfSq8MaxLists;
  out->pool_blocks = ix->blocks;
  if (ix->last_slot >= 0) {
    fvdb_ctx* ctx = ix->last_ctx;
    const IvfSq8Slot& S = ix->slots[ix->last_slot];
    PlanWords w{};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, download(ctx, &w, S.words.p, sizeof(w)));
    out->item_bound = S.item_bound;
    out->rows_scored = w.stats[0];
    out->items = w.stats[1];
  }
  return FVDB_OK;
}

int fvdb_ivfsq8_add(fvdb_ivfsq8* ix, const uint64_t* ids, const float* rows, uint64_t n) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->ctx;
  if (n == 0) return FVDB_OK;
  if (!ids || !rows) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (!ix->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "index not trained");
  if (ix->n + n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "index limited to 2^32-1 rows");
  int rc = sq8_check_rows(ctx, rows, n, ix->d);
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
    if ((pos & 31u) == 0) {
      tail[L] = (uint32_t)blocks++;
      fresh.emplace_back(L, tail[L]);
    }
    dest[i] = tail[L] * 32u + (pos & 31u);
  }
  if (blocks * 32 >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "pool limited to 2^32-1 rows");
  if (blocks > ix->cap_blocks) {  // code blocks come zeroed, the new blocks' rows dead until a row is placed there
    const uint64_t nb = std::max<uint64_t>(blocks, ix->cap_blocks + ix->cap_blocks / 2), ob = ix->blocks;
    const size_t wb = (size_t)ix->ksteps * 1024;
    HIPCHK(ctx, grow_keeping(ix->codes, nb * wb, ob * wb, /*zero_rest=*/true, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->info, nb * 32 * 16, ob * 32 * 16, /*zero_rest=*/true, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->seq_of_row, nb * 32 * 4, ob * 32 * 4, /*zero_rest=*/true, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->dead, nb * 32 * 4, ob * 32 * 4, /*zero_rest=*/false, ctx->stream));
    launch_fill(ctx, ix->dead.as<uint32_t>() + ob * 32, (nb - ob) * 32, 1u);
    ix->cap_blocks = nb;
  }
  if (ix->n + n > ix->cap_seq) {
    const uint64_t ns = std::max<uint64_t>(ix->n + n, ix->cap_seq + ix->cap_seq / 2);
    HIPCHK(ctx, grow_keeping(ix->row_of_seq, ns * 4, ix->n * 4, /*zero_rest=*/false, ctx->stream));
    HIPCHK(ctx, grow_keeping(ix->ids, ns * 8, ix->n * 8, /*zero_rest=*/false, ctx->stream));
    ix->cap_seq = ns;
  }
  HIPCHK(ctx, ix->s_in.ensure(n * ix->d * 4));
  HIPCHK(ctx, ix->s_rows.ensure(n * 4));
  HIPCHK(ctx, upload(ctx, ix->s_in.p, rows, n * ix->d * 4));
  HIPCHK(ctx, upload(ctx, ix->s_rows.p, dest.data(), n * 4));
  Sq8EncodeArgs a{};
  a.rows = ix->s_in.as<float>();
  a.d = ix->d;
  a.ksteps = ix->ksteps;
  a.n = n;
  a.blocks = ix->codes.as<uint4>();
  a.info = ix->info.as<uint4>();
  a.dest = ix->s_rows.as<uint32_t>();
  hipLaunchKernelGGL(sq8_encode_kernel, dim3(cdiv(n, 4)), dim3(256), 0, ctx->stream, a);
  hipLaunchKernelGGL(ivfsq8_place_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, ix->s_rows.as<uint32_t>(), n, (uint32_t)ix->n,
                     ix->seq_of_row.as<uint32_t>(), ix->row_of_seq.as<uint32_t>(), ix->dead.as<uint32_t>());
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, upload(ctx, ix->ids.as<uint64_t>() + ix->n, ids, n * 8));
  if (ix->store) {
    uint64_t first = 0;
    rc = fvdb_store_append(ix->store, rows, n, &first);
    if (rc) return rc;
  }
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

int fvdb_ivfsq8_set_deleted(fvdb_ivfsq8* ix, const uint64_t* ids, uint64_t n, int flag) {
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
  hipLaunchKernelGGL(ivfsq8_set_flags_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, ix->s_rows.as<uint32_t>(), n, flag ? 1u : 0u,
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

int fvdb_ivfsq8_search_dev_slot(fvdb_ivfsq8* ix, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t k, uint32_t nprobe,
                                uint32_t fetch_k, int refine_mode, const uint32_t* dead_dev, uint64_t* out_ids_dev, float* out_dist_dev,
                                uint32_t* out_counts_dev) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = on ? on : ix->ctx;
  if (slot >= kSlots) FAIL(ctx, FVDB_E_INVALID, "slot out of range");
  if (ctx->device != ix->ctx->device) FAIL(ctx, FVDB_E_INVALID, "context of another device");
  int rc = check_search(ix, ctx, k, nprobe, fetch_k, refine_mode);
  if (rc) return rc;
  if (!q_dev || !out_ids_dev || !out_dist_dev || !out_counts_dev) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  IvfSq8Slot& S = ix->slots[slot];
  const uint32_t d = ix->d, ksteps = ix->ksteps, nlist = ix->nlist;
  const uint32_t np = std::min(nprobe, nlist);
  const uint32_t kk = fetch_k ? fetch_k : k;
  const uint32_t kr = kk <= 64 ? 1 : (kk <= 128 ? 2 : 4);
  const uint32_t segb = ix->segb(), segs = ix->segments(), slices = np * segs;
  const bool decoded = fetch_k && refine_mode == FVDB_SQ8_REFINE_DECODED;
  const uint32_t rpad = decoded ? ix->dpad4() : (fetch_k ? ix->store->dpad : 0);  // row stride of the refine source
  // the probe lists of the whole batch, by the IVF-flat index's own coarse stage
  HIPCHK(ctx, S.probes.ensure((size_t)B * np * 4));
  rc = fvdb_ivf_coarse_dev_slot(ix->ivf, ctx, slot, q_dev, B, np, S.probes.as<uint32_t>());
  if (rc) return rc;
  // plan scratch; cnt[] starts zero and every plan leaves it zero
  HIPCHK(ctx, S.fill.ensure((size_t)nlist * 4));
  HIPCHK(ctx, S.eoff.ensure((size_t)(nlist + 1) * 4));
  HIPCHK(ctx, S.ioff.ensure((size_t)(nlist + 1) * 4));
  HIPCHK(ctx, S.words.ensure(sizeof(PlanWords)));
  if (S.cnt_lists < nlist) {
    HIPCHK(ctx, S.cnt.ensure((size_t)nlist * 4));
    launch_fill(ctx, S.cnt.p, nlist, 0u);
    S.cnt_lists = nlist;
  }
  PlanWords* pw = S.words.as<PlanWords>();
  uint32_t sub = (uint32_t)std::max<size_t>(1, std::min<size_t>(B, kArenaBytes / ((size_t)slices * kk * 8)));
  if (decoded) sub = (uint32_t)std::max<size_t>(1, std::min<size_t>(sub, kDecodedBytes / ((size_t)kk * rpad * 4)));
  for (uint32_t b0 = 0; b0 < B; b0 += sub) {
    const uint32_t Bs = std::min(sub, B - b0), pairs = Bs * np;
    const float* qs = q_dev + (size_t)b0 * d;
    const uint32_t* probes = S.probes.as<uint32_t>() + (size_t)b0 * np;
    // the queries, encoded once by the rows' rule into the per-query form
    HIPCHK(ctx, S.qwords.ensure((size_t)Bs * ksteps * 32));
    HIPCHK(ctx, S.qinfo.ensure((size_t)Bs * 16));
    Sq8EncodeArgs e{};
    e.rows = qs;
    e.d = d;
    e.ksteps = ksteps;
    e.n = Bs;
    e.blocks = S.qwords.as<uint4>();
    e.info = S.qinfo.as<uint4>();
    e.per_row = 1;
    hipLaunchKernelGGL(sq8_encode_kernel, dim3(cdiv(Bs, 4)), dim3(256), 0, ctx->stream, e);
    // the plan: probes[Bs][np] -> per-list entries and work items (list, segment, group of 32 entries)
    HIPCHK(ctx, S.entries.ensure((size_t)pairs * 8));
    hipLaunchKernelGGL(plan_count_kernel, dim3(cdiv(pairs, 256)), dim3(256), 0, ctx->stream, probes, pairs, S.cnt.as<uint32_t>(),
                       ix->list_off.as<uint32_t>());
    hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, S.cnt.as<uint32_t>(), ix->list_off.as<uint32_t>(),
                       ix->list_len.as<uint32_t>(), nlist, segb, kSq8Tile, S.eoff.as<uint32_t>(), S.ioff.as<uint32_t>(), S.fill.as<uint32_t>(),
                       &pw->n_items, &pw->head, pw->stats, S.cnt.as<uint32_t>(), 0xFFFFFFFFu, 0u);
    hipLaunchKernelGGL(plan_fill_kernel, dim3(cdiv(pairs, 256)), dim3(256), 0, ctx->stream, probes, pairs, np, S.eoff.as<uint32_t>(),
                       S.fill.as<uint32_t>(), S.entries.as<uint2>(), ix->list_off.as<uint32_t>());
    // every list with entries has at most segs (items per group) * (entries / 32 + 1) items
    const uint32_t bound = ix->blocks ? segs * (pairs / kSq8Tile + std::min(nlist, pairs)) : 0u;
    S.item_bound = bound;
    HIPCHK(ctx, S.part.ensure((size_t)slices * Bs * kk * 8));
    launch_fill(ctx, S.part.p, (uint64_t)slices * Bs * kk * 2, 0xFFFFFFFFu);
    IvfSq8ScanArgs a{};
    a.codes = ix->codes.as<uint4>();
    a.info = ix->info.as<uint4>();
    a.dead = dead_dev ? dead_dev : ix->dead.as<uint32_t>();
    a.seq_of_row = ix->seq_of_row.as<uint32_t>();
    a.list_off = ix->list_off.as<uint32_t>();
    a.list_blocks = ix->list_blocks.as<uint32_t>();
    a.qwords = S.qwords.as<uint4>();
    a.qinfo = S.qinfo.as<uint4>();
    a.item_off = S.ioff.as<uint32_t>();
    a.entry_off = S.eoff.as<uint32_t>();
    a.entries = S.entries.as<uint2>();
    a.n_items = &pw->n_items;
    a.part = S.part.as<uint64_t>();
    a.nlist = nlist;
    a.d = d;
    a.ksteps = ksteps;
    a.B = Bs;
    a.k = kk;
    a.segb = segb;
    a.segs = segs;
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
    const bool qlds = ix->qlds(kr);
    switch (kr) {
      case 1: rc = launch_scan_q<1>(qlds, ctx, a, bound, slices, nodes, dist, counts); break;
      case 2: rc = launch_scan_q<2>(qlds, ctx, a, bound, slices, nodes, dist, counts); break;
      default: rc = launch_scan_q<4>(qlds, ctx, a, bound, slices, nodes, dist, counts); break;
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
        hipLaunchKernelGGL(ivfsq8_decode_cand_kernel, dim3(cdiv((uint64_t)Bs * kk * rpad, 256)), dim3(256), 0, ctx->stream,
                           ix->codes.as<uint4>(), ix->info.as<uint4>(), ix->row_of_seq.as<uint32_t>(), ksteps, d, rpad, nodes, counts, Bs, kk,
                           S.decoded.as<float>());
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
  ix->last_slot = (int)slot;
  ix->last_ctx = ctx;
  return FVDB_OK;
}

int fvdb_ivfsq8_search(fvdb_ivfsq8* ix, const float* q, uint32_t B, uint32_t k, uint32_t nprobe, uint32_t fetch_k, int refine_mode,
                       const uint64_t* allowed_ids, uint64_t n_allowed, uint64_t* out_ids, float* out_dist, uint32_t* out_counts) {
  if (!ix) return FVDB_E_INVALID;
  fvdb_ctx* ctx = ix->ctx;
  if (B == 0) return FVDB_OK;
  if (!q || !out_ids || !out_dist || !out_counts) FAIL(ctx, FVDB_E_INVALID, "null argument");
  if (n_allowed && !allowed_ids) FAIL(ctx, FVDB_E_INVALID, "null allow-set");
  int rc = check_search(ix, ctx, k, nprobe, fetch_k, refine_mode);
  if (rc) return rc;
  rc = sq8_check_rows(ctx, q, B, ix->d);  // a query is encoded by the rows' rule
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  IvfSq8Slot& S = ix->slots[0];
  HIPCHK(ctx, S.q.ensure((size_t)B * ix->d * 4));
  HIPCHK(ctx, S.out.ensure((size_t)B * k * 16 + (size_t)B * 4));
  HIPCHK(ctx, upload(ctx, S.q.p, q, (size_t)B * ix->d * 4));
  const uint32_t* dead_dev = nullptr;
  if (allowed_ids && ix->blocks) {  // the allow-set as the scan's "dead" words: unfilled, deleted, or not allowed
    std::vector<uint32_t> dw(ix->blocks * 32, 1u);
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
  rc = fvdb_ivfsq8_search_dev_slot(ix, ctx, 0, S.q.as<float>(), B, k, nprobe, fetch_k, refine_mode, dead_dev, oi, od, oc);
  if (rc) return rc;
  HIPCHK(ctx, download(ctx, out_ids, oi, (size_t)B * k * 8));
  HIPCHK(ctx, download(ctx, out_dist, od, (size_t)B * k * 4));
  HIPCHK(ctx, download(ctx, out_counts, oc, (size_t)B * 4));
  return FVDB_OK;
}

}  // extern "C"
