// fvdb_hip.cpp — C ABI (include/fvdb.h) over the HIP kernels.  gfx950 only; compiled with
//   hipcc -x hip -O3 -ffp-contract=off --offload-arch=gfx950
// Host side here is plumbing: memory, launch order, list bookkeeping.  All arithmetic on
// vectors happens in the kernels; there is no CPU fallback anywhere in this library.
#include "fvdb_internal.h"

#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "common.h"
#include "pool.h"
#include "kernels_misc.h"
#include "kernels_scan.h"
#include "kernels_wide.h"
#include "kernels_range.h"
#include "kernels_rank.h"
#include "kernels_curve.h"
#include "kernels_coarse.h"
#include "kernels_mfma.h"
#include "kernels_mfma_wg.h"
#include "kernels_util.h"
#include "kernels_maint.h"
#include "kernels_rows.h"
#include "kernels_mmr.h"
#include "kernels_group.h"

using namespace fvdb;


// Words of the counter block of an index (fvdb_ivf::s_fallbacks, 32 bytes, and its pinned copy h_fb): running totals
// since the centroids were installed, added to by the kernels named.
enum FbWord : uint32_t {
  FB_COARSE = 0,    // coarse_select_kernel: queries whose 64 proposals did not prove the ranking (exact ranking instead)
  FB_SCAN = 1,      // select_kernel: queries not proven, rescanned exactly (VerifyArgs::fallbacks)
  FB_REASONS = 2,   // [2..5] why, one word per reason (VerifyArgs::reasons): [2] the survivor buffer overflowed,
                    // [3] more candidates than the select stage scores, [4] the k-th kept distance not strictly below
                    // the bound, [5] no usable threshold
  FB_OVERFLOW = 2,  // the first of them, watched by AUTO's refine decision
  FB_REFINED = 6,   // refine_threshold_kernel: queries given a tighter threshold and a second filter pass
  FB_WORDS = 8,     // [7] unused
};
constexpr size_t kFbBytes = FB_WORDS * 4;
// The index keeps the block twice, one after the other: the second copy takes the counts of the searches under an
// allow-set mask, so that what AUTO's watches read (the first, through its pinned copy) is the unmasked traffic alone.
// The public counters report the sum of both.
constexpr size_t kFbAllBytes = 2 * kFbBytes;
constexpr uint32_t kFbReasonWords = 5;  // fvdb_ivf_scan_fallback_reasons: words 2..6, the four reasons and the refine counter

// Stage events of a search, recorded while profiling is on; finish_profile turns pairs of them into stage times.
enum StageEvent {
  EV_COARSE_BEGIN = 0,
  EV_COARSE_SCANNED,  // centroid distances (or partial lists) done, selection / merge follows
  EV_COARSE_DONE,
  EV_SCAN_BEGIN,      // exact path: after the plan kernels; matrix-core path: before query prep
  EV_SCAN_DONE,       // partial lists / survivors done, merge / select follows
  EV_FINE_DONE,
  EV_FILTER_BEGIN,    // the matrix-core filter kernel alone (inside the scan interval)
  EV_FILTER_DONE,
  EV_COUNT
};

// Words of IvfScratch::s_scalars (64 bytes).
enum ScalWord : uint32_t {
  SC_COARSE_ITEMS = 0,  // coarse scan: work items, queue head
  SC_COARSE_HEAD = 1,
  SC_FINE_ITEMS = 2,    // list scan: the same
  SC_FINE_HEAD = 3,
  SC_STATS = 4,         // [4..9] 3 x u64: rows scanned, work items, list rows touched (fvdb_ivf_last_stats)
};
constexpr size_t kScalarsBytes = 64;

// Per-search scratch of an IVF index.  Set 0 lives in the index itself (also used by the mutating entry points);
// sets 1..7 serve the other explicit slots of the *_slot entry points; a further pool of leased sets, each with a
// stream of its own, serves the blocking host-pointer searches, so any number of host threads may search one index
// at once (reference: searches hold a read guard, bindings/node/src/session.rs:253).  A search never modifies the
// index object: the scratch set and the stream it runs on are passed down explicitly (Env).
struct IvfScratch {
  std::mutex enq;  // held while one search's launches are enqueued: searches sharing a set are ordered by the stream
  bool pend_filter = false;
  bool pending_profile = false, pend_coarse = false, pend_fine = false, collecting = false;
  DBuf s_qnorm, s_A;
  DBuf s_qh, s_qn2, s_thr, s_tA, s_pa, s_surv, s_scnt, s_fail, s_mslots;
  DBuf s_sdist, s_probes2;
  DBuf s_q, s_cpart, s_probes, s_cnt, s_fill, s_eoff, s_ioff, s_entries;
  DBuf s_part, s_scalars, s_ceoff, s_cioff;
  DBuf s_wbase, s_arena;  // the wide selection (kernels_wide.h): per-query rank bases, distance arena
  DBuf s_wgbase;          // the same bases over the logical index, for the keys of a shard's wide search
  DBuf s_gwords, s_group;  // a grouped search: the live-word pointer table [G + 1], the group of each query [B]
  DBuf s_rbase, s_rarena;  // the full centroid ranking (kernels_rank.h): the same for the centroid table
  DBuf s_qual;            // fvdb_ivf_search_quality_dev: the two result blocks
  // fvdb_ivf_quality_curve_dev (kernels_curve.h): live rows per list; per chunk the ranking, the truth's keys and hit
  // counts, and the per-query recall and precision at every nprobe
  DBuf s_clive, s_cprobes, s_ckeys, s_cval;
  DBuf s_in, s_slots, s_ids, s_clusters, s_out_ids, s_out_dist, s_out_cnt, s_cdist;
  // fvdb_ivf_get_rows (ivf_rows.h): slots and gathered rows of one fetch.  Not s_slots / s_in: in set 0 those are the
  // insert staging.  fetch_done: the last fetch that read s_fslots on a stream other than the set's own
  DBuf s_fslots, s_frows;
  DevEvent fetch_done;
  DevEvent sev[EV_COUNT];
  uint32_t* scalar(ScalWord w) const { return s_scalars.as<uint32_t>() + w; }
};

struct fvdb_ivf : IvfScratch {
  static constexpr uint32_t kSlots = 16;
  IvfScratch spare[kSlots - 1];  // slots 1..15
  // leased sets for blocking searches called from several host threads: each has its own stream (a private context)
  static constexpr uint32_t kLeases = 8;
  IvfScratch lease_set[kLeases];
  fvdb_ctx* lease_ctx[kLeases] = {};
  uint32_t lease_busy = 0;  // bit i: set i is out (under mu)
  std::mutex mu;            // list table upload, lease bookkeeping, AUTO-mode counters
  std::condition_variable lease_cv;
  std::atomic<IvfScratch*> last_set{nullptr};  // scratch set of the most recent search (diagnostic entry points)
  std::atomic<fvdb_ctx*> last_ctx{nullptr};    // and the context (stream) it ran on
  fvdb_ctx* ctx = nullptr;
  uint32_t d = 0, dpad = 0, d4 = 0, nlist = 0;
  bool trained = false;
  bool f16 = false;  // inverted-list rows stored as fp16 (centroids and queries stay f32)

  // centroid table: row-major copy (host + device) and a blocked pool scanned as "list 0"
  std::vector<float> h_centroids;
  DBuf d_centroids_rm;   // [nlist][d]
  DBuf d_cent_pad;       // [nlist][dpad] zero padded (only when d != dpad)
  DBuf d_cnorm, d_cnmax; // |c|^2 per centroid, max |c|^2 (matrix-core coarse stage)
  DBuf s_fallbacks;      // counter block (FbWord)
  uint32_t* fb_word(FbWord w, bool masked = false) const { return s_fallbacks.as<uint32_t>() + (masked ? FB_WORDS : 0) + w; }
  int coarse_mode = 0;   // 0 = matrix cores + exact verification when applicable, 1 = exact scan only
  int scan_mode = 0;     // same choice for the inverted-list scan
  // AUTO scan mode watches its own hit rate: the rescan counter is copied to pinned host memory behind every
  // matrix-core batch (no sync); when too many queries of the recent batches needed the exact rescan (data the
  // filter cannot separate, e.g. no cluster structure), the next batches go straight to the exact scan
  HBuf h_fb;                 // pinned copy of s_fallbacks
  uint64_t mfma_q = 0;       // queries sent down the matrix-core path
  uint64_t fb_seen = 0, q_seen = 0;  // counter / queries at the last decision
  uint32_t exact_batches_left = 0;   // > 0: AUTO is backing off to the exact scan
  uint32_t backoff_len = 0;
  // the second filter pass for queries whose survivors outgrew the buffer (refine_threshold_kernel) costs five small
  // launches per batch: AUTO enqueues them only while such queries have been seen recently (FB_OVERFLOW + FB_REFINED)
  uint64_t overflow_seen = 0, overflow_q = 0;
  uint32_t refine_batches_left = 0;
  // diagnostic build only (-DFVDB_MFMA_STAMPS_BUILD): the filter's per-item timeline and the launches counted so far
  DBuf d_mfma_stamps;
  int mfma_stamps_launch = 0;
  DBuf d_xmax;           // max |x|^2 over the rows ever added (float bits)
  Pool cpool;
  DBuf c_off, c_blocks, c_glob;  // single-list table for the centroid pool

  // inverted lists: paged blocks
  Pool pool;
  std::vector<std::vector<uint32_t>> list_blocks;  // per list: pool block indices
  std::vector<uint32_t> list_len;                  // rows per list (including soft-deleted)
  uint64_t total_rows = 0;
  // bumped by everything that changes the rows a search sees or where they sit (add, set_deleted, clear, new centroids,
  // compact, refill, reserve): a mask (fvdb_mask) built before the bump is refused by the masked searches
  uint64_t mutations = 0;
  uint32_t max_list_blocks = 0;
  bool table_dirty = true;
  DBuf t_off, t_blocks, t_glob, t_len;  // device list table, logical (global) block counts, rows per list
  std::vector<uint32_t> glob_blocks_host;  // empty => local sizes
  bool glob_set = false;

  // resident maintenance (ivf_maint.h): the sequence map and the destinations of the source index whose rows
  // fvdb_ivf_assign_from ranked against this index's centroids, kept for fvdb_ivf_refill_from; the figures of the
  // last job
  DBuf m_seq, m_dest, m_ids;
  fvdb_ivf* m_src = nullptr;
  uint64_t m_rows = 0;
  bool m_assigned = false;  // m_dest holds fvdb_ivf_assign_from's ranking of m_src's m_rows rows
  bool m_store_job = false; // m_info holds fvdb_ivf_assign_from_store's figures: the add that follows continues them
  fvdb_maintenance_info_t m_info{};

  // per-search scratch
  fvdb_search_stats last_stats{};
  // coarse scan, coarse merge, plan, fine scan, fine merge, [5] the matrix-core filter kernel alone (kStageSpan)
  float stage_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t stage_calls = 0;
};

namespace {
// what a search runs with: the stream (context) its launches go to and the scratch set they may touch
struct Env {
  fvdb_ctx* ctx;
  IvfScratch* S;
  const uint64_t* live = nullptr;  // masked search: these words stand for pool.valid in every stage of the list scan
};
inline IvfScratch& slot_scratch(fvdb_ivf* ivf, uint32_t slot) { return slot == 0 ? *ivf : ivf->spare[slot - 1]; }
// The liveness words of the inverted lists as this search sees them, and the pool with them in place: the one place
// every argument block of the list scan takes them from.
inline const uint64_t* live_words(const fvdb_ivf* ivf, const Env& E) { return E.live ? E.live : ivf->pool.valid(); }
inline PoolView list_pool(const fvdb_ivf* ivf, const Env& E) {
  PoolView v = ivf->pool.view();
  v.valid = live_words(ivf, E);
  return v;
}
}  // namespace


// ---------------------------------------------------------------------------------------------
// knobs and launch helpers
// ---------------------------------------------------------------------------------------------
namespace {

// Environment knobs of the IVF search path: tuning aids for A/B runs, read once per process when the
// first search asks for them, clamped here to values the code below can use as they are.
struct IvfKnobs {
  static int num(const char* name, int unset) { return getenv(name) ? atoi(getenv(name)) : unset; }
  static bool has(const char* name) { return getenv(name) != nullptr; }
  static int tiles(int m) { return m >= 4 ? 4 : (m >= 2 ? 2 : 1); }
  bool coarse_exact = has("FVDB_COARSE_EXACT");  // centroid ranking by the exact scan only
  bool scan_exact = has("FVDB_SCAN_EXACT");      // list scan by the exact scan only
  uint32_t scan_wgs_per_cu = (uint32_t)num("FVDB_SCAN_WGS_PER_CU", 8);  // exact scan: workgroups per CU
  int segb = num("FVDB_SEGB", 0);                                       // > 0: its blocks per segment, fixed
  bool no_shared_thr = has("FVDB_NO_SHARED_THR");  // sharded search: every rank computes every threshold itself
  // the matrix-core list scan (run_fine_mfma), wave form
  int mfma_m = tiles(num("FVDB_MFMA_M", 2));  // 16-query tiles per group: 1, 2 or 4
  int mfma_segb = num("FVDB_MFMA_SEGB", 0);   // > 0: blocks per segment, fixed
  uint32_t mfma_wgs_per_cu = (uint32_t)std::max(1, num("FVDB_MFMA_WGS_PER_CU", 2));
  bool mfma_groups_in_item = num("FVDB_MFMA_GROUPS_IN_ITEM", 0) != 0;  // MfmaScanArgs::groups_in_item (A/B)
  // its workgroup form (kernels_mfma_wg.h); 0 = always the wave form
  bool mfma_wg = num("FVDB_MFMA_WG", 1) != 0;
  int mfma_wg_m = num("FVDB_MFMA_WG_M", 4) >= 4 ? 4 : 2;
  uint32_t mfma_wg_segb = (uint32_t)std::max(4, num("FVDB_MFMA_WG_SEGB", 16));
  uint32_t mfma_wg_per_cu = (uint32_t)std::max(1, num("FVDB_MFMA_WG_PER_CU", 2));
  int mfma_wg_tail_pct = num("FVDB_MFMA_WG_TAIL_PCT", 25);    // the last quarter of the lists ...
  int mfma_wg_segb_tail = num("FVDB_MFMA_WG_SEGB_TAIL", 4);   // ... in small segments (MfmaScanArgs::lsplit)
  // the threshold: blocks sampled; the earlier matrix-core pass instead of the direct kernel (A/B), and its segments
  uint32_t mfma_cap_a = (uint32_t)std::max(1, num("FVDB_MFMA_CAP_A", 4));
  bool mfma_threshold_pass = has("FVDB_MFMA_THRESHOLD_PASS");
  uint32_t mfma_segb_a = (uint32_t)std::max(1, num("FVDB_MFMA_SEGB_A", 1));
  bool mfma_no_refine = has("FVDB_MFMA_NO_REFINE");  // no second filter pass (A/B)
#ifdef FVDB_MFMA_STAMPS_BUILD
  int mfma_stamps = num("FVDB_MFMA_STAMPS", 0);  // first launch whose per-item timeline is printed (and the two after)
#endif
};
const IvfKnobs& ivf_knobs() {
  static const IvfKnobs knobs{};
  return knobs;
}

struct ScanLaunch {
  PoolView pool;
  const uint32_t* list_off;
  const uint32_t* list_blocks;
  uint32_t nlist;
  const uint32_t* entry_off;
  const uint32_t* item_off;
  const uint2* entries;
  const uint32_t* n_items;
  uint32_t* head;
  const float* queries;
  uint32_t dpad, segb, k, nprobe, maxsegs;
  uint2* part;
  uint32_t max_items = 0;  // host-side upper bound on work items (0 = unknown): sizes the persistent grid
  bool f16 = false;        // rows of `pool` are fp16
};

inline int kr_for(uint32_t k) { return k <= 64 ? 1 : (k <= 128 ? 2 : 4); }
inline uint32_t q_for(uint32_t k) { return k <= 64 ? 16u : (k <= 128 ? 8u : 4u); }

template <int Q, int KR, int ROLE, int ST>
void launch_scan_t(fvdb_ctx* ctx, const ScanLaunch& s) {
  uint32_t grid = (uint32_t)ctx->num_cus * ivf_knobs().scan_wgs_per_cu;  // more than fit: surplus workgroups find the queue empty
  if (s.max_items) grid = std::min(grid, std::max<uint32_t>(1u, (s.max_items + 3) / 4));  // 4 waves per workgroup
  hipLaunchKernelGGL((scan_topk_kernel<Q, KR, ROLE, ST>), dim3(grid), dim3(256), 0, ctx->stream, s.pool.data, s.pool.valid,
                     s.pool.d4, s.list_off, s.list_blocks, s.nlist, s.entry_off, s.item_off, (const u32x2*)s.entries,
                     s.n_items, s.head, s.queries, s.dpad, s.segb, s.k, s.nprobe, s.maxsegs, (u32x2*)s.part);
}

template <int ROLE, int ST>
void launch_scan_rs(fvdb_ctx* ctx, const ScanLaunch& s) {
  switch (kr_for(s.k)) {
    case 1: launch_scan_t<16, 1, ROLE, ST>(ctx, s); break;
    case 2: launch_scan_t<8, 2, ROLE, ST>(ctx, s); break;
    default: launch_scan_t<4, 4, ROLE, ST>(ctx, s); break;
  }
}
template <int ROLE>
void launch_scan_r(fvdb_ctx* ctx, const ScanLaunch& s) {
  if (s.f16) launch_scan_rs<ROLE, 1>(ctx, s); else launch_scan_rs<ROLE, 0>(ctx, s);
}
enum { ROLE_COARSE = 0, ROLE_LIST = 1, ROLE_ALL = 2 };
void launch_scan(fvdb_ctx* ctx, const ScanLaunch& s, int role) {
  if (role == ROLE_COARSE) launch_scan_r<ROLE_COARSE>(ctx, s);
  else if (role == ROLE_LIST) launch_scan_r<ROLE_LIST>(ctx, s);
  else launch_scan_r<ROLE_ALL>(ctx, s);
}

void launch_merge(fvdb_ctx* ctx, const MergeArgs& m) {
  const uint32_t grid = cdiv(m.B, 4);
  switch (kr_for(m.k)) {
    case 1: hipLaunchKernelGGL((merge_topk_kernel<1>), dim3(grid), dim3(256), 0, ctx->stream, m); break;
    case 2: hipLaunchKernelGGL((merge_topk_kernel<2>), dim3(grid), dim3(256), 0, ctx->stream, m); break;
    default: hipLaunchKernelGGL((merge_topk_kernel<4>), dim3(grid), dim3(256), 0, ctx->stream, m); break;
  }
}

int upload_table(fvdb_ivf* ivf) {
  fvdb_ctx* ctx = ivf->ctx;
  std::lock_guard<std::mutex> lk(ivf->mu);  // concurrent searches after a mutation: one of them uploads
  if (!ivf->table_dirty) return FVDB_OK;
  std::vector<uint32_t> off(ivf->nlist + 1, 0), blocks;
  std::vector<uint32_t> glob(ivf->nlist, 0);
  uint32_t mx = 0;
  for (uint32_t L = 0; L < ivf->nlist; ++L) {
    off[L] = (uint32_t)blocks.size();
    blocks.insert(blocks.end(), ivf->list_blocks[L].begin(), ivf->list_blocks[L].end());
    mx = std::max<uint32_t>(mx, (uint32_t)ivf->list_blocks[L].size());
    glob[L] = ivf->glob_set ? ivf->glob_blocks_host[L] : (uint32_t)ivf->list_blocks[L].size();
  }
  off[ivf->nlist] = (uint32_t)blocks.size();
  ivf->max_list_blocks = mx;
  HIPCHK(ctx, ivf->t_off.ensure(off.size() * 4));
  HIPCHK(ctx, ivf->t_blocks.ensure(std::max<size_t>(blocks.size(), 1) * 4));
  HIPCHK(ctx, ivf->t_glob.ensure(glob.size() * 4));
  HIPCHK(ctx, hipMemcpyAsync(ivf->t_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (!blocks.empty())
    HIPCHK(ctx, hipMemcpyAsync(ivf->t_blocks.p, blocks.data(), blocks.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ivf->t_glob.p, glob.data(), glob.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, ivf->t_len.ensure((size_t)ivf->nlist * 4));
  HIPCHK(ctx, hipMemcpyAsync(ivf->t_len.p, ivf->list_len.data(), (size_t)ivf->nlist * 4, hipMemcpyHostToDevice,
                             ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // host vectors go out of scope
  ivf->table_dirty = false;
  return FVDB_OK;
}

// queries as [B][dpad] in HBM: q_dev itself when d is a multiple of 4, else a padded copy
int padded_queries(fvdb_ivf* ivf, const Env& E, const float* q_dev, uint32_t B, const float** out) {
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  if (ivf->d == ivf->dpad) {
    *out = q_dev;
    return FVDB_OK;
  }
  HIPCHK(ctx, S.s_q.ensure((size_t)B * ivf->dpad * 4));
  const uint64_t tot = (uint64_t)B * ivf->dpad;
  hipLaunchKernelGGL(pad_rows_kernel, dim3(cdiv(tot, 256)), dim3(256), 0, ctx->stream, q_dev, ivf->d, ivf->dpad,
                     (uint64_t)B, S.s_q.as<float>());
  *out = S.s_q.as<float>();
  return FVDB_OK;
}

inline void mark(const fvdb_ivf* ivf, const Env& E, StageEvent e) {
  if (ivf->ctx->profiling) (void)hipEventRecord(E.S->sev[e], E.ctx->stream);
}

// One batch of a scan stage: B queries ([B][dpad], padded) with their probes[B][np] in HBM (nullptr: the single list of
// the centroid pool), and where the k results per query go (any of them may be null).
struct Batch {
  const float* qpad;
  const uint32_t* probes;
  uint32_t B, k, np;
  uint64_t* out_ids;
  float* out_dist;
  uint32_t* out_counts;
  uint64_t* out_keys;
  const float* given_thr = nullptr;  // sharded search: filter thresholds already agreed between the ranks ([B], device)
  bool glob_keys = false;            // wide selection: keys carry the logical index's seq (a shard of a larger index)
  // wide selection, one allow-set per query: the device table of live words and each query's entry in it (both null otherwise)
  const uint64_t* const* words = nullptr;
  const uint32_t* group = nullptr;
  // wide selection, radius search: the ball of radius[q] capped at k, its size to out_totals
  const float* radius = nullptr;  // [B], device
  uint32_t* out_totals = nullptr;
};

inline ListTable list_table(const fvdb_ivf* ivf) {
  return ListTable{ivf->t_off.as<uint32_t>(), ivf->t_blocks.as<uint32_t>(), ivf->nlist};
}

// merge of the partial lists a scan of `pool` left in `part`; the caller adds what only it has (out_probes, qlist)
MergeArgs merge_args(const PoolView& pool, const ListTable& lists, const uint32_t* glob_blocks, const DBuf& part,
                     uint32_t maxsegs, uint32_t segb, const Batch& b) {
  MergeArgs m{};
  m.pool = pool;
  m.lists = lists;
  m.probes = b.probes;
  m.glob_blocks = glob_blocks;
  m.part = part.as<uint2>();
  m.B = b.B;
  m.k = b.k;
  m.nprobe = b.np;
  m.maxsegs = maxsegs;
  m.segb = segb;
  m.out_ids = b.out_ids;
  m.out_dist = b.out_dist;
  m.out_counts = b.out_counts;
  m.out_keys = b.out_keys;
  return m;
}

// ---- the full centroid ranking (kernels_rank.h): kc above the register top-k ----
// Arena of one chunk of queries: the ranking is cut so that its distance words stay under this.
constexpr uint64_t kRankArenaBytes = 256ull << 20;
// What a search of np = min(nprobe, nlist) lists needs beyond the register path, asked by every entry point before it
// touches the device: the full ranking sorts the whole centroid table in one workgroup's LDS.
int check_rank(fvdb_ctx* ctx, const fvdb_ivf* ivf, uint32_t np) {
  if (np > FVDB_MAX_K && ivf->nlist > kRankSortMaxLists)
    FAIL(ctx, FVDB_E_UNSUPPORTED, "nprobe above FVDB_MAX_K needs an index of at most 16384 lists");
  return FVDB_OK;
}

// Coarse stage for kc > FVDB_MAX_K: every centroid scored into a per-query arena with the exact fold, then one
// workgroup per query sorts (distance bits, cluster position) and keeps the first kc.  Same outputs as run_coarse.
int run_coarse_rank(fvdb_ivf* ivf, const Env& E, const float* qpad, uint32_t B, uint32_t kc, uint32_t* out_probes,
                    float* out_dist) {
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  int rc = check_rank(ctx, ivf, kc);
  if (rc) return rc;
  const uint32_t cblocks = ivf->cpool.used_blocks, n = cblocks * 64;
  uint32_t P = 1;
  while (P < n) P <<= 1;
  const uint32_t lds = P * 8;
  const uint32_t threads = std::min<uint32_t>(kRankThreads, std::max<uint32_t>(64, P / 2));
  const uint32_t chunk = (uint32_t)std::min<uint64_t>(B, std::max<uint64_t>(1, kRankArenaBytes / ((uint64_t)n * 4)));
  HIPCHK(ctx, S.s_rarena.ensure((size_t)chunk * n * 4));
  HIPCHK(ctx, S.s_rbase.ensure((size_t)chunk * 2 * 4));
  HIPCHK(ctx, S.s_entries.ensure((size_t)chunk * 8));
  HIPCHK(ctx, S.s_ceoff.ensure(16));
  HIPCHK(ctx, S.s_cioff.ensure(16));
  HIPCHK(ctx, S.s_scalars.ensure(kScalarsBytes));
  // the attribute belongs to the function (on this device), not to the launch: every call sets the same value, the
  // largest sort served, so that searches of indexes of different sizes on different host threads never lower it
  // under one another
  HIPCHK(ctx, hipFuncSetAttribute((const void*)rank_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(kRankSortMaxLists * 8)));
  const ListTable clist{ivf->c_off.as<uint32_t>(), ivf->c_blocks.as<uint32_t>(), 1};
  const PoolView cpool = ivf->cpool.view();
  const uint32_t grid = (uint32_t)ctx->num_cus * ivf_knobs().scan_wgs_per_cu;
  mark(ivf, E, EV_COARSE_BEGIN);
  for (uint32_t o = 0; o < B; o += chunk) {
    const uint32_t b = std::min(chunk, B - o);
    hipLaunchKernelGGL(plan_all_kernel, dim3(cdiv(b, 256)), dim3(256), 0, ctx->stream, b, cblocks, 1u, 16u,
                       S.s_ceoff.as<uint32_t>(), S.s_cioff.as<uint32_t>(), S.s_entries.as<uint2>(),
                       S.scalar(SC_COARSE_ITEMS), S.scalar(SC_COARSE_HEAD));
    hipLaunchKernelGGL(rank_base_kernel, dim3(cdiv(b, 256)), dim3(256), 0, ctx->stream, b, cblocks, S.s_rbase.as<uint32_t>());
    const uint32_t items = cblocks * cdiv(b, 16);
    hipLaunchKernelGGL(wide_score_kernel<0>, dim3(std::min(grid, std::max<uint32_t>(1u, cdiv(items, 4)))), dim3(256), 0,
                       ctx->stream, cpool.data, cpool.valid, cpool.d4, clist.off, clist.blocks, 1u, S.s_ceoff.as<uint32_t>(),
                       S.s_cioff.as<uint32_t>(), (const u32x2*)S.s_entries.as<uint2>(), S.scalar(SC_COARSE_ITEMS),
                       S.scalar(SC_COARSE_HEAD), qpad + (size_t)o * ivf->dpad, ivf->dpad, 1u, 1u, S.s_rbase.as<uint32_t>(),
                       S.s_rarena.as<uint32_t>(), (uint64_t)n);
    if (o + b == B) mark(ivf, E, EV_COARSE_SCANNED);
    RankArgs r{};
    r.pool = cpool;
    r.lists = clist;
    r.arena = S.s_rarena.as<uint32_t>();
    r.n = n;
    r.P = P;
    r.np = kc;
    r.out_probes = out_probes + (size_t)o * kc;
    r.out_dist = out_dist ? out_dist + (size_t)o * kc : nullptr;
    hipLaunchKernelGGL(rank_sort_kernel, dim3(b), dim3(threads), lds, ctx->stream, r);
  }
  mark(ivf, E, EV_COARSE_DONE);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// Coarse stage: rank the centroid table for B queries, keep kc nearest per query.
// Writes u32 cluster ids to out_probes[B][kc] (probe order) and, optionally, their distances.
int run_coarse(fvdb_ivf* ivf, const Env& E, const float* qpad, uint32_t B, uint32_t kc, uint32_t* out_probes,
               float* out_dist) {
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  if (kc > FVDB_MAX_K) return run_coarse_rank(ivf, E, qpad, B, kc, out_probes, out_dist);
  if (ivf->coarse_mode == 0 && !ivf_knobs().coarse_exact && ivf->dpad % 16 == 0 && kc <= 48 && ivf->nlist >= 64 && B > 0 &&
      (uint64_t)B * ivf->nlist < (1ull << 31)) {
    // matrix cores propose 64 candidates per query; the reference's arithmetic decides (kernels_coarse.h)
    const uint32_t nlist = ivf->nlist;
    const float* cpad = ivf->d == ivf->dpad ? ivf->d_centroids_rm.as<float>() : ivf->d_cent_pad.as<float>();
    HIPCHK(ctx, S.s_qnorm.ensure((size_t)B * 4));
    HIPCHK(ctx, S.s_A.ensure((size_t)B * nlist * 4));
    mark(ivf, E, EV_COARSE_BEGIN);
    hipLaunchKernelGGL(row_sqnorm_wave_kernel, dim3(cdiv(B, 4)), dim3(256), 0, ctx->stream, qpad, ivf->dpad, ivf->dpad, B,
                       S.s_qnorm.as<float>());
    const uint32_t waves = cdiv(B, 32) * cdiv(nlist, 64);
    hipLaunchKernelGGL(coarse_gemm_kernel, dim3(cdiv(waves, 4)), dim3(256), 0, ctx->stream, qpad, cpad,
                       S.s_qnorm.as<float>(), ivf->d_cnorm.as<float>(), B, nlist, ivf->dpad, S.s_A.as<float>());
    mark(ivf, E, EV_COARSE_SCANNED);
    hipLaunchKernelGGL(coarse_select_kernel, dim3(cdiv(B, 4)), dim3(256), 0, ctx->stream, S.s_A.as<float>(), qpad, cpad,
                       S.s_qnorm.as<float>(), ivf->d_cnmax.as<float>(), B, nlist, ivf->d, ivf->dpad, 64u, kc,
                       out_probes, out_dist, ivf->fb_word(FB_COARSE));
    mark(ivf, E, EV_COARSE_DONE);
    HIPCHK(ctx, hipGetLastError());
    return FVDB_OK;
  }
  const uint32_t cblocks = ivf->cpool.used_blocks;
  const uint32_t segb = 1, Q = q_for(kc);
  const uint32_t maxsegs = cblocks;
  HIPCHK(ctx, S.s_cpart.ensure((size_t)B * maxsegs * kc * 8));
  HIPCHK(ctx, S.s_entries.ensure((size_t)B * std::max<uint32_t>(kc, 1) * 8));
  HIPCHK(ctx, S.s_ceoff.ensure(16));
  HIPCHK(ctx, S.s_cioff.ensure(16));
  HIPCHK(ctx, S.s_scalars.ensure(kScalarsBytes));
  hipLaunchKernelGGL(plan_all_kernel, dim3(cdiv(std::max<uint32_t>(B, 1), 256)), dim3(256), 0, ctx->stream, B, cblocks,
                     segb, Q, S.s_ceoff.as<uint32_t>(), S.s_cioff.as<uint32_t>(), S.s_entries.as<uint2>(),
                     S.scalar(SC_COARSE_ITEMS), S.scalar(SC_COARSE_HEAD));
  const ListTable clist{ivf->c_off.as<uint32_t>(), ivf->c_blocks.as<uint32_t>(), 1};
  ScanLaunch s{ivf->cpool.view(), clist.off, clist.blocks, 1, S.s_ceoff.as<uint32_t>(), S.s_cioff.as<uint32_t>(),
               S.s_entries.as<uint2>(), S.scalar(SC_COARSE_ITEMS), S.scalar(SC_COARSE_HEAD), qpad, ivf->dpad, segb, kc, 1,
               maxsegs, S.s_cpart.as<uint2>(), cdiv(cblocks, segb) * cdiv(B, Q)};
  mark(ivf, E, EV_COARSE_BEGIN);
  launch_scan(ctx, s, ROLE_COARSE);
  mark(ivf, E, EV_COARSE_SCANNED);
  MergeArgs m = merge_args(ivf->cpool.view(), clist, ivf->c_glob.as<uint32_t>(), S.s_cpart, maxsegs, segb,
                           Batch{qpad, nullptr, B, kc, 1, nullptr, out_dist, nullptr, nullptr});
  m.out_probes = out_probes;
  launch_merge(ctx, m);
  mark(ivf, E, EV_COARSE_DONE);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// Blocks per segment of the exact scan over lists of at most max_blocks blocks: enough (segment, group) items to fill
// 256 CUs x 32 waves, without shredding long lists.
uint32_t segb_for(uint32_t max_blocks, uint32_t B, uint32_t nprobe) {
  const uint64_t pairs = (uint64_t)B * nprobe;
  if (max_blocks >= 4096) return 16;
  if (pairs >= 4096) return 4;
  if (pairs >= 512) return 2;
  return 1;
}
uint32_t pick_segb(fvdb_ivf* ivf, uint32_t B, uint32_t nprobe) {
  const int forced = ivf_knobs().segb;
  return forced > 0 ? (uint32_t)forced : segb_for(ivf->max_list_blocks, B, nprobe);
}
// queries whose fine-stage partial buffer stays under ~1 GiB
uint64_t queries_per_gib(uint32_t max_blocks, uint32_t segb, uint32_t k, uint32_t np) {
  const uint64_t per_q = (uint64_t)np * std::max<uint32_t>(1, cdiv(max_blocks, segb)) * k * 8;
  return (1ull << 30) / std::max<uint64_t>(per_q, 1);
}

// The plan kernels (kernels_scan.h): n = B * np (query, probe) pairs -> per-list entries and the scan's work items.
// cnt[] must be zero on entry; with rezero_cnt the scan kernel leaves it zero again for the next plan of the batch.
void launch_plan(fvdb_ivf* ivf, const Env& E, const uint32_t* probes, uint32_t n, uint32_t np, uint32_t segb, uint32_t Q,
                 unsigned long long* stats, uint32_t* rezero_cnt, uint32_t lsplit = 0xFFFFFFFFu, uint32_t segb_tail = 0) {
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  const uint32_t* list_off = ivf->t_off.as<uint32_t>();
  hipLaunchKernelGGL(plan_count_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, probes, n, S.s_cnt.as<uint32_t>(),
                     list_off);
  hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, S.s_cnt.as<uint32_t>(), list_off,
                     ivf->t_len.as<uint32_t>(), ivf->nlist, segb, Q, S.s_eoff.as<uint32_t>(), S.s_ioff.as<uint32_t>(),
                     S.s_fill.as<uint32_t>(), S.scalar(SC_FINE_ITEMS), S.scalar(SC_FINE_HEAD), stats, rezero_cnt, lsplit,
                     segb_tail);
  hipLaunchKernelGGL(plan_fill_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, probes, n, np,
                     S.s_eoff.as<uint32_t>(), S.s_fill.as<uint32_t>(), S.s_entries.as<uint2>(), list_off);
}
inline unsigned long long* scan_stats(const IvfScratch& S) { return (unsigned long long*)S.scalar(SC_STATS); }

// what the plan kernels write (s_cnt is also cleared by prep_queries_kernel, s_part sized by the caller)
int plan_scratch(fvdb_ivf* ivf, const Env& E, uint32_t B, uint32_t np) {
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  const uint32_t nlist = ivf->nlist;
  HIPCHK(ctx, S.s_cnt.ensure((size_t)nlist * 4));
  HIPCHK(ctx, S.s_fill.ensure((size_t)nlist * 4));
  HIPCHK(ctx, S.s_eoff.ensure((size_t)(nlist + 1) * 4));
  HIPCHK(ctx, S.s_ioff.ensure((size_t)(nlist + 1) * 4));
  HIPCHK(ctx, S.s_entries.ensure((size_t)B * np * 8));
  return FVDB_OK;
}

// Fine stage for B queries whose probes[B][np] are already in HBM: every row scored with the reference's fold.
int run_fine_exact(fvdb_ivf* ivf, const Env& E, const Batch& b, int role) {
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  const uint32_t nlist = ivf->nlist;
  const uint32_t segb = pick_segb(ivf, b.B, b.np), Q = q_for(b.k);
  const uint32_t maxsegs = std::max<uint32_t>(1, cdiv(ivf->max_list_blocks, segb));
  const uint64_t part_elems = (uint64_t)b.B * b.np * maxsegs * b.k;
  if (part_elems >= (1ull << 32)) FAIL(ctx, FVDB_E_UNSUPPORTED, "batch too large for one launch (sub-batch it)");
  int rc = plan_scratch(ivf, E, b.B, b.np);
  if (rc) return rc;
  HIPCHK(ctx, S.s_part.ensure((size_t)part_elems * 8));
  HIPCHK(ctx, S.s_scalars.ensure(kScalarsBytes));
  // nobody cleared cnt[] for this path, and no later plan of the batch needs it cleared again
  HIPCHK(ctx, hipMemsetAsync(S.s_cnt.p, 0, (size_t)nlist * 4, ctx->stream));
  launch_plan(ivf, E, b.probes, b.B * b.np, b.np, segb, Q, scan_stats(S), /*rezero_cnt=*/nullptr);
  mark(ivf, E, EV_SCAN_BEGIN);
  const ListTable lists = list_table(ivf);
  ScanLaunch s{list_pool(ivf, E), lists.off, lists.blocks, nlist, S.s_eoff.as<uint32_t>(), S.s_ioff.as<uint32_t>(),
               S.s_entries.as<uint2>(), S.scalar(SC_FINE_ITEMS), S.scalar(SC_FINE_HEAD), b.qpad, ivf->dpad, segb, b.k, b.np,
               maxsegs, S.s_part.as<uint2>()};
  s.f16 = ivf->f16;
  launch_scan(ctx, s, role);
  mark(ivf, E, EV_SCAN_DONE);
  launch_merge(ctx, merge_args(list_pool(ivf, E), lists, ivf->t_glob.as<uint32_t>(), S.s_part, maxsegs, segb, b));
  mark(ivf, E, EV_FINE_DONE);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// ---- fine stage on the matrix cores (kernels_mfma.h): threshold from the nearest list, fp16 MFMA filter over all
// probed lists, exact verification of the survivors, exact rescan of unproven queries.  Same outputs as run_fine_exact.
constexpr uint32_t kMfmaSlack = 6;     // phase A scores k + 6 rows
constexpr uint32_t kMfmaCmax = 4096;   // survivor slots per query

// Shapes the matrix-core filter serves.  thr_share_ok asks this too, and there every rank of a sharded search must
// answer alike: nothing that differs between the ranks may enter.
bool mfma_shape_ok(const fvdb_ivf* ivf, uint32_t B, uint32_t k, uint32_t np) {
  return ivf->dpad % 16 == 0 && k + kMfmaSlack <= 32 && np <= 256 && B >= 32 && B <= 16384;
}
// the filter reads fp16 rows (stored or mirrored)
inline bool half_rows(const fvdb_ivf* ivf) { return ivf->f16 || ivf->pool.half() != nullptr; }
// those rows against the rows the reference sees (mfma_error_bound): 0 the same, 1 rounded to nearest, 2 truncated
inline int x_rounded(const fvdb_ivf* ivf) { return ivf->f16 ? 0 : (ivf->pool.half() ? 1 : 2); }

// What one matrix-core batch runs with, derived once from the index, the knobs and the batch shape.
struct MfmaPlan {
  bool wg;            // the workgroup form of the filter (kernels_mfma_wg.h), else the wave form
  int M;              // 16-query tiles per group
  uint32_t Q, ka, cmax;
  uint32_t segb, segbA;              // blocks per segment: the filter, the threshold pass
  uint32_t lsplit, segb_tail;        // workgroup form: lists >= lsplit in segments of segb_tail (MfmaScanArgs::lsplit)
  uint32_t fsegb, fmaxsegs;          // partial lists of the exact rescan: same geometry as the exact scan's
  uint64_t fpart;
  uint32_t grid, wg_grid, wg_lds;    // wave form (and the rescan); workgroup form and its LDS bytes
  bool half_rows;
  int x_rounded;
};

int mfma_plan(fvdb_ivf* ivf, fvdb_ctx* ctx, const IvfKnobs& kn, uint32_t B, uint32_t k, uint32_t np, MfmaPlan* out) {
  MfmaPlan P{};
  P.half_rows = half_rows(ivf);
  P.x_rounded = x_rounded(ivf);
  // workgroup form: fp16 rows, dpad a multiple of 128, 32 or 64 queries per group
  int wgM = kn.mfma_wg_m;
  if (mfma_wg_lds_bytes(ivf->dpad, 16u * wgM) > 64u * 1024u) wgM = 2;  // wide rows: the 32-query tile still fits
  P.wg = kn.mfma_wg && kn.mfma_m == 2 && P.half_rows && ivf->dpad % 128 == 0 &&
         mfma_wg_lds_bytes(ivf->dpad, 16u * wgM) <= 64u * 1024u;
  P.M = P.wg ? wgM : kn.mfma_m;
  P.Q = 16u * P.M;
  P.ka = k + kMfmaSlack;
  P.cmax = kMfmaCmax;
  P.segbA = kn.mfma_segb_a;
  P.segb = P.wg ? kn.mfma_wg_segb : (kn.mfma_segb > 0 ? (uint32_t)kn.mfma_segb : pick_segb(ivf, B, np));
  P.lsplit = 0xFFFFFFFFu;
  P.segb_tail = P.segb;
  if (P.wg && kn.mfma_wg_tail_pct > 0 && kn.mfma_wg_segb_tail > 0 && (uint32_t)kn.mfma_wg_segb_tail < P.segb) {
    P.lsplit = (uint32_t)((uint64_t)ivf->nlist * (uint32_t)(100 - std::min(kn.mfma_wg_tail_pct, 100)) / 100);
    P.segb_tail = (uint32_t)kn.mfma_wg_segb_tail;
  }
  P.fsegb = pick_segb(ivf, B, np);
  P.fmaxsegs = std::max<uint32_t>(1, cdiv(ivf->max_list_blocks, P.fsegb));
  P.fpart = (uint64_t)B * np * P.fmaxsegs * k;
  if (P.fpart >= (1ull << 32)) FAIL(ctx, FVDB_E_UNSUPPORTED, "batch too large for one launch (sub-batch it)");
  P.grid = (uint32_t)ctx->num_cus * kn.mfma_wgs_per_cu;
  P.wg_grid = (uint32_t)ctx->num_cus * kn.mfma_wg_per_cu;
  P.wg_lds = mfma_wg_lds_bytes(ivf->dpad, P.Q);
  *out = P;
  return FVDB_OK;
}

int mfma_scratch(fvdb_ivf* ivf, const Env& E, const MfmaPlan& P, uint32_t B, uint32_t np) {
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  HIPCHK(ctx, S.s_qh.ensure((size_t)(B + 1) * ivf->dpad * 2));
  HIPCHK(ctx, S.s_qn2.ensure((size_t)B * 4));
  HIPCHK(ctx, S.s_thr.ensure((size_t)B * 4));
  HIPCHK(ctx, S.s_tA.ensure((size_t)B * 4));
  HIPCHK(ctx, S.s_pa.ensure((size_t)B * 4));
  HIPCHK(ctx, S.s_mslots.ensure((size_t)B * 64 * 4));
  HIPCHK(ctx, S.s_surv.ensure((size_t)B * P.cmax * 8));
  HIPCHK(ctx, S.s_sdist.ensure((size_t)B * P.cmax * 4));
  HIPCHK(ctx, S.s_scnt.ensure((size_t)(B + 2) * 4));  // [B] survivor counts, then nfail and the rescan queue head
  HIPCHK(ctx, S.s_fail.ensure((size_t)B * 4));
  HIPCHK(ctx, S.s_part.ensure((size_t)P.fpart * 8));
  int rc = plan_scratch(ivf, E, B, np);
  if (rc) return rc;
  HIPCHK(ctx, S.s_scalars.ensure(kScalarsBytes));
  return FVDB_OK;
}

// fp16 queries (+ the zero row), |q|^2; clears cnt[], the survivor counts with nfail and the queue head, the row slots
void launch_prep_queries(fvdb_ivf* ivf, const Env& E, const float* qpad, uint32_t B) {
  IvfScratch& S = *E.S;
  hipLaunchKernelGGL(prep_queries_kernel, dim3(cdiv(B + 1, 4)), dim3(256), 0, E.ctx->stream, qpad, B, ivf->dpad,
                     (_Float16*)S.s_qh.p, S.s_qn2.as<float>(), S.s_cnt.as<uint32_t>(), ivf->nlist,
                     S.s_scnt.as<uint32_t>(), S.s_mslots.as<uint32_t>());
}

ThresholdArgs threshold_args(fvdb_ivf* ivf, const Env& E, const float* qpad, const uint32_t* probes, uint32_t B,
                             uint32_t k, uint32_t np, float* thr_out) {
  const IvfScratch& S = *E.S;
  ThresholdArgs t{};
  t.rows = ivf->pool.half() ? ivf->pool.half() : ivf->pool.data();
  t.pool_valid = live_words(ivf, E);
  t.pool_norms = ivf->pool.norms();
  t.d4 = ivf->d4;
  t.lists = list_table(ivf);
  t.list_len = ivf->t_len.as<uint32_t>();
  t.probes = probes;
  t.qh = (const _Float16*)S.s_qh.p;
  t.queries = qpad;
  t.qn = S.s_qn2.as<float>();
  t.xmax_bits = ivf->d_xmax.as<uint32_t>();
  t.B = B;
  t.np = np;
  t.ka = k + kMfmaSlack;
  t.dpad = ivf->dpad;
  t.capA = ivf_knobs().mfma_cap_a;
  t.min_rows = 256u;
  t.rows_f16 = x_rounded(ivf);
  t.thr = thr_out;
  return t;
}
void launch_threshold_direct(fvdb_ivf* ivf, fvdb_ctx* ctx, const ThresholdArgs& t) {
  if (half_rows(ivf)) hipLaunchKernelGGL((threshold_direct_kernel<true>), dim3(cdiv(t.B, 4)), dim3(256), 0, ctx->stream, t);
  else hipLaunchKernelGGL((threshold_direct_kernel<false>), dim3(cdiv(t.B, 4)), dim3(256), 0, ctx->stream, t);
}

MfmaScanArgs mfma_scan_args(fvdb_ivf* ivf, const Env& E, const MfmaPlan& P, const Batch& b) {
  const IvfScratch& S = *E.S;
  MfmaScanArgs a{};
  a.pool_data = ivf->pool.half() ? ivf->pool.half() : ivf->pool.data();
  a.pool_valid = live_words(ivf, E);
  a.pool_norms = ivf->pool.norms();
  a.d4 = ivf->d4;
  a.list_off = ivf->t_off.as<uint32_t>();
  a.list_blocks = ivf->t_blocks.as<uint32_t>();
  a.nlist = ivf->nlist;
  a.entry_off = S.s_eoff.as<uint32_t>();
  a.item_off = S.s_ioff.as<uint32_t>();
  a.entries = (const u32x2*)S.s_entries.p;
  a.n_items = S.scalar(SC_FINE_ITEMS);
  a.head = S.scalar(SC_FINE_HEAD);
  a.qh = (const _Float16*)S.s_qh.p;
  a.zero_row = b.B;
  a.dpad = ivf->dpad;
  a.segb = P.segb;
  // sharded search: the thresholds were computed once per query by the rank owning the list and combined across the
  // ranks before this call (ivf_shared_thresholds + the exchange in comm_sharded.h)
  a.thr = b.given_thr ? b.given_thr : S.s_thr.as<float>();
  a.cmax = P.cmax;
  a.surv = (u32x2*)S.s_surv.p;
  a.sval = S.s_sdist.as<float>();
  a.scnt = S.s_scnt.as<uint32_t>();
  a.slots = S.s_mslots.as<uint32_t>();
  a.capA = ivf_knobs().mfma_cap_a;
  a.groups_in_item = ivf_knobs().mfma_groups_in_item ? 1u : 0u;
  a.lsplit = P.lsplit;
  a.segb_tail = P.segb_tail;
  return a;
}

// the wave form of the matrix-core scan: MODE 0 filters, MODE 1 collects the smallest v per row slot
using MfmaKernel = decltype(&scan_mfma_kernel<2, 1, 0>);
template <int M, int MODE>
MfmaKernel mfma_kernel_of(bool f16) {
  return f16 ? scan_mfma_kernel<M, 1, MODE> : scan_mfma_kernel<M, 0, MODE>;
}
template <int MODE>
void launch_mfma(fvdb_ctx* ctx, const MfmaScanArgs& a, const MfmaPlan& P) {
  const MfmaKernel kernel = P.M == 1   ? mfma_kernel_of<1, MODE>(P.half_rows)
                            : P.M == 2 ? mfma_kernel_of<2, MODE>(P.half_rows)
                                       : mfma_kernel_of<4, MODE>(P.half_rows);
  hipLaunchKernelGGL(kernel, dim3(P.grid), dim3(256), 0, ctx->stream, a);
}

// A. threshold: the smallest v per row slot over the head of a near, well-filled list -> (k+6)-th smallest -> thr.
//    Direct form: one wave per query, one launch (kernels_mfma.h).  FVDB_MFMA_THRESHOLD_PASS=1 keeps the earlier
//    form (first_probe + plan + matrix-core MODE 1 pass + threshold_kernel) for A/B runs.
void mfma_threshold(fvdb_ivf* ivf, const Env& E, const MfmaPlan& P, const Batch& b, const MfmaScanArgs& a) {
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  if (b.given_thr) return;
  if (!ivf_knobs().mfma_threshold_pass) {
    launch_threshold_direct(ivf, ctx, threshold_args(ivf, E, b.qpad, b.probes, b.B, b.k, b.np, S.s_thr.as<float>()));
    return;
  }
  hipLaunchKernelGGL(first_probe_kernel, dim3(cdiv(b.B, 256)), dim3(256), 0, ctx->stream, b.probes, b.B, b.np,
                     ivf->t_len.as<uint32_t>(), 256u, S.s_pa.as<uint32_t>());
  // cnt[] is zero on entry: cleared by prep_queries_kernel for this plan, by plan_scan_kernel for the filter's
  launch_plan(ivf, E, S.s_pa.as<uint32_t>(), b.B, 1, P.segbA, P.Q, nullptr, S.s_cnt.as<uint32_t>());
  MfmaScanArgs head = a;
  head.segb = P.segbA;
  launch_mfma<1>(ctx, head, P);
  hipLaunchKernelGGL(threshold_kernel, dim3(cdiv(b.B, 4)), dim3(256), 0, ctx->stream, S.s_mslots.as<uint32_t>(),
                     S.s_pa.as<uint32_t>(), S.s_qn2.as<float>(), ivf->d_xmax.as<uint32_t>(), b.B, P.ka, ivf->dpad,
                     P.x_rounded, S.s_thr.as<float>());
}

// the filter over the planned items, in the form the plan chose
void launch_filter(fvdb_ctx* ctx, const MfmaScanArgs& a, const MfmaPlan& P) {
  if (P.wg) {
    const MfmaKernel kernel = P.M == 4 ? scan_mfma_wg_kernel<4> : scan_mfma_wg_kernel<2>;
    hipLaunchKernelGGL(kernel, dim3(P.wg_grid), dim3(256), P.wg_lds, ctx->stream, a);
  } else {
    launch_mfma<0>(ctx, a, P);
  }
}

#ifdef FVDB_MFMA_STAMPS_BUILD
// diagnostic build (FVDB_MFMA_STAMPS=<first launch to print>): per-item timeline of the workgroup filter, written by
// the kernel into a buffer the index owns, read back and summarised on stderr for three launches
constexpr uint32_t kStampsCap = 32768;
int mfma_stamps_begin(fvdb_ivf* ivf, fvdb_ctx* ctx, const MfmaPlan& P, MfmaScanArgs* a) {
  const int stamps_env = ivf_knobs().mfma_stamps;
  const bool stamp_now = P.wg && stamps_env && ++ivf->mfma_stamps_launch >= stamps_env && ivf->mfma_stamps_launch < stamps_env + 3;
  if (!stamp_now) return FVDB_OK;
  HIPCHK(ctx, ivf->d_mfma_stamps.ensure((size_t)kStampsCap * 64));
  HIPCHK(ctx, hipMemsetAsync(ivf->d_mfma_stamps.p, 0, (size_t)kStampsCap * 64, ctx->stream));
  a->stamps = ivf->d_mfma_stamps.as<unsigned long long>();
  a->stamps_cap = kStampsCap;
  return FVDB_OK;
}
int mfma_stamps_report(fvdb_ivf* ivf, fvdb_ctx* ctx, MfmaScanArgs* a) {
  if (!a->stamps) return FVDB_OK;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<unsigned long long> h((size_t)kStampsCap * 8);
  HIPCHK(ctx, hipMemcpy(h.data(), a->stamps, h.size() * 8, hipMemcpyDeviceToHost));
  unsigned long long t_min = ~0ull, t_max = 0;
  size_t n = 0;
  for (size_t i = 0; i < kStampsCap; ++i)
    if (h[i * 8 + 3]) {
      t_min = std::min(t_min, h[i * 8]);
      t_max = std::max(t_max, h[i * 8 + 3]);
      ++n;
    }
  double s_loc = 0, s_tile = 0, s_comp = 0, s_steps = 0, s_blocks = 0;
  size_t per_xcd[16] = {0};
  std::vector<double> per_step;
  for (size_t i = 0; i < kStampsCap; ++i) {
    const unsigned long long* r = &h[i * 8];
    if (!r[3]) continue;
    const double steps = (double)((r[5] + 3) / 4) * (double)(ivf->dpad / 16);
    s_loc += (double)(r[1] - r[0]);
    s_tile += (double)(r[2] - r[1]);
    s_comp += (double)(r[3] - r[2]);
    s_steps += steps;
    s_blocks += (double)r[5];
    per_xcd[r[7] & 15]++;
    per_step.push_back((double)(r[3] - r[2]) / steps);
  }
  std::sort(per_step.begin(), per_step.end());
  const double tick = 0.01;  // us per tick of the 100 MHz wall clock
  fprintf(stderr,
          "[mfma stamps] launch %d: %zu items, %0.f blocks, span %.1f us | per item (wave 0): locate %.2f us, tile %.2f us, "
          "compute %.2f us | per 16-dim step: mean %.3f us, p10 %.3f, p50 %.3f, p90 %.3f | items per XCD",
          ivf->mfma_stamps_launch, n, s_blocks, (double)(t_max - t_min) * tick, s_loc / n * tick, s_tile / n * tick, s_comp / n * tick,
          s_comp / s_steps * tick, per_step.empty() ? 0.0 : per_step[per_step.size() / 10] * tick,
          per_step.empty() ? 0.0 : per_step[per_step.size() / 2] * tick,
          per_step.empty() ? 0.0 : per_step[per_step.size() * 9 / 10] * tick);
  for (int x = 0; x < 8; ++x) fprintf(stderr, " %zu", per_xcd[x]);
  // when did the last item START, and how long were the items that finished last
  unsigned long long last_start = 0;
  for (size_t i = 0; i < kStampsCap; ++i)
    if (h[i * 8 + 3]) last_start = std::max(last_start, h[i * 8]);
  fprintf(stderr, " | last item drawn at %.1f us\n", (double)(last_start - t_min) * tick);
  a->stamps = nullptr;  // the refine pass is not stamped
  return FVDB_OK;
}
#else
inline int mfma_stamps_begin(fvdb_ivf*, fvdb_ctx*, const MfmaPlan&, MfmaScanArgs*) { return FVDB_OK; }
inline int mfma_stamps_report(fvdb_ivf*, fvdb_ctx*, MfmaScanArgs*) { return FVDB_OK; }
#endif

// B. filter over all probed lists
int mfma_filter(fvdb_ivf* ivf, const Env& E, const MfmaPlan& P, const Batch& b, MfmaScanArgs* a) {
  fvdb_ctx* ctx = E.ctx;
  launch_plan(ivf, E, b.probes, b.B * b.np, b.np, P.segb, P.Q, scan_stats(*E.S), E.S->s_cnt.as<uint32_t>(), P.lsplit,
              P.segb_tail);
  mark(ivf, E, EV_FILTER_BEGIN);
  int rc = mfma_stamps_begin(ivf, ctx, P, a);
  if (rc) return rc;
  launch_filter(ctx, *a, P);
  rc = mfma_stamps_report(ivf, ctx, a);
  if (rc) return rc;
  mark(ivf, E, EV_FILTER_DONE);
  return FVDB_OK;
}

// AUTO scan mode steers itself by two counters of the pinned copy of the counter block, each looked at every 2048
// matrix-core queries under ivf->mu (the watch is shared by every search on the index; the counters lag by the batches
// in flight).  First watch: does this batch go to the exact scan instead?
bool auto_backs_off(fvdb_ivf* ivf) {
  std::lock_guard<std::mutex> lk(ivf->mu);
  if (ivf->exact_batches_left > 0) {
    ivf->exact_batches_left -= 1;
    return true;
  }
  if (!(ivf->h_fb.p && ivf->mfma_q - ivf->q_seen >= 2048)) return false;
  // rescans among the matrix-core queries since the last look
  const uint64_t fb_now = ((volatile uint32_t*)ivf->h_fb.p)[FB_SCAN];
  const uint64_t dq = ivf->mfma_q - ivf->q_seen, dfb = fb_now - ivf->fb_seen;
  ivf->q_seen = ivf->mfma_q;
  ivf->fb_seen = fb_now;
  if (dfb * 8 > dq) {  // more than 1 in 8: the exact scan is cheaper here; look again after a while, ever more rarely
    ivf->backoff_len = std::min<uint32_t>(ivf->backoff_len ? ivf->backoff_len * 2 : 64, 4096);
    ivf->exact_batches_left = ivf->backoff_len;
    return true;
  }
  ivf->backoff_len = 0;
  return false;
}
// Second watch: does this batch get the refine pass?
bool auto_refines(fvdb_ivf* ivf) {
  std::lock_guard<std::mutex> lk(ivf->mu);
  if (ivf->h_fb.p && ivf->mfma_q - ivf->overflow_q >= 2048) {
    // worth five more launches per batch once more than one query in a thousand overflows (a stray one is cheaper to
    // rescan exactly)
    const volatile uint32_t* c = (const volatile uint32_t*)ivf->h_fb.p;
    const uint64_t now = (uint64_t)c[FB_OVERFLOW] + c[FB_REFINED], dq = ivf->mfma_q - ivf->overflow_q;
    if ((now - ivf->overflow_seen) * 1000 > dq) ivf->refine_batches_left = 1024;
    ivf->overflow_seen = now;
    ivf->overflow_q = ivf->mfma_q;
  }
  if (ivf->refine_batches_left == 0) return false;
  ivf->refine_batches_left -= 1;
  return true;
}

// B'. queries whose survivors outgrew the buffer get a threshold from those survivors and a second filter pass over
//     their probes alone (normally nobody: the three plan kernels and the filter find nothing to do)
int mfma_refine(fvdb_ivf* ivf, const Env& E, const MfmaPlan& P, const Batch& b, const MfmaScanArgs& a) {
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  HIPCHK(ctx, S.s_probes2.ensure((size_t)b.B * b.np * 4));
  hipLaunchKernelGGL(refine_threshold_kernel, dim3(cdiv(b.B, 4)), dim3(256), 0, ctx->stream, S.s_sdist.as<float>(),
                     S.s_scnt.as<uint32_t>(), b.probes, S.s_qn2.as<float>(), ivf->d_xmax.as<uint32_t>(), b.B, b.np, P.ka, P.cmax,
                     ivf->dpad, P.x_rounded, S.s_thr.as<float>(), S.s_probes2.as<uint32_t>(), ivf->fb_word(FB_REFINED, E.live != nullptr));
  launch_plan(ivf, E, S.s_probes2.as<uint32_t>(), b.B * b.np, b.np, P.segb, P.Q, nullptr, S.s_cnt.as<uint32_t>(), P.lsplit,
              P.segb_tail);
  launch_filter(ctx, a, P);
  return FVDB_OK;
}

// C. select
VerifyArgs verify_args(fvdb_ivf* ivf, const Env& E, const MfmaPlan& P, const Batch& b) {
  const IvfScratch& S = *E.S;
  VerifyArgs v{};
  v.pool = list_pool(ivf, E);
  v.lists = list_table(ivf);
  v.probes = b.probes;
  v.glob_blocks = ivf->t_glob.as<uint32_t>();
  v.queries = b.qpad;
  v.qn = S.s_qn2.as<float>();
  v.xmax_bits = ivf->d_xmax.as<uint32_t>();
  v.thr = b.given_thr ? b.given_thr : S.s_thr.as<float>();
  v.remote_thr = b.given_thr ? 1 : 0;
  v.surv = (const u32x2*)S.s_surv.p;
  v.sval = S.s_sdist.as<float>();
  v.scnt = S.s_scnt.as<uint32_t>();
  v.B = b.B;
  v.k = b.k;
  v.ka = P.ka;
  v.nprobe = b.np;
  v.d = ivf->dpad;
  v.dpad = ivf->dpad;
  v.cmax = P.cmax;
  v.rows_f16 = P.x_rounded;
  v.rows_rm = ivf->pool.rm();
  v.out_ids = b.out_ids;
  v.out_dist = b.out_dist;
  v.out_counts = b.out_counts;
  v.out_keys = b.out_keys;
  v.fallbacks = ivf->fb_word(FB_SCAN, E.live != nullptr);
  v.reasons = ivf->fb_word(FB_REASONS, E.live != nullptr);
  v.fail_list = S.s_fail.as<uint32_t>();
  v.nfail = S.s_scnt.as<uint32_t>() + b.B;
  return v;
}
void launch_select(fvdb_ivf* ivf, fvdb_ctx* ctx, const VerifyArgs& v) {
  if (ivf->f16) hipLaunchKernelGGL((select_kernel<1>), dim3(cdiv(v.B, 4)), dim3(256), 0, ctx->stream, v);
  else hipLaunchKernelGGL((select_kernel<0>), dim3(cdiv(v.B, 4)), dim3(256), 0, ctx->stream, v);
}

FallbackArgs fallback_args(fvdb_ivf* ivf, const Env& E, const MfmaPlan& P, const Batch& b, const VerifyArgs& v) {
  const IvfScratch& S = *E.S;
  FallbackArgs fa{};
  fa.pool = list_pool(ivf, E);
  fa.lists = v.lists;
  fa.probes = b.probes;
  fa.queries = b.qpad;
  fa.fail_list = v.fail_list;
  fa.nfail = v.nfail;
  fa.head = S.s_scnt.as<uint32_t>() + b.B + 1;
  fa.k = b.k;
  fa.nprobe = b.np;
  fa.dpad = ivf->dpad;
  fa.segb = P.fsegb;
  fa.maxsegs = P.fmaxsegs;
  fa.part = (u32x2*)S.s_part.p;
  return fa;
}

// exact rescan of the queries the select stage did not prove (normally none: both kernels return at once)
void mfma_rescan(fvdb_ivf* ivf, const Env& E, const MfmaPlan& P, const Batch& b, const VerifyArgs& v) {
  fvdb_ctx* ctx = E.ctx;
  const FallbackArgs fa = fallback_args(ivf, E, P, b, v);
  if (ivf->f16) hipLaunchKernelGGL((fallback_scan_kernel<1>), dim3(P.grid), dim3(256), 0, ctx->stream, fa);
  else hipLaunchKernelGGL((fallback_scan_kernel<0>), dim3(P.grid), dim3(256), 0, ctx->stream, fa);
  MergeArgs fm = merge_args(fa.pool, fa.lists, v.glob_blocks, E.S->s_part, P.fmaxsegs, P.fsegb, b);
  fm.qlist = v.fail_list;
  fm.nq = v.nfail;
  launch_merge(ctx, fm);
}

// the counter block, for AUTO's watches: a 32-byte copy into pinned memory, nobody waits for it
int mfma_watch_counters(fvdb_ivf* ivf, fvdb_ctx* ctx, uint32_t B) {
  {
    std::lock_guard<std::mutex> lk(ivf->mu);
    const bool fresh = ivf->h_fb.p == nullptr;
    HIPCHK(ctx, ivf->h_fb.ensure(64));
    if (fresh) std::memset(ivf->h_fb.p, 0, 64);
    ivf->mfma_q += B;
  }
  HIPCHK(ctx, hipMemcpyAsync(ivf->h_fb.p, ivf->s_fallbacks.p, kFbBytes, hipMemcpyDeviceToHost, ctx->stream));
  return FVDB_OK;
}

int run_fine_mfma(fvdb_ivf* ivf, const Env& E, const Batch& b) {
  fvdb_ctx* ctx = E.ctx;
  const IvfKnobs& kn = ivf_knobs();
  MfmaPlan P;
  int rc = mfma_plan(ivf, ctx, kn, b.B, b.k, b.np, &P);
  if (rc) return rc;
  rc = mfma_scratch(ivf, E, P, b.B, b.np);
  if (rc) return rc;
  mark(ivf, E, EV_SCAN_BEGIN);
  launch_prep_queries(ivf, E, b.qpad, b.B);
  MfmaScanArgs a = mfma_scan_args(ivf, E, P, b);
  mfma_threshold(ivf, E, P, b, a);
  rc = mfma_filter(ivf, E, P, b, &a);
  if (rc) return rc;
  // thresholds agreed between the ranks are not refined; AUTO refines only while it has seen the need
  if (!b.given_thr && !kn.mfma_no_refine && (ivf->scan_mode != FVDB_SCAN_AUTO || auto_refines(ivf))) {
    rc = mfma_refine(ivf, E, P, b, a);
    if (rc) return rc;
  }
  mark(ivf, E, EV_SCAN_DONE);
  E.S->pend_filter = true;
  const VerifyArgs v = verify_args(ivf, E, P, b);
  launch_select(ivf, ctx, v);
  mfma_rescan(ivf, E, P, b, v);
  mark(ivf, E, EV_FINE_DONE);
  if (!E.live) {  // a masked batch is none of the watches' business: it counts into the second block
    rc = mfma_watch_counters(ivf, ctx, b.B);
    if (rc) return rc;
  }
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int run_fine(fvdb_ivf* ivf, const Env& E, const Batch& b, int role) {
  E.S->pend_filter = false;
  // beyond the shape: this index's own state (norms, lists rather than the one flat list), which thr_share_ok must not ask
  bool mfma = (ivf->scan_mode == FVDB_SCAN_AUTO || ivf->scan_mode == FVDB_SCAN_FILTER) && !ivf_knobs().scan_exact &&
              mfma_shape_ok(ivf, b.B, b.k, b.np) && role == ROLE_LIST && ivf->pool.norms() != nullptr;
  // a mask thins the lists the filter samples its threshold from: AUTO scans exactly under one and keeps its hit-rate
  // watch for the unmasked traffic (FVDB_SCAN_FILTER still forces the filter)
  if (mfma && E.live && ivf->scan_mode == FVDB_SCAN_AUTO) mfma = false;
  if (mfma && ivf->scan_mode == FVDB_SCAN_AUTO && auto_backs_off(ivf)) mfma = false;
  if (mfma) return run_fine_mfma(ivf, E, b);
  return run_fine_exact(ivf, E, b, role);
}

// stage_ms[i]: the time between two stage events
struct StageSpan {
  StageEvent from, to;
};
constexpr StageSpan kStageSpan[6] = {
    {EV_COARSE_BEGIN, EV_COARSE_SCANNED}, {EV_COARSE_SCANNED, EV_COARSE_DONE},  // coarse scan, coarse merge
    {EV_COARSE_DONE, EV_SCAN_BEGIN},                                            // plan
    {EV_SCAN_BEGIN, EV_SCAN_DONE},        {EV_SCAN_DONE, EV_FINE_DONE},         // fine scan, fine merge
    {EV_FILTER_BEGIN, EV_FILTER_DONE}};                                         // the filter kernel alone

int finish_profile(fvdb_ivf* ivf, const Env& E, bool coarse, bool fine) {
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  if (!ivf->ctx->profiling) return FVDB_OK;
  if (ivf->ctx->profiling == 2 && !S.collecting) {  // deferred: remember what to fold in later
    S.pend_coarse = coarse;
    S.pend_fine = fine;
    S.pending_profile = true;
    return FVDB_OK;
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  float ms = 0;
  auto add = [&](int stage) {
    (void)hipEventElapsedTime(&ms, S.sev[kStageSpan[stage].from], S.sev[kStageSpan[stage].to]);
    ivf->stage_ms[stage] += ms;
  };
  if (coarse) {
    add(0);
    add(1);
  }
  if (fine) {
    if (coarse) add(2);
    add(3);
    add(4);
    if (S.pend_filter) add(5);
  }
  ivf->stage_calls += 1;
  return FVDB_OK;
}

// largest sub-batch whose fine-stage partial buffer stays under ~1 GiB
uint32_t sub_batch(fvdb_ivf* ivf, uint32_t B, uint32_t k, uint32_t np) {
  uint64_t fit = queries_per_gib(ivf->max_list_blocks, pick_segb(ivf, B, np), k, np);
  fit = std::max<uint64_t>(fit, 1);
  fit = std::min<uint64_t>(fit, 16384);
  return (uint32_t)std::min<uint64_t>(fit, B);
}

// ---- the wide selection (kernels_wide.h): 1 <= k <= FVDB_MAX_K_WIDE ----
static_assert(kWideMaxK == FVDB_MAX_K_WIDE && kWideMaxProbes == FVDB_MAX_K, "kernels_wide.h sizes its LDS by these");
// Arena budget of one sub-batch: 1 GiB of distance words, the figure the partial lists of the register path are held to.
constexpr uint64_t kWideArenaBytes = 1ull << 30;
// Blocks a query's arena is sized for: its np probed lists are distinct, so they hold no more than np longest lists
// and no more than every list together.
uint32_t wide_arena_blocks(const fvdb_ivf* ivf, uint32_t np) {
  const uint64_t all = ivf->pool.used_blocks;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)np * ivf->max_list_blocks, all));
}
uint32_t wide_sub_batch(const fvdb_ivf* ivf, uint32_t B, uint32_t np) {
  const uint64_t per_q = (uint64_t)wide_arena_blocks(ivf, np) * 256;
  const uint64_t fit = std::min<uint64_t>(std::max<uint64_t>(kWideArenaBytes / per_q, 1), 16384);
  return (uint32_t)std::min<uint64_t>(fit, B);
}

// Fine stage of the wide path: every row of the probed lists scored into the arena, then one workgroup per query
// selects.  Same outputs as run_fine_exact.
int run_fine_wide(fvdb_ivf* ivf, const Env& E, const Batch& b) {
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  S.pend_filter = false;  // no filter kernel in this path: finish_profile has no interval of it to add
  const uint32_t nlist = ivf->nlist;
  const uint32_t segb = pick_segb(ivf, b.B, b.np);
  const uint32_t cap_blocks = wide_arena_blocks(ivf, b.np);
  const uint64_t stride = (uint64_t)cap_blocks * 64;
  int rc = plan_scratch(ivf, E, b.B, b.np);
  if (rc) return rc;
  HIPCHK(ctx, S.s_wbase.ensure((size_t)b.B * (b.np + 1) * 4));
  HIPCHK(ctx, S.s_arena.ensure((size_t)b.B * stride * 4));
  HIPCHK(ctx, S.s_scalars.ensure(kScalarsBytes));
  HIPCHK(ctx, hipMemsetAsync(S.s_cnt.p, 0, (size_t)nlist * 4, ctx->stream));
  launch_plan(ivf, E, b.probes, b.B * b.np, b.np, segb, /*Q=*/16, scan_stats(S), /*rezero_cnt=*/nullptr);
  const ListTable lists = list_table(ivf);
  hipLaunchKernelGGL(wide_base_kernel, dim3(cdiv(b.B, 256)), dim3(256), 0, ctx->stream, b.probes, lists.off, b.B, b.np,
                     cap_blocks, S.s_wbase.as<uint32_t>());
  mark(ivf, E, EV_SCAN_BEGIN);
  const PoolView pool = list_pool(ivf, E);
  const uint32_t grid = (uint32_t)ctx->num_cus * ivf_knobs().scan_wgs_per_cu;
  if (b.group) {
    auto score = ivf->f16 ? wide_score_kernel<1, WideGroups> : wide_score_kernel<0, WideGroups>;
    hipLaunchKernelGGL(score, dim3(grid), dim3(256), 0, ctx->stream, pool.data, pool.valid, pool.d4, lists.off, lists.blocks,
                       nlist, S.s_eoff.as<uint32_t>(), S.s_ioff.as<uint32_t>(), (const u32x2*)S.s_entries.as<uint2>(),
                       S.scalar(SC_FINE_ITEMS), S.scalar(SC_FINE_HEAD), b.qpad, ivf->dpad, segb, b.np,
                       S.s_wbase.as<uint32_t>(), S.s_arena.as<uint32_t>(), stride, WideGroups{b.words, b.group});
  } else {
    auto score = ivf->f16 ? wide_score_kernel<1> : wide_score_kernel<0>;
    hipLaunchKernelGGL(score, dim3(grid), dim3(256), 0, ctx->stream, pool.data, pool.valid, pool.d4, lists.off, lists.blocks,
                       nlist, S.s_eoff.as<uint32_t>(), S.s_ioff.as<uint32_t>(), (const u32x2*)S.s_entries.as<uint2>(),
                       S.scalar(SC_FINE_ITEMS), S.scalar(SC_FINE_HEAD), b.qpad, ivf->dpad, segb, b.np,
                       S.s_wbase.as<uint32_t>(), S.s_arena.as<uint32_t>(), stride);
  }
  mark(ivf, E, EV_SCAN_DONE);
  WideArgs w{};
  w.pool = pool;
  w.lists = lists;
  w.probes = b.probes;
  w.base = S.s_wbase.as<uint32_t>();
  w.arena = S.s_arena.as<uint32_t>();
  w.stride = stride;
  w.B = b.B;
  w.k = b.k;
  w.nprobe = b.np;
  w.out_ids = b.out_ids;
  w.out_dist = b.out_dist;
  w.out_counts = b.out_counts;
  w.out_keys = b.out_keys;
  if (b.radius) {
    const RangeListArgs ra{w, b.radius, b.out_totals};
    if (b.np <= kWideMaxProbes)
      hipLaunchKernelGGL(range_list_select_kernel<true>, dim3(b.B), dim3(kWideSelThreads), 0, ctx->stream, ra);
    else
      hipLaunchKernelGGL(range_list_select_kernel<false>, dim3(b.B), dim3(kWideSelThreads), 0, ctx->stream, ra);
  } else if (b.glob_keys) {
    HIPCHK(ctx, S.s_wgbase.ensure((size_t)b.B * b.np * 4));
    hipLaunchKernelGGL(wide_gbase_kernel, dim3(cdiv(b.B, 256)), dim3(256), 0, ctx->stream, b.probes, ivf->t_glob.as<uint32_t>(),
                       b.B, b.np, S.s_wgbase.as<uint32_t>());
    w.gbase = S.s_wgbase.as<uint32_t>();
    if (b.np <= kWideMaxProbes)
      hipLaunchKernelGGL((wide_select_kernel<true, true>), dim3(b.B), dim3(kWideSelThreads), 0, ctx->stream, w);
    else
      hipLaunchKernelGGL((wide_select_kernel<false, true>), dim3(b.B), dim3(kWideSelThreads), 0, ctx->stream, w);
  } else if (b.np <= kWideMaxProbes)
    hipLaunchKernelGGL(wide_select_kernel<true>, dim3(b.B), dim3(kWideSelThreads), 0, ctx->stream, w);
  else
    hipLaunchKernelGGL(wide_select_kernel<false>, dim3(b.B), dim3(kWideSelThreads), 0, ctx->stream, w);
  mark(ivf, E, EV_FINE_DONE);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// ---- sharded search: filter thresholds computed once per query across the ranks (comm_sharded.h) ----
// Whether a sharded step of B scanned queries uses the shared thresholds.  Every rank must answer alike (the answer
// decides whether a collective is issued), so only quantities that are the same on every rank enter: shapes, and the
// LOGICAL index's longest list.  Unlike run_fine it therefore does not ask whether this rank has rows (pool.norms).
bool thr_share_ok(fvdb_ivf* ivf, uint32_t B, uint32_t k, uint32_t np) {
  const IvfKnobs& kn = ivf_knobs();
  if (kn.scan_exact || kn.no_shared_thr || ivf->scan_mode != FVDB_SCAN_AUTO) return false;
  if (!mfma_shape_ok(ivf, B, k, np)) return false;
  uint32_t gmax = 0;
  if (ivf->glob_set) {
    for (uint32_t b : ivf->glob_blocks_host) gmax = std::max(gmax, b);
  } else {
    gmax = ivf->max_list_blocks;
  }
  // one sub-batch on every rank: sub_batch() with the logical index's longest list (local lists are no longer) and
  // with segb_for rather than pick_segb, that is, without a forced FVDB_SEGB
  return queries_per_gib(gmax, segb_for(gmax, B, np), k, np) >= B;
}

// U_q (kernels_mfma.h, ThresholdArgs::glob_blocks) for the B queries of a sharded step, +inf where this rank does
// not own the list the threshold comes from.  Leaves the slot's fp16 queries and |q|^2 in place for thr_combine.
int ivf_shared_thresholds(fvdb_ivf* ivf, const Env& E, const float* q_dev, const uint32_t* probes, uint32_t B, uint32_t k,
                          uint32_t np, float* u_out) {
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = upload_table(ivf);
  if (rc) return rc;
  std::lock_guard<std::mutex> enq(S.enq);
  HIPCHK(ctx, S.s_qn2.ensure((size_t)B * 4));
  if (!ivf->pool.norms() || !ivf->d_xmax.p) {  // no rows on this rank yet: it owns nothing
    HIPCHK(ctx, hipMemsetAsync(S.s_qn2.p, 0, (size_t)B * 4, ctx->stream));
    hipLaunchKernelGGL(fill_f32_kernel, dim3(cdiv(B, 256)), dim3(256), 0, ctx->stream, u_out, (uint64_t)B, __builtin_huge_valf());
    HIPCHK(ctx, hipGetLastError());
    return FVDB_OK;
  }
  const float* qpad = nullptr;
  rc = padded_queries(ivf, E, q_dev, B, &qpad);
  if (rc) return rc;
  HIPCHK(ctx, S.s_qh.ensure((size_t)(B + 1) * ivf->dpad * 2));
  HIPCHK(ctx, S.s_cnt.ensure((size_t)ivf->nlist * 4));
  HIPCHK(ctx, S.s_scnt.ensure((size_t)(B + 2) * 4));
  HIPCHK(ctx, S.s_mslots.ensure((size_t)B * 64 * 4));
  launch_prep_queries(ivf, E, qpad, B);
  ThresholdArgs t = threshold_args(ivf, E, qpad, probes, B, k, np, u_out);
  t.glob_blocks = ivf->t_glob.as<uint32_t>();
  launch_threshold_direct(ivf, ctx, t);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// thr = min over the ranks' U arrays + this rank's own error bound
int ivf_thr_combine(fvdb_ivf* ivf, const Env& E, const float* u_all, uint32_t W, uint32_t B, float* thr_out,
                    bool loopback_fill = false) {
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  if (!ivf->d_xmax.p) {
    HIPCHK(ctx, ivf->d_xmax.ensure(4));
    HIPCHK(ctx, hipMemsetAsync(ivf->d_xmax.p, 0, 4, ctx->stream));
  }
  hipLaunchKernelGGL(thr_combine_kernel, dim3(cdiv(B, 256)), dim3(256), 0, ctx->stream, u_all, W, B, S.s_qn2.as<float>(),
                     ivf->d_xmax.as<uint32_t>(), (float)ivf->dpad, x_rounded(ivf), thr_out);
#ifdef FVDB_DEV_TOOLS
  if (loopback_fill)
    hipLaunchKernelGGL(thr_loopback_fill_kernel, dim3(1), dim3(1024), 0, ctx->stream, thr_out, S.s_qn2.as<float>(), B);
#else
  (void)loopback_fill;
#endif
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int check_finite(fvdb_ctx* ctx, const float* x, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (!std::isfinite(x[i])) FAIL(ctx, FVDB_E_NONFINITE, "non-finite input value");
  return FVDB_OK;
}

}  // namespace

// GPU_MAX_HW_QUEUES bookkeeping (fvdb_ctx_create / fvdb_ctx_info): 0 unknown, 1 set by the host application, 2 set by this
// library before HIP came up, 3 could not be applied (the HIP runtime was already initialised in this process)
static std::mutex g_hwq_mu;
static int g_hwq_state = 0, g_hwq_value = 0;
static bool hip_runtime_already_up() {  // the ROCm runtime holds /dev/kfd open once it is initialised
  char path[64], tgt[256];
  for (int fd = 0; fd < 1024; ++fd) {
    snprintf(path, sizeof path, "/proc/self/fd/%d", fd);
    const ssize_t n = readlink(path, tgt, sizeof tgt - 1);
    if (n <= 0) continue;
    tgt[n] = 0;
    if (strstr(tgt, "/dev/kfd")) return true;
  }
  return false;
}

// =============================================================================================
// context
// =============================================================================================
extern "C" {

const char* fvdb_version(void) { return "fvdb-hip 0.1 (gfx950)"; }

int fvdb_ctx_create(int device, fvdb_ctx** out) {
  if (!out) return FVDB_E_INVALID;
  *out = nullptr;
  // Batches in flight run on streams of their own (two per batch); the HIP runtime multiplexes streams onto
  // GPU_MAX_HW_QUEUES hardware queues (default 4) and kernels of streams that share a queue run one after the other.
  // Ask for 16 unless the host application chose a value; this only takes effect if HIP has not been initialised
  // yet in this process (measured: 8 batches in flight, traversal only, 0.42 -> 0.27 ms per 1024-query step).
  // Whether that request can still take effect is recorded for fvdb_ctx_info (and said once on stderr when it cannot).
  {
    std::lock_guard<std::mutex> lk(g_hwq_mu);
    if (g_hwq_state == 0) {
      const char* set = getenv("GPU_MAX_HW_QUEUES");
      if (set) {
        g_hwq_value = atoi(set);
        g_hwq_state = 1;  // the host application's choice
      } else if (hip_runtime_already_up()) {
        g_hwq_value = 4;  // the runtime's default: several batches in flight share hardware queues
        g_hwq_state = 3;
        fprintf(stderr, "[fvdb] warning: HIP was initialised before fvdb_ctx_create, so GPU_MAX_HW_QUEUES=16 cannot be applied; "
                        "with the default of 4 hardware queues batches in flight overlap less (export GPU_MAX_HW_QUEUES=16 before "
                        "the process touches the GPU)\n");
      } else {
        (void)setenv("GPU_MAX_HW_QUEUES", "16", 0);
        g_hwq_value = 16;
        g_hwq_state = 2;
      }
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return FVDB_E_HIP;
  fvdb_ctx* ctx = new (std::nothrow) fvdb_ctx();
  if (!ctx) return FVDB_E_OOM;
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess || ctx->stream.create(hipStreamNonBlocking) != hipSuccess ||
      ctx->ev0.create() != hipSuccess || ctx->ev1.create() != hipSuccess) {
    delete ctx;
    return FVDB_E_HIP;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->num_cus = prop.multiProcessorCount;
  *out = ctx;
  return FVDB_OK;
}

int fvdb_ctx_device(fvdb_ctx* ctx) { return ctx ? ctx->device : -1; }

int fvdb_ctx_info(fvdb_ctx* ctx, fvdb_ctx_info_t* out) {
  if (!ctx || !out) return FVDB_E_INVALID;
  std::lock_guard<std::mutex> lk(g_hwq_mu);
  out->device = ctx->device;
  out->compute_units = ctx->num_cus;
  out->hw_queues = g_hwq_value;
  out->hw_queues_source = g_hwq_state;
  return FVDB_OK;
}

void fvdb_ctx_destroy(fvdb_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  delete ctx;
}

int fvdb_ctx_synchronize(fvdb_ctx* ctx) {
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}
int fvdb_device_synchronize(fvdb_ctx* ctx) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipDeviceSynchronize());
  return FVDB_OK;
}
void* fvdb_ctx_stream(fvdb_ctx* ctx) { return (void*)ctx->stream; }
const char* fvdb_last_error(fvdb_ctx* ctx) {
  if (!ctx) return "null context";
  static thread_local std::string copy;  // another thread's failure must not pull the text from under the reader
  std::lock_guard<std::mutex> lk(ctx->err_mu);
  copy = ctx->err;
  return copy.c_str();
}
int fvdb_ctx_set_profiling(fvdb_ctx* ctx, int on) {
  ctx->profiling = on;
  return FVDB_OK;
}

int fvdb_dev_alloc(fvdb_ctx* ctx, size_t bytes, void** out) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, DeviceMem::alloc(out, std::max<size_t>(bytes, 16), 0));  // the caller's block from here on
  return FVDB_OK;
}
int fvdb_dev_free(fvdb_ctx* ctx, void* p) {
  HIPCHK(ctx, DeviceMem::free(p));
  return FVDB_OK;
}
int fvdb_dev_upload(fvdb_ctx* ctx, void* dst, const void* src, size_t bytes) {
  HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}
int fvdb_dev_download(fvdb_ctx* ctx, void* dst, const void* src, size_t bytes) {
  HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}
// ---- pieces for keeping more than one batch in flight (pinned host memory, non-blocking copies, events) ----
int fvdb_host_alloc(fvdb_ctx* ctx, size_t bytes, void** out) {
  *out = nullptr;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, PinnedMem::alloc(out, std::max<size_t>(bytes, 16), hipHostMallocDefault));
  return FVDB_OK;
}
void fvdb_host_free(fvdb_ctx* ctx, void* p) {
  (void)ctx;
  if (p) (void)PinnedMem::free(p);
}
int fvdb_dev_download_async(fvdb_ctx* ctx, void* dst_pinned, const void* src, size_t bytes) {
  HIPCHK(ctx, hipMemcpyAsync(dst_pinned, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  return FVDB_OK;
}
int fvdb_dev_copy_async(fvdb_ctx* ctx, void* dst, const void* src, size_t bytes) {
  HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return FVDB_OK;
}
struct fvdb_event {
  DevEvent ev;
};
int fvdb_event_create(fvdb_ctx* ctx, fvdb_event** out) {
  *out = nullptr;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  fvdb_event* e = new (std::nothrow) fvdb_event();
  if (!e) return FVDB_E_OOM;
  if (e->ev.create(hipEventDisableTiming) != hipSuccess) {
    delete e;
    FAIL(ctx, FVDB_E_HIP, "event creation failed");
  }
  *out = e;
  return FVDB_OK;
}
void fvdb_event_destroy(fvdb_event* e) {
  delete e;
}
int fvdb_event_record(fvdb_ctx* ctx, fvdb_event* e) {
  HIPCHK(ctx, hipEventRecord(e->ev, ctx->stream));
  return FVDB_OK;
}
int fvdb_event_wait(fvdb_ctx* ctx, fvdb_event* e) {
  HIPCHK(ctx, hipEventSynchronize(e->ev));
  return FVDB_OK;
}

int fvdb_timer_start(fvdb_ctx* ctx) {
  HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  return FVDB_OK;
}
int fvdb_timer_stop_ms(fvdb_ctx* ctx, float* out_ms) {
  HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
  HIPCHK(ctx, hipEventElapsedTime(out_ms, ctx->ev0, ctx->ev1));
  return FVDB_OK;
}

// =============================================================================================
// similarity utilities (a3)
// =============================================================================================
static int dot_cosine(fvdb_ctx* ctx, const float* q, uint32_t B, const float* x, uint64_t n, uint32_t d, float* out,
                      int cosine) {
  if (!ctx || !q || !x || !out || d == 0) return FVDB_E_INVALID;
  if (B == 0 || n == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = check_finite(ctx, q, (uint64_t)B * d);
  if (rc) return rc;
  rc = check_finite(ctx, x, n * d);
  if (rc) return rc;
  DBuf dq, dx, dout;
  if (dq.exact((size_t)B * d * 4) != hipSuccess || dx.exact(n * d * 4) != hipSuccess ||
      dout.exact((size_t)B * n * 4) != hipSuccess)
    FAIL(ctx, FVDB_E_OOM, "similarity scratch allocation failed");
  (void)hipMemcpyAsync(dq.p, q, (size_t)B * d * 4, hipMemcpyHostToDevice, ctx->stream);
  (void)hipMemcpyAsync(dx.p, x, n * d * 4, hipMemcpyHostToDevice, ctx->stream);
  hipLaunchKernelGGL(dot_cosine_kernel, dim3(cdiv((uint64_t)B * n, 256)), dim3(256), 0, ctx->stream, dq.as<float>(),
                     dx.as<float>(), B, n, d, cosine, dout.as<float>());
  hipError_t e = hipMemcpyAsync(out, dout.p, (size_t)B * n * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) FAIL(ctx, FVDB_E_HIP, hipGetErrorString(e));
  return FVDB_OK;
}
int fvdb_dot_products(fvdb_ctx* ctx, const float* q, uint32_t B, const float* x, uint64_t n, uint32_t d, float* out) {
  return dot_cosine(ctx, q, B, x, n, d, out, 0);
}
int fvdb_cosine_similarities(fvdb_ctx* ctx, const float* q, uint32_t B, const float* x, uint64_t n, uint32_t d,
                             float* out) {
  return dot_cosine(ctx, q, B, x, n, d, out, 1);
}

// =============================================================================================
// IVF
// =============================================================================================
int fvdb_ivf_create(fvdb_ctx* ctx, uint32_t d, uint32_t nlist, fvdb_ivf** out) {
  return fvdb_ivf_create_ex(ctx, d, nlist, FVDB_F32, out);
}

int fvdb_ivf_create_ex(fvdb_ctx* ctx, uint32_t d, uint32_t nlist, int row_dtype, fvdb_ivf** out) {
  if (!ctx || !out) return FVDB_E_INVALID;
  *out = nullptr;
  if (row_dtype != FVDB_F32 && row_dtype != FVDB_F16) FAIL(ctx, FVDB_E_INVALID, "row_dtype must be FVDB_F32 or FVDB_F16");
  if (d == 0 || nlist == 0) FAIL(ctx, FVDB_E_INVALID, "d and nlist must be > 0");
  if (d > 2048 * 4) FAIL(ctx, FVDB_E_INVALID, "d too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  fvdb_ivf* ivf = new (std::nothrow) fvdb_ivf();
  if (!ivf) return FVDB_E_OOM;
  ivf->ctx = ctx;
  ivf->d = d;
  ivf->f16 = row_dtype == FVDB_F16;
  ivf->dpad = ivf->f16 ? ((d + 15) / 16) * 16 : ((d + 3) / 4) * 4;  // fp16 rows: whole 16-dim steps
  ivf->d4 = ivf->dpad / 4;
  ivf->nlist = nlist;
  ivf->list_blocks.assign(nlist, {});
  ivf->list_len.assign(nlist, 0);
  ivf->pool.d4 = ivf->d4;
  ivf->pool.esize = ivf->f16 ? 2 : 4;
  static const bool no_mirror = getenv("FVDB_NO_FP16_MIRROR") != nullptr;  // tuning aid: filter from the f32 rows
  ivf->pool.mirror = !ivf->f16 && ivf->dpad % 16 == 0 && !no_mirror;
  ivf->cpool.d4 = ivf->d4;
  for (auto& e : ivf->sev) (void)e.create();
  *out = ivf;
  return FVDB_OK;
}

void fvdb_ivf_destroy(fvdb_ivf* ivf) {
  if (!ivf) return;
  (void)hipSetDevice(ivf->ctx->device);
  (void)hipStreamSynchronize(ivf->ctx->stream);
  for (auto& c : ivf->lease_ctx)
    if (c) fvdb_ctx_destroy(c);
  delete ivf;
}

static int install_centroids(fvdb_ivf* ivf, const float* d_rowmajor /* device [nlist][d] */) {
  ivf->mutations += 1;
  fvdb_ctx* ctx = ivf->ctx;
  const uint32_t nlist = ivf->nlist, cblocks = cdiv(nlist, 64);
  int rc = ivf->cpool.reserve(ctx, cblocks);
  if (rc) return rc;
  HIPCHK(ctx, hipMemsetAsync(ivf->cpool.valid(), 0, (size_t)ivf->cpool.cap_blocks * 8, ctx->stream));
  ivf->cpool.used_blocks = cblocks;
  std::vector<uint32_t> slots(nlist), off{0, cblocks}, blocks(cblocks), glob{cblocks};
  for (uint32_t i = 0; i < nlist; ++i) slots[i] = i;
  for (uint32_t i = 0; i < cblocks; ++i) blocks[i] = i;
  HIPCHK(ctx, ivf->s_slots.ensure((size_t)nlist * 4));
  HIPCHK(ctx, ivf->c_off.ensure(8));
  HIPCHK(ctx, ivf->c_blocks.ensure((size_t)cblocks * 4));
  HIPCHK(ctx, ivf->c_glob.ensure(4));
  HIPCHK(ctx, hipMemcpyAsync(ivf->s_slots.p, slots.data(), (size_t)nlist * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ivf->c_off.p, off.data(), 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ivf->c_blocks.p, blocks.data(), (size_t)cblocks * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ivf->c_glob.p, glob.data(), 4, hipMemcpyHostToDevice, ctx->stream));
  const uint64_t threads = (uint64_t)nlist * ivf->d4;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(cdiv(threads, 256)), dim3(256), 0, ctx->stream, d_rowmajor, ivf->d,
                     ivf->d4, (uint64_t)nlist, ivf->s_slots.as<uint32_t>(), (const uint64_t*)nullptr,
                     (float4*)ivf->cpool.data(), ivf->cpool.ids(), (unsigned long long*)ivf->cpool.valid(), (void*)nullptr,
                     (float4*)nullptr);
  // matrix-core coarse stage: padded row-major table, |c|^2, max |c|^2
  const float* cpad = d_rowmajor;
  if (ivf->d != ivf->dpad) {
    HIPCHK(ctx, ivf->d_cent_pad.ensure((size_t)nlist * ivf->dpad * 4));
    const uint64_t tot = (uint64_t)nlist * ivf->dpad;
    hipLaunchKernelGGL(pad_rows_kernel, dim3(cdiv(tot, 256)), dim3(256), 0, ctx->stream, d_rowmajor, ivf->d, ivf->dpad,
                       (uint64_t)nlist, ivf->d_cent_pad.as<float>());
    cpad = ivf->d_cent_pad.as<float>();
  }
  HIPCHK(ctx, ivf->d_cnorm.ensure((size_t)nlist * 4));
  HIPCHK(ctx, ivf->d_cnmax.ensure(4));
  HIPCHK(ctx, ivf->s_fallbacks.ensure(kFbAllBytes));
  hipLaunchKernelGGL(row_sqnorm_kernel, dim3(cdiv(nlist, 256)), dim3(256), 0, ctx->stream, cpad, ivf->dpad, ivf->dpad,
                     nlist, ivf->d_cnorm.as<float>());
  hipLaunchKernelGGL(max_f32_kernel, dim3(1), dim3(64), 0, ctx->stream, ivf->d_cnorm.as<float>(), nlist,
                     ivf->d_cnmax.as<float>());
  HIPCHK(ctx, hipMemsetAsync(ivf->s_fallbacks.p, 0, kFbAllBytes, ctx->stream));
  if (ivf->h_fb.p) *(volatile uint32_t*)ivf->h_fb.p = 0;
  ivf->mfma_q = ivf->fb_seen = ivf->q_seen = 0;
  ivf->exact_batches_left = ivf->backoff_len = 0;
  ivf->overflow_seen = ivf->overflow_q = 0;
  ivf->refine_batches_left = 0;
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ivf->trained = true;
  return FVDB_OK;
}

static void reset_lists(fvdb_ivf* ivf) {
  ivf->list_blocks.assign(ivf->nlist, {});
  ivf->list_len.assign(ivf->nlist, 0);
  ivf->total_rows = 0;
  ivf->pool.used_blocks = 0;
  ivf->max_list_blocks = 0;
  ivf->table_dirty = true;
}

int fvdb_ivf_set_centroids(fvdb_ivf* ivf, const float* centroids) {
  fvdb_ctx* ctx = ivf->ctx;
  if (!centroids) FAIL(ctx, FVDB_E_INVALID, "null centroids");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)ivf->nlist * ivf->d;
  int rc = check_finite(ctx, centroids, n);
  if (rc) return rc;
  ivf->h_centroids.assign(centroids, centroids + n);
  HIPCHK(ctx, ivf->d_centroids_rm.ensure(n * 4));
  HIPCHK(ctx, hipMemcpyAsync(ivf->d_centroids_rm.p, centroids, n * 4, hipMemcpyHostToDevice, ctx->stream));
  rc = install_centroids(ivf, ivf->d_centroids_rm.as<float>());
  if (rc) return rc;
  reset_lists(ivf);
  if (ivf->pool.valid() && ivf->pool.cap_blocks)
    HIPCHK(ctx, hipMemsetAsync(ivf->pool.valid(), 0, (size_t)ivf->pool.cap_blocks * 8, ctx->stream));
  return FVDB_OK;
}

int fvdb_ivf_get_centroids(fvdb_ivf* ivf, float* out) {
  if (!ivf->trained) FAIL(ivf->ctx, FVDB_E_NOT_TRAINED, "index not trained");
  std::memcpy(out, ivf->h_centroids.data(), ivf->h_centroids.size() * 4);
  return FVDB_OK;
}

int fvdb_ivf_clear(fvdb_ivf* ivf) {
  ivf->mutations += 1;
  fvdb_ctx* ctx = ivf->ctx;
  reset_lists(ivf);
  if (ivf->pool.valid() && ivf->pool.cap_blocks)
    HIPCHK(ctx, hipMemsetAsync(ivf->pool.valid(), 0, (size_t)ivf->pool.cap_blocks * 8, ctx->stream));
  return FVDB_OK;
}

int fvdb_ivf_reserve(fvdb_ivf* ivf, uint64_t n_rows) {
  ivf->mutations += 1;
  HIPCHK(ivf->ctx, hipSetDevice(ivf->ctx->device));
  // every list may end in a partly filled block
  return ivf->pool.reserve(ivf->ctx, cdiv(n_rows, 64) + ivf->nlist);
}

int fvdb_ivf_list_sizes(fvdb_ivf* ivf, uint64_t* out) {
  for (uint32_t L = 0; L < ivf->nlist; ++L) out[L] = ivf->list_len[L];
  return FVDB_OK;
}
uint64_t fvdb_ivf_total_rows(fvdb_ivf* ivf) { return ivf->total_rows; }

// Copy one inverted list back to the host in list-position order (the save path of the chunked on-disk format,
// src/hybrid/persistence.rs:289-311 walks every inverted list).  fp16 rows are widened exactly.
int fvdb_ivf_list_export(fvdb_ivf* ivf, uint32_t list, float* rows, uint64_t* ids, uint8_t* live) {
  fvdb_ctx* ctx = ivf->ctx;
  if (list >= ivf->nlist) FAIL(ctx, FVDB_E_INVALID, "no such list");
  const uint32_t len = ivf->list_len[list];
  if (len == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const Pool& P = ivf->pool;
  const size_t bb = P.block_bytes();
  std::vector<uint8_t> blk(bb);
  uint64_t bid[64], valid = 0;
  const uint32_t d = ivf->d;
  for (uint32_t b = 0; b * 64 < len; ++b) {
    const uint32_t pb = ivf->list_blocks[list][b];
    HIPCHK(ctx, hipMemcpyAsync(blk.data(), (const char*)P.data() + (size_t)pb * bb, bb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(bid, P.ids() + (size_t)pb * 64, sizeof bid, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(&valid, P.valid() + pb, sizeof valid, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t rows_here = std::min<uint32_t>(64, len - b * 64);
    for (uint32_t lane = 0; lane < rows_here; ++lane) {
      const size_t r = (size_t)b * 64 + lane;
      if (rows) {
        float* out = rows + r * d;
        if (P.esize == 4) {  // [d4][64] chunks of 4 floats, lane = row
          const float* src = (const float*)blk.data();
          for (uint32_t j = 0; j < d; ++j) out[j] = src[((size_t)(j >> 2) * 64 + lane) * 4 + (j & 3)];
        } else {  // [d8][64] chunks of 8 halves
          const _Float16* src = (const _Float16*)blk.data();
          for (uint32_t j = 0; j < d; ++j) out[j] = (float)src[((size_t)(j >> 3) * 64 + lane) * 8 + (j & 7)];
        }
      }
      if (ids) ids[r] = bid[lane];
      if (live) live[r] = (uint8_t)((valid >> lane) & 1);
    }
  }
  return FVDB_OK;
}

int fvdb_ivf_set_global_list_sizes(fvdb_ivf* ivf, const uint64_t* sizes) {
  ivf->glob_blocks_host.resize(ivf->nlist);
  for (uint32_t L = 0; L < ivf->nlist; ++L) ivf->glob_blocks_host[L] = cdiv(sizes[L], 64);
  ivf->glob_set = true;
  ivf->table_dirty = true;
  return FVDB_OK;
}

// device-side assign: clusters for n rows already in HBM (row-major [n][d])
static int assign_dev(fvdb_ivf* ivf, const float* x_dev, uint64_t n, uint32_t* out_dev) {
  fvdb_ctx* ctx = ivf->ctx;
  const uint32_t step = 65536;
  for (uint64_t o = 0; o < n; o += step) {
    const uint32_t B = (uint32_t)std::min<uint64_t>(step, n - o);
    const float* qpad = nullptr;
    const Env E{ivf->ctx, ivf};
    int rc = padded_queries(ivf, E, x_dev + o * ivf->d, B, &qpad);
    if (rc) return rc;
    rc = run_coarse(ivf, E, qpad, B, 1, out_dev + o, nullptr);
    if (rc) return rc;
  }
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int fvdb_ivf_assign(fvdb_ivf* ivf, const float* x, uint64_t n, uint32_t* out_cluster) {
  fvdb_ctx* ctx = ivf->ctx;
  if (!ivf->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "index not trained");
  if (n == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = check_finite(ctx, x, n * ivf->d);
  if (rc) return rc;
  HIPCHK(ctx, ivf->s_in.ensure(n * ivf->d * 4));
  HIPCHK(ctx, ivf->s_clusters.ensure(n * 4));
  HIPCHK(ctx, hipMemcpyAsync(ivf->s_in.p, x, n * ivf->d * 4, hipMemcpyHostToDevice, ctx->stream));
  rc = assign_dev(ivf, ivf->s_in.as<float>(), n, ivf->s_clusters.as<uint32_t>());
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out_cluster, ivf->s_clusters.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}

// rows already staged in s_in (device, row-major); clusters on host
static int append_staged(fvdb_ivf* ivf, const uint64_t* ids, uint64_t n, const uint32_t* cluster, uint32_t* out_pos) {
  ivf->mutations += 1;
  fvdb_ctx* ctx = ivf->ctx;
  // count new blocks first so the pool grows once
  std::vector<uint32_t> add_len(ivf->nlist, 0);
  for (uint64_t i = 0; i < n; ++i) {
    if (cluster[i] >= ivf->nlist) FAIL(ctx, FVDB_E_INVALID, "cluster id out of range");
    add_len[cluster[i]]++;
  }
  uint64_t new_blocks = 0;
  for (uint32_t L = 0; L < ivf->nlist; ++L)
    new_blocks += cdiv((uint64_t)ivf->list_len[L] + add_len[L], 64) - ivf->list_blocks[L].size();
  if ((uint64_t)ivf->pool.used_blocks + new_blocks >= (1ull << 26)) FAIL(ctx, FVDB_E_UNSUPPORTED, "pool too large");
  int rc = ivf->pool.reserve(ctx, ivf->pool.used_blocks + (uint32_t)new_blocks);
  if (rc) return rc;
  std::vector<uint32_t> slots(n);
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t L = cluster[i];
    const uint32_t pos = ivf->list_len[L]++;
    if ((pos & 63) == 0) ivf->list_blocks[L].push_back(ivf->pool.used_blocks++);
    slots[i] = ivf->list_blocks[L][pos >> 6] * 64 + (pos & 63);
    if (out_pos) out_pos[i] = pos;
  }
  ivf->total_rows += n;
  ivf->table_dirty = true;
  HIPCHK(ctx, ivf->s_slots.ensure(n * 4));
  HIPCHK(ctx, ivf->s_ids.ensure(n * 8));
  HIPCHK(ctx, hipMemcpyAsync(ivf->s_slots.p, slots.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
  if (ids) HIPCHK(ctx, hipMemcpyAsync(ivf->s_ids.p, ids, n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (ivf->f16) {
    const uint32_t d8 = ivf->dpad / 8;
    hipLaunchKernelGGL(scatter_rows_f16_kernel, dim3(cdiv(n * d8, 256)), dim3(256), 0, ctx->stream,
                       ivf->s_in.as<float>(), ivf->d, d8, n, ivf->s_slots.as<uint32_t>(),
                       ids ? ivf->s_ids.as<uint64_t>() : nullptr, ivf->pool.data(), ivf->pool.ids(),
                       (unsigned long long*)ivf->pool.valid());
  } else {
    const uint64_t threads = n * ivf->d4;
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(cdiv(threads, 256)), dim3(256), 0, ctx->stream, ivf->s_in.as<float>(),
                       ivf->d, ivf->d4, n, ivf->s_slots.as<uint32_t>(), ids ? ivf->s_ids.as<uint64_t>() : nullptr,
                       (float4*)ivf->pool.data(), ivf->pool.ids(), (unsigned long long*)ivf->pool.valid(), ivf->pool.half(),
                       (float4*)ivf->pool.rm());
  }
  if (!ivf->d_xmax.p) {
    HIPCHK(ctx, ivf->d_xmax.ensure(4));
    HIPCHK(ctx, hipMemsetAsync(ivf->d_xmax.p, 0, 4, ctx->stream));
  }
  hipLaunchKernelGGL(pool_row_norms_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, ivf->s_in.as<float>(), ivf->d, n,
                     ivf->f16 ? 1 : 0, ivf->s_slots.as<uint32_t>(), ivf->pool.norms(), ivf->d_xmax.as<uint32_t>());
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}

int fvdb_ivf_add_assigned(fvdb_ivf* ivf, const float* x, const uint64_t* ids, uint64_t n, const uint32_t* cluster,
                          uint32_t* out_pos) {
  fvdb_ctx* ctx = ivf->ctx;
  if (!ivf->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "index not trained");
  if (n == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = check_finite(ctx, x, n * ivf->d);
  if (rc) return rc;
  HIPCHK(ctx, ivf->s_in.ensure(n * ivf->d * 4));
  HIPCHK(ctx, hipMemcpyAsync(ivf->s_in.p, x, n * ivf->d * 4, hipMemcpyHostToDevice, ctx->stream));
  return append_staged(ivf, ids, n, cluster, out_pos);
}

int fvdb_ivf_add(fvdb_ivf* ivf, const float* x, const uint64_t* ids, uint64_t n, uint32_t* out_cluster,
                 uint32_t* out_pos) {
  fvdb_ctx* ctx = ivf->ctx;
  if (!ivf->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "index not trained");
  if (n == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = check_finite(ctx, x, n * ivf->d);
  if (rc) return rc;
  HIPCHK(ctx, ivf->s_in.ensure(n * ivf->d * 4));
  HIPCHK(ctx, ivf->s_clusters.ensure(n * 4));
  HIPCHK(ctx, hipMemcpyAsync(ivf->s_in.p, x, n * ivf->d * 4, hipMemcpyHostToDevice, ctx->stream));
  rc = assign_dev(ivf, ivf->s_in.as<float>(), n, ivf->s_clusters.as<uint32_t>());
  if (rc) return rc;
  std::vector<uint32_t> cl(n);
  HIPCHK(ctx, hipMemcpyAsync(cl.data(), ivf->s_clusters.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (out_cluster) std::memcpy(out_cluster, cl.data(), n * 4);
  return append_staged(ivf, ids, n, cl.data(), out_pos);
}

int fvdb_ivf_set_deleted(fvdb_ivf* ivf, const uint32_t* cluster, const uint32_t* pos, uint64_t n, int deleted) {
  fvdb_ctx* ctx = ivf->ctx;
  if (n == 0) return FVDB_OK;
  ivf->mutations += 1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> slots(n);
  for (uint64_t i = 0; i < n; ++i) {
    if (cluster[i] >= ivf->nlist || pos[i] >= ivf->list_len[cluster[i]]) FAIL(ctx, FVDB_E_NOT_FOUND, "no such row");
    slots[i] = ivf->list_blocks[cluster[i]][pos[i] >> 6] * 64 + (pos[i] & 63);
  }
  HIPCHK(ctx, ivf->s_slots.ensure(n * 4));
  HIPCHK(ctx, hipMemcpyAsync(ivf->s_slots.p, slots.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(set_valid_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, ivf->s_slots.as<uint32_t>(), n,
                     deleted, (unsigned long long*)ivf->pool.valid());
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}

// ---------------------------------------------------------------------------------------------
// IVF search: one request, one sub-batch driver, one way onto a scratch set
// ---------------------------------------------------------------------------------------------
extern "C++" {
namespace {
// What an entry point asks for, stated once.  Everything per query — the queries, the optional inputs, every output —
// lives here, so that slice() can cut all of it alike.
struct IvfSearch {
  enum Kind {
    PROBED,       // the nprobe nearest lists: k <= FVDB_MAX_K up to 256 lists probed; above that it is served as WIDE
                  // (k <= FVDB_MAX_K_WIDE)
    ALL,          // every list (ROLE_ALL), no coarse stage
    WIDE,         // the nprobe nearest lists, k <= FVDB_MAX_K_WIDE (run_fine_wide)
    SHARD_WIDE,   // WIDE on an index that may hold a shard of a larger one: keys by the logical index's seq
    RADIUS,       // WIDE's lists and score stage; per query the rows within radius[b], at most k of them, and their number
    COARSE_ONLY,  // the coarse stage alone: probes_out is the result
  } kind;
  const float* q_dev;  // [B][d]
  uint32_t B, k, nprobe;
  // results [B][k], counts [B]; any of them may be null
  uint64_t* ids = nullptr;
  float* dist = nullptr;
  uint32_t* counts = nullptr;
  uint64_t* keys = nullptr;
  const uint32_t* given_probes = nullptr;  // [B][np] cluster ids in probe order: the coarse stage is skipped
  const float* given_thr = nullptr;        // [B] filter thresholds agreed between the ranks (Batch::given_thr)
  uint32_t* probes_out = nullptr;          // [B][np] the ranking goes here: COARSE_ONLY's result; any other kind scans
                                           // the lists from here instead of the set's own block, and the caller keeps it
  // WIDE with one allow-set per query (fvdb_ivf_search_groups_dev_slot): the live words of each group, G masks and then
  // the pool's own, and each query's index into them.  Device pointers; the driver fills them in from GroupSource.
  const uint64_t* const* words = nullptr;  // [G + 1]
  const uint32_t* group = nullptr;         // [B]
  // RADIUS: the radius of each query and where the size of its ball goes
  const float* radius = nullptr;           // [B]
  uint32_t* totals = nullptr;              // [B]

  // Queries o .. o + b of the request; np = min(nprobe, nlist) as the driver clamped it.  The only place a stride is written.
  IvfSearch slice(uint32_t o, uint32_t b, uint32_t d, uint32_t np) const {
    auto at = [o](auto* p, size_t stride) { return p ? p + (size_t)o * stride : nullptr; };
    IvfSearch s = *this;
    s.B = b;
    s.q_dev = at(q_dev, d);
    s.ids = at(ids, k);
    s.dist = at(dist, k);
    s.counts = at(counts, 1);
    s.keys = at(keys, k);
    s.given_probes = at(given_probes, np);
    s.given_thr = at(given_thr, 1);
    s.probes_out = at(probes_out, np);
    s.group = at(group, 1);
    s.radius = at(radius, 1);
    s.totals = at(totals, 1);
    return s;
  }
};

// Whether a request takes the wide selection (run_fine_wide): asked for, or more lists probed (np = min(nprobe, nlist))
// than the register path ranks and merges.
inline bool wide_route(IvfSearch::Kind kind, uint32_t np) {
  return kind == IvfSearch::WIDE || kind == IvfSearch::SHARD_WIDE || kind == IvfSearch::RADIUS ||
         (kind == IvfSearch::PROBED && np > FVDB_MAX_K);
}
// The keys of a shard's wide search hold the logical index's seq in 32 bits, as the register path's do: 64 x the blocks
// of np probed lists of the logical index must stay below 2^32.  Bounded by np longest lists and by all lists together.
int check_shard_seq(fvdb_ctx* ctx, const fvdb_ivf* ivf, uint32_t np) {
  uint64_t gmax = 0, gsum = 0;
  for (uint32_t L = 0; L < ivf->nlist; ++L) {
    const uint64_t nb = ivf->glob_set ? ivf->glob_blocks_host[L] : ivf->list_blocks[L].size();
    gmax = std::max(gmax, nb);
    gsum += nb;
  }
  if (std::min((uint64_t)np * gmax, gsum) * 64 >= (1ull << 32))
    FAIL(ctx, FVDB_E_UNSUPPORTED, "the probed lists of the logical index hold more than 2^32 scan positions");
  return FVDB_OK;
}
inline uint32_t probed_lists(const fvdb_ivf* ivf, IvfSearch::Kind kind, uint32_t nprobe) {
  return kind == IvfSearch::ALL ? ivf->nlist : std::min(nprobe, ivf->nlist);
}

// The k a search serves.  The driver asks for every entry point; search_host asks first, before it stages anything.
int check_k(fvdb_ctx* ctx, IvfSearch::Kind kind, uint32_t k, uint32_t np) {
  if (wide_route(kind, np)) {
    if (k == 0 || k > FVDB_MAX_K_WIDE) FAIL(ctx, FVDB_E_UNSUPPORTED, "k must be in 1..FVDB_MAX_K_WIDE");
  } else if (k == 0 || k > FVDB_MAX_K) {
    FAIL(ctx, FVDB_E_UNSUPPORTED, "k must be in 1..FVDB_MAX_K");
  }
  return FVDB_OK;
}

// the stage events of a scratch set exist from the first profiled search on it
void ensure_stage_events(const fvdb_ivf* ivf, IvfScratch& S) {
  if (!ivf->ctx->profiling) return;
  for (auto& e : S.sev) (void)e.create();
}

// A grouped search's host side: the table of live-word pointers (device addresses, [n_words]) and the group of each
// query ([B], every entry checked against the table by the entry point).  The driver copies both into the scratch set.
struct GroupSource {
  const uint64_t* const* words;
  uint32_t n_words;
  const uint32_t* group;
};

// Every IVF search: validated, cut into sub-batches that fit the scratch budget, each through its coarse and fine stage.
int ivf_search(fvdb_ivf* ivf, const Env& E, const IvfSearch& R_in, const GroupSource* groups = nullptr) {
  IvfSearch R = R_in;
  fvdb_ctx* ctx = E.ctx;
  IvfScratch& S = *E.S;
  const uint32_t np = probed_lists(ivf, R.kind, R.nprobe);
  const bool all = R.kind == IvfSearch::ALL, wide = wide_route(R.kind, np);
  if (!ivf->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "index not trained");
  int rc = check_k(ctx, R.kind, R.k, np);
  if (rc) return rc;
  if (wide && ivf->glob_set && R.kind != IvfSearch::SHARD_WIDE)
    FAIL(ctx, FVDB_E_UNSUPPORTED, "the wide search (k or nprobe above FVDB_MAX_K) does not serve a shard of a larger index");
  if (R.B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (np == 0) FAIL(ctx, FVDB_E_INVALID, "nprobe must be > 0");
  if (!all && (rc = check_rank(ctx, ivf, np))) return rc;
  if (R.kind == IvfSearch::SHARD_WIDE && (rc = check_shard_seq(ctx, ivf, np))) return rc;
  rc = upload_table(ivf);
  if (rc) return rc;
  std::lock_guard<std::mutex> enq(S.enq);  // one search's launches go in as a block
  ensure_stage_events(ivf, S);
  if (groups) {
    // in the set's own buffers, behind whatever the stream still runs from them; the caller's arrays are its own again
    // when this returns
    HIPCHK(ctx, S.s_gwords.ensure((size_t)groups->n_words * 8));
    HIPCHK(ctx, S.s_group.ensure((size_t)R.B * 4));
    HIPCHK(ctx, hipMemcpyAsync(S.s_gwords.p, groups->words, (size_t)groups->n_words * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(S.s_group.p, groups->group, (size_t)R.B * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    R.words = S.s_gwords.as<const uint64_t*>();
    R.group = S.s_group.as<uint32_t>();
  }
  const uint32_t step = wide ? wide_sub_batch(ivf, R.B, np) : sub_batch(ivf, R.B, R.k, np);
  for (uint32_t o = 0; o < R.B; o += step) {
    const IvfSearch r = R.slice(o, std::min(step, R.B - o), ivf->d, np);
    const float* qpad = nullptr;
    rc = padded_queries(ivf, E, r.q_dev, r.B, &qpad);
    if (rc) return rc;
    HIPCHK(ctx, S.s_probes.ensure((size_t)r.B * np * 4));
    const uint32_t* probes = S.s_probes.as<uint32_t>();
    if (all) {
      hipLaunchKernelGGL(probes_all_kernel, dim3(cdiv((uint64_t)r.B * np, 256)), dim3(256), 0, ctx->stream, r.B, np,
                         S.s_probes.as<uint32_t>());
      mark(ivf, E, EV_COARSE_DONE);
    } else if (r.given_probes) {
      probes = r.given_probes;
      // no coarse stage in this call: zero-length stage intervals
      mark(ivf, E, EV_COARSE_BEGIN);
      mark(ivf, E, EV_COARSE_SCANNED);
      mark(ivf, E, EV_COARSE_DONE);
    } else {
      uint32_t* ranked = r.probes_out ? r.probes_out : S.s_probes.as<uint32_t>();
      rc = run_coarse(ivf, E, qpad, r.B, np, ranked, nullptr);
      if (rc) return rc;
      probes = ranked;
    }
    if (R.kind == IvfSearch::COARSE_ONLY) continue;
    const Batch b{qpad, probes, r.B, r.k, np, r.ids, r.dist, r.counts, r.keys, r.given_thr, R.kind == IvfSearch::SHARD_WIDE,
                  r.words, r.group, r.radius, r.totals};
    rc = wide ? run_fine_wide(ivf, E, b) : run_fine(ivf, E, b, all ? ROLE_ALL : ROLE_LIST);
    if (rc) return rc;
    // per sub-batch: each one records the stage events anew, so their intervals are folded in before the next does
    rc = finish_profile(ivf, E, !all, true);
    if (rc) return rc;
  }
  ivf->last_set.store(E.S);
  ivf->last_ctx.store(E.ctx);
  return FVDB_OK;
}

// The explicit-slot entry points: the caller names the scratch set (slot) and the stream (`on`); nothing in the index
// object changes, so calls on different slots may come from different host threads at the same time.
int slot_env(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, Env* E) {
  if (slot >= fvdb_ivf::kSlots) FAIL(ivf->ctx, FVDB_E_INVALID, "slot out of range");
  if (on && on->device != ivf->ctx->device) FAIL(ivf->ctx, FVDB_E_INVALID, "context of another device");
  E->ctx = on ? on : ivf->ctx;
  E->S = &slot_scratch(ivf, slot);
  return FVDB_OK;
}
// The same under an allow-set mask (fvdb_mask_create_ivf): the mask's words take the place of the pool's live words in
// every stage that reads them.  A mask built before the index last changed is refused.
int mask_env(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, Env* E) {
  if (!ivf) return FVDB_E_INVALID;
  int rc = slot_env(ivf, on, slot, E);
  if (rc) return rc;
  if (!mask || mask->ivf != ivf) FAIL(ivf->ctx, FVDB_E_INVALID, "mask of another index");
  if (mask->stamp != ivf->mutations) FAIL(ivf->ctx, FVDB_E_INVALID, "stale mask: the index changed after the mask was created");
  E->live = mask->words.as<uint64_t>();
  return FVDB_OK;
}
int slot_done(fvdb_ivf* ivf, const Env& E, int rc) {
  if (rc && E.ctx != ivf->ctx) {  // the failure text is read from the index's own context
    std::string m;
    {
      std::lock_guard<std::mutex> lk(E.ctx->err_mu);
      m = E.ctx->err;
    }
    ivf->ctx->set_err(m);
  }
  return rc;
}

// How a call names its mask: none, or one that must be this index's and fresh (a null pointer is then refused).
struct SlotMask {
  bool required = false;
  fvdb_mask* mask = nullptr;
};
constexpr SlotMask kNoMask{};
inline SlotMask masked_by(fvdb_mask* mask) { return SlotMask{true, mask}; }

// body(E) on slot `slot` and `on`'s stream: every launch goes to that stream and touches only that slot's scratch, so
// slots can be in flight together.
template <class Body>
int on_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, SlotMask m, Body body) {
  Env E{};
  int rc = m.required ? mask_env(ivf, on, slot, m.mask, &E) : slot_env(ivf, on, slot, &E);
  if (rc) return rc;
  const int done = body(E);
  return slot_done(ivf, E, done);
}
inline int search_on_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, SlotMask m, const IvfSearch& R) {
  return on_slot(ivf, on, slot, m, [&](const Env& E) { return ivf_search(ivf, E, R); });
}

// A leased scratch set + stream for one blocking call: any number of host threads may call the host-pointer
// entry points on one index; each call takes a free set (or waits for one) and gives it back when it returns.
// With stage profiling on, the call runs on the index's own stream with set 0 instead (a measuring run is one thread).
struct Lease {
  fvdb_ivf* ivf;
  int idx = -1;
  Env E{};
  int rc = FVDB_OK;
  explicit Lease(fvdb_ivf* ivf_) : ivf(ivf_) {
    if (ivf->ctx->profiling) {
      E = Env{ivf->ctx, ivf};
      return;
    }
    std::unique_lock<std::mutex> lk(ivf->mu);
    ivf->lease_cv.wait(lk, [&] { return ivf->lease_busy != (1u << fvdb_ivf::kLeases) - 1u; });
    for (uint32_t i = 0; i < fvdb_ivf::kLeases; ++i)
      if (!(ivf->lease_busy & (1u << i))) {
        idx = (int)i;
        break;
      }
    ivf->lease_busy |= 1u << idx;
    if (!ivf->lease_ctx[idx]) {
      rc = fvdb_ctx_create(ivf->ctx->device, &ivf->lease_ctx[idx]);
      if (rc) ivf->ctx->set_err("could not create a stream for a concurrent search");
    }
    E = Env{ivf->lease_ctx[idx], &ivf->lease_set[idx]};
  }
  ~Lease() {
    if (idx < 0) return;
    {
      std::lock_guard<std::mutex> lk(ivf->mu);
      ivf->lease_busy &= ~(1u << idx);
    }
    ivf->lease_cv.notify_one();
  }
};
// body(E) on a leased set, which goes back when the call returns
template <class Body>
int on_lease(fvdb_ivf* ivf, Body body) {
  Lease L(ivf);
  if (L.rc) return L.rc;
  return slot_done(ivf, L.E, body(L.E));
}
}  // namespace
}  // extern "C++"

int fvdb_ivf_search_dev(fvdb_ivf* ivf, const float* q_dev, uint32_t B, uint32_t k, uint32_t nprobe,
                        uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev, uint64_t* out_keys_dev) {
  return ivf_search(ivf, Env{ivf->ctx, ivf},
                    IvfSearch{IvfSearch::PROBED, q_dev, B, k, nprobe, out_ids_dev, out_dist_dev, out_counts_dev, out_keys_dev});
}

int fvdb_ivf_search_all_dev(fvdb_ivf* ivf, const float* q_dev, uint32_t B, uint32_t k, uint64_t* out_ids_dev,
                            float* out_dist_dev, uint32_t* out_counts_dev) {
  return ivf_search(ivf, Env{ivf->ctx, ivf}, IvfSearch{IvfSearch::ALL, q_dev, B, k, 0, out_ids_dev, out_dist_dev, out_counts_dev});
}

int fvdb_ivf_coarse_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t nprobe,
                             uint32_t* out_probes_dev) {
  if (!out_probes_dev) FAIL(ivf->ctx, FVDB_E_INVALID, "null output");
  IvfSearch R{IvfSearch::COARSE_ONLY, q_dev, B, 1, nprobe};
  R.probes_out = out_probes_dev;
  return search_on_slot(ivf, on, slot, kNoMask, R);
}

int fvdb_ivf_search_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t k,
                             uint32_t nprobe, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev,
                             uint64_t* out_keys_dev) {
  return search_on_slot(ivf, on, slot, kNoMask,
                        IvfSearch{IvfSearch::PROBED, q_dev, B, k, nprobe, out_ids_dev, out_dist_dev, out_counts_dev, out_keys_dev});
}

int fvdb_ivf_search_probes_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, const float* q_dev,
                                    const uint32_t* probes_dev, uint32_t B, uint32_t k, uint32_t nprobe,
                                    uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev,
                                    uint64_t* out_keys_dev) {
  if (!probes_dev) FAIL(ivf->ctx, FVDB_E_INVALID, "null probes");
  return search_on_slot(ivf, on, slot, kNoMask,
                        IvfSearch{IvfSearch::PROBED, q_dev, B, k, nprobe, out_ids_dev, out_dist_dev, out_counts_dev, out_keys_dev,
                                  probes_dev});
}

int fvdb_ivf_search_dev_slot_masked(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                    uint32_t k, uint32_t nprobe, uint64_t* out_ids_dev, float* out_dist_dev,
                                    uint32_t* out_counts_dev, uint64_t* out_keys_dev) {
  return search_on_slot(ivf, on, slot, masked_by(mask),
                        IvfSearch{IvfSearch::PROBED, q_dev, B, k, nprobe, out_ids_dev, out_dist_dev, out_counts_dev, out_keys_dev});
}

int fvdb_ivf_search_probes_dev_slot_masked(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev,
                                           const uint32_t* probes_dev, uint32_t B, uint32_t k, uint32_t nprobe,
                                           uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev,
                                           uint64_t* out_keys_dev) {
  return on_slot(ivf, on, slot, masked_by(mask), [&](const Env& E) -> int {
    if (!probes_dev) FAIL(E.ctx, FVDB_E_INVALID, "null probes");  // after the slot and the mask, as ever
    return ivf_search(ivf, E,
                      IvfSearch{IvfSearch::PROBED, q_dev, B, k, nprobe, out_ids_dev, out_dist_dev, out_counts_dev, out_keys_dev,
                                probes_dev});
  });
}

int fvdb_ivf_search_wide_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                  uint32_t k, uint32_t nprobe, uint64_t* out_ids_dev, float* out_dist_dev,
                                  uint32_t* out_counts_dev, uint64_t* out_keys_dev) {
  if (!ivf) return FVDB_E_INVALID;
  return search_on_slot(ivf, on, slot, mask ? masked_by(mask) : kNoMask,
                        IvfSearch{IvfSearch::WIDE, q_dev, B, k, nprobe, out_ids_dev, out_dist_dev, out_counts_dev, out_keys_dev});
}

// Radius search over the probed lists: fvdb_ivf_search_wide_dev_slot's lists, score stage and
// rules; the selection keeps the rows within radius_dev[b], at most max_results of them, and counts them all.
int fvdb_ivf_search_radius_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                    const float* radius_dev, uint32_t max_results, uint32_t nprobe, uint64_t* out_ids_dev,
                                    float* out_dist_dev, uint32_t* out_counts_dev, uint32_t* out_totals_dev) {
  if (!ivf) return FVDB_E_INVALID;
  return on_slot(ivf, on, slot, mask ? masked_by(mask) : kNoMask, [&](const Env& E) -> int {
    if (!radius_dev || !out_totals_dev) FAIL(E.ctx, FVDB_E_INVALID, "null argument");  // after the slot and the mask, as ever
    IvfSearch R{IvfSearch::RADIUS, q_dev, B, max_results, nprobe, out_ids_dev, out_dist_dev, out_counts_dev};
    R.radius = radius_dev;
    R.totals = out_totals_dev;
    return ivf_search(ivf, E, R);
  });
}

// The wide search with one allow-set per query.  Everything is checked before anything is enqueued:
// every mask of the table, named by a query or not, and every group index.
int fvdb_ivf_search_groups_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* const* masks, uint32_t G,
                                    const uint32_t* group_of_query, const float* q_dev, uint32_t B, uint32_t k, uint32_t nprobe,
                                    uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev, uint64_t* out_keys_dev) {
  if (!ivf) return FVDB_E_INVALID;
  return on_slot(ivf, on, slot, kNoMask, [&](Env& E) -> int {
    fvdb_ctx* ctx = E.ctx;
    if (G && !masks) FAIL(ctx, FVDB_E_INVALID, "null mask table");
    if (B && !group_of_query) FAIL(ctx, FVDB_E_INVALID, "null group array");
    if (B && G == 0) FAIL(ctx, FVDB_E_INVALID, "queries but no group");
    // the last entry is the pool's own words: what a null mask ("no filter") maps to
    std::vector<const uint64_t*> words((size_t)G + 1, ivf->pool.valid());
    for (uint32_t g = 0; g < G; ++g) {
      const fvdb_mask* m = masks[g];
      if (!m) continue;
      if (m->ivf != ivf) FAIL(ctx, FVDB_E_INVALID, "mask of another index");
      if (m->stamp != ivf->mutations) FAIL(ctx, FVDB_E_INVALID, "stale mask: the index changed after the mask was created");
      words[g] = m->words.as<uint64_t>();
    }
    for (uint32_t b = 0; b < B; ++b)
      if (group_of_query[b] >= G) FAIL(ctx, FVDB_E_INVALID, "group index out of range");
    // a grouped search is a masked one to everything that asks (the counter blocks, AUTO's watch); the words a stage
    // reads per batch are the pool's, the score stage reads each query's own
    E.live = ivf->pool.valid();
    const GroupSource src{words.data(), G + 1, group_of_query};
    return ivf_search(ivf, E, IvfSearch{IvfSearch::WIDE, q_dev, B, k, nprobe, out_ids_dev, out_dist_dev, out_counts_dev, out_keys_dev},
                      &src);
  });
}

int fvdb_ivf_search_shard_wide_dev_slot(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                        uint32_t k, uint32_t nprobe, const uint32_t* given_probes_dev, uint64_t* out_ids_dev,
                                        float* out_dist_dev, uint32_t* out_counts_dev, uint64_t* out_keys_dev) {
  if (!ivf) return FVDB_E_INVALID;
  return search_on_slot(ivf, on, slot, mask ? masked_by(mask) : kNoMask,
                        IvfSearch{IvfSearch::SHARD_WIDE, q_dev, B, k, nprobe, out_ids_dev, out_dist_dev, out_counts_dev,
                                  out_keys_dev, given_probes_dev});
}

// evaluate_search_quality's two searches and their comparison (src/ivf/operations.rs:344-377), resident: the search at
// nprobe and the search of every list in centroid-rank order run on the slot, their results stay in the slot's scratch,
// and one wave per query counts the matches.
int fvdb_ivf_search_quality_dev(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t k,
                                uint32_t nprobe, float* out_recall_dev, float* out_precision_dev) {
  if (!ivf) return FVDB_E_INVALID;
  if (!q_dev || !out_recall_dev || !out_precision_dev) FAIL(ivf->ctx, FVDB_E_INVALID, "null buffer");
  return on_slot(ivf, on, slot, kNoMask, [&](const Env& E) -> int {
    fvdb_ctx* ctx = E.ctx;
    IvfScratch& S = *E.S;
    if (!ivf->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "index not trained");
    const IvfSearch::Kind kind = k > FVDB_MAX_K ? IvfSearch::WIDE : IvfSearch::PROBED;
    int rc = check_k(ctx, kind, k, probed_lists(ivf, kind, nprobe));
    if (rc) return rc;
    if (B == 0) return FVDB_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)B * k;
    HIPCHK(ctx, S.s_qual.ensure(2 * (n * 12 + (size_t)B * 4)));
    char* p = (char*)S.s_qual.p;
    uint64_t* ids[2] = {(uint64_t*)p, (uint64_t*)p + n};
    float* dist[2] = {(float*)(p + n * 16), (float*)(p + n * 16) + n};
    uint32_t* cnt[2] = {(uint32_t*)(p + n * 24), (uint32_t*)(p + n * 24) + B};
    const uint32_t probes[2] = {nprobe, ivf->nlist};  // the configured search, the ground truth
    for (int i = 0; i < 2; ++i) {
      rc = ivf_search(ivf, E, IvfSearch{kind, q_dev, B, k, probes[i], ids[i], dist[i], cnt[i]});
      if (rc) return rc;
    }
    hipLaunchKernelGGL(search_quality_kernel, dim3(cdiv(B, 4)), dim3(256), 0, ctx->stream, ids[0], cnt[0], ids[1], cnt[1], B, k,
                       out_recall_dev, out_precision_dev);
    HIPCHK(ctx, hipGetLastError());
    return FVDB_OK;
  });
}

// evaluate_search_quality at every nprobe from one search of every list (kernels_curve.h; src/ivf/operations.rs
// :329-391 answers for one n_probe per call).  Per chunk of queries: the every-list search in centroid-rank order leaves
// its ranking and its keys in blocks this call owns, one workgroup per query counts the truth rows of each rank, and one
// thread per nprobe adds the chunk's values to the running sums in query order.
// The chunk's ranking [chunk][nlist] and its two f32 matrices of that shape stay under this.
constexpr uint64_t kCurveArenaBytes = 256ull << 20;
static_assert(kCurveMaxLists == kRankSortMaxLists, "the curve's LDS tables and the ranking's sort serve the same indexes");
int fvdb_ivf_quality_curve_dev(fvdb_ivf* ivf, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                               uint32_t k, uint32_t chunk_queries, float* out_recall_sum_dev, float* out_precision_sum_dev) {
  if (!ivf) return FVDB_E_INVALID;
  if (!q_dev || !out_recall_sum_dev || !out_precision_sum_dev) FAIL(ivf->ctx, FVDB_E_INVALID, "null buffer");
  return on_slot(ivf, on, slot, mask ? masked_by(mask) : kNoMask, [&](const Env& E) -> int {
    fvdb_ctx* ctx = E.ctx;
    IvfScratch& S = *E.S;
    if (!ivf->trained) FAIL(ctx, FVDB_E_NOT_TRAINED, "index not trained");
    const uint32_t nlist = ivf->nlist;
    const IvfSearch::Kind kind = k > FVDB_MAX_K ? IvfSearch::WIDE : IvfSearch::PROBED;
    int rc = check_k(ctx, kind, k, nlist);
    if (rc) return rc;
    if ((rc = check_rank(ctx, ivf, nlist))) return rc;
    if (ivf->glob_set) FAIL(ctx, FVDB_E_UNSUPPORTED, "the quality curve does not serve a shard of a larger index");
    if (B == 0) return FVDB_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if ((rc = upload_table(ivf))) return rc;
    uint32_t chunk = (uint32_t)std::max<uint64_t>(1, kCurveArenaBytes / ((uint64_t)nlist * 12));
    if (chunk_queries) chunk = std::min(chunk, chunk_queries);
    chunk = std::min(chunk, B);
    const size_t mat = (size_t)chunk * nlist;
    HIPCHK(ctx, S.s_clive.ensure((size_t)nlist * 4));
    HIPCHK(ctx, S.s_cprobes.ensure(mat * 4));
    HIPCHK(ctx, S.s_ckeys.ensure((size_t)chunk * k * 8 + (size_t)chunk * 4));
    HIPCHK(ctx, S.s_cval.ensure(2 * mat * 4));
    uint64_t* keys = S.s_ckeys.as<uint64_t>();
    uint32_t* counts = (uint32_t*)(keys + (size_t)chunk * k);
    float* recall = S.s_cval.as<float>();
    float* precision = recall + mat;
    // like rank_sort_kernel's: the attribute belongs to the function, so every call sets the same value, the largest served
    HIPCHK(ctx, hipFuncSetAttribute((const void*)curve_query_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(kCurveMaxLists * 8)));
    const ListTable lists = list_table(ivf);
    hipLaunchKernelGGL(list_live_kernel, dim3(cdiv(nlist, 4)), dim3(256), 0, ctx->stream, lists.off, lists.blocks,
                       live_words(ivf, E), nlist, S.s_clive.as<uint32_t>());
    HIPCHK(ctx, hipMemsetAsync(out_recall_sum_dev, 0, (size_t)nlist * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(out_precision_sum_dev, 0, (size_t)nlist * 4, ctx->stream));
    for (uint32_t o = 0; o < B; o += chunk) {
      const uint32_t b = std::min(chunk, B - o);
      IvfSearch R{kind, q_dev + (size_t)o * ivf->d, b, k, nlist, nullptr, nullptr, counts, keys};
      R.probes_out = S.s_cprobes.as<uint32_t>();
      if ((rc = ivf_search(ivf, E, R))) return rc;
      CurveArgs a{};
      a.probes = S.s_cprobes.as<uint32_t>();
      a.list_off = lists.off;
      a.list_live = S.s_clive.as<uint32_t>();
      a.keys = keys;
      a.counts = counts;
      a.np = nlist;
      a.k = k;
      a.recall = recall;
      a.precision = precision;
      hipLaunchKernelGGL(curve_query_kernel, dim3(b), dim3(kCurveThreads), (size_t)nlist * 8, ctx->stream, a);
      hipLaunchKernelGGL(curve_sum_kernel, dim3(cdiv(nlist, 256)), dim3(256), 0, ctx->stream, recall, precision, b, nlist,
                         out_recall_sum_dev, out_precision_sum_dev);
    }
    HIPCHK(ctx, hipGetLastError());
    return FVDB_OK;
  });
}

// The blocking host-pointer searches: the batch is staged in a leased set, searched there, and the results copied back.
// RADIUS: radius[B] goes in behind the queries and out_totals[B] comes back behind the counts.
static int search_host(fvdb_ivf* ivf, IvfSearch::Kind kind, const float* q, uint32_t B, uint32_t k, uint32_t nprobe,
                       uint64_t* out_ids, float* out_dist, uint32_t* out_counts, const float* radius = nullptr,
                       uint32_t* out_totals = nullptr) {
  // ivf_search makes these refusals again, for every entry point; here they come before the input is read and a set is
  // leased, in the order callers know: not trained, nothing to do, k, non-finite input
  if (!ivf->trained) FAIL(ivf->ctx, FVDB_E_NOT_TRAINED, "index not trained");
  if (B == 0) return FVDB_OK;
  int rc = check_k(ivf->ctx, kind, k, probed_lists(ivf, kind, nprobe));
  if (rc) return rc;
  rc = check_finite(ivf->ctx, q, (uint64_t)B * ivf->d);
  if (rc) return rc;
  if (kind == IvfSearch::RADIUS) {
    if (!radius || !out_totals) FAIL(ivf->ctx, FVDB_E_INVALID, "null argument");
    for (uint32_t b = 0; b < B; ++b)
      if (!(radius[b] >= 0.0f)) FAIL(ivf->ctx, FVDB_E_INVALID, "radius must be >= 0 (+inf allowed), not negative or NaN");
  }
  return on_lease(ivf, [&](const Env& E) -> int {
    fvdb_ctx* ctx = E.ctx;
    IvfScratch& S = *E.S;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t q_bytes = (size_t)B * ivf->d * 4;
    HIPCHK(ctx, S.s_in.ensure(q_bytes + (size_t)B * 4));
    HIPCHK(ctx, S.s_out_ids.ensure((size_t)B * k * 8));
    HIPCHK(ctx, S.s_out_dist.ensure((size_t)B * k * 4));
    HIPCHK(ctx, S.s_out_cnt.ensure((size_t)B * 8));
    HIPCHK(ctx, hipMemcpyAsync(S.s_in.p, q, q_bytes, hipMemcpyHostToDevice, ctx->stream));
    IvfSearch R{kind, S.s_in.as<float>(), B, k, nprobe, S.s_out_ids.as<uint64_t>(), S.s_out_dist.as<float>(),
                S.s_out_cnt.as<uint32_t>()};
    if (radius) {
      HIPCHK(ctx, hipMemcpyAsync((char*)S.s_in.p + q_bytes, radius, (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
      R.radius = (const float*)((char*)S.s_in.p + q_bytes);
      R.totals = S.s_out_cnt.as<uint32_t>() + B;
    }
    int r = ivf_search(ivf, E, R);
    if (r) return r;
    if (out_totals)
      HIPCHK(ctx, hipMemcpyAsync(out_totals, S.s_out_cnt.as<uint32_t>() + B, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out_ids, S.s_out_ids.p, (size_t)B * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out_dist, S.s_out_dist.p, (size_t)B * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out_counts)
      HIPCHK(ctx, hipMemcpyAsync(out_counts, S.s_out_cnt.p, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FVDB_OK;
  });
}

int fvdb_ivf_search(fvdb_ivf* ivf, const float* q, uint32_t B, uint32_t k, uint32_t nprobe, uint64_t* out_ids,
                    float* out_dist, uint32_t* out_counts) {
  return search_host(ivf, IvfSearch::PROBED, q, B, k, nprobe, out_ids, out_dist, out_counts);
}
int fvdb_ivf_search_wide(fvdb_ivf* ivf, const float* q, uint32_t B, uint32_t k, uint32_t nprobe, uint64_t* out_ids,
                         float* out_dist, uint32_t* out_counts) {
  return search_host(ivf, IvfSearch::WIDE, q, B, k, nprobe, out_ids, out_dist, out_counts);
}
int fvdb_ivf_search_radius(fvdb_ivf* ivf, const float* q, uint32_t B, const float* radius, uint32_t max_results, uint32_t nprobe,
                           uint64_t* out_ids, float* out_dist, uint32_t* out_counts, uint32_t* out_totals) {
  return search_host(ivf, IvfSearch::RADIUS, q, B, max_results, nprobe, out_ids, out_dist, out_counts, radius, out_totals);
}
int fvdb_ivf_search_all(fvdb_ivf* ivf, const float* q, uint32_t B, uint32_t k, uint64_t* out_ids, float* out_dist,
                        uint32_t* out_counts) {
  return search_host(ivf, IvfSearch::ALL, q, B, k, 0, out_ids, out_dist, out_counts);
}

// The coarse stage with its centroid distances, for host rows: one batch, not sub-batched.
int fvdb_ivf_coarse(fvdb_ivf* ivf, const float* q, uint32_t B, uint32_t nprobe, uint32_t* out_clusters,
                    float* out_dist) {
  if (!ivf->trained) FAIL(ivf->ctx, FVDB_E_NOT_TRAINED, "index not trained");
  if (B == 0) return FVDB_OK;
  const uint32_t np = std::min(nprobe, ivf->nlist);
  if (np == 0) FAIL(ivf->ctx, FVDB_E_UNSUPPORTED, "nprobe must be > 0");
  int rc = check_rank(ivf->ctx, ivf, np);
  if (rc) return rc;
  rc = check_finite(ivf->ctx, q, (uint64_t)B * ivf->d);
  if (rc) return rc;
  return on_lease(ivf, [&](const Env& E) -> int {
    fvdb_ctx* ctx = E.ctx;
    IvfScratch& S = *E.S;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> enq(S.enq);
    HIPCHK(ctx, S.s_in.ensure((size_t)B * ivf->d * 4));
    HIPCHK(ctx, S.s_probes.ensure((size_t)B * np * 4));
    HIPCHK(ctx, S.s_cdist.ensure((size_t)B * np * 4));
    HIPCHK(ctx, hipMemcpyAsync(S.s_in.p, q, (size_t)B * ivf->d * 4, hipMemcpyHostToDevice, ctx->stream));
    const float* qpad = nullptr;
    int r = padded_queries(ivf, E, S.s_in.as<float>(), B, &qpad);
    if (r) return r;
    ensure_stage_events(ivf, S);
    r = run_coarse(ivf, E, qpad, B, np, S.s_probes.as<uint32_t>(), S.s_cdist.as<float>());
    if (r) return r;
    HIPCHK(ctx, hipMemcpyAsync(out_clusters, S.s_probes.p, (size_t)B * np * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out_dist)
      HIPCHK(ctx, hipMemcpyAsync(out_dist, S.s_cdist.p, (size_t)B * np * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FVDB_OK;
  });
}

int fvdb_ivf_set_coarse_mode(fvdb_ivf* ivf, int mode) {
  if (!ivf) return FVDB_E_INVALID;
  if (mode != FVDB_COARSE_AUTO && mode != FVDB_COARSE_EXACT) FAIL(ivf->ctx, FVDB_E_INVALID, "unknown coarse mode");
  ivf->coarse_mode = mode;
  return FVDB_OK;
}

int fvdb_ivf_set_scan_mode(fvdb_ivf* ivf, int mode) {
  if (!ivf) return FVDB_E_INVALID;
  if (mode != FVDB_SCAN_AUTO && mode != FVDB_SCAN_EXACT && mode != FVDB_SCAN_FILTER) FAIL(ivf->ctx, FVDB_E_INVALID, "unknown scan mode");
  ivf->scan_mode = mode;
  return FVDB_OK;
}

// the diagnostic entry points below describe the most recent search on the index, whichever scratch set it ran with
// (call them with no search in flight)
static IvfScratch& last_scratch(fvdb_ivf* ivf) {
  IvfScratch* S = ivf->last_set.load();
  return S ? *S : *ivf;
}

int fvdb_ivf_scan_survivors(fvdb_ivf* ivf, uint32_t* out, uint32_t B) {
  fvdb_ctx* ctx = ivf->ctx;
  IvfScratch& S = last_scratch(ivf);
  if (!S.s_scnt.p || S.s_scnt.cap < (size_t)B * 4) FAIL(ctx, FVDB_E_INVALID, "no matrix-core scan of that size has run");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipDeviceSynchronize());
  HIPCHK(ctx, hipMemcpyAsync(out, S.s_scnt.p, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}

int fvdb_ivf_scan_survivor_dump(fvdb_ivf* ivf, uint32_t query, uint32_t max_n, uint32_t* rank, uint32_t* pos, float* v,
                                uint32_t* n_out) {
  fvdb_ctx* ctx = ivf->ctx;
  *n_out = 0;
  IvfScratch& S = last_scratch(ivf);
  if (!S.s_scnt.p || !S.s_surv.p || S.s_scnt.cap < (size_t)(query + 1) * 4)
    FAIL(ctx, FVDB_E_INVALID, "no matrix-core scan holding that query has run");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipDeviceSynchronize());
  uint32_t cnt = 0;
  HIPCHK(ctx, hipMemcpyAsync(&cnt, S.s_scnt.as<uint32_t>() + query, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const uint32_t n = std::min(std::min(cnt, kMfmaCmax), max_n);
  std::vector<uint32_t> sv((size_t)n * 2);
  if (n) {
    HIPCHK(ctx, hipMemcpyAsync(sv.data(), (const char*)S.s_surv.p + (size_t)query * kMfmaCmax * 8, (size_t)n * 8,
                               hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(v, S.s_sdist.as<float>() + (size_t)query * kMfmaCmax, (size_t)n * 4, hipMemcpyDeviceToHost,
                               ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  for (uint32_t i = 0; i < n; ++i) {
    rank[i] = sv[2 * i];
    pos[i] = sv[2 * i + 1];
  }
  *n_out = n;
  return FVDB_OK;
}

// n words of the counter block from `first` on (zeros while there is no block yet)
static int read_counters(fvdb_ivf* ivf, FbWord first, uint32_t n, uint64_t* out) {
  fvdb_ctx* ctx = ivf->ctx;
  for (uint32_t i = 0; i < n; ++i) out[i] = 0;
  if (!ivf->s_fallbacks.p) return FVDB_OK;
  uint32_t v[2 * FB_WORDS] = {};  // the unmasked searches' block, then the masked searches'
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(v, ivf->s_fallbacks.p, kFbAllBytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (uint32_t i = 0; i < n; ++i) out[i] = (uint64_t)v[first + i] + v[FB_WORDS + first + i];
  return FVDB_OK;
}
int fvdb_ivf_scan_fallbacks(fvdb_ivf* ivf, uint64_t* out) { return read_counters(ivf, FB_SCAN, 1, out); }
int fvdb_ivf_scan_fallback_reasons(fvdb_ivf* ivf, uint64_t* out5) { return read_counters(ivf, FB_REASONS, kFbReasonWords, out5); }
int fvdb_ivf_coarse_fallbacks(fvdb_ivf* ivf, uint64_t* out) { return read_counters(ivf, FB_COARSE, 1, out); }

int fvdb_ivf_last_stats(fvdb_ivf* ivf, fvdb_search_stats* out) {
  fvdb_ctx* ctx = ivf->ctx;
  IvfScratch& S = last_scratch(ivf);
  if (!S.s_scalars.p) {
    std::memset(out, 0, sizeof(*out));
    return FVDB_OK;
  }
  unsigned long long st[3];
  HIPCHK(ctx, hipDeviceSynchronize());
  HIPCHK(ctx, hipMemcpyAsync(st, S.scalar(SC_STATS), sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  out->rows_scanned = st[0];
  out->work_items = st[1];
  out->list_rows_touched = st[2];
  return FVDB_OK;
}

int fvdb_ivf_profile_collect(fvdb_ivf* ivf) {
  IvfScratch* S = ivf->last_set.load();  // the most recent search, whichever scratch set and stream it used
  fvdb_ctx* c = ivf->last_ctx.load();
  if (!S || !c || !S->pending_profile) return FVDB_OK;
  S->collecting = true;
  int rc = finish_profile(ivf, Env{c, S}, S->pend_coarse, S->pend_fine);
  S->collecting = false;
  S->pending_profile = false;
  return rc;
}

// stage times accumulated while profiling is on: ms[5] = coarse scan, coarse merge, plan, fine scan,
// fine merge; returns the number of searches accumulated and resets.
uint64_t fvdb_ivf_stage_times(fvdb_ivf* ivf, float* ms_out) {
  for (int i = 0; i < 8; ++i) {
    ms_out[i] = ivf->stage_ms[i];
    ivf->stage_ms[i] = 0;
  }
  const uint64_t c = ivf->stage_calls;
  ivf->stage_calls = 0;
  return c;
}

// =============================================================================================
// k-means training on the GPU (src/ivf/core.rs:240-429)
// =============================================================================================
namespace {
struct TrainJob {
  fvdb_ivf* ivf;
  const float* X;
  uint64_t n;
  DBuf dmind, dassign, dnew, ddist, dsc;  // freed when the job returns
  float* cent = nullptr;                  // ivf->d_centroids_rm
  uint32_t gn = 0;
  int seed_centroids(uint64_t seed), error(float* out_err), iterate(uint32_t max_iterations, fvdb_train_result* res);
};

// k-means++ seeding (:336-371); draws from SplitMix64(seed)
int TrainJob::seed_centroids(uint64_t seed) {
  fvdb_ctx* ctx = ivf->ctx;
  const uint32_t nlist = ivf->nlist, d = ivf->d;
  struct {
    uint64_t s;
    uint64_t next() {
      uint64_t z = (s += 0x9E3779B97F4A7C15ull);
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      return z ^ (z >> 31);
    }
  } rng{seed};
  uint64_t pick = rng.next() % n;
  HIPCHK(ctx, hipMemcpyAsync(cent, X + pick * d, (size_t)d * 4, hipMemcpyDeviceToDevice, ctx->stream));
  hipLaunchKernelGGL(fill_f32_kernel, dim3(gn), dim3(256), 0, ctx->stream, dmind.as<float>(), n,
                     __builtin_huge_valf());
  uint32_t chosen = 1;
  for (uint32_t i = 1; i < nlist; ++i) {
    hipLaunchKernelGGL(kpp_min_dist_kernel, dim3(gn), dim3(256), 0, ctx->stream, X, d, n, pick,
                       dmind.as<float>());
    const float u = (float)(rng.next() >> 40) * (1.0f / 16777216.0f);
    hipLaunchKernelGGL(kpp_pick_kernel, dim3(1), dim3(256), 0, ctx->stream, dmind.as<float>(), n, u,
                       (unsigned long long*)dsc.p);
    unsigned long long p = 0;
    HIPCHK(ctx, hipMemcpyAsync(&p, dsc.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (p == ~0ull) continue;  // reference: the loop never fired, no centroid pushed this round
    pick = p;
    HIPCHK(ctx, hipMemcpyAsync(cent + (size_t)chosen * d, X + pick * d, (size_t)d * 4,
                               hipMemcpyDeviceToDevice, ctx->stream));
    chosen++;
  }
  if (chosen < nlist) FAIL(ctx, FVDB_E_INVALID, "k-means++ produced fewer centroids than n_clusters (degenerate data)");
  return FVDB_OK;
}

int TrainJob::error(float* out_err) {
  fvdb_ctx* ctx = ivf->ctx;
  hipLaunchKernelGGL(kmeans_point_dist_kernel, dim3(gn), dim3(256), 0, ctx->stream, X, ivf->d, n,
                     dassign.as<uint32_t>(), cent, ddist.as<float>());
  hipLaunchKernelGGL(seq_sqsum_mean_kernel, dim3(1), dim3(256), 0, ctx->stream, ddist.as<float>(), n,
                     (float*)dsc.p + 4);
  float r[2];
  HIPCHK(ctx, hipMemcpyAsync(r, (float*)dsc.p + 4, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *out_err = r[0];
  return FVDB_OK;
}

// Lloyd iterations from the seeded centroids; fills iterations, converged and the two errors of `res`
int TrainJob::iterate(uint32_t max_iterations, fvdb_train_result* res) {
  fvdb_ctx* ctx = ivf->ctx;
  HIPCHK(ctx, hipMemsetAsync(dassign.p, 0, n * 4, ctx->stream));  // assignments start at ClusterId(0) (:280)
  float prev_error = __builtin_huge_valf();
  int rc = error(&res->initial_error);
  if (rc) return rc;
  bool converged = false;
  uint32_t iterations = 0;
  for (uint32_t iter = 0; iter < max_iterations; ++iter) {
    iterations = iter + 1;
    rc = install_centroids(ivf, cent);
    if (rc) return rc;
    rc = assign_dev(ivf, X, n, dnew.as<uint32_t>());
    if (rc) return rc;
    HIPCHK(ctx, hipMemsetAsync(dsc.p, 0, 4, ctx->stream));
    hipLaunchKernelGGL(count_changed_kernel, dim3(gn), dim3(256), 0, ctx->stream, dnew.as<uint32_t>(),
                       dassign.as<uint32_t>(), n, (uint32_t*)dsc.p);
    uint32_t changed = 0;
    HIPCHK(ctx, hipMemcpyAsync(&changed, dsc.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    hipLaunchKernelGGL(kmeans_update_kernel, dim3(ivf->nlist), dim3(256), 0, ctx->stream, X, ivf->d, n,
                       dassign.as<uint32_t>(), cent);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (iterations >= max_iterations) break;
    float cur = 0;
    rc = error(&cur);
    if (rc) return rc;
    const float change = std::fabs(prev_error - cur) / prev_error;
    if (changed == 0 || change < 1e-4f) {
      converged = true;
      if (max_iterations == 10 && n < 20) {  // reference's small-test special case (:313-317)
        prev_error = cur;
        continue;
      }
      break;
    }
    prev_error = cur;
  }
  res->iterations = iterations;
  res->converged = converged ? 1 : 0;
  return error(&res->final_error);
}
}  // namespace

// Everything after "the rows are in HBM": X is [n][d] f32 on the device.  fvdb_ivf_train uploads its rows there,
// fvdb_ivf_train_from (ivf_maint.h) gathers them from another index's lists; the arithmetic is shared.
static int train_resident(fvdb_ivf* ivf, const float* X, uint64_t n, uint32_t max_iterations, uint64_t seed,
                          fvdb_train_result* out) {
  fvdb_ctx* ctx = ivf->ctx;
  const uint32_t nlist = ivf->nlist, d = ivf->d;
  TrainJob J{ivf, X, n};
  HIPCHK(ctx, J.dmind.ensure(n * 4));
  HIPCHK(ctx, J.dassign.ensure(n * 4));
  HIPCHK(ctx, J.dnew.ensure(n * 4));
  HIPCHK(ctx, J.ddist.ensure(n * 4));
  HIPCHK(ctx, J.dsc.ensure(64));
  HIPCHK(ctx, ivf->d_centroids_rm.ensure((size_t)nlist * d * 4));
  J.cent = ivf->d_centroids_rm.as<float>();
  J.gn = cdiv(n, 256);
  fvdb_train_result res{};
  int rc = J.seed_centroids(seed);
  if (rc) return rc;
  rc = J.iterate(max_iterations, &res);
  if (rc) return rc;
  ivf->h_centroids.resize((size_t)nlist * d);
  HIPCHK(ctx, hipMemcpyAsync(ivf->h_centroids.data(), J.cent, (size_t)nlist * d * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  rc = install_centroids(ivf, J.cent);
  if (rc) return rc;
  reset_lists(ivf);
  if (ivf->pool.valid() && ivf->pool.cap_blocks)
    HIPCHK(ctx, hipMemsetAsync(ivf->pool.valid(), 0, (size_t)ivf->pool.cap_blocks * 8, ctx->stream));
  if (out) *out = res;
  return FVDB_OK;
}

static int train_args_ok(fvdb_ivf* ivf, uint64_t n, uint32_t max_iterations) {
  fvdb_ctx* ctx = ivf->ctx;
  if (n == 0 || n < ivf->nlist) FAIL(ctx, FVDB_E_INSUFFICIENT, "insufficient training data");
  if (max_iterations == 0) FAIL(ctx, FVDB_E_INVALID, "max_iterations must be > 0");
  if (ivf->d > 2048) FAIL(ctx, FVDB_E_UNSUPPORTED, "training supports d <= 2048");
  return FVDB_OK;
}

int fvdb_ivf_train(fvdb_ivf* ivf, const float* x, uint64_t n, uint32_t max_iterations, uint64_t seed,
                   fvdb_train_result* out) {
  fvdb_ctx* ctx = ivf->ctx;
  int rc = train_args_ok(ivf, n, max_iterations);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = check_finite(ctx, x, n * ivf->d);
  if (rc) return rc;
  DBuf dx;
  HIPCHK(ctx, dx.ensure(n * ivf->d * 4));
  hipError_t e = hipMemcpyAsync(dx.p, x, n * ivf->d * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) FAIL(ctx, FVDB_E_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
  return train_resident(ivf, dx.as<float>(), n, max_iterations, seed, out);
}

// =============================================================================================
// merge of per-shard partial results
// =============================================================================================
int fvdb_merge_keys_dev(fvdb_ctx* ctx, const uint64_t* keys, const uint64_t* ids, uint32_t G, uint32_t B, uint32_t k,
                        uint64_t* out_ids, float* out_dist, uint32_t* out_counts) {
  if (k == 0 || k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "k must be in 1..FVDB_MAX_K");
  if (B == 0 || G == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint32_t grid = cdiv(B, 4);
  switch (kr_for(k)) {
    case 1: hipLaunchKernelGGL((merge_keys_kernel<1>), dim3(grid), dim3(256), 0, ctx->stream, keys, ids, G, B, k, out_ids, out_dist, out_counts); break;
    case 2: hipLaunchKernelGGL((merge_keys_kernel<2>), dim3(grid), dim3(256), 0, ctx->stream, keys, ids, G, B, k, out_ids, out_dist, out_counts); break;
    default: hipLaunchKernelGGL((merge_keys_kernel<4>), dim3(grid), dim3(256), 0, ctx->stream, keys, ids, G, B, k, out_ids, out_dist, out_counts); break;
  }
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int fvdb_merge_keys_wide_dev(fvdb_ctx* ctx, const uint64_t* keys, const uint64_t* ids, uint32_t G, uint32_t B, uint32_t k,
                             uint64_t* out_ids, float* out_dist, uint32_t* out_counts) {
  if (!ctx) return FVDB_E_INVALID;
  if (k == 0 || k > FVDB_MAX_K_WIDE) FAIL(ctx, FVDB_E_UNSUPPORTED, "k must be in 1..FVDB_MAX_K_WIDE");
  if (B == 0 || G == 0) return FVDB_OK;
  if (!keys || !ids || !out_ids || !out_dist) FAIL(ctx, FVDB_E_INVALID, "null buffer");
  if ((uint64_t)G * k >= (1ull << 31)) FAIL(ctx, FVDB_E_UNSUPPORTED, "too many partial lists for one merge");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(merge_keys_wide_kernel, dim3(B), dim3(256), 0, ctx->stream, keys, ids, G, B, k, out_ids, out_dist, out_counts);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// Diverse selection (kernels_mmr.h): one workgroup per query, everything in device memory
int fvdb_mmr_select_dev(fvdb_ctx* ctx, const float* rows_dev, uint32_t row_stride, const uint64_t* ids_dev, const float* dist_dev,
                        const uint32_t* counts_dev, uint32_t B, uint32_t fetch_k, uint32_t k, float lam, int distinct,
                        uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_rank_dev, uint32_t* out_counts_dev) {
  if (!ctx) return FVDB_E_INVALID;
  if (fetch_k == 0 || fetch_k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "fetch_k must be in 1..FVDB_MAX_K");
  if (k == 0 || k > fetch_k) FAIL(ctx, FVDB_E_INVALID, "k must be in 1..fetch_k");
  if (!(lam >= 0.0f && lam <= 1.0f)) FAIL(ctx, FVDB_E_INVALID, "lam must be in [0, 1]");
  if (row_stride == 0 || row_stride % 4 != 0) FAIL(ctx, FVDB_E_INVALID, "row_stride must be a positive multiple of 4");
  if (B == 0) return FVDB_OK;
  if (!rows_dev || !ids_dev || !dist_dev || !counts_dev || !out_ids_dev || !out_dist_dev || !out_rank_dev || !out_counts_dev)
    FAIL(ctx, FVDB_E_INVALID, "null buffer");
  if ((uintptr_t)rows_dev % 16 != 0) FAIL(ctx, FVDB_E_INVALID, "rows_dev must be 16-byte aligned");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const float a = lam, b = 1.0f - a;
  hipLaunchKernelGGL(mmr_select_kernel, dim3(B), dim3(256), 0, ctx->stream, rows_dev, row_stride, ids_dev, dist_dev, counts_dev,
                     fetch_k, k, a, b, distinct ? 1u : 0u, out_ids_dev, out_dist_dev, out_rank_dev, out_counts_dev);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// Grouped selection (kernels_group.h): one workgroup per query, everything in device memory.  Up to
// FVDB_MAX_K candidates the small instantiation (256 threads, 6.3 KiB of LDS), above it the full one (1024 threads,
// 100 KiB).
int fvdb_group_select_dev(fvdb_ctx* ctx, const uint64_t* ids_dev, const float* dist_dev, const uint32_t* counts_dev,
                          const uint8_t* key_tag_dev, const uint64_t* key_val_dev, uint32_t B, uint32_t fetch_k, uint32_t k,
                          uint32_t group_size, int distinct, int missing, uint64_t* out_ids_dev, float* out_dist_dev,
                          uint32_t* out_rank_dev, uint32_t* out_members_dev, uint32_t* out_group_total_dev, uint8_t* out_key_tag_dev,
                          uint64_t* out_key_val_dev, uint32_t* out_groups_dev, uint32_t* out_flags_dev) {
  if (!ctx) return FVDB_E_INVALID;
  if (fetch_k == 0 || fetch_k > FVDB_MAX_K_WIDE) FAIL(ctx, FVDB_E_UNSUPPORTED, "fetch_k must be in 1..FVDB_MAX_K_WIDE");
  if (k == 0 || group_size == 0) FAIL(ctx, FVDB_E_INVALID, "k and group_size must be at least 1");
  if ((uint64_t)k * group_size > FVDB_MAX_K_WIDE) FAIL(ctx, FVDB_E_UNSUPPORTED, "k * group_size must be at most FVDB_MAX_K_WIDE");
  if (missing != FVDB_GROUP_MISSING_DROP && missing != FVDB_GROUP_MISSING_OWN) FAIL(ctx, FVDB_E_INVALID, "missing must be DROP or OWN");
  if (B == 0) return FVDB_OK;
  if (!ids_dev || !dist_dev || !counts_dev || !key_tag_dev || !key_val_dev || !out_ids_dev || !out_dist_dev || !out_rank_dev ||
      !out_members_dev || !out_group_total_dev || !out_key_tag_dev || !out_key_val_dev || !out_groups_dev || !out_flags_dev)
    FAIL(ctx, FVDB_E_INVALID, "null buffer");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  GroupArgs a{};
  a.ids = ids_dev;
  a.dist = dist_dev;
  a.counts = counts_dev;
  a.key_tag = key_tag_dev;
  a.key_val = key_val_dev;
  a.fetch_k = fetch_k;
  a.k = k;
  a.group_size = group_size;
  a.distinct = distinct ? 1u : 0u;
  a.missing = missing == FVDB_GROUP_MISSING_OWN ? kGroupMissingOwn : kGroupMissingDrop;
  a.out_ids = out_ids_dev;
  a.out_dist = out_dist_dev;
  a.out_rank = out_rank_dev;
  a.out_members = out_members_dev;
  a.out_total = out_group_total_dev;
  a.out_key_tag = out_key_tag_dev;
  a.out_key_val = out_key_val_dev;
  a.out_groups = out_groups_dev;
  a.out_flags = out_flags_dev;
  if (fetch_k <= kGroupSmallMax) {
    hipLaunchKernelGGL((group_select_kernel<kGroupSmallMax, 256>), dim3(B), dim3(256), sizeof(GroupLds<kGroupSmallMax>), ctx->stream, a);
  } else {
    // like rank_sort_kernel's: the attribute belongs to the function, every call sets the same value
    HIPCHK(ctx, hipFuncSetAttribute((const void*)group_select_kernel<kGroupFullMax, 1024>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)sizeof(GroupLds<kGroupFullMax>)));
    hipLaunchKernelGGL((group_select_kernel<kGroupFullMax, 1024>), dim3(B), dim3(1024), sizeof(GroupLds<kGroupFullMax>), ctx->stream, a);
  }
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// =============================================================================================
// top-k / merge utilities (a4): src/core/vector_ops.rs:12-32,180-263, src/core/types.rs:206-223
// =============================================================================================
static int check_no_nan(fvdb_ctx* ctx, const float* x, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (x[i] != x[i]) FAIL(ctx, FVDB_E_NONFINITE, "NaN score (the reference panics in partial_cmp().unwrap())");
  return FVDB_OK;
}

int fvdb_top_k_indices_dev(fvdb_ctx* ctx, const float* scores_dev, uint32_t B, uint64_t n, uint32_t k, int heap,
                           uint64_t* out_idx_dev, uint32_t* out_counts_dev) {
  if (!ctx || !out_idx_dev || !out_counts_dev) return FVDB_E_INVALID;
  if (k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "k above FVDB_MAX_K");
  if (n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "rows longer than 2^32-2 scores");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (k == 0) {  // :181-183 `if k == 0 { return vec![] }`; take(0)
    HIPCHK(ctx, hipMemsetAsync(out_counts_dev, 0, (size_t)B * 4, ctx->stream));
    return FVDB_OK;
  }
  if (heap) {
    const size_t lds = (size_t)(k + 64) * sizeof(UItem) + 16;
    hipLaunchKernelGGL((topk_heap_kernel<false>), dim3(B), dim3(64), lds, ctx->stream, scores_dev, (const uint64_t*)nullptr, B,
                       (uint32_t)n, k, out_idx_dev, (float*)nullptr, out_counts_dev);
  } else {
    const uint32_t grid = cdiv(B, 4);
    switch (kr_for(k)) {
      case 1: hipLaunchKernelGGL((topk_sort_kernel<1>), dim3(grid), dim3(256), 0, ctx->stream, scores_dev, B, (uint32_t)n, k, out_idx_dev, out_counts_dev); break;
      case 2: hipLaunchKernelGGL((topk_sort_kernel<2>), dim3(grid), dim3(256), 0, ctx->stream, scores_dev, B, (uint32_t)n, k, out_idx_dev, out_counts_dev); break;
      default: hipLaunchKernelGGL((topk_sort_kernel<4>), dim3(grid), dim3(256), 0, ctx->stream, scores_dev, B, (uint32_t)n, k, out_idx_dev, out_counts_dev); break;
    }
  }
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int fvdb_streaming_top_k_dev(fvdb_ctx* ctx, const uint64_t* ids_dev, const float* scores_dev, uint32_t B, uint64_t n,
                             uint32_t k, uint64_t* out_ids_dev, float* out_scores_dev, uint32_t* out_counts_dev) {
  if (!ctx || !out_ids_dev || !out_counts_dev) return FVDB_E_INVALID;
  if (k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "k above FVDB_MAX_K");
  if (n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "rows longer than 2^32-2 scores");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (k == 0) {
    HIPCHK(ctx, hipMemsetAsync(out_counts_dev, 0, (size_t)B * 4, ctx->stream));
    return FVDB_OK;
  }
  const size_t lds = (size_t)(k + 64) * sizeof(UItem) + 16;
  hipLaunchKernelGGL((topk_heap_kernel<true>), dim3(B), dim3(64), lds, ctx->stream, scores_dev, ids_dev, B, (uint32_t)n, k,
                     out_ids_dev, out_scores_dev, out_counts_dev);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int fvdb_merge_search_results_dev(fvdb_ctx* ctx, const uint64_t* ids_dev, const float* dist_dev, uint32_t B, uint64_t n,
                                  uint32_t k, uint64_t* out_ids_dev, float* out_dist_dev, uint32_t* out_counts_dev) {
  if (!ctx || !out_ids_dev || !out_dist_dev || !out_counts_dev) return FVDB_E_INVALID;
  if (k > FVDB_MAX_K) FAIL(ctx, FVDB_E_UNSUPPORTED, "k above FVDB_MAX_K");
  if (n >= (1ull << 20)) FAIL(ctx, FVDB_E_UNSUPPORTED, "more than 2^20 results per query");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (k == 0) {
    HIPCHK(ctx, hipMemsetAsync(out_counts_dev, 0, (size_t)B * 4, ctx->stream));
    return FVDB_OK;
  }
  const uint32_t grid = cdiv(B, 4);
  switch (kr_for(k)) {
    case 1: hipLaunchKernelGGL((merge_dedup_kernel<1>), dim3(grid), dim3(256), 0, ctx->stream, ids_dev, dist_dev, B, (uint32_t)n, k, out_ids_dev, out_dist_dev, out_counts_dev); break;
    case 2: hipLaunchKernelGGL((merge_dedup_kernel<2>), dim3(grid), dim3(256), 0, ctx->stream, ids_dev, dist_dev, B, (uint32_t)n, k, out_ids_dev, out_dist_dev, out_counts_dev); break;
    default: hipLaunchKernelGGL((merge_dedup_kernel<4>), dim3(grid), dim3(256), 0, ctx->stream, ids_dev, dist_dev, B, (uint32_t)n, k, out_ids_dev, out_dist_dev, out_counts_dev); break;
  }
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// host-pointer forms: stage, run the device form, copy back
static int top_k_host(fvdb_ctx* ctx, const float* scores, uint32_t B, uint64_t n, uint32_t k, int heap, uint64_t* out_idx,
                      uint32_t* out_counts) {
  if (!ctx || !scores || !out_counts || (!out_idx && k)) return FVDB_E_INVALID;
  if (B == 0) return FVDB_OK;
  int rc = check_no_nan(ctx, scores, (uint64_t)B * n);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DBuf a, o1, oc;
  HIPCHK(ctx, a.exact(std::max<size_t>((size_t)B * n * 4, 16)));
  HIPCHK(ctx, o1.exact(std::max<size_t>((size_t)B * k * 8, 16)));
  HIPCHK(ctx, oc.exact((size_t)B * 4));
  HIPCHK(ctx, hipMemcpyAsync(a.p, scores, (size_t)B * n * 4, hipMemcpyHostToDevice, ctx->stream));
  rc = fvdb_top_k_indices_dev(ctx, a.as<const float>(), B, n, k, heap, o1.as<uint64_t>(), oc.as<uint32_t>());
  if (rc) return rc;
  if (k) HIPCHK(ctx, hipMemcpyAsync(out_idx, o1.p, (size_t)B * k * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(out_counts, oc.p, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}
int fvdb_top_k_indices(fvdb_ctx* ctx, const float* scores, uint32_t B, uint64_t n, uint32_t k, uint64_t* out_idx,
                       uint32_t* out_counts) {
  return top_k_host(ctx, scores, B, n, k, 0, out_idx, out_counts);
}
int fvdb_top_k_indices_heap(fvdb_ctx* ctx, const float* scores, uint32_t B, uint64_t n, uint32_t k, uint64_t* out_idx,
                            uint32_t* out_counts) {
  return top_k_host(ctx, scores, B, n, k, 1, out_idx, out_counts);
}

static int pairs_host(fvdb_ctx* ctx, const uint64_t* ids, const float* vals, uint32_t B, uint64_t n, uint32_t k, int merge,
                      uint64_t* out_ids, float* out_vals, uint32_t* out_counts) {
  if (!ctx || !ids || !vals || !out_counts || ((!out_ids || !out_vals) && k)) return FVDB_E_INVALID;
  if (B == 0) return FVDB_OK;
  int rc = check_no_nan(ctx, vals, (uint64_t)B * n);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DBuf a, b, o1, o2, oc;
  HIPCHK(ctx, a.exact(std::max<size_t>((size_t)B * n * 8, 16)));
  HIPCHK(ctx, b.exact(std::max<size_t>((size_t)B * n * 4, 16)));
  HIPCHK(ctx, o1.exact(std::max<size_t>((size_t)B * k * 8, 16)));
  HIPCHK(ctx, o2.exact(std::max<size_t>((size_t)B * k * 4, 16)));
  HIPCHK(ctx, oc.exact((size_t)B * 4));
  HIPCHK(ctx, hipMemcpyAsync(a.p, ids, (size_t)B * n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(b.p, vals, (size_t)B * n * 4, hipMemcpyHostToDevice, ctx->stream));
  rc = merge ? fvdb_merge_search_results_dev(ctx, a.as<const uint64_t>(), b.as<const float>(), B, n, k, o1.as<uint64_t>(),
                                             o2.as<float>(), oc.as<uint32_t>())
             : fvdb_streaming_top_k_dev(ctx, a.as<const uint64_t>(), b.as<const float>(), B, n, k, o1.as<uint64_t>(),
                                        o2.as<float>(), oc.as<uint32_t>());
  if (rc) return rc;
  if (k) {
    HIPCHK(ctx, hipMemcpyAsync(out_ids, o1.p, (size_t)B * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out_vals, o2.p, (size_t)B * k * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(ctx, hipMemcpyAsync(out_counts, oc.p, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}
int fvdb_streaming_top_k(fvdb_ctx* ctx, const uint64_t* ids, const float* scores, uint32_t B, uint64_t n, uint32_t k,
                         uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
  return pairs_host(ctx, ids, scores, B, n, k, 0, out_ids, out_scores, out_counts);
}
int fvdb_merge_search_results(fvdb_ctx* ctx, const uint64_t* ids, const float* dist, uint32_t B, uint64_t n, uint32_t k,
                              uint64_t* out_ids, float* out_dist, uint32_t* out_counts) {
  return pairs_host(ctx, ids, dist, B, n, k, 1, out_ids, out_dist, out_counts);
}

// =============================================================================================
// row store + candidate scoring
// =============================================================================================
int fvdb_store_create(fvdb_ctx* ctx, uint32_t d, uint64_t capacity_rows, fvdb_store** out) {
  return fvdb_store_create_ex(ctx, d, capacity_rows, FVDB_F32, out);
}

int fvdb_store_create_ex(fvdb_ctx* ctx, uint32_t d, uint64_t capacity_rows, int row_dtype, fvdb_store** out) {
  if (!ctx || !out) return FVDB_E_INVALID;
  *out = nullptr;
  if (d == 0) FAIL(ctx, FVDB_E_INVALID, "d must be > 0");
  if (row_dtype != FVDB_F32 && row_dtype != FVDB_F16) FAIL(ctx, FVDB_E_INVALID, "row_dtype must be FVDB_F32 or FVDB_F16");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  fvdb_store* s = new (std::nothrow) fvdb_store();
  if (!s) return FVDB_E_OOM;
  s->ctx = ctx;
  s->d = d;
  s->dpad = ((d + 3) / 4) * 4;  // either element: the row stride stays a multiple of 8 bytes
  s->dtype = (uint32_t)row_dtype;
  s->cap = std::max<uint64_t>(capacity_rows, 64);
  if (s->rows_buf.exact(s->cap * s->row_bytes()) != hipSuccess) {
    delete s;
    FAIL(ctx, FVDB_E_OOM, "store allocation failed");
  }
  s->data = s->rows_buf.p;
  *out = s;
  return FVDB_OK;
}

void fvdb_store_destroy(fvdb_store* s) {
  if (!s) return;
  (void)hipSetDevice(s->ctx->device);
  (void)hipStreamSynchronize(s->ctx->stream);
  delete s;
}

uint64_t fvdb_store_rows(fvdb_store* s) { return s->rows; }
int fvdb_store_dtype(fvdb_store* s) { return (int)s->dtype; }
uint64_t fvdb_store_bytes(fvdb_store* s) { return s->rows * (uint64_t)s->row_bytes(); }

int fvdb_store_append(fvdb_store* s, const float* rows, uint64_t n, uint64_t* first_row) {
  fvdb_ctx* ctx = s->ctx;
  if (first_row) *first_row = s->rows;
  if (n == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = check_finite(ctx, rows, n * s->d);
  if (rc) return rc;
  if (s->rows + n >= 0xFFFFFFFFull) FAIL(ctx, FVDB_E_UNSUPPORTED, "store limited to 2^32-1 rows");
  if (s->rows + n > s->cap) {
    uint64_t ncap = std::max<uint64_t>(s->rows + n, s->cap + s->cap / 2);
    HIPCHK(ctx, grow_keeping(s->rows_buf, ncap * s->row_bytes(), s->rows * s->row_bytes(), /*zero_rest=*/false, ctx->stream));
    s->data = s->rows_buf.p;
    s->cap = ncap;
  }
  void* dstv = (char*)s->data + s->rows * s->row_bytes();
  float* dst = (float*)dstv;
  if (s->f16()) {  // rounded to nearest even on the device, pads zero
    HIPCHK(ctx, s->s_in.ensure(n * s->d * 4));
    HIPCHK(ctx, hipMemcpyAsync(s->s_in.p, rows, n * s->d * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(pad_rows_f16_kernel, dim3(cdiv(n * s->dpad, 256)), dim3(256), 0, ctx->stream, s->s_in.as<float>(),
                       s->d, s->dpad, n, (half_t*)dstv);
    HIPCHK(ctx, hipGetLastError());
  } else if (s->d == s->dpad) {
    HIPCHK(ctx, hipMemcpyAsync(dst, rows, n * s->d * 4, hipMemcpyHostToDevice, ctx->stream));
  } else {
    HIPCHK(ctx, s->s_in.ensure(n * s->d * 4));
    HIPCHK(ctx, hipMemcpyAsync(s->s_in.p, rows, n * s->d * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(pad_rows_kernel, dim3(cdiv(n * s->dpad, 256)), dim3(256), 0, ctx->stream, s->s_in.as<float>(),
                       s->d, s->dpad, n, dst);
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  s->rows += n;
  return FVDB_OK;
}

int fvdb_store_get(fvdb_store* s, uint64_t row, float* out) {
  fvdb_ctx* ctx = s->ctx;
  if (row >= s->rows) FAIL(ctx, FVDB_E_NOT_FOUND, "row out of range");
  if (s->f16()) {  // widened on the host: exact
    std::vector<_Float16> h(s->d);
    HIPCHK(ctx, hipMemcpyAsync(h.data(), (const char*)s->data + row * s->row_bytes(), (size_t)s->d * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t j = 0; j < s->d; ++j) out[j] = (float)h[j];
    return FVDB_OK;
  }
  HIPCHK(ctx, hipMemcpyAsync(out, (const float*)s->data + row * s->dpad, (size_t)s->d * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}

int fvdb_score_candidates(fvdb_store* s, const float* q, uint32_t B, const uint32_t* cand, uint32_t C, float* out) {
  fvdb_ctx* ctx = s->ctx;
  if (B == 0 || C == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = check_finite(ctx, q, (uint64_t)B * s->d);
  if (rc) return rc;
  for (uint64_t i = 0; i < (uint64_t)B * C; ++i)
    if (cand[i] != FVDB_NO_ROW && cand[i] >= s->rows) FAIL(ctx, FVDB_E_NOT_FOUND, "candidate row out of range");
  HIPCHK(ctx, s->s_in.ensure((size_t)B * s->d * 4));
  HIPCHK(ctx, s->s_q.ensure((size_t)B * s->dpad * 4));
  HIPCHK(ctx, s->s_cand.ensure((size_t)B * C * 4));
  HIPCHK(ctx, s->s_out.ensure((size_t)B * C * 4));
  const float* qd = nullptr;
  if (s->d == s->dpad) {
    HIPCHK(ctx, hipMemcpyAsync(s->s_q.p, q, (size_t)B * s->d * 4, hipMemcpyHostToDevice, ctx->stream));
  } else {
    HIPCHK(ctx, hipMemcpyAsync(s->s_in.p, q, (size_t)B * s->d * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(pad_rows_kernel, dim3(cdiv((uint64_t)B * s->dpad, 256)), dim3(256), 0, ctx->stream,
                       s->s_in.as<float>(), s->d, s->dpad, (uint64_t)B, s->s_q.as<float>());
  }
  qd = s->s_q.as<float>();
  HIPCHK(ctx, hipMemcpyAsync(s->s_cand.p, cand, (size_t)B * C * 4, hipMemcpyHostToDevice, ctx->stream));
  if (s->f16())
    hipLaunchKernelGGL(score_candidates_kernel<half_t>, dim3(cdiv((uint64_t)B * C, 256)), dim3(256), 0, ctx->stream, (const half_t*)s->data,
                       s->dpad, qd, s->s_cand.as<uint32_t>(), B, C, C, s->s_out.as<float>());
  else
    hipLaunchKernelGGL(score_candidates_kernel<float>, dim3(cdiv((uint64_t)B * C, 256)), dim3(256), 0, ctx->stream, (const float*)s->data,
                       s->dpad, qd, s->s_cand.as<uint32_t>(), B, C, C, s->s_out.as<float>());
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(out, s->s_out.p, (size_t)B * C * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}

int fvdb_scorer_create(fvdb_store* s, uint32_t max_B, uint32_t max_C, fvdb_scorer** out) {
  fvdb_ctx* ctx = s->ctx;
  if (!out || max_B == 0 || max_C == 0) FAIL(ctx, FVDB_E_INVALID, "bad scorer shape");
  *out = nullptr;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  fvdb_scorer* sc = new (std::nothrow) fvdb_scorer();
  if (!sc) return FVDB_E_OOM;
  sc->store = s;
  sc->max_B = max_B;
  sc->max_C = max_C;
  const size_t nc = (size_t)max_B * max_C;
  if (sc->stream.create(hipStreamNonBlocking) != hipSuccess ||
      sc->q_buf.exact((size_t)max_B * s->dpad * 4) != hipSuccess ||
      sc->cand_buf.exact(nc * 4, hipHostMallocMapped) != hipSuccess ||
      sc->dist_buf.exact(nc * 4, hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer((void**)&sc->d_cand, sc->cand_buf.p, 0) != hipSuccess ||
      hipHostGetDevicePointer((void**)&sc->d_dist, sc->dist_buf.p, 0) != hipSuccess) {
    delete sc;
    FAIL(ctx, FVDB_E_OOM, "scorer allocation failed");
  }
  sc->d_q = sc->q_buf.as<float>();
  sc->h_cand = sc->cand_buf.as<uint32_t>();
  sc->h_dist = sc->dist_buf.as<float>();
  std::memset(sc->h_cand, 0xFF, nc * 4);
  *out = sc;
  return FVDB_OK;
}

void fvdb_scorer_destroy(fvdb_scorer* sc) {
  if (!sc) return;
  (void)hipSetDevice(sc->store->ctx->device);
  if (sc->stream) (void)hipStreamSynchronize(sc->stream);
  delete sc;
}

int fvdb_scorer_set_queries(fvdb_scorer* sc, const float* q, uint32_t B) {
  fvdb_store* s = sc->store;
  fvdb_ctx* ctx = s->ctx;
  if (B > sc->max_B) FAIL(ctx, FVDB_E_INVALID, "B above scorer capacity");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = check_finite(ctx, q, (uint64_t)B * s->d);
  if (rc) return rc;
  if (s->d == s->dpad) {
    HIPCHK(ctx, hipMemcpyAsync(sc->d_q, q, (size_t)B * s->d * 4, hipMemcpyHostToDevice, sc->stream));
  } else {
    HIPCHK(ctx, sc->s_in.ensure((size_t)B * s->d * 4));
    HIPCHK(ctx, hipMemcpyAsync(sc->s_in.p, q, (size_t)B * s->d * 4, hipMemcpyHostToDevice, sc->stream));
    hipLaunchKernelGGL(pad_rows_kernel, dim3(cdiv((uint64_t)B * s->dpad, 256)), dim3(256), 0, sc->stream,
                       sc->s_in.as<float>(), s->d, s->dpad, (uint64_t)B, sc->d_q);
  }
  HIPCHK(ctx, hipStreamSynchronize(sc->stream));
  return FVDB_OK;
}

int fvdb_scorer_set_query_rows(fvdb_scorer* sc, const uint32_t* rows, uint32_t B) {
  fvdb_store* s = sc->store;
  fvdb_ctx* ctx = s->ctx;
  if (B > sc->max_B) FAIL(ctx, FVDB_E_INVALID, "B above scorer capacity");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  for (uint32_t i = 0; i < B; ++i)
    if (rows[i] >= s->rows) FAIL(ctx, FVDB_E_NOT_FOUND, "query row out of range");
  HIPCHK(ctx, sc->s_rows.ensure((size_t)B * 4));
  HIPCHK(ctx, hipMemcpyAsync(sc->s_rows.p, rows, (size_t)B * 4, hipMemcpyHostToDevice, sc->stream));
  if (s->f16())
    hipLaunchKernelGGL(gather_rows_kernel<half_t>, dim3(cdiv((uint64_t)B * s->dpad, 256)), dim3(256), 0, sc->stream, (const half_t*)s->data,
                       sc->s_rows.as<uint32_t>(), s->dpad, B, sc->d_q);
  else
    hipLaunchKernelGGL(gather_rows_kernel<float>, dim3(cdiv((uint64_t)B * s->dpad, 256)), dim3(256), 0, sc->stream, (const float*)s->data,
                       sc->s_rows.as<uint32_t>(), s->dpad, B, sc->d_q);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(sc->stream));
  return FVDB_OK;
}

int fvdb_scorer_set_queries_dev(fvdb_scorer* sc, const float* q_dev, uint32_t B) {
  fvdb_store* s = sc->store;
  fvdb_ctx* ctx = s->ctx;
  if (B > sc->max_B) FAIL(ctx, FVDB_E_INVALID, "B above scorer capacity");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (s->d == s->dpad) {
    HIPCHK(ctx, hipMemcpyAsync(sc->d_q, q_dev, (size_t)B * s->d * 4, hipMemcpyDeviceToDevice, sc->stream));
  } else {
    hipLaunchKernelGGL(pad_rows_kernel, dim3(cdiv((uint64_t)B * s->dpad, 256)), dim3(256), 0, sc->stream, q_dev, s->d,
                       s->dpad, (uint64_t)B, sc->d_q);
    HIPCHK(ctx, hipGetLastError());
  }
  return FVDB_OK;  // stream-ordered before the next fvdb_scorer_run on this context
}

uint32_t* fvdb_scorer_cand_buffer(fvdb_scorer* sc) { return sc->h_cand; }
const float* fvdb_scorer_dist_buffer(fvdb_scorer* sc) { return sc->h_dist; }

int fvdb_scorer_launch(fvdb_scorer* sc, uint32_t B, uint32_t C) {
  fvdb_store* s = sc->store;
  fvdb_ctx* ctx = s->ctx;
  if (B > sc->max_B || C > sc->max_C) FAIL(ctx, FVDB_E_INVALID, "shape above scorer capacity");
  if (B == 0 || C == 0) return FVDB_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) return FVDB_E_HIP;  // current device is per host thread
  if (s->f16())
    hipLaunchKernelGGL(score_candidates_kernel<half_t>, dim3(cdiv((uint64_t)B * C, 256)), dim3(256), 0, sc->stream, (const half_t*)s->data,
                       s->dpad, sc->d_q, sc->d_cand, B, C, sc->max_C, sc->d_dist);
  else
    hipLaunchKernelGGL(score_candidates_kernel<float>, dim3(cdiv((uint64_t)B * C, 256)), dim3(256), 0, sc->stream, (const float*)s->data,
                       s->dpad, sc->d_q, sc->d_cand, B, C, sc->max_C, sc->d_dist);
  if (hipGetLastError() != hipSuccess) return FVDB_E_HIP;
  return FVDB_OK;
}

int fvdb_scorer_wait(fvdb_scorer* sc) {
  if (hipStreamSynchronize(sc->stream) != hipSuccess) return FVDB_E_HIP;
  return FVDB_OK;
}

int fvdb_scorer_run(fvdb_scorer* sc, uint32_t B, uint32_t C) {
  int rc = fvdb_scorer_launch(sc, B, C);
  if (rc) return rc;
  return fvdb_scorer_wait(sc);
}


}  // extern "C"

#include "ivf_maint.h"
#include "ivf_rows.h"
#include "comm_sharded.h"
#include "allow_masks.h"
#include "flat_search.h"
#include "meta_table.h"
