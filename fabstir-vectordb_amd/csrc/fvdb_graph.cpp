// fvdb_graph.cpp — the HNSW graph resident in HBM: traversal (fvdb_graph_search_dev*) and construction
// (fvdb_graph_insert_linked) entry points of the C ABI (include/fvdb.h).  gfx950 only.
//
// Adjacency has a fixed stride on every layer — row = [count, neighbours in list order] — so an insert rewrites only
// the rows it touches: the device-side insert (kernels_graph_build.h) edits them in place, a host-side insert patches
// them through fvdb_graph_set_lists.  Nothing re-flattens or re-uploads the whole graph after a mutation.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "fvdb_internal.h"
#include "common.h"
#include "kernels_graph.h"
#include "kernels_graph_fast.h"
#include "kernels_graph_build.h"
#include "kernels_graph_maint.h"
#include "kernels_graph_health.h"

using namespace fvdb;

struct fvdb_graph {
  fvdb_store* store = nullptr;
  uint32_t M = 0, M0 = 0;  // degree caps the strides are sized for (fvdb_graph_configure); 0 = follow the uploaded lists
  uint32_t stride0 = 0, strideU = 0;
  uint32_t n = 0, n_cap = 0;        // nodes (= store rows mirrored), capacity
  uint32_t u_rows = 0, u_cap = 0;   // rows of the layers above 0
  uint32_t entry = 0, top_level = 0;
  bool has_entry = false;
  DBuf d_level, d_deleted, d_ubase, d_adj0, d_adjU, d_dist0, d_distU, d_stamp0, d_stampU, d_state;
  DBuf d_spec, d_elog, d_chg, s_patch, s_codes;
  HBuf h_state, h_patch;
  bool dist_valid = false;          // dist0 / distU hold the distance of every stored edge
  uint32_t tag = 0;                 // batch counter for the row stamps (never 0)
  std::vector<uint32_t> h_level, h_ubase;
  uint64_t upload_bytes = 0;        // host -> device bytes of graph STRUCTURE (not vectors) since creation
  fvdb_graph_insert_stats last{};
  fvdb_graph_maintenance_info_t m_info{};  // the last fvdb_graph_vacuum
  // per-node results of the last fvdb_graph_health: the reach bitmap, the layer-0 component labels, and `mutations` then
  DBuf d_hreach, d_hlabel;
  uint32_t health_has = 0, health_n = 0;  // bit 0: d_hreach is filled, bit 1: d_hlabel is; the node count then
  uint64_t health_at = ~0ull;
  // form of the device insert's `visited` (fvdb_graph_set_insert_visited) and what the hashed form has seen since creation
  int ins_vis_mode = 0;
  uint32_t ins_vis_slots = 0;
  uint64_t ins_hashed = 0, ins_vis_over = 0, ins_vis_searches = 0, ins_vis_entries = 0;
  uint32_t ins_vis_peak = 0;
  DBuf s_q, d_counters;
  DBuf d_stamps, d_build_stamps;  // diagnostic builds only (-DFVDB_GRAPH_STAMPS, -DFVDB_BUILD_STAMPS)
  uint64_t tot_queries = 0, tot_again = 0;  // traversal counters [3], [2] folded in at every fvdb_graph_kernel_times
  static constexpr uint32_t kSlots = kGraphSlots;  // batches that may be in flight at once, each on its own stream
  DBuf s_visited[kSlots], s_touched[kSlots], s_spill[kSlots];
  uint32_t vis_B[kSlots] = {}, vis_words = 0, vis_tcap = 0, vis_stride = 0;
  bool uploaded = false;
  std::vector<uint8_t> h_deleted;  // host copy of the flags: searches skip the per-neighbour flag load when none is set
  uint64_t n_deleted = 0;
  // bumped by everything that changes the nodes, their links or their flags (upload, append_nodes, insert_linked,
  // set_lists, set_entry, set_deleted): a mask (fvdb_mask) built before the bump is refused by the masked searches
  uint64_t mutations = 0;
  DBuf s_scan[kSlots];  // exact scan under a mask (allow_masks.h): padded queries and partial lists, one per slot
  // profiling: HIP events around the last launches of the traversal kernel (ring of 64)
  DevEvent kev[64][2];
  uint32_t kev_n = 0;   // launches recorded since the last fvdb_graph_kernel_times call
  std::mutex mu;        // launch bookkeeping: searches in different slots may come from different host threads
};

namespace {

__global__ void graph_pad_rows_kernel(const float* __restrict__ src, uint32_t d, uint32_t dpad, uint64_t n, float* __restrict__ dst) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * dpad) return;
  const uint64_t r = i / dpad;
  const uint32_t c = (uint32_t)(i - r * dpad);
  dst[i] = c < d ? src[r * d + c] : 0.0f;
}

// packed rows [code, count, neighbours ...] (stride `ps` words) -> adjacency rows; one wave per row
__global__ __launch_bounds__(256) void graph_patch_kernel(const uint32_t* __restrict__ packed, uint32_t ps, uint32_t n_rows, uint32_t* __restrict__ adj0,
                                                          uint32_t stride0, uint32_t* __restrict__ adjU, uint32_t strideU) {
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (i >= n_rows) return;
  const uint32_t* p = packed + (size_t)i * ps;
  const uint32_t code = p[0], cnt = p[1];
  uint32_t* row = (code >> 31) ? adjU + (size_t)(code & 0x7FFFFFFFu) * strideU : adj0 + (size_t)code * stride0;
  if (lane < cnt) row[1 + lane] = p[2 + lane];
  if (lane == 0) row[0] = cnt;
}

// grow a device array to `new_bytes`, keeping the first `keep_bytes` and zeroing the rest
int grow_keep(fvdb_ctx* ctx, DBuf& b, size_t keep_bytes, size_t new_bytes) {
  if (new_bytes <= b.cap) return FVDB_OK;
  HIPCHK(ctx, grow_keeping(b, new_bytes, keep_bytes, /*zero_rest=*/true, ctx->stream));
  return FVDB_OK;
}

int reserve_nodes(fvdb_graph* g, uint32_t n_nodes, uint32_t u_rows) {
  fvdb_ctx* ctx = g->store->ctx;
  if (n_nodes > g->n_cap) {
    const uint32_t nc = std::max<uint32_t>(n_nodes, g->n_cap + g->n_cap / 2 + 1024);
    const size_t keep = g->n;
    int rc;
    if ((rc = grow_keep(ctx, g->d_level, keep * 4, (size_t)nc * 4))) return rc;
    if ((rc = grow_keep(ctx, g->d_deleted, keep * 4, (size_t)nc * 4))) return rc;
    if ((rc = grow_keep(ctx, g->d_ubase, keep * 4, (size_t)nc * 4))) return rc;
    if ((rc = grow_keep(ctx, g->d_stamp0, keep * 4, (size_t)nc * 4))) return rc;
    if ((rc = grow_keep(ctx, g->d_adj0, keep * g->stride0 * 4, (size_t)nc * g->stride0 * 4))) return rc;
    if ((rc = grow_keep(ctx, g->d_dist0, keep * g->stride0 * 4, (size_t)nc * g->stride0 * 4))) return rc;
    g->n_cap = nc;
    for (auto& v : g->vis_B) v = 0;  // visited maps are sized by the node count
  }
  if (u_rows > g->u_cap) {
    const uint32_t uc = std::max<uint32_t>(u_rows, g->u_cap + g->u_cap / 2 + 1024);
    const size_t keep = g->u_rows;
    int rc;
    if ((rc = grow_keep(ctx, g->d_stampU, keep * 4, (size_t)uc * 4))) return rc;
    if ((rc = grow_keep(ctx, g->d_adjU, keep * g->strideU * 4, (size_t)uc * g->strideU * 4))) return rc;
    if ((rc = grow_keep(ctx, g->d_distU, keep * g->strideU * 4, (size_t)uc * g->strideU * 4))) return rc;
    g->u_cap = uc;
  }
  return FVDB_OK;
}

int push_state(fvdb_graph* g, const BuildState& st) {
  fvdb_ctx* ctx = g->store->ctx;
  HIPCHK(ctx, g->d_state.ensure(sizeof(BuildState)));
  HIPCHK(ctx, g->h_state.ensure(sizeof(BuildState)));
  std::memcpy(g->h_state.p, &st, sizeof(BuildState));
  HIPCHK(ctx, hipMemcpyAsync(g->d_state.p, g->h_state.p, sizeof(BuildState), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}

int pull_state(fvdb_graph* g, BuildState* st) {
  fvdb_ctx* ctx = g->store->ctx;
  HIPCHK(ctx, g->h_state.ensure(sizeof(BuildState)));
  HIPCHK(ctx, hipMemcpyAsync(g->h_state.p, g->d_state.p, sizeof(BuildState), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(st, g->h_state.p, sizeof(BuildState));
  return FVDB_OK;
}

// The construction kernels are instantiated per 128-dim block count NB, FULL (no bounds checks) for the BASELINE
// dimensions 384 and 768, and, the insert pair, per form of the insert's `visited` (HASH: kernels_graph_build.h,
// Visited<>), and per row element (float, half_t).  Every instantiation of one template has the same signature, so
// choosing one is a lookup.
struct BuildKernels {
  decltype(&hnsw_insert_search_kernel<3, true, false>) search;
  decltype(&hnsw_insert_commit_kernel<3, true, false>) commit;
  decltype(&graph_edge_dist_kernel<3, true>) edge_dist;
};
template <int NB, bool FULL, typename RT>
BuildKernels build_kernels_rows(bool hashed) {
  if (hashed) return {hnsw_insert_search_kernel<NB, FULL, true, RT>, hnsw_insert_commit_kernel<NB, FULL, true, RT>, graph_edge_dist_kernel<NB, FULL, RT>};
  return {hnsw_insert_search_kernel<NB, FULL, false, RT>, hnsw_insert_commit_kernel<NB, FULL, false, RT>, graph_edge_dist_kernel<NB, FULL, RT>};
}
template <int NB, bool FULL>
BuildKernels build_kernels_of(const fvdb_store* s, bool hashed) {
  return s->f16() ? build_kernels_rows<NB, FULL, half_t>(hashed) : build_kernels_rows<NB, FULL, float>(hashed);
}
BuildKernels build_kernels(const fvdb_store* s, bool hashed) {
  const uint32_t dpad = s->dpad, nb128 = (dpad + 127) / 128;
  if (dpad == 384) return build_kernels_of<3, true>(s, hashed);
  if (dpad == 768) return build_kernels_of<6, true>(s, hashed);
  if (nb128 == 1) return build_kernels_of<1, false>(s, hashed);
  if (nb128 == 2) return build_kernels_of<2, false>(s, hashed);
  if (nb128 == 3) return build_kernels_of<3, false>(s, hashed);
  if (nb128 == 4) return build_kernels_of<4, false>(s, hashed);
  if (nb128 <= 6) return build_kernels_of<6, false>(s, hashed);
  return build_kernels_of<8, false>(s, hashed);
}

// What fvdb_graph_insert_linked would put in LDS for this graph now.  The fixed tables come first; `visited` and the
// restated `candidates` heap (512 .. 4096 slots) share what is left of the budget.
//   bitmap: one bit per node index — serves the graph while that still leaves the heap its minimum;
//   hashed: a table of node indices whose size does not depend on the graph — by default the largest power of two
//           that leaves the heap 2048 slots (8192 at ef_construction 200).
// FVDB_BUILD_LDS_LIMIT (the LDS budget, default 160 KiB) and FVDB_BUILD_BITMAP_MAX_NODES (a cap on the node count the
// bitmap serves) are test hooks, read at every call: they bring a small graph to the limits.
struct InsertPlan {
  uint32_t repr = 0;  // 0: nothing fits, 1 bitmap, 2 hashed
  uint32_t words = 0, slots = 0, cand_cap = 0, lds_bytes = 0, bitmap_max_nodes = 0;
  const char* why = "";
};
InsertPlan insert_plan(const fvdb_graph* g, uint32_t ef) {
  InsertPlan p;
  const uint32_t lds_max = getenv("FVDB_BUILD_LDS_LIMIT") ? (uint32_t)atoi(getenv("FVDB_BUILD_LDS_LIMIT")) : 160u * 1024u;
  const uint32_t fixed0 = build_lds_layout(0, ef, 0).total;
  const uint32_t kMinCand = 512 * 8;
  const uint32_t room = lds_max > fixed0 ? lds_max - fixed0 : 0;  // bytes for `visited` + `candidates`
  uint64_t bmax = room > kMinCand ? (uint64_t)((room - kMinCand) / 16) * 128 : 0;  // (the carve is padded to 16 bytes)
  if (getenv("FVDB_BUILD_BITMAP_MAX_NODES")) bmax = std::min<uint64_t>(bmax, (uint64_t)atoll(getenv("FVDB_BUILD_BITMAP_MAX_NODES")));
  p.bitmap_max_nodes = (uint32_t)std::min<uint64_t>(bmax, 0x7FFFFFFFu);
  auto cand_for = [&](uint32_t visited_bytes) -> uint32_t {
    return room >= visited_bytes ? std::min<uint32_t>(4096, ((room - visited_bytes) / 8) & ~1u) : 0u;
  };
  const bool bitmap_ok = g->n <= p.bitmap_max_nodes;
  uint32_t slots = 0;
  if (g->ins_vis_slots) {
    if (cand_for(g->ins_vis_slots * 4) >= 512) slots = g->ins_vis_slots;
  } else {
    for (uint32_t need : {2048u, 512u}) {
      for (uint32_t s2 = 32768; s2 >= 256 && !slots; s2 >>= 1)
        if (cand_for(s2 * 4) >= need) slots = s2;
      if (slots) break;
    }
  }
  if (g->ins_vis_mode != 2 && bitmap_ok) {
    p.repr = 1;
    p.words = (g->n + 31) / 32;
    p.cand_cap = cand_for((p.words * 4 + 15u) & ~15u);
  } else if (g->ins_vis_mode != 1 && slots) {
    p.repr = 2;
    p.words = p.slots = slots;
    p.cand_cap = cand_for(slots * 4);
  } else {
    p.why = g->ins_vis_mode == 2 ? "device insert: the LDS budget does not hold the hashed visited set"
            : g->ins_vis_mode == 1 || !bitmap_ok ? "device insert: graph too large for the on-chip visited bitmap"
                                                 : "device insert: the LDS budget holds neither form of the visited set";
    return p;
  }
  p.lds_bytes = build_lds_layout(p.words, ef, p.cand_cap).total;
  return p;
}

// the graph as the construction kernels see it; an insert adds ef and its LDS plan, the edge distances need neither
BuildView build_view(fvdb_graph* g, uint32_t ef = 0, const InsertPlan& plan = InsertPlan{}) {
  const fvdb_store* s = g->store;
  BuildView v{s->data, s->dpad, g->d_level.as<uint32_t>(), g->d_deleted.as<uint32_t>(), g->n_deleted ? 1u : 0u, g->d_ubase.as<uint32_t>(),
              g->d_adj0.as<uint32_t>(), g->d_dist0.as<float>(), g->d_adjU.as<uint32_t>(), g->d_distU.as<float>(), g->stride0, g->strideU,
              g->d_stamp0.as<uint32_t>(), g->d_stampU.as<uint32_t>(), g->M, g->M0, ef, plan.words, plan.cand_cap};
  v.state = (BuildState*)g->d_state.p;
  return v;
}

// distances of the stored edges: all rows (codes == nullptr) or the listed ones
int edge_dist(fvdb_graph* g, const uint32_t* codes_dev, const uint32_t* owner_dev, uint32_t n_rows, bool upper_all) {
  fvdb_ctx* ctx = g->store->ctx;
  if (n_rows == 0) return FVDB_OK;
  const size_t lds = 4 * (size_t)kTileRows * kScoreStride * 4;
  hipLaunchKernelGGL(build_kernels(g->store, false).edge_dist, dim3((n_rows + 3) / 4), dim3(256), lds, ctx->stream, build_view(g), codes_dev,
                     owner_dev, n_rows, upper_all ? 1u : 0u);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int ensure_edge_dist(fvdb_graph* g) {
  fvdb_ctx* ctx = g->store->ctx;
  if (g->dist_valid) return FVDB_OK;
  int rc = edge_dist(g, nullptr, nullptr, g->n, false);
  if (rc) return rc;
  if (g->u_rows) {  // owner of every upper row
    std::vector<uint32_t> owner(g->u_rows);
    for (uint32_t i = 0; i < g->n; ++i)
      for (uint32_t l = 1; l <= g->h_level[i]; ++l) owner[g->h_ubase[i] + l - 1] = i;
    HIPCHK(ctx, g->s_codes.ensure((size_t)g->u_rows * 4));
    HIPCHK(ctx, hipMemcpyAsync(g->s_codes.p, owner.data(), (size_t)g->u_rows * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    rc = edge_dist(g, nullptr, g->s_codes.as<uint32_t>(), g->u_rows, true);
    if (rc) return rc;
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  g->dist_valid = true;
  return FVDB_OK;
}

// Environment knobs of the schedule and its launches: tuning aids for A/B runs (include/fvdb.h), read once per process.
struct BuildKnobs {
  static int num(const char* name, int unset) { return getenv(name) ? atoi(getenv(name)) : unset; }
  int mode = num("FVDB_BUILD_MODE", 0);  // not 0: replaces the caller's mode
  int k = num("FVDB_BUILD_K", 0);        // > 0: the batch size, fixed
  int kmax = num("FVDB_BUILD_KMAX", 0);  // > 0: the largest batch size the schedule adapts to
  // 0: the commit workgroup adopts speculated searches up to the first one an earlier insert of the batch invalidated,
  // searches that ONE itself (so every launch pair makes progress) and stops; the rest of the batch is speculated again,
  // in parallel, against the graph as it then stands
  uint32_t max_rerun = (uint32_t)std::max(0, num("FVDB_BUILD_RERUN", -1));
  // FVDB_BUILD_STRICT=1: a speculation is dropped when ANY row it expanded changed (round-3 first form; A/B runs)
  uint32_t strict = (uint32_t)num("FVDB_BUILD_STRICT", 0);
  // below this many nodes every insert lands in every other's neighbourhood: one at a time, no speculation
  uint32_t seq_below = (uint32_t)num("FVDB_BUILD_SEQ_BELOW", 256);
  bool exact_first = num("FVDB_BUILD_EXACT_FIRST", 1) != 0;  // A/B
};

// One launch group: what runs between two reads of the device's BuildState.
struct BuildGroup {
  bool speculate;        // true: `count` pairs of launches, the schedule's K speculated searches and then one commit;
  uint32_t count;        // false: one commit launch that searches and links `count` nodes itself, one after the other
  uint32_t exact_first;  // 1: the group's searches go straight to the restated heaps
};

// The schedule of one fvdb_graph_insert_linked call: host arithmetic between launch groups.
struct BuildSchedule {
  const BuildKnobs& knobs;
  const int mode;  // speculation pays once an insert touches a small part of the graph (mode 0 = choose; 1 = never; 2 = always)
  const uint32_t first, n;
  // (a call never speculates further than it has nodes to link: the logs of a batch are 160 KB per (insert, layer) slot)
  const uint32_t Kmax = std::min<uint32_t>((uint32_t)std::max(1, std::min(knobs.k > 0 ? knobs.k : (knobs.kmax > 0 ? knobs.kmax : 128), 256)),
                                           std::max<uint32_t>(8, n));
  uint32_t K = knobs.k > 0 ? Kmax : std::min<uint32_t>(16, Kmax);  // adapts to the run length of adopted speculations
  uint32_t exact_positions = 4;  // speculated searches of a batch that may start again with the restated heaps on a tie
  uint32_t ties_seen = 0;
  // where ties are the rule (duplicate vectors) the register-set attempt is wasted work: the next `exact_left` groups go
  // straight to the restated heaps, then the question is asked again
  uint32_t exact_left = 0, commit_ties_seen = 0;

  // the group to launch when `done` nodes of the call are linked
  BuildGroup next(uint32_t done) {
    BuildGroup grp{};
    grp.speculate = mode == 2 || (mode == 0 && (uint64_t)first + done >= knobs.seq_below && n - done >= 8);
    grp.exact_first = exact_left > 0 ? 1u : 0u;
    if (exact_left) exact_left -= 1;
    if (grp.speculate) {
      grp.count = std::min<uint32_t>(16, (n - done + K - 1) / K);  // the cursor lives on the device: no sync in between
    } else {
      grp.count = std::min<uint32_t>(n - done, 2048);  // bounds one launch to a fraction of a second
      if (mode == 0 && (uint64_t)first + done < knobs.seq_below) grp.count = std::min<uint32_t>(grp.count, knobs.seq_below - (first + done));
    }
    return grp;
  }

  // `st`: the state read back after `grp`, which started with `done` nodes linked
  void update(const BuildGroup& grp, uint32_t done, const BuildState& st) {
    const uint32_t linked = st.cursor - done;
    if (grp.speculate && knobs.k <= 0) {
      // a batch is adopted up to its first conflict: speculating much further than the usual run only adds stragglers
      // (the slowest of the batch's searches sets the launch's duration)
      const uint32_t run = linked / grp.count;
      K = std::min<uint32_t>(Kmax, std::max<uint32_t>(8, 2 * run + 4));
    }
    if (grp.speculate) {  // where ties are the rule (duplicate vectors) every speculation takes the exact search
      const uint32_t searched = grp.count * K, tied = st.spec_ties - ties_seen;  // (K as just adapted, not the group's)
      if (!grp.exact_first) exact_positions = 4 * tied > searched ? Kmax : 4;
      if (knobs.exact_first && !grp.exact_first && 2 * tied > searched) exact_left = 8;
      ties_seen = st.spec_ties;
    }
    if (!grp.speculate && knobs.exact_first && !grp.exact_first && 2 * (st.ties - commit_ties_seen) > linked) exact_left = 8;
    commit_ties_seen = st.ties;
  }
};

// the device's record of construction at the start of a call: entry point and n_linked stay, the cursor, the status and
// every counter start at zero
int reset_build_state(fvdb_graph* g, uint32_t first, BuildState* st) {
  int rc;
  if ((rc = pull_state(g, st))) return rc;
  if (st->n_linked != first) FAIL(g->store->ctx, FVDB_E_INVALID, "nodes are linked in store-row order");
  *st = BuildState{st->has_entry, st->entry, st->entry_level, st->n_linked};
  return push_state(g, *st);
}

// the launches of one group on the graph's stream, each with its own row-stamp tag
void launch_group(fvdb_graph* g, const BuildKernels& kernels, const BuildView& v, uint32_t lds, const BuildSchedule& sched, const BuildGroup& grp) {
  const uint32_t first = sched.first, n = sched.n;
  hipStream_t stream = g->store->ctx->stream;
  if (!grp.speculate) {
    g->tag += 1;
    hipLaunchKernelGGL(kernels.commit, dim3(1), dim3(kBuildThreads), lds, stream, v, first, n, grp.count, g->tag, 0u, nullptr, nullptr, nullptr, 1u);
    return;
  }
  for (uint32_t p = 0; p < grp.count; ++p) {
    g->tag += 1;
    hipLaunchKernelGGL(kernels.search, dim3(sched.K, kBuildLayers), dim3(kBuildThreads), lds, stream, v, first, n, sched.exact_positions,
                       g->tag, g->d_spec.as<uint32_t>(), g->d_elog.as<uint32_t>());
    hipLaunchKernelGGL(kernels.commit, dim3(1), dim3(kBuildThreads), lds, stream, v, first, n, sched.K, g->tag, sched.knobs.max_rerun,
                       g->d_spec.as<uint32_t>(), g->d_elog.as<uint32_t>(), g->d_chg.as<uint32_t>(), sched.knobs.strict);
  }
}

#ifdef FVDB_BUILD_STAMPS
// diagnostic build: the insert kernels add their phase times (10 ns ticks) into 64 words that this call owns
void build_stamps_begin(fvdb_graph* g, BuildView* v) {
  (void)g->d_build_stamps.ensure(64 * 8);
  (void)hipMemset(g->d_build_stamps.p, 0, 64 * 8);
  v->dbg = g->d_build_stamps.as<unsigned long long>();
}
void build_stamps_print(fvdb_graph* g, const BuildState& st, uint32_t done) {
  unsigned long long h[16] = {};
  (void)hipMemcpy(h, g->d_build_stamps.p, sizeof(h), hipMemcpyDeviceToHost);
  fprintf(stderr, "[build stamps] of replay+select (us): replay %.1f  select %.1f  (table = the rest) | admissions %.1f\n", h[6] * 0.01 / std::max(1u, st.n_rerun),
          h[7] * 0.01 / std::max(1u, st.n_rerun), (double)h[8] / std::max(1u, st.n_rerun));
  const double us = 0.01, nn = std::max(1u, st.n_rerun);
  fprintf(stderr, "[build stamps] per searched insert (us): replay+select %.1f  fetch %.1f  score %.1f | greedy %.1f  all searches %.1f  links %.1f"
          " | rounds %.1f expanded %.1f scored %.0f\n", h[0] * us / nn, h[1] * us / nn, h[2] * us / nn, h[3] * us / nn, h[4] * us / nn,
          h[5] * us / std::max(1u, done), st.rounds / nn, st.consumed / nn, st.scored / nn);
}
#else
inline void build_stamps_begin(fvdb_graph*, BuildView*) {}
inline void build_stamps_print(fvdb_graph*, const BuildState&, uint32_t) {}
#endif

// FVDB_BUILD_DEBUG: per-call diagnostics on stderr
void report_insert(const InsertPlan& plan, const BuildState& st) {
  if (!getenv("FVDB_BUILD_DEBUG")) return;
  fprintf(stderr, "[device insert] %u linked, %u adopted, stops %u: entry %u, gave-up %u, order/strict %u, caps %u, added node nearer than a later pop %u, added node inside the final set %u, dropped node matters %u | "
          "checks %u, touched rows %u\n", st.cursor, st.n_valid, st.n_stopped, st.why[1], st.why[2], st.why[3], st.why[4], st.why[5], st.why[6],
          st.why[9], st.why[7], st.why[8]);
  fprintf(stderr, "[device insert] searches that left the register set: pops tied %u, evictions tied %u, result tied %u, heap overflow %u | speculations given up or restarted %u\n",
          st.why[11], st.why[12], st.why[13], st.why[14], st.spec_ties);
  fprintf(stderr, "[device insert] second looks: overlapping %u, nodes the popped newcomer would bring in %u, later pop is the maximum %u\n", st.why[15], st.why[16], st.why[17]);
  if (plan.repr == 2)
    fprintf(stderr, "[device insert] hashed visited set, %u slots: %u searches gave up on a full set (%u of them inserts handed to the host), "
            "entries after a search: largest %u, mean %.0f over %u searches\n", plan.slots, st.why[18], st.vis_host, st.vis_peak,
            (double)st.vis_sum / std::max(1u, st.vis_searches), st.vis_searches);
}

// what a finished call leaves on the graph (entry point, the hashed set's totals, `last`) and hands to its caller
void fold_insert(fvdb_graph* g, const InsertPlan& plan, const BuildState& st, uint32_t launches, uint32_t* n_done,
                 fvdb_graph_insert_stats* stats) {
  if (plan.repr == 2) {
    g->ins_hashed += st.cursor;
    g->ins_vis_over += st.vis_host;
    g->ins_vis_searches += st.vis_searches;
    g->ins_vis_entries += st.vis_sum;
    g->ins_vis_peak = std::max(g->ins_vis_peak, st.vis_peak);
  }
  g->entry = st.entry;
  g->top_level = st.entry_level;
  g->has_entry = st.has_entry != 0;
  // n_done, needs_host | speculated_ok, searched_in_commit, commit_stops | rounds, expanded, rows_scored, tie_restarts | launches
  const fvdb_graph_insert_stats acc{st.cursor, st.status, st.n_valid, st.n_rerun, st.n_stopped, st.rounds, st.consumed, st.scored, st.ties, launches};
  g->last = acc;
  if (stats) *stats = acc;
  if (n_done) *n_done = st.cursor;
}

// The traversal kernels: the sorted-register kernel per (128-dim blocks NB, rows per scoring round R, byte map or bitmap
// as `visited`, row element), the exact-heap kernel per place of its `nearest` heap and row element.  The rows per round
// are the f32 table's for fp16 rows too: nothing has been measured that would justify another.
using FastKernel = decltype(&hnsw_search_fast_kernel<3, 16, true>);
using ExactKernel = decltype(&hnsw_search_kernel<true>);
template <int NB, int R>
FastKernel fast_kernel_of(bool bytemap, bool f16) {
  if (f16) return bytemap ? hnsw_search_fast_kernel<NB, R, true, half_t> : hnsw_search_fast_kernel<NB, R, false, half_t>;
  return bytemap ? hnsw_search_fast_kernel<NB, R, true> : hnsw_search_fast_kernel<NB, R, false>;
}
FastKernel fast_kernel(uint32_t nb128, int R, bool bytemap, bool f16) {
  switch (nb128) {
    case 1: return fast_kernel_of<1, 16>(bytemap, f16);
    case 2: return fast_kernel_of<2, 16>(bytemap, f16);
    case 3: return R == 8 ? fast_kernel_of<3, 8>(bytemap, f16) : R == 12 ? fast_kernel_of<3, 12>(bytemap, f16) : fast_kernel_of<3, 16>(bytemap, f16);
    case 4: return fast_kernel_of<4, 12>(bytemap, f16);
    case 5:
    case 6: return fast_kernel_of<6, 8>(bytemap, f16);
    default: return fast_kernel_of<8, 6>(bytemap, f16);
  }
}
ExactKernel exact_kernel(bool rh, bool f16) {
  if (f16) return rh ? hnsw_search_kernel<true, half_t> : hnsw_search_kernel<false, half_t>;
  return rh ? hnsw_search_kernel<true> : hnsw_search_kernel<false>;
}

// What one traversal launch works with.  search_plan decides all of it from (graph, B, ef) and touches nothing: the
// launch path and fvdb_graph_search_info both ask it, so a report cannot drift from what runs.  search_scratch then sizes
// the slot's buffers for the plan.
struct SearchPlan {
  bool bytemap;  // `visited` of a query: one byte per node, else one bit
  uint32_t words, vstride, tcap, spill_cap, cand_cap;
  uint32_t nb128;     // 128-dimension blocks of a padded row
  int R;              // rows per scoring round of the sorted-register kernel (0: the exact-heap kernel runs)
  size_t lds;         // dynamic LDS of a workgroup of the kernel chosen
  uint32_t wave_lds;  // the sorted-register kernel's share of it per query (4 queries to a workgroup)
  FastKernel fast;    // the sorted-register kernel, or
  ExactKernel exact;  // the exact-heap kernel, one query per workgroup;
  bool rh;            // its `nearest` in registers (ef <= 63): the candidates heap may continue in the HBM spill
};

int search_plan(const fvdb_graph* g, fvdb_ctx* ctx, uint32_t B, uint32_t ef, SearchPlan* sp) {
  // visited-log capacity per query: a query that outgrows it clears its whole map at the end of the layer instead of
  // entry by entry (FVDB_GRAPH_TCAP: test hook that forces that)
  sp->words = (g->n + 31) / 32;
  sp->tcap = getenv("FVDB_GRAPH_TCAP") ? std::max(1, atoi(getenv("FVDB_GRAPH_TCAP"))) : 8192;
  // visited set per query: one byte per node while a batch's maps stay under 1 GiB (no atomics, see
  // kernels_graph_fast.h), else one bit per node; the row stride is the same for both views
  static const bool no_bytes = getenv("FVDB_GRAPH_BITMAP") != nullptr;  // tuning aid / A-B (byte map: ~2.5 % faster, 8x the memory)
  const uint32_t vbytes = ((g->n + 63) / 64) * 64;
  sp->bytemap = !no_bytes && (uint64_t)vbytes * std::max<uint32_t>(B, 1024) <= (1ull << 30);
  sp->vstride = sp->bytemap ? vbytes : sp->words * 4;
  // where the restated candidates heap continues when it outgrows its LDS slots (duplicate-heavy data): no node is
  // admitted twice, so a query never needs more than n slots
  sp->spill_cap = std::min<uint32_t>(((g->n + 63) / 64) * 64, 8192);
  // candidate-heap slots of the exact-heap search: it holds every admitted node not yet expanded; a query that
  // overflows it goes to the host walk (data with many duplicate vectors fills it quickly, so it stays generous:
  // at the default tile size the sorted-register kernel's LDS need is larger anyway)
  const int cand_env = getenv("FVDB_GRAPH_CAND_CAP") ? atoi(getenv("FVDB_GRAPH_CAND_CAP")) : 0;  // test hook: forces the host-walk fallback
  sp->cand_cap = cand_env > 0 ? (uint32_t)cand_env : std::max<uint32_t>(1024, 8 * ef);
  sp->lds = graph_lds_bytes(g->store->dpad, ef, sp->cand_cap);  // of the exact-heap search
  if (sp->lds > 160 * 1024) FAIL(ctx, FVDB_E_UNSUPPORTED, "dimension / ef too large for the on-chip traversal state");
  static const bool lds_heaps = getenv("FVDB_GRAPH_LDS_HEAPS") != nullptr;  // tuning aid: lane-0 heaps for any ef
  sp->rh = ef <= 63 && !lds_heaps;
  // ef <= 63: the sorted-register kernel; a query in which two heap members meet with equal distances is re-run by
  // the same wave with the reference's heaps restated (exact on ties)
  static const bool no_fast = getenv("FVDB_GRAPH_NO_FAST") != nullptr;  // tuning aid / A-B
  static const int fast_r = getenv("FVDB_GRAPH_FAST_R") ? atoi(getenv("FVDB_GRAPH_FAST_R")) : 0;
  sp->nb128 = (g->store->dpad + 127) / 128;
  sp->R = 0;
  sp->wave_lds = 0;
  sp->fast = nullptr;
  sp->exact = nullptr;
  if (no_fast || !sp->rh || sp->nb128 > 8 || g->n >= 0x80000000u) {
    sp->exact = exact_kernel(sp->rh, g->store->f16());
    return FVDB_OK;
  }
  sp->R = sp->nb128 <= 3 ? 16 : (sp->nb128 == 4 ? 12 : (sp->nb128 <= 6 ? 8 : 6));  // rows per scoring round: registers R*NB*2
  if (sp->nb128 == 3 && (fast_r == 8 || fast_r == 12)) sp->R = fast_r;
  sp->wave_lds = (uint32_t)((std::max(graph_fast_lds_bytes((uint32_t)sp->R), sp->lds) + 15) & ~(size_t)15);
  sp->lds = 4 * (size_t)sp->wave_lds;
  if (sp->lds > 160 * 1024) FAIL(ctx, FVDB_E_UNSUPPORTED, "dimension / ef too large for the on-chip traversal state");
  sp->fast = fast_kernel(sp->nb128, sp->R, sp->bytemap, g->store->f16());
  return FVDB_OK;
}

// sizes and (re)zeroes the slot's visited maps, touched log and spill for the plan of (B, n)
int search_scratch(fvdb_graph* g, fvdb_ctx* ctx, uint32_t slot, uint32_t B, const SearchPlan* sp) {
  if (sp->words != g->vis_words || sp->tcap != g->vis_tcap || sp->vstride != g->vis_stride) {
    for (auto& v : g->vis_B) v = 0;
    g->vis_words = sp->words;
    g->vis_tcap = sp->tcap;
    g->vis_stride = sp->vstride;
  }
  if (B > g->vis_B[slot]) {  // the maps are left all-zero by every search: zero once
    HIPCHK(ctx, g->s_visited[slot].ensure((size_t)B * sp->vstride));
    HIPCHK(ctx, hipMemsetAsync(g->s_visited[slot].p, 0, g->s_visited[slot].cap, ctx->stream));
    HIPCHK(ctx, g->s_touched[slot].ensure((size_t)B * sp->tcap * 4));
    g->vis_B[slot] = B;
  }
  HIPCHK(ctx, g->s_spill[slot].ensure((size_t)B * sp->spill_cap * 8));
  return FVDB_OK;
}

#ifdef FVDB_GRAPH_STAMPS
// diagnostic build: prints what the traversal launches since the last call stamped (sums, and per query of the last
// launch: cycles, placement, start and lifetime), clears it and returns the words for the next launch to write
unsigned long long* graph_stamps_report(fvdb_graph* g) {
  constexpr size_t kStampWords = 8 + 3 * 16384 + 4;  // 8 sums, then per query (cycles, hops, start tick) of the last launch
  if (!g->d_stamps.p) {
    (void)g->d_stamps.ensure(kStampWords * 8);
    (void)hipMemset(g->d_stamps.p, 0, kStampWords * 8);
  }
  unsigned long long* d_stamps = g->d_stamps.as<unsigned long long>();
  (void)hipDeviceSynchronize();
  std::vector<unsigned long long> h(kStampWords);
  (void)hipMemcpy(h.data(), d_stamps, kStampWords * 8, hipMemcpyDeviceToHost);
  fprintf(stderr, "[graph stamps, cumulative] s0 %llu s1 %llu s2 %llu s3 %llu | rows %llu rounds %llu hops %llu total %llu | score: issue %llu "
          "first-block wait+products %llu other-block products %llu adds %llu\n",
          h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8 + 3 * 16384], h[8 + 3 * 16384 + 1], h[8 + 3 * 16384 + 2], h[8 + 3 * 16384 + 3]);
  std::vector<unsigned long long> cyc, hp, rt;
  {
    // placement: HW_ID bits [3:0] wave, [5:4] simd, [11:8] cu, [12] sh, [15:13] se; top nibble = XCC
    std::map<unsigned, unsigned> per_cu, per_simd;
    unsigned late = 0;
    unsigned long long first = ~0ull;
    for (uint32_t q = 0; q < 16384; ++q)
      if (h[8 + 3 * q]) first = std::min(first, h[8 + 3 * q + 1]);
    for (uint32_t q = 0; q < 16384; ++q)
      if (h[8 + 3 * q]) {
        const unsigned hw = (unsigned)((h[8 + 3 * q] >> 32) & 0x0FFFFFFFu), xcc = (unsigned)(h[8 + 3 * q] >> 60);
        const unsigned cu = (xcc << 16) | (hw & 0xFF00u);
        per_cu[cu]++;
        per_simd[(cu << 2) | ((hw >> 4) & 3)]++;
        if (h[8 + 3 * q + 1] - first > 10000) late++;
        h[8 + 3 * q] &= 0xFFFFFFFFull;
      }
    unsigned mx_cu = 0, mx_simd = 0;
    for (auto& kv : per_cu) mx_cu = std::max(mx_cu, kv.second);
    for (auto& kv : per_simd) mx_simd = std::max(mx_simd, kv.second);
    fprintf(stderr, "[graph stamps, placement] CUs used %zu (max waves on one CU %u), SIMDs used %zu (max on one %u), waves starting > 100 us late: %u\n",
            per_cu.size(), mx_cu, per_simd.size(), mx_simd, late);
  }
  for (uint32_t q = 0; q < 16384; ++q)
    if (h[8 + 3 * q]) {
      cyc.push_back(h[8 + 3 * q]);
      hp.push_back(h[8 + 3 * q + 1]);
      rt.push_back(h[8 + 3 * q + 2]);
    }
  if (!cyc.empty()) {
    double csum = 0, rsum = 0;
    for (size_t i = 0; i < cyc.size(); ++i) {
      csum += (double)cyc[i];
      rsum += (double)rt[i];
    }
    // hp = start tick (100 MHz), rt = lifetime ticks
    unsigned long long t0 = ~0ull, t1 = 0;
    for (size_t i = 0; i < cyc.size(); ++i) {
      t0 = std::min(t0, hp[i]);
      t1 = std::max(t1, hp[i] + rt[i]);
    }
    std::vector<unsigned long long> st;
    for (size_t i = 0; i < cyc.size(); ++i) st.push_back(hp[i] - t0);
    std::sort(cyc.begin(), cyc.end());
    std::sort(st.begin(), st.end());
    std::sort(rt.begin(), rt.end());
    const size_t n = cyc.size();
    fprintf(stderr, "[graph stamps, last launch] queries %zu  cycles p50 %llu max %llu | wave lifetime us p50 %.1f p99 %.1f max %.1f | clock %.2f GHz | "
            "first start .. last end %.1f us; starts us: p25 %.1f p50 %.1f p75 %.1f p90 %.1f max %.1f\n", n, cyc[n / 2], cyc[n - 1],
            rt[n / 2] / 100.0, rt[n * 99 / 100] / 100.0, rt[n - 1] / 100.0, csum / rsum / 10.0, (t1 - t0) / 100.0, st[n / 4] / 100.0,
            st[n / 2] / 100.0, st[n * 3 / 4] / 100.0, st[n * 9 / 10] / 100.0, st[n - 1] / 100.0);
  }
  (void)hipMemset(d_stamps, 0, kStampWords * 8);
  return d_stamps;
}
#else
inline unsigned long long* graph_stamps_report(fvdb_graph*) { return nullptr; }
#endif

}  // namespace

extern "C" {

// =============================================================================================
// device-resident graph: structure
// =============================================================================================
int fvdb_graph_create(fvdb_store* s, fvdb_graph** out) {
  if (!s || !out) return FVDB_E_INVALID;
  *out = nullptr;
  fvdb_graph* g = new (std::nothrow) fvdb_graph();
  if (!g) return FVDB_E_OOM;
  g->store = s;
  *out = g;
  return FVDB_OK;
}

void fvdb_graph_destroy(fvdb_graph* g) {
  if (!g) return;
  (void)hipSetDevice(g->store->ctx->device);
  (void)hipStreamSynchronize(g->store->ctx->stream);
  delete g;
}

int fvdb_graph_configure(fvdb_graph* g, uint32_t max_connections, uint32_t max_connections_layer_0) {
  fvdb_ctx* ctx = g->store->ctx;
  if (max_connections == 0 || max_connections_layer_0 == 0) FAIL(ctx, FVDB_E_INVALID, "degree caps must be > 0");
  if (g->n != 0 && (max_connections != g->M || max_connections_layer_0 != g->M0))
    FAIL(ctx, FVDB_E_INVALID, "degree caps are fixed once the graph holds nodes");
  g->M = max_connections;
  g->M0 = max_connections_layer_0;
  return FVDB_OK;
}

int fvdb_graph_upload(fvdb_graph* g, uint32_t n, const uint32_t* levels, const uint8_t* deleted,
                      const uint32_t* slot_start, const uint32_t* adj, uint32_t entry_node) {
  g->mutations += 1;
  fvdb_ctx* ctx = g->store->ctx;
  if (n == 0 || n > g->store->rows || entry_node >= n) FAIL(ctx, FVDB_E_INVALID, "graph does not match the store");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> slot_of(n), del32(n), ubase(n);
  uint32_t slots = 0, urows = 0;
  for (uint32_t i = 0; i < n; ++i) {
    slot_of[i] = slots;
    ubase[i] = urows;
    slots += levels[i] + 1;
    urows += levels[i];
    del32[i] = deleted ? deleted[i] : 0;
  }
  uint32_t max0 = 0, maxU = 0;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t l = 0; l <= levels[i]; ++l) {
      const uint32_t c = slot_start[slot_of[i] + l + 1] - slot_start[slot_of[i] + l];
      if (c > 64) FAIL(ctx, FVDB_E_UNSUPPORTED, "neighbour list longer than 64");
      if (l == 0) max0 = std::max(max0, c);
      else maxU = std::max(maxU, c);
    }
  // fixed strides: the configured caps, or the longest list seen if that is longer (an installed graph may exceed them)
  const uint32_t stride0 = std::max(max0, g->M0) + 1, strideU = std::max(maxU, std::max(g->M, 1u)) + 1;
  // start over: the arrays are rebuilt whole (restore / bulk build / vacuum — O(n) operations themselves)
  DBuf* bufs[] = {&g->d_level, &g->d_deleted, &g->d_ubase, &g->d_adj0, &g->d_adjU, &g->d_dist0, &g->d_distU, &g->d_stamp0, &g->d_stampU};
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (DBuf* b : bufs) b->release();
  g->n = g->n_cap = g->u_rows = g->u_cap = 0;
  g->stride0 = stride0;
  g->strideU = strideU;
  int rc = reserve_nodes(g, n + n / 8 + 1024, urows + urows / 8 + 1024);
  if (rc) return rc;
  std::vector<uint32_t> adj0((size_t)n * stride0, 0u), adjU((size_t)std::max(urows, 1u) * strideU, 0u);
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t l = 0; l <= levels[i]; ++l) {
      const uint32_t a0 = slot_start[slot_of[i] + l], c = slot_start[slot_of[i] + l + 1] - a0;
      uint32_t* row = l == 0 ? &adj0[(size_t)i * stride0] : &adjU[(size_t)(ubase[i] + l - 1) * strideU];
      row[0] = c;
      for (uint32_t e = 0; e < c; ++e) {
        if (adj[a0 + e] >= n) FAIL(ctx, FVDB_E_INVALID, "neighbour index out of range");
        row[1 + e] = adj[a0 + e];
      }
    }
  HIPCHK(ctx, hipMemcpyAsync(g->d_adj0.p, adj0.data(), adj0.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (urows) HIPCHK(ctx, hipMemcpyAsync(g->d_adjU.p, adjU.data(), (size_t)urows * strideU * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(g->d_level.p, levels, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(g->d_deleted.p, del32.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(g->d_ubase.p, ubase.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  g->upload_bytes += adj0.size() * 4 + (size_t)urows * strideU * 4 + (size_t)n * 12;
  g->h_deleted.assign(n, 0);
  g->n_deleted = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (del32[i]) {
      g->h_deleted[i] = 1;
      g->n_deleted += 1;
    }
  g->h_level.assign(levels, levels + n);
  g->h_ubase = ubase;
  g->n = n;
  g->u_rows = urows;
  g->entry = entry_node;
  g->top_level = levels[entry_node];
  g->has_entry = true;
  g->uploaded = true;
  g->dist_valid = false;
  BuildState st{};
  st.has_entry = 1;
  st.entry = entry_node;
  st.entry_level = levels[entry_node];
  st.n_linked = n;
  rc = push_state(g, st);
  if (rc) return rc;
  for (auto& v : g->vis_B) v = 0;  // node count may have changed: re-size (and re-zero) the visited bitmaps
  return FVDB_OK;
}

int fvdb_graph_append_nodes(fvdb_graph* g, uint32_t first, uint32_t n_new, const uint32_t* levels) {
  g->mutations += 1;
  fvdb_ctx* ctx = g->store->ctx;
  if (n_new == 0) return FVDB_OK;
  if (first != g->n || (uint64_t)first + n_new > g->store->rows) FAIL(ctx, FVDB_E_INVALID, "nodes are appended in store-row order");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (g->n == 0 && g->stride0 == 0) {
    g->stride0 = std::max(g->M0, 1u) + 1;
    g->strideU = std::max(g->M, 1u) + 1;
  }
  uint32_t urows = g->u_rows;
  std::vector<uint32_t> ub(n_new);
  for (uint32_t i = 0; i < n_new; ++i) {
    ub[i] = urows;
    urows += levels[i];
  }
  int rc = reserve_nodes(g, first + n_new, urows);
  if (rc) return rc;
  HIPCHK(ctx, g->h_patch.ensure((size_t)n_new * 8));
  uint32_t* hp = (uint32_t*)g->h_patch.p;
  std::memcpy(hp, levels, (size_t)n_new * 4);
  std::memcpy(hp + n_new, ub.data(), (size_t)n_new * 4);
  HIPCHK(ctx, hipMemcpyAsync(g->d_level.as<uint32_t>() + first, hp, (size_t)n_new * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(g->d_ubase.as<uint32_t>() + first, hp + n_new, (size_t)n_new * 4, hipMemcpyHostToDevice, ctx->stream));
  // empty lists, clean flags and stamps for the new rows (rows only grow; a reclaiming vacuum writes fresh arrays)
  HIPCHK(ctx, hipMemsetAsync(g->d_adj0.as<uint32_t>() + (size_t)first * g->stride0, 0, (size_t)n_new * g->stride0 * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(g->d_deleted.as<uint32_t>() + first, 0, (size_t)n_new * 4, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(g->d_stamp0.as<uint32_t>() + first, 0, (size_t)n_new * 4, ctx->stream));
  if (urows > g->u_rows) {
    HIPCHK(ctx, hipMemsetAsync(g->d_adjU.as<uint32_t>() + (size_t)g->u_rows * g->strideU, 0, (size_t)(urows - g->u_rows) * g->strideU * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(g->d_stampU.as<uint32_t>() + g->u_rows, 0, (size_t)(urows - g->u_rows) * 4, ctx->stream));
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  g->upload_bytes += (uint64_t)n_new * 8;
  g->h_level.insert(g->h_level.end(), levels, levels + n_new);
  g->h_ubase.insert(g->h_ubase.end(), ub.begin(), ub.end());
  g->h_deleted.resize(first + n_new, 0);
  g->n = first + n_new;
  g->u_rows = urows;
  if (!g->d_state.p) {
    BuildState st{};
    rc = push_state(g, st);
    if (rc) return rc;
  }
  g->uploaded = true;
  for (auto& v : g->vis_B) v = 0;
  return FVDB_OK;
}

int fvdb_graph_set_lists(fvdb_graph* g, uint32_t n_lists, const uint32_t* nodes, const uint32_t* layers, const uint32_t* offsets,
                         const uint32_t* nbrs) {
  fvdb_ctx* ctx = g->store->ctx;
  g->mutations += 1;
  if (n_lists == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint32_t ps = 2 + 64;
  HIPCHK(ctx, g->h_patch.ensure((size_t)n_lists * (ps + 2) * 4));
  HIPCHK(ctx, g->s_patch.ensure((size_t)n_lists * (ps + 2) * 4));
  uint32_t* hp = (uint32_t*)g->h_patch.p;
  uint32_t* codes = hp + (size_t)n_lists * ps;
  uint32_t* owner = codes + n_lists;
  for (uint32_t i = 0; i < n_lists; ++i) {
    const uint32_t node = nodes[i], layer = layers[i], c = offsets[i + 1] - offsets[i];
    if (node >= g->n || layer > g->h_level[node]) FAIL(ctx, FVDB_E_NOT_FOUND, "no such (node, layer)");
    if (c + 1 > (layer == 0 ? g->stride0 : g->strideU)) FAIL(ctx, FVDB_E_UNSUPPORTED, "list longer than the row stride");
    const uint32_t code = layer == 0 ? node : (0x80000000u | (g->h_ubase[node] + layer - 1));
    hp[(size_t)i * ps] = code;
    hp[(size_t)i * ps + 1] = c;
    for (uint32_t e = 0; e < c; ++e) {
      if (nbrs[offsets[i] + e] >= g->n) FAIL(ctx, FVDB_E_INVALID, "neighbour index out of range");
      hp[(size_t)i * ps + 2 + e] = nbrs[offsets[i] + e];
    }
    codes[i] = code;
    owner[i] = node;
  }
  const size_t bytes = (size_t)n_lists * (ps + 2) * 4;
  HIPCHK(ctx, hipMemcpyAsync(g->s_patch.p, hp, bytes, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(graph_patch_kernel, dim3((n_lists + 3) / 4), dim3(256), 0, ctx->stream, g->s_patch.as<uint32_t>(), ps, n_lists,
                     g->d_adj0.as<uint32_t>(), g->stride0, g->d_adjU.as<uint32_t>(), g->strideU);
  HIPCHK(ctx, hipGetLastError());
  g->upload_bytes += bytes;
  if (g->dist_valid) {  // keep the edge distances of the rewritten rows current
    const uint32_t* dcodes = g->s_patch.as<uint32_t>() + (size_t)n_lists * ps;
    int rc = edge_dist(g, dcodes, dcodes + n_lists, n_lists, false);
    if (rc) return rc;
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}

int fvdb_graph_set_entry(fvdb_graph* g, uint32_t entry_node, uint32_t n_linked) {
  g->mutations += 1;
  fvdb_ctx* ctx = g->store->ctx;
  if (entry_node >= g->n || n_linked > g->n) FAIL(ctx, FVDB_E_INVALID, "no such node");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  g->entry = entry_node;
  g->top_level = g->h_level[entry_node];
  g->has_entry = true;
  BuildState st{};
  st.has_entry = 1;
  st.entry = entry_node;
  st.entry_level = g->top_level;
  st.n_linked = n_linked;
  g->upload_bytes += 16;
  return push_state(g, st);
}

int fvdb_graph_entry(fvdb_graph* g, uint32_t* entry_node, uint32_t* n_nodes) {
  if (entry_node) *entry_node = g->has_entry ? g->entry : FVDB_NO_ROW;
  if (n_nodes) *n_nodes = g->n;
  return FVDB_OK;
}

uint64_t fvdb_graph_upload_bytes(fvdb_graph* g) { return g->upload_bytes; }

int fvdb_graph_download(fvdb_graph* g, uint32_t* slot_start, uint32_t* adj, uint64_t adj_cap, uint64_t* n_edges) {
  fvdb_ctx* ctx = g->store->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> a0((size_t)g->n * g->stride0), aU((size_t)std::max(g->u_rows, 1u) * g->strideU);
  if (g->n) HIPCHK(ctx, hipMemcpyAsync(a0.data(), g->d_adj0.p, a0.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (g->u_rows) HIPCHK(ctx, hipMemcpyAsync(aU.data(), g->d_adjU.p, (size_t)g->u_rows * g->strideU * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t e = 0;
  uint32_t slot = 0;
  for (uint32_t i = 0; i < g->n; ++i)
    for (uint32_t l = 0; l <= g->h_level[i]; ++l, ++slot) {
      const uint32_t* row = l == 0 ? &a0[(size_t)i * g->stride0] : &aU[(size_t)(g->h_ubase[i] + l - 1) * g->strideU];
      if (slot_start) slot_start[slot] = (uint32_t)e;
      if (adj) {
        if (e + row[0] > adj_cap) FAIL(ctx, FVDB_E_INVALID, "adjacency buffer too small");
        std::memcpy(adj + e, row + 1, (size_t)row[0] * 4);
      }
      e += row[0];
    }
  if (slot_start) slot_start[slot] = (uint32_t)e;
  if (n_edges) *n_edges = e;
  return FVDB_OK;
}

int fvdb_graph_set_deleted(fvdb_graph* g, uint32_t node, int deleted) {
  g->mutations += 1;
  fvdb_ctx* ctx = g->store->ctx;
  if (!g->uploaded || node >= g->n) FAIL(ctx, FVDB_E_NOT_FOUND, "no such node");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint32_t v = deleted ? 1u : 0u;
  if (g->h_deleted[node] != (uint8_t)v) {
    g->n_deleted += v ? 1 : -1;
    g->h_deleted[node] = (uint8_t)v;
  }
  HIPCHK(ctx, hipMemcpyAsync(g->d_deleted.as<uint32_t>() + node, &v, 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  g->upload_bytes += 4;
  return FVDB_OK;
}

// =============================================================================================
// device-resident graph: construction (HNSWIndex::insert, src/hnsw/core.rs:226-378)
// =============================================================================================
int fvdb_graph_insert_linked(fvdb_graph* g, uint32_t first, uint32_t n, uint32_t ef_construction, int mode, uint32_t* n_done,
                             fvdb_graph_insert_stats* stats) {
  fvdb_store* s = g->store;
  fvdb_ctx* ctx = s->ctx;
  g->mutations += 1;
  if (n_done) *n_done = 0;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n == 0) return FVDB_OK;
  if (!g->uploaded || (uint64_t)first + n > g->n) FAIL(ctx, FVDB_E_INVALID, "append the nodes first");
  if (g->M == 0 || g->M0 == 0) FAIL(ctx, FVDB_E_INVALID, "fvdb_graph_configure first");
  if (g->M > 63 || g->M0 > 63 || g->stride0 > 64 || g->strideU > 64)
    FAIL(ctx, FVDB_E_UNSUPPORTED, "device insert: neighbour lists of at most 63 entries");
  if (ef_construction == 0 || ef_construction > 512) FAIL(ctx, FVDB_E_UNSUPPORTED, "device insert: ef_construction in 1..512");
  if (s->dpad > 1024) FAIL(ctx, FVDB_E_UNSUPPORTED, "device insert: at most 1024 dimensions");
  if (g->n >= 0x80000000u) FAIL(ctx, FVDB_E_UNSUPPORTED, "device insert: node index needs 31 bits");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // plan — LDS: `visited` (a bitmap over all nodes while that fits, a hashed set beyond) + fixed tables; the restated
  // candidates heap gets what is left (<= 4096 slots)
  const InsertPlan plan = insert_plan(g, ef_construction);
  if (plan.repr == 0) FAIL(ctx, FVDB_E_UNSUPPORTED, plan.why);
  int rc;
  BuildState st{};
  if ((rc = ensure_edge_dist(g)) || (rc = reset_build_state(g, first, &st))) return rc;
  static const BuildKnobs knobs{};
  BuildSchedule sched{knobs, knobs.mode ? knobs.mode : mode, first, n};
  // launch: the batch logs, the kernels for this dimension and form of `visited`, then group after group
  HIPCHK(ctx, g->d_spec.ensure((size_t)sched.Kmax * kSpecWords * 4));
  HIPCHK(ctx, g->d_elog.ensure((size_t)sched.Kmax * kBuildLayers * kLogWords * 4));
  HIPCHK(ctx, g->d_chg.ensure((size_t)kChgCap * 4 * 4));
  if (n >= 8)  // (a call that cannot speculate skips this)
    HIPCHK(ctx, hipMemsetAsync(g->d_spec.p, 0, (size_t)sched.Kmax * kSpecWords * 4, ctx->stream));  // no stale "usable" flags
  const BuildKernels kernels = build_kernels(s, plan.repr == 2);
  HIPCHK(ctx, hipFuncSetAttribute((const void*)kernels.commit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes));
  HIPCHK(ctx, hipFuncSetAttribute((const void*)kernels.search, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes));
  BuildView v = build_view(g, ef_construction, plan);
  build_stamps_begin(g, &v);
  uint32_t done = 0, launches = 0;
  while (done < n) {
    const BuildGroup grp = sched.next(done);
    v.exact_first = grp.exact_first;
    launch_group(g, kernels, v, plan.lds_bytes, sched, grp);
    HIPCHK(ctx, hipGetLastError());
    if ((rc = pull_state(g, &st))) return rc;
    launches += grp.speculate ? 2 * grp.count : 1;
    sched.update(grp, done, st);
    if (st.cursor == done && st.status == 0) FAIL(ctx, FVDB_E_HIP, "device insert made no progress");
    done = st.cursor;
    if (st.status) break;
  }
  build_stamps_print(g, st, done);
  report_insert(plan, st);
  fold_insert(g, plan, st, launches, n_done, stats);
  return FVDB_OK;
}

int fvdb_graph_set_insert_visited(fvdb_graph* g, int mode, uint32_t table_slots) {
  fvdb_ctx* ctx = g->store->ctx;
  if (mode < 0 || mode > 2) FAIL(ctx, FVDB_E_INVALID, "insert visited mode: 0 auto, 1 bitmap, 2 hashed");
  if (table_slots != 0 && (table_slots < 256 || table_slots > 32768 || (table_slots & (table_slots - 1)) != 0))
    FAIL(ctx, FVDB_E_INVALID, "insert visited table: a power of two in 256..32768 slots (0 = default)");
  g->ins_vis_mode = mode;
  g->ins_vis_slots = table_slots;
  return FVDB_OK;
}

int fvdb_graph_insert_info(fvdb_graph* g, uint32_t ef_construction, fvdb_graph_insert_info_t* out) {
  fvdb_ctx* ctx = g->store->ctx;
  if (!out) FAIL(ctx, FVDB_E_INVALID, "insert info: no output");
  if (ef_construction == 0 || ef_construction > 512) FAIL(ctx, FVDB_E_UNSUPPORTED, "device insert: ef_construction in 1..512");
  const InsertPlan p = insert_plan(g, ef_construction);
  std::memset(out, 0, sizeof(*out));
  out->mode = (uint32_t)g->ins_vis_mode;
  out->representation = p.repr;
  out->table_slots = p.slots;
  out->cand_cap = p.cand_cap;
  out->lds_bytes = p.lds_bytes;
  out->bitmap_max_nodes = p.bitmap_max_nodes;
  out->visited_peak = g->ins_vis_peak;
  out->hashed_inserts = g->ins_hashed;
  out->visited_overflows = g->ins_vis_over;
  out->visited_searches = g->ins_vis_searches;
  out->visited_entries = g->ins_vis_entries;
  return FVDB_OK;
}

int fvdb_graph_search_info(fvdb_graph* g, uint32_t B, uint32_t ef, fvdb_graph_search_info_t* out) {
  if (!g) return FVDB_E_INVALID;
  fvdb_ctx* ctx = g->store->ctx;
  if (!out) FAIL(ctx, FVDB_E_INVALID, "search info: no output");
  if (!g->uploaded || !g->has_entry) FAIL(ctx, FVDB_E_INVALID, "graph not uploaded");
  if (ef == 0 || ef > 4096) FAIL(ctx, FVDB_E_UNSUPPORTED, "ef must be in 1..4096");
  std::lock_guard<std::mutex> lk(g->mu);
  SearchPlan sp{};
  if (int rc = search_plan(g, ctx, B, ef, &sp)) return rc;
  std::memset(out, 0, sizeof(*out));
  out->visited = sp.bytemap ? FVDB_GRAPH_VISITED_BYTES : FVDB_GRAPH_VISITED_BITS;
  out->kernel = sp.fast ? FVDB_GRAPH_KERNEL_SORTED : FVDB_GRAPH_KERNEL_HEAPS;
  out->nb128 = sp.nb128;
  out->rows_per_round = (uint32_t)sp.R;
  out->nearest_in_registers = sp.rh ? 1u : 0u;
  out->tcap = sp.tcap;
  out->cand_cap = sp.cand_cap;
  out->spill_cap = sp.spill_cap;
  out->lds_bytes = (uint32_t)sp.lds;
  out->visited_bytes = (uint64_t)B * sp.vstride;
  return FVDB_OK;
}

// =============================================================================================
// device-resident graph traversal
// =============================================================================================
int fvdb_graph_search_dev(fvdb_graph* g, const float* q_dev, uint32_t B, uint32_t k, uint32_t ef,
                          uint32_t* out_nodes_dev, float* out_dist_dev, uint32_t* out_counts_dev,
                          uint32_t* out_status_dev) {
  return fvdb_graph_search_dev_slot(g, nullptr, 0, q_dev, B, k, ef, out_nodes_dev, out_dist_dev, out_counts_dev,
                                    out_status_dev);
}

// The traversal, unmasked (mask == nullptr: the graph's own flags) or under an allow-set mask, whose flags then stand
// for `deleted` in the one GraphView the kernels are handed.
static int graph_search_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, const fvdb_mask* mask, const float* q_dev, uint32_t B,
                             uint32_t k, uint32_t ef, uint32_t* out_nodes_dev, float* out_dist_dev, uint32_t* out_counts_dev,
                             uint32_t* out_status_dev) {
  fvdb_store* s = g->store;
  fvdb_ctx* ctx = on ? on : s->ctx;
  if (slot >= fvdb_graph::kSlots) FAIL(ctx, FVDB_E_INVALID, "slot out of range");
  if (mask && mask->graph != g) FAIL(ctx, FVDB_E_INVALID, "mask of another graph");
  if (mask && mask->stamp != g->mutations) FAIL(ctx, FVDB_E_INVALID, "stale mask: the graph changed after the mask was created");
  if (on && on->device != s->ctx->device) FAIL(ctx, FVDB_E_INVALID, "context of another device");
  if (s->d != s->dpad && slot != 0) FAIL(ctx, FVDB_E_UNSUPPORTED, "padded dimensions use slot 0 only");
  if (!g->uploaded || !g->has_entry) FAIL(ctx, FVDB_E_INVALID, "graph not uploaded");
  if (k == 0 || ef == 0 || ef > 4096) FAIL(ctx, FVDB_E_UNSUPPORTED, "ef must be in 1..4096");
  if (B == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> lk(g->mu);
  const float* qd = q_dev;
  if (s->d != s->dpad) {
    HIPCHK(ctx, g->s_q.ensure((size_t)B * s->dpad * 4));
    hipLaunchKernelGGL(graph_pad_rows_kernel, dim3(cdiv((uint64_t)B * s->dpad, 256)), dim3(256), 0, ctx->stream, q_dev, s->d,
                       s->dpad, (uint64_t)B, g->s_q.as<float>());
    qd = g->s_q.as<float>();
  }
  SearchPlan sp{};
  int rc;
  if ((rc = search_plan(g, ctx, B, ef, &sp)) || (rc = search_scratch(g, ctx, slot, B, &sp))) return rc;
  if (sp.lds > 48 * 1024)
    HIPCHK(ctx, hipFuncSetAttribute(sp.fast ? (const void*)sp.fast : (const void*)sp.exact, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp.lds));
  if (!g->d_counters.p) {
    HIPCHK(ctx, g->d_counters.ensure(32));
    HIPCHK(ctx, hipMemsetAsync(g->d_counters.p, 0, 32, ctx->stream));
  }
  const uint32_t* deleted = mask ? mask->flags.as<uint32_t>() : g->d_deleted.as<uint32_t>();
  const uint32_t any_deleted = mask ? 1u : (g->n_deleted ? 1u : 0u);
  const GraphView gv{s->data, g->d_level.as<uint32_t>(), deleted, g->d_adj0.as<uint32_t>(), g->d_ubase.as<uint32_t>(),
                     g->d_adjU.as<uint32_t>(), g->stride0, g->strideU, g->n, s->dpad, g->entry, g->top_level, any_deleted,
                     g->d_counters.as<unsigned long long>(), graph_stamps_report(g)};
  DevEvent* ev = nullptr;
  if (s->ctx->profiling) {  // the store's context carries the switch, whichever stream the launch goes to
    ev = g->kev[g->kev_n & 63];
    (void)ev[0].create();
    (void)ev[1].create();
    (void)hipEventRecord(ev[0], ctx->stream);
  }
  if (sp.fast)
    hipLaunchKernelGGL(sp.fast, dim3(cdiv(B, 4)), dim3(256), sp.lds, ctx->stream, gv, qd, B, k, ef, sp.cand_cap, sp.wave_lds,
                       g->s_visited[slot].as<uint8_t>(), sp.vstride, sp.words, g->s_touched[slot].as<uint32_t>(), sp.tcap, out_nodes_dev,
                       out_dist_dev, out_counts_dev, out_status_dev, (HItem*)g->s_spill[slot].p, sp.spill_cap);
  else  // (lane-0 heaps stay in LDS: no spill)
    hipLaunchKernelGGL(sp.exact, dim3(B), dim3(64), sp.lds, ctx->stream, gv, qd, B, k, ef, sp.cand_cap, g->s_visited[slot].as<uint32_t>(),
                       sp.vstride / 4, g->s_touched[slot].as<uint32_t>(), sp.tcap, out_nodes_dev, out_dist_dev, out_counts_dev,
                       out_status_dev, sp.rh ? (HItem*)g->s_spill[slot].p : nullptr, sp.rh ? sp.spill_cap : 0u);
  if (ev) {
    (void)hipEventRecord(ev[1], ctx->stream);
    g->kev_n += 1;
  }
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

int fvdb_graph_search_dev_slot(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, const float* q_dev, uint32_t B, uint32_t k,
                               uint32_t ef, uint32_t* out_nodes_dev, float* out_dist_dev, uint32_t* out_counts_dev,
                               uint32_t* out_status_dev) {
  return graph_search_slot(g, on, slot, nullptr, q_dev, B, k, ef, out_nodes_dev, out_dist_dev, out_counts_dev, out_status_dev);
}

int fvdb_graph_search_dev_slot_masked(fvdb_graph* g, fvdb_ctx* on, uint32_t slot, fvdb_mask* mask, const float* q_dev, uint32_t B,
                                      uint32_t k, uint32_t ef, uint32_t* out_nodes_dev, float* out_dist_dev,
                                      uint32_t* out_counts_dev, uint32_t* out_status_dev) {
  if (!g) return FVDB_E_INVALID;
  if (!mask) FAIL(on ? on : g->store->ctx, FVDB_E_INVALID, "null mask");
  return graph_search_slot(g, on, slot, mask, q_dev, B, k, ef, out_nodes_dev, out_dist_dev, out_counts_dev, out_status_dev);
}

int fvdb_graph_tie_restarts(fvdb_graph* g, uint64_t* queries, uint64_t* searched_again) {
  fvdb_ctx* ctx = g->store->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipDeviceSynchronize());  // searches may run on several streams
  unsigned long long c[4] = {0, 0, 0, 0};
  if (g->d_counters.p) HIPCHK(ctx, hipMemcpy(c, g->d_counters.p, 32, hipMemcpyDeviceToHost));
  if (queries) *queries = g->tot_queries + c[3];
  if (searched_again) *searched_again = g->tot_again + c[2];
  return FVDB_OK;
}

int fvdb_graph_kernel_times(fvdb_graph* g, float* ms_sum, uint32_t* launches, uint64_t* rows_scored, uint64_t* hops) {
  fvdb_ctx* ctx = g->store->ctx;
  *ms_sum = 0.0f;
  *launches = 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  unsigned long long c[4] = {0, 0, 0, 0};  // rows scored, hops, queries searched again with the restated heaps, queries
  if (g->d_counters.p) {
    HIPCHK(ctx, hipMemcpy(c, g->d_counters.p, 32, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemset(g->d_counters.p, 0, 32));
  }
  g->tot_queries += c[3];
  g->tot_again += c[2];
  if (getenv("FVDB_GRAPH_DEBUG"))
    fprintf(stderr, "[graph traversal] %llu queries, %llu searched again with the restated heaps (equal distances)\n", c[3], c[2]);
  if (rows_scored) *rows_scored = c[0];
  if (hops) *hops = c[1];
  const uint32_t n = std::min<uint32_t>(g->kev_n, 64);
  for (uint32_t i = 0; i < n; ++i) {
    const DevEvent* ev = g->kev[(g->kev_n - 1 - i) & 63];
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) {
      *ms_sum += ms;
      *launches += 1;
    }
  }
  g->kev_n = 0;
  return FVDB_OK;
}

}  // extern "C"

// =============================================================================================
// device-resident graph: maintenance (HNSWIndex::vacuum, src/hnsw/operations.rs:176-200; kernels_graph_maint.h)
// =============================================================================================
namespace {

uint32_t prune_grid(const fvdb_ctx* ctx, uint32_t rows) { return std::max(1u, std::min<uint32_t>(cdiv(rows, 4), (uint32_t)ctx->num_cus * 8u)); }

// the fresh arrays of a reclaiming vacuum: all allocated before the first change, gone again if one cannot be had
struct FreshGraph {
  DBuf level, deleted, ubase, adj0, adjU, dist0, distU, stamp0, stampU, rows;
};

struct VacuumJob {
  fvdb_graph* g;
  fvdb_store* s;
  fvdb_ctx* ctx;
  hipStream_t st;
  bool keep_rows;
  uint32_t n, u_rows, n_wg;
  uint32_t n_out, u_out;  // the survivors by the host's copy of the flags, and their upper rows
  uint32_t n_cap, u_cap;
  StageTimer<6> ev;
  // scratch: [new_index n | src_node n | u_src or owner u_rows | wg_nodes n_wg | wg_urows n_wg | totals 2] words, counters
  DBuf scratch, counters;
  uint32_t *new_index = nullptr, *src_node = nullptr, *u_aux = nullptr, *wg_nodes = nullptr, *wg_urows = nullptr, *totals = nullptr;
  FreshGraph f;
  GmPrune p0{}, pU{};
  uint64_t host_bytes = 0;
  unsigned long long h_cnt[4] = {0, 0, 0, 0};
  unsigned long long* cnt() const { return (unsigned long long*)counters.p; }
  int alloc_scratch(), scan_in_place(), alloc_fresh(), scan_reclaim(), prune_move(), adopt();  // the stages, in this order
};

int VacuumJob::alloc_scratch() {
  HIPCHK(ctx, ev.create());
  HIPCHK(ctx, scratch.ensure(((size_t)2 * n + u_rows + 2 * (size_t)n_wg + 2) * 4));
  HIPCHK(ctx, counters.ensure(32));
  new_index = scratch.as<uint32_t>();
  src_node = new_index + n;
  u_aux = src_node + n;
  wg_nodes = u_aux + u_rows;
  wg_urows = wg_nodes + n_wg;
  totals = wg_urows + n_wg;
  HIPCHK(ctx, hipMemsetAsync(counters.p, 0, 32, st));
  return FVDB_OK;
}

// keep_rows: nothing moves, the lists are pruned in place
int VacuumJob::scan_in_place() {
  const uint32_t* d_deleted = g->d_deleted.as<uint32_t>();
  n_out = n;
  u_out = u_rows;
  HIPCHK(ctx, ev.mark(0, st));
  if (u_rows)
    hipLaunchKernelGGL(gm_owner_kernel, dim3(n_wg), dim3(256), 0, st, g->d_level.as<uint32_t>(), g->d_ubase.as<uint32_t>(), n, u_rows, u_aux);
  HIPCHK(ctx, ev.mark(1, st));
  HIPCHK(ctx, ev.mark(2, st));
  p0 = GmPrune{g->d_adj0.as<uint32_t>(), g->d_dist0.as<float>(), g->d_adj0.as<uint32_t>(), g->d_dist0.as<float>(), g->stride0, n, n,
               nullptr, nullptr, 1u, d_deleted, n, nullptr, nullptr, nullptr, cnt()};
  pU = GmPrune{g->d_adjU.as<uint32_t>(), g->d_distU.as<float>(), g->d_adjU.as<uint32_t>(), g->d_distU.as<float>(), g->strideU, u_rows, u_rows,
               nullptr, u_aux, 1u, d_deleted, n, nullptr, nullptr, nullptr, cnt()};
  return FVDB_OK;
}

// the fresh arrays, exactly sized (the capacities carry the growth slack already); every allocation precedes the first change
int VacuumJob::alloc_fresh() {
  n_cap = n_out + n_out / 8 + 1024;
  u_cap = u_out + u_out / 8 + 1024;
  const size_t nc = n_cap, uc = u_cap;
  const struct {
    DBuf* b;
    size_t bytes;
  } want[10] = {{&f.level, nc * 4},  {&f.deleted, nc * 4}, {&f.ubase, nc * 4},
                {&f.adj0, nc * g->stride0 * 4}, {&f.adjU, uc * g->strideU * 4},
                {&f.dist0, nc * g->stride0 * 4}, {&f.distU, uc * g->strideU * 4},
                {&f.stamp0, nc * 4}, {&f.stampU, uc * 4},
                {&f.rows, nc * s->row_bytes()}};
  for (const auto& w : want) {
    const hipError_t e = w.b->exact(std::max<size_t>(w.bytes, 256));
    if (e != hipSuccess)
      FAIL(ctx, e == hipErrorOutOfMemory ? FVDB_E_OOM : FVDB_E_HIP, "graph vacuum: no memory for the compacted copy (graph unchanged)");
  }
  for (int b = 0; b < 9; ++b) HIPCHK(ctx, hipMemsetAsync(want[b].b->p, 0, want[b].b->cap, st));  // (the store's rows are written whole)
  return FVDB_OK;
}

// reclaiming: the survivors are counted and mapped to their new indices, the lists pruned into the fresh arrays
int VacuumJob::scan_reclaim() {
  const uint32_t* d_deleted = g->d_deleted.as<uint32_t>();
  // stage 1a: survivors and their upper rows, counted on the device and checked against the host's copy of the flags
  HIPCHK(ctx, ev.mark(0, st));
  hipLaunchKernelGGL(gm_count_kernel, dim3(n_wg), dim3(256), 0, st, d_deleted, g->d_level.as<uint32_t>(), n, wg_nodes, wg_urows);
  hipLaunchKernelGGL(block_excl_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, wg_nodes, n_wg, totals);
  hipLaunchKernelGGL(block_excl_scan_kernel<uint32_t>, dim3(1), dim3(1024), 0, st, wg_urows, n_wg, totals + 1);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, ev.mark(1, st));
  uint32_t h_tot[2] = {0, 0};
  HIPCHK(ctx, hipMemcpyAsync(h_tot, totals, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  host_bytes += 8;
  if (h_tot[0] != n_out || h_tot[1] != u_out) FAIL(ctx, FVDB_E_HIP, "graph vacuum: the device's deleted flags differ from the host's copy");
  int rc = alloc_fresh();
  if (rc) return rc;
  // stage 1b: the maps, and level / upper-row base of every survivor at its new index
  HIPCHK(ctx, ev.mark(2, st));
  hipLaunchKernelGGL(gm_map_kernel, dim3(n_wg), dim3(256), 0, st, d_deleted, g->d_level.as<uint32_t>(), g->d_ubase.as<uint32_t>(), n, wg_nodes,
                     wg_urows, n_out, u_out, new_index, src_node, u_aux, f.level.as<uint32_t>(), f.ubase.as<uint32_t>());
  HIPCHK(ctx, hipGetLastError());
  p0 = GmPrune{g->d_adj0.as<uint32_t>(), g->d_dist0.as<float>(), f.adj0.as<uint32_t>(), f.dist0.as<float>(), g->stride0, n_out, n,
               src_node, nullptr, 0u, d_deleted, n, new_index, g->d_stamp0.as<uint32_t>(), f.stamp0.as<uint32_t>(), cnt()};
  pU = GmPrune{g->d_adjU.as<uint32_t>(), g->d_distU.as<float>(), f.adjU.as<uint32_t>(), f.distU.as<float>(), g->strideU, u_out, u_rows,
               u_aux, nullptr, 0u, d_deleted, n, new_index, g->d_stampU.as<uint32_t>(), f.stampU.as<uint32_t>(), cnt()};
  return FVDB_OK;
}

int VacuumJob::prune_move() {
  // stage 2: prune + remap, one wave per destination row
  HIPCHK(ctx, ev.mark(3, st));
  hipLaunchKernelGGL(gm_edges_kernel, dim3(prune_grid(ctx, n)), dim3(256), 0, st, g->d_adj0.as<uint32_t>(), g->stride0, n, cnt());
  if (u_rows)
    hipLaunchKernelGGL(gm_edges_kernel, dim3(prune_grid(ctx, u_rows)), dim3(256), 0, st, g->d_adjU.as<uint32_t>(), g->strideU, u_rows,
                       cnt());
  if (p0.rows) hipLaunchKernelGGL(gm_prune_kernel, dim3(prune_grid(ctx, p0.rows)), dim3(256), 0, st, p0);
  if (pU.rows) hipLaunchKernelGGL(gm_prune_kernel, dim3(prune_grid(ctx, pU.rows)), dim3(256), 0, st, pU);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, ev.mark(4, st));
  // stage 3: store rows, one wave per destination row
  if (!keep_rows && n_out) {
    if (s->f16())  // a half row is dpad * 2 bytes: whole 8-byte chunks
      hipLaunchKernelGGL(gm_move_kernel<float2>, dim3(cdiv(n_out, 4)), dim3(256), 0, st, src_node, (const float2*)s->data, n, s->dpad / 4, n_out, (float2*)f.rows.p);
    else
      hipLaunchKernelGGL(gm_move_kernel<float4>, dim3(cdiv(n_out, 4)), dim3(256), 0, st, src_node, (const float4*)s->data, n, s->dpad / 4, n_out, (float4*)f.rows.p);
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, ev.mark(5, st));
  HIPCHK(ctx, hipMemcpyAsync(h_cnt, counters.p, 32, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  host_bytes += 32;
  return FVDB_OK;
}

// the graph and the store take the compacted arrays; the host's bookkeeping follows them
int VacuumJob::adopt() {
  std::swap(g->d_level, f.level);
  std::swap(g->d_deleted, f.deleted);
  std::swap(g->d_ubase, f.ubase);
  std::swap(g->d_adj0, f.adj0);
  std::swap(g->d_adjU, f.adjU);
  std::swap(g->d_dist0, f.dist0);
  std::swap(g->d_distU, f.distU);
  std::swap(g->d_stamp0, f.stamp0);
  std::swap(g->d_stampU, f.stampU);
  // the store adopts the compacted rows: scorers read store->data at every launch
  std::swap(s->rows_buf, f.rows);
  s->data = s->rows_buf.p;
  s->cap = n_cap;
  s->rows = n_out;
  f = FreshGraph{};  // the old arrays go now, not when the job returns: the host bookkeeping below allocates
  std::vector<uint32_t> lv(n_out), ub(n_out);
  uint32_t w = 0, u = 0, entry = 0;
  bool entry_alive = false;
  for (uint32_t i = 0; i < n; ++i) {
    if (g->h_deleted[i]) continue;
    if (g->has_entry && i == g->entry) {
      entry = w;
      entry_alive = true;
    }
    lv[w] = g->h_level[i];
    ub[w] = u;
    u += lv[w];
    w += 1;
  }
  g->h_level.swap(lv);
  g->h_ubase.swap(ub);
  g->h_deleted.assign(n_out, 0);
  g->n_deleted = 0;
  g->n = n_out;
  g->n_cap = n_cap;
  g->u_rows = u_out;
  g->u_cap = u_cap;
  g->has_entry = entry_alive;
  g->entry = entry_alive ? entry : 0;
  g->top_level = entry_alive ? g->h_level[entry] : 0;
  for (auto& v : g->vis_B) v = 0;  // visited maps are sized by the node count
  BuildState bs{};
  bs.has_entry = entry_alive ? 1u : 0u;
  bs.entry = g->entry;
  bs.entry_level = g->top_level;
  bs.n_linked = n_out;
  host_bytes += sizeof(BuildState);
  return push_state(g, bs);
}

}  // namespace

extern "C" int fvdb_graph_vacuum(fvdb_graph* g, uint32_t flags, uint64_t* removed) {
  if (!g) return FVDB_E_INVALID;
  fvdb_store* s = g->store;
  fvdb_ctx* ctx = s->ctx;
  if (removed) *removed = 0;
  if (flags & ~FVDB_VACUUM_KEEP_ROWS) FAIL(ctx, FVDB_E_INVALID, "graph vacuum: unknown flag");
  if (!g->uploaded || g->n == 0) FAIL(ctx, FVDB_E_INVALID, "graph vacuum: no device graph");
  const bool keep_rows = (flags & FVDB_VACUUM_KEEP_ROWS) != 0;
  if (!keep_rows && s->rows != g->n) FAIL(ctx, FVDB_E_INVALID, "graph vacuum: the graph does not cover the store");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipDeviceSynchronize());  // searches of other slots run on streams of their own
  const auto t0 = std::chrono::steady_clock::now();
  fvdb_graph_maintenance_info_t info{};
  const uint32_t n = g->n, u_rows = g->u_rows;
  info.nodes_in = info.nodes_out = n;
  // the survivors by the host's copy of the flags: new index = undeleted nodes before it
  uint32_t n_out = 0, u_out = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (!g->h_deleted[i]) {
      n_out += 1;
      u_out += g->h_level[i];
    }
  if (n_out == n) {  // nothing is deleted: nothing to prune, nothing to move
    g->m_info = info;
    return FVDB_OK;
  }
  VacuumJob J{g, s, ctx, ctx->stream, keep_rows, n, u_rows, cdiv(n, 256), n_out, u_out, g->n_cap, g->u_cap};
  int rc = J.alloc_scratch();
  if (rc) return rc;
  rc = keep_rows ? J.scan_in_place() : J.scan_reclaim();
  if (rc) return rc;
  rc = J.prune_move();
  if (rc) return rc;
  // stage 4: bookkeeping
  g->mutations += 1;
  info.edges_in = J.h_cnt[0];
  info.edges_out = J.h_cnt[1];
  if (keep_rows) {
    if (removed) *removed = J.h_cnt[2];
  } else {
    info.nodes_out = n_out;
    info.rows_reclaimed = n - n_out;
    info.bytes_reclaimed = (uint64_t)(n - n_out) * ((uint64_t)s->row_bytes() + (uint64_t)g->stride0 * 8 + 16) +
                           (uint64_t)(u_rows - u_out) * ((uint64_t)g->strideU * 8 + 4);
    info.move_bytes = 2ull * n_out * s->row_bytes();
    rc = J.adopt();
    if (removed) *removed = n - n_out;
    if (rc) return rc;
  }
  info.host_bytes = J.host_bytes;
  info.ms_scan = J.ev.ms(0, 1) + (keep_rows ? 0.0f : J.ev.ms(2, 3));
  info.ms_prune = J.ev.ms(3, 4);
  info.ms_move = J.ev.ms(4, 5);
  info.ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  g->m_info = info;
  return FVDB_OK;
}

extern "C" int fvdb_graph_maintenance_info(fvdb_graph* g, fvdb_graph_maintenance_info_t* out) {
  if (!g || !out) return FVDB_E_INVALID;
  *out = g->m_info;
  return FVDB_OK;
}

// =============================================================================================
// device-resident graph: health (kernels_graph_health.h).  Read-only: no flag, list, stamp, visited
// map or counter of the graph is written, and `mutations` does not move.
// =============================================================================================
namespace {

struct HealthJob {
  fvdb_graph* g;
  fvdb_ctx* ctx;
  hipStream_t st;
  uint32_t n;
  bool want_reach, want_comp;
  size_t bitmap_bytes, node_bytes, head_bytes;
  struct Scratch {  // head: [counters | state] words; bitmap and label become the graph's per-node results
    DBuf head, list, parent, size, bitmap, label;
  } sc;
  StageTimer<2> ev;
  unsigned long long* counters = nullptr;
  uint32_t *state = nullptr, *h_words = nullptr;
  GhGraph gg{};
  bool has_entry = false;
  uint32_t entry = kGhNone;
  uint32_t launches = 0, reach_launches = 0, host_syncs = 0, rounds0 = 0, reached = 0;
  int alloc(fvdb_graph_health_t* out), census(), reach(), components(), report(fvdb_graph_health_t* out);  // the stages
};

// every allocation precedes the first launch
int HealthJob::alloc(fvdb_graph_health_t* out) {
  HIPCHK(ctx, sc.head.ensure(head_bytes));
  if (want_reach) {
    HIPCHK(ctx, sc.list.ensure(node_bytes));
    HIPCHK(ctx, sc.bitmap.ensure(bitmap_bytes));
  }
  if (want_comp) {
    HIPCHK(ctx, sc.parent.ensure(node_bytes));
    HIPCHK(ctx, sc.size.ensure(node_bytes));
    HIPCHK(ctx, sc.label.ensure(node_bytes));
  }
  HIPCHK(ctx, g->h_state.ensure(std::max(head_bytes, sizeof(BuildState))));
  out->scratch_bytes = sc.head.cap + sc.list.cap + sc.parent.cap + sc.size.cap + sc.bitmap.cap + sc.label.cap;
  HIPCHK(ctx, ev.create());
  counters = sc.head.as<unsigned long long>();
  state = (uint32_t*)(counters + kGhCounters);
  h_words = (uint32_t*)g->h_state.p;
  gg = GhGraph{g->d_adj0.as<uint32_t>(), g->d_adjU.as<uint32_t>(), g->d_level.as<uint32_t>(), g->d_deleted.as<uint32_t>(),
               g->d_ubase.as<uint32_t>(), n, g->u_rows, g->stride0, g->strideU};
  has_entry = g->has_entry && g->entry < n;
  entry = has_entry ? g->entry : kGhNone;
  return FVDB_OK;
}

int HealthJob::census() {
  HIPCHK(ctx, ev.mark(0, st));
  HIPCHK(ctx, hipMemsetAsync(sc.head.p, 0, head_bytes, st));
  hipLaunchKernelGGL(gh_census_kernel, dim3(prune_grid(ctx, n)), dim3(256), 0, st, gg, counters);
  launches += 1;
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// reach: layer by layer from the entry point's level, each layer closed step by step
int HealthJob::reach() {
  uint32_t* bitmap = sc.bitmap.as<uint32_t>();
  uint32_t* list = sc.list.as<uint32_t>();
  HIPCHK(ctx, hipMemsetAsync(bitmap, 0, bitmap_bytes, st));
  if (!has_entry) return FVDB_OK;
  hipLaunchKernelGGL(gh_seed_kernel, dim3(1), dim3(64), 0, st, entry, n, bitmap, list, state);
  launches += 1;
  uint32_t tail = 1;
  for (uint32_t layer = g->h_level[entry] + 1; layer-- > 0;) {
    uint32_t lo = 0, hi = tail;  // the layer starts from everything reached so far
    while (hi > lo) {
      const bool narrow = hi - lo <= kGhQueue;
      if (narrow)
        hipLaunchKernelGGL(gh_reach_narrow_kernel, dim3(1), dim3(kGhNarrowThreads), 0, st, gg, layer, entry, lo, hi, bitmap, list, state);
      else
        hipLaunchKernelGGL(gh_reach_wide_kernel, dim3(prune_grid(ctx, hi - lo)), dim3(256), 0, st, gg, layer, entry, lo, hi, bitmap, list,
                           state);
      launches += 1;
      reach_launches += 1;
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipMemcpyAsync(h_words, state, kGhStateWords * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      host_syncs += 1;
      tail = std::min(h_words[kGhTail], n);
      if (tail < hi) FAIL(ctx, FVDB_E_HIP, "graph health: the reach list shrank");  // cannot happen: the list only grows
      if (layer == 0) rounds0 += narrow ? h_words[kGhSteps] : 1u;
      lo = narrow ? std::min(std::max(h_words[kGhFrontier], hi), tail) : hi;
      hi = tail;
    }
  }
  reached = tail;
  return FVDB_OK;
}

// weak components of the live layer-0 graph
int HealthJob::components() {
  uint32_t *parent = sc.parent.as<uint32_t>(), *size = sc.size.as<uint32_t>(), *label = sc.label.as<uint32_t>();
  hipLaunchKernelGGL(uf_init_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, n, parent, size);
  hipLaunchKernelGGL(uf_union_kernel, dim3(prune_grid(ctx, n)), dim3(256), 0, st, gg, parent);
  hipLaunchKernelGGL(uf_label_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, gg.deleted, n, parent, label, size);
  hipLaunchKernelGGL(uf_summary_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, label, size, n, counters);
  launches += 4;
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// the counters come back (the job's last sync) and become the report
int HealthJob::report(fvdb_graph_health_t* out) {
  HIPCHK(ctx, ev.mark(1, st));
  HIPCHK(ctx, hipMemcpyAsync(g->h_state.p, counters, (size_t)kGhCounters * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  host_syncs += 1;
  const unsigned long long* c = (const unsigned long long*)g->h_state.p;
  out->n_nodes = n;
  out->n_live = (uint32_t)c[kGhLive];
  out->has_entry = has_entry ? 1u : 0u;
  out->entry_live = has_entry && !g->h_deleted[entry] ? 1u : 0u;
  out->entry_level = has_entry ? g->h_level[entry] : 0u;
  out->max_level_live = (uint32_t)c[kGhMaxLevel];
  out->edge_slots_live = c[kGhSlots];
  out->dangling = c[kGhDangling];
  out->dangling0 = c[kGhDangling0];
  for (uint32_t b = 0; b < 65; ++b) out->degree0_hist[b] = (uint32_t)c[kGhHist + b];
  if (want_reach) {
    // the entry point is in R whether it is live or not; everything else in R is live
    out->reachable_live = reached - ((has_entry && !out->entry_live) ? 1u : 0u);
    out->unreachable_live = out->n_live - out->reachable_live;
    out->reach_rounds0 = rounds0;
  }
  if (want_comp) {
    out->components0 = (uint32_t)c[kGhComponents];
    out->largest_component0 = (uint32_t)c[kGhLargest];
    out->isolated0 = (uint32_t)c[kGhIsolated];
  }
  out->launches = launches;
  out->reach_launches = reach_launches;
  out->host_syncs = host_syncs;
  out->ms = ev.ms(0, 1);
  return FVDB_OK;
}

}  // namespace

extern "C" int fvdb_graph_health(fvdb_graph* g, uint32_t flags, fvdb_graph_health_t* out) {
  if (!g || !out) return FVDB_E_INVALID;
  fvdb_ctx* ctx = g->store->ctx;
  std::memset(out, 0, sizeof *out);
  if (flags & ~(FVDB_HEALTH_SKIP_REACH | FVDB_HEALTH_SKIP_COMPONENTS)) FAIL(ctx, FVDB_E_INVALID, "graph health: unknown flag");
  if (!g->uploaded) FAIL(ctx, FVDB_E_INVALID, "graph health: no device graph");
  const bool want_reach = !(flags & FVDB_HEALTH_SKIP_REACH), want_comp = !(flags & FVDB_HEALTH_SKIP_COMPONENTS);
  const uint32_t n = g->n;
  if (n >= 0x80000000u) FAIL(ctx, FVDB_E_UNSUPPORTED, "graph health: 2^31 nodes or more");
  g->health_has = 0;
  if (n == 0) {
    g->health_has = (want_reach ? 1u : 0u) | (want_comp ? 2u : 0u);
    g->health_n = 0;
    g->health_at = g->mutations;
    return FVDB_OK;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HealthJob J{g, ctx, ctx->stream, n, want_reach, want_comp, (size_t)cdiv(n, 32) * 4, (size_t)n * 4,
              (size_t)kGhCounters * 8 + kGhStateWords * 4};
  int rc = J.alloc(out);
  if (rc) return rc;
  if ((rc = J.census())) return rc;
  if (want_reach && (rc = J.reach())) return rc;
  if (want_comp && (rc = J.components())) return rc;
  if ((rc = J.report(out))) return rc;
  std::swap(g->d_hreach, J.sc.bitmap);
  std::swap(g->d_hlabel, J.sc.label);
  J.sc = HealthJob::Scratch{};  // the scratch goes back (the last job's results with it); the per-node results stay until the next job
  g->health_has = (want_reach ? 1u : 0u) | (want_comp ? 2u : 0u);
  g->health_n = n;
  g->health_at = g->mutations;
  return FVDB_OK;
}

extern "C" int fvdb_graph_health_nodes(fvdb_graph* g, uint8_t* reached, uint32_t* label0) {
  if (!g) return FVDB_E_INVALID;
  fvdb_ctx* ctx = g->store->ctx;
  if (g->health_at != g->mutations || g->health_n != g->n) FAIL(ctx, FVDB_E_INVALID, "graph health: the graph changed since the last job (or none ran)");
  if ((reached && !(g->health_has & 1u)) || (label0 && !(g->health_has & 2u))) FAIL(ctx, FVDB_E_INVALID, "graph health: the last job skipped that part");
  const uint32_t n = g->health_n;
  if (n == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (reached) {
    std::vector<uint32_t> words(cdiv(n, 32));
    HIPCHK(ctx, hipMemcpyAsync(words.data(), g->d_hreach.p, words.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < n; ++i) reached[i] = (uint8_t)((words[i >> 5] >> (i & 31)) & 1u);
  }
  if (label0) {
    HIPCHK(ctx, hipMemcpyAsync(label0, g->d_hlabel.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return FVDB_OK;
}

// what allow_masks.h builds a graph mask from, and the inputs of its exact scan
int graph_mask_source(fvdb_graph* g, GraphMaskSource* out) {
  out->store = g->store;
  out->deleted = g->d_deleted.as<uint32_t>();
  out->n = g->uploaded ? g->n : 0;
  out->mutations = g->mutations;
  return FVDB_OK;
}
int graph_scan_inputs(fvdb_graph* g, fvdb_ctx* ctx, uint32_t slot, const float* q_dev, uint32_t B, size_t part_bytes,
                      const float** queries, uint64_t** part) {
  const fvdb_store* s = g->store;
  DBuf& scratch = g->s_scan[slot];
  const size_t q_bytes = s->d != s->dpad ? (((size_t)B * s->dpad * 4 + 255) & ~(size_t)255) : 0;
  HIPCHK(ctx, scratch.ensure(std::max<size_t>(q_bytes + part_bytes, 8)));
  *queries = q_dev;
  if (q_bytes) {
    hipLaunchKernelGGL(graph_pad_rows_kernel, dim3(cdiv((uint64_t)B * s->dpad, 256)), dim3(256), 0, ctx->stream, q_dev, s->d,
                       s->dpad, (uint64_t)B, scratch.as<float>());
    *queries = scratch.as<float>();
  }
  *part = (uint64_t*)((char*)scratch.p + q_bytes);
  return FVDB_OK;
}
