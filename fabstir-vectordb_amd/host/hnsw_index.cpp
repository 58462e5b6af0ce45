// hnsw_index.cpp — HNSWIndex mirror (src/hnsw/core.rs, src/hnsw/operations.rs).
// Ids, levels, flags and a copy of the adjacency live here.  Inserts and batch searches normally run whole on the
// device against the adjacency in HBM (fvdb_graph_insert_linked / fvdb_graph_search_dev*); the host algorithm below —
// heaps and visited sets here, every distance batch scored on the GPU through fvdb_scorer_* — is the other mode of
// both (same results), and what takes over for shapes the device kernels do not serve.  The reference's search_layer
// is restated once (HNSWIndex::search_layer, B queries in lock step): search_host_walk runs it for a batch of queries,
// link_host for the one vector being inserted, each on its own Walk (scorer and heaps).
#include <omp.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fvdb_host.hpp"

namespace fvdbh {

// ---- round_f16: the doors of an index with fp16 rows (fvdb_host.hpp) -------------------------
// f32 -> binary16 (round to nearest, ties to even) -> f32, on the bit patterns.  binary16: 1 sign, 5 exponent (bias 15),
// 10 mantissa bits; normal range 2^-14 .. 65504, subnormals k * 2^-24.  Rounding to nearest even of the value at the
// target's spacing is: add half a unit in the last kept place, less one when the kept part is even, and cut.
void round_f16(const float* in, uint64_t n, float* out) {
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t u;
    std::memcpy(&u, &in[i], 4);
    const uint32_t sign = u & 0x80000000u;
    uint32_t a = u & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) {
      // Inf and NaN are themselves
    } else if (a >= 0x477FF000u) {
      a = 0x7F800000u;  // >= 65520 = 65504 + half a unit: rounds past the largest half, to infinity
    } else if (a >= 0x38800000u) {
      // normal half (>= 2^-14): keep 10 of the 23 mantissa bits; a carry into the exponent is the right answer
      a += 0x00000FFFu + ((a >> 13) & 1u);
      a &= 0xFFFFE000u;
    } else if (a <= 0x33000000u) {
      a = 0;  // <= 2^-25, half the smallest subnormal: the tie goes to the even neighbour, zero
    } else {
      // subnormal half: a multiple of 2^-24.  m = the 24-bit significand, to be cut by `shift` more bits than it has
      const uint32_t e = a >> 23;  // 102 .. 112
      const uint32_t m = (a & 0x007FFFFFu) | 0x00800000u;
      const uint32_t shift = 126 - e;  // 14 .. 24: value = m * 2^(e - 150) = (m >> shift) * 2^-24 and a remainder
      const uint32_t k = (m + ((1u << (shift - 1)) - 1u) + ((m >> shift) & 1u)) >> shift;  // 0 .. 1024 (2^-14)
      // k * 2^-24 as f32: exact in float arithmetic, k < 2^11
      const float f = (float)k * 5.9604644775390625e-8f;
      std::memcpy(&a, &f, 4);
    }
    a |= sign;
    std::memcpy(&out[i], &a, 4);
  }
}

// ---- RustHeap ------------------------------------------------------------------------------
void RustHeap::sift_up(size_t start, size_t pos) {
  Cand elt = data[pos];
  while (pos > start) {
    size_t parent = (pos - 1) / 2;
    if (le(elt, data[parent])) break;
    data[pos] = data[parent];
    pos = parent;
  }
  data[pos] = elt;
}
void RustHeap::push(Cand c) {
  size_t old = data.size();
  data.push_back(c);
  sift_up(0, old);
}
Cand RustHeap::pop() {
  Cand item = data.back();
  data.pop_back();
  if (!data.empty()) {
    std::swap(item, data[0]);
    const size_t end = data.size();
    size_t pos = 0;
    Cand elt = data[0];
    size_t child = 1;
    const size_t lim = end >= 2 ? end - 2 : 0;
    while (child <= lim) {
      if (le(data[child], data[child + 1])) child += 1;
      data[pos] = data[child];
      pos = child;
      child = 2 * pos + 1;
    }
    if (child == end - 1) {
      data[pos] = data[child];
      pos = child;
    }
    data[pos] = elt;
    sift_up(0, pos);
  }
  return item;
}

// ---- Visited -------------------------------------------------------------------------------
void Visited::reset(size_t expect) {
  size_t want = 64;
  while (want < expect * 2) want <<= 1;
  if (keys.size() < want) {
    keys.assign(want, 0);
    stamp.assign(want, 0);
    epoch = 0;
  }
  epoch += 1;
  if (epoch == 0) {  // wrapped
    std::fill(stamp.begin(), stamp.end(), 0u);
    epoch = 1;
  }
  used = 0;
}
void Visited::grow() {
  std::vector<uint32_t> ok;
  ok.reserve(used);
  for (size_t i = 0; i < keys.size(); ++i)
    if (stamp[i] == epoch) ok.push_back(keys[i]);
  const size_t nsz = keys.size() * 2;
  keys.assign(nsz, 0);
  stamp.assign(nsz, 0);
  epoch = 1;
  used = 0;
  for (uint32_t v : ok) insert(v);
}
bool Visited::insert(uint32_t v) {
  if ((used + 1) * 2 > keys.size()) grow();
  const size_t mask = keys.size() - 1;
  size_t h = (v * 2654435761u) & mask;
  for (;;) {
    if (stamp[h] != epoch) {
      stamp[h] = epoch;
      keys[h] = v;
      used++;
      return true;
    }
    if (keys[h] == v) return false;
    h = (h + 1) & mask;
  }
}

// Worker threads for the lock-step traversal: the CPUs this process may actually use — the
// smaller of its affinity mask and its cgroup CPU quota (a container can see 256 CPUs and own
// 16; oversubscribed OpenMP barriers then collapse under CFS throttling).  FVDB_HOST_THREADS overrides.
static int usable_cpus() {
  if (const char* e = getenv("FVDB_HOST_THREADS")) {
    int v = atoi(e);
    if (v > 0) return v;
  }
  int n = omp_get_num_procs();
  long quota = -1, period = -1;
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota|max> <period>"
    char q[64];
    if (fscanf(f, "%63s %ld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atol(q);
    fclose(f);
  } else if (FILE* f1 = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {  // cgroup v1
    if (fscanf(f1, "%ld", &quota) != 1) quota = -1;
    fclose(f1);
    if (FILE* f2 = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
      if (fscanf(f2, "%ld", &period) != 1) period = -1;
      fclose(f2);
    }
  }
  if (quota > 0 && period > 0) n = std::min<long>(n, std::max<long>(1, (quota + period - 1) / period));
  return std::max(1, std::min(n, 64));
}

static inline bool set_insert(std::vector<uint32_t>& s, uint32_t v) {
  if (std::find(s.begin(), s.end(), v) != s.end()) return false;
  s.push_back(v);
  return true;
}

// ---- HNSWIndex -----------------------------------------------------------------------------
HNSWIndex::HNSWIndex(fvdb_ctx* ctx, const HNSWConfig& cfg) : ctx_(ctx), cfg_(cfg), rng_(cfg.seed) {}

HNSWIndex::~HNSWIndex() {
  view_.reset();  // the cached mask goes before the graph it points into
  if (graph_) fvdb_graph_destroy(graph_);
  for (uint32_t i = 0; i < kSlots; ++i) {
    slots_[i].buf.release();
    slots_[i].gq.release();
    if (i > 0 && slots_[i].ctx) fvdb_ctx_destroy(slots_[i].ctx);
  }
  d_q_.release();
  qual_.release();
  diverse_.release();
  for (Walk* w : {&search_walk_, &insert_walk_})
    if (w->sc) fvdb_scorer_destroy(w->sc);
  if (store_) fvdb_store_destroy(store_);
}

bool HNSWIndex::entry_point(uint64_t* id) const {
  if (!has_entry_) return false;
  *id = ids_[entry_];
  return true;
}

// src/hnsw/core.rs:211-224
size_t HNSWIndex::assign_level() {
  size_t level = 0;
  while (rng_.gen_f64() < 0.408) level += 1;
  return level;
}

int HNSWIndex::ensure_store(uint32_t dim) {
  if (store_) return FVDB_OK;
  return fvdb_store_create_ex(ctx_, dim, 1024, cfg_.row_dtype, &store_);
}

int HNSWIndex::walk_begin(Walk& w, uint32_t B, uint32_t C) {
  if (!w.sc || w.cap_B < B || w.cap_C < C) {
    if (w.sc) fvdb_scorer_destroy(w.sc);
    w.sc = nullptr;
    w.cap_B = std::max(B, w.cap_B);
    w.cap_C = std::max(C, w.cap_C);
    int rc = fvdb_scorer_create(store_, w.cap_B, w.cap_C, &w.sc);
    if (rc) return rc;
  }
  if (w.qs.size() < B) w.qs.resize(B);
  w.prev_cnt.assign(w.cap_B, w.cap_C);  // rows start dirty: blanked on first use, so no stale candidate is ever scored
  return FVDB_OK;
}

const float* HNSWIndex::vector_of(uint64_t id) const {
  auto it = index_of_.find(id);
  return it == index_of_.end() ? nullptr : &host_vecs_[(size_t)it->second * dim_];
}

void HNSWIndex::get_vectors(const uint64_t* ids, uint64_t n, float* out, uint8_t* found) const {
  for (uint64_t i = 0; i < n; ++i) {
    const float* v = vector_of(ids[i]);
    found[i] = v != nullptr;
    if (v) std::memcpy(out + i * dim_, v, (size_t)dim_ * sizeof(float));
  }
}

bool HNSWIndex::store_row_of(uint64_t id, uint32_t* row) const {
  auto it = index_of_.find(id);
  if (it == index_of_.end() || !store_ || it->second >= fvdb_store_rows(store_)) return false;
  *row = it->second;
  return true;
}

int64_t HNSWIndex::level_of(uint64_t id) const {
  auto it = index_of_.find(id);
  return it == index_of_.end() ? -1 : (int64_t)level_[it->second];
}

int64_t HNSWIndex::neighbors(uint64_t id, uint32_t layer, uint64_t* out, uint64_t cap_out) {
  if (ensure_host_graph()) return -1;
  auto it = index_of_.find(id);
  if (it == index_of_.end() || layer > level_[it->second]) return -1;
  const auto& s = nbrs_[it->second][layer];
  for (size_t i = 0; i < s.size() && i < cap_out; ++i) out[i] = ids_[s[i]];
  return (int64_t)s.size();
}

// src/hnsw/operations.rs:127-137
int HNSWIndex::mark_deleted(uint64_t id) {
  auto it = index_of_.find(id);
  if (it == index_of_.end()) return FVDB_E_NOT_FOUND;
  deleted_[it->second] = 1;
  if (graph_ && !host_ahead_) fvdb_graph_set_deleted(graph_, it->second, 1);
  return FVDB_OK;
}
bool HNSWIndex::is_deleted(uint64_t id) const {
  auto it = index_of_.find(id);
  return it != index_of_.end() && deleted_[it->second];
}
uint64_t HNSWIndex::active_count() const {
  uint64_t n = 0;
  for (size_t i = 0; i < ids_.size(); ++i)
    if (registered_[i] && !deleted_[i]) ++n;
  return n;
}

// --------------------------------------------------------------------------------------------
// search_layer (src/hnsw/core.rs:469-554) for B queries in lock-step.  The queries are already
// in the scorer, each query's entry is cur[0].  Per hop every active query pops candidates until
// one of them has unvisited, live neighbours; those go to the GPU in one launch; the admission
// rule (:517-531) is then applied in neighbour order with the returned distances.  cur becomes
// the layer's result — and stays what it was if the layer returned nothing (:445-447).
// --------------------------------------------------------------------------------------------
int HNSWIndex::search_layer(Walk& w, uint32_t B, uint32_t ef, uint32_t layer) {
  const uint32_t maxC = w.cap_C;
  uint32_t* cand = fvdb_scorer_cand_buffer(w.sc);
  const float* dist = fvdb_scorer_dist_buffer(w.sc);
  static const int auto_threads = usable_cpus();
  const int nt = B >= 32 ? std::max(1, threads_ > 0 ? threads_ : auto_threads) : 1;  // OpenMP threads of the host phases
  const uint8_t* del = w.del ? w.del : deleted_.data();  // a filtered search sees the nodes outside its allow-set as deleted

#pragma omp parallel for schedule(static) num_threads(nt) if (nt > 1)
  for (uint32_t b = 0; b < B; ++b) {
    Query& s = w.qs[b];
    s.candidates.clear();
    s.nearest.clear();
    s.pending.clear();
    s.visited.reset((size_t)ef * 8 + 64);
    const Cand e = s.cur[0];
    s.candidates.push({e.node, e.distance});
    s.nearest.push({e.node, -e.distance});
    s.visited.insert(e.node);
    s.active = true;
  }

  for (;;) {
    // prepare: the hop's candidates into the scorer's rows, what the previous hop left there blanked
    uint32_t hopC = 0;
    uint64_t hop_dists = 0;
#pragma omp parallel for schedule(static) num_threads(nt) reduction(max : hopC) reduction(+ : hop_dists) if (nt > 1)
    for (uint32_t b = 0; b < B; ++b) {
      Query& s = w.qs[b];
      s.pending.clear();
      if (s.active) {
        for (;;) {
          if (s.candidates.empty()) {
            s.active = false;
            break;
          }
          const Cand cur = s.candidates.pop();
          if (cur.distance > -s.nearest.peek().distance) {  // :499-501
            s.active = false;
            break;
          }
          const uint32_t node = cur.node;
          if (registered_[node] && level_[node] >= layer) {
            for (uint32_t nbv : nbrs_[node][layer]) {
              if (!s.visited.insert(nbv)) continue;  // :506-507
              if (!registered_[nbv]) continue;       // nodes.get() == None (:509)
              if (del[nbv]) continue;                // :511-513
              s.pending.push_back(nbv);
            }
          }
          if (!s.pending.empty()) break;
        }
      }
      uint32_t* row = cand + (size_t)b * maxC;
      const uint32_t n = (uint32_t)s.pending.size();
      for (uint32_t i = 0; i < n; ++i) row[i] = s.pending[i];
      for (uint32_t i = n; i < w.prev_cnt[b]; ++i) row[i] = FVDB_NO_ROW;
      w.prev_cnt[b] = n;
      hopC = std::max(hopC, n);
      hop_dists += n;
    }
    if (hopC == 0) break;
    int rc = fvdb_scorer_run(w.sc, B, hopC);  // score: one launch for the whole batch
    if (rc) return rc;
    n_hops_ += 1;
    n_dist_ += hop_dists;
    // apply
#pragma omp parallel for schedule(static) num_threads(nt) if (nt > 1)
    for (uint32_t b = 0; b < B; ++b) {
      Query& s = w.qs[b];
      const float* drow = dist + (size_t)b * maxC;
      for (size_t i = 0; i < s.pending.size(); ++i) {
        const float d = drow[i];
        if (d < -s.nearest.peek().distance || s.nearest.len() < ef) {  // :517-519
          s.candidates.push({s.pending[i], d});
          s.nearest.push({s.pending[i], -d});
          if (s.nearest.len() > ef) s.nearest.pop();
        }
      }
    }
  }

#pragma omp parallel for schedule(static) num_threads(nt) if (nt > 1)
  for (uint32_t b = 0; b < B; ++b) {
    Query& s = w.qs[b];
    if (s.nearest.empty()) continue;  // search_layer returned nothing: keep the previous nearest (:445-447)
    auto& r = s.cur;
    r.clear();
    r.reserve(s.nearest.len());
    for (const Cand& c : s.nearest.data) r.push_back({c.node, -c.distance});  // :541-547 (heap order)
    std::stable_sort(r.begin(), r.end(), [](const Cand& a, const Cand& c) { return a.distance < c.distance; });
  }
  return FVDB_OK;
}

int HNSWIndex::ensure_graph_handle() {
  if (graph_) return FVDB_OK;
  int rc = fvdb_graph_create(store_, &graph_);
  if (rc) return rc;
  rc = fvdb_graph_set_insert_visited(graph_, visited_mode_, visited_slots_);
  if (rc) return rc;
  return fvdb_graph_configure(graph_, cfg_.max_connections, cfg_.max_connections_layer_0);
}

int HNSWIndex::set_insert_visited(int mode, uint32_t table_slots) {
  if (mode < 0 || mode > 2) return FVDB_E_INVALID;
  if (table_slots != 0 && (table_slots < 256 || table_slots > 32768 || (table_slots & (table_slots - 1)) != 0)) return FVDB_E_INVALID;
  visited_mode_ = mode;
  visited_slots_ = table_slots;
  return graph_ ? fvdb_graph_set_insert_visited(graph_, mode, table_slots) : FVDB_OK;
}

int HNSWIndex::insert_info(fvdb_graph_insert_info_t* out) {
  if (!graph_) return FVDB_E_NOT_FOUND;
  return fvdb_graph_insert_info(graph_, cfg_.ef_construction, out);
}

// host -> device: install the whole graph, once, when nbrs_ holds changes the device has not seen
int HNSWIndex::sync_graph() {
  std::lock_guard<std::mutex> lk(sync_mu_);  // the first of several concurrent searches after such a change uploads
  int rc = ensure_graph_handle();
  if (rc) return rc;
  if (!host_ahead_) return FVDB_OK;
  const uint32_t n = (uint32_t)ids_.size();
  if (n == 0) {
    host_ahead_ = false;
    return FVDB_OK;
  }
  std::vector<uint32_t> slot_start, adj;
  slot_start.reserve(graph_slots() + 1);
  uint64_t edges = 0;
  for (const auto& nd : nbrs_)
    for (const auto& l : nd) edges += l.size();
  adj.reserve(edges);
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t l = 0; l <= level_[i]; ++l) {
      slot_start.push_back((uint32_t)adj.size());
      adj.insert(adj.end(), nbrs_[i][l].begin(), nbrs_[i][l].end());
    }
  slot_start.push_back((uint32_t)adj.size());
  rc = fvdb_graph_upload(graph_, n, level_.data(), deleted_.data(), slot_start.data(), adj.data(), entry_);
  if (rc) return rc;
  host_ahead_ = false;
  return FVDB_OK;
}

// device -> host: pull the lists device inserts have made
int HNSWIndex::ensure_host_graph() {
  std::lock_guard<std::mutex> lk(sync_mu_);
  if (!dev_ahead_) return FVDB_OK;
  const uint32_t n = (uint32_t)ids_.size();
  uint64_t slots = 0;
  for (uint32_t i = 0; i < n; ++i) slots += level_[i] + 1;
  std::vector<uint32_t> slot_start(slots + 1);
  uint64_t edges = 0;
  int rc = fvdb_graph_download(graph_, slot_start.data(), nullptr, 0, &edges);
  if (rc) return rc;
  std::vector<uint32_t> adj(std::max<uint64_t>(edges, 1));
  rc = fvdb_graph_download(graph_, slot_start.data(), adj.data(), adj.size(), &edges);
  if (rc) return rc;
  uint64_t sidx = 0;
  for (uint32_t i = 0; i < n; ++i) {
    nbrs_[i].resize(level_[i] + 1);
    for (uint32_t l = 0; l <= level_[i]; ++l, ++sidx)
      nbrs_[i][l].assign(adj.begin() + slot_start[sidx], adj.begin() + slot_start[sidx + 1]);
  }
  dev_ahead_ = false;
  return FVDB_OK;
}

// one device block and one pinned block per slot, [nodes B*k | dist B*k | counts B | status B] -> a single copy
namespace {
struct WalkBlock {
  uint32_t* nodes;
  float* dist;
  uint32_t *counts, *status;
  uint64_t bytes;
  WalkBlock(void* base, uint32_t B, uint32_t k) {
    const uint64_t need = (uint64_t)B * std::max<uint32_t>(k, 1);
    nodes = (uint32_t*)base;
    dist = (float*)base + need;
    counts = (uint32_t*)base + 2 * need;
    status = counts + B;
    bytes = (2 * need + 2 * (uint64_t)B) * 4;
  }
};
}  // namespace

// --------------------------------------------------------------------------------------------
// The five steps of a search (fvdb_host.hpp, HNSWIndex::Search)
// --------------------------------------------------------------------------------------------
// What an entry point answers before it reaches the device — DESIGN.md section 9l has the table.  The entry points
// differ in WHERE the empty batch (B == 0 or k == 0) is answered, and a caller can tell: the filtered traversal
// answers it before it looks at the dimension, the exact search after that, search() / search_dev() last of all.
int HNSWIndex::admit(Search& s) {
  s.route = Search::kAnswered;
  const bool exact = s.kind == Search::kExact, filtered = s.by_list || s.view, nothing = s.B == 0 || s.k == 0;
  if (exact && (s.k == 0 || s.k > (s.wide ? FVDB_MAX_K_WIDE : FVDB_MAX_K))) return FVDB_E_UNSUPPORTED;
  if (exact && s.slot >= kSlots) return FVDB_E_INVALID;  // a traversal's slot is launch()'s to refuse, after all of this
  if (s.ids) fill_empty(s.ids, s.dist, s.counts, s.B, s.k);
  if (s.totals) std::memset(s.totals, 0, (size_t)s.B * 4);
  // empty index -> empty results (:404-407); the exact scan needs the store too (a graph that has never held a row)
  if (!has_entry_ || (exact && !store_)) return FVDB_OK;
  if (!exact && filtered && nothing) return FVDB_OK;
  if (has_dim_ && s.dim != dim_) return FVDB_E_DIM;
  if (exact && nothing) return FVDB_OK;
  if (s.by_list) {
    if (int rc = allowed_view(s.allowed, s.n_allowed, &s.held)) return rc;
    s.view = s.held.get();
  }
  // "Entry point node not found in index" (:422-429); the exact search does not start from it and still answers
  if (!exact && entry_lost_) return FVDB_E_NOT_FOUND;
  if (nothing) return FVDB_OK;
  if (exact && s.view && !s.view->mask) return FVDB_OK;
  // the scans are device kernels whatever the traversal setting; the traversal kernel has one lane per neighbour
  static const bool env_off = getenv("FVDB_HNSW_DEVICE") && atoi(getenv("FVDB_HNSW_DEVICE")) == 0;
  const uint32_t maxdeg = std::max(cfg_.max_connections, cfg_.max_connections_layer_0);
  s.scanned = exact || (s.view && scans(*s.view, s.k));
  s.route = s.scanned || (device_traversal_ && !env_off && maxdeg <= 64 && s.ef <= 4096) ? Search::kDevice : Search::kHostWalk;
  return FVDB_OK;
}

int HNSWIndex::stage(Search& s) {
  s.q_dev = s.q;
  if (s.q_on_device) return FVDB_OK;
  const uint64_t bytes = (uint64_t)s.B * s.dim * 4;
  int rc = d_q_.reserve(ctx_, bytes, false);
  if (!rc) rc = fvdb_dev_upload(ctx_, d_q_.dev, s.q, bytes);
  s.q_dev = (const float*)d_q_.dev;
  return rc;
}

// whole batch in one launch, results copied to pinned host memory — all asynchronous on the slot's stream
int HNSWIndex::launch(Search& s) {
  if (s.slot >= kSlots) return FVDB_E_INVALID;
  int rc = sync_graph();
  if (rc) return rc;
  DevSlot& sl = slots_[s.slot];
  rc = slot_ctx(ctx_, s.slot == 0, &sl.ctx);
  if (rc) return rc;
  const uint64_t bytes = WalkBlock(nullptr, s.B, s.k).bytes;
  // a radius search's radii ride behind the result block and the sizes of its balls come back in the status words
  const uint64_t r_bytes = s.radius ? (uint64_t)s.B * 4 : 0;
  rc = sl.buf.reserve(sl.ctx, bytes + r_bytes, true);
  if (rc) return rc;
  const WalkBlock d(sl.buf.dev, s.B, s.k);
  fvdb_ctx* on = s.slot == 0 ? nullptr : sl.ctx;
  fvdb_mask* mask = s.view ? s.view->mask.get() : nullptr;
  const float* r_dev = (const float*)((char*)sl.buf.dev + bytes);
  if (s.radius && (rc = fvdb_dev_upload(sl.ctx, (char*)sl.buf.dev + bytes, s.radius, (size_t)r_bytes))) return rc;
  if (s.kind == Search::kExact && s.radius)
    rc = s.count_only ? fvdb_graph_count_within_dev_slot(graph_, on, s.slot, mask, s.q_dev, s.B, r_dev, d.status)
                      : fvdb_graph_search_flat_radius_dev_slot(graph_, on, s.slot, mask, s.q_dev, s.B, r_dev, s.k, d.nodes, d.dist,
                                                               d.counts, d.status);
  else if (s.kind == Search::kExact)
    rc = (s.wide ? fvdb_graph_search_flat_wide_dev_slot : fvdb_graph_search_flat_dev_slot)(graph_, on, s.slot, mask, s.q_dev, s.B, s.k,
                                                                                          d.nodes, d.dist, d.counts);
  else if (!s.view)
    rc = fvdb_graph_search_dev_slot(graph_, on, s.slot, s.q_dev, s.B, s.k, s.ef, d.nodes, d.dist, d.counts, d.status);
  else if (s.scanned)
    rc = fvdb_graph_scan_allowed_dev_slot(graph_, on, s.slot, mask, s.q_dev, s.B, s.k, d.nodes, d.dist, d.counts);
  else
    rc = fvdb_graph_search_dev_slot_masked(graph_, on, s.slot, mask, s.q_dev, s.B, s.k, s.ef, d.nodes, d.dist, d.counts, d.status);
  if (!rc) rc = fvdb_dev_download_async(sl.ctx, sl.buf.host, sl.buf.dev, (size_t)bytes);
  sl.enqueued = rc == FVDB_OK;
  sl.scanned = s.scanned;
  return rc;
}

// wait + translate; then, rare, the queries the kernel could not finish on chip (heap / visited log overflow) walk on
// the host.  A slot nothing was enqueued in: the search runs now, in slot 0.
int HNSWIndex::finish(Search& s) {
  if (s.slot >= kSlots) return FVDB_E_INVALID;
  DevSlot& sl = slots_[s.slot];
  // a request run() launched a moment ago (route kDevice) is collected whatever the mark says; one that arrives from
  // search_dev_end has not been through admit() in this call
  if (!sl.enqueued && s.route != Search::kDevice) {
    s.slot = 0;
    s.owns_slot = false;
    return run(s);
  }
  sl.enqueued = false;
  const uint32_t B = s.B, k = s.k;
  uint64_t* const ids = s.ids;  // the loop below runs B x k times per batch: everything it reads is a local
  uint32_t* const counts = s.counts;
  const bool scanned = sl.scanned;
  int rc = fvdb_ctx_synchronize(sl.ctx);
  if (rc) return rc;
  const WalkBlock h(sl.buf.host, B, k);
  if (s.totals) std::memcpy(s.totals, h.status, (size_t)B * 4);
  if (s.count_only) return FVDB_OK;
  std::memcpy(s.dist, h.dist, (size_t)B * k * 4);
  std::memcpy(counts, h.counts, (size_t)B * 4);
  std::vector<uint32_t> failed;
  for (uint32_t b = 0; b < B; ++b) {
    if (!scanned && h.status[b]) {
      failed.push_back(b);
      counts[b] = 0;
      continue;
    }
    for (uint32_t i = 0; i < k; ++i) {
      const uint32_t nd = h.nodes[(size_t)b * k + i];
      ids[(size_t)b * k + i] = i < counts[b] ? ids_[nd] : FVDB_NO_ID;
    }
  }
  if (failed.empty()) return FVDB_OK;
  n_fallback_ += failed.size();
  if ((rc = ensure_host_graph())) return rc;
  std::lock_guard<std::mutex> lk(walk_mu_);  // the host walk's scorer and heaps are one set per index
  const uint32_t dim = s.dim;
  std::vector<float> hq((size_t)failed.size() * dim);
  for (size_t i = 0; i < failed.size(); ++i) {
    if (s.q_on_device) {
      if ((rc = fvdb_dev_download(ctx_, &hq[i * dim], s.q + (size_t)failed[i] * dim, (size_t)dim * 4))) return rc;
    } else {
      std::memcpy(&hq[i * dim], s.q + (size_t)failed[i] * dim, (size_t)dim * 4);
    }
  }
  std::vector<uint64_t> fi(failed.size() * (size_t)k);
  std::vector<float> fd(failed.size() * (size_t)k);
  std::vector<uint32_t> fc(failed.size());
  rc = search_host_walk(hq.data(), false, (uint32_t)failed.size(), k, s.ef, fi.data(), fd.data(), fc.data(), s.view);
  if (rc) return rc;
  for (size_t i = 0; i < failed.size(); ++i) {
    std::memcpy(s.ids + (size_t)failed[i] * k, &fi[i * k], (size_t)k * 8);
    std::memcpy(s.dist + (size_t)failed[i] * k, &fd[i * k], (size_t)k * 4);
    s.counts[failed[i]] = fc[i];
  }
  return FVDB_OK;
}

// The standalone entry points work in slot 0 with one staging buffer, so calls from several host threads take turns
// (HybridIndex gives each of its concurrent searches a slot of its own and says so: owns_slot).
int HNSWIndex::run(Search& s) {
  int rc = admit(s);
  if (rc || s.route == Search::kAnswered) return rc;
  std::unique_lock<std::mutex> serial(search_mu_, std::defer_lock);
  if (!s.owns_slot) serial.lock();
  if (s.route == Search::kHostWalk) {  // the queries go to the scorer from wherever they are
    if ((rc = ensure_host_graph())) return rc;
    std::lock_guard<std::mutex> lk(walk_mu_);
    return search_host_walk(s.q, s.q_on_device, s.B, s.k, s.ef, s.ids, s.dist, s.counts, s.view);
  }
  if ((rc = stage(s)) || (rc = launch(s))) return rc;
  return finish(s);
}

// --------------------------------------------------------------------------------------------
// search (src/hnsw/core.rs:398-467), batched — the entry points
// --------------------------------------------------------------------------------------------
int HNSWIndex::search(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, uint64_t* ids, float* dist,
                      uint32_t* counts) {
  Search s{Search::kTraversal, q, false, B, dim, k, ef, ids, dist, counts};
  return run(s);
}

int HNSWIndex::search_dev(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, uint64_t* ids,
                          float* dist, uint32_t* counts) {
  Search s{Search::kTraversal, q_dev, true, B, dim, k, ef, ids, dist, counts};
  return run(s);
}

int HNSWIndex::search_allowed(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, const uint64_t* allowed,
                              uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts) {
  Search s{Search::kTraversal, q, false, B, dim, k, ef, ids, dist, counts};
  s.by_list = true, s.allowed = allowed, s.n_allowed = n_allowed;
  return run(s);
}

bool HNSWIndex::search_dev_begin(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, int* rc,
                                 uint32_t slot, const AllowView* view) {
  Search s{Search::kTraversal, q_dev, true, B, dim, k, ef, nullptr, nullptr, nullptr};
  s.slot = slot, s.view = view;
  *rc = FVDB_OK;
  if (slot < kSlots) slots_[slot].enqueued = false;
  // whatever the checks found, the end reports it: it runs them again with somewhere to put the answer
  if (admit(s) != FVDB_OK || s.route != Search::kDevice) return false;
  if ((*rc = stage(s)) == FVDB_OK) *rc = launch(s);
  return *rc == FVDB_OK;
}

int HNSWIndex::search_dev_end(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, uint64_t* ids,
                              float* dist, uint32_t* counts, uint32_t slot, const AllowView* view) {
  Search s{Search::kTraversal, q_dev, true, B, dim, k, ef, ids, dist, counts};
  s.slot = slot, s.view = view;
  return finish(s);
}

// ---- filtered search ----
int HNSWIndex::allowed_view(const uint64_t* allowed, uint64_t n_allowed, ViewRef* out) {
  if (n_allowed && !allowed) return FVDB_E_INVALID;
  if (!has_entry_ || !store_) {
    // a graph that has never held a row (a hybrid index fed only historical rows): every search of it answers "nothing"
    // before it reaches the device, a filtered one too — there is no store to build a device graph over, and no need
    *out = std::make_shared<AllowView>();
    return FVDB_OK;
  }
  int rc = sync_graph();  // the mask is built against the device graph as the next search will see it
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(view_mu_);
  const bool same = view_ && view_key_.size() == n_allowed &&
                    (n_allowed == 0 || std::memcmp(view_key_.data(), allowed, n_allowed * 8) == 0);
  if (!same || !mask_fresh(view_->mask)) {
    view_.reset();
    view_key_.clear();
    ViewRef v;
    if ((rc = make_view(allowed, n_allowed, &v))) return rc;
    view_ = v;
    view_key_.assign(allowed, allowed + n_allowed);
    mask_builds_ += 1;
  }
  *out = view_;
  return FVDB_OK;
}

// the allow-set as the synced device graph sees it: ids -> node indices, the device mask, the host copy of its flags
// scan_k > 0: the caller scans the view when scans(view, scan_k) and never hands such a view to the host walk, so the
// host flags — one byte per node of the graph, per view — are then left out.
int HNSWIndex::make_view(const uint64_t* allowed, uint64_t n_allowed, ViewRef* out, uint32_t scan_k) {
  auto v = std::make_shared<AllowView>();
  std::vector<uint32_t> nodes;
  nodes.reserve(n_allowed);
  for (uint64_t i = 0; i < n_allowed; ++i) {
    auto it = index_of_.find(allowed[i]);
    if (it == index_of_.end()) continue;  // an id this index does not hold
    nodes.push_back(it->second);
  }
  fvdb_mask* m = nullptr;
  int rc = fvdb_mask_create_graph(graph_, nodes.data(), nodes.size(), &m);
  if (rc) return rc;
  v->mask = adopt_mask(m);
  fvdb_mask_info_t info;
  if ((rc = fvdb_mask_info(m, &info))) return rc;
  v->allowed_live = info.allowed_live;
  if (!(scan_k && scans(*v, scan_k))) {
    v->eff.assign(ids_.size(), 1);
    for (uint32_t node : nodes) v->eff[node] = deleted_[node];
  }
  *out = v;
  return FVDB_OK;
}

// ---- one allow-set per query ----
int HNSWIndex::scan_groups(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, const std::vector<fvdb_mask*>& masks,
                           const std::vector<uint32_t>& local, uint32_t slot, uint64_t* ids, float* dist, uint32_t* counts) {
  DevSlot& sl = slots_[slot];
  int rc = slot_ctx(ctx_, slot == 0, &sl.ctx);
  if (rc) return rc;
  const uint64_t bytes = WalkBlock(nullptr, B, k).bytes;
  if ((rc = sl.buf.reserve(sl.ctx, bytes, true))) return rc;
  const WalkBlock d(sl.buf.dev, B, k);
  rc = fvdb_graph_scan_allowed_groups_dev_slot(graph_, slot == 0 ? nullptr : sl.ctx, slot, masks.data(), (uint32_t)masks.size(),
                                               local.data(), q_dev, B, k, d.nodes, d.dist, d.counts);
  if (rc) return rc;
  if ((rc = fvdb_dev_download_async(sl.ctx, sl.buf.host, sl.buf.dev, (size_t)bytes)) || (rc = fvdb_ctx_synchronize(sl.ctx))) return rc;
  const WalkBlock h(sl.buf.host, B, k);
  std::memcpy(dist, h.dist, (size_t)B * k * 4);
  std::memcpy(counts, h.counts, (size_t)B * 4);
  for (uint32_t b = 0; b < B; ++b)
    for (uint32_t i = 0; i < k; ++i) ids[(size_t)b * k + i] = i < counts[b] ? ids_[h.nodes[(size_t)b * k + i]] : FVDB_NO_ID;
  return FVDB_OK;
}

int HNSWIndex::search_allowed_groups(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, const AllowGroups& groups,
                                     uint64_t* ids, float* dist, uint32_t* counts, uint32_t slot, bool owns_slot) {
  // what search_allowed answers before it reaches the device, in its order (admit)
  fill_empty(ids, dist, counts, B, k);
  if (!groups.valid(B)) return FVDB_E_INVALID;
  if (!has_entry_ || B == 0 || k == 0) return FVDB_OK;
  if (has_dim_ && dim != dim_) return FVDB_E_DIM;
  if (slot >= kSlots) return FVDB_E_INVALID;
  std::unique_lock<std::mutex> serial(search_mu_, std::defer_lock);
  if (!owns_slot) serial.lock();  // the searches below run in the slot this call holds
  int rc = sync_graph();  // the masks are built against the device graph as the searches will see it
  if (rc) return rc;
  const uint32_t G = groups.G;
  std::vector<ViewRef> views(G);  // of this call: dropped at return
  for (uint32_t g = 0; g < G; ++g) {
    if (!groups.filtered[g]) continue;
    if ((rc = make_view(groups.set(g), groups.size(g), &views[g], k))) return rc;
    std::lock_guard<std::mutex> lk(view_mu_);
    mask_builds_ += 1;
  }
  if (entry_lost_) return FVDB_E_NOT_FOUND;
  // the queries in group order, the scanned groups first: every group is one run of rows, the scanned ones one block
  std::vector<uint32_t> n_of(G, 0);
  for (uint32_t b = 0; b < B; ++b) n_of[groups.group_of_query[b]] += 1;
  std::vector<uint32_t> order, first(G, 0), local_of(G, 0);
  std::vector<fvdb_mask*> scan_masks;
  for (int scanned = 1; scanned >= 0; --scanned)
    for (uint32_t g = 0; g < G; ++g) {
      const bool sc = views[g] && views[g]->mask && scans(*views[g], k);
      if (sc != (scanned == 1) || n_of[g] == 0) continue;
      order.push_back(g);
      if (sc) {
        local_of[g] = (uint32_t)scan_masks.size();
        scan_masks.push_back(views[g]->mask.get());
      }
    }
  uint32_t at = 0, B_scan = 0;
  for (uint32_t g : order) {
    first[g] = at;
    at += n_of[g];
    if (views[g] && views[g]->mask && scans(*views[g], k)) B_scan = at;
  }
  std::vector<uint32_t> place(B), fill = first, local(B_scan);
  for (uint32_t b = 0; b < B; ++b) place[b] = fill[groups.group_of_query[b]]++;
  std::vector<float> gq((size_t)B * dim);
  for (uint32_t b = 0; b < B; ++b) {
    std::memcpy(&gq[(size_t)place[b] * dim], q + (size_t)b * dim, (size_t)dim * 4);
    if (place[b] < B_scan) local[place[b]] = local_of[groups.group_of_query[b]];
  }
  DevSlot& sl = slots_[slot];
  if ((rc = sl.gq.reserve(ctx_, (uint64_t)B * dim * 4, false)) || (rc = fvdb_dev_upload(ctx_, sl.gq.dev, gq.data(), (size_t)B * dim * 4)))
    return rc;
  const float* q_dev = (const float*)sl.gq.dev;
  std::vector<uint64_t> gi((size_t)B * k);
  std::vector<float> gd((size_t)B * k);
  std::vector<uint32_t> gc(B, 0);
  fill_empty(gi.data(), gd.data(), gc.data(), B, k);
  if (B_scan && (rc = scan_groups(q_dev, B_scan, dim, k, scan_masks, local, slot, gi.data(), gd.data(), gc.data()))) return rc;
  for (uint32_t g : order) {
    if (first[g] < B_scan) continue;
    // a group too large to scan: the masked traversal of its queries alone; "no filter": the plain one
    const size_t o = first[g];
    Search s{Search::kTraversal, q_dev + o * dim, true, n_of[g], dim, k, ef, &gi[o * k], &gd[o * k], &gc[o]};
    s.view = views[g].get(), s.slot = slot, s.owns_slot = true;
    rc = run(s);
    // A traversal the caller's slot cannot hold runs in slot 0 under search_mu_, the way finish() runs a search nothing was
    // enqueued for.  The case in mind is padded dimensions (d not a multiple of 4: fvdb_graph_search_dev_slot pads the
    // queries into one buffer, slot 0's); any other FVDB_E_UNSUPPORTED fails there the same way again.  Before, a
    // grouped search of a HybridIndex at such a d with an unfiltered request was refused.  Like finish(), this does not
    // exclude a HybridIndex call that holds the lease on slot 0 without search_mu_.
    if (rc == FVDB_E_UNSUPPORTED && slot != 0) {
      s.slot = 0, s.owns_slot = false;
      rc = run(s);
    }
    if (rc) return rc;
  }
  for (uint32_t b = 0; b < B; ++b) {
    std::memcpy(ids + (size_t)b * k, &gi[(size_t)place[b] * k], (size_t)k * 8);
    std::memcpy(dist + (size_t)b * k, &gd[(size_t)place[b] * k], (size_t)k * 4);
    counts[b] = gc[place[b]];
  }
  return FVDB_OK;
}

// ---- exact search and search quality ----
int compare_id_blocks(fvdb_ctx* ctx, DevBuf& stage, uint32_t B, uint32_t k, const uint64_t* res_ids, const uint32_t* res_counts,
                      const uint64_t* truth_ids, const uint32_t* truth_counts, float* total_recall, float* total_precision) {
  const uint64_t n = (uint64_t)B * k;
  const uint64_t o_tid = n * 8, o_rc = 2 * n * 8, o_tc = o_rc + (uint64_t)B * 4, o_out = o_tc + (uint64_t)B * 4;
  const uint64_t bytes = o_out + (uint64_t)B * 8;
  int rc = stage.reserve(ctx, bytes, true);
  if (rc) return rc;
  char* h = (char*)stage.host;
  char* d = (char*)stage.dev;
  std::memcpy(h, res_ids, n * 8);
  std::memcpy(h + o_tid, truth_ids, n * 8);
  std::memcpy(h + o_rc, res_counts, (size_t)B * 4);
  std::memcpy(h + o_tc, truth_counts, (size_t)B * 4);
  if ((rc = fvdb_dev_upload(ctx, d, h, o_out))) return rc;
  float* out = (float*)(d + o_out);
  rc = fvdb_search_quality_lists_dev(ctx, (const uint64_t*)d, (const uint32_t*)(d + o_rc), (const uint64_t*)(d + o_tid),
                                     (const uint32_t*)(d + o_tc), B, k, out, out + B);
  if (rc) return rc;
  if ((rc = fvdb_dev_download_async(ctx, h + o_out, d + o_out, (size_t)B * 8)) || (rc = fvdb_ctx_synchronize(ctx))) return rc;
  const float* r = (const float*)(h + o_out);
  float tr = 0.0f, tp = 0.0f;
  for (uint32_t b = 0; b < B; ++b) {  // `total_recall += recall` (operations.rs:374-375), in query order
    tr += r[b];
    tp += r[B + b];
  }
  *total_recall = tr;
  *total_precision = tp;
  return FVDB_OK;
}

int HNSWIndex::search_exact_dev(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, const AllowView* view, uint64_t* ids,
                                float* dist, uint32_t* counts, uint32_t slot) {
  Search s{Search::kExact, q_dev, true, B, dim, k, 0, ids, dist, counts};
  s.view = view, s.slot = slot, s.owns_slot = true;
  return run(s);
}

int HNSWIndex::search_exact(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint64_t* ids, float* dist, uint32_t* counts) {
  Search s{Search::kExact, q, false, B, dim, k, 0, ids, dist, counts};
  return run(s);
}

int HNSWIndex::search_exact_allowed(const float* q, uint32_t B, uint32_t dim, uint32_t k, const uint64_t* allowed,
                                    uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts) {
  Search s{Search::kExact, q, false, B, dim, k, 0, ids, dist, counts};
  s.by_list = true, s.allowed = allowed, s.n_allowed = n_allowed;
  return run(s);
}

// ---- the same at k up to FVDB_MAX_K_WIDE: the request's `wide` flag and nothing else ----
int HNSWIndex::search_exact_wide_dev(const float* q_dev, uint32_t B, uint32_t dim, uint32_t k, const AllowView* view, uint64_t* ids,
                                     float* dist, uint32_t* counts, uint32_t slot) {
  Search s{Search::kExact, q_dev, true, B, dim, k, 0, ids, dist, counts};
  s.view = view, s.slot = slot, s.owns_slot = true, s.wide = true;
  return run(s);
}

int HNSWIndex::search_exact_wide(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint64_t* ids, float* dist, uint32_t* counts) {
  Search s{Search::kExact, q, false, B, dim, k, 0, ids, dist, counts};
  s.wide = true;
  return run(s);
}

int HNSWIndex::search_exact_wide_allowed(const float* q, uint32_t B, uint32_t dim, uint32_t k, const uint64_t* allowed,
                                         uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts) {
  Search s{Search::kExact, q, false, B, dim, k, 0, ids, dist, counts};
  s.by_list = true, s.allowed = allowed, s.n_allowed = n_allowed, s.wide = true;
  return run(s);
}

// ---- radius search: the wide request with a radius per query ----
int HNSWIndex::search_radius_dev(const float* q_dev, uint32_t B, uint32_t dim, const float* radius, uint32_t max_results,
                                 const AllowView* view, uint64_t* ids, float* dist, uint32_t* counts, uint32_t* totals, uint32_t slot) {
  if (int rc = check_radius(radius, B)) return rc;
  Search s{Search::kExact, q_dev, true, B, dim, max_results, 0, ids, dist, counts};
  s.view = view, s.slot = slot, s.owns_slot = true, s.wide = true, s.radius = radius, s.totals = totals;
  return run(s);
}

int HNSWIndex::search_radius(const float* q, uint32_t B, uint32_t dim, const float* radius, uint32_t max_results, uint64_t* ids,
                             float* dist, uint32_t* counts, uint32_t* totals) {
  if (int rc = check_radius(radius, B)) return rc;
  Search s{Search::kExact, q, false, B, dim, max_results, 0, ids, dist, counts};
  s.wide = true, s.radius = radius, s.totals = totals;
  return run(s);
}

int HNSWIndex::search_radius_allowed(const float* q, uint32_t B, uint32_t dim, const float* radius, uint32_t max_results,
                                     const uint64_t* allowed, uint64_t n_allowed, uint64_t* ids, float* dist, uint32_t* counts,
                                     uint32_t* totals) {
  if (int rc = check_radius(radius, B)) return rc;
  Search s{Search::kExact, q, false, B, dim, max_results, 0, ids, dist, counts};
  s.by_list = true, s.allowed = allowed, s.n_allowed = n_allowed, s.wide = true, s.radius = radius, s.totals = totals;
  return run(s);
}

int HNSWIndex::count_within(const float* q, uint32_t B, uint32_t dim, const float* radius, const uint64_t* allowed, uint64_t n_allowed,
                            uint32_t* totals) {
  if (int rc = check_radius(radius, B)) return rc;
  Search s{Search::kExact, q, false, B, dim, 1, 0, nullptr, nullptr, nullptr};
  s.by_list = allowed != nullptr, s.allowed = allowed, s.n_allowed = n_allowed;
  s.wide = true, s.radius = radius, s.totals = totals, s.count_only = true;
  return run(s);
}

int HNSWIndex::evaluate_search_quality(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, SearchQuality* out) {
  return quality_impl(q, B, dim, k, ef, out, false);
}

int HNSWIndex::evaluate_search_quality_wide(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, SearchQuality* out) {
  return quality_impl(q, B, dim, k, ef, out, true);
}

int HNSWIndex::quality_impl(const float* q, uint32_t B, uint32_t dim, uint32_t k, uint32_t ef, SearchQuality* out, bool wide) {
  if (B == 0 || !q || !out) return FVDB_E_INVALID;  // "No test queries provided" (operations.rs:334-338)
  if (k == 0 || k > (wide ? FVDB_MAX_K_WIDE : FVDB_MAX_K)) return FVDB_E_UNSUPPORTED;
  if (has_dim_ && dim != dim_) return FVDB_E_DIM;
  const auto start = std::chrono::steady_clock::now();
  const size_t n = (size_t)B * k;
  std::vector<uint64_t> rid(n), tid(n);
  std::vector<float> rd(n), td(n);
  std::vector<uint32_t> rcn(B), tcn(B);
  int rc;
  if ((rc = search(q, B, dim, k, ef, rid.data(), rd.data(), rcn.data()))) return rc;
  if ((rc = (wide ? search_exact_wide(q, B, dim, k, tid.data(), td.data(), tcn.data())
                  : search_exact(q, B, dim, k, tid.data(), td.data(), tcn.data()))))
    return rc;
  float tr = 0.0f, tp = 0.0f;
  {
    std::lock_guard<std::mutex> serial(search_mu_);  // qual_ is one block: calls take turns
    if ((rc = compare_id_blocks(ctx_, qual_, B, k, rid.data(), rcn.data(), tid.data(), tcn.data(), &tr, &tp))) return rc;
  }
  *out = quality_of(tr, tp, B, start);
  return FVDB_OK;
}

// ---- search quality over a grid of ef and n_probe ----
uint64_t quality_grid_budget() {
  const char* e = getenv("FVDB_QUALITY_GRID_BYTES");
  return e ? strtoull(e, nullptr, 10) : kQualityGridBytes;
}

int quality_grid_totals(fvdb_ctx* ctx, DevBuf& stage, const GridParts& p, float* total_recall, float* total_precision) {
  const uint32_t B = p.B, k = p.k, E = p.E, P = p.P, rk = p.rk, hk = p.hk;
  const uint32_t pairs = p.rows() * p.cols();
  for (uint32_t i = 0; i < pairs; ++i) total_recall[i] = total_precision[i] = 0.0f;
  const uint32_t step = quality_grid_step(quality_grid_budget(), p);
  // one sub-batch of n queries: the 8-byte blocks first, then the 4-byte ones, the figures last
  const uint64_t ns = step;
  const uint64_t o_gid = ns * k * 8, o_hid = o_gid + ns * E * rk * 8, o_gd = o_hid + ns * P * hk * 8, o_hd = o_gd + ns * E * rk * 4,
                 o_tc = o_hd + ns * P * hk * 4, o_gc = o_tc + ns * 4, o_hc = o_gc + ns * E * 4, o_out = o_hc + ns * P * 4;
  const uint64_t bytes = o_out + ns * pairs * 8;
  int rc = stage.reserve(ctx, bytes, true);
  if (rc) return rc;
  char* h = (char*)stage.host;
  char* d = (char*)stage.dev;
  for (uint32_t b0 = 0; b0 < B; b0 += step) {
    const uint32_t n = std::min(step, B - b0);
    // list e of a part is [B][width] on the host and [n][width] in the sub-batch: rows b0 .. b0 + n of it
    std::memcpy(h, p.tid + (size_t)b0 * k, (size_t)n * k * 8);
    std::memcpy(h + o_tc, p.tcn + b0, (size_t)n * 4);
    for (uint32_t e = 0; e < E; ++e) {
      const size_t src = (size_t)e * B + b0, dst = (size_t)e * n;
      std::memcpy(h + o_gid + dst * rk * 8, p.rid + src * rk, (size_t)n * rk * 8);
      std::memcpy(h + o_gd + dst * rk * 4, p.rd + src * rk, (size_t)n * rk * 4);
      std::memcpy(h + o_gc + dst * 4, p.rcn + src, (size_t)n * 4);
    }
    for (uint32_t j = 0; j < P; ++j) {
      const size_t src = (size_t)j * B + b0, dst = (size_t)j * n;
      std::memcpy(h + o_hid + dst * hk * 8, p.hid + src * hk, (size_t)n * hk * 8);
      std::memcpy(h + o_hd + dst * hk * 4, p.hd + src * hk, (size_t)n * hk * 4);
      std::memcpy(h + o_hc + dst * 4, p.hcn + src, (size_t)n * 4);
    }
    if ((rc = fvdb_dev_upload(ctx, d, h, o_out))) return rc;
    float* out = (float*)(d + o_out);
    rc = fvdb_quality_grid_dev(ctx, (const uint64_t*)d, (const uint32_t*)(d + o_tc), (const uint64_t*)(d + o_gid),
                               (const float*)(d + o_gd), (const uint32_t*)(d + o_gc), (const uint64_t*)(d + o_hid),
                               (const float*)(d + o_hd), (const uint32_t*)(d + o_hc), n, k, rk, hk, E, P, out, out + (size_t)pairs * n);
    if (rc) return rc;
    if ((rc = fvdb_dev_download_async(ctx, h + o_out, d + o_out, (size_t)pairs * n * 8)) || (rc = fvdb_ctx_synchronize(ctx))) return rc;
    const float* r = (const float*)(h + o_out);
    const float* pr = r + (size_t)pairs * n;
    for (uint32_t i = 0; i < pairs; ++i) {
      float tr = total_recall[i], tp = total_precision[i];
      for (uint32_t b = 0; b < n; ++b) {  // `total_recall += recall` (operations.rs:374-375), in query order
        tr += r[(size_t)i * n + b];
        tp += pr[(size_t)i * n + b];
      }
      total_recall[i] = tr;
      total_precision[i] = tp;
    }
  }
  return FVDB_OK;
}

int HNSWIndex::quality_by_ef(const float* q, uint32_t B, uint32_t dim, uint32_t k, const uint32_t* efs, uint32_t E, QualityGrid* out) {
  if (B == 0 || !q || !out || !efs || E == 0) return FVDB_E_INVALID;  // "No test queries provided" (operations.rs:334-338)
  if (k == 0 || k > FVDB_MAX_K_WIDE || E > 64) return FVDB_E_UNSUPPORTED;
  if (has_dim_ && dim != dim_) return FVDB_E_DIM;
  const auto start = std::chrono::steady_clock::now();
  const size_t n = (size_t)B * k;
  std::vector<uint64_t> tid(n), rid(n * E);
  std::vector<float> td(n), rd(n * E);
  std::vector<uint32_t> tcn(B), rcn((size_t)B * E);
  int rc;
  // the register form and the wide form agree for k <= FVDB_MAX_K (section 9q); each is what the single call uses there
  if ((rc = (k > FVDB_MAX_K ? search_exact_wide(q, B, dim, k, tid.data(), td.data(), tcn.data())
                            : search_exact(q, B, dim, k, tid.data(), td.data(), tcn.data()))))
    return rc;
  for (uint32_t e = 0; e < E; ++e)
    if ((rc = search(q, B, dim, k, efs[e], &rid[e * n], &rd[e * n], &rcn[(size_t)e * B]))) return rc;
  const GridParts p{B, k, tid.data(), tcn.data(), E, k, rid.data(), rd.data(), rcn.data(), 0, 0, nullptr, nullptr, nullptr};
  std::vector<float> tr(E), tp(E);
  {
    std::lock_guard<std::mutex> serial(search_mu_);  // qual_ is one block: calls take turns
    if ((rc = quality_grid_totals(ctx_, qual_, p, tr.data(), tp.data()))) return rc;
  }
  out->rows = E, out->cols = 1;
  out->avg_recall.resize(E);
  out->avg_precision.resize(E);
  for (uint32_t e = 0; e < E; ++e) {
    const SearchQuality s = quality_of(tr[e], tp[e], B, start);
    out->avg_recall[e] = s.avg_recall;
    out->avg_precision[e] = s.avg_precision;
    out->avg_query_time_ms = s.avg_query_time_ms;
  }
  out->queries_evaluated = B;
  return FVDB_OK;
}

// The layered walk on the host (:398-467) for chunks of at most 16384 queries in lock step: one scorer launch per hop
// for the whole chunk.  (Several smaller groups on a stream each, driven round-robin so that one group's hop is on the
// GPU while another's host phase runs, were measured slower: launch + stream sync cost more than the overlap wins,
// profiles/r01_hnsw_lanes.log.)  The caller holds walk_mu_ and has pulled nbrs_.
int HNSWIndex::search_host_walk(const float* q, bool q_on_device, uint32_t B, uint32_t k, uint32_t ef, uint64_t* ids,
                                float* dist, uint32_t* counts, const AllowView* view) {
  fill_empty(ids, dist, counts, B, k);
  Walk& w = search_walk_;
  w.del = view ? view->eff.data() : nullptr;
  const uint8_t* del = view ? view->eff.data() : deleted_.data();
  const uint32_t maxdeg = std::max(cfg_.max_connections, cfg_.max_connections_layer_0) + 1;
  const uint32_t step = 16384;
  for (uint32_t lo = 0; lo < B; lo += step) {
    const uint32_t n = std::min(step, B - lo);
    int rc = walk_begin(w, n, maxdeg);
    if (rc) return rc;
    rc = q_on_device ? fvdb_scorer_set_queries_dev(w.sc, q + (size_t)lo * dim_, n)
                     : fvdb_scorer_set_queries(w.sc, q + (size_t)lo * dim_, n);
    if (rc) return rc;
    uint32_t* cand = fvdb_scorer_cand_buffer(w.sc);  // distance to the entry point (:432-435)
    for (uint32_t b = 0; b < n; ++b) cand[(size_t)b * w.cap_C] = entry_;
    rc = fvdb_scorer_run(w.sc, n, 1);
    if (rc) return rc;
    n_dist_ += n;
    n_hops_ += 1;
    const float* dbuf = fvdb_scorer_dist_buffer(w.sc);
    for (uint32_t b = 0; b < n; ++b) w.qs[b].cur.assign(1, Cand{entry_, dbuf[(size_t)b * w.cap_C]});
    for (uint32_t layer = level_[entry_] + 1; layer-- > 0;) {  // :437-448: ef = 1 above layer 0
      rc = search_layer(w, n, layer == 0 ? ef : 1, layer);
      if (rc) return rc;
    }
    for (uint32_t b = 0; b < n; ++b) {  // :451-466 filter deleted, take k
      uint32_t nw = 0;
      const size_t o = (size_t)(lo + b) * k;
      for (const Cand& c : w.qs[b].cur) {
        if (!registered_[c.node] || del[c.node]) continue;
        if (nw >= k) break;
        ids[o + nw] = ids_[c.node];
        dist[o + nw] = c.distance;
        ++nw;
      }
      counts[lo + b] = nw;
    }
  }
  return FVDB_OK;
}

// distances from stored row `base_row` to a list of candidate rows (prune: :588-624)
int HNSWIndex::score_pairs_from_row(uint32_t base_row, const std::vector<uint32_t>& cands, std::vector<float>& out) {
  int rc = fvdb_scorer_set_query_rows(insert_walk_.sc, &base_row, 1);
  if (rc) return rc;
  uint32_t* cand = fvdb_scorer_cand_buffer(insert_walk_.sc);
  for (size_t i = 0; i < cands.size(); ++i) cand[i] = cands[i];
  rc = fvdb_scorer_run(insert_walk_.sc, 1, (uint32_t)cands.size());
  if (rc) return rc;
  n_dist_ += cands.size();
  n_hops_ += 1;
  const float* d = fvdb_scorer_dist_buffer(insert_walk_.sc);
  out.assign(d, d + cands.size());
  for (size_t i = 0; i < cands.size(); ++i) cand[i] = FVDB_NO_ROW;
  return FVDB_OK;
}

// --------------------------------------------------------------------------------------------
// insert (src/hnsw/core.rs:226-378)
// --------------------------------------------------------------------------------------------
// the reference's checks, in its order (:227-245); non-finite values would panic its partial_cmp().unwrap()
int HNSWIndex::check_insert(uint64_t id, const float* v, uint32_t dim) const {
  if (index_of_.count(id)) return FVDB_E_DUPLICATE;
  if (has_dim_ && dim != dim_) return FVDB_E_DIM;
  if (entry_lost_) return FVDB_E_NOT_FOUND;  // the reference unwraps the missing entry node here (:268-274)
  for (uint32_t j = 0; j < dim; ++j)
    if (!(v[j] - v[j] == 0.0f)) return FVDB_E_NONFINITE;
  return FVDB_OK;
}

bool HNSWIndex::device_insert_ok() const {
  static const bool env_off = getenv("FVDB_HNSW_DEVICE_INSERT") && atoi(getenv("FVDB_HNSW_DEVICE_INSERT")) == 0;
  return device_insert_ && !env_off && cfg_.max_connections <= 63 && cfg_.max_connections_layer_0 <= 63 &&
         cfg_.ef_construction >= 1 && cfg_.ef_construction <= 512 && dim_ <= 1024;
}

int HNSWIndex::insert(uint64_t id, const float* v, uint32_t dim, int64_t forced_level) {
  uint64_t ok = 0;
  int err = 0;
  int rc = batch_insert(&id, v, 1, dim, &forced_level, &ok, &err);
  return rc ? rc : err;
}

int HNSWIndex::append_nodes(const uint64_t* ids, const uint32_t* levels, const float* v, uint32_t m, uint32_t* first) {
  uint64_t first64 = 0;
  int rc = fvdb_store_append(store_, v, m, &first64);  // the vectors are resident before the graph links to them
  if (rc) return rc;
  *first = (uint32_t)first64;
  host_vecs_.insert(host_vecs_.end(), v, v + (size_t)m * dim_);
  for (uint32_t j = 0; j < m; ++j) {
    ids_.push_back(ids[j]);
    level_.push_back(levels[j]);
    deleted_.push_back(0);
    registered_.push_back(0);  // "not yet in the nodes map" while its links are being made (:370)
    nbrs_.emplace_back(levels[j] + 1);
  }
  return FVDB_OK;
}

void HNSWIndex::finalize_insert(uint32_t row) {  // "nodes.insert(id, node)" (:367-370)
  index_of_[ids_[row]] = row;
  registered_[row] = 1;
  n_registered_ += 1;
}

template <class L>
int HNSWIndex::adopt_nodes(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const L* levels) {
  dim_ = dim;
  has_dim_ = true;
  int rc = ensure_store(dim);
  if (rc) return rc;
  uint64_t first = 0;
  rc = fvdb_store_append(store_, v, n, &first);
  if (rc) return rc;
  host_vecs_.assign(v, v + n * dim);
  ids_.assign(ids, ids + n);
  level_.resize(n);
  for (uint64_t i = 0; i < n; ++i) level_[i] = levels ? (uint32_t)levels[i] : (uint32_t)assign_level();
  deleted_.assign(n, 0);
  registered_.assign(n, 1);
  n_registered_ = n;
  index_of_.reserve(n * 2);
  for (uint64_t i = 0; i < n; ++i) index_of_[ids[i]] = (uint32_t)i;
  nbrs_.assign(n, {});
  for (uint64_t i = 0; i < n; ++i) nbrs_[i].resize(level_[i] + 1);
  return FVDB_OK;
}

void HNSWIndex::add_insert_stats(const fvdb_graph_insert_stats& st) {
  insert_stats_.n_done += st.n_done;
  insert_stats_.speculated_ok += st.speculated_ok;
  insert_stats_.searched_in_commit += st.searched_in_commit;
  insert_stats_.commit_stops += st.commit_stops;
  insert_stats_.rounds += st.rounds;
  insert_stats_.expanded += st.expanded;
  insert_stats_.rows_scored += st.rows_scored;
  insert_stats_.tie_restarts += st.tie_restarts;
  insert_stats_.launches += st.launches;
  n_dist_ += st.rows_scored;  // of the searches the commit workgroup ran (speculated ones are not counted)
  n_hops_ += st.rounds;
}

int HNSWIndex::batch_insert(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const int64_t* levels, uint64_t* n_ok,
                            int* first_error) {
  if (n_ok) *n_ok = 0;
  if (first_error) *first_error = 0;
  uint64_t ok = 0;
  int err = 0;
  auto finish = [&](int rc) {
    if (n_ok) *n_ok = ok;
    if (first_error) *first_error = err;
    return rc;
  };
  std::vector<float> rounded;  // fp16 rows: the checks, the store and host_vecs_ all see the rounded values
  v = rows_at_the_door(cfg_.row_dtype, v, n * dim, rounded);
  for (uint64_t at = 0; at < n;) {
    // the next run of inserts that pass the reference's checks (a failed insert draws no level and changes nothing)
    std::vector<uint64_t> acc;
    std::unordered_set<uint64_t> in_run;
    uint64_t end = at;
    for (; end < n && acc.size() < (1u << 20); ++end) {
      int rc = check_insert(ids[end], v + end * dim, dim);
      if (!rc && in_run.count(ids[end])) rc = FVDB_E_DUPLICATE;
      if (rc) {
        if (!err) err = rc;
        continue;
      }
      if (!has_dim_) {
        dim_ = dim;
        has_dim_ = true;
      }
      in_run.insert(ids[end]);
      acc.push_back(end);
    }
    at = end;
    if (acc.empty()) continue;
    if (!device_insert_ok()) {
      for (uint64_t i : acc) {
        int rc = insert_host(ids[i], v + i * dim, dim, levels ? levels[i] : -1);
        if (rc == 0) ++ok;
        else if (!err) err = rc;
      }
      continue;
    }
    static const bool dbg = getenv("FVDB_BUILD_DEBUG") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t_a = now();
    int rc = ensure_store(dim);
    if (rc) return finish(rc);
    rc = sync_graph();  // the device rows must be current before they are edited in place
    if (rc) return finish(rc);
    const auto t_b = now();
    const uint32_t m = (uint32_t)acc.size();
    std::vector<uint32_t> lv(m);
    std::vector<uint64_t> run_ids(m);
    for (uint32_t j = 0; j < m; ++j) {
      const int64_t f = levels ? levels[acc[j]] : -1;
      lv[j] = f >= 0 ? (uint32_t)f : (uint32_t)assign_level();
      run_ids[j] = ids[acc[j]];
    }
    // vectors: one upload
    const float* src = v + acc[0] * dim;
    std::vector<float> packed;
    if (acc.back() - acc[0] + 1 != m) {
      packed.resize((size_t)m * dim);
      for (uint32_t j = 0; j < m; ++j) std::memcpy(&packed[(size_t)j * dim], v + acc[j] * dim, (size_t)dim * 4);
      src = packed.data();
    }
    uint32_t first = 0;
    rc = append_nodes(run_ids.data(), lv.data(), src, m, &first);
    if (rc) return finish(rc);
    const auto t_c = now();
    rc = fvdb_graph_append_nodes(graph_, first, m, lv.data());
    if (rc) return finish(rc);
    const auto t_d = now();
    uint32_t done = 0;
    while (done < m) {
      uint32_t nd = 0;
      fvdb_graph_insert_stats st{};
      rc = fvdb_graph_insert_linked(graph_, first + done, m - done, cfg_.ef_construction, insert_mode_, &nd, &st);
      if (rc == FVDB_E_UNSUPPORTED) {  // e.g. an LDS budget that holds neither form of `visited`: the host algorithm links
        rc = FVDB_OK;                  // this node (rows patched into HBM), and the question is asked again for the next
        nd = 0;
        st.needs_host = 1;
        if (!host_link_reported_) {    // a few hundred inserts/s instead of thousands: said once per index, not per node
          fprintf(stderr, "[fvdb] HNSWIndex: the device insert refused the graph (%s); nodes are linked by the host algorithm\n",
                  fvdb_last_error(ctx_));
          host_link_reported_ = true;
        }
      }
      if (rc) return finish(rc);
      add_insert_stats(st);
      for (uint32_t j = 0; j < nd; ++j) finalize_insert(first + done + j);
      done += nd;
      dev_ahead_ = dev_ahead_ || nd > 0;
      uint32_t e = FVDB_NO_ROW;
      fvdb_graph_entry(graph_, &e, nullptr);
      if (e != FVDB_NO_ROW) {
        entry_ = e;
        has_entry_ = true;
      }
      if (done < m && st.needs_host) {  // level >= 16 or an on-chip heap outgrown: this node takes the host algorithm
        rc = ensure_host_graph();
        if (rc) return finish(rc);
        rc = link_and_publish(first + done, true);
        if (rc) return finish(rc);
        done += 1;
      } else if (nd == 0 && done < m) {
        return finish(FVDB_E_HIP);  // no progress and no request for the host path: never expected
      }
    }
    ok += m;
    if (dbg)
      fprintf(stderr, "[batch_insert] %u rows: graph sync %.1f ms, vectors + host bookkeeping %.1f ms, node append %.1f ms, linking %.1f ms\n", m,
              ms(t_a, t_b), ms(t_b, t_c), ms(t_c, t_d), ms(t_d, now()));
  }
  return finish(FVDB_OK);
}

// one insert by the host algorithm (the other mode; also dims / degree caps the device insert does not take)
int HNSWIndex::insert_host(uint64_t id, const float* v, uint32_t dim, int64_t forced_level) {
  int rc = ensure_store(dim);
  if (rc) return rc;
  rc = ensure_host_graph();
  if (rc) return rc;
  const uint32_t level = forced_level >= 0 ? (uint32_t)forced_level : (uint32_t)assign_level();
  uint32_t row = 0;
  rc = append_nodes(&id, &level, v, 1, &row);
  if (rc) return rc;
  return link_and_publish(row, false);
}

int HNSWIndex::link_and_publish(uint32_t row, bool on_device) {
  std::vector<std::pair<uint32_t, uint32_t>> touched;
  int rc = link_host(row, &touched);
  if (rc) return rc;
  finalize_insert(row);
  n_host_inserts_ += 1;
  if (!graph_ || host_ahead_) {  // no device copy that agrees with nbrs_: the next device use installs the whole graph
    host_ahead_ = true;
    return FVDB_OK;
  }
  // the device copy agrees with nbrs_ up to this insert: patch the rows `touched` (node, layer) into it
  if (!on_device) {
    rc = fvdb_graph_append_nodes(graph_, row, 1, &level_[row]);
    if (rc) return rc;
  }
  std::vector<uint32_t> nodes, layers, off{0}, flat;
  for (const auto& t : touched) {
    nodes.push_back(t.first);
    layers.push_back(t.second);
    const auto& l = nbrs_[t.first][t.second];
    flat.insert(flat.end(), l.begin(), l.end());
    off.push_back((uint32_t)flat.size());
  }
  if (flat.empty()) flat.push_back(0);
  rc = fvdb_graph_set_lists(graph_, (uint32_t)nodes.size(), nodes.data(), layers.data(), off.data(), flat.data());
  if (rc) return rc;
  return fvdb_graph_set_entry(graph_, entry_, row + 1);
}

int HNSWIndex::link_host(uint32_t row, std::vector<std::pair<uint32_t, uint32_t>>* touched) {
  const uint32_t level = level_[row];
  bool is_first = false;
  if (!has_entry_) {
    has_entry_ = true;
    entry_ = row;
    is_first = true;
  }
  for (uint32_t lc = 0; lc <= level; ++lc) touched->push_back({row, lc});
  uint32_t entry_level = 0;
  int rc = FVDB_OK;
  if (!is_first) {
    const uint32_t ep = entry_;
    entry_level = level_[ep];
    const uint32_t maxdeg = std::max(cfg_.max_connections, cfg_.max_connections_layer_0) + 1;
    Walk& w = insert_walk_;
    rc = walk_begin(w, 1, maxdeg);
    if (rc) return rc;
    std::vector<float> d0;
    rc = score_pairs_from_row(row, {ep}, d0);  // also loads the new vector as the scorer's query
    if (rc) return rc;
    std::vector<Cand>& res = w.qs[0].cur;  // search_layer's entry going in, its result coming out
    res.assign(1, Cand{ep, d0[0]});
    const uint32_t search_level = std::min(level, entry_level);
    for (uint32_t lc = search_level + 1; lc-- > 0;) {  // :284-290
      rc = search_layer(w, 1, 1, lc);
      if (rc) return rc;
    }
    const std::vector<Cand> current_nearest = res;
    for (uint32_t lc = 0; lc <= level; ++lc) {  // :293-362
      const uint32_t m = cap(lc);
      const Cand start = (lc <= search_level && !current_nearest.empty()) ? current_nearest[0] : Cand{ep, d0[0]};
      res.assign(1, start);
      rc = search_layer(w, 1, cfg_.ef_construction, lc);
      if (rc) return rc;
      std::vector<uint32_t> chosen;  // select_neighbors :556-558
      for (size_t i = 0; i < res.size() && i < m; ++i) chosen.push_back(res[i].node);
      for (uint32_t nbv : chosen) set_insert(nbrs_[row][lc], nbv);
      std::vector<uint32_t> to_prune;
      for (uint32_t nbv : chosen) {
        if (!registered_[nbv]) continue;
        if (level_[nbv] >= lc) {
          set_insert(nbrs_[nbv][lc], row);
          touched->push_back({nbv, lc});
          if (nbrs_[nbv][lc].size() > m) to_prune.push_back(nbv);
        }
      }
      for (uint32_t nbv : to_prune) {  // prune_neighbors_with_new_node :588-624
        const std::vector<uint32_t> list = nbrs_[nbv][lc];
        std::vector<float> ds;
        rc = score_pairs_from_row(nbv, list, ds);
        if (rc) return rc;
        std::vector<Cand> cs(list.size());
        for (size_t i = 0; i < list.size(); ++i) cs[i] = {list[i], ds[i]};
        std::stable_sort(cs.begin(), cs.end(), [](const Cand& a, const Cand& c) { return a.distance < c.distance; });
        if (cs.size() > m) cs.resize(m);
        nbrs_[nbv][lc].clear();
        for (const Cand& c : cs) set_insert(nbrs_[nbv][lc], c.node);
      }
      if (!to_prune.empty()) {  // put the new vector back as the query for the next layer
        rc = fvdb_scorer_set_query_rows(insert_walk_.sc, &row, 1);
        if (rc) return rc;
      }
    }
  }
  if (!is_first && level > entry_level) entry_ = row;  // :372-375
  return FVDB_OK;
}

// --------------------------------------------------------------------------------------------
// graph install / export, bulk build
// --------------------------------------------------------------------------------------------
int HNSWIndex::restore(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const uint32_t* levels,
                       const uint64_t* nbr_offsets, const uint64_t* nbrs, uint64_t entry_id) {
  if (!ids_.empty()) return FVDB_E_INVALID;
  if (n == 0) return FVDB_OK;
  std::vector<float> rounded;
  v = rows_at_the_door(cfg_.row_dtype, v, n * dim, rounded);
  int rc = adopt_nodes(ids, v, n, dim, levels);
  if (rc) return rc;
  uint64_t slot = 0;
  for (uint64_t i = 0; i < n; ++i) {
    for (uint32_t l = 0; l <= levels[i]; ++l, ++slot) {
      auto& s = nbrs_[i][l];
      for (uint64_t e = nbr_offsets[slot]; e < nbr_offsets[slot + 1]; ++e) {
        auto it = index_of_.find(nbrs[e]);
        if (it == index_of_.end()) return FVDB_E_NOT_FOUND;
        s.push_back(it->second);
      }
    }
  }
  auto it = index_of_.find(entry_id);
  if (it == index_of_.end()) return FVDB_E_NOT_FOUND;
  entry_ = it->second;
  has_entry_ = true;
  host_ahead_ = true;
  return FVDB_OK;
}

// src/hnsw/operations.rs:176-200: deleted nodes leave the node map and every neighbour set.  The reference does not
// repair an entry point that was removed: its searches then fail and its insert panics.  `registered_ == 0` is this
// mirror's "nodes.get() == None" for a node whose rows are still held (host form, keep-rows form); the resident job
// drops such nodes for good, together with the ones it removes itself (fvdb_host.hpp).
int HNSWIndex::vacuum(uint64_t* removed_out) {
  if (removed_out) *removed_out = 0;
  std::vector<uint8_t> dead(ids_.size(), 0);
  uint64_t removed = 0;
  for (size_t i = 0; i < ids_.size(); ++i)
    if (registered_[i] && deleted_[i]) {
      dead[i] = 1;
      ++removed;
    }
  if (removed == 0) return FVDB_OK;
  int rc;
  bool resident = resident_vacuum_ && graph_ != nullptr;
  if (resident && host_ahead_) {  // the device copy is brought up to date first; a graph it cannot hold takes the host form
    rc = sync_graph();
    if (rc == FVDB_E_UNSUPPORTED) resident = false;
    else if (rc) return rc;
  }
  if (resident) {
    const bool entry_dead = has_entry_ && deleted_[entry_];  // removed now, or by an earlier vacuum (entry_lost_): the numbering stays
    uint32_t flags = (vacuum_keep_rows_ || entry_dead) ? FVDB_VACUUM_KEEP_ROWS : 0u;
    rc = fvdb_graph_vacuum(graph_, flags, nullptr);
    if (rc == FVDB_E_OOM && flags == 0) {  // no room for the second copy: a vacuum that worked before still works
      flags = FVDB_VACUUM_KEEP_ROWS;
      rc = fvdb_graph_vacuum(graph_, flags, nullptr);
    }
    if (rc && rc != FVDB_E_UNSUPPORTED) return rc;
    if (rc == FVDB_OK) {
      fvdb_graph_maintenance_info(graph_, &vacuum_info_);
      vacuum_path_ = flags ? VACUUM_RESIDENT_KEEP_ROWS : VACUUM_RESIDENT;
      vacuum_adopt(flags == 0, dead);
      n_registered_ -= removed;
      if (removed_out) *removed_out = removed;
      return FVDB_OK;
    }
  }
  if ((rc = ensure_host_graph())) return rc;
  vacuum_host(dead, removed);
  if (removed_out) *removed_out = removed;
  return FVDB_OK;
}

uint64_t HNSWIndex::vacuum_host(const std::vector<uint8_t>& dead, uint64_t removed) {
  for (size_t i = 0; i < ids_.size(); ++i) {
    if (dead[i]) {
      registered_[i] = 0;
      auto it = index_of_.find(ids_[i]);
      if (it != index_of_.end() && it->second == i) index_of_.erase(it);
      for (auto& l : nbrs_[i]) l.clear();
    } else if (registered_[i]) {
      for (auto& l : nbrs_[i])
        l.erase(std::remove_if(l.begin(), l.end(), [&](uint32_t x) { return dead[x] != 0; }), l.end());
    }
  }
  n_registered_ -= removed;
  if (has_entry_ && dead[entry_]) entry_lost_ = true;
  host_ahead_ = true;
  vacuum_path_ = VACUUM_HOST;
  vacuum_info_ = fvdb_graph_maintenance_info_t{};
  return removed;
}

// The device job has pruned the lists (and, `reclaimed`, renumbered the nodes: new index = undeleted nodes before it).
// The lists now exist on the device only: whoever needs nbrs_ pulls them, as after a device insert.
void HNSWIndex::vacuum_adopt(bool reclaimed, const std::vector<uint8_t>& dead) {
  {
    std::lock_guard<std::mutex> lk(view_mu_);  // the cached allow view names node indices and a mask that is now stale
    view_.reset();
    view_key_.clear();
  }
  const size_t n = ids_.size();
  if (!reclaimed) {
    for (size_t i = 0; i < n; ++i)
      if (dead[i]) {
        registered_[i] = 0;
        auto it = index_of_.find(ids_[i]);
        if (it != index_of_.end() && it->second == i) index_of_.erase(it);
      }
    if (has_entry_ && dead[entry_]) entry_lost_ = true;
  } else {
    // every deleted node goes: the ones removed now and those an earlier host-form or keep-rows vacuum left behind
    size_t w = 0;
    uint32_t entry = entry_;
    index_of_.clear();
    for (size_t i = 0; i < n; ++i) {
      if (deleted_[i]) continue;
      if (has_entry_ && i == entry_) entry = (uint32_t)w;
      if (w != i) {
        ids_[w] = ids_[i];
        level_[w] = level_[i];
        registered_[w] = registered_[i];
        std::memmove(&host_vecs_[w * dim_], &host_vecs_[i * dim_], (size_t)dim_ * 4);
      }
      if (registered_[w]) index_of_[ids_[w]] = (uint32_t)w;
      ++w;
    }
    ids_.resize(w);
    level_.resize(w);
    registered_.resize(w);
    deleted_.assign(w, 0);
    host_vecs_.resize(w * dim_);
    host_vecs_.shrink_to_fit();
    entry_ = entry;
  }
  nbrs_.assign(ids_.size(), {});
  for (size_t i = 0; i < ids_.size(); ++i) nbrs_[i].resize(level_[i] + 1);
  dev_ahead_ = true;
}

uint64_t HNSWIndex::graph_slots() const {
  uint64_t s = 0;
  for (size_t i = 0; i < ids_.size(); ++i)
    if (registered_[i]) s += level_[i] + 1;
  return s;
}
uint64_t HNSWIndex::graph_edges() {
  if (ensure_host_graph()) return 0;
  uint64_t e = 0;
  for (const auto& n : nbrs_)
    for (const auto& l : n) e += l.size();
  return e;
}
void HNSWIndex::export_graph(uint64_t* ids, uint32_t* levels, uint64_t* nbr_offsets, uint64_t* nbrs) {
  (void)ensure_host_graph();
  uint64_t slot = 0, e = 0, w = 0;
  for (size_t i = 0; i < ids_.size(); ++i) {
    if (!registered_[i]) continue;  // vacuumed
    ids[w] = ids_[i];
    levels[w++] = level_[i];
    for (uint32_t l = 0; l <= level_[i]; ++l, ++slot) {
      nbr_offsets[slot] = e;
      for (uint32_t x : nbrs_[i][l]) nbrs[e++] = ids_[x];
    }
  }
  nbr_offsets[slot] = e;
}

// --------------------------------------------------------------------------------------------
// graph stats and health (the definitions are stated in include/fvdb.h, fvdb_graph_health)
// --------------------------------------------------------------------------------------------
// src/hnsw/core.rs:667-670 and :673-684: every node the map holds, deleted ones included
uint32_t HNSWIndex::get_max_level() const {
  uint32_t m = 0;
  for (size_t i = 0; i < ids_.size(); ++i)
    if (registered_[i]) m = std::max(m, level_[i]);
  return m;
}
void HNSWIndex::get_level_distribution(uint64_t* out) const {
  const uint32_t m = get_max_level();
  std::fill(out, out + m + 1, 0);
  for (size_t i = 0; i < ids_.size(); ++i)
    if (registered_[i])
      for (uint32_t l = 0; l <= level_[i]; ++l) out[l] += 1;
}

// src/hnsw/operations.rs:227-272 from the census part of the health job
int HNSWIndex::get_graph_stats(GraphStats* out) {
  *out = GraphStats{};
  fvdb_graph_health_t h;
  int rc = graph_health(&h, FVDB_HEALTH_SKIP_REACH | FVDB_HEALTH_SKIP_COMPONENTS);
  if (rc) return rc;
  if (h.n_live == 0) return FVDB_OK;
  out->total_nodes = h.n_live;
  out->total_edges = h.edge_slots_live / 2;  // "Since edges are bidirectional, divide by 2"
  out->avg_degree = (float)(out->total_edges * 2) / (float)out->total_nodes;
  out->max_layer = h.max_level_live;
  out->connected_components = 1;  // the reference's stub: "assume 1 component"
  return FVDB_OK;
}

// the definitions once more, in plain host code over nbrs_ (pulled by the caller)
void HNSWIndex::health_host(uint32_t flags, fvdb_graph_health_t* out, std::vector<uint8_t>* reached, std::vector<uint32_t>* label) const {
  const uint32_t n = (uint32_t)ids_.size();
  auto live = [&](uint32_t u) { return registered_[u] && !deleted_[u]; };
  for (uint32_t u = 0; u < n; ++u) {
    if (!live(u)) continue;
    out->n_live += 1;
    out->max_level_live = std::max(out->max_level_live, level_[u]);
    for (uint32_t l = 0; l <= level_[u]; ++l) {
      uint64_t dead = 0;
      for (uint32_t v : nbrs_[u][l]) dead += live(v) ? 0 : 1;
      out->edge_slots_live += nbrs_[u][l].size();
      out->dangling += dead;
      if (l == 0) {
        out->dangling0 += dead;
        out->degree0_hist[std::min<size_t>(nbrs_[u][0].size(), 64)] += 1;
      }
    }
  }
  const bool entry_ok = has_entry_ && !entry_lost_ && entry_ < n;
  out->has_entry = entry_ok;
  out->entry_live = entry_ok && live(entry_);
  out->entry_level = entry_ok ? level_[entry_] : 0;
  if (!(flags & FVDB_HEALTH_SKIP_REACH)) {
    std::vector<uint8_t> in(n, 0);
    std::vector<uint32_t> all, frontier, next;
    if (entry_ok) {
      in[entry_] = 1;
      all.push_back(entry_);
      for (uint32_t l = level_[entry_] + 1; l-- > 0;) {
        frontier = all;  // what the layer above left seeds this one
        while (!frontier.empty()) {
          if (l == 0) out->reach_rounds0 += 1;
          next.clear();
          for (uint32_t u : frontier) {
            if (level_[u] < l || !(live(u) || u == entry_)) continue;
            for (uint32_t v : nbrs_[u][l])
              if (live(v) && !in[v]) {
                in[v] = 1;
                next.push_back(v);
              }
          }
          all.insert(all.end(), next.begin(), next.end());
          frontier.swap(next);
        }
      }
    }
    for (uint32_t u : all) out->reachable_live += live(u) ? 1 : 0;
    out->unreachable_live = out->n_live - out->reachable_live;
    if (reached) reached->swap(in);
  }
  if (!(flags & FVDB_HEALTH_SKIP_COMPONENTS)) {
    std::vector<uint32_t> parent(n), size(n, 0);
    for (uint32_t u = 0; u < n; ++u) parent[u] = u;
    auto find = [&](uint32_t x) {
      while (parent[x] != x) x = parent[x] = parent[parent[x]];
      return x;
    };
    for (uint32_t u = 0; u < n; ++u) {
      if (!live(u)) continue;
      for (uint32_t v : nbrs_[u][0]) {
        if (!live(v)) continue;
        const uint32_t a = find(u), b = find(v);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);  // a root is the smallest index of its tree
      }
    }
    std::vector<uint32_t> lab(n, 0xFFFFFFFFu);
    for (uint32_t u = 0; u < n; ++u)
      if (live(u)) size[lab[u] = find(u)] += 1;
    for (uint32_t u = 0; u < n; ++u)
      if (lab[u] == u) {
        out->components0 += 1;
        out->isolated0 += size[u] == 1 ? 1 : 0;
        out->largest_component0 = std::max(out->largest_component0, size[u]);
      }
    if (label) label->swap(lab);
  }
}

int HNSWIndex::health_run(uint32_t flags, fvdb_graph_health_t* out, int* path, std::vector<uint8_t>* reached, std::vector<uint32_t>* label) {
  std::memset(out, 0, sizeof *out);
  if (path) *path = HEALTH_NONE;
  if (flags & ~(FVDB_HEALTH_SKIP_REACH | FVDB_HEALTH_SKIP_COMPONENTS)) return FVDB_E_INVALID;
  const uint32_t n = (uint32_t)ids_.size();
  const bool want_reach = !(flags & FVDB_HEALTH_SKIP_REACH), want_comp = !(flags & FVDB_HEALTH_SKIP_COMPONENTS);
  bool device = device_traversal_ && n > 0;
  int rc;
  if (device) {
    rc = sync_graph();  // uploads when host_ahead_
    if (rc == FVDB_E_UNSUPPORTED) device = false;
    else if (rc) return rc;
  }
  if (device) {
    // an entry point lost to a vacuum still has its (emptied, deleted) node on the device: no search starts there
    const uint32_t dev_flags = flags | (entry_lost_ ? FVDB_HEALTH_SKIP_REACH : 0u);
    if ((rc = fvdb_graph_health(graph_, dev_flags, out))) return rc;
    if (entry_lost_) {
      out->has_entry = out->entry_live = out->entry_level = 0;
      if (want_reach) out->unreachable_live = out->n_live;
    }
    if (reached && want_reach) {
      reached->assign(n, 0);
      if (!entry_lost_ && (rc = fvdb_graph_health_nodes(graph_, reached->data(), nullptr))) return rc;
    }
    if (label && want_comp) {
      label->assign(n, 0xFFFFFFFFu);
      if ((rc = fvdb_graph_health_nodes(graph_, nullptr, label->data()))) return rc;
    }
    if (path) *path = HEALTH_DEVICE;
  } else {
    if ((rc = ensure_host_graph())) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    health_host(flags, out, reached, label);
    out->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();  // wall clock: no device job ran
    if (path) *path = HEALTH_HOST;
  }
  out->n_nodes = (uint32_t)n_registered_;
  return FVDB_OK;
}

int HNSWIndex::graph_health(fvdb_graph_health_t* out, uint32_t flags, int* path) { return health_run(flags, out, path, nullptr, nullptr); }

int HNSWIndex::unreachable(std::vector<uint64_t>* ids_out) {
  ids_out->clear();
  fvdb_graph_health_t h;
  std::vector<uint8_t> reached;
  int rc = health_run(FVDB_HEALTH_SKIP_COMPONENTS, &h, nullptr, &reached, nullptr);
  if (rc) return rc;
  for (size_t u = 0; u < ids_.size(); ++u)
    if (registered_[u] && !deleted_[u] && !reached[u]) ids_out->push_back(ids_[u]);
  return FVDB_OK;
}

int HNSWIndex::component_labels(uint64_t* labels_out) {
  fvdb_graph_health_t h;
  std::vector<uint32_t> label;
  int rc = health_run(FVDB_HEALTH_SKIP_REACH, &h, nullptr, nullptr, &label);
  if (rc) return rc;
  uint64_t w = 0;
  for (size_t u = 0; u < ids_.size(); ++u) {
    if (!registered_[u]) continue;
    labels_out[w++] = label[u] < ids_.size() ? ids_[label[u]] : UINT64_MAX;
  }
  return FVDB_OK;
}

int HNSWIndex::bulk_build(const uint64_t* ids, const float* v, uint64_t n, uint32_t dim, const int64_t* levels) {
  if (!ids_.empty()) return FVDB_E_INVALID;
  if (n == 0) return FVDB_OK;
  if (n >= 0xFFFFFFFFull) return FVDB_E_UNSUPPORTED;
  std::vector<float> rounded;
  v = rows_at_the_door(cfg_.row_dtype, v, n * dim, rounded);
  {
    std::unordered_set<uint64_t> seen;
    seen.reserve(n * 2);
    for (uint64_t i = 0; i < n; ++i)
      if (!seen.insert(ids[i]).second) return FVDB_E_DUPLICATE;
  }
  int rc = adopt_nodes(ids, v, n, dim, levels);
  if (rc) return rc;
  const uint32_t maxlevel = *std::max_element(level_.begin(), level_.end());
  // entry = earliest node carrying the maximum level (what sequential insertion ends with, :372-375)
  for (uint64_t i = 0; i < n; ++i)
    if (level_[i] == maxlevel) {
      entry_ = (uint32_t)i;
      break;
    }
  has_entry_ = true;

  std::vector<float> zero(dim, 0.0f);
  for (uint32_t l = 0; l <= maxlevel; ++l) {
    std::vector<uint32_t> members;
    for (uint64_t i = 0; i < n; ++i)
      if (level_[i] >= l) members.push_back((uint32_t)i);
    if (members.size() < 2) continue;
    const uint32_t kk = (uint32_t)std::min<uint64_t>(cap(l), members.size() - 1);
    const uint32_t k = kk + 1;  // the member itself comes back at distance 0
    if (k > FVDB_MAX_K) return FVDB_E_UNSUPPORTED;
    fvdb_ivf* flat = nullptr;
    rc = fvdb_ivf_create(ctx_, dim, 1, &flat);
    if (rc) return rc;
    rc = fvdb_ivf_set_centroids(flat, zero.data());
    std::vector<float> mv;
    std::vector<uint64_t> mid(members.size());
    std::vector<uint32_t> mcl(members.size(), 0);
    const float* src = v;
    if (rc == FVDB_OK && members.size() != n) {
      mv.resize(members.size() * (size_t)dim);
      for (size_t j = 0; j < members.size(); ++j)
        std::memcpy(&mv[j * dim], v + (size_t)members[j] * dim, dim * sizeof(float));
      src = mv.data();
    }
    for (size_t j = 0; j < members.size(); ++j) mid[j] = members[j];
    if (rc == FVDB_OK) rc = fvdb_ivf_add_assigned(flat, src, mid.data(), members.size(), mcl.data(), nullptr);
    const uint32_t step = 16384;
    std::vector<uint64_t> oi((size_t)step * k);
    std::vector<float> od((size_t)step * k);
    std::vector<uint32_t> oc(step);
    for (size_t o = 0; rc == FVDB_OK && o < members.size(); o += step) {
      const uint32_t b = (uint32_t)std::min<size_t>(step, members.size() - o);
      rc = fvdb_ivf_search_all(flat, src + o * dim, b, k, oi.data(), od.data(), oc.data());
      if (rc) break;
      for (uint32_t i = 0; i < b; ++i) {
        const uint32_t self = members[o + i];
        auto& s = nbrs_[self][l];
        for (uint32_t e = 0; e < oc[i] && s.size() < kk; ++e) {
          const uint32_t nbv = (uint32_t)oi[(size_t)i * k + e];
          if (nbv != self) s.push_back(nbv);
        }
      }
    }
    fvdb_ivf_destroy(flat);
    if (rc) return rc;
  }
  host_ahead_ = true;
  return FVDB_OK;
}

}  // namespace fvdbh
