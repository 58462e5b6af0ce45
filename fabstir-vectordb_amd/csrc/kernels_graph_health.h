// kernels_graph_health.h — a read-only job over the adjacency in HBM: what any search can still
// reach after deletes and vacuums, the weak components of the live layer-0 graph, degree and dangling-link figures.
// The reference's own get_graph_stats (src/hnsw/operations.rs:227-272) reports "1 component" from a stub; the rules
// restated here are read off search / search_layer (src/hnsw/core.rs:398-554: a deleted neighbour is marked visited and
// never expanded, :510-513; a deleted entry point is still seeded and expanded).  No vector row is read: the job does
// not depend on d or on the row dtype.  gfx950, wave64.  A row is [count, neighbours ...] at a fixed stride; a row
// longer than one wave is walked in chunks of 64, as gm_prune does.
//
//   gh_census    one wave per LIVE node, its rows layer by layer, lane i holding neighbour i: the lane loads the
//                neighbour's deleted flag and a ballot counts the entries that name deleted nodes; figures are summed
//                per workgroup in LDS (the degree histogram too), then one integer atomic per figure per workgroup
//   gh_seed      the entry point into the reach bitmap and the reach list
//   gh_reach_wide    one step of the layer's closure, one wave per frontier node: the lane of a live neighbour does
//                atomicOr on the bitmap word, a lane whose bit was newly set appends its node to the reach list — one
//                atomicAdd per wave (ballot, popcount, lane rank).  Steps are separated by kernel boundaries.
//   gh_reach_narrow  ONE workgroup runs step after step (barriers between them) while the frontier fits its LDS queue;
//                it stops when the frontier is empty or has outgrown the queue.  A path-like graph is one launch.
//   uf_init / uf_union / uf_label / uf_summary   lock-free union-find: a live-live layer-0 pair is united by linking the
//                LARGER root under the smaller with atomicCAS (so a root is the minimum index of its tree), parents are
//                read with agent-scope atomic loads; labels and sizes in a launch of their own; roots, the largest size
//                and the singletons by ballots and one atomic per workgroup.
//
// The reach list is append-only: a node enters it once, when its bit is first set, so n entries bound it.  The frontier
// of a step is the segment the step before appended; the frontier a layer starts with is the whole list ("whatever is in
// R when layer l finishes seeds layer l - 1").
#pragma once
#include "common.h"
#include "wave_ops.h"

namespace fvdb {

constexpr uint32_t kGhNone = 0xFFFFFFFFu;
constexpr uint32_t kGhQueue = 1024;       // nodes the narrow loop's LDS queue holds (two of them: 8 KiB)
constexpr uint32_t kGhNarrowThreads = 1024;
// counters (unsigned long long each)
enum : uint32_t { kGhLive = 0, kGhSlots, kGhDangling, kGhDangling0, kGhMaxLevel, kGhComponents, kGhLargest, kGhIsolated, kGhHist, kGhCounters = kGhHist + 65 };
// reach state (uint32 each): list length; where the last frontier starts in the list; steps the last narrow launch ran
enum : uint32_t { kGhTail = 0, kGhFrontier, kGhSteps, kGhStateWords = 4 };

struct GhGraph {
  const uint32_t* adj0;  // [n][stride0]
  const uint32_t* adjU;  // [u_rows][strideU]
  const uint32_t* level;
  const uint32_t* deleted;
  const uint32_t* ubase;
  uint32_t n, u_rows, stride0, strideU;
};

// the stored list of node u on layer l (nullptr: the layout holds no such row), its length clamped to the stride
__device__ __forceinline__ const uint32_t* gh_row(const GhGraph& g, uint32_t u, uint32_t l, uint32_t* cnt) {
  const uint32_t* row;
  uint32_t cap;
  if (l == 0) {
    row = g.adj0 + (size_t)u * g.stride0;
    cap = g.stride0 - 1;
  } else {
    const uint32_t r = g.ubase[u] + l - 1;
    if (r >= g.u_rows) {
      *cnt = 0;
      return nullptr;
    }
    row = g.adjU + (size_t)r * g.strideU;
    cap = g.strideU - 1;
  }
  const uint32_t c = row[0];
  *cnt = c < cap ? c : cap;
  return row;
}

__global__ __launch_bounds__(256) void gh_census_kernel(const GhGraph g, unsigned long long* __restrict__ counters) {
  __shared__ uint32_t s_hist[65];
  __shared__ unsigned long long s_acc[4];  // live, slots, dangling, dangling0
  __shared__ uint32_t s_maxlevel;
  const uint32_t lane = threadIdx.x & 63;
  if (threadIdx.x < 65) s_hist[threadIdx.x] = 0;
  if (threadIdx.x < 4) s_acc[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_maxlevel = 0;
  __syncthreads();
  unsigned long long live = 0, slots = 0, dang = 0, dang0 = 0;
  uint32_t maxlevel = 0;
  const uint32_t waves = gridDim.x * 4;
  for (uint32_t u = blockIdx.x * 4 + (threadIdx.x >> 6); u < g.n; u += waves) {
    if (g.deleted[u] != 0u) continue;  // wave-uniform
    const uint32_t lv = g.level[u];
    live += 1;
    maxlevel = lv > maxlevel ? lv : maxlevel;
    for (uint32_t l = 0; l <= lv; ++l) {
      uint32_t cnt;
      const uint32_t* row = gh_row(g, u, l, &cnt);
      uint32_t dead = 0;
      for (uint32_t base = 0; base < cnt; base += 64) {
        const uint32_t e = base + lane;
        const uint32_t nb = e < cnt ? row[1 + e] : kGhNone;
        const bool gone = nb < g.n && g.deleted[nb] != 0u;
        dead += (uint32_t)__popcll(__ballot(gone));
      }
      slots += cnt;
      dang += dead;
      if (l == 0) {
        dang0 += dead;
        if (lane == 0) atomicAdd(&s_hist[cnt < 64 ? cnt : 64], 1u);
      }
    }
  }
  if (lane == 0) {
    if (live) {
      atomicAdd(&s_acc[0], live);
      atomicMax(&s_maxlevel, maxlevel);
    }
    if (slots) atomicAdd(&s_acc[1], slots);
    if (dang) atomicAdd(&s_acc[2], dang);
    if (dang0) atomicAdd(&s_acc[3], dang0);
  }
  __syncthreads();
  if (threadIdx.x < 65 && s_hist[threadIdx.x]) atomicAdd(&counters[kGhHist + threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
  if (threadIdx.x < 4 && s_acc[threadIdx.x]) atomicAdd(&counters[kGhLive + threadIdx.x], s_acc[threadIdx.x]);  // kGhLive .. kGhDangling0
  if (threadIdx.x == 0 && s_maxlevel) atomicMax(&counters[kGhMaxLevel], (unsigned long long)s_maxlevel);
}

// bitmap and state are zero going in
__global__ void gh_seed_kernel(uint32_t entry, uint32_t n, uint32_t* __restrict__ bitmap, uint32_t* __restrict__ list, uint32_t* __restrict__ state) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || entry >= n) return;
  bitmap[entry >> 5] = 1u << (entry & 31);
  list[0] = entry;
  state[kGhTail] = 1;
  state[kGhFrontier] = 0;
}

// One wave expands node u on `layer`: every live neighbour whose bit this lane set first is handed to `take(nb, m)`,
// called by ALL lanes with m = the ballot of the lanes that hold such a neighbour (so `take` may rank and aggregate).
template <typename Take>
__device__ __forceinline__ void gh_expand(const GhGraph& g, uint32_t u, uint32_t layer, uint32_t entry, uint32_t* __restrict__ bitmap,
                                          uint32_t lane, Take take) {
  if (u >= g.n || g.level[u] < layer) return;              // wave-uniform
  if (g.deleted[u] != 0u && u != entry) return;            // expandable(u): live, or the entry point
  uint32_t cnt;
  const uint32_t* row = gh_row(g, u, layer, &cnt);
  for (uint32_t base = 0; base < cnt; base += 64) {
    const uint32_t e = base + lane;
    const uint32_t nb = e < cnt ? row[1 + e] : kGhNone;
    bool fresh = false;
    if (nb < g.n && g.deleted[nb] == 0u) {
      const uint32_t bit = 1u << (nb & 31);
      fresh = (atomicOr(&bitmap[nb >> 5], bit) & bit) == 0u;
    }
    const uint64_t m = __ballot(fresh);
    if (m) take(nb, fresh, m);
  }
}

// frontier = list[lo, hi); appends at state[kGhTail]
__global__ __launch_bounds__(256) void gh_reach_wide_kernel(const GhGraph g, uint32_t layer, uint32_t entry, uint32_t lo, uint32_t hi,
                                                            uint32_t* __restrict__ bitmap, uint32_t* __restrict__ list,
                                                            uint32_t* __restrict__ state) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * 4;
  for (uint32_t i = lo + blockIdx.x * 4 + (threadIdx.x >> 6); i < hi; i += waves) {
    const uint32_t u = list[i];
    gh_expand(g, u, layer, entry, bitmap, lane, [&](uint32_t nb, bool fresh, uint64_t m) {
      uint32_t base = 0;
      if (lane == (uint32_t)__ffsll((unsigned long long)m) - 1u) base = atomicAdd(&state[kGhTail], (uint32_t)__popcll(m));
      base = rlane(base, (uint32_t)__ffsll((unsigned long long)m) - 1u);
      const uint32_t pos = base + ballot_rank(m, lane);
      if (fresh && pos < g.n) list[pos] = nb;  // a node is appended once: the list never outgrows n
    });
  }
}

// frontier = list[lo, hi), hi - lo <= kGhQueue; the list's length going in is hi.  One workgroup.
__global__ __launch_bounds__(kGhNarrowThreads) void gh_reach_narrow_kernel(const GhGraph g, uint32_t layer, uint32_t entry, uint32_t lo,
                                                                           uint32_t hi, uint32_t* __restrict__ bitmap,
                                                                           uint32_t* __restrict__ list, uint32_t* __restrict__ state) {
  __shared__ uint32_t s_q[2][kGhQueue];
  __shared__ uint32_t s_next;
  if (blockIdx.x != 0) return;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr uint32_t kWaves = kGhNarrowThreads / 64;
  uint32_t cnt = hi - lo;
  if (cnt > kGhQueue) cnt = kGhQueue;  // cannot happen: the host picks the wide step for such a frontier
  for (uint32_t i = threadIdx.x; i < cnt; i += kGhNarrowThreads) s_q[0][i] = list[lo + i];
  if (threadIdx.x == 0) s_next = 0;
  __syncthreads();
  uint32_t tail = hi, cur = 0, steps = 0, found = 0;
  while (cnt > 0) {
    uint32_t* next = s_q[cur ^ 1];
    for (uint32_t i = wave; i < cnt; i += kWaves) {
      const uint32_t u = s_q[cur][i];
      gh_expand(g, u, layer, entry, bitmap, lane, [&](uint32_t nb, bool fresh, uint64_t m) {
        uint32_t base = 0;
        if (lane == (uint32_t)__ffsll((unsigned long long)m) - 1u) base = atomicAdd(&s_next, (uint32_t)__popcll(m));
        base = rlane(base, (uint32_t)__ffsll((unsigned long long)m) - 1u);
        const uint32_t pos = base + ballot_rank(m, lane);
        if (fresh) {
          if (pos < kGhQueue) next[pos] = nb;
          if (tail + pos < g.n) list[tail + pos] = nb;  // the list keeps every reached node, whoever runs the next step
        }
      });
    }
    __syncthreads();
    found = s_next;
    steps += 1;
    tail += found;
    __syncthreads();
    if (threadIdx.x == 0) s_next = 0;
    __syncthreads();
    if (found > kGhQueue) break;  // the next step is a wide one: its frontier is list[tail - found, tail)
    cnt = found;
    cur ^= 1;
  }
  if (threadIdx.x == 0) {
    state[kGhTail] = tail;
    state[kGhFrontier] = tail - found;
    state[kGhSteps] = steps;
  }
}

// ---- weak components of the live layer-0 graph ----------------------------------------------------------------------
__device__ __forceinline__ uint32_t uf_parent(const uint32_t* parent, uint32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// parent[x] <= x always and only a root's word is ever changed by a link, so halving a path (a non-root's word moved to
// an ancestor further up) can be a plain agent-scope store: it never races with a link and any ancestor is a right value
__device__ __forceinline__ uint32_t uf_find(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = uf_parent(parent, x);
    if (p == x) return x;
    const uint32_t gp = uf_parent(parent, p);
    if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gp;
  }
}
__device__ __forceinline__ void uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a > b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(&parent[b], b, a) == b) return;  // b was still a root: linked under the smaller one
  }
}

__global__ __launch_bounds__(256) void uf_init_kernel(uint32_t n, uint32_t* __restrict__ parent, uint32_t* __restrict__ size) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  parent[i] = i;
  size[i] = 0;
}

__global__ __launch_bounds__(256) void uf_union_kernel(const GhGraph g, uint32_t* __restrict__ parent) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * 4;
  for (uint32_t u = blockIdx.x * 4 + (threadIdx.x >> 6); u < g.n; u += waves) {
    if (g.deleted[u] != 0u) continue;
    uint32_t cnt;
    const uint32_t* row = gh_row(g, u, 0, &cnt);
    for (uint32_t base = 0; base < cnt; base += 64) {
      const uint32_t e = base + lane;
      const uint32_t nb = e < cnt ? row[1 + e] : kGhNone;
      if (nb < g.n && nb != u && g.deleted[nb] == 0u) uf_unite(parent, u, nb);
    }
  }
}

// label[v] = the root of v (the smallest index of its component), kGhNone for a deleted node; size[root] += 1, one
// atomic per distinct root a wave holds
__global__ __launch_bounds__(256) void uf_label_kernel(const uint32_t* __restrict__ deleted, uint32_t n, uint32_t* __restrict__ parent,
                                                       uint32_t* __restrict__ label, uint32_t* __restrict__ size) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const bool alive = i < n && deleted[i] == 0u;
  const uint32_t root = alive ? uf_find(parent, i) : kGhNone;
  if (i < n) label[i] = root;
  uint64_t todo = __ballot(alive);
  while (todo) {
    const uint32_t lead = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
    const uint32_t r = rlane(root, lead);
    const uint64_t same = __ballot(alive && root == r) & todo;
    if (lane == lead && r < n) atomicAdd(&size[r], (uint32_t)__popcll(same));
    todo &= ~same;
  }
}

__global__ __launch_bounds__(256) void uf_summary_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ size, uint32_t n,
                                                         unsigned long long* __restrict__ counters) {
  __shared__ uint32_t s_roots, s_single, s_largest;
  if (threadIdx.x == 0) s_roots = s_single = s_largest = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool root = i < n && label[i] == i;
  const uint32_t sz = root ? size[i] : 0u;
  const uint32_t roots = (uint32_t)__popcll(__ballot(root));
  const uint32_t single = (uint32_t)__popcll(__ballot(root && sz == 1u));
  const uint32_t largest = wave_max_u(sz);
  if ((threadIdx.x & 63) == 0 && roots) {
    atomicAdd(&s_roots, roots);
    atomicAdd(&s_single, single);
    atomicMax(&s_largest, largest);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_roots) {
    atomicAdd(&counters[kGhComponents], (unsigned long long)s_roots);
    if (s_single) atomicAdd(&counters[kGhIsolated], (unsigned long long)s_single);
    atomicMax(&counters[kGhLargest], (unsigned long long)s_largest);
  }
}

}  // namespace fvdb
