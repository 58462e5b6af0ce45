// kernels_allow.h — allow-set masks: a filtered search sees the index "as if every row outside the allow-set had been
// soft-deleted" (DESIGN.md section 9c).  The scan and traversal kernels are not touched: they read liveness through one
// pointer (pool `valid` words; GraphView::deleted), and a masked search points them at the words / flags built here.
//
//   allow_set_build_kernel    the allowed ids into an open-addressing hash set (below: why hashed, not sorted)
//   allow_pool_words_kernel   IVF: out[blk] = valid[blk] & "row's id is allowed", one wave per 64-row pool block
//   allow_graph_*_kernel      graph: flags[node] = deleted[node] | !allowed[node], the count of allowed live nodes and
//                             their indices in ascending order (count per workgroup, scan, write)
//   allow_scan_kernel         exact scan of the allowed live nodes: the reference's f32 fold (score_rows.h) over gathered
//                             rows, per-(query, slice) top k by (distance bits, position in the node list)
//   allow_merge_kernel        the slices of a query merged by the same key
//                             both also in a grouped form (GR): every query scans the node list of its own group
//
// Membership: a hash set rather than a sorted array.  Both are exact.  The set is built by one pass of independent
// inserts (a sort needs log^2 n passes or a radix sort this project does not otherwise have), and a lookup is one or two
// dependent loads at load factor <= 1/2 against log2(n) for a binary search — the lookup runs once per live pool row.
#pragma once
#include "common.h"
#include "kernels_scan.h"
#include "score_rows.h"
#include "wave_ops.h"

namespace fvdb {

constexpr unsigned long long kAllowEmpty = ~0ull;  // = FVDB_NO_ID: never a row's id

__device__ __forceinline__ uint32_t allow_hash(uint64_t id) {  // the 64-bit finaliser of MurmurHash3
  id ^= id >> 33;
  id *= 0xff51afd7ed558ccdULL;
  id ^= id >> 33;
  id *= 0xc4ceb9fe1a85ec53ULL;
  id ^= id >> 33;
  return (uint32_t)id;
}

// table: slots + 1 = a power of two >= 2 n entries, all kAllowEmpty on entry.  Duplicates in ids[] are harmless.
__global__ __launch_bounds__(256) void allow_set_build_kernel(const uint64_t* __restrict__ ids, uint64_t n,
                                                              unsigned long long* __restrict__ table, uint32_t slot_mask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long id = ids[i];
  if (id == kAllowEmpty) return;
  uint32_t h = allow_hash(id) & slot_mask;
  for (uint32_t probe = 0; probe <= slot_mask; ++probe) {
    const unsigned long long prev = atomicCAS(&table[h], kAllowEmpty, id);
    if (prev == kAllowEmpty || prev == id) return;
    h = (h + 1) & slot_mask;
  }
}

__device__ __forceinline__ bool allow_set_has(const unsigned long long* __restrict__ table, uint32_t slot_mask, unsigned long long id) {
  if (id == kAllowEmpty) return false;
  uint32_t h = allow_hash(id) & slot_mask;
  for (uint32_t probe = 0; probe <= slot_mask; ++probe) {  // half the slots are empty: ends after a few steps
    const unsigned long long v = table[h];
    if (v == id) return true;
    if (v == kAllowEmpty) return false;
    h = (h + 1) & slot_mask;
  }
  return false;
}

// One wave per pool block: 512 contiguous bytes of ids in, one word out.  Rows that are not live are not looked up.
__global__ __launch_bounds__(256) void allow_pool_words_kernel(const uint64_t* __restrict__ pool_ids, const uint64_t* __restrict__ pool_valid,
                                                               uint32_t blocks, const unsigned long long* __restrict__ table,
                                                               uint32_t slot_mask, uint64_t* __restrict__ out_words,
                                                               unsigned long long* __restrict__ out_count) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t blk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (blk >= blocks) return;
  const uint64_t live = pool_valid[blk];
  bool in = false;
  if ((live >> lane) & 1) in = allow_set_has(table, slot_mask, pool_ids[(size_t)blk * 64 + lane]);
  const uint64_t word = __ballot(in);
  if (lane == 0) {
    out_words[blk] = word;
    if (word) atomicAdd(out_count, (unsigned long long)__popcll(word));
  }
}

// flags[] is all 1 on entry ("not allowed"); an allowed node gets 0.  Indices the graph does not hold are ignored.
__global__ __launch_bounds__(256) void allow_graph_mark_kernel(const uint32_t* __restrict__ nodes, uint64_t n_allowed, uint32_t n,
                                                               uint32_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_allowed) return;
  const uint32_t node = nodes[i];
  if (node < n) flags[node] = 0u;
}

// flags[node] |= deleted[node]; wg_count[workgroup] = allowed live nodes among its 256
__global__ __launch_bounds__(256) void allow_graph_count_kernel(uint32_t* __restrict__ flags, const uint32_t* __restrict__ deleted, uint32_t n,
                                                                uint32_t* __restrict__ wg_count) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool ok = false;
  if (i < n) {
    const uint32_t f = (flags[i] | deleted[i]) ? 1u : 0u;
    flags[i] = f;
    ok = f == 0u;
  }
  const uint64_t m = __ballot(ok);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) wg_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// node i of workgroup b goes to out[wg_offset[b] + its rank among the workgroup's allowed live nodes]: ascending
__global__ __launch_bounds__(256) void allow_graph_write_kernel(const uint32_t* __restrict__ flags, uint32_t n, const uint32_t* __restrict__ wg_offset,
                                                                uint32_t* __restrict__ out_nodes) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool ok = i < n && flags[i] == 0u;
  const uint64_t m = __ballot(ok);
  if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t base = wg_offset[blockIdx.x];
  for (uint32_t w = 0; w < wave; ++w) base += s_cnt[w];
  if (ok) out_nodes[base + ballot_rank(m, lane)] = i;
}

// ---- exact scan of the allowed live nodes -----------------------------------------------------------------------------
// A workgroup = 4 waves = 4 consecutive queries over ONE slice of the node list, so the four gathers of a row meet in the
// cache.  A wave scores 64 nodes per round with score_rows_wave (the traversal's arithmetic: sub, mul, sequential add,
// sqrt) and keeps its k best by (distance bits, position in the node list): position order is node-index order.
struct AllowGroup {  // the node list of one mask
  const uint32_t* nodes;  // [n_nodes] ascending
  uint32_t n_nodes, reserved;
};
struct AllowScanArgs {
  const void* rows;        // the store: [node][dpad] of the kernel's RT (float or half_t)
  const float* queries;    // [B][dpad]
  const uint32_t* nodes;   // [n_nodes] ascending
  uint32_t dpad, n_nodes, B, k;
  uint32_t slices, slice_len;  // slice s = positions [s * slice_len, min(n_nodes, (s + 1) * slice_len))
  uint64_t* part;              // [slices][B][k] keys, ~0 = none
  // grouped form: query q scans groups[group[q]] (the host has checked every group[] entry); nodes / n_nodes above are
  // not read, and the slices are laid out for the longest list — a slice past the end of a shorter one scores nothing
  const AllowGroup* groups;
  const uint32_t* group;  // [B]
};

template <int KR, typename RT = float, bool GR = false>
__global__ __launch_bounds__(256) void allow_scan_kernel(const AllowScanArgs a) {
  __shared__ __attribute__((aligned(16))) float s_tile[4][kScoreTileFloats];
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x * 4 + w, s = blockIdx.y;
  if (q >= a.B) return;  // whole waves leave; no workgroup barrier below
  const float* qrow = a.queries + (size_t)q * a.dpad;
  const uint32_t* nodes = a.nodes;
  uint32_t n_nodes = a.n_nodes;
  if constexpr (GR) {
    const AllowGroup g = a.groups[a.group[q]];
    nodes = g.nodes;
    n_nodes = g.n_nodes;
  }
  const uint32_t lo = s * a.slice_len;
  const uint32_t hi = min(n_nodes, lo + a.slice_len);  // below lo where the slice lies past the list: no round runs
  WaveTopK<KR> tk;
  tk.init();
  uint32_t th = kInf32, tl = kInf32;
  for (uint32_t e0 = lo; e0 < hi; e0 += 64) {
    const uint32_t cnt = min(64u, hi - e0);
    const uint32_t pos = e0 + (uint32_t)lane;
    const bool have = (uint32_t)lane < cnt;
    const uint32_t node = have ? nodes[pos] : 0u;
    const float d = score_rows_wave((const RT*)a.rows, a.dpad, qrow, node, cnt, s_tile[w], lane);
    offer<KR>(tk, a.k, have ? __float_as_uint(d) : kInf32, pos, th, tl, lane);
  }
  uint64_t* out = a.part + ((size_t)s * a.B + q) * a.k;
#pragma unroll
  for (int rr = 0; rr < KR; ++rr) {
    const uint32_t e = rr * 64 + lane;
    if (e < a.k) out[e] = ((uint64_t)tk.hi[rr] << 32) | tk.lo[rr];  // (kInf32, kInf32) = ~0 where the list is short
  }
}

// one wave per query: the slices' lists merged by key; positions become node indices.  slices == 0 writes empty rows.
// GR: positions are those of the query's own group (groups / group as in AllowScanArgs; `nodes` is not read).
template <int KR, bool GR = false>
__global__ __launch_bounds__(256) void allow_merge_kernel(const uint64_t* __restrict__ part, const uint32_t* __restrict__ nodes, uint32_t slices,
                                                          uint32_t B, uint32_t k, uint32_t* __restrict__ out_nodes, float* __restrict__ out_dist,
                                                          uint32_t* __restrict__ out_counts, const AllowGroup* __restrict__ groups,
                                                          const uint32_t* __restrict__ group) {
  const int lane = threadIdx.x & 63;
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= B) return;
  if constexpr (GR) nodes = groups[group[q]].nodes;
  WaveTopK<KR> tk;
  tk.init();
  uint32_t th = kInf32, tl = kInf32;
  for (uint32_t s = 0; s < slices; ++s)
    for (uint32_t e0 = 0; e0 < k; e0 += 64) {
      const uint32_t e = e0 + lane;
      uint32_t chi = kInf32, clo = 0;
      if (e < k) {
        const uint64_t key = part[((size_t)s * B + q) * k + e];
        chi = (uint32_t)(key >> 32);
        clo = (uint32_t)key;
      }
      offer<KR>(tk, k, chi, clo, th, tl, lane);
    }
  uint32_t count = 0;
#pragma unroll
  for (int rr = 0; rr < KR; ++rr) {
    const uint32_t e = rr * 64 + lane;
    const bool have = e < k && tk.hi[rr] != kInf32;
    count += __popcll(__ballot(have));
    if (e < k) {
      out_nodes[(size_t)q * k + e] = have ? nodes[tk.lo[rr]] : 0xFFFFFFFFu;
      out_dist[(size_t)q * k + e] = have ? __uint_as_float(tk.hi[rr]) : __uint_as_float(0x7F800000u);
    }
  }
  if (lane == 0) out_counts[q] = count;
}

}  // namespace fvdb
