// kernels_range.h — radius search: every candidate row within a distance of the query, counted
// exactly and returned up to a cap, where every other search here answers "the k nearest".
//
// The ball of (query, radius r): the candidate rows whose distance word satisfies bits(dist) <= bits(r) — non-negative
// f32 bits are monotone as u32, so the radius is a cut word the caller supplies where the wide selection (kernels_wide.h)
// has to find one.  total = the size of the ball, never capped; results = its first min(total, m) rows by the wide
// selection's unique key (distance bits << 32 | arena index), i.e. search_wide(k = m) truncated at the radius.
//
//   range_select_keys         one pass counts the words at or below the cut (ballot + popcount per 64-word block).  If
//                             they number no more than m, one more pass gathers them as keys and the LDS sort orders
//                             them: no histogram pass runs.  Otherwise more than m words are at or below the cut, so the
//                             m-th smallest word is too, and wide_select_keys(m) as it stands is the answer.
//   range_flat_select_kernel  flat_select_kernel with that selection: the arena index is the node.
//   range_list_select_kernel  wide_select_kernel with that selection: seq -> (rank, position) -> pool slot -> id.
//   flat_count_kernel         the flat scan with no arena: flat_fold_slice's fold, each wave counting the rows of its
//                             slice within each query's radius, one integer atomic per (query, slice).
//
// Dead rows, masked rows and padding hold kInf32 and a NaN distance is above 0x7F800000: neither is ever in a ball.  A
// radius that is negative or NaN has an empty ball (-0.0 is 0.0): the cut word is never trusted to be below kInf32.
#pragma once
#include "kernels_flat_wide.h"
#include "kernels_wide.h"

#pragma clang fp contract(off)

namespace fvdb {

// the cut word of a radius, plus one: a distance word w is in the ball iff w < range_cut_end(r).  0 = the empty ball.
__device__ __forceinline__ uint32_t range_cut_end(const float r) {
  const uint32_t b = __float_as_uint(r);
  if (b == 0x80000000u) return 1u;             // -0.0
  return b <= 0x7F800000u ? b + 1u : 0u;       // +inf included; negative and NaN: nothing
}

// The selection of a ball, once: of the n (a multiple of 64) distance words ar[0, n), those below cut_end number
// *total; the min(*total, m) smallest of them come back as keys (word << 32 | index), ties in index order — the rule of
// wide_select_keys, whose calling convention this has: every thread of a workgroup of kWideSelThreads calls it, it owns
// `s`, and on return s.keys[0, count) are ascending and visible to every thread.  1 <= m <= kWideMaxK.
__device__ __forceinline__ uint32_t range_select_keys(const uint32_t* __restrict__ ar, const uint32_t n, const uint32_t cut_end,
                                                      const uint32_t m, WideSelectLds& s, uint32_t* total) {
  constexpr uint32_t T = kWideSelThreads, W = T / 64;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // each wave owns a contiguous run of whole 64-word blocks, in index order (wide_select_keys' split)
  const uint32_t per = ((n / 64 + W - 1) / W) * 64;
  const uint32_t w0 = min(wave * per, n), w1 = min(w0 + per, n);

  // ---- 1: the size of the ball ----
  uint32_t mine = 0;
  for (uint32_t i = w0 + lane; i < w1; i += 64) mine += (uint32_t)__popcll(__ballot(ar[i] < cut_end));
  if (lane == 0) s.wties[wave] = mine;
  if (tid == 0) s.taken = 0;
  __syncthreads();
  uint32_t all = 0;
  for (uint32_t w = 0; w < W; ++w) all += s.wties[w];
  *total = all;

  if (all > m) {  // ---- 3: more than m words in the ball: its m smallest are the m smallest of all ----
    __syncthreads();  // every thread has read the wave sums before the selection takes `s` over
    return wide_select_keys(ar, n, m, s);
  }

  // ---- 2: the whole ball as keys, any order: they are unique and the sort follows ----
  for (uint32_t i = w0 + lane; i < w1; i += 64) {
    const uint32_t v = ar[i];
    if (v < cut_end) {
      const uint32_t at = atomicAdd(&s.taken, 1u);
      if (at < kWideMaxK) s.keys[at] = ((uint64_t)v << 32) | i;  // at < all <= m <= kWideMaxK
    }
  }
  uint32_t P = 1;
  while (P < all) P <<= 1;
  __syncthreads();
  for (uint32_t e = all + tid; e < P; e += T) s.keys[e] = ~0ull;
  __syncthreads();
  lds_bitonic_sort_u64(s.keys, P, tid, T);
  return all;
}

struct RangeFlatArgs {
  FlatSelectArgs sel;      // k = max_results; outputs [B][k] with flat_select_kernel's tails
  const float* radius;     // [B]
  uint32_t* out_totals;    // [B]
};

// One workgroup per query; the key's low word is the node, as in flat_select_kernel.
__global__ __launch_bounds__(kWideSelThreads) void range_flat_select_kernel(const RangeFlatArgs a) {
  __shared__ WideSelectLds s_sel;
  const uint32_t tid = threadIdx.x, q = blockIdx.x, k = a.sel.k;
  uint32_t total = 0;
  const uint32_t count =
      range_select_keys(a.sel.arena + (size_t)q * a.sel.stride, a.sel.n_words, range_cut_end(a.radius[q]), k, s_sel, &total);

  for (uint32_t e = tid; e < k; e += kWideSelThreads) {
    const bool have = e < count;
    const uint64_t key = have ? s_sel.keys[e] : ~0ull;
    const size_t o = (size_t)q * k + e;
    a.sel.out_nodes[o] = have ? (uint32_t)key : 0xFFFFFFFFu;
    a.sel.out_dist[o] = have ? __uint_as_float((uint32_t)(key >> 32)) : __uint_as_float(0x7F800000u);
  }
  if (tid == 0) {
    a.sel.out_counts[q] = count;
    a.out_totals[q] = total;
  }
}

struct RangeListArgs {
  WideArgs w;              // k = max_results; out_ids / out_dist / out_counts as wide_select_kernel writes them
  const float* radius;     // [B]
  uint32_t* out_totals;    // [B]
};

// One workgroup per query.  LDS_BASE as in wide_select_kernel: the rank bases staged in LDS while nprobe <= kWideMaxProbes.
template <bool LDS_BASE>
__global__ __launch_bounds__(kWideSelThreads) void range_list_select_kernel(const RangeListArgs ra) {
  constexpr uint32_t T = kWideSelThreads;
  __shared__ WideSelectLds s_sel;
  __shared__ uint32_t s_base_lds[LDS_BASE ? kWideMaxProbes + 1 : 1];
  const WideArgs& a = ra.w;

  const uint32_t tid = threadIdx.x;
  const uint32_t q = blockIdx.x, np = a.nprobe, k = a.k;
  const uint32_t* s_base = a.base + (size_t)q * (np + 1);
  if (LDS_BASE) {
    for (uint32_t r = tid; r <= np; r += T) s_base_lds[r] = a.base[(size_t)q * (np + 1) + r];
    s_base = s_base_lds;
    __syncthreads();
  }
  uint32_t total = 0;
  const uint32_t count =
      range_select_keys(a.arena + (size_t)q * a.stride, s_base[np] * 64, range_cut_end(ra.radius[q]), k, s_sel, &total);
  const uint64_t* s_keys = s_sel.keys;

  // ---- seq -> (rank, position) -> pool slot -> id ----
  for (uint32_t e = tid; e < k; e += T) {
    const bool have = e < count;
    uint64_t key = ~0ull, id = ~0ull;
    if (have) {
      key = s_keys[e];
      const uint32_t seq = (uint32_t)key;
      const uint32_t r = wide_rank_of(s_base, np, seq >> 6);
      const uint32_t L = a.probes[(size_t)q * np + r];
      const uint32_t pos = seq - s_base[r] * 64;
      const uint32_t blk = a.lists.blocks[a.lists.off[L] + (pos >> 6)];
      id = a.pool.ids[(size_t)blk * 64 + (pos & 63)];
    }
    const size_t o = (size_t)q * k + e;
    if (a.out_ids) a.out_ids[o] = id;
    if (a.out_dist) a.out_dist[o] = have ? __uint_as_float((uint32_t)(key >> 32)) : __uint_as_float(0x7F800000u);
  }
  if (tid == 0) {
    if (a.out_counts) a.out_counts[q] = count;
    if (ra.out_totals) ra.out_totals[q] = total;
  }
}

struct FlatCountArgs {
  const void* rows;       // the store: [node][dpad] of the kernel's RT
  const float* queries;   // [B][dpad], zero beyond d, 16-byte aligned
  const uint32_t* dead;   // [n]: non-zero = not live (the graph's deleted flags, or a mask's)
  uint32_t dpad, n, B;
  uint32_t slices, slice_tiles;  // flat_score_kernel's
  const float* radius;    // [B]
  uint32_t* counts;       // [B], zeroed on the stream ahead of the launch
};

// flat_score_kernel's work item with the ball's test in place of the arena store: a wave sums, per query, the rows of
// its slice within the radius and adds each sum once.  Integer adds: the result does not depend on their order.
template <int Q, typename RT>
__global__ __launch_bounds__(256) void flat_count_kernel(const FlatCountArgs a) {
  __shared__ __attribute__((aligned(16))) float s_tile[4][kFlatTileFloats];
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t s = blockIdx.y * 4 + w;
  if (s >= a.slices) return;  // whole waves leave; no workgroup barrier below
  const uint32_t q0 = blockIdx.x * Q;
  const uint32_t ne = min((uint32_t)Q, a.B - q0);
  uint32_t qoff[Q], rw[Q], cnt[Q];
#pragma unroll
  for (int j = 0; j < Q; ++j) {
    const uint32_t qj = q0 + ((uint32_t)j < ne ? (uint32_t)j : 0u);  // a short group repeats its first query
    qoff[j] = qj * a.dpad;
    rw[j] = (uint32_t)j < ne ? range_cut_end(cload(a.radius + qj)) : 0u;
    cnt[j] = 0;
  }
  const uint32_t tiles = (a.n + 63) >> 6;
  const uint32_t t0 = s * a.slice_tiles, t1 = min(tiles, t0 + a.slice_tiles);

  auto count = [&](uint32_t, uint32_t, bool live, const float(&acc)[Q]) {
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const float dist = sqrtf(acc[j]);
      cnt[j] += (uint32_t)__popcll(__ballot(live && __float_as_uint(dist) < rw[j]));
    }
  };
  flat_fold_slice<Q>((const RT*)a.rows, a.queries, a.dead, a.dpad, a.n, qoff, s_tile[w], t0, t1, lane, count);

  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < Q; ++j)
      if ((uint32_t)j < ne && cnt[j]) atomicAdd(a.counts + q0 + j, cnt[j]);
  }
}

}  // namespace fvdb
