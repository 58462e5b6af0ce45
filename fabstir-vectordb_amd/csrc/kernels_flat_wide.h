// kernels_flat_wide.h — the flat exact scan for k <= 4096: the result kernels_flat.h defines —
// every live node scored with the reference's fold, the k best by the unique key (distance bits << 32 | node index) —
// selected the way kernels_wide.h selects, because WaveTopK's 64 x 4 register list ends at k = 256.
//
//   flat_score_kernel   flat_scan_kernel's work item and its fold, flat_fold_slice (kernels_flat.h: one text, so the two
//                       round alike); the word `live ? bits(dist) : kInf32` of (query, row) goes to arena[query][row]
//                       instead of a register list.  Lane = row: a store instruction writes 64 contiguous words.  The
//                       arena stride is tiles * 64 words and the lanes at or beyond n write kInf32, so every word the
//                       selection reads has been written and nothing needs a memset.
//   flat_select_kernel  wide_select_keys (kernels_wide.h), the selection of wide_select_kernel, over those tiles * 64
//                       words.  The arena index is the node index, so the key's low word is the result and nothing is
//                       resolved.
//
// The tie rule "arena order at the cut" is the flat scan's own: among equal distance bits the lower node index wins.
#pragma once
#include "kernels_flat.h"
#include "kernels_wide.h"

#pragma clang fp contract(off)

namespace fvdb {

struct FlatScoreArgs {
  const void* rows;       // the store: [node][dpad] of the kernel's RT
  const float* queries;   // [B][dpad], zero beyond d, 16-byte aligned
  const uint32_t* dead;   // [n]: non-zero = not live (the graph's deleted flags, or a mask's)
  uint32_t dpad, n, B;
  uint32_t slices, slice_tiles;  // slice s = tiles [s * slice_tiles, min(tiles, (s + 1) * slice_tiles)), a tile = 64 rows
  uint32_t* arena;               // [B][stride] distance bits by node index
  uint64_t stride;               // words per query: tiles * 64
};

template <int Q, typename RT>
__global__ __launch_bounds__(256) void flat_score_kernel(const FlatScoreArgs a) {
  __shared__ __attribute__((aligned(16))) float s_tile[4][kFlatTileFloats];
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t s = blockIdx.y * 4 + w;
  if (s >= a.slices) return;  // whole waves leave; no workgroup barrier below
  const uint32_t q0 = blockIdx.x * Q;
  const uint32_t ne = min((uint32_t)Q, a.B - q0);
  uint32_t qoff[Q];
#pragma unroll
  for (int j = 0; j < Q; ++j) qoff[j] = (q0 + ((uint32_t)j < ne ? (uint32_t)j : 0u)) * a.dpad;  // a short group repeats its first query
  const uint32_t tiles = (a.n + 63) >> 6;
  const uint32_t t0 = s * a.slice_tiles, t1 = min(tiles, t0 + a.slice_tiles);

  // row < tiles * 64 = stride: padding lanes of the last tile write too
  auto store = [&](uint32_t, uint32_t row, bool live, const float(&acc)[Q]) {
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const float dist = sqrtf(acc[j]);
      if ((uint32_t)j < ne) a.arena[(uint64_t)(q0 + j) * a.stride + row] = live ? __float_as_uint(dist) : kInf32;
    }
  };
  flat_fold_slice<Q>((const RT*)a.rows, a.queries, a.dead, a.dpad, a.n, qoff, s_tile[w], t0, t1, lane, store);
}

struct FlatSelectArgs {
  const uint32_t* arena;  // [B][stride] distance bits by node index, kInf32 = not a row
  uint64_t stride;        // words per query
  uint32_t n_words;       // words of a query the selection reads: tiles * 64 (a multiple of 64, <= stride)
  uint32_t k;
  uint32_t* out_nodes;    // [B][k], tail 0xFFFFFFFF
  float* out_dist;        // [B][k], tail +inf
  uint32_t* out_counts;   // [B]
};

// One workgroup per query; dead rows and padding hold kInf32.
__global__ __launch_bounds__(kWideSelThreads) void flat_select_kernel(const FlatSelectArgs a) {
  __shared__ WideSelectLds s_sel;
  const uint32_t tid = threadIdx.x, q = blockIdx.x, k = a.k;
  const uint32_t count = wide_select_keys(a.arena + (size_t)q * a.stride, a.n_words, k, s_sel);

  // ---- the key's low word is the node ----
  for (uint32_t e = tid; e < k; e += kWideSelThreads) {
    const bool have = e < count;
    const uint64_t key = have ? s_sel.keys[e] : ~0ull;
    const size_t o = (size_t)q * k + e;
    a.out_nodes[o] = have ? (uint32_t)key : 0xFFFFFFFFu;
    a.out_dist[o] = have ? __uint_as_float((uint32_t)(key >> 32)) : __uint_as_float(0x7F800000u);
  }
  if (tid == 0) a.out_counts[q] = count;
}

}  // namespace fvdb
