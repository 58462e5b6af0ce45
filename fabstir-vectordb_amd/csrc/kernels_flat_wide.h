// kernels_flat_wide.h — the flat exact scan for k <= 4096: the result kernels_flat.h defines —
// every live node scored with the reference's fold, the k best by the unique key (distance bits << 32 | node index) —
// selected the way kernels_wide.h selects, because WaveTopK's 64 x 4 register list ends at k = 256.
//
//   flat_score_kernel   flat_scan_kernel's work item, loads, LDS transposition and fold, statement for statement (the
//                       two must round alike); the word `live ? bits(dist) : kInf32` of (query, row) goes to
//                       arena[query][row] instead of a register list.  Lane = row: a store instruction writes 64
//                       contiguous words.  The arena stride is tiles * 64 words and the lanes at or beyond n write
//                       kInf32, so every word the selection reads has been written and nothing needs a memset.
//   flat_select_kernel  wide_select_kernel's selection over those tiles * 64 words: radix select (8-bit digits, LDS
//                       histogram) of the k-th smallest word, the words below the cut in any order and the first
//                       `want` words AT the cut in arena order gathered as 64-bit keys into LDS, sorted there.  The
//                       arena index is the node index, so the key's low word is the result and nothing is resolved.
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
  using Quad = typename RowVec<RT>::Quad;
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t s = blockIdx.y * 4 + w;
  if (s >= a.slices) return;  // whole waves leave; no workgroup barrier below
  const uint32_t q0 = blockIdx.x * Q;
  const uint32_t ne = min((uint32_t)Q, a.B - q0);
  uint32_t qoff[Q];
#pragma unroll
  for (int j = 0; j < Q; ++j) qoff[j] = (q0 + ((uint32_t)j < ne ? (uint32_t)j : 0u)) * a.dpad;  // a short group repeats its first query

  float* tile = s_tile[w];
  const uint32_t tiles = (a.n + 63) >> 6;
  const uint32_t t0 = s * a.slice_tiles, t1 = min(tiles, t0 + a.slice_tiles);
  const uint32_t nchunks = (a.dpad + kFlatChunk - 1) / kFlatChunk;
  const uint32_t lr = (uint32_t)lane >> 3, lc = 4u * ((uint32_t)lane & 7u);  // the load role: row within 8, dims within the chunk
  const RT* rows = (const RT*)a.rows;

  // chunk c of tile t: instruction i reads dims [32 c + lc, + 4) of row 64 t + 8 i + lr (rows at or beyond n repeat the
  // last one: a valid address, never live)
  Quad x[8];
  auto load = [&](uint32_t t, uint32_t c) {
    const uint32_t j = c * kFlatChunk + lc;
    const bool in = j < a.dpad;  // dpad % 4 == 0: a quad never straddles the end
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t row = min(t * 64u + (uint32_t)i * 8u + lr, a.n - 1u);
      Quad v = {};
      if (in) v = *(const Quad*)(rows + (size_t)row * a.dpad + j);
      x[i] = v;
    }
  };

  if (t0 < t1) load(t0, 0);
  for (uint32_t t = t0; t < t1; ++t) {
    float acc[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) acc[j] = 0.0f;
    for (uint32_t c = 0; c < nchunks; ++c) {
#pragma unroll
      for (int i = 0; i < 8; ++i) *(float4*)(tile + ((uint32_t)i * 8u + lr) * kFlatStride + lc) = row_widen(x[i]);
      if (c + 1 < nchunks) load(t, c + 1);
      else if (t + 1 < t1) load(t + 1, 0);
      score_tile_publish();
      float xr[kFlatChunk];
      {
        const float4* p = (const float4*)(tile + (uint32_t)lane * kFlatStride);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float4 v = p[i];
          xr[4 * i + 0] = v.x;
          xr[4 * i + 1] = v.y;
          xr[4 * i + 2] = v.z;
          xr[4 * i + 3] = v.w;
        }
      }
      score_tile_retire();  // every lane holds its row's chunk: the tile may be rewritten
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t dbase = c * kFlatChunk + 16u * (uint32_t)h;  // wave-uniform
        const float* qb = a.queries + dbase;
        if (dbase + 16u <= a.dpad) {
          f32x16 qn = cload16(qb + qoff[0]);
#pragma unroll
          for (int j = 0; j < Q; ++j) {
            const f32x16 qv = qn;
            if (j + 1 < Q) qn = cload16(qb + qoff[j + 1]);
            __builtin_amdgcn_sched_barrier(0);  // the next query's request stays ahead of the 48 ops it overlaps with
            float tt, s2 = acc[j];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              tt = qv[i] - xr[16 * h + i];
              s2 = s2 + tt * tt;
            }
            acc[j] = s2;
          }
        } else {  // the row's last dimensions: quads below dpad only, so no query is read past its end
#pragma unroll
          for (int i4 = 0; i4 < 4; ++i4) {
            if (dbase + 4u * (uint32_t)i4 < a.dpad) {
#pragma unroll
              for (int j = 0; j < Q; ++j) {
                const f32x4 qv = cload((const f32x4*)(qb + qoff[j] + 4 * i4));
                float tt, s2 = acc[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  tt = qv[i] - xr[16 * h + 4 * i4 + i];
                  s2 = s2 + tt * tt;
                }
                acc[j] = s2;
              }
            }
          }
        }
      }
    }
    const uint32_t row = t * 64u + (uint32_t)lane;  // < tiles * 64 = stride: padding lanes of the last tile write too
    const bool live = row < a.n && a.dead[row] == 0u;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const float dist = sqrtf(acc[j]);
      if ((uint32_t)j < ne) a.arena[(uint64_t)(q0 + j) * a.stride + row] = live ? __float_as_uint(dist) : kInf32;
    }
  }
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

// One workgroup per query.  The selection is wide_select_kernel's (kernels_wide.h), restated: that kernel's four
// instantiations keep their code.
__global__ __launch_bounds__(kWideSelThreads) void flat_select_kernel(const FlatSelectArgs a) {
  constexpr uint32_t T = kWideSelThreads, W = T / 64;
  __shared__ uint64_t s_keys[kWideMaxK];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_wties[W];
  __shared__ uint32_t s_prefix, s_below, s_want, s_taken;

  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t q = blockIdx.x, k = a.k;
  if (tid == 0) {
    s_prefix = 0;
    s_below = 0;
    s_taken = 0;
  }
  __syncthreads();
  const uint32_t n = a.n_words;  // dead rows and padding hold kInf32
  const uint32_t* __restrict__ ar = a.arena + (size_t)q * a.stride;
  // each wave owns a contiguous run of whole tiles, in node order
  const uint32_t per = ((n / 64 + W - 1) / W) * 64;
  const uint32_t w0 = min(wave * per, n), w1 = min(w0 + per, n);

  // ---- the k-th smallest word: cut = its value, below = words smaller than it ----
  const uint32_t kk = min(k, n);  // n == 0: nothing to select
  uint32_t cut = 0, below = 0, want = 0;
  if (kk) {
    if (tid == 0) s_want = kk;
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (uint32_t b = tid; b < 256; b += T) s_hist[b] = 0;
      __syncthreads();
      const uint32_t prefix = s_prefix;
      const uint32_t himask = shift == 24 ? 0u : ~0u << (shift + 8);
      for (uint32_t i = w0 + lane; i < w1; i += 64) {  // whole tiles: all 64 lanes run every round
        const uint32_t v = ar[i];
        const bool in = (v & himask) == prefix;
        const uint32_t dg = (v >> shift) & 255u;
        // distances of one query share their leading bits: a wave whose words all fall in one bin adds once
        const uint32_t dg0 = rfl(dg);
        const uint64_t m_in = __ballot(in);
        if (__ballot(in && dg != dg0) == 0) {
          if (lane == 0 && m_in) atomicAdd(&s_hist[dg0], (uint32_t)__popcll(m_in));
        } else if (in) {
          atomicAdd(&s_hist[dg], 1u);
        }
      }
      __syncthreads();
      if (wave == 0) {  // the bin holding the s_want-th word of this round: 4 bins per lane, prefix across lanes
        const uint32_t h0 = s_hist[4 * lane], h1 = s_hist[4 * lane + 1], h2 = s_hist[4 * lane + 2], h3 = s_hist[4 * lane + 3];
        const uint32_t mine = h0 + h1 + h2 + h3;
        const uint32_t inc = wave_incl_scan_u(mine, (int)lane);
        const uint32_t wantr = s_want, exc = inc - mine;
        if (exc < wantr && wantr <= inc) {  // exactly one lane
          uint32_t bin = 4 * lane, acc = exc;
          if (acc + h0 < wantr) { acc += h0; ++bin;
            if (acc + h1 < wantr) { acc += h1; ++bin;
              if (acc + h2 < wantr) { acc += h2; ++bin; } } }
          s_prefix = prefix | (bin << shift);
          s_below += acc;
          s_want = wantr - acc;
        }
      }
      __syncthreads();
    }
    cut = s_prefix;
    below = s_below;
    want = s_want;  // words equal to `cut` still wanted: the first `want` of them in node order
    if (cut == kInf32) want = 0;  // fewer than k live rows: "no row" words are never results
  }

  // ---- words at the cut ahead of each wave ----
  uint32_t ties = 0;
  if (want)
    for (uint32_t i = w0 + lane; i < w1; i += 64) ties += (uint32_t)__popcll(__ballot(ar[i] == cut));
  if (lane == 0) s_wties[wave] = ties;
  __syncthreads();
  uint32_t tie_rank = 0;  // of the first word at the cut in this wave's run
  for (uint32_t w = 0; w < wave; ++w) tie_rank += s_wties[w];

  // ---- gather the survivors as (distance bits << 32 | node index) ----
  if (kk)
    for (uint32_t i = w0 + lane; i < w1; i += 64) {
      const uint32_t v = ar[i];
      const uint64_t m_tie = __ballot(v == cut);
      const uint32_t my_tie = tie_rank + ballot_rank(m_tie, lane);
      tie_rank += (uint32_t)__popcll(m_tie);
      uint32_t at = kInf32;
      if (v < cut) at = atomicAdd(&s_taken, 1u);       // slots [0, below): any order, the sort follows
      else if (v == cut && my_tie < want) at = below + my_tie;
      if (at < kWideMaxK) s_keys[at] = ((uint64_t)v << 32) | i;
    }
  const uint32_t count = below + want;  // the selection found at least `want` words at the cut
  uint32_t P = 1;
  while (P < count) P <<= 1;
  __syncthreads();
  for (uint32_t e = count + tid; e < P; e += T) s_keys[e] = ~0ull;
  __syncthreads();

  // ---- sort ascending ----
  for (uint32_t kb = 2; kb <= P; kb <<= 1)
    for (uint32_t j = kb >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < P / 2; t += T) {
        const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const uint64_t x = s_keys[lo], y = s_keys[hi];
        const bool up = (lo & kb) == 0;
        if ((x > y) == up) {
          s_keys[lo] = y;
          s_keys[hi] = x;
        }
      }
      __syncthreads();
    }

  // ---- the key's low word is the node ----
  for (uint32_t e = tid; e < k; e += T) {
    const bool have = e < count;
    const uint64_t key = have ? s_keys[e] : ~0ull;
    const size_t o = (size_t)q * k + e;
    a.out_nodes[o] = have ? (uint32_t)key : 0xFFFFFFFFu;
    a.out_dist[o] = have ? __uint_as_float((uint32_t)(key >> 32)) : __uint_as_float(0x7F800000u);
  }
  if (tid == 0) a.out_counts[q] = count;
}

}  // namespace fvdb
