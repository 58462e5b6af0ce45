// score_rows.h — the "transposed product" scorer: the reference's distance (src/core/vector_ops.rs:51-57,
// src/hnsw/core.rs:691-697) for a handful of arbitrary row-major rows against one query, by ONE wavefront, without each
// lane walking its own row.  This file is its only home; the traversal (kernels_graph_fast.h), the insert and the edge
// distances (kernels_graph_build.h), the coarse select, the allow-set exact scan and the matrix-core select all call it.
//
// Rows are f32 or fp16 (row_types.h): the row element is a template parameter, the loads read pairs of it, and
// score_products widens a pair exactly before it subtracts.  Everything after the load is the same code for both.
//
// Scoring keeps the reference's arithmetic — per row t = q_i - x_i; sum = sum + t*t, i ascending, f32, no FMA — but
// splits it where it is order-free:
//   * the products t*t are computed with the rows loaded COALESCED: a wave instruction reads 512 contiguous bytes of ONE
//     row (lane l = dims 2l, 2l+1 of a 128-dim block), and all of a round's loads are in flight together;
//   * each 128-dim block of products is transposed through a small LDS tile (row stride 132 floats: lane r's
//     ds_read_b128s are bank-conflict free);
//   * lane r then adds row r's products in dimension order — the reference's running sum, addend for addend.
// The sum sees the same addends in the same order, so the bits are the reference's, and (q - x)^2 and (x - q)^2 are the
// same bits, so the result equals a per-lane fold's bit for bit.  Against the per-lane row walk the VALU work per hop
// drops from 3 ops per dim per lane-pass to ~1, and its 12 dependent L2 round trips become one HBM latency.
//
// The core (score_products, score_tile_publish / score_add_row / score_tile_retire) is stated once; two schedules run it:
//   score_fixed<NB, RC, FULL, TILES>   query and rows in registers, dimension at compile time (NB blocks of 128)
//   score_rows_stream<RC>              dimension at run time, the next block's loads in flight while one is folded
#pragma once
#include "common.h"
#include "row_types.h"

#pragma clang fp contract(off)

namespace fvdb {

#ifndef FVDB_FAST_ADD_UNROLL
#define FVDB_FAST_ADD_UNROLL 16  // LDS reads in flight ahead of the add chain (8: 1 % slower; 32: spills)
#endif
constexpr int kScoreAddUnroll = FVDB_FAST_ADD_UNROLL;
constexpr uint32_t kScoreStride = 132;  // floats per staged row: 128 products + 4 pad (lane r's reads hit 16 distinct bank quads)
constexpr uint32_t kScoreTileFloats = 16 * kScoreStride;  // one wave's tile (<= 16 rows)

// Diagnostic builds (-DFVDB_GRAPH_STAMPS): the traversal hands score_fixed its per-wave cycle sums — slot 8 the row
// loads, 9 the first block's products, 11 the folds — and every other caller hands it nothing.  Absent otherwise.
#ifdef FVDB_GRAPH_STAMPS
#define SCORE_STAMP_PARAM , unsigned long long* t_acc = nullptr
#define SCORE_STAMP(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define SCORE_STAMP_ADD(slot, a, b) \
  do {                              \
    if (t_acc) t_acc[slot] += (b) - (a); \
  } while (0)
#else
#define SCORE_STAMP_PARAM
#define SCORE_STAMP(var)
#define SCORE_STAMP_ADD(slot, a, b)
#endif

// ---------------------------------------------------------------------------------------------
// the core
// ---------------------------------------------------------------------------------------------
// products of block c of RC rows into `tile`: x[r][c] = dims (128c + 2*lane, +1) of row r, q the same dims of the query
// (x as loaded — float2, or a half pair kept packed until here and widened exactly)
template <typename P, int RC, int NB>
__device__ __forceinline__ void score_products(const P (&x)[RC][NB], int c, const float2 q, float* tile, int lane) {
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    const float2 xv = row_widen(x[r][c]);
    const float t0 = q.x - xv.x, t1 = q.y - xv.y;
    *(float2*)(tile + (uint32_t)r * kScoreStride + 2u * (uint32_t)lane) = make_float2(t0 * t0, t1 * t1);
  }
}

// the tile row a lane adds: its own, or the last one — idle lanes add a valid row too: no branch
template <int RC>
__device__ __forceinline__ uint32_t score_lane_row(int lane) {
  return (uint32_t)lane < (uint32_t)RC ? (uint32_t)lane : (uint32_t)(RC - 1);
}

// The fold of one tile row is publish, add, retire.  The pieces are apart because the two-tile schedule writes the next
// block's products between the first two.
__device__ __forceinline__ void score_tile_publish() {  // the wave's products are in the tile
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ float score_add_row(const float* tile, uint32_t lrow, float acc) {
  const float4* p = (const float4*)(tile + lrow * kScoreStride);
#pragma unroll kScoreAddUnroll
  for (int i = 0; i < 32; ++i) {
    const float4 v = p[i];
    acc = acc + v.x;
    acc = acc + v.y;
    acc = acc + v.z;
    acc = acc + v.w;
  }
  return acc;
}
__device__ __forceinline__ void score_tile_retire() {  // every lane has read its row: the tile may be rewritten
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ float score_fold(const float* tile, uint32_t lrow, float acc) {
  score_tile_publish();
  acc = score_add_row(tile, lrow, acc);
  score_tile_retire();
  return acc;
}

// ---------------------------------------------------------------------------------------------
// register-resident schedule
// ---------------------------------------------------------------------------------------------
// Distances of the wave's query to `cnt` rows (1 <= cnt <= RC; lane r of `pn` holds the r-th row's node): returns, in
// lane r < cnt, sqrt of the reference's sum.  q2[c] = dims (128c + 2*lane, +1) of the query, held in registers by the
// caller.  Straight-line code for exactly RC rows — rows past cnt repeat the last one (an L2 hit) and their sums are
// ignored.  FULL: dpad == NB * 128, no bounds checks.
// TILES = 2: `stage` holds two tiles, tile_floats apart, and the products of block c + 1 go to the other tile, so the
// scheduler can fill the bubbles of the dependent add chain of block c with them.  TILES = 1: one tile — products of
// block c, fence, fold of block c, fence.
template <int NB, int RC, bool FULL, int TILES, typename RT>
__device__ __forceinline__ float score_fixed(const RT* __restrict__ rows, uint32_t dpad, const float2 (&q2)[NB], uint32_t pn,
                                             uint32_t cnt, float* stage, uint32_t tile_floats, int lane SCORE_STAMP_PARAM) {
  static_assert(TILES == 1 || TILES == 2, "one or two product tiles");
  SCORE_STAMP(ta);
  using P = typename RowVec<RT>::Pair;
  P x[RC][NB];
  const uint32_t last = cnt - 1;
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    const uint32_t rr = (uint32_t)r < last ? (uint32_t)r : last;  // wave-uniform
    const uint32_t node = __builtin_amdgcn_readlane(pn, rr);
    const RT* row = rows + (size_t)node * dpad;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      const uint32_t j = (uint32_t)c * 128u + 2u * (uint32_t)lane;
      if (FULL) x[r][c] = *(const P*)(row + j);
      else x[r][c] = j < dpad ? *(const P*)(row + j) : RowVec<RT>::zero_pair();  // dpad % 4 == 0: pairs never straddle it
    }
  }
  SCORE_STAMP(tb);
  SCORE_STAMP_ADD(8, ta, tb);
  const uint32_t lrow = score_lane_row<RC>(lane);
  score_products(x, 0, q2[0], stage, lane);
  score_tile_publish();
  SCORE_STAMP(tc1);
  SCORE_STAMP_ADD(9, tb, tc1);
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    const float* cur = TILES == 2 ? stage + (uint32_t)(c & 1) * tile_floats : stage;
    if (TILES == 2 && c + 1 < NB) score_products(x, c + 1, q2[c + 1], stage + (uint32_t)((c + 1) & 1) * tile_floats, lane);
    acc = score_add_row(cur, lrow, acc);
    score_tile_retire();  // two tiles: tile c is rewritten by block c + 2, tile c + 1 is complete
    if (TILES == 1 && c + 1 < NB) {  // one tile: the next block's products only now
      score_products(x, c + 1, q2[c + 1], stage, lane);
      score_tile_publish();
    }
  }
  SCORE_STAMP(tc2);
  SCORE_STAMP_ADD(11, tc1, tc2);
  return sqrtf(acc);
}

// ---------------------------------------------------------------------------------------------
// streamed schedule
// ---------------------------------------------------------------------------------------------
// Distances of query `q` (dpad floats, 8-byte aligned, dpad % 4 == 0) to RC rows: row r (< cnt) is
// rows + readlane(pn, base + r) * dpad.  Returns, in lane r < cnt, sqrt of the reference's sum.  `tile`: kScoreTileFloats
// floats of LDS private to the wave.  Rows past cnt repeat the last one (their sums are ignored).
template <int RC, typename RT>
__device__ __forceinline__ float score_rows_stream(const RT* __restrict__ rows, uint32_t dpad, const float* __restrict__ q, uint32_t pn,
                                                   uint32_t base, uint32_t cnt, float* tile, int lane) {
  const uint32_t nb = (dpad + 127) >> 7;
  using P = typename RowVec<RT>::Pair;
  const RT* rp[RC];
  const uint32_t last = cnt - 1;
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    const uint32_t rr = (uint32_t)r < last ? (uint32_t)r : last;  // wave-uniform
    rp[r] = rows + (size_t)__builtin_amdgcn_readlane(pn, base + rr) * dpad;
  }
  const uint32_t j0 = 2u * (uint32_t)lane;
  auto load = [&](uint32_t c, P (&x)[RC][1], float2& qv) {
    const uint32_t j = c * 128u + j0;
    const bool in = j < dpad;  // dpad % 4 == 0: a pair never straddles the end
    qv = in ? *(const float2*)(q + j) : make_float2(0.0f, 0.0f);
#pragma unroll
    for (int r = 0; r < RC; ++r) x[r][0] = in ? *(const P*)(rp[r] + j) : RowVec<RT>::zero_pair();
  };
  const uint32_t lrow = score_lane_row<RC>(lane);
  float acc = 0.0f;
  auto fold = [&](const P (&x)[RC][1], const float2 qv) {
    score_products(x, 0, qv, tile, lane);
    acc = score_fold(tile, lrow, acc);
  };
  P xa[RC][1], xb[RC][1];
  float2 qa, qb;
  load(0, xa, qa);
  for (uint32_t c = 0; c < nb; c += 2) {
    if (c + 1 < nb) load(c + 1, xb, qb);
    fold(xa, qa);
    if (c + 1 < nb) {
      if (c + 2 < nb) load(c + 2, xa, qa);
      fold(xb, qb);
    }
  }
  return sqrtf(acc);
}

// up to 16 rows, the smallest straight-line form that holds them
template <typename RT>
__device__ __forceinline__ float score_rows_upto16(const RT* __restrict__ rows, uint32_t dpad, const float* __restrict__ q, uint32_t pn,
                                                   uint32_t base, uint32_t cnt, float* tile, int lane) {
  if (cnt > 8) return score_rows_stream<16>(rows, dpad, q, pn, base, cnt, tile, lane);
  if (cnt > 4) return score_rows_stream<8>(rows, dpad, q, pn, base, cnt, tile, lane);
  return score_rows_stream<4>(rows, dpad, q, pn, base, cnt, tile, lane);
}

// lane i < n (n <= 64): distance to row rows + pn_i * dpad; chunks of 16 one after the other
template <typename RT>
__device__ __forceinline__ float score_rows_wave(const RT* __restrict__ rows, uint32_t dpad, const float* __restrict__ q, uint32_t pn,
                                                 uint32_t n, float* tile, int lane) {
  float out = 0.0f;
  for (uint32_t base = 0; base < n; base += 16) {
    const uint32_t cnt = min(16u, n - base);
    const float d = score_rows_upto16(rows, dpad, q, pn, base, cnt, tile, lane);
    const float mine = __shfl(d, (int)((uint32_t)lane - base) & 63);
    if ((uint32_t)lane >= base && (uint32_t)lane < base + cnt) out = mine;
  }
  return out;
}

}  // namespace fvdb
