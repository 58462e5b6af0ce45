// kernels_flat.h — the flat exact scan of a graph's row store: every live node scored against
// every query of the batch with the reference's distance (src/core/vector_ops.rs:51-57: t = q_i - x_i; sum = sum + t*t,
// i ascending, f32, multiply and add separate, sqrt correctly rounded), the k best per query kept by the unique key
// (distance bits << 32 | node index).  An fp16 row is widened exactly first (row_types.h).
//
//   flat_fold_slice     the work of one wave, shared with the wide form (kernels_flat_wide.h): the distances of the rows of
//                       a slice of 64-row tiles to a group of Q queries, tile by tile, handed to the caller's sink
//   flat_scan_kernel    one wave per (group of Q queries, slice of 64-row tiles): per-(query, slice) top k
//   flat_merge_kernel   one wave per query: the slices' lists merged by the same key, the result block written
//
// Mapping (the list scan's, kernels_scan.h, adapted to row-major rows): lane = row, the Q queries of a group are
// wave-uniform and arrive through the scalar path (cload16), so a row chunk held in VGPRs serves Q running sums.  The
// store is row-major, so a chunk of kFlatChunk dimensions of the 64 rows of a tile is loaded COALESCED — 8 lanes read
// the 128 (f32) or 64 (fp16) contiguous bytes of one row, 8 rows per load instruction — and transposed through a tile of
// LDS private to the wave into "lane = row, dimension order".  The next chunk's global loads (the next tile's first
// chunk after a tile's last) are issued before the fold of the present one, so they are in flight while it runs.
//
// LDS: row stride 36 floats = 9 quads; ds_read_b128 is served in groups of 16 lanes whose indices are distinct mod 16
// (MI355X: {0-3,12-15,20-27}, ...), 9 r mod 16 is then distinct too, so the 16 reads of a group cover the 64 banks once.
#pragma once
#include "common.h"
#include "kernels_scan.h"
#include "row_types.h"
#include "score_rows.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kFlatChunk = 32;                        // dimensions per staged chunk (two cload16 per query)
constexpr uint32_t kFlatStride = kFlatChunk + 4;           // floats per staged row
constexpr uint32_t kFlatTileFloats = 64 * kFlatStride;     // one wave's tile: 9216 bytes

struct FlatScanArgs {
  const void* rows;       // the store: [node][dpad] of the kernel's RT
  const float* queries;   // [B][dpad], zero beyond d, 16-byte aligned
  const uint32_t* dead;   // [n]: non-zero = not live (the graph's deleted flags, or a mask's)
  uint32_t dpad, n, B, k;
  uint32_t slices, slice_tiles;  // slice s = tiles [s * slice_tiles, min(tiles, (s + 1) * slice_tiles)), a tile = 64 rows
  uint64_t* part;                // [slices][B][k] keys, ~0 = none
};

// One wave's pass over the 64-row tiles [t0, t1) of the store against Q queries (queries + qoff[j], wave-uniform): the
// prefetch, the staging of a chunk into the wave's LDS tile, the read-back as "lane = row" and the fold — the ONE text
// of it, so flat_scan_kernel and flat_score_kernel (kernels_flat_wide.h) round alike.  At the end of tile t it calls
// sink(t, row, live, acc): row = 64 t + lane, live = row < n && !dead[row], acc[j] = the squared distance to query j
// (the sqrtf is the sink's).  No workgroup barrier: waves of a workgroup run slices of different lengths.
template <int Q, typename RT, class Sink>
__device__ __forceinline__ void flat_fold_slice(const RT* rows, const float* queries, const uint32_t* dead, const uint32_t dpad,
                                                const uint32_t n, const uint32_t (&qoff)[Q], float* tile, const uint32_t t0,
                                                const uint32_t t1, const int lane, Sink&& sink) {
  using Quad = typename RowVec<RT>::Quad;
  const uint32_t nchunks = (dpad + kFlatChunk - 1) / kFlatChunk;
  const uint32_t lr = (uint32_t)lane >> 3, lc = 4u * ((uint32_t)lane & 7u);  // the load role: row within 8, dims within the chunk

  // chunk c of tile t: instruction i reads dims [32 c + lc, + 4) of row 64 t + 8 i + lr (rows at or beyond n repeat the
  // last one: a valid address, never live)
  Quad x[8];
  auto load = [&](uint32_t t, uint32_t c) {
    const uint32_t j = c * kFlatChunk + lc;
    const bool in = j < dpad;  // dpad % 4 == 0: a quad never straddles the end
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t row = min(t * 64u + (uint32_t)i * 8u + lr, n - 1u);
      Quad v = {};
      if (in) v = *(const Quad*)(rows + (size_t)row * dpad + j);
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
        const float* qb = queries + dbase;
        if (dbase + 16u <= dpad) {
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
            if (dbase + 4u * (uint32_t)i4 < dpad) {
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
    const uint32_t row = t * 64u + (uint32_t)lane;
    const bool live = row < n && dead[row] == 0u;
    sink(t, row, live, acc);
  }
}

template <int Q, int KR, typename RT>
__global__ __launch_bounds__(256) void flat_scan_kernel(const FlatScanArgs a) {
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

  WaveTopK<KR> tk[Q];
#pragma unroll
  for (int j = 0; j < Q; ++j) tk[j].init();

  auto keep = [&](uint32_t t, uint32_t row, bool live, const float(&acc)[Q]) {
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const float dist = sqrtf(acc[j]);
      const uint32_t chi = live ? __float_as_uint(dist) : kInf32;
      if (t == t0) {  // empty list: the sorted tile IS the list (registers 1.. stay +inf)
        uint32_t shi = chi, slo = live ? row : kInf32;
        wave_sort64(shi, slo, lane);
        tk[j].hi[0] = shi;
        tk[j].lo[0] = slo;
      } else {
        uint32_t th, tl;
        tk[j].kth(a.k, th, tl);
        offer<KR>(tk[j], a.k, chi, row, th, tl, lane);
      }
    }
  };
  flat_fold_slice<Q>((const RT*)a.rows, a.queries, a.dead, a.dpad, a.n, qoff, s_tile[w], t0, t1, lane, keep);

#pragma unroll
  for (int j = 0; j < Q; ++j) {
    if ((uint32_t)j < ne) {
      uint64_t* out = a.part + ((size_t)s * a.B + q0 + j) * a.k;
#pragma unroll
      for (int rr = 0; rr < KR; ++rr) {
        const uint32_t e = rr * 64 + lane;
        if (e < a.k) out[e] = ((uint64_t)tk[j].hi[rr] << 32) | tk[j].lo[rr];  // (kInf32, kInf32) = ~0 where the list is short
      }
    }
  }
}

// one wave per query: the slices' lists merged by key (allow_merge_kernel's form; the key's low word is the node index
// itself).  slices == 0 writes empty rows.
template <int KR>
__global__ __launch_bounds__(256) void flat_merge_kernel(const uint64_t* __restrict__ part, uint32_t slices, uint32_t B, uint32_t k,
                                                         uint32_t* __restrict__ out_nodes, float* __restrict__ out_dist,
                                                         uint32_t* __restrict__ out_counts) {
  const int lane = threadIdx.x & 63;
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= B) return;
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
      out_nodes[(size_t)q * k + e] = have ? tk.lo[rr] : 0xFFFFFFFFu;
      out_dist[(size_t)q * k + e] = have ? __uint_as_float(tk.hi[rr]) : __uint_as_float(0x7F800000u);
    }
  }
  if (lane == 0) out_counts[q] = count;
}

}  // namespace fvdb
