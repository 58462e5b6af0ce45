// kernels_ivfrpq.h — what the inverted file over RESIDUAL PQ codes adds to kernels_ivfpq.h (DESIGN.md section 9zd;
// include/fvdb.h, "IVF over residual PQ codes").  A row's codes are the quantizer's encode of r = x - c, c its list's
// centroid, and the score of a candidate is split so that nothing a query keeps in LDS depends on the list:
//
//   |q - c - r^|^2 = |q - c|^2 + r^.(r^ + 2c) - 2 q.r^        r^ the decoded residual
//                    base[b][rank]  term[row]    ip from P[b][j][code]
//
//   ivfrpq_encode_kernel   add: lane = source row; the residual is formed while the sub-vectors are staged, encoded by the
//                          quantizer's rule, and the row term is accumulated from the winning centroids: the residual
//                          rows never visit HBM and nothing is decoded afterwards
//   ivfrpq_table_kernel    P[b][j][c] = q_b's sub-vector j . centroid c: subspace j's centroids in LDS once for QB queries
//   ivfrpq_base_kernel     base[b][r] = the squared fold of q_b against the centroid of probe rank r
//
// The scan is kernels_ivfpq.h's own, instantiated with RES.  All arithmetic is f32 with multiply and add separate.
#pragma once
#include "common.h"
#include "kernels_ivfpq.h"
#include "score_rows.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kIvfRpqTableQueries = 8;  // QB: queries of one table workgroup (chosen from the code: section 9zd)

// ---- add: residual, encode and row term in one pass -----------------------------------------------------------------
struct IvfRpqEncodeArgs {
  const float* rows;        // [n][d] source rows, unpadded
  const uint32_t* cluster;  // [n] the list of every source row
  const float* cent;        // [nlist][dpad] centroids, zero beyond d
  const float* books;
  PqGeom g;
  uint64_t n;
  uint32_t nlist, dpad;
  uint8_t* flat;            // [n][m] codes
  float* term;              // [n] row terms
};

// pq_encode_kernel's shape (lane = row, a wave owns 64 rows, subspaces j ascending, 32-dim chunks transposed through the
// wave's LDS tile, the codebook staged in runs of kPqBookFloats) over 64 consecutive SOURCE rows.  The staging thread of
// (row, dim) reads the row's own centroid at the same dim — coalesced like the row, the list id by a lane shuffle — and
// writes x - c, so the registers hold the residual.  After the argmin the tile is used a second time, for the centroid
// slice itself, and the lane adds r^_i * (r^_i + (c_i + c_i)) with r^ the winning centroid: from s_book where the
// subspace was staged in one run, from the codebook in HBM (an L2 hit) where an earlier run may have held the winner.
template <int DMAX>
__global__ __launch_bounds__(256) void ivfrpq_encode_kernel(const IvfRpqEncodeArgs a) {
  __shared__ __attribute__((aligned(16))) float s_tile[4][kFlatTileFloats];
  __shared__ __attribute__((aligned(16))) float s_book[kPqBookFloats];
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const PqGeom g = a.g;
  const uint64_t tile0 = ((uint64_t)blockIdx.x * 4 + w) * 64;  // first source row of the wave's tile
  const uint64_t idx = tile0 + (uint64_t)lane;
  const bool have = idx < a.n;
  float* tile = s_tile[w];
  constexpr int kChunks = DMAX > 32 ? DMAX / 32 : 1;
  constexpr int kQuads = DMAX > 32 ? 8 : DMAX / 4;  // float4s a lane takes of a staged chunk
  const uint32_t mycl = have ? min(a.cluster[idx], a.nlist - 1u) : 0u;

  float term = 0.0f;
  for (uint32_t j = 0; j < g.m; ++j) {
    const uint32_t off = g.off(j), dj = g.dims(j), djp = (dj + 3u) & ~3u;
    float x[DMAX];
#pragma unroll
    for (int i = 0; i < DMAX; ++i) x[i] = 0.0f;
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
      if ((uint32_t)c * 32u < djp) {  // wave-uniform
        const uint32_t dim = (uint32_t)c * 32u + ((uint32_t)lane & 31u);
#pragma unroll 8
        for (uint32_t t = 0; t < 32; ++t) {
          const uint32_t r = 2u * t + ((uint32_t)lane >> 5);
          const uint32_t cl = __shfl(mycl, (int)r);
          float v = 0.0f;
          if (dim < dj && tile0 + r < a.n) v = a.rows[(size_t)(tile0 + r) * g.d + off + dim] - a.cent[(size_t)cl * a.dpad + off + dim];
          tile[r * kFlatStride + ((uint32_t)lane & 31u)] = v;
        }
        score_tile_publish();
        const float4* p = (const float4*)(tile + (uint32_t)lane * kFlatStride);
#pragma unroll
        for (int i = 0; i < kQuads; ++i) {
          const float4 v = p[i];
          x[32 * c + 4 * i + 0] = v.x;
          x[32 * c + 4 * i + 1] = v.y;
          x[32 * c + 4 * i + 2] = v.z;
          x[32 * c + 4 * i + 3] = v.w;
        }
        score_tile_retire();
      }
    }

    float best = __uint_as_float(0x7F800000u);
    uint32_t code = 0;  // every distance +inf: the first centroid, as min_by
    const float* book = a.books + g.book(j);
    const uint32_t per = min(g.ka, kPqBookFloats / djp);
    for (uint32_t c0 = 0; c0 < g.ka; c0 += per) {
      const uint32_t cnt = min(per, g.ka - c0);
      __syncthreads();  // the previous run has been read
      for (uint32_t e = threadIdx.x; e < cnt * djp; e += 256) {
        const uint32_t c = e / djp, i = e - c * djp;
        s_book[e] = i < dj ? book[(size_t)(c0 + c) * dj + i] : 0.0f;
      }
      __syncthreads();
      for (uint32_t c = 0; c < cnt; ++c) {
        const float4* cb = (const float4*)(s_book + c * djp);
        float s = 0.0f, t;
#pragma unroll
        for (int i = 0; i < DMAX / 4; ++i) {
          if ((uint32_t)(4 * i) < djp) {  // wave-uniform
            const float4 v = cb[i];
            t = x[4 * i + 0] - v.x;
            s = s + t * t;
            t = x[4 * i + 1] - v.y;
            s = s + t * t;
            t = x[4 * i + 2] - v.z;
            s = s + t * t;
            t = x[4 * i + 3] - v.w;
            s = s + t * t;
          }
        }
        const float dist = sqrtf(s);
        if (dist < best) {
          best = dist;
          code = c0 + c;
        }
      }
    }
    if (have) a.flat[(size_t)idx * g.m + j] = (uint8_t)code;

    // the row term of this subspace, i ascending: the centroid slices take the way the rows took
    const bool staged = per == g.ka;  // one run: the winner is still in s_book
    const float* win = staged ? s_book + code * djp : book + (size_t)code * dj;
    for (uint32_t c = 0; c * 32u < dj; ++c) {
      const uint32_t dim = c * 32u + ((uint32_t)lane & 31u);
#pragma unroll 8
      for (uint32_t t = 0; t < 32; ++t) {
        const uint32_t r = 2u * t + ((uint32_t)lane >> 5);
        const uint32_t cl = __shfl(mycl, (int)r);
        tile[r * kFlatStride + ((uint32_t)lane & 31u)] = dim < dj ? a.cent[(size_t)cl * a.dpad + off + dim] : 0.0f;
      }
      score_tile_publish();
      const float* cv = tile + (uint32_t)lane * kFlatStride;
      const uint32_t cn = min(32u, dj - c * 32u);
      for (uint32_t i = 0; i < cn; ++i) {
        const float rh = win[c * 32u + i], ci = cv[i];
        term = term + rh * (rh + (ci + ci));
      }
      score_tile_retire();
    }
  }
  if (have) a.term[idx] = term;
}

// ---- the inner-product tables ----------------------------------------------------------------------------------------
// block (j, tile of QB queries), thread = centroid.  Subspace j's centroids are staged once for the tile's queries, in
// runs of at most kPqBookFloats, at a stride of dj | 1 floats: an odd stride sends the 64 centroids a wave reads at
// one dim to 64 different banks (a stride that is a multiple of 32 would send them all to one).  The tile's query
// sub-vectors are read at wave-uniform addresses (scalar loads), one LDS read serves QB multiply-adds, and the stores to
// [B][m][ka] are coalesced over the centroid.
template <int QB>
__global__ __launch_bounds__(256) void ivfrpq_table_kernel(const float* __restrict__ q /* [B][d] */, const float* __restrict__ books, PqGeom g,
                                                           uint32_t B, float* __restrict__ tables /* [B][m][ka] */) {
  __shared__ float s_book[kPqBookFloats];
  const uint32_t j = blockIdx.x, b0 = blockIdx.y * QB;
  const uint32_t off = g.off(j), dj = g.dims(j), st = dj | 1u;
  const uint32_t nq = min((uint32_t)QB, B - b0);
  const float* book = books + g.book(j);
  const uint32_t per = min(min(g.ka, 256u), kPqBookFloats / st);  // st <= 129: at least 47 centroids a run
  for (uint32_t c0 = 0; c0 < g.ka; c0 += per) {
    const uint32_t cnt = min(per, g.ka - c0);
    __syncthreads();  // the previous run has been read
    for (uint32_t e = threadIdx.x; e < cnt * dj; e += 256) {
      const uint32_t c = e / dj, i = e - c * dj;
      s_book[c * st + i] = book[(size_t)(c0 + c) * dj + i];
    }
    __syncthreads();
    const uint32_t c = threadIdx.x;
    if (c < cnt) {
      const float* cb = s_book + c * st;
      float acc[QB];
#pragma unroll
      for (int t = 0; t < QB; ++t) acc[t] = 0.0f;
      for (uint32_t i = 0; i < dj; ++i) {
        const float v = cb[i];
#pragma unroll
        for (int t = 0; t < QB; ++t) {
          const uint32_t b = b0 + min((uint32_t)t, nq - 1u);  // a short tile repeats its last query
          acc[t] = acc[t] + q[(size_t)b * g.d + off + i] * v;
        }
      }
#pragma unroll
      for (int t = 0; t < QB; ++t)
        if ((uint32_t)t < nq) tables[((size_t)(b0 + (uint32_t)t) * g.m + j) * g.ka + c0 + c] = acc[t];
    }
  }
}

// ---- base[b][r] -------------------------------------------------------------------------------------------------------
// One wave per (query, 16 probe ranks), lane = rank: score_rows.h's core in its streamed schedule (coalesced loads of
// the centroid rows, the products transposed through the wave's tile, lane r adds row r's products in dimension order)
// without the root, which the score takes after the whole sum.  q: [B][dpad] with dpad % 4 == 0, zero beyond d, as the
// centroid rows are.  A probe entry that names no list scores list 0; the scan never reads its base.
static __global__ __launch_bounds__(256) void ivfrpq_base_kernel(const float* __restrict__ q, const float* __restrict__ cent, uint32_t dpad,
                                                                 const uint32_t* __restrict__ probes, uint32_t B, uint32_t np, uint32_t nlist,
                                                                 float* __restrict__ base /* [B][np] */) {
  __shared__ __attribute__((aligned(16))) float s_tile[4][kScoreTileFloats];
  constexpr int RC = 16;
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6, b = blockIdx.y;
  const uint32_t r0 = (blockIdx.x * 4 + w) * RC;
  if (r0 >= np) return;  // whole waves leave; no workgroup barrier below
  const uint32_t cnt = min((uint32_t)RC, np - r0);
  float* tile = s_tile[w];
  uint32_t pn = 0;
  if ((uint32_t)lane < cnt) {
    pn = probes[(size_t)b * np + r0 + (uint32_t)lane];
    if (pn >= nlist) pn = 0;
  }
  const float* qb = q + (size_t)b * dpad;
  const float* rp[RC];
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    const uint32_t rr = (uint32_t)r < cnt - 1 ? (uint32_t)r : cnt - 1;  // wave-uniform; rows past cnt repeat the last one
    rp[r] = cent + (size_t)__builtin_amdgcn_readlane(pn, rr) * dpad;
  }
  const uint32_t lrow = score_lane_row<RC>(lane);
  const uint32_t nb = (dpad + 127) >> 7;
  float acc = 0.0f;
  for (uint32_t c = 0; c < nb; ++c) {
    const uint32_t jx = c * 128u + 2u * (uint32_t)lane;
    const bool in = jx < dpad;  // dpad % 4 == 0: a pair never straddles the end
    const float2 qv = in ? *(const float2*)(qb + jx) : make_float2(0.0f, 0.0f);
    float2 x[RC][1];
#pragma unroll
    for (int r = 0; r < RC; ++r) x[r][0] = in ? *(const float2*)(rp[r] + jx) : make_float2(0.0f, 0.0f);
    score_products(x, 0, qv, tile, lane);
    acc = score_fold(tile, lrow, acc);
  }
  if ((uint32_t)lane < cnt) base[(size_t)b * np + r0 + (uint32_t)lane] = acc;
}

}  // namespace fvdb
