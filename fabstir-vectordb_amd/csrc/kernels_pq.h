// kernels_pq.h — product quantization on the device: the reference's ProductQuantizer
// (src/core/vector_ops.rs:390-578: train, encode, decode) and the search over codes the C ABI defines beside it.
//
//   pq_encode_kernel     lane = row, a wave owns a 64-row tile and walks the subspaces; nearest centroid per subspace
//   pq_update_kernel     one block per (subspace, centroid): the member sum in data order, the mean, the refill copy
//   pq_decode_kernel     a gather of centroid slices
//   pq_table_kernel      T[b][j][c]: the squared fold of query b's sub-vector j against centroid c
//   pq_adc_scan_kernel   the hot path: one workgroup per QT queries, their tables in LDS, lane = row over 64-row code blocks
//   pq_refine_kernel     one wave per query: the ADC candidates re-scored against their stored rows (score_rows.h)
//
// Arithmetic is the reference's euclidean_distance_scalar everywhere a distance is formed: t = a_i - b_i; s = s + t*t,
// i ascending, f32, multiply and add separate (this file is compiled with -ffp-contract=off and carries the pragma
// below), sqrtf correctly rounded.  Encode compares AFTER the root with a strict <, so two sums the root merges tie and
// the lower centroid wins (min_by keeps the first).  No matrix instruction fits: encode and the tables must be that
// sequential fold, and the scan is table lookups and adds.
//
// Subspace geometry (the reference's, :411-421): dsub = d / m, subspace j covers dims [j dsub, (j + 1) dsub), the last one
// runs to d.  A codebook is [m][ka][dims of j] f32, ka = ksub_actual: subspace j starts at float ka * j * dsub.
// Staged sub-vectors and centroids are padded to a multiple of four dims with zeros: (0 - 0)^2 = +0 leaves an f32 sum
// of non-negative terms unchanged.
#pragma once
#include "common.h"
#include "kernels_flat.h"
#include "kernels_refine.h"
#include "score_rows.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kPqMaxSubDims = 128;   // dims of one subspace (the encode kernel's registers)
constexpr uint32_t kPqMaxDims = 2048;
constexpr uint32_t kPqBookFloats = 6144;  // staged centroids of one subspace: 24 KiB beside the four 9 KiB tiles
constexpr int kPqAhead = 8;               // code words a scan wave keeps in flight: 8 KiB (half of it at four queries)

// ---- encode ---------------------------------------------------------------------------------------------------------
struct PqEncodeArgs {
  const float* rows;   // [n][d], row-major, unpadded
  const float* books;
  PqGeom g;
  uint64_t n;          // source rows
  uint64_t first;      // index row of source row 0 (block form; 0 for the flat form)
  uint8_t* flat;       // [n][m] codes, or null
  uint4* blocks;       // codes[(block * m16 + chunk) * 64 + lane]: 16 consecutive codes of row 64 block + lane, or null
  uint32_t m16;        // 16-code chunks of a row
};

// A tile is 64 consecutive INDEX rows aligned to a code block, so a lane's 16-byte code word is its own and one wave
// store covers 1 KiB; index row i is source row i - first.  Per subspace: the tile's sub-vectors come in 32-dim chunks,
// coalesced (32 lanes read 128 contiguous bytes of one row) and transposed through the wave's LDS tile at
// flat_fold_slice's stride (36 floats: a lane's ds_read_b128s cover the banks once) into registers; the codebook is
// staged once per workgroup (in runs of kPqBookFloats) and every lane reads the same centroid address — a broadcast.
// All four waves stay to the end: the staging has workgroup barriers.
template <int DMAX>
__global__ __launch_bounds__(256) void pq_encode_kernel(const PqEncodeArgs a) {
  __shared__ __attribute__((aligned(16))) float s_tile[4][kFlatTileFloats];
  __shared__ __attribute__((aligned(16))) float s_book[kPqBookFloats];
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const PqGeom g = a.g;
  const uint64_t tile0 = (a.first / 64 + (uint64_t)blockIdx.x * 4 + w) * 64;  // first index row of the wave's tile
  const uint64_t idx = tile0 + (uint64_t)lane;
  const bool have = idx >= a.first && idx - a.first < a.n;
  float* tile = s_tile[w];
  constexpr int kChunks = DMAX > 32 ? DMAX / 32 : 1;
  constexpr int kQuads = DMAX > 32 ? 8 : DMAX / 4;  // float4s a lane takes of a staged chunk

  uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
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
          const uint64_t ir = tile0 + r;
          float v = 0.0f;
          if (dim < dj && ir >= a.first && ir - a.first < a.n) v = a.rows[(size_t)(ir - a.first) * g.d + off + dim];
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

    if (a.flat) {
      if (have) a.flat[(size_t)(idx - a.first) * g.m + j] = (uint8_t)code;
    } else {
      const uint32_t sh = code << (8u * (j & 3u)), sel = (j >> 2) & 3u;  // sel is wave-uniform
      if (sel == 0) w0 |= sh;
      else if (sel == 1) w1 |= sh;
      else if (sel == 2) w2 |= sh;
      else w3 |= sh;
      if ((j & 15u) == 15u || j + 1 == g.m) {  // pad codes of the last chunk stay 0
        if (have) a.blocks[((size_t)(idx >> 6) * a.m16 + (j >> 4)) * 64 + (uint32_t)lane] = make_uint4(w0, w1, w2, w3);
        w0 = w1 = w2 = w3 = 0;
      }
    }
  }
}

// ---- one Lloyd update (vector_ops.rs:467-523) ------------------------------------------------------------------------
struct PqUpdateArgs {
  const float* rows;       // [n][d] training rows
  const uint8_t* codes;    // [n][m]: the assignment
  float* books;
  const uint32_t* refill;  // [m][ka]: the training row an empty centroid becomes a copy of
  PqGeom g;
  uint64_t n;
};

// block (c, j), thread = dim: the members of centroid c of subspace j are found 128 rows at a time (two ballots) and
// added in data order from 0.0f; the sum is divided by (float)count.
static __global__ __launch_bounds__(128) void pq_update_kernel(const PqUpdateArgs a) {
  __shared__ uint64_t s_mask[2];
  const PqGeom g = a.g;
  const uint32_t c = blockIdx.x, j = blockIdx.y, i = threadIdx.x;
  const uint32_t off = g.off(j), dj = g.dims(j);
  float acc = 0.0f;
  uint32_t count = 0;
  for (uint64_t r0 = 0; r0 < a.n; r0 += 128) {
    const uint64_t r = r0 + i;
    const bool mine = r < a.n && a.codes[(size_t)r * g.m + j] == c;
    const uint64_t b = __ballot(mine);
    if ((i & 63u) == 0) s_mask[i >> 6] = b;
    __syncthreads();
    for (uint32_t h = 0; h < 2; ++h) {
      uint64_t mk = s_mask[h];
      count += (uint32_t)__popcll(mk);
      while (mk) {
        const uint32_t l = (uint32_t)__builtin_ctzll(mk);
        mk &= mk - 1;
        if (i < dj) acc = acc + a.rows[(size_t)(r0 + 64u * h + l) * g.d + off + i];
      }
    }
    __syncthreads();
  }
  if (i < dj) {
    float* out = a.books + g.book(j) + (size_t)c * dj + i;
    *out = count ? acc / (float)count : a.rows[(size_t)a.refill[j * g.ka + c] * g.d + off + i];
  }
}

// ---- decode (vector_ops.rs:563-577) ----------------------------------------------------------------------------------
// one thread per output float, bit copies; a code at or above ka reads the last centroid (the host form refuses it first)
static __global__ void pq_decode_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ books, PqGeom g, uint64_t n,
                                 float* __restrict__ out) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * g.d) return;
  const uint64_t r = e / g.d;
  const uint32_t i = (uint32_t)(e - r * g.d);
  const uint32_t j = min(i / g.dsub, g.m - 1);
  const uint32_t c = min((uint32_t)codes[r * g.m + j], g.ka - 1);
  out[e] = books[g.book(j) + (size_t)c * g.dims(j) + (i - g.off(j))];
}

// ---- the ADC tables --------------------------------------------------------------------------------------------------
// block (j, b): T[b][j][c] for every c, one thread per entry; the query's sub-vector is wave-uniform (scalar loads)
static __global__ __launch_bounds__(256) void pq_table_kernel(const float* __restrict__ q /* [B][d] */, const float* __restrict__ books, PqGeom g,
                                                       float* __restrict__ tables /* [B][m][ka] */) {
  const uint32_t j = blockIdx.x, b = blockIdx.y;
  const uint32_t off = g.off(j), dj = g.dims(j);
  const float* qs = q + (size_t)b * g.d + off;
  const float* book = books + g.book(j);
  for (uint32_t c = threadIdx.x; c < g.ka; c += 256) {
    const float* cb = book + (size_t)c * dj;
    float s = 0.0f;
    for (uint32_t i = 0; i < dj; ++i) {
      const float t = qs[i] - cb[i];
      s = s + t * t;
    }
    tables[((size_t)b * g.m + j) * g.ka + c] = s;
  }
}

// ---- the ADC scan ----------------------------------------------------------------------------------------------------
struct PqScanArgs {
  const uint4* codes;    // [blocks][m16][64] code words
  const uint32_t* dead;  // [n]: non-zero = not live (deleted, or outside an allow-set)
  const float* tables;   // [B][m][ka]
  uint64_t* part;        // [slices][B][k] keys (adc bits << 32 | row), ~0 = none
  uint32_t n, m, m16, ka, ts /* floats of a table row in LDS: ka or ka + 1 */, B, k, slices, slice_blocks;
};

// 16 codes of a lane against the tables of QT queries: acc[q] = acc[q] + T_q[j][code_j], j ascending
template <int QT, bool FULL>
__device__ __forceinline__ void pq_fold_word(const uint4 cw, const float* tab, uint32_t tsz, uint32_t ts, uint32_t jn, float (&acc)[QT]) {
  const uint32_t wv[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (FULL || (uint32_t)i < jn) {  // wave-uniform
      const uint32_t code = (wv[i >> 2] >> (8 * (i & 3))) & 255u;
      const float* e = tab + (uint32_t)i * ts + code;
#pragma unroll
      for (int q = 0; q < QT; ++q) acc[q] = acc[q] + e[(uint32_t)q * tsz];
    }
  }
}

// Workgroup = 4 waves and QT queries: their tables go to LDS, one barrier, then each wave runs its own slice of code
// blocks.  A slice is one contiguous run of 1 KiB code words; kPqAhead of them are in flight while one is folded.
template <int QT, int KR>
__global__ __launch_bounds__(256) void pq_adc_scan_kernel(const PqScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_tab[];  // [QT][m][ts]
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t q0 = blockIdx.x * QT;
  const uint32_t ne = min((uint32_t)QT, a.B - q0);
  const uint32_t tsz = a.m * a.ts;
#pragma unroll
  for (int q = 0; q < QT; ++q) {  // a short group repeats its first query
    const float* src = a.tables + (size_t)(q0 + ((uint32_t)q < ne ? (uint32_t)q : 0u)) * a.m * a.ka;
    for (uint32_t e = threadIdx.x; e < tsz; e += 256) {
      const uint32_t j = e / a.ts, c = e - j * a.ts;
      s_tab[(uint32_t)q * tsz + e] = c < a.ka ? src[j * a.ka + c] : 0.0f;
    }
  }
  __syncthreads();
  const uint32_t s = blockIdx.y * 4 + w;
  if (s >= a.slices) return;  // whole waves leave; no workgroup barrier below
  const uint32_t blocks = (a.n + 63) >> 6;
  const uint32_t b0 = s * a.slice_blocks, b1 = min(blocks, b0 + a.slice_blocks);
  const uint64_t nw = (uint64_t)(b1 - b0) * a.m16;  // words of the slice
  const uint4* p = a.codes + ((size_t)b0 * a.m16) * 64 + (uint32_t)lane;

  WaveTopK<KR> tk[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) tk[q].init();

  constexpr int AH = QT == 4 ? kPqAhead / 2 : kPqAhead;  // four queries: the unrolled body of eight words no longer stays in registers
  uint4 buf[AH];
#pragma unroll
  for (int u = 0; u < AH; ++u) buf[u] = (uint64_t)u < nw ? p[(size_t)u * 64] : make_uint4(0, 0, 0, 0);

  uint32_t chunk = 0, blk = b0;
  float acc[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) acc[q] = 0.0f;
  for (uint64_t wi = 0; wi < nw; wi += AH) {
#pragma unroll
    for (int u = 0; u < AH; ++u) {
      if (wi + u < nw) {  // wave-uniform
        const uint4 cw = buf[u];
        if (wi + u + AH < nw) buf[u] = p[(size_t)(wi + u + AH) * 64];
        const uint32_t jn = min(16u, a.m - 16u * chunk);
        const float* tab = s_tab + 16u * chunk * a.ts;
        if (jn == 16u) pq_fold_word<QT, true>(cw, tab, tsz, a.ts, jn, acc);
        else pq_fold_word<QT, false>(cw, tab, tsz, a.ts, jn, acc);
        if (++chunk == a.m16) {
          const uint32_t row = blk * 64u + (uint32_t)lane;
          const bool live = row < a.n && a.dead[row] == 0u;
#pragma unroll
          for (int q = 0; q < QT; ++q) {
            const float dist = sqrtf(acc[q]);
            acc[q] = 0.0f;
            const uint32_t chi = live ? __float_as_uint(dist) : kInf32;
            if (blk == b0) {  // empty list: the sorted tile IS the list
              uint32_t shi = chi, slo = live ? row : kInf32;
              wave_sort64(shi, slo, lane);
              tk[q].hi[0] = shi;
              tk[q].lo[0] = slo;
            } else {
              uint32_t th, tl;
              tk[q].kth(a.k, th, tl);
              offer<KR>(tk[q], a.k, chi, row, th, tl, lane);
            }
          }
          chunk = 0;
          ++blk;
        }
      }
    }
  }

#pragma unroll
  for (int q = 0; q < QT; ++q) {
    if ((uint32_t)q < ne) {
      uint64_t* out = a.part + ((size_t)s * a.B + q0 + q) * a.k;
#pragma unroll
      for (int rr = 0; rr < KR; ++rr) {
        const uint32_t e = rr * 64 + lane;
        if (e < a.k) out[e] = ((uint64_t)tk[q].hi[rr] << 32) | tk[q].lo[rr];
      }
    }
  }
}

// rows of a merged result to the caller's ids
static __global__ void pq_map_ids_kernel(const uint32_t* __restrict__ nodes, const uint64_t* __restrict__ ids, uint64_t total,
                                  uint64_t* __restrict__ out_ids) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const uint32_t r = nodes[e];
  out_ids[e] = r == 0xFFFFFFFFu ? ~0ull : ids[r];
}

// ---- refine ----------------------------------------------------------------------------------------------------------
// one wave per query over the ADC candidates (kernels_refine.h, shared with the SQ8 index)
using PqRefineArgs = RefineArgs;

template <int KR, typename RT>
__global__ __launch_bounds__(256) void pq_refine_kernel(const PqRefineArgs a) {
  __shared__ __attribute__((aligned(16))) float s_tile[4][kScoreTileFloats];
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x * 4 + w;
  if (q >= a.B) return;
  refine_wave<KR, RT>(a, q, s_tile[w], lane);
}

// ---- small helpers ---------------------------------------------------------------------------------------------------
// [B][d] -> [B][dpad], zero beyond d
static __global__ void pq_pad_queries_kernel(const float* __restrict__ src, uint32_t d, uint32_t dpad, uint64_t B, float* __restrict__ dst) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * dpad) return;
  const uint64_t b = e / dpad;
  const uint32_t i = (uint32_t)(e - b * dpad);
  dst[e] = i < d ? src[b * d + i] : 0.0f;
}

static __global__ void pq_set_flags_kernel(const uint32_t* __restrict__ rows, uint64_t n, uint32_t flag, uint32_t* __restrict__ dead) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) dead[rows[e]] = flag;
}

}  // namespace fvdb
