// kernels_bq.h — binary quantization on the device (include/fvdb.h, "binary quantization"): one
// sign bit a dimension, the Hamming search over those codes, and the exact re-score of its candidates.
//
//   bq_encode_kernel   one wave per row, lane = dim: a ballot of (x - c) > 0 is 64 code bits; the same kernel writes the
//                      flat form, the index form and the queries of a search
//   bq_scan_kernel     the hot path: lane = row, a wave holds a 64-row block's codes in registers and walks a tile of 32
//                      queries whose words arrive through the scalar path; W xor and W popcount-adds a pair
//   bq_refine_kernel   kernels_refine.h's wave over the stored rows
//
// Index form.  Blocks of 64 rows; word (block, chunk, lane) is 16 bytes: code words 4 chunk .. 4 chunk + 3 (128 dims) of
// row 64 block + lane, so a wave's load is 1 KiB contiguous and a row's code is C loads of 16 bytes.  C = the chunks of
// a row rounded up to a count the scan is built for (1, 2, 3, 4, 8, 16); dims beyond d and words beyond W are 0 on both
// sides and add nothing to a distance.  The queries of a search are encoded as [query][4 C] words.
#pragma once
#include "common.h"
#include "kernels_flat.h"
#include "kernels_refine.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kBqMaxDims = 2048;
constexpr uint32_t kBqTile = 32;           // queries of a scan workgroup (lane j of a wave keeps query j's bound): three workgroups a CU at k <= 64
constexpr uint32_t kBqRoundRows = 256;     // rows a workgroup scores between two looks at its survivor buffers
constexpr uint32_t kBqSlack = 64;          // keys a buffer takes beyond 64 KR before it is cut: k = 64 KR is not cut every round
constexpr uint32_t kBqRowBits = 20;        // an in-slice key is (ham << 20) | row in slice: 12 bits hold ham <= 2048
constexpr uint32_t kBqMaxSliceBlocks = (1u << kBqRowBits) / 64;

typedef uint32_t bq_u32x4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline uint32_t bq_words(uint32_t d) { return (d + 31u) >> 5; }
// 16-byte words of a row in the index: ceil(W / 4), rounded up to an instantiation of the scan
__host__ __device__ inline uint32_t bq_chunks(uint32_t d) {
  const uint32_t c = (bq_words(d) + 3u) >> 2;
  return c <= 4u ? c : (c <= 8u ? 8u : 16u);
}
__host__ __device__ inline uint32_t bq_buf_cap(uint32_t kr) { return kr * 64u + kBqSlack + kBqRoundRows; }
// dynamic LDS of a scan workgroup: the 4-byte survivor buffers, then a count and a bound per query
__host__ __device__ inline uint32_t bq_scan_lds(uint32_t kr) { return kBqTile * bq_buf_cap(kr) * 4u + 2u * kBqTile * 4u; }

// ---- encode ------------------------------------------------------------------------------------------------------------
struct BqEncodeArgs {
  const float* rows;    // [n][d], row-major, unpadded
  const float* centre;  // [d], or null = zeros
  uint32_t d, chunks;
  uint64_t n;
  uint64_t first;       // index row of source row 0 (index form)
  uint8_t* flat;        // [n][ceil(d / 8)] bytes, dim i = bit i & 7 of byte i >> 3; or null
  uint32_t* blocks;     // the index form above as words; or null
  uint32_t* per_row;    // [n][4 chunks] words, a row's words together (a search's queries); or null
};

// Pass p covers dims 64 p .. 64 p + 63, one a lane, from 256 contiguous bytes: bit = (x - c) > 0, one f32 subtraction
// (so -0 and +0 give 0 and a subnormal difference keeps its sign); a dim at or beyond d gives 0.  The ballot is code
// words 2 p and 2 p + 1: lanes 0 and 1 write them (word forms, through word 4 chunks - 1), lanes 0..7 its bytes (flat form).
static __global__ __launch_bounds__(256) void bq_encode_kernel(const BqEncodeArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.n) return;  // whole waves leave; no barrier below
  const float* row = a.rows + (size_t)r * a.d;
  const uint32_t nwords = 4u * a.chunks, nbytes = (a.d + 7u) >> 3;
  const uint32_t passes = a.flat ? (a.d + 63u) >> 6 : 2u * a.chunks;
  const uint64_t idx = a.first + r;
  for (uint32_t p = 0; p < passes; ++p) {
    const uint32_t i = 64u * p + lane;
    bool bit = false;
    if (i < a.d) {
      const float t = row[i] - (a.centre ? a.centre[i] : 0.0f);
      bit = t > 0.0f;
    }
    const uint64_t m = __ballot(bit);
    if (a.flat) {
      const uint32_t b = 8u * p + lane;
      if (lane < 8u && b < nbytes) a.flat[(size_t)r * nbytes + b] = (uint8_t)(m >> (8u * lane));
    } else {
      const uint32_t wi = 2u * p + lane;
      if (lane < 2u && wi < nwords) {
        const uint32_t word = (uint32_t)(m >> (32u * lane));
        if (a.per_row) a.per_row[(size_t)r * nwords + wi] = word;
        else a.blocks[(((size_t)(idx >> 6) * a.chunks + (wi >> 2)) * 64u + (uint32_t)(idx & 63u)) * 4u + (wi & 3u)] = word;
      }
    }
  }
}

// ---- the Hamming scan ------------------------------------------------------------------------------------------------
struct BqScanArgs {
  const uint4* codes;      // [blocks][C][64] row words
  const uint32_t* dead;    // [rows]: non-zero = not a candidate (deleted, or outside an allow-set)
  const uint32_t* qcodes;  // [B][4 C] query words
  uint64_t* part;          // [slices][B][k] keys (bits((float)ham) << 32 | row), ~0 = none
  uint32_t n, B, k, slices, slice_blocks;  // slice_blocks <= kBqMaxSliceBlocks
};

// The cut of one query's buffer by one wave: cnt > k unique 4-byte keys, 64 KR + 320 at the most, KR + 5 a lane in
// registers.  The k-th smallest key v is found bit by bit from the top — v keeps a bit iff fewer than k keys lie below
// v with that bit set, a ballot and a count a register — so the cost is 32 steps whatever the keys are, with no sort
// and no insertion.  The keys <= v, exactly k of them, go back to buf[0 .. k) by ballot rank, in no particular order
// (the merge takes them in any order).  Returns v.
template <int KR>
__device__ __forceinline__ uint32_t bq_cut(uint32_t* buf, uint32_t cnt, uint32_t k, int lane) {
  constexpr int NK = KR + 5;  // bq_buf_cap / 64
  uint32_t key[NK];
#pragma unroll
  for (int i = 0; i < NK; ++i) {
    const uint32_t e = i * 64 + lane;
    key[i] = e < cnt ? buf[e] : kInf32;
  }
  uint32_t v = 0;
#pragma unroll 1
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t t = v | (1u << bit);
    uint32_t below = 0;
#pragma unroll
    for (int i = 0; i < NK; ++i) below += (uint32_t)__popcll(__ballot(key[i] < t));
    if (below < k) v = t;  // wave-uniform
  }
  uint32_t base = 0;
#pragma unroll
  for (int i = 0; i < NK; ++i) {
    const bool keep = key[i] <= v;
    const uint64_t m = __ballot(keep);
    if (keep) buf[base + ballot_rank(m, (uint32_t)lane)] = key[i];
    base += (uint32_t)__popcll(m);
  }
  return v;
}

// Workgroup = 4 waves, one tile of 32 queries (grid x) and one contiguous slice of 64-row blocks (grid y), a quarter of
// it per wave.  A round is one block per wave: its C words sit in registers (the next block's are loaded behind the
// query loop), and for every query of the tile the wave reads the query's words as scalars, folds W xor / popcount
// pairs into ham and forms the in-slice key (ham << 20) | row in slice.  The key is unique in the slice and ordered as
// the result is, so the test against the query's bound — the k-th key of the last cut, kept by lane = query and read
// with v_readlane — is exact under any number of ties: a key at or above it can never enter.  A survivor is appended to
// the query's LDS buffer (an LDS counter hands out the slot).  Between two barriers wave w then looks at buffers
// 8 w .. 8 w + 7: one holding more than 64 KR + 64 keys is cut to its k best and the bound becomes the k-th key.  A
// buffer holds 64 KR + 64 + 256 keys and a round adds at most 256 to at most 64 KR + 64, so none overflows.  Every
// wave runs every round, with or without a block of its own: the barriers are workgroup-wide.
template <int KR, int C>
__global__ __launch_bounds__(256) void bq_scan_kernel(const BqScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  constexpr uint32_t CAP = KR * 64u + kBqSlack + kBqRoundRows;
  uint32_t* s_buf = (uint32_t*)s_raw;  // [32][CAP]
  uint32_t* s_cnt = s_buf + kBqTile * CAP;
  uint32_t* s_bound = s_cnt + kBqTile;
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t q0 = blockIdx.x * kBqTile;
  const uint32_t nq = min(kBqTile, a.B - q0);
  const bq_u32x4* qc = (const bq_u32x4*)a.qcodes + (size_t)q0 * C;

  if (threadIdx.x < kBqTile) {
    s_cnt[threadIdx.x] = 0u;
    s_bound[threadIdx.x] = kInf32;
  }
  __syncthreads();

  const uint32_t blocks = (a.n + 63u) >> 6;
  const uint32_t b0 = blockIdx.y * a.slice_blocks, b1 = min(blocks, b0 + a.slice_blocks);
  const uint32_t nb = b1 - b0, rounds = (nb + 3u) >> 2;  // workgroup-uniform
  const uint32_t wb0 = b0 + min(nb, w * rounds);         // the wave's quarter
  const uint32_t nbw = b0 + min(nb, (w + 1u) * rounds) - wb0;
  const uint4* p = a.codes + (size_t)wb0 * C * 64 + (uint32_t)lane;

  uint4 nxt[C];
  uint32_t nxt_dead = 1u;
  auto load = [&](uint32_t r) {  // block wb0 + r: rows at or beyond n are zero words of the last block, never live
#pragma unroll
    for (int c = 0; c < C; ++c) nxt[c] = p[((size_t)r * C + c) * 64];
    const uint32_t row = (wb0 + r) * 64u + (uint32_t)lane;
    nxt_dead = row < a.n ? a.dead[row] : 1u;
  };
#pragma unroll
  for (int c = 0; c < C; ++c) nxt[c] = make_uint4(0u, 0u, 0u, 0u);
  if (nbw) load(0);

  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t vbound = s_bound[(uint32_t)lane & (kBqTile - 1u)];  // lane j < 32: query j's bound
    if (r < nbw) {                          // wave-uniform
      uint4 cur[C];
#pragma unroll
      for (int c = 0; c < C; ++c) cur[c] = nxt[c];
      const bool live = nxt_dead == 0u;
      if (r + 1u < nbw) load(r + 1u);
      const uint32_t rel = (wb0 + r - b0) * 64u + (uint32_t)lane;  // < 2^20
      auto score = [&](uint32_t j, const bq_u32x4(&qv)[C]) {
        uint32_t ham = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          ham += __popc(cur[c].x ^ qv[c][0]);
          ham += __popc(cur[c].y ^ qv[c][1]);
          ham += __popc(cur[c].z ^ qv[c][2]);
          ham += __popc(cur[c].w ^ qv[c][3]);
        }
        const uint32_t key = (ham << kBqRowBits) | rel;
        if (live && key < rlane(vbound, j)) {
          const uint32_t slot = atomicAdd(&s_cnt[j], 1u);
          s_buf[j * CAP + slot] = key;
        }
      };
      // two queries a turn, their words in two sets of scalar registers: each set is requested a fold ahead of its use
      // and no set is copied
      bq_u32x4 qa[C], qb[C];
#pragma unroll
      for (int c = 0; c < C; ++c) qb[c] = qa[c] = cload(qc + c);
      for (uint32_t j = 0; j < nq; j += 2) {
        const bool two = j + 1u < nq;
        if (two) {
#pragma unroll
          for (int c = 0; c < C; ++c) qb[c] = cload(qc + (size_t)(j + 1u) * C + c);
        }
        score(j, qa);
        if (j + 2u < nq) {
#pragma unroll
          for (int c = 0; c < C; ++c) qa[c] = cload(qc + (size_t)(j + 2u) * C + c);
        }
        if (two) score(j + 1u, qb);
      }
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t j = 0; j < kBqTile / 4; ++j) {
      const uint32_t qi = w * (kBqTile / 4) + j;
      const uint32_t cnt = rfl(s_cnt[qi]);
      if (cnt > CAP - kBqRoundRows) {  // wave-uniform; cnt > 64 KR >= k
        const uint32_t kth = bq_cut<KR>(s_buf + qi * CAP, cnt, a.k, lane);
        if (lane == 0) {
          s_cnt[qi] = a.k;
          s_bound[qi] = kth;
        }
      }
    }
    __syncthreads();
  }

  // the slice's partial lists, its k best in no particular order, widened to the merge's keys: bits((float)ham) and
  // the index row
#pragma unroll 1
  for (uint32_t j = 0; j < kBqTile / 4; ++j) {
    const uint32_t qi = w * (kBqTile / 4) + j;
    if (qi >= nq) break;
    uint32_t cnt = rfl(s_cnt[qi]);  // <= 64 KR + 64
    if (cnt > a.k) {
      bq_cut<KR>(s_buf + qi * CAP, cnt, a.k, lane);
      cnt = a.k;
    }
    uint64_t* out = a.part + ((size_t)blockIdx.y * a.B + q0 + qi) * a.k;
#pragma unroll
    for (int rr = 0; rr < KR; ++rr) {
      const uint32_t e = rr * 64 + lane;
      if (e < a.k) {
        const uint32_t key = e < cnt ? s_buf[qi * CAP + e] : kInf32;
        out[e] = key == kInf32 ? ~0ull
                               : ((uint64_t)__float_as_uint((float)(key >> kBqRowBits)) << 32) | (b0 * 64u + (key & ((1u << kBqRowBits) - 1u)));
      }
    }
  }
}

// ---- refine ----------------------------------------------------------------------------------------------------------
template <int KR, typename RT>
__global__ __launch_bounds__(256) void bq_refine_kernel(const RefineArgs a) {
  __shared__ __attribute__((aligned(16))) float s_tile[4][kScoreTileFloats];
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x * 4 + w;
  if (q >= a.B) return;
  refine_wave<KR, RT>(a, q, s_tile[w], lane);
}

// rows of a merged result to the caller's ids
static __global__ void bq_map_ids_kernel(const uint32_t* __restrict__ nodes, const uint64_t* __restrict__ ids, uint64_t total,
                                         uint64_t* __restrict__ out_ids) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const uint32_t r = nodes[e];
  out_ids[e] = r == 0xFFFFFFFFu ? ~0ull : ids[r];
}

// [B][d] -> [B][dpad], zero beyond d
static __global__ void bq_pad_queries_kernel(const float* __restrict__ src, uint32_t d, uint32_t dpad, uint64_t B, float* __restrict__ dst) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * dpad) return;
  const uint64_t b = e / dpad;
  const uint32_t i = (uint32_t)(e - b * dpad);
  dst[e] = i < d ? src[b * d + i] : 0.0f;
}

static __global__ void bq_set_flags_kernel(const uint32_t* __restrict__ rows, uint64_t n, uint32_t flag, uint32_t* __restrict__ dead) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) dead[rows[e]] = flag;
}

}  // namespace fvdb
