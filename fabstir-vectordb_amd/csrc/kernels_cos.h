// kernels_cos.h — cosine k-NN search on the device: the reference's batch_search_parallel
// (src/core/vector_ops.rs:310-346: batch_cosine_similarity, then a top-k) and batch_normalize (:138-150), with the
// similarity of Embedding::cosine_similarity (src/core/types.rs:79-103) as include/fvdb.h defines it beside them.
//
//   cos_prepare_kernel   one wave per row: the magnitude by the reference's fold, the unit row (batch_normalize's
//                        output), the padded f32 copy and the fp16 operand words of the matrix instruction
//   cos_scan_kernel      the hot path: a workgroup holds 32 unit queries in LDS as fp16 operands and streams 32-row
//                        operand blocks through v_mfma_f32_32x32x16_f16; the accumulators ARE the approximate cosines;
//                        a running per-query threshold keeps the rows that can reach the answer, which go to a
//                        per-query survivor arena in HBM
//   cos_exact_kernel     the reference's f32 arithmetic on the survivors (or on every live row: the overflow path and
//                        mode "exact"): rows gathered by index through a wave-private LDS tile, lane = row, the query
//                        on the scalar path, the k best by (similarity descending, row ascending)
//   cos_merge_kernel     one wave per query: the exact waves' lists merged, ids, similarities and counts written
//
// Operand form.  Unit rows rounded to fp16 in blocks of 32 rows: word (block, kstep, lane) is the 8 halves of row
// 32 block + (lane & 31), dims 16 kstep + 8 (lane >> 5) .. + 7.  One lane's operand is one 16-byte load and a wave's
// load is 1 KiB contiguous.  Dims beyond d and zero-magnitude rows are zeros.  The queries of a search take the same
// form, 32 a tile.
//
// Why the filter is exact.  |accumulator - reference similarity| <= kCosE for every (query, row) whose magnitudes lie in
// the window (DESIGN 9y derives the constant term by term).  tau = the k-th largest accumulator among the live rows a
// workgroup has seen; a row with accumulator < tau - 2 kCosE has a reference value < tau - kCosE, and k other live rows
// have reference values >= tau - kCosE: it can neither enter nor tie.
#pragma once
#include "common.h"
#include "kernels_scan.h"
#include "score_rows.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kCosMaxDims = 2048;
constexpr uint32_t kCosTile = 32;        // queries of a workgroup (the instruction's M) and rows of a block (its N)
constexpr uint32_t kCosRoundRows = 128;  // rows a workgroup scores between two looks at its round buffers
constexpr int kCosAhead = 4;             // 1 KiB operand words a scan wave keeps in flight
constexpr float kCosE = 0.001953125f;    // 2^-9: DESIGN 9y's bound (its sum is 2^-9.29) rounded up to a power of two
constexpr float kCosMargin = 2.0f * kCosE;
constexpr float kCosMagMin = 9.094947017729282e-13f;  // 2^-40
constexpr float kCosMagMax = 1099511627776.0f;        // 2^40
constexpr uint32_t kCosChunk = 32;                 // dims of one staged chunk of the exact stage
constexpr uint32_t kCosStride = kCosChunk + 4;     // floats per staged row (kernels_flat.h's bank argument)
constexpr uint32_t kCosTileFloats = 64 * kCosStride;

typedef _Float16 cos_h8 __attribute__((ext_vector_type(8)));
typedef float cos_f32x16 __attribute__((ext_vector_type(16)));

// descending monotone map of a similarity's bits: a larger similarity has a smaller key; no finite value maps to kInf32
__device__ __forceinline__ uint32_t cos_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
__device__ __forceinline__ float cos_unkey(uint32_t key) {
  const uint32_t a = ~key;
  return __uint_as_float((a & 0x80000000u) ? (a & 0x7FFFFFFFu) : ~a);
}

// dynamic LDS of a scan workgroup: round buffers, the k best values of each query, counts and thresholds, and (when
// they are staged) the query operands
__host__ __device__ inline uint32_t cos_scan_lds(uint32_t kr, uint32_t ksteps, bool qlds) {
  return kCosTile * kCosRoundRows * 8u + kCosTile * kr * 64u * 4u + 2u * kCosTile * 4u + (qlds ? ksteps * 1024u : 0u);
}

// ---- prepare (vector_ops.rs:138-150 and the index forms) -------------------------------------------------------------
struct CosPrepArgs {
  const float* rows;  // [n][d], row-major, unpadded
  uint32_t d, ksteps, cpad;
  uint64_t n, n_pad;  // source rows; rows n .. n_pad get zero operand words (the tail of a query tile)
  uint64_t first;     // index row of source row 0
  float* unit;        // [n][d]: x / norm, a zero-norm row unchanged; or null
  float* copy;        // [first + r][cpad]: the row as given, zero beyond d; or null
  float* mag;         // [first + r]; or null
  uint4* ops;         // the operand form above; or null
};

// norm = sqrt of the left-to-right f32 fold of the squares (every lane folds the whole row: the order is the
// reference's and the value is wave-uniform); the lanes then share the dims.  f32 division, then one rounding to fp16.
__global__ __launch_bounds__(256) void cos_prepare_kernel(const CosPrepArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.n_pad) return;  // whole waves leave; no barrier below
  const uint64_t idx = a.first + r;
  const uint32_t words = 2u * a.ksteps;
  if (r >= a.n) {
    for (uint32_t c = lane; c < words; c += 64)
      a.ops[((size_t)(idx >> 5) * a.ksteps + (c >> 1)) * 64 + (c & 1u) * 32u + (uint32_t)(idx & 31u)] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const float* row = a.rows + (size_t)r * a.d;
  float s = 0.0f;
#pragma unroll 8
  for (uint32_t i = 0; i < a.d; ++i) {
    const float v = row[i];
    s = s + v * v;
  }
  const float norm = sqrtf(s);
  if (a.mag && lane == 0) a.mag[idx] = norm;
  if (a.copy)
    for (uint32_t i = lane; i < a.cpad; i += 64) a.copy[(size_t)idx * a.cpad + i] = i < a.d ? row[i] : 0.0f;
  if (a.unit)
    for (uint32_t i = lane; i < a.d; i += 64) a.unit[(size_t)r * a.d + i] = norm == 0.0f ? row[i] : row[i] / norm;
  if (a.ops)
    for (uint32_t c = lane; c < words; c += 64) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t i = 8u * c + j;
        if (i < a.d && norm != 0.0f) {
          const _Float16 h = (_Float16)(row[i] / norm);
          w[j >> 1] |= (uint32_t)__builtin_bit_cast(unsigned short, h) << (16u * (j & 1u));
        }
      }
      a.ops[((size_t)(idx >> 5) * a.ksteps + (c >> 1)) * 64 + (c & 1u) * 32u + (uint32_t)(idx & 31u)] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ---- the filter scan -------------------------------------------------------------------------------------------------
struct CosScanArgs {
  const uint4* ops;      // [blocks][ksteps][64] row operand words
  const uint32_t* dead;  // [rows]: non-zero = not a candidate (deleted, or outside an allow-set)
  const uint4* qops;     // [tiles][ksteps][64] query operand words
  uint32_t* arena;       // [B][cap] survivor rows, in no particular order
  uint32_t* arena_cnt;   // [B] slots reserved (may pass cap: the query has then overflowed)
  uint32_t* overflow;    // [B] non-zero = the arena filled up
  uint32_t n, ksteps, B, k, cap, slice_blocks;
};

// Workgroup = 4 waves, one tile of 32 queries (grid x) and one contiguous slice of row blocks (grid y), a quarter of it
// per wave.  The A operand is the query tile (M = query), the B operand a row block (N = row), so a lane's 16
// accumulators are 16 queries against ONE row.  C/D layout of a 32x32 tile: N = lane & 31,
// M = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
//
// A round is one block per wave.  A live pair whose accumulator is not below its query's threshold (tau - 2E as of the
// last round; -inf until k live rows were seen) goes to that query's round buffer as (key, row); an LDS counter hands
// out the slot.  Between two barriers each wave then serves 8 of the 32 queries: the round's keys are offered to the
// query's sorted list of its k best values (LDS, loaded into a WaveTopK and stored back), which raises tau; the
// entries not below the NEW threshold are appended to the query's arena in HBM, their space reserved by one atomic add.
// A reservation that passes the arena's end marks the query as overflowed instead.  A buffer holds 128 entries and a
// round adds at most 128.  Every wave runs every round, with or without a block: the barriers are workgroup-wide.
template <int KR, bool QLDS>
__global__ __launch_bounds__(256) void cos_scan_kernel(const CosScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  uint64_t* s_buf = (uint64_t*)s_raw;                              // [32][128]
  uint32_t* s_top = (uint32_t*)(s_buf + kCosTile * kCosRoundRows);  // [32][64 KR] ascending keys, kInf32 = none
  uint32_t* s_cnt = s_top + kCosTile * KR * 64;
  float* s_thr = (float*)(s_cnt + kCosTile);
  const uint4* s_q = (const uint4*)(s_thr + kCosTile);  // [ksteps][64], QLDS only
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t q0 = blockIdx.x * kCosTile;
  const uint32_t nq = min(kCosTile, a.B - q0);
  const uint4* qg = a.qops + (size_t)blockIdx.x * a.ksteps * 64;

  for (uint32_t e = threadIdx.x; e < kCosTile * KR * 64; e += 256) s_top[e] = kInf32;
  if (threadIdx.x < kCosTile) {
    s_cnt[threadIdx.x] = 0u;
    s_thr[threadIdx.x] = __uint_as_float(0xFF800000u);
  }
  if (QLDS)
    for (uint32_t e = threadIdx.x; e < a.ksteps * 64u; e += 256) ((uint4*)s_q)[e] = qg[e];
  __syncthreads();

  const uint32_t blocks = (a.n + 31u) >> 5;
  const uint32_t b0 = blockIdx.y * a.slice_blocks, b1 = min(blocks, b0 + a.slice_blocks);
  const uint32_t nb = b1 - b0, rounds = (nb + 3u) >> 2;  // workgroup-uniform
  const uint32_t wb0 = b0 + min(nb, w * rounds);         // the wave's quarter
  const uint32_t nbw = b0 + min(nb, (w + 1u) * rounds) - wb0;
  const uint32_t ksteps = a.ksteps;
  const uint4* p = a.ops + (size_t)wb0 * ksteps * 64 + (uint32_t)lane;
  const uint32_t h = (uint32_t)lane >> 5;

  uint4 buf[kCosAhead];
#pragma unroll
  for (int u = 0; u < kCosAhead; ++u) buf[u] = nbw && (uint32_t)u < ksteps ? p[(size_t)u * 64] : make_uint4(0u, 0u, 0u, 0u);

  for (uint32_t r = 0; r < rounds; ++r) {
    if (r < nbw) {  // wave-uniform
      cos_f32x16 acc = {0};
      const uint4* pb = p + (size_t)r * ksteps * 64;
      const bool has_next = r + 1u < nbw;
      // ring slot u holds a word with kstep = u mod kCosAhead; the block's last group refills it from the next block
      for (uint32_t ks0 = 0; ks0 < ksteps; ks0 += kCosAhead) {
        const bool last = ks0 + kCosAhead >= ksteps;
#pragma unroll
        for (int u = 0; u < kCosAhead; ++u) {
          const uint32_t ks = ks0 + (uint32_t)u;
          const uint4 cw = buf[u];
          if (!last) {
            if (ks + kCosAhead < ksteps) buf[u] = pb[(size_t)(ks + kCosAhead) * 64];
          } else if (has_next && (uint32_t)u < ksteps) {
            buf[u] = pb[(size_t)(ksteps + (uint32_t)u) * 64];
          }
          if (ks < ksteps) {
            const uint4 qw = QLDS ? s_q[ks * 64u + (uint32_t)lane] : qg[ks * 64u + (uint32_t)lane];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cos_h8, qw), __builtin_bit_cast(cos_h8, cw), acc, 0, 0, 0);
          }
        }
      }

      const uint32_t row = (wb0 + r) * 32u + ((uint32_t)lane & 31u);
      if (row < a.n && a.dead[row] == 0u) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const uint32_t qi = (uint32_t)(reg & 3) + 8u * (uint32_t)(reg >> 2) + 4u * h;
          if (qi < nq && acc[reg] >= s_thr[qi]) {
            const uint32_t slot = atomicAdd(&s_cnt[qi], 1u);
            s_buf[qi * kCosRoundRows + slot] = ((uint64_t)cos_key(acc[reg]) << 32) | row;
          }
        }
      }
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t j = 0; j < 8; ++j) {
      const uint32_t qi = w * 8u + j;
      const uint32_t cnt = rfl(s_cnt[qi]);
      if (cnt == 0u) continue;  // wave-uniform
      const uint64_t* qb = s_buf + qi * kCosRoundRows;
      uint32_t* top = s_top + qi * KR * 64;
      WaveTopK<KR> tk;
#pragma unroll
      for (int rr = 0; rr < KR; ++rr) {
        tk.hi[rr] = top[rr * 64 + lane];
        tk.lo[rr] = tk.hi[rr] == kInf32 ? kInf32 : 0u;
      }
      uint32_t th, tl;
      tk.kth(a.k, th, tl);
      uint64_t e0 = 0, e1 = 0;  // this lane's entries of the round
      if ((uint32_t)lane < cnt) e0 = qb[lane];
      if ((uint32_t)lane + 64u < cnt) e1 = qb[lane + 64];
      offer<KR>(tk, a.k, (uint32_t)lane < cnt ? (uint32_t)(e0 >> 32) : kInf32, 0u, th, tl, lane);
      if (cnt > 64u) offer<KR>(tk, a.k, (uint32_t)lane + 64u < cnt ? (uint32_t)(e1 >> 32) : kInf32, 0u, th, tl, lane);
#pragma unroll
      for (int rr = 0; rr < KR; ++rr) top[rr * 64 + lane] = tk.hi[rr];
      const float thr = th == kInf32 ? __uint_as_float(0xFF800000u) : cos_unkey(th) - kCosMargin;
      const bool keep0 = (uint32_t)lane < cnt && cos_unkey((uint32_t)(e0 >> 32)) >= thr;
      const bool keep1 = (uint32_t)lane + 64u < cnt && cos_unkey((uint32_t)(e1 >> 32)) >= thr;
      const uint64_t m0 = __ballot(keep0), m1 = __ballot(keep1);
      const uint32_t c0 = (uint32_t)__popcll(m0), total = c0 + (uint32_t)__popcll(m1);
      if (total) {
        const uint32_t q = q0 + qi;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&a.arena_cnt[q], total);
        base = rfl(base);
        if (base + total <= a.cap) {
          uint32_t* dst = a.arena + (size_t)q * a.cap + base;
          if (keep0) dst[ballot_rank(m0, (uint32_t)lane)] = (uint32_t)e0;
          if (keep1) dst[c0 + ballot_rank(m1, (uint32_t)lane)] = (uint32_t)e1;
        } else if (lane == 0) {
          a.overflow[q] = 1u;
        }
      }
      if (lane == 0) {
        s_cnt[qi] = 0u;
        s_thr[qi] = thr;
      }
    }
    __syncthreads();
  }
}

// ---- the exact stage -------------------------------------------------------------------------------------------------
struct CosExactArgs {
  const float* rows;     // [n][dpad] f32 rows as given, zero beyond d (dpad % 4 == 0)
  const float* mag;      // [n]
  const uint32_t* dead;  // [n]
  const float* queries;  // [B][dq] as given, zero beyond d (dq % 32 == 0)
  const float* qmag;     // [B]
  const uint32_t* arena;      // [B][cap]
  const uint32_t* arena_cnt;  // [B]
  const uint32_t* overflow;   // [B]
  uint64_t* part;             // [W][B][k] keys (cos_key << 32 | row), ~0 = none
  unsigned long long* pairs;  // the (query, row) pairs scored
  uint32_t* fallbacks;        // the queries that overflowed
  uint32_t n, dpad, dq, B, k, cap, W;
  uint32_t all;  // pass 1 only: every query (mode "exact"), not only the overflowed
};

// Wave wv of W serves query q (grid x = cdiv(W, 4), y = query): chunks wv, wv + W, ... of 64 list entries.  PASS 0: the
// list is the query's arena, and an overflowed query is left to pass 1.  PASS 1: the list is the identity over all n
// rows, dead ones skipped, for the overflowed queries (or all).  Each query is written by exactly one pass.
//
// A chunk's rows are gathered 32 dims at a time: 8 lanes read the 128 contiguous bytes of one row, 8 rows per load
// instruction, into the wave's LDS tile, and each lane reads its own row back (lane = row).  dot = dot + q_i * x_i in
// dimension order, f32, multiply and add separate, the query through the scalar path; then dot / (mag_q * mag_r), or
// 0.0 when either magnitude is 0 — dot_cosine_kernel's arithmetic.
template <int KR, int PASS>
__global__ __launch_bounds__(256) void cos_exact_kernel(const CosExactArgs a) {
  __shared__ __attribute__((aligned(16))) float s_tile[4][kCosTileFloats];
  const int lane = threadIdx.x & 63;
  const uint32_t wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t q = blockIdx.y;
  if (wv >= a.W) return;  // whole waves leave; no workgroup barrier below
  const bool over = a.overflow[q] != 0u;
  if (PASS == 0 ? over : !(over || a.all)) return;
  const uint32_t cnt = PASS == 0 ? min(a.arena_cnt[q], a.cap) : a.n;
  const uint32_t* list = a.arena + (size_t)q * a.cap;
  float* tile = s_tile[threadIdx.x >> 6];
  const float* qrow = a.queries + (size_t)q * a.dq;
  const float mq = a.qmag[q];
  const uint32_t lr = (uint32_t)lane >> 3, lc = 4u * ((uint32_t)lane & 7u);  // the load role: row within 8, dims within the chunk
  const uint32_t nchunks = a.dq / kCosChunk;

  WaveTopK<KR> tk;
  tk.init();
  uint32_t th = kInf32, tl = kInf32, scored = 0;
  for (uint32_t base = wv * 64u; base < cnt; base += a.W * 64u) {
    const uint32_t e = base + (uint32_t)lane;
    uint32_t row = 0;  // lanes past the list gather row 0: a valid address, never offered
    bool live = false;
    if (e < cnt) {
      row = PASS == 0 ? list[e] : e;
      live = PASS == 0 ? true : a.dead[row] == 0u;
    }
    float dot = 0.0f;
    for (uint32_t c = 0; c < nchunks; ++c) {
      const uint32_t jd = c * kCosChunk + lc;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint32_t src = __shfl(row, i * 8 + (int)lr);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (jd < a.dpad) v = *(const float4*)(a.rows + (size_t)src * a.dpad + jd);  // dpad % 4 == 0: a quad never straddles the end
        *(float4*)(tile + ((uint32_t)i * 8u + lr) * kCosStride + lc) = v;
      }
      score_tile_publish();
      float xr[kCosChunk];
      {
        const float4* pt = (const float4*)(tile + (uint32_t)lane * kCosStride);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float4 v = pt[i];
          xr[4 * i + 0] = v.x;
          xr[4 * i + 1] = v.y;
          xr[4 * i + 2] = v.z;
          xr[4 * i + 3] = v.w;
        }
      }
      score_tile_retire();  // every lane holds its row's chunk: the tile may be rewritten
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const f32x16 qv = cload16(qrow + c * kCosChunk + 16u * (uint32_t)hh);
#pragma unroll
        for (int i = 0; i < 16; ++i) dot = dot + qv[i] * xr[16 * hh + i];
      }
    }
    const float mr = a.mag[row];
    const float sim = (mq == 0.0f || mr == 0.0f) ? 0.0f : dot / (mq * mr);
    scored += (uint32_t)__popcll(__ballot(live));
    offer<KR>(tk, a.k, live ? cos_key(sim) : kInf32, row, th, tl, lane);
  }
  uint64_t* out = a.part + ((size_t)wv * a.B + q) * a.k;
#pragma unroll
  for (int rr = 0; rr < KR; ++rr) {
    const uint32_t e = rr * 64 + lane;
    if (e < a.k) out[e] = ((uint64_t)tk.hi[rr] << 32) | tk.lo[rr];  // (kInf32, kInf32) = ~0 where the list is short
  }
  if (lane == 0) {
    if (scored) atomicAdd(a.pairs, (unsigned long long)scored);
    if (PASS == 1 && wv == 0 && over) atomicAdd(a.fallbacks, 1u);
  }
}

// one wave per query: the W lists merged by key; ids, similarities and counts written (tail = FVDB_NO_ID / -inf).
// W == 0 writes empty rows.
template <int KR>
__global__ __launch_bounds__(256) void cos_merge_kernel(const uint64_t* __restrict__ part, uint32_t W, uint32_t B, uint32_t k,
                                                        const uint64_t* __restrict__ ids, uint64_t* __restrict__ out_ids,
                                                        float* __restrict__ out_sim, uint32_t* __restrict__ out_counts) {
  const int lane = threadIdx.x & 63;
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= B) return;
  WaveTopK<KR> tk;
  tk.init();
  uint32_t th = kInf32, tl = kInf32;
  for (uint32_t s = 0; s < W; ++s)
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
      out_ids[(size_t)q * k + e] = have ? ids[tk.lo[rr]] : ~0ull;
      out_sim[(size_t)q * k + e] = have ? cos_unkey(tk.hi[rr]) : __uint_as_float(0xFF800000u);
    }
  }
  if (lane == 0) out_counts[q] = count;
}

// the per-search counters of a slot: arena_cnt[B], overflow[B], then pairs (8 bytes) and fallbacks
__global__ void cos_clear_kernel(uint32_t* __restrict__ words, uint64_t n) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) words[e] = 0u;
}

__global__ void cos_set_flags_kernel(const uint32_t* __restrict__ rows, uint64_t n, uint32_t flag, uint32_t* __restrict__ dead) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) dead[rows[e]] = flag;
}

}  // namespace fvdb
