// kernels_flat_mfma.h — the exact scan of a graph's row store with a matrix-core filter in front of it (DESIGN.md
// section 9z): a second route to the answer of flat_scan_kernel (kernels_flat.h) — the same nodes, distance bits and
// counts, ties to the lower node — that scores every (query, row) pair approximately on v_mfma_f32_32x32x16_f16 and
// only the few pairs that can reach the answer with the reference's sequential f32 fold.
//
//   flat_mfma_mirror_kernel   one wave per row, straight from the store: the row rounded to fp16 (exact on an fp16 store)
//                             in the instruction's operand form, |x|^2 in f32 and the running maximum of the norms
//   flat_mfma_query_kernel    one wave per query: the fp16 operand words of a 32-query tile, |q|^2, and the margin
//                             2 E_q + G_q of the filter (mfma_error_bound; +inf = the query is "unbounded")
//   flat_mfma_scan_kernel     the hot path: a workgroup holds 32 queries as the A operand (LDS, or HBM when they do not
//                             fit) and streams 32-row operand words; v = |x|^2 - 2 x~.q~ per pair; a running per-query
//                             k-th value tau keeps v <= tau + margin, which go to a per-query survivor arena in HBM
//   flat_mfma_exact_kernel    flat_fold_slice's arithmetic on the survivors (PASS 0) or on every live row (PASS 1: the
//                             queries whose arena overflowed or whose bound is infinite), rows gathered from the STORE
//   flat_merge_kernel         (kernels_flat.h, unchanged) merges the exact waves' lists and writes the result block
//
// Operand form (section 9y's).  Blocks of 32 rows: word (block, kstep, lane) is the 8 halves of row 32 block + (lane & 31),
// dims 16 kstep + 8 (lane >> 5) .. + 7; a wave's load of one word is 1 KiB contiguous.  Dims beyond d and rows beyond n
// are zeros.  The queries of a search take the same form, 32 a tile.
//
// Why the filter is exact.  S = the reference's f32 sum of a pair, v its filter value: |v + |q|^2 - S| <= E_q
// (mfma_error_bound, kernels_mfma.h).  tau = the k-th smallest v among the live rows a workgroup has seen, so k live
// rows of the slice have S <= tau + |q|^2 + E.  A dropped row has v > tau + 2 E + G, so S > tau + |q|^2 + E + G: it is
// farther in S than each of those k by more than G = 4e-6 (|x|max + |q|)^2 >= 2^-17.9 S.  A relative gap of 2^-19.9 in S
// is one of 2^-20.9 in sqrt(S), two ulps at the least: the rounded roots differ, so the dropped row's key is strictly
// above k keys of its own slice and it can neither enter the answer nor tie.  The rest of G pays for the roundings of
// v = xn - 2 acc and of tau + margin (2^-24 (|x|max + |q|)^2 each).  DESIGN 9z has the arithmetic.
#pragma once
#include "common.h"
#include "kernels_flat.h"
#include "kernels_mfma.h"
#include "kernels_scan.h"
#include "row_types.h"
#include "score_rows.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kFmMaxDims = 2048;
constexpr uint32_t kFmTile = 32;        // queries of a workgroup (the instruction's M) and rows of a block (its N)
constexpr uint32_t kFmRoundRows = 128;  // rows a workgroup scores between two looks at its round buffers
constexpr int kFmAhead = 4;             // 1 KiB operand words a scan wave keeps in flight
constexpr float kFmGap = 4e-6f;         // G_q / (|x|max + |q|)^2: the sqrt step and the filter's own two roundings
constexpr uint32_t kFmUnbounded = 2u, kFmOverflow = 1u;  // bits of a query's flag word

// dynamic LDS of a scan workgroup: round buffers, the k smallest values of each query, counts, thresholds and margins,
// and (when they are staged) the query operands
__host__ __device__ inline uint32_t flat_mfma_scan_lds(uint32_t kr, uint32_t ksteps, bool qlds) {
  return kFmTile * kFmRoundRows * 8u + kFmTile * kr * 64u * 4u + 3u * kFmTile * 4u + (qlds ? ksteps * 1024u : 0u);
}

__device__ __forceinline__ size_t flat_mfma_word(uint64_t row, uint32_t ksteps, uint32_t c) {
  return ((size_t)(row >> 5) * ksteps + (c >> 1)) * 64 + (c & 1u) * 32u + (uint32_t)(row & 31u);
}

// 8 consecutive dims of a stored row from dim 8 c, rounded to nearest even into one operand word; the f32 values the
// reference sees go to s as s + v * v
template <typename RT>
__device__ __forceinline__ uint4 flat_mfma_pack(const RT* row, uint32_t c, uint32_t d, float& s) {
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j) {
    const uint32_t i = 8u * c + j;
    if (i < d) {
      const float v = row_widen(row[i]);
      s = s + v * v;
      const _Float16 h = (_Float16)v;
      w[j >> 1] |= (uint32_t)__builtin_bit_cast(unsigned short, h) << (16u * (j & 1u));
    }
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ float flat_mfma_wave_sum(float s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
  return s;
}

// ---- the mirror ------------------------------------------------------------------------------------------------------
struct FlatMirrorArgs {
  const void* rows;      // the store: [node][dpad] of the kernel's RT
  uint32_t d, dpad, ksteps;
  uint64_t first, n, n_pad;  // rows [first, n) are mirrored, rows [n, n_pad) get zero words (the tail of the last block)
  uint4* ops;            // [blocks][ksteps][64]
  float* xn;             // [n] |x|^2
  uint32_t* xmax_bits;   // the largest |x|^2 so far (a non-negative float's bits order as unsigned)
};

// The lanes of a wave share the row's operand words; each adds the squares of its own dims and the wave adds the 64
// partial sums: any order of an f32 sum of squares is inside mfma_error_bound's norm term.
template <typename RT>
__global__ __launch_bounds__(256) void flat_mfma_mirror_kernel(const FlatMirrorArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t r = a.first + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.n_pad) return;  // whole waves leave; no barrier below
  const uint32_t words = 2u * a.ksteps;
  if (r >= a.n) {
    for (uint32_t c = lane; c < words; c += 64) a.ops[flat_mfma_word(r, a.ksteps, c)] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const RT* row = (const RT*)a.rows + (size_t)r * a.dpad;
  float s = 0.0f;
  for (uint32_t c = lane; c < words; c += 64) a.ops[flat_mfma_word(r, a.ksteps, c)] = flat_mfma_pack(row, c, a.d, s);
  s = flat_mfma_wave_sum(s);
  if (lane == 0) {
    a.xn[r] = s;
    atomicMax(a.xmax_bits, __float_as_uint(s));
  }
}

// ---- the queries of a sub-batch ---------------------------------------------------------------------------------------
struct FlatMfmaQueryArgs {
  const float* queries;  // [B][dpad], zero beyond d
  uint32_t d, dpad, ksteps, B, B_pad;  // B_pad = whole tiles; queries B .. B_pad get zero words
  const uint32_t* xmax_bits;
  int x_rounded;         // mfma_error_bound's: 0 = an fp16 store (the mirror is a copy), 1 = an f32 store
  uint4* qops;           // [tiles][ksteps][64]
  float* margin;         // [B] 2 E_q + G_q, +inf = unbounded
  uint32_t* flags;       // [B] cleared before; kFmUnbounded is set here
  uint32_t* unbounded;   // the search's count of unbounded queries
};

__global__ __launch_bounds__(256) void flat_mfma_query_kernel(const FlatMfmaQueryArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B_pad) return;
  const uint32_t words = 2u * a.ksteps;
  if (b >= a.B) {
    for (uint32_t c = lane; c < words; c += 64) a.qops[flat_mfma_word(b, a.ksteps, c)] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const float* row = a.queries + (size_t)b * a.dpad;
  float s = 0.0f;
  for (uint32_t c = lane; c < words; c += 64) a.qops[flat_mfma_word(b, a.ksteps, c)] = flat_mfma_pack(row, c, a.d, s);
  s = flat_mfma_wave_sum(s);
  if (lane == 0) {
    const float xmax2 = __uint_as_float(*a.xmax_bits);
    const float E = mfma_error_bound(xmax2, s, (float)(16u * a.ksteps), a.x_rounded);
    float m = __builtin_huge_valf();
    if (E < m) {
      const float sum = sqrtf(xmax2) * 1.000001f + sqrtf(s) * 1.000001f;
      m = 2.0f * E + kFmGap * sum * sum;
    }
    a.margin[b] = m;
    if (!(m < __builtin_huge_valf())) {
      a.flags[b] = kFmUnbounded;
      atomicAdd(a.unbounded, 1u);
    }
  }
}

// ---- the filter scan --------------------------------------------------------------------------------------------------
struct FlatMfmaScanArgs {
  const uint4* ops;      // [blocks][ksteps][64] row operand words
  const float* xn;       // [n] |x|^2
  const uint32_t* dead;  // [n]: non-zero = not a candidate (deleted, or outside an allow-set)
  const uint4* qops;     // [tiles][ksteps][64] query operand words
  const float* margin;   // [B]
  uint32_t* arena;       // [B][cap] survivor nodes, in no particular order
  uint32_t* arena_cnt;   // [B] slots reserved (may pass cap: the query has then overflowed)
  uint32_t* flags;       // [B] kFmOverflow is set here
  uint32_t n, ksteps, B, k, cap, slice_blocks;
};

// Workgroup = 4 waves, one tile of 32 queries (grid x) and one contiguous slice of row blocks (grid y), a quarter of it
// per wave.  The A operand is the query tile (M = query), the B operand a row block (N = row), so a lane's 16
// accumulators are 16 queries against ONE row, whose |x|^2 and liveness the lane loads once.  C/D layout of a 32x32
// tile: N = lane & 31, M = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
//
// A round is one block per wave.  A live pair with v <= its query's threshold (tau + margin as of the last round; +inf
// until k live rows were seen; -inf for an unbounded query, which emits nothing) goes to that query's round buffer as
// (key of v, node); an LDS counter hands out the slot.  Between two barriers each wave then serves 8 of the 32 queries:
// the round's keys are offered to the query's sorted list of its k smallest values (LDS, loaded into a WaveTopK and
// stored back), which lowers tau; the entries not above the NEW threshold are appended to the query's arena in HBM,
// their space reserved by one atomic add.  A reservation that passes the arena's end marks the query as overflowed
// instead.  A buffer holds 128 entries and a round adds at most 128.  Every wave runs every round, with or without a
// block: the barriers are workgroup-wide.
template <int KR, bool QLDS>
__global__ __launch_bounds__(256) void flat_mfma_scan_kernel(const FlatMfmaScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  uint64_t* s_buf = (uint64_t*)s_raw;                            // [32][128]
  uint32_t* s_top = (uint32_t*)(s_buf + kFmTile * kFmRoundRows);  // [32][64 KR] ascending keys, kInf32 = none
  uint32_t* s_cnt = s_top + kFmTile * KR * 64;
  float* s_thr = (float*)(s_cnt + kFmTile);
  float* s_mar = s_thr + kFmTile;
  const uint4* s_q = (const uint4*)(s_mar + kFmTile);  // [ksteps][64], QLDS only
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t q0 = blockIdx.x * kFmTile;
  const uint32_t nq = min(kFmTile, a.B - q0);
  const uint4* qg = a.qops + (size_t)blockIdx.x * a.ksteps * 64;
  const float inf = __builtin_huge_valf();

  for (uint32_t e = threadIdx.x; e < kFmTile * KR * 64; e += 256) s_top[e] = kInf32;
  if (threadIdx.x < kFmTile) {
    const float m = threadIdx.x < nq ? a.margin[q0 + threadIdx.x] : inf;
    s_cnt[threadIdx.x] = 0u;
    s_mar[threadIdx.x] = m;
    s_thr[threadIdx.x] = m < inf ? inf : -inf;
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

  uint4 buf[kFmAhead];
#pragma unroll
  for (int u = 0; u < kFmAhead; ++u) buf[u] = nbw && (uint32_t)u < ksteps ? p[(size_t)u * 64] : make_uint4(0u, 0u, 0u, 0u);

  for (uint32_t r = 0; r < rounds; ++r) {
    if (r < nbw) {  // wave-uniform
      const uint32_t row = (wb0 + r) * 32u + ((uint32_t)lane & 31u);
      const bool live = row < a.n && a.dead[row] == 0u;  // issued ahead of the products
      const float xn = row < a.n ? a.xn[row] : 0.0f;
      f32x16m acc = {0};
      const uint4* pb = p + (size_t)r * ksteps * 64;
      const bool has_next = r + 1u < nbw;
      // ring slot u holds a word with kstep = u mod kFmAhead; the block's last group refills it from the next block
      for (uint32_t ks0 = 0; ks0 < ksteps; ks0 += kFmAhead) {
        const bool last = ks0 + kFmAhead >= ksteps;
#pragma unroll
        for (int u = 0; u < kFmAhead; ++u) {
          const uint32_t ks = ks0 + (uint32_t)u;
          const uint4 cw = buf[u];
          if (!last) {
            if (ks + kFmAhead < ksteps) buf[u] = pb[(size_t)(ks + kFmAhead) * 64];
          } else if (has_next && (uint32_t)u < ksteps) {
            buf[u] = pb[(size_t)(ksteps + (uint32_t)u) * 64];
          }
          if (ks < ksteps) {
            const uint4 qw = QLDS ? s_q[ks * 64u + (uint32_t)lane] : qg[ks * 64u + (uint32_t)lane];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8v, qw), __builtin_bit_cast(h8v, cw), acc, 0, 0, 0);
          }
        }
      }
      if (live) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const uint32_t qi = (uint32_t)(reg & 3) + 8u * (uint32_t)(reg >> 2) + 4u * h;
          const float v = xn - 2.0f * acc[reg];
          if (qi < nq && v <= s_thr[qi]) {
            const uint32_t slot = atomicAdd(&s_cnt[qi], 1u);
            s_buf[qi * kFmRoundRows + slot] = ((uint64_t)fmap_u32(v) << 32) | row;
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
      const uint64_t* qb = s_buf + qi * kFmRoundRows;
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
      const float thr = th == kInf32 ? inf : funmap_u32(th) + s_mar[qi];  // a query that emits has a finite margin
      const bool keep0 = (uint32_t)lane < cnt && funmap_u32((uint32_t)(e0 >> 32)) <= thr;
      const bool keep1 = (uint32_t)lane + 64u < cnt && funmap_u32((uint32_t)(e1 >> 32)) <= thr;
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
          a.flags[q] = kFmOverflow;
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

// ---- the exact stage --------------------------------------------------------------------------------------------------
struct FlatMfmaExactArgs {
  const void* rows;           // the store: [node][dpad] of the kernel's RT
  const float* queries;       // [B][dpad], zero beyond d, 16-byte aligned
  const uint32_t* dead;       // [n]
  const uint32_t* arena;      // [B][cap]
  const uint32_t* arena_cnt;  // [B]
  const uint32_t* flags;      // [B]
  uint64_t* part;             // [W][B][k] keys (distance bits << 32 | node), ~0 = none
  unsigned long long* pairs;  // the (query, row) pairs scored
  uint32_t* fallbacks;        // the queries whose arena overflowed
  uint32_t n, dpad, B, k, cap, W;
};

// Wave wv of W serves query q (grid x = cdiv(W, 4), y = query): chunks wv, wv + W, ... of 64 list entries.  PASS 0: the
// list is the query's arena; a query with a flag is left to pass 1.  PASS 1: the list is the identity over all n rows,
// dead ones skipped, for the flagged queries.  Each query is written by exactly one pass.
//
// A chunk's rows are gathered from the store 32 dims at a time as flat_fold_slice loads a tile — 8 lanes read the 128
// (f32) or 64 (fp16) contiguous bytes of one row, 8 rows per load instruction — into the wave's LDS tile, and each lane
// reads its own row back (lane = row).  Then flat_fold_slice's fold for one query: t = q_i - x_i; acc = acc + t * t in
// dimension order, the query through the scalar path, quads below dpad only at the row's end; sqrtf.
template <int KR, int PASS, typename RT>
__global__ __launch_bounds__(256) void flat_mfma_exact_kernel(const FlatMfmaExactArgs a) {
  using Quad = typename RowVec<RT>::Quad;
  __shared__ __attribute__((aligned(16))) float s_tile[4][kFlatTileFloats];
  const int lane = threadIdx.x & 63;
  const uint32_t wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t q = blockIdx.y;
  if (wv >= a.W) return;  // whole waves leave; no workgroup barrier below
  const uint32_t flag = a.flags[q];
  if (PASS == 0 ? flag != 0u : flag == 0u) return;
  const uint32_t cnt = PASS == 0 ? min(a.arena_cnt[q], a.cap) : a.n;
  const uint32_t* list = a.arena + (size_t)q * a.cap;
  float* tile = s_tile[threadIdx.x >> 6];
  const RT* rows = (const RT*)a.rows;
  const float* qrow = a.queries + (size_t)q * a.dpad;
  const uint32_t dpad = a.dpad;
  const uint32_t lr = (uint32_t)lane >> 3, lc = 4u * ((uint32_t)lane & 7u);  // the load role: row within 8, dims within the chunk
  const uint32_t nchunks = (dpad + kFlatChunk - 1) / kFlatChunk;

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
    float acc = 0.0f;
    for (uint32_t c = 0; c < nchunks; ++c) {
      const uint32_t jd = c * kFlatChunk + lc;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint32_t src = __shfl(row, i * 8 + (int)lr);
        Quad v = {};
        if (jd < dpad) v = *(const Quad*)(rows + (size_t)src * dpad + jd);  // dpad % 4 == 0: a quad never straddles the end
        *(float4*)(tile + ((uint32_t)i * 8u + lr) * kFlatStride + lc) = row_widen(v);
      }
      score_tile_publish();
      float xr[kFlatChunk];
      {
        const float4* pt = (const float4*)(tile + (uint32_t)lane * kFlatStride);
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
        const uint32_t dbase = c * kFlatChunk + 16u * (uint32_t)hh;  // wave-uniform
        if (dbase + 16u <= dpad) {
          const f32x16 qv = cload16(qrow + dbase);
          float tt;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            tt = qv[i] - xr[16 * hh + i];
            acc = acc + tt * tt;
          }
        } else {  // the row's last dimensions: quads below dpad only, so no query is read past its end
#pragma unroll
          for (int i4 = 0; i4 < 4; ++i4) {
            if (dbase + 4u * (uint32_t)i4 < dpad) {
              const f32x4 qv = cload((const f32x4*)(qrow + dbase + 4 * i4));
              float tt;
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                tt = qv[i] - xr[16 * hh + 4 * i4 + i];
                acc = acc + tt * tt;
              }
            }
          }
        }
      }
    }
    const float dist = sqrtf(acc);
    scored += (uint32_t)__popcll(__ballot(live));
    offer<KR>(tk, a.k, live ? __float_as_uint(dist) : kInf32, row, th, tl, lane);
  }
  uint64_t* out = a.part + ((size_t)wv * a.B + q) * a.k;
#pragma unroll
  for (int rr = 0; rr < KR; ++rr) {
    const uint32_t e = rr * 64 + lane;
    if (e < a.k) out[e] = ((uint64_t)tk.hi[rr] << 32) | tk.lo[rr];  // (kInf32, kInf32) = ~0 where the list is short
  }
  if (lane == 0) {
    if (scored) atomicAdd(a.pairs, (unsigned long long)scored);
    if (PASS == 1 && wv == 0 && (flag & kFmOverflow)) atomicAdd(a.fallbacks, 1u);
  }
}

// the per-search counters and a sub-batch's arena counts and flags (no memset: a kernel)
__global__ void flat_mfma_clear_kernel(uint32_t* __restrict__ words, uint64_t n) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) words[e] = 0u;
}

}  // namespace fvdb
