// kernels_sq8.h — scalar quantization to u8 on the device: the reference's scalar_quantize_u8 /
// ScalarQuantizedVector::dequantize (src/core/vector_ops.rs:348-387) and the search over its codes that include/fvdb.h
// defines beside them.
//
//   sq8_encode_kernel        one wave per row: min / max by wave reduction, the codes, their sum and sum of squares
//   sq8_decode_kernel        flat codes and (lo, hi) to f32 rows
//   sq8_scan_kernel          the hot path: a workgroup holds 32 encoded queries in LDS and streams 32-row code blocks
//                            through v_mfma_i32_32x32x32_i8; the score and the selection run on the accumulators
//   sq8_decode_cand_kernel   the candidates of a refined search, decoded from the index form into scratch rows
//   sq8_refine_kernel        kernels_refine.h's wave over those rows, or over the stored originals
//
// Index form.  Codes are stored biased by -128 as signed bytes (the matrix instruction's operand type), in blocks of
// 32 rows x 32 dims of 1 KiB: word (block, kstep, lane) is the 16 bytes of row 32 block + (lane & 31), dims
// 32 kstep + 16 (lane >> 5) .. + 15.  One lane's operand is one 16-byte load and a wave's load is 1 KiB contiguous.
// Dims beyond d hold the byte 0, which adds nothing to a signed product.  A 16-byte record per row carries lo, range,
// C1 = sum of codes and C2 = sum of squared codes.  The queries of a search are encoded into the same form, 32 a tile.
// With a' = a - 128 and c' = c - 128 over the d real dims, sum(a' c') = P - 128 (A1 + C1) + 16384 d, all in integers.
#pragma once
#include "common.h"
#include "kernels_flat.h"
#include "kernels_refine.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kSq8MaxDims = 2048;
constexpr uint32_t kSq8Tile = 32;        // queries of a workgroup (the instruction's M) and rows of a block (its N)
constexpr uint32_t kSq8RoundRows = 128;  // rows a workgroup scores between two looks at its survivor buffers
constexpr int kSq8Ahead = 4;             // 1 KiB code words a scan wave keeps in flight
constexpr uint32_t kSq8ScalarBytes = 32 * 4 * 8 + 3 * 32 * 4;  // per-query doubles, counts, bounds, A1

typedef int sq8_i32x4 __attribute__((ext_vector_type(4)));
typedef int sq8_i32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ inline uint32_t sq8_buf_cap(uint32_t kr) { return kr * 64u + kSq8RoundRows; }
// dynamic LDS of a scan workgroup: the survivor buffers, the scalars and (when they are staged) the query operands
__host__ __device__ inline uint32_t sq8_scan_lds(uint32_t kr, uint32_t ksteps, bool qlds) {
  return kSq8Tile * sq8_buf_cap(kr) * 8u + kSq8ScalarBytes + (qlds ? ksteps * 1024u : 0u);
}

// ---- encode (vector_ops.rs:369-387) ----------------------------------------------------------------------------------
struct Sq8EncodeArgs {
  const float* rows;  // [n][d], row-major, unpadded
  uint32_t d, ksteps;
  uint64_t n;
  uint64_t first;     // index row of source row 0 (index form)
  uint8_t* flat;      // [n][d] unsigned codes, with flat_lo[n] and flat_hi[n]; or null
  float* flat_lo;
  float* flat_hi;
  uint4* blocks;      // the index form above, with info[row] = (lo, range, C1, C2); or null
  uint4* info;
  const uint32_t* dest;  // [n] index row of every source row (kernels_ivfsq8.h: a row goes to its list's block); null: first + r
  uint32_t per_row;      // non-zero: blocks is [row][2 ksteps] words, a row's words together (the probed scan's query form)
};

// A lane takes dims 16 c .. 16 c + 15 of chunk c = lane, lane + 64: its codes are one 16-byte word of the index form.
// All in f32, no FMA: code = round_half_away((v - lo) / range * 255), the division first; range == 0: every code 0.
// Of equal extremes the earliest dim is kept (it decides the sign of a zero lo).
static __global__ __launch_bounds__(256) void sq8_encode_kernel(const Sq8EncodeArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.n) return;  // whole waves leave; no barrier below
  const float* row = a.rows + (size_t)r * a.d;
  const uint32_t chunks = (a.d + 15u) >> 4;
  float mn = __uint_as_float(0x7F800000u), mx = __uint_as_float(0xFF800000u);
  uint32_t imn = 0xFFFFFFFFu, imx = 0xFFFFFFFFu;
  for (uint32_t c = (uint32_t)lane; c < chunks; c += 64) {
    for (uint32_t j = 0; j < 16; ++j) {
      const uint32_t i = 16u * c + j;
      if (i < a.d) {
        const float v = row[i];
        if (v < mn) {
          mn = v;
          imn = i;
        }
        if (v > mx) {
          mx = v;
          imx = i;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float on = __shfl_xor(mn, o), ox = __shfl_xor(mx, o);
    const uint32_t oin = __shfl_xor(imn, o), oix = __shfl_xor(imx, o);
    if (on < mn || (on == mn && oin < imn)) {
      mn = on;
      imn = oin;
    }
    if (ox > mx || (ox == mx && oix < imx)) {
      mx = ox;
      imx = oix;
    }
  }
  const float range = mx - mn;
  const uint64_t idx = a.dest ? (uint64_t)a.dest[r] : a.first + r;
  uint32_t s1 = 0, s2 = 0;
  const uint32_t words = a.blocks ? 2u * a.ksteps : chunks;  // the index form writes its pad word too
  for (uint32_t c = (uint32_t)lane; c < words; c += 64) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
      const uint32_t i = 16u * c + j;
      if (i < a.d) {
        uint32_t code = 0;
        if (range != 0.0f) {
          float x = (row[i] - mn) / range;
          x = x * 255.0f;
          const float f = floorf(x);
          code = (uint32_t)f + ((x - f) >= 0.5f ? 1u : 0u);
        }
        s1 += code;
        s2 += code * code;
        if (a.flat) a.flat[(size_t)r * a.d + i] = (uint8_t)code;
        w[j >> 2] |= (code ^ 0x80u) << (8u * (j & 3u));  // code - 128 as a two's complement byte
      }
    }
    if (a.blocks)
      a.blocks[a.per_row ? (size_t)idx * words + c : ((size_t)(idx >> 5) * a.ksteps + (c >> 1)) * 64 + (c & 1u) * 32u + (uint32_t)(idx & 31u)] =
          make_uint4(w[0], w[1], w[2], w[3]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  if (lane == 0) {
    if (a.flat) {
      a.flat_lo[r] = mn;
      a.flat_hi[r] = mx;
    }
    if (a.info) a.info[idx] = make_uint4(__float_as_uint(mn), __float_as_uint(range), s1, s2);
  }
}

// ---- decode (vector_ops.rs:357-366) ----------------------------------------------------------------------------------
__device__ __forceinline__ float sq8_value(float lo, float range, uint32_t code) {
  const float t = (float)code / 255.0f;
  return lo + t * range;
}

// one thread per output float
static __global__ void sq8_decode_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ lo, const float* __restrict__ hi, uint32_t d,
                                  uint64_t n, float* __restrict__ out) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * d) return;
  const uint64_t r = e / d;
  const float l = lo[r];
  out[e] = sq8_value(l, hi[r] - l, codes[e]);
}

// candidate slot (b, j) of a refined search -> out[b * fk + j][dpad], zero beyond d; slots beyond the count are skipped
static __global__ void sq8_decode_cand_kernel(const uint4* __restrict__ blocks, const uint4* __restrict__ info, uint32_t ksteps, uint32_t d,
                                       uint32_t dpad, const uint32_t* __restrict__ cand, const uint32_t* __restrict__ cand_cnt, uint32_t B,
                                       uint32_t fk, float* __restrict__ out) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (uint64_t)B * fk * dpad) return;
  const uint64_t slot = e / dpad;
  const uint32_t i = (uint32_t)(e - slot * dpad);
  const uint32_t b = (uint32_t)(slot / fk), j = (uint32_t)(slot - (uint64_t)b * fk);
  if (j >= min(cand_cnt[b], fk)) return;
  float v = 0.0f;
  if (i < d) {
    const uint32_t row = cand[slot];
    const uint8_t* word = (const uint8_t*)(blocks + ((size_t)(row >> 5) * ksteps + (i >> 5)) * 64 + ((i >> 4) & 1u) * 32u + (row & 31u));
    const uint4 inf = info[row];
    v = sq8_value(__uint_as_float(inf.x), __uint_as_float(inf.y), (uint32_t)word[i & 15u] ^ 0x80u);
  }
  out[e] = v;
}

// ---- the symmetric scan ----------------------------------------------------------------------------------------------
struct Sq8ScanArgs {
  const uint4* codes;    // [blocks][ksteps][64] row words
  const uint4* info;     // [rows]: lo, range, C1, C2
  const uint32_t* dead;  // [rows]: non-zero = not a candidate (deleted, or outside an allow-set)
  const uint4* qcodes;   // [tiles][ksteps][64] query words, the same form
  const uint4* qinfo;    // [B]: lo, range, A1, A2
  uint64_t* part;        // [slices][B][k] keys (bits(dist) << 32 | row), ~0 = none
  uint32_t n, d, ksteps, B, k, slices, slice_blocks;
};

// The survivors of one query (cnt keys) to a sorted WaveTopK; th is the k-th key's high word afterwards.  The first
// `sorted` keys (0, or k after an earlier cut) are already the ascending list: they are loaded as they are, and only the
// keys appended since are offered, so a cut costs what it inserts.
template <int KR>
__device__ __forceinline__ void sq8_select(const uint64_t* buf, uint32_t cnt, uint32_t sorted, uint32_t k, int lane, WaveTopK<KR>& tk,
                                           uint32_t& th) {
  tk.init();
  uint32_t tl = kInf32;
  th = kInf32;
  if (sorted) {
#pragma unroll
    for (int rr = 0; rr < KR; ++rr) {
      const uint32_t e = rr * 64 + lane;
      if (e < sorted) {
        const uint64_t key = buf[e];
        tk.hi[rr] = (uint32_t)(key >> 32);
        tk.lo[rr] = (uint32_t)key;
      }
    }
    tk.kth(k, th, tl);
  }
  for (uint32_t base = sorted; base < cnt; base += 64) {
    const uint32_t e = base + (uint32_t)lane;
    uint32_t chi = kInf32, clo = kInf32;
    if (e < cnt) {
      const uint64_t key = buf[e];
      chi = (uint32_t)(key >> 32);
      clo = (uint32_t)key;
    }
    if (base == 0) {  // empty list: the sorted tile IS the list
      wave_sort64(chi, clo, lane);
      tk.hi[0] = chi;
      tk.lo[0] = clo;
      tk.kth(k, th, tl);
    } else {
      offer<KR>(tk, k, chi, clo, th, tl, lane);
    }
  }
}

// The symmetric score of include/fvdb.h, the one text of it for the flat scan below and the probed scan
// (kernels_ivfsq8.h).  A row's record gives its terms once; a query's are qd[0..3] = lo_q, sq A1, (sq sq) A2, 2 sq and A1.
struct Sq8RowTerms {
  double lo, s, s1, s2;  // lo_r, sr, sr C1, (sr sr) C2
  int32_t fix;           // 128 C1 - 16384 d: with 128 A1, what turns the signed product sum into the unsigned one; |.| < 2^26
};
__device__ __forceinline__ Sq8RowTerms sq8_row_terms(const uint4 inf, uint32_t d) {
  Sq8RowTerms t;
  t.lo = (double)__uint_as_float(inf.x);
  t.s = (double)__uint_as_float(inf.y) / 255.0;
  t.s1 = t.s * (double)inf.z;
  t.s2 = (t.s * t.s) * (double)inf.w;
  t.fix = 128 * (int32_t)inf.z - 16384 * (int32_t)d;
  return t;
}
// bits of dist for one accumulator; dd = (double)d
__device__ __forceinline__ uint32_t sq8_score_bits(int32_t acc, int32_t a1, const double* qd, const Sq8RowTerms& t, double dd) {
  const int32_t P = acc + 128 * a1 + t.fix;  // the unsigned product sum, < 2^27
  const double dl = qd[0] - t.lo;
  const double S = (((dd * dl) * dl + (2.0 * dl) * (qd[1] - t.s1)) + (qd[2] + t.s2)) - (qd[3] * t.s) * (double)P;
  return __float_as_uint(sqrtf((float)(S > 0.0 ? S : 0.0)));
}
// a query's scalars from its record (lo, range, A1, A2), by the thread that owns slot t
__device__ __forceinline__ void sq8_query_terms(const uint4 qi, uint32_t t, double* s_qd, int32_t* s_a1) {
  const double sq = (double)__uint_as_float(qi.y) / 255.0;
  s_qd[4 * t + 0] = (double)__uint_as_float(qi.x);
  s_qd[4 * t + 1] = sq * (double)qi.z;
  s_qd[4 * t + 2] = (sq * sq) * (double)qi.w;
  s_qd[4 * t + 3] = 2.0 * sq;
  s_a1[t] = (int32_t)qi.z;
}

// Between a round's two barriers wave w looks at buffers 8 w .. 8 w + 7: one holding more than 64 KR keys is cut to
// its k best (the buffer then starts with that sorted list, and a bound other than "none" says so) and the bound
// becomes the k-th distance.
template <int KR>
__device__ __forceinline__ void sq8_cut_round(uint64_t* s_buf, uint32_t* s_cnt, uint32_t* s_bound, uint32_t w, uint32_t k, int lane) {
  constexpr uint32_t CAP = KR * 64u + kSq8RoundRows;
#pragma unroll 1
  for (uint32_t j = 0; j < 8; ++j) {
    const uint32_t qi = w * 8u + j;
    const uint32_t cnt = rfl(s_cnt[qi]);
    if (cnt > KR * 64u) {  // wave-uniform
      WaveTopK<KR> tk;
      uint32_t th;
      sq8_select<KR>(s_buf + qi * CAP, cnt, rfl(s_bound[qi]) != kInf32 ? k : 0u, k, lane, tk, th);
#pragma unroll
      for (int rr = 0; rr < KR; ++rr) {
        const uint32_t e = rr * 64 + lane;
        if (e < k) s_buf[qi * CAP + e] = ((uint64_t)tk.hi[rr] << 32) | tk.lo[rr];
      }
      if (lane == 0) {
        s_cnt[qi] = k;  // cnt > 64 KR >= k
        s_bound[qi] = th;
      }
    }
  }
}

// Workgroup = 4 waves, one tile of 32 queries (grid x) and one contiguous slice of row blocks (grid y), a quarter of it
// per wave.  The A operand is the query tile (M = query), the B operand a row block (N = row), so a lane's 16
// accumulators are 16 queries against ONE row: the row's record sits in registers, the queries' scalars are LDS
// broadcasts.  C/D layout of a 32x32 tile: N = lane & 31, M = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
//
// A round is one block per wave.  A pair whose distance bits do not exceed its query's bound is appended to that
// query's buffer (an LDS counter hands out the slot; the key sort decides the order later).  Between two barriers each
// wave then looks at 8 of the 32 buffers: one holding more than 64 KR keys is cut to its k best by sq8_select (the
// buffer then starts with that sorted list, and a bound other than "none" says so) and the bound becomes the k-th distance.  A buffer holds 64 KR + 128 keys, a round adds at most 128, so none overflows.
// Every wave runs every round, with or without a block of its own: the barriers are workgroup-wide.
template <int KR, bool QLDS>
__global__ __launch_bounds__(256) void sq8_scan_kernel(const Sq8ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  constexpr uint32_t CAP = KR * 64u + kSq8RoundRows;
  uint64_t* s_buf = (uint64_t*)s_raw;                // [32][CAP]
  double* s_qd = (double*)(s_buf + kSq8Tile * CAP);  // [32][4]: lo_q, sq A1, (sq sq) A2, 2 sq
  uint32_t* s_cnt = (uint32_t*)(s_qd + kSq8Tile * 4);
  uint32_t* s_bound = s_cnt + kSq8Tile;
  int32_t* s_a1 = (int32_t*)(s_bound + kSq8Tile);
  const uint4* s_q = (const uint4*)(s_a1 + kSq8Tile);  // [ksteps][64], QLDS only
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t q0 = blockIdx.x * kSq8Tile;
  const uint32_t nq = min(kSq8Tile, a.B - q0);
  const uint4* qg = a.qcodes + (size_t)blockIdx.x * a.ksteps * 64;

  if (threadIdx.x < kSq8Tile) {
    const uint32_t t = threadIdx.x;
    uint4 qi = make_uint4(0u, 0u, 0u, 0u);
    if (t < nq) qi = a.qinfo[q0 + t];
    sq8_query_terms(qi, t, s_qd, s_a1);
    s_cnt[t] = 0u;
    s_bound[t] = kInf32;
  }
  if (QLDS)
    for (uint32_t e = threadIdx.x; e < a.ksteps * 64u; e += 256) ((uint4*)s_q)[e] = qg[e];
  __syncthreads();

  const uint32_t blocks = (a.n + 31u) >> 5;
  const uint32_t b0 = blockIdx.y * a.slice_blocks, b1 = min(blocks, b0 + a.slice_blocks);
  const uint32_t nb = b1 - b0, rounds = (nb + 3u) >> 2;        // workgroup-uniform
  const uint32_t wb0 = b0 + min(nb, w * rounds);               // the wave's quarter
  const uint32_t nbw = b0 + min(nb, (w + 1u) * rounds) - wb0;
  const uint32_t ksteps = a.ksteps;
  const uint4* p = a.codes + (size_t)wb0 * ksteps * 64 + (uint32_t)lane;
  const uint32_t h = (uint32_t)lane >> 5;
  const double dd = (double)a.d;

  uint4 buf[kSq8Ahead];
#pragma unroll
  for (int u = 0; u < kSq8Ahead; ++u) buf[u] = nbw && (uint32_t)u < ksteps ? p[(size_t)u * 64] : make_uint4(0u, 0u, 0u, 0u);

  for (uint32_t r = 0; r < rounds; ++r) {
    if (r < nbw) {  // wave-uniform
      sq8_i32x16 acc = {0};
      const uint4* pb = p + (size_t)r * ksteps * 64;
      const bool has_next = r + 1u < nbw;
      // ring slot u holds a word with kstep = u mod kSq8Ahead; the block's last group refills it from the next block
      for (uint32_t ks0 = 0; ks0 < ksteps; ks0 += kSq8Ahead) {
        const bool last = ks0 + kSq8Ahead >= ksteps;
#pragma unroll
        for (int u = 0; u < kSq8Ahead; ++u) {
          const uint32_t ks = ks0 + (uint32_t)u;
          const uint4 cw = buf[u];
          if (!last) {
            if (ks + kSq8Ahead < ksteps) buf[u] = pb[(size_t)(ks + kSq8Ahead) * 64];
          } else if (has_next && (uint32_t)u < ksteps) {
            buf[u] = pb[(size_t)(ksteps + (uint32_t)u) * 64];
          }
          if (ks < ksteps) {
            const uint4 qw = QLDS ? s_q[ks * 64u + (uint32_t)lane] : qg[ks * 64u + (uint32_t)lane];
            const sq8_i32x4 av = {(int)qw.x, (int)qw.y, (int)qw.z, (int)qw.w};
            const sq8_i32x4 bv = {(int)cw.x, (int)cw.y, (int)cw.z, (int)cw.w};
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc, 0, 0, 0);
          }
        }
      }

      const uint32_t row = (wb0 + r) * 32u + ((uint32_t)lane & 31u);
      if (row < a.n && a.dead[row] == 0u) {
        const Sq8RowTerms rt = sq8_row_terms(a.info[row], a.d);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const uint32_t qi = (uint32_t)(reg & 3) + 8u * (uint32_t)(reg >> 2) + 4u * h;
          if (qi < nq) {
            const uint32_t chi = sq8_score_bits(acc[reg], s_a1[qi], s_qd + 4 * qi, rt, dd);
            if (chi <= s_bound[qi]) {
              const uint32_t slot = atomicAdd(&s_cnt[qi], 1u);
              s_buf[qi * CAP + slot] = ((uint64_t)chi << 32) | row;
            }
          }
        }
      }
    }
    __syncthreads();
    sq8_cut_round<KR>(s_buf, s_cnt, s_bound, w, a.k, lane);
    __syncthreads();
  }

#pragma unroll 1
  for (uint32_t j = 0; j < 8; ++j) {
    const uint32_t qi = w * 8u + j;
    if (qi >= nq) break;
    WaveTopK<KR> tk;
    uint32_t th;
    sq8_select<KR>(s_buf + qi * CAP, rfl(s_cnt[qi]), rfl(s_bound[qi]) != kInf32 ? a.k : 0u, a.k, lane, tk, th);
    uint64_t* out = a.part + ((size_t)blockIdx.y * a.B + q0 + qi) * a.k;
#pragma unroll
    for (int rr = 0; rr < KR; ++rr) {
      const uint32_t e = rr * 64 + lane;
      if (e < a.k) out[e] = ((uint64_t)tk.hi[rr] << 32) | tk.lo[rr];  // (kInf32, kInf32) = ~0 where the list is short
    }
  }
}

// ---- refine and small helpers ----------------------------------------------------------------------------------------
template <int KR, typename RT>
__global__ __launch_bounds__(256) void sq8_refine_kernel(const RefineArgs a) {
  __shared__ __attribute__((aligned(16))) float s_tile[4][kScoreTileFloats];
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x * 4 + w;
  if (q >= a.B) return;
  refine_wave<KR, RT>(a, q, s_tile[w], lane);
}

// rows of a merged result to the caller's ids
static __global__ void sq8_map_ids_kernel(const uint32_t* __restrict__ nodes, const uint64_t* __restrict__ ids, uint64_t total,
                                   uint64_t* __restrict__ out_ids) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const uint32_t r = nodes[e];
  out_ids[e] = r == 0xFFFFFFFFu ? ~0ull : ids[r];
}

// [B][d] -> [B][dpad], zero beyond d
static __global__ void sq8_pad_queries_kernel(const float* __restrict__ src, uint32_t d, uint32_t dpad, uint64_t B, float* __restrict__ dst) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * dpad) return;
  const uint64_t b = e / dpad;
  const uint32_t i = (uint32_t)(e - b * dpad);
  dst[e] = i < d ? src[b * d + i] : 0.0f;
}

static __global__ void sq8_set_flags_kernel(const uint32_t* __restrict__ rows, uint64_t n, uint32_t flag, uint32_t* __restrict__ dead) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) dead[rows[e]] = flag;
}

}  // namespace fvdb
