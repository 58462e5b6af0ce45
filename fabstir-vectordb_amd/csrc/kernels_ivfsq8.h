// kernels_ivfsq8.h — the probed scan over SQ8 codes held in inverted lists (include/fvdb.h,
// "IVF over SQ8 codes").  The codec, the symmetric score, the survivor buffers and their cut are kernels_sq8.h's, the
// plan that inverts a probe table is kernels_scan.h's; what is here is the kernel between them.
//
//   ivfsq8_scan_kernel         one workgroup per work item (list, segment of its blocks, up to 32 of the queries that
//                              probe it): the queries are gathered into the A tile, the segment's 32-row code blocks
//                              are streamed through v_mfma_i32_32x32x32_i8, each query's k best go to the arena
//   ivfsq8_place_kernel        add: the tables between pool rows and add ordinals (seq), and the live words
//   ivfsq8_decode_cand_kernel  the candidates of a refined search (seq), decoded from their pool rows into scratch rows
//   ivfsq8_fill_kernel         32-bit fill (the arena's ~0, the pool's "dead" words)
//
// Pool.  Code blocks in kernels_sq8.h's index form, each owned by one list; per pool row the 16-byte record, a dead word
// (1 also for the unfilled tail of a list's last block) and seq_of_row.  list_blocks[list_off[L] .. list_off[L + 1]) are
// list L's blocks in fill order.  The key of a candidate is (bits(dist) << 32) | seq, so ties go to the row added first
// whichever lists hold the tied rows.
#pragma once
#include "common.h"
#include "kernels_sq8.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kIvfSq8MaxSegments = 4;   // S: a list is cut into at most this many segments
constexpr uint32_t kIvfSq8MinSegBlocks = 16; // 512 rows: a segment shorter than this does not pay for its partial lists
constexpr uint32_t kIvfSq8MaxProbe = 256;
constexpr uint32_t kIvfSq8MaxLists = 16384;

// dynamic LDS of a scan workgroup: kernels_sq8.h's buffers and scalars, the item's 32 (query, probe rank) entries and,
// when they are staged, the gathered query operands
__host__ __device__ inline uint32_t ivfsq8_scan_lds(uint32_t kr, uint32_t ksteps, bool qlds) {
  return kSq8Tile * sq8_buf_cap(kr) * 8u + kSq8ScalarBytes + kSq8Tile * 8u + (qlds ? ksteps * 1024u : 0u);
}

struct IvfSq8ScanArgs {
  const uint4* codes;            // [pool blocks][ksteps][64] row words
  const uint4* info;             // [pool rows]: lo, range, C1, C2
  const uint32_t* dead;          // [pool rows]: non-zero = not a candidate (unfilled, deleted, or outside an allow-set)
  const uint32_t* seq_of_row;    // [pool rows]
  const uint32_t* list_off;      // [nlist + 1] into list_blocks
  const uint32_t* list_blocks;   // pool block ids, list by list
  const uint4* qwords;           // [B][ksteps][2] query words: dims 32 kstep + 16 half .. + 15, biased like the rows
  const uint4* qinfo;            // [B]: lo, range, A1, A2
  const uint32_t* item_off;      // [nlist + 1]: the plan's prefix sums of work items
  const uint32_t* entry_off;     // [nlist + 1]: of entries
  const uint2* entries;          // (query, probe rank), list by list
  const uint32_t* n_items;       // the plan's item count; workgroups beyond it return
  uint64_t* part;                // [nprobe * segs][B][k] keys, pre-filled with ~0
  uint32_t nlist, d, ksteps, B, k, segb, segs;
};

// Item -> (list, segment, group): the list by a binary search of item_off, then item = group * nseg + segment inside it.
// Four waves take a quarter of the segment's blocks each; the MFMA has M = gathered query and N = row, so a lane's 16
// accumulators are 16 queries against one row whose record and seq sit in registers (C/D layout as in kernels_sq8.h).
// A wave keeps kSq8Ahead code words in flight; the id of its next block is read from list_blocks when the present one
// starts, so the last words of a block are followed by the first of the next without a stall on the table.
// Rounds, buffers, cut and bound are sq8_scan_kernel's.  Query (q, rank) of segment s writes its list to slice
// rank * segs + s of the arena: one writer per (slice, query), slices nobody writes keep their ~0.
template <int KR, bool QLDS>
__global__ __launch_bounds__(256) void ivfsq8_scan_kernel(const IvfSq8ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  constexpr uint32_t CAP = KR * 64u + kSq8RoundRows;
  uint64_t* s_buf = (uint64_t*)s_raw;                // [32][CAP]
  double* s_qd = (double*)(s_buf + kSq8Tile * CAP);  // [32][4]: lo_q, sq A1, (sq sq) A2, 2 sq
  uint32_t* s_cnt = (uint32_t*)(s_qd + kSq8Tile * 4);
  uint32_t* s_bound = s_cnt + kSq8Tile;
  int32_t* s_a1 = (int32_t*)(s_bound + kSq8Tile);
  uint2* s_ent = (uint2*)(s_a1 + kSq8Tile);          // [32]: (query, probe rank) of a slot
  uint4* s_q = (uint4*)(s_ent + kSq8Tile);           // [ksteps][64], QLDS only
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t item = blockIdx.x;
  if (item >= *a.n_items) return;  // the grid is the host's bound on the item count

  uint32_t L = 0, hi = a.nlist;  // the last list with item_off[L] <= item: lists without items share their offset
  while (hi - L > 1) {
    const uint32_t mid = (L + hi) >> 1;
    if (a.item_off[mid] <= item) L = mid;
    else hi = mid;
  }
  const uint32_t lb0 = a.list_off[L], nblk = a.list_off[L + 1] - lb0;
  const uint32_t nseg = (nblk + a.segb - 1) / a.segb;
  const uint32_t local = item - a.item_off[L];
  const uint32_t seg = local % nseg, grp = local / nseg;
  const uint32_t e0 = a.entry_off[L] + grp * kSq8Tile;
  const uint32_t nq = min(kSq8Tile, a.entry_off[L + 1] - e0);
  const uint32_t ksteps = a.ksteps;

  if (threadIdx.x < kSq8Tile) {
    const uint32_t t = threadIdx.x;
    uint2 en = make_uint2(0u, 0u);
    uint4 qi = make_uint4(0u, 0u, 0u, 0u);
    if (t < nq) {
      en = a.entries[e0 + t];
      qi = a.qinfo[en.x];
    }
    s_ent[t] = en;
    sq8_query_terms(qi, t, s_qd, s_a1);
    s_cnt[t] = 0u;
    s_bound[t] = kInf32;
  }
  __syncthreads();
  const uint32_t h = (uint32_t)lane >> 5, slot = (uint32_t)lane & 31u;
  // the lane's own operand words: query s_ent[slot], half h (an empty slot reads query 0; the epilogue masks it)
  const uint4* qp = a.qwords + (size_t)s_ent[slot].x * ksteps * 2 + h;
  if (QLDS) {  // the gather: word (kstep, lane) <- query of slot lane & 31, half lane >> 5; zero for an empty slot
    for (uint32_t ks = w; ks < ksteps; ks += 4) s_q[ks * 64u + (uint32_t)lane] = slot < nq ? qp[ks * 2u] : make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
  }

  const uint32_t sb0 = seg * a.segb, nb = min(nblk, sb0 + a.segb) - sb0;  // nb >= 1: seg < nseg
  const uint32_t rounds = (nb + 3u) >> 2;                                 // workgroup-uniform
  const uint32_t wb0 = min(nb, w * rounds);                               // the wave's quarter
  const uint32_t nbw = min(nb, (w + 1u) * rounds) - wb0;
  const uint32_t* bl = a.list_blocks + lb0 + sb0 + wb0;                   // the wave's block ids
  const double dd = (double)a.d;

  uint32_t blk = nbw ? rfl(bl[0]) : 0u;
  uint4 buf[kSq8Ahead];
  {
    const uint4* p = a.codes + (size_t)blk * ksteps * 64 + (uint32_t)lane;
#pragma unroll
    for (int u = 0; u < kSq8Ahead; ++u) buf[u] = nbw && (uint32_t)u < ksteps ? p[(size_t)u * 64] : make_uint4(0u, 0u, 0u, 0u);
  }

  for (uint32_t r = 0; r < rounds; ++r) {
    if (r < nbw) {  // wave-uniform
      sq8_i32x16 acc = {0};
      const bool has_next = r + 1u < nbw;
      const uint32_t nxt = has_next ? rfl(bl[r + 1u]) : blk;
      const uint4* pb = a.codes + (size_t)blk * ksteps * 64 + (uint32_t)lane;
      const uint4* pn = a.codes + (size_t)nxt * ksteps * 64 + (uint32_t)lane;
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
            buf[u] = pn[(size_t)u * 64];
          }
          if (ks < ksteps) {
            const uint4 qw = QLDS ? s_q[ks * 64u + (uint32_t)lane] : qp[ks * 2u];
            const sq8_i32x4 av = {(int)qw.x, (int)qw.y, (int)qw.z, (int)qw.w};
            const sq8_i32x4 bv = {(int)cw.x, (int)cw.y, (int)cw.z, (int)cw.w};
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc, 0, 0, 0);
          }
        }
      }

      const uint32_t row = blk * 32u + slot;  // a pool row: every block of a list is whole in the pool
      if (a.dead[row] == 0u) {
        const Sq8RowTerms rt = sq8_row_terms(a.info[row], a.d);
        const uint32_t seq = a.seq_of_row[row];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const uint32_t qi = (uint32_t)(reg & 3) + 8u * (uint32_t)(reg >> 2) + 4u * h;
          if (qi < nq) {
            const uint32_t chi = sq8_score_bits(acc[reg], s_a1[qi], s_qd + 4 * qi, rt, dd);
            if (chi <= s_bound[qi]) {
              const uint32_t at = atomicAdd(&s_cnt[qi], 1u);
              s_buf[qi * CAP + at] = ((uint64_t)chi << 32) | seq;
            }
          }
        }
      }
      blk = nxt;
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
    const uint2 en = s_ent[qi];
    uint64_t* out = a.part + ((size_t)(en.y * a.segs + seg) * a.B + en.x) * a.k;
#pragma unroll
    for (int rr = 0; rr < KR; ++rr) {
      const uint32_t e = rr * 64 + lane;
      if (e < a.k) out[e] = ((uint64_t)tk.hi[rr] << 32) | tk.lo[rr];  // (kInf32, kInf32) = ~0 where the list is short
    }
  }
}

// add: source row i of the call took ordinal seq0 + i and pool row dest[i]
static __global__ void ivfsq8_place_kernel(const uint32_t* __restrict__ dest, uint64_t n, uint32_t seq0, uint32_t* __restrict__ seq_of_row,
                                    uint32_t* __restrict__ row_of_seq, uint32_t* __restrict__ dead) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const uint32_t row = dest[e];
  seq_of_row[row] = seq0 + (uint32_t)e;
  row_of_seq[seq0 + e] = row;
  dead[row] = 0u;
}

// candidate slot (b, j) of a refined search, a seq -> out[b * fk + j][dpad], zero beyond d; slots beyond the count are
// skipped (sq8_decode_cand_kernel with the pool row looked up)
static __global__ void ivfsq8_decode_cand_kernel(const uint4* __restrict__ blocks, const uint4* __restrict__ info, const uint32_t* __restrict__ row_of_seq,
                                          uint32_t ksteps, uint32_t d, uint32_t dpad, const uint32_t* __restrict__ cand,
                                          const uint32_t* __restrict__ cand_cnt, uint32_t B, uint32_t fk, float* __restrict__ out) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (uint64_t)B * fk * dpad) return;
  const uint64_t slot = e / dpad;
  const uint32_t i = (uint32_t)(e - slot * dpad);
  const uint32_t b = (uint32_t)(slot / fk), j = (uint32_t)(slot - (uint64_t)b * fk);
  if (j >= min(cand_cnt[b], fk)) return;
  float v = 0.0f;
  if (i < d) {
    const uint32_t row = row_of_seq[cand[slot]];
    const uint8_t* word = (const uint8_t*)(blocks + ((size_t)(row >> 5) * ksteps + (i >> 5)) * 64 + ((i >> 4) & 1u) * 32u + (row & 31u));
    const uint4 inf = info[row];
    v = sq8_value(__uint_as_float(inf.x), __uint_as_float(inf.y), (uint32_t)word[i & 15u] ^ 0x80u);
  }
  out[e] = v;
}

static __global__ void ivfsq8_fill_kernel(uint32_t* __restrict__ p, uint64_t n, uint32_t v) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) p[e] = v;
}

// set_deleted: seqs -> the dead words of their pool rows
static __global__ void ivfsq8_set_flags_kernel(const uint32_t* __restrict__ seqs, uint64_t n, uint32_t flag, const uint32_t* __restrict__ row_of_seq,
                                        uint32_t* __restrict__ dead) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) dead[row_of_seq[seqs[e]]] = flag;
}

}  // namespace fvdb
