// kernels_ivfpq.h — the probed ADC scan over PQ codes held in inverted lists (include/fvdb.h,
// "IVF over PQ codes").  The tables, the fold of a code word, the refine and the merge are kernels_pq.h's and
// kernels_flat.h's, unchanged; what is here is the walk between them.
//
//   ivfpq_scan_kernel   query-stationary: a workgroup holds the ADC tables of QT queries in LDS; after the one barrier a
//                       wave belongs to ONE query and one slice of its probe ranks, walks those lists block by block and
//                       carries one WaveTopK across all of them, so the bound is shared between a query's lists
//   ivfpq_place_kernel  add: flat [n][m] codes packed into the 16-byte words of their destination blocks, the tables
//                       between pool rows and add ordinals (seq)
//   ivfpq_live_kernel   add, last: the placed rows' dead words cleared
//   ivfpq_fill_kernel   32-bit fill (the pool's "dead" words, the counters)
//
// Pool.  64-row code blocks in kernels_pq.h's block form, codes[(block * m16 + chunk) * 64 + lane], each owned by one
// list; per pool row a dead word (1 also for the unfilled tail of a list's last block) and seq_of_row.
// list_blocks[list_off[L] .. list_off[L + 1]) are list L's blocks in fill order.  The key of a candidate is
// (bits(adc) << 32) | seq, so ties go to the row added first whichever lists hold the tied rows.
#pragma once
#include "common.h"
#include "kernels_pq.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kIvfPqMaxLists = 16384;
constexpr int kIvfPqChains = 1;       // blocks a lane folds side by side in independent add chains (2 measured no faster: section 9zc)
constexpr int kIvfPqAhead = kPqAhead;  // code words a scan wave keeps in flight, across block and list boundaries

struct IvfPqScanArgs {
  const uint4* codes;            // [pool blocks][m16][64] code words
  const uint32_t* dead;          // [pool rows]: non-zero = not a candidate (unfilled, deleted, or outside an allow-set)
  const uint32_t* seq_of_row;    // [pool rows]
  const uint32_t* list_off;      // [nlist + 1] into list_blocks
  const uint32_t* list_len;      // [nlist] rows
  const uint32_t* list_blocks;   // pool block ids, list by list
  const uint32_t* probes;        // [B][np] list ids in probe order
  const float* tables;           // [B][m][ka]
  uint64_t* part;                // [S][B][k] keys (adc bits << 32 | seq), ~0 = none
  unsigned long long* stats;     // [2]: rows scored, (query, list) pairs; added to
  uint32_t nlist, np, m, m16, ka, ts /* floats of a table row in LDS: ka or ka + 1 */, B, k, S;
  // residual codes (RES; kernels_ivfrpq.h), null otherwise: `tables` then holds inner products
  const float* term_of_row;      // [pool rows] the row term r^.(r^ + 2c)
  const float* base;             // [B][np] the squared fold of the query against the centroid of each probe rank
};

// The blocks of a wave's lists, in walk order: ranks r, r + S, ... of one query, every list's blocks in fill order.
// Wave-uniform throughout.  next() past the last block returns 0 and is never dereferenced.  `rank` is the probe rank of
// the list that the block last returned belongs to (the residual scan's base is per rank).
struct IvfPqWalk {
  const uint32_t* pr;  // the query's probe row
  const uint32_t* list_off;
  const uint32_t* list_blocks;
  uint32_t r, S, np, nlist, pos, end;
  uint32_t rank = 0;
  __device__ __forceinline__ uint32_t next() {
    while (pos == end) {
      if (r >= np) return 0u;
      const uint32_t L = rfl(pr[r]);
      if (L < nlist) rank = r;
      r += S;
      if (L < nlist) {
        pos = rfl(list_off[L]);
        end = rfl(list_off[L + 1]);
      }
    }
    return rfl(list_blocks[pos++]);
  }
};

// Workgroup = 4 waves and QT queries: the tables go to LDS, one barrier, then wave w is query w % QT of the group and
// slice blockIdx.y * (4 / QT) + w / QT of that query's probe ranks (rank r belongs to slice r mod S: near and far lists
// mix).  Lane = row.  The wave's code words form ONE sequence over all its lists; kIvfPqAhead of them are in flight, and
// the fetch side and the fold side each know their next block a block ahead (two walks over the same tables: the second
// reads what the first brought in), so neither a block's nor a list's end drains the pipeline.  A block's dead words and
// seqs are loaded when the fold reaches the block before it.  CH blocks are folded side by side in independent add
// chains (their words alternate in the sequence); the index launches kIvfPqChains.
//
// RES (residual codes): the tables are inner products, the fold side also carries the probe rank
// of each block, and with a block's dead words and seqs it loads the lane's row term and (one address a wave) the base
// of the block's list; the block-end step is sqrt(max((base + term) - 2 ip, +0)).  Without RES none of this is compiled.
template <int QT, int KR, int CH, bool RES = false>
__global__ __launch_bounds__(256) void ivfpq_scan_kernel(const IvfPqScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_tab[];  // [QT][m][ts]
  constexpr int AH = kIvfPqAhead;
  constexpr uint32_t SPW = 4 / QT;  // slices a workgroup's own waves take
  const int lane = threadIdx.x & 63;
  const uint32_t w = threadIdx.x >> 6;
  const uint32_t q0 = blockIdx.x * QT;
  const uint32_t ne = min((uint32_t)QT, a.B - q0);
  const uint32_t tsz = a.m * a.ts;
#pragma unroll
  for (int q = 0; q < QT; ++q) {
    if ((uint32_t)q < ne) {  // workgroup-uniform
      const float* src = a.tables + (size_t)(q0 + (uint32_t)q) * a.m * a.ka;
      for (uint32_t e = threadIdx.x; e < tsz; e += 256) {
        const uint32_t j = e / a.ts, c = e - j * a.ts;
        s_tab[(uint32_t)q * tsz + e] = c < a.ka ? src[j * a.ka + c] : 0.0f;
      }
    }
  }
  __syncthreads();
  const uint32_t qi = w % QT, s = blockIdx.y * SPW + w / QT;
  if (qi >= ne || s >= a.S) return;  // whole waves leave; no workgroup barrier below
  const uint32_t b = q0 + qi;
  const float* tab = s_tab + qi * tsz;
  const uint32_t* pr = a.probes + (size_t)b * a.np;

  // the wave's lists, counted once: blocks (the length of the word sequence), rows and lists for the counters
  uint32_t nblk = 0, nrows = 0, nlists = 0;
  for (uint32_t r = s + (uint32_t)lane * a.S; r < a.np; r += 64u * a.S) {
    const uint32_t L = pr[r];
    if (L < a.nlist) {
      nblk += a.list_off[L + 1] - a.list_off[L];
      nrows += a.list_len[L];
      ++nlists;
    }
  }
  nblk = rfl(wave_sum_u(nblk));
  nrows = wave_sum_u(nrows);
  nlists = wave_sum_u(nlists);
  if (lane == 0) {
    atomicAdd(a.stats + 0, (unsigned long long)nrows);
    atomicAdd(a.stats + 1, (unsigned long long)nlists);
  }
  const uint32_t ngrp = (nblk + CH - 1) / CH;           // groups of CH blocks folded side by side
  const uint64_t nw = (uint64_t)ngrp * CH * a.m16;      // words of the wave: chunk c of a group's blocks, then chunk c + 1

  IvfPqWalk fw{pr, a.list_off, a.list_blocks, s, a.S, a.np, a.nlist, 0u, 0u};  // the fetch side
  IvfPqWalk cw = fw;                                                            // the fold side
  // a group's blocks and the next group's; a block past the wave's last reads as pool block 0, whose words are loaded
  // (the pool is not empty when nblk > 0) and whose rows are dropped
  uint32_t fblk[CH], fnxt[CH], cblk[CH], cnxt[CH], fch = 0;
  uint32_t crk[CH], cnrk[CH];  // RES: the probe ranks of cblk and cnxt
#pragma unroll
  for (int c = 0; c < CH; ++c) fblk[c] = fw.next();
#pragma unroll
  for (int c = 0; c < CH; ++c) fnxt[c] = fw.next();
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    cblk[c] = cw.next();
    crk[c] = cw.rank;
  }
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    cnxt[c] = cw.next();
    cnrk[c] = cw.rank;
  }
  auto fetch = [&](const int sel) {  // sel = position in the unrolled body mod CH: a constant after unrolling
    const uint4 v = a.codes[((size_t)fblk[sel] * a.m16 + fch) * 64 + (uint32_t)lane];
    if (sel == CH - 1 && ++fch == a.m16) {
      fch = 0;
#pragma unroll
      for (int c = 0; c < CH; ++c) fblk[c] = fnxt[c];
#pragma unroll
      for (int c = 0; c < CH; ++c) fnxt[c] = fw.next();
    }
    return v;
  };

  static_assert(kIvfPqAhead % CH == 0, "a group's words keep their places in the unrolled body");
  uint4 buf[AH];
#pragma unroll
  for (int u = 0; u < AH; ++u) {
    buf[u] = make_uint4(0, 0, 0, 0);
    if ((uint64_t)u < nw) buf[u] = fetch(u % CH);
  }
  uint32_t dw[CH], sq[CH];  // of the lane's rows in the blocks being folded
  // RES: the lane's row term, and the base of the block's list.  The base is one address a wave but stays in a VGPR:
  // moving it to an SGPR where it is loaded waits for that load, and with it for every code word in flight (section 9zd)
  float tm[CH], bs[CH];
  const float* basew = a.base + (size_t)b * a.np;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    dw[c] = 1u;
    sq[c] = kInf32;
    tm[c] = bs[c] = 0.0f;
    if ((uint32_t)c < nblk) {
      dw[c] = a.dead[(size_t)cblk[c] * 64 + (uint32_t)lane];
      sq[c] = a.seq_of_row[(size_t)cblk[c] * 64 + (uint32_t)lane];
      if (RES) {
        tm[c] = a.term_of_row[(size_t)cblk[c] * 64 + (uint32_t)lane];
        bs[c] = basew[crk[c]];
      }
    }
  }

  WaveTopK<KR> tk;
  tk.init();
  float acc[CH][1];
#pragma unroll
  for (int c = 0; c < CH; ++c) acc[c][0] = 0.0f;
  uint32_t chunk = 0, done = 0;  // blocks folded
  for (uint64_t wi = 0; wi < nw; wi += AH) {
#pragma unroll
    for (int u = 0; u < AH; ++u) {
      if (wi + u < nw) {  // wave-uniform
        const int sel = u % CH;
        const uint4 cwd = buf[u];
        if (wi + u + AH < nw) buf[u] = fetch(sel);
        const uint32_t jn = min(16u, a.m - 16u * chunk);
        const float* t = tab + 16u * chunk * a.ts;
        if (jn == 16u) pq_fold_word<1, true>(cwd, t, tsz, a.ts, jn, acc[sel]);
        else pq_fold_word<1, false>(cwd, t, tsz, a.ts, jn, acc[sel]);
        if (sel == CH - 1 && ++chunk == a.m16) {
          chunk = 0;
          uint32_t chi[CH], seq[CH];
#pragma unroll
          for (int c = 0; c < CH; ++c) {
            float sum = acc[c][0];
            if (RES) {
              const float v = (bs[c] + tm[c]) - (sum + sum);
              sum = v > 0.0f ? v : 0.0f;
            }
            chi[c] = dw[c] == 0u ? __float_as_uint(sqrtf(sum)) : kInf32;
            acc[c][0] = 0.0f;
            seq[c] = sq[c];
            cblk[c] = cnxt[c];
            crk[c] = cnrk[c];
          }
#pragma unroll
          for (int c = 0; c < CH; ++c) {
            cnxt[c] = cw.next();
            cnrk[c] = cw.rank;
          }
#pragma unroll
          for (int c = 0; c < CH; ++c) {  // the next group's words, a group ahead of their use
            dw[c] = 1u;
            if (done + CH + (uint32_t)c < nblk) {
              dw[c] = a.dead[(size_t)cblk[c] * 64 + (uint32_t)lane];
              sq[c] = a.seq_of_row[(size_t)cblk[c] * 64 + (uint32_t)lane];
              if (RES) {
                tm[c] = a.term_of_row[(size_t)cblk[c] * 64 + (uint32_t)lane];
                bs[c] = basew[crk[c]];
              }
            }
          }
#pragma unroll
          for (int c = 0; c < CH; ++c) {
            if (done == 0 && c == 0) {  // empty list: the sorted tile IS the list (the low key word is seq, not the pool row)
              uint32_t shi = chi[0], slo = chi[0] != kInf32 ? seq[0] : kInf32;
              wave_sort64(shi, slo, lane);
              tk.hi[0] = shi;
              tk.lo[0] = slo;
            } else {
              uint32_t th, tl;
              tk.kth(a.k, th, tl);
              offer<KR>(tk, a.k, chi[c], seq[c], th, tl, lane);
            }
          }
          done += CH;
        }
      }
    }
  }

  uint64_t* out = a.part + ((size_t)s * a.B + b) * a.k;  // a wave without a live row writes an empty list
#pragma unroll
  for (int rr = 0; rr < KR; ++rr) {
    const uint32_t e = rr * 64 + lane;
    if (e < a.k) out[e] = ((uint64_t)tk.hi[rr] << 32) | tk.lo[rr];
  }
}

// add: source row i of the call took ordinal seq0 + i and pool row dest[i]; thread (i, chunk) packs 16 of its flat codes
// (code 0 beyond m) into the row's word of that chunk
static __global__ void ivfpq_place_kernel(const uint8_t* __restrict__ flat /* [n][m] */, const uint32_t* __restrict__ dest, uint64_t n,
                                          uint32_t m, uint32_t m16, uint32_t seq0, uint4* __restrict__ codes,
                                          uint32_t* __restrict__ seq_of_row, uint32_t* __restrict__ row_of_seq,
                                          const float* __restrict__ term /* [n], or null */, float* __restrict__ term_of_row) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * m16) return;
  const uint64_t i = e / m16;
  const uint32_t chunk = (uint32_t)(e - i * m16);
  const uint32_t row = dest[i];
  uint32_t wv[4] = {0u, 0u, 0u, 0u};
  const uint32_t jn = min(16u, m - 16u * chunk);
  for (uint32_t j = 0; j < jn; ++j) wv[j >> 2] |= (uint32_t)flat[i * m + 16u * chunk + j] << (8u * (j & 3u));
  codes[((size_t)(row >> 6) * m16 + chunk) * 64 + (row & 63u)] = make_uint4(wv[0], wv[1], wv[2], wv[3]);
  if (chunk == 0) {
    seq_of_row[row] = seq0 + (uint32_t)i;
    row_of_seq[seq0 + i] = row;
    if (term) term_of_row[row] = term[i];  // residual codes: the row term travels with the row
  }
}

// add, last step: the placed rows become candidates once everything else of the call is in HBM
static __global__ void ivfpq_live_kernel(const uint32_t* __restrict__ dest, uint64_t n, uint32_t* __restrict__ dead) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) dead[dest[e]] = 0u;
}

static __global__ void ivfpq_fill_kernel(uint32_t* __restrict__ p, uint64_t n, uint32_t v) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) p[e] = v;
}

// set_deleted: seqs -> the dead words of their pool rows
static __global__ void ivfpq_set_flags_kernel(const uint32_t* __restrict__ seqs, uint64_t n, uint32_t flag, const uint32_t* __restrict__ row_of_seq,
                                              uint32_t* __restrict__ dead) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) dead[row_of_seq[seqs[e]]] = flag;
}

}  // namespace fvdb
