// kernels_curve.h — recall and precision at EVERY nprobe from one search of every list.
// Extends IVFIndex::evaluate_search_quality (src/ivf/operations.rs:329-391), which answers for one n_probe per call.
//
// The reference's ground truth is the top k of the search of every list in centroid-rank order; a search at nprobe = p
// scans the first p ranked lists at the same scan positions.  A truth row whose list ranks below p is therefore always
// in the p-probe result (fewer rows precede it there), and a p-probe result row that is in the truth is such a row.  So,
// per query, with no id stored in two lists:
//   matches(p)    = truth entries whose list has centroid rank < p
//   len_result(p) = min(k, live rows of the first p ranked lists)
//   recall(p)     = truth empty ? 1 : matches(p) / min(len(truth), k)
//   precision(p)  = len_result(p) == 0 ? 0 : matches(p) / len_result(p)      (search_quality_kernel's f32 divisions)
//
//   live    list_live_kernel: live rows per list, a popcount of the live words of its blocks; once per call.
//   count   curve_query_kernel: one workgroup per query.  Two u32 tables over the ranks in dynamic LDS: the exclusive
//           prefix of the ranked lists' block counts (wide_base_kernel's rule: seq / 64 falls in exactly one rank) and
//           the inclusive prefix of their live rows.  Every truth key finds its rank by binary search (wide_rank_of);
//           the block table, no longer needed, becomes the per-rank histogram, and its inclusive scan is matches(p).
//   sum     curve_sum_kernel: one thread per p adds the chunk's per-query values to the running totals in query order,
//           plain f32 adds: the reference's `total_recall += recall` (:379-387).
#pragma once
#include "kernels_wide.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kCurveThreads = 512;
constexpr uint32_t kCurveKeysPerThread = kWideMaxK / kCurveThreads;  // ranks of a thread's truth keys stay in registers
constexpr uint32_t kCurveMaxLists = 16384;  // two u32 tables of this many ranks fill 128 KiB of the CU's 160 KiB of LDS

// out[L] = live rows of list L: the set bits of `live` (the pool's words, or a mask's) over the list's blocks.  A bit
// past the list's last row is never set.  One wave per list.
__global__ __launch_bounds__(256) void list_live_kernel(const uint32_t* __restrict__ list_off,
                                                        const uint32_t* __restrict__ list_blocks,
                                                        const uint64_t* __restrict__ live, uint32_t nlist,
                                                        uint32_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t L = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (L >= nlist) return;
  const uint32_t b1 = list_off[L + 1];
  uint32_t n = 0;
  for (uint32_t b = list_off[L] + lane; b < b1; b += 64) n += (uint32_t)__popcll(live[list_blocks[b]]);
  n = wave_sum_u(n);
  if (lane == 0) out[L] = n;
}

// s[0 .. n) <- its prefix sums (INCL: s[i] counts itself), by a whole workgroup of kCurveThreads; s in LDS, s_wave one
// word per wave.  The wave scan is wave_ops.h's; the carry between rounds of kCurveThreads words is workgroup-uniform.
template <bool INCL>
__device__ __forceinline__ void curve_scan(uint32_t* s, uint32_t n, uint32_t* s_wave) {
  constexpr uint32_t T = kCurveThreads, W = T / 64;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t carry = 0;
  for (uint32_t c0 = 0; c0 < n; c0 += T) {
    const uint32_t i = c0 + tid;
    const uint32_t x = i < n ? s[i] : 0u;
    const uint32_t incl = wave_incl_scan_u(x, (int)lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = carry, round = 0;
    for (uint32_t w = 0; w < W; ++w) {
      const uint32_t t = s_wave[w];
      if (w < wave) before += t;
      round += t;
    }
    if (i < n) s[i] = before + incl - (INCL ? 0u : x);
    carry += round;
    __syncthreads();
  }
}

struct CurveArgs {
  const uint32_t* probes;     // [B][np] every list in centroid-rank order (0xFFFFFFFF = "no list": empty)
  const uint32_t* list_off;   // the list table's block offsets
  const uint32_t* list_live;  // [nlist] list_live_kernel
  const uint64_t* keys;       // [B][k] the truth: keys of the every-list search, low word = seq
  const uint32_t* counts;     // [B] its hit counts
  uint32_t np, k;             // np = nlist
  float* recall;              // [B][np] entry p - 1 <-> nprobe = p
  float* precision;
};

__global__ __launch_bounds__(kCurveThreads) void curve_query_kernel(const CurveArgs a) {
  extern __shared__ uint32_t s_curve[];  // [np] block prefix, then histogram and matches; [np] live prefix
  __shared__ uint32_t s_wave[kCurveThreads / 64];
  constexpr uint32_t T = kCurveThreads;
  const uint32_t tid = threadIdx.x, q = blockIdx.x, np = a.np, k = a.k;
  uint32_t* s_blk = s_curve;
  uint32_t* s_live = s_curve + np;
  const uint32_t* __restrict__ pr = a.probes + (size_t)q * np;
  for (uint32_t r = tid; r < np; r += T) {
    const uint32_t L = pr[r];
    const bool have = L != kInf32;
    s_blk[r] = have ? a.list_off[L + 1] - a.list_off[L] : 0u;
    s_live[r] = have ? a.list_live[L] : 0u;
  }
  __syncthreads();
  curve_scan<false>(s_blk, np, s_wave);
  curve_scan<true>(s_live, np, s_wave);

  // rank of every truth key: seq / 64 is a block of exactly one rank
  const uint32_t nt = min(a.counts[q], k);
  const uint64_t* __restrict__ keys = a.keys + (size_t)q * k;
  uint32_t rank[kCurveKeysPerThread];
#pragma unroll
  for (uint32_t j = 0; j < kCurveKeysPerThread; ++j) {
    const uint32_t e = j * T + tid;
    rank[j] = e < nt ? wide_rank_of(s_blk, np, (uint32_t)keys[e] >> 6) : kInf32;
  }
  __syncthreads();
  for (uint32_t r = tid; r < np; r += T) s_blk[r] = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < kCurveKeysPerThread; ++j)
    if (rank[j] != kInf32) atomicAdd(&s_blk[rank[j]], 1u);
  __syncthreads();
  curve_scan<true>(s_blk, np, s_wave);  // matches(p) at p - 1

  float* __restrict__ rec = a.recall + (size_t)q * np;
  float* __restrict__ prec = a.precision + (size_t)q * np;
  for (uint32_t r = tid; r < np; r += T) {
    const uint32_t matches = s_blk[r], nr = min(k, s_live[r]);
    rec[r] = nt == 0 ? 1.0f : (float)matches / (float)nt;
    prec[r] = nr == 0 ? 0.0f : (float)matches / (float)nr;
  }
}

// total[p] = total[p] + value[b][p] for b ascending: the reference's sum in query order, no tree.  One thread per p.
__global__ __launch_bounds__(256) void curve_sum_kernel(const float* __restrict__ recall, const float* __restrict__ precision,
                                                        uint32_t B, uint32_t np, float* __restrict__ total_recall,
                                                        float* __restrict__ total_precision) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= np) return;
  float tr = total_recall[p], tp = total_precision[p];
#pragma unroll 8
  for (uint32_t b = 0; b < B; ++b) {
    tr = tr + recall[(size_t)b * np + p];
    tp = tp + precision[(size_t)b * np + p];
  }
  total_recall[p] = tr;
  total_precision[p] = tp;
}

}  // namespace fvdb
