// kernels_mmr.h — diverse selection: of the n <= 256 candidates a search of fetch_k returned for
// one query, keep k that are near the query and far from each other (maximal marginal relevance), optionally after
// dropping every later copy of an id.  No counterpart in the reference beyond the grouping by id in
// ResultMerger::merge (src/hybrid/search_integration.rs:226-296); the definition is this project's and is exact:
//
//   kept[c]   = !distinct || no c' < c has id[c'] == id[c]
//   pick 0    = the first kept candidate
//   after every pick s, for each kept unpicked c:
//     t       = dist(x_c, x_s) by the reference fold (score_rows.h: the picked row is the "query")
//     m[c]    = min(m[c], t)                          m starts at +inf
//     gain[c] = b * m[c] - a * dq[c]                  a = f32(lam), b = 1 - a; two multiplies and a subtract, no FMA
//   next pick = the largest gain as an f32 value, the smallest c among equals
//   min(k, kept) picks, written in pick order
//
// ONE WORKGROUP of 256 per query: thread c owns candidate c for the id scan, the gain and the argmax; the four waves
// share a round's scoring in chunks of up to 16 rows, each wave with its own product tile.  The round count is uniform
// over the workgroup, and no __syncthreads sits under a lane- or wave-dependent condition.
#pragma once
#include "common.h"
#include "score_rows.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kMmrMax = 256;      // candidates per query = threads per workgroup (FVDB_MAX_K)
constexpr uint32_t kMmrNone = 0xFFFFFFFFu;

// rows [B][fetch_k][stride] f32 (stride % 4 == 0, dimensions from d up to stride zero), ids / dq [B][fetch_k],
// counts[B] -> out_ids / out_dist / out_rank [B][k], out_counts[B]
__global__ __launch_bounds__(256) void mmr_select_kernel(const float* __restrict__ rows, uint32_t stride,
                                                         const uint64_t* __restrict__ ids, const float* __restrict__ dq,
                                                         const uint32_t* __restrict__ counts, uint32_t fetch_k, uint32_t k, float a,
                                                         float b, uint32_t distinct, uint64_t* __restrict__ out_ids,
                                                         float* __restrict__ out_dist, uint32_t* __restrict__ out_rank,
                                                         uint32_t* __restrict__ out_counts) {
  __shared__ __attribute__((aligned(16))) float s_tile[4][kScoreTileFloats];
  __shared__ uint64_t s_id[kMmrMax];
  __shared__ float s_m[kMmrMax];
  __shared__ uint32_t s_list[kMmrMax];  // the kept unpicked candidates of a round, ascending
  __shared__ uint32_t s_wcnt[4], s_wc[4];
  __shared__ float s_wg[4];
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t qb = (size_t)blockIdx.x;
  const uint32_t n = min(counts[qb], fetch_k);
  const float* qrows = rows + qb * fetch_k * stride;
  const float pinf = __uint_as_float(0x7F800000u), ninf = __uint_as_float(0xFF800000u);

  const uint64_t my_id = t < n ? ids[qb * fetch_k + t] : ~0ull;
  const float my_dq = t < n ? dq[qb * fetch_k + t] : pinf;
  s_id[t] = my_id;
  s_m[t] = pinf;
  __syncthreads();
  // step 1: all-pairs compare in LDS (every lane reads the same word: a broadcast)
  bool kept = t < n;
  if (distinct && kept)
    for (uint32_t c = 0; c < t; ++c) kept = kept && s_id[c] != my_id;
  const uint32_t n_kept = (uint32_t)__syncthreads_count(kept);
  const uint32_t rounds = min(k, n_kept);  // uniform
  bool open = kept;                        // kept and not yet picked
  uint32_t pick = kMmrNone;
  for (uint32_t r = 0; r < rounds; ++r) {
    // the open candidates, compacted in ascending order
    const uint64_t vote = __ballot(open);
    if (lane == 0) s_wcnt[wave] = (uint32_t)__popcll(vote);
    __syncthreads();
    uint32_t before = 0, nopen = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      const uint32_t cw = s_wcnt[w];
      before += w < wave ? cw : 0u;
      nopen += cw;
    }
    if (open) s_list[before + ballot_rank(vote, lane)] = t;
    __syncthreads();
    nopen = rfl(nopen);
    if (r > 0) {
      // distances of the last pick's row to every open row: chunks of `step` rows dealt round-robin to the waves
      const uint32_t step = nopen > 32 ? 16u : nopen > 16 ? 8u : 4u;
      const float* last = qrows + (size_t)pick * stride;
      for (uint32_t c0 = wave * step; c0 < nopen; c0 += 4 * step) {
        const uint32_t cnt = min(step, nopen - c0);
        const uint32_t c = s_list[c0 + min(lane, cnt - 1)];
        const float d = score_rows_upto16<float>(qrows, stride, last, c, 0u, cnt, s_tile[wave], (int)lane);
        if (lane < cnt) s_m[c] = fminf(s_m[c], d);
      }
      __syncthreads();
    }
    // argmax of the gain; round 0 has no pick behind it: the first kept candidate
    float g = ninf;
    if (open) {
      if (r > 0) {
        const float bm = b * s_m[t];
        const float ad = a * my_dq;
        const float gain = bm - ad;
        g = gain == gain ? gain : ninf;
      } else {
        g = 0.0f;
      }
    }
    const float wmax = wave_max_f(g);
    const uint64_t best = __ballot(open && g == wmax);
    if (lane == 0) {
      s_wg[wave] = wmax;
      s_wc[wave] = best ? wave * 64u + (uint32_t)__ffsll((unsigned long long)best) - 1u : kMmrNone;
    }
    __syncthreads();
    float bg = ninf;
    pick = kMmrNone;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {  // waves ascending and a strict compare: the smallest c among equal gains
      const uint32_t cw = s_wc[w];
      const float gw = s_wg[w];
      if (cw != kMmrNone && (pick == kMmrNone || gw > bg)) {
        bg = gw;
        pick = cw;
      }
    }
    pick = rfl(pick);  // rounds <= n_kept: an open candidate exists in every round
    if (t == pick) {
      open = false;
      out_ids[qb * k + r] = my_id;
      out_dist[qb * k + r] = my_dq;
      out_rank[qb * k + r] = t;
    }
  }
  if (t >= rounds && t < k) {
    out_ids[qb * k + t] = ~0ull;
    out_dist[qb * k + t] = pinf;
    out_rank[qb * k + t] = kMmrNone;
  }
  if (t == 0) out_counts[qb] = rounds;
}

}  // namespace fvdb
