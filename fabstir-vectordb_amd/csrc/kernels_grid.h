// kernels_grid.h — recall and precision of the hybrid search at EVERY pair (efs[i], n_probes[j]) from one exact search,
// one traversal per listed ef and one list search per listed n_probe.  Extends
// evaluate_search_quality of the graph and the hybrid index (sections 9k, 9q), which answers for one pair per call.
//
// Per query: G = the recent part at efs[i] (<= rk entries, ascending), H = the historical part at n_probes[j] (<= hk
// entries, ascending), T = the ids of the exact result (<= k).  The hybrid result is the first L = min(k, |G| + |H|)
// entries of the stable merge, recent first on equal distances (merge_parts, host/hybrid_index.cpp; src/hybrid/core.rs
// :476-485).  Membership in that prefix is monotone in each part, so the result is the first a entries of G and the
// first L - a of H, and a comes from one binary search: entry a of G is inside iff a + #{h in H : d_h < d_G[a]} < L.
// With fG[x] = entries among the first x of G whose id is in T, and fH likewise,
//   matches   = fG[a] + fH[L - a]                                (an id held twice counts twice)
//   recall    = T empty ? 1 : matches / min(|T|, k)
//   precision = L == 0  ? 0 : matches / L                         (search_quality_kernel's f32 divisions)
// fG and fH depend on one list and T only, not on the pair: (E + P) k log k for the flags, E P log k for the pairs.
//
//   flags   grid_flags_kernel: one workgroup per query.  T goes into LDS and is sorted there (lds_bitonic_sort_u64,
//           kernels_wide.h: the wide selection's sort); then one wave per list: every entry finds its id by binary search
//           and the wave's ballot gives the inclusive prefix counts, written to pfx[list][query][0 .. n].
//   pairs   grid_pairs_kernel: one lane per (i, j, query), the query fastest.  The binary search above, two prefix
//           reads, two divisions.
// The sums over the queries are the caller's, in query order (compare_id_blocks' loop).
#pragma once
#include "kernels_wide.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kGridThreads = 512;
constexpr uint32_t kGridMaxPoints = 64;  // listed efs, listed n_probes

struct GridArgs {
  const uint64_t* t_ids;   // [B][k] the truth
  const uint32_t* t_cnt;   // [B]
  const uint64_t* g_ids;   // [E][B][rk] the recent parts (null when E == 0)
  const float* g_dist;
  const uint32_t* g_cnt;   // [E][B]
  const uint64_t* h_ids;   // [P][B][hk] the historical parts (null when P == 0)
  const float* h_dist;
  const uint32_t* h_cnt;   // [P][B]
  uint32_t B, k, rk, hk, E, P;
  uint32_t* g_pfx;         // [E][B][rk + 1] fG; entries 0 .. min(count, rk) are written
  uint32_t* h_pfx;         // [P][B][hk + 1] fH
  float* recall;           // [max(E, 1)][max(P, 1)][B]
  float* precision;
};

// id among the n ascending keys of s?
__device__ __forceinline__ bool grid_has(const uint64_t* s, uint32_t n, uint64_t id) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (s[mid] < id) lo = mid + 1; else hi = mid;
  }
  return lo < n && s[lo] == id;
}

__global__ __launch_bounds__(kGridThreads) void grid_flags_kernel(const GridArgs a) {
  constexpr uint32_t T = kGridThreads, W = T / 64;
  __shared__ uint64_t s_t[kWideMaxK];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
  const uint32_t nt = min(a.t_cnt[q], a.k);
  uint32_t N = 1;  // <= kWideMaxK: k is
  while (N < nt) N <<= 1;
  const uint64_t* __restrict__ truth = a.t_ids + (size_t)q * a.k;
  for (uint32_t e = tid; e < N; e += T) s_t[e] = e < nt ? truth[e] : ~0ull;
  __syncthreads();
  lds_bitonic_sort_u64(s_t, N, tid, T);
  // the first nt keys are the truth's ids ascending (a pad is ~0, the largest key: it sorts behind or beside them)

  for (uint32_t l = wave; l < a.E + a.P; l += W) {  // wave-uniform: no barrier below
    const bool rec = l < a.E;
    const uint32_t width = rec ? a.rk : a.hk;
    const size_t row = (size_t)(rec ? l : l - a.E) * a.B + q;
    const uint32_t n = rfl(min((rec ? a.g_cnt : a.h_cnt)[row], width));
    const uint64_t* __restrict__ ids = (rec ? a.g_ids : a.h_ids) + row * width;
    uint32_t* __restrict__ pfx = (rec ? a.g_pfx : a.h_pfx) + row * (width + 1);
    if (lane == 0) pfx[0] = 0;
    uint32_t before = 0;
    for (uint32_t e0 = 0; e0 < n; e0 += 64) {
      const uint32_t e = e0 + lane;
      const bool hit = e < n && grid_has(s_t, nt, ids[e]);
      const uint64_t m = __ballot(hit);
      if (e < n) pfx[e + 1] = before + ballot_rank(m, lane) + (hit ? 1u : 0u);
      before += (uint32_t)__popcll(m);
    }
  }
}

// entries of the n ascending distances d that are < x
__device__ __forceinline__ uint32_t grid_below(const float* __restrict__ d, uint32_t n, float x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (d[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void grid_pairs_kernel(const GridArgs a) {
  const uint32_t Pe = max(a.P, 1u), B = a.B;
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (uint64_t)max(a.E, 1u) * Pe * B) return;
  const uint32_t b = (uint32_t)(t % B), ij = (uint32_t)(t / B), i = ij / Pe, j = ij % Pe;
  const size_t grow = (size_t)i * B + b, hrow = (size_t)j * B + b;
  const uint32_t nG = a.E ? min(a.g_cnt[grow], a.rk) : 0u, nH = a.P ? min(a.h_cnt[hrow], a.hk) : 0u;
  const uint32_t L = min(a.k, nG + nH);
  const float* __restrict__ gd = a.E ? a.g_dist + grow * a.rk : nullptr;
  const float* __restrict__ hd = a.P ? a.h_dist + hrow * a.hk : nullptr;
  // recent entries among the first L of the merge: the first x in [L - nH, min(L, nG)] that is outside
  uint32_t lo = L > nH ? L - nH : 0u, hi = min(L, nG);
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;  // < nG
    if (mid + grid_below(hd, nH, gd[mid]) < L) lo = mid + 1; else hi = mid;
  }
  uint32_t matches = 0;
  if (a.E) matches += a.g_pfx[grow * (a.rk + 1) + lo];       // lo <= nG
  if (a.P) matches += a.h_pfx[hrow * (a.hk + 1) + (L - lo)];  // L - lo <= nH
  const uint32_t nt = min(a.t_cnt[b], a.k);
  a.recall[t] = nt == 0 ? 1.0f : (float)matches / (float)nt;
  a.precision[t] = L == 0 ? 0.0f : (float)matches / (float)L;
}

}  // namespace fvdb
