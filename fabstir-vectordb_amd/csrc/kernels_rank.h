// kernels_rank.h — the coarse stage for nprobe > 256: a full ranking of the centroid table, and the recall kernel of
// evaluate_search_quality.  Replaces IVFIndex::search_with_config's centroid ranking (src/ivf/core.rs:645-656) where
// nprobe outgrows the 64 x 4 register list of WaveTopK.
//
//   score   wide_score_kernel (kernels_wide.h) over the one-list table of the centroid pool: every centroid scored with
//           the fold of scan_item, its distance bits written to a per-query arena [cblocks * 64] at its cluster
//           position.  Slots past nlist are dead rows of the pool and hold kInf32.  rank_base_kernel writes the
//           {0, cblocks} rank bases that kernel reads for a single list.
//   rank    rank_sort_kernel: one workgroup per query sorts the keys (distance bits << 32 | cluster position)
//           ascending in dynamic LDS — the order of the reference's stable sort over `centroids` — and writes the
//           first np cluster ids (and distances).  lds_bitonic_sort_u64 (kernels_wide.h) over next_pow2(cblocks * 64)
//           keys: at most 128 KiB.
//
// search_quality_kernel: matches / recall / precision of one result list against another (src/ivf/operations.rs
// :357-377), one wave per query.
#pragma once
#include "kernels_wide.h"

namespace fvdb {

constexpr uint32_t kRankSortMaxLists = 16384;  // 16384 u64 keys fill 128 KiB of the CU's 160 KiB of LDS
constexpr uint32_t kRankThreads = 1024;

__global__ void rank_base_kernel(uint32_t B, uint32_t cblocks, uint32_t* __restrict__ base) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= B) return;
  base[2 * q] = 0;
  base[2 * q + 1] = cblocks;
}

struct RankArgs {
  PoolView pool;          // the centroid pool: ids[slot] = cluster id
  ListTable lists;        // its one-list table
  const uint32_t* arena;  // [B][n] distance bits by cluster position
  uint32_t n, P;          // words per query (cblocks * 64) and the power of two they are padded to
  uint32_t np;            // clusters kept per query, <= nlist <= n
  uint32_t* out_probes;   // [B][np]
  float* out_dist;        // [B][np] or null
};

__global__ __launch_bounds__(kRankThreads) void rank_sort_kernel(const RankArgs a) {
  extern __shared__ uint64_t s_rank[];  // P keys
  const uint32_t tid = threadIdx.x, T = blockDim.x, q = blockIdx.x;
  const uint32_t* __restrict__ ar = a.arena + (size_t)q * a.n;
  for (uint32_t i = tid; i < a.P; i += T) s_rank[i] = i < a.n ? ((uint64_t)ar[i] << 32) | i : ~0ull;
  __syncthreads();
  lds_bitonic_sort_u64(s_rank, a.P, tid, T);

  // cluster position -> pool slot -> cluster id, as merge_topk_kernel resolves a coarse result
  for (uint32_t e = tid; e < a.np; e += T) {
    const uint64_t key = s_rank[e];
    const uint32_t khi = (uint32_t)(key >> 32), pos = (uint32_t)key;
    const bool have = khi != kInf32;
    uint32_t id = kInf32;
    if (have) {
      const uint32_t blk = a.lists.blocks[a.lists.off[0] + (pos >> 6)];
      id = (uint32_t)a.pool.ids[(size_t)blk * 64 + (pos & 63)];
    }
    const size_t o = (size_t)q * a.np + e;
    a.out_probes[o] = id;
    if (a.out_dist) a.out_dist[o] = have ? __uint_as_float(khi) : __uint_as_float(0x7F800000u);
  }
}

// res / truth: [B][k] ids with their hit counts.  matches = result entries whose id occurs among the truth's;
// recall = truth empty ? 1 : matches / min(len(truth), k); precision = result empty ? 0 : matches / len(result).
__global__ __launch_bounds__(256) void search_quality_kernel(const uint64_t* __restrict__ res_ids,
                                                             const uint32_t* __restrict__ res_cnt,
                                                             const uint64_t* __restrict__ truth_ids,
                                                             const uint32_t* __restrict__ truth_cnt, uint32_t B, uint32_t k,
                                                             float* __restrict__ out_recall,
                                                             float* __restrict__ out_precision) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= B) return;
  const uint32_t nr = min(res_cnt[q], k), nt = min(truth_cnt[q], k);
  const uint64_t* __restrict__ res = res_ids + (size_t)q * k;
  const uint64_t* __restrict__ truth = truth_ids + (size_t)q * k;
  uint32_t matches = 0;
  for (uint32_t e0 = 0; e0 < nr; e0 += 64) {
    const uint32_t e = e0 + lane;
    const uint64_t id = e < nr ? res[e] : 0;
    bool hit = false;
    for (uint32_t t = 0; t < nt; ++t) hit |= truth[t] == id;
    matches += (uint32_t)__popcll(__ballot(e < nr && hit));
  }
  if (lane == 0) {
    out_recall[q] = nt == 0 ? 1.0f : (float)matches / (float)nt;
    out_precision[q] = nr == 0 ? 0.0f : (float)matches / (float)nr;
  }
}

}  // namespace fvdb
