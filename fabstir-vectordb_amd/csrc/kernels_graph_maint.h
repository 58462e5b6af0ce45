// kernels_graph_maint.h — HNSWIndex::vacuum (src/hnsw/operations.rs:176-200) on the adjacency in HBM: deleted nodes
// leave every neighbour list, and (unless the caller keeps the rows) the node map itself — the survivors are renumbered
// densely IN THEIR OLD ORDER and the row store and every per-node array are compacted.
//
//   gm_count / scan      survivors and the sum of their levels per 256 nodes, exclusive prefix over the workgroups
//   gm_map               node -> new index (kGmNone = dropped), new index -> old node, new upper row -> old upper row,
//                        level and upper-row base of every survivor at its new index
//   gm_owner             (keep-rows form) upper row -> the node it belongs to
//   gm_edges             the stored neighbours before the job, summed
//   gm_prune             one wave per DESTINATION adjacency row: lane i holds neighbour i, a ballot names the survivors,
//                        popcount(ballot & lanes below) is a survivor's new position — a list keeps its survivors in
//                        their old order, which is what remove_if does on the host — the value written is the
//                        neighbour's new index, and its edge distance travels with it.  A row longer than one wave is
//                        walked in chunks of 64 with the count carried, so any stride is served.  The source row may be
//                        the destination row (keep-rows form): a chunk is read whole before any of it is written, and
//                        what is written never lies beyond what was read.
//   gm_move              one wave per destination store row, a chunk per lane (16 bytes of an f32 row, 8 of an fp16 row:
//                        dpad / 4 chunks either way): whole rows, every load and
//                        store a contiguous run; destination <= source, neighbouring waves share nothing
#pragma once
#include "common.h"
#include "wave_ops.h"

namespace fvdb {

constexpr uint32_t kGmNone = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void gm_count_kernel(const uint32_t* __restrict__ deleted, const uint32_t* __restrict__ level, uint32_t n,
                                                       uint32_t* __restrict__ wg_nodes, uint32_t* __restrict__ wg_urows) {
  __shared__ uint32_t s_n[4], s_u[4];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool alive = i < n && deleted[i] == 0u;
  const uint32_t cnt = (uint32_t)__popcll(__ballot(alive));
  const uint32_t lv = wave_sum_u(alive ? level[i] : 0u);
  if ((threadIdx.x & 63) == 0) {
    s_n[threadIdx.x >> 6] = cnt;
    s_u[threadIdx.x >> 6] = lv;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    wg_nodes[blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    wg_urows[blockIdx.x] = s_u[0] + s_u[1] + s_u[2] + s_u[3];
  }
}

// wg_nodes / wg_urows: the exclusive prefixes.  n_out / u_out bound every write (they are the totals of the same scan).
__global__ __launch_bounds__(256) void gm_map_kernel(const uint32_t* __restrict__ deleted, const uint32_t* __restrict__ level,
                                                     const uint32_t* __restrict__ ubase, uint32_t n, const uint32_t* __restrict__ wg_nodes,
                                                     const uint32_t* __restrict__ wg_urows, uint32_t n_out, uint32_t u_out,
                                                     uint32_t* __restrict__ new_index, uint32_t* __restrict__ src_node,
                                                     uint32_t* __restrict__ u_src, uint32_t* __restrict__ dst_level,
                                                     uint32_t* __restrict__ dst_ubase) {
  __shared__ uint32_t s_n[4], s_u[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool alive = i < n && deleted[i] == 0u;
  const uint32_t lv = alive ? level[i] : 0u;
  const uint64_t m = __ballot(alive);
  const uint32_t incl = wave_incl_scan_u(lv, (int)lane);
  if (lane == 63) {
    s_n[wave] = (uint32_t)__popcll(m);
    s_u[wave] = incl;
  }
  __syncthreads();
  uint32_t ni = wg_nodes[blockIdx.x] + ballot_rank(m, lane);
  uint32_t nu = wg_urows[blockIdx.x] + incl - lv;
  for (uint32_t w = 0; w < wave; ++w) {
    ni += s_n[w];
    nu += s_u[w];
  }
  if (i < n) new_index[i] = alive ? ni : kGmNone;
  if (!alive || ni >= n_out) return;
  src_node[ni] = i;
  dst_level[ni] = lv;
  dst_ubase[ni] = nu;
  const uint32_t ub = ubase[i];
  for (uint32_t l = 0; l < lv; ++l)
    if (nu + l < u_out) u_src[nu + l] = ub + l;
}

__global__ __launch_bounds__(256) void gm_owner_kernel(const uint32_t* __restrict__ level, const uint32_t* __restrict__ ubase, uint32_t n,
                                                       uint32_t u_rows, uint32_t* __restrict__ owner) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t lv = level[i], ub = ubase[i];
  for (uint32_t l = 0; l < lv; ++l)
    if (ub + l < u_rows) owner[ub + l] = i;
}

struct GmPrune {
  const uint32_t* src_adj;  // [src_rows][stride]: count, neighbours
  const float* src_dist;    // same indexing
  uint32_t* dst_adj;        // [rows][stride]; may be src_adj (keep-rows form)
  float* dst_dist;
  uint32_t stride, rows, src_rows;
  const uint32_t* src_of_dst;  // [rows] source row of a destination row; nullptr: the same row
  const uint32_t* owner;       // [rows] node a row belongs to; nullptr: row = node (layer 0).  Read when clear_dead.
  uint32_t clear_dead;         // 1 (keep-rows form): the rows of deleted nodes are emptied
  const uint32_t* deleted;     // [n] flags of the OLD numbering
  uint32_t n;
  const uint32_t* new_index;   // [n] old -> new; nullptr: identity
  const uint32_t* src_stamp;   // row stamps travel with their rows (nullptr: stay)
  uint32_t* dst_stamp;
  unsigned long long* counters;  // [1] edges written, [2] deleted nodes whose layer-0 row was emptied ([0]: gm_edges_kernel)
};

// counters[0] += the stored neighbours of `rows` adjacency rows (the job's edges_in)
__global__ __launch_bounds__(256) void gm_edges_kernel(const uint32_t* __restrict__ adj, uint32_t stride, uint32_t rows,
                                                       unsigned long long* __restrict__ counters) {
  unsigned long long sum = 0;
  for (uint32_t r = blockIdx.x * 256 + threadIdx.x; r < rows; r += gridDim.x * 256) sum += adj[(size_t)r * stride];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&counters[0], sum);
}

__global__ __launch_bounds__(256) void gm_prune_kernel(const GmPrune a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t below = (1ull << lane) - 1ull;
  const uint32_t waves = gridDim.x * 4;
  unsigned long long e_out = 0, emptied = 0;
  for (uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6); r < a.rows; r += waves) {
    const uint32_t s = a.src_of_dst ? a.src_of_dst[r] : r;
    if (s >= a.src_rows) continue;  // cannot happen: the map names rows that exist; never read outside
    const uint32_t* in = a.src_adj + (size_t)s * a.stride;
    const float* ind = a.src_dist + (size_t)s * a.stride;
    uint32_t* out = a.dst_adj + (size_t)r * a.stride;
    float* outd = a.dst_dist + (size_t)r * a.stride;
    uint32_t cnt = in[0];
    if (cnt > a.stride - 1) cnt = a.stride - 1;
    bool dead_row = false;
    if (a.clear_dead) {
      const uint32_t node = a.owner ? a.owner[r] : r;
      dead_row = node < a.n && a.deleted[node] != 0u;
    }
    uint32_t kept = 0;
    for (uint32_t base = 0; base < cnt; base += 64) {
      const uint32_t e = base + lane;
      const bool have = e < cnt;
      const uint32_t nb = have ? in[1 + e] : 0u;
      const float dv = have ? ind[1 + e] : 0.0f;
      const bool keep = have && !dead_row && nb < a.n && a.deleted[nb] == 0u;
      const uint64_t m = __ballot(keep);
      if (keep) {
        const uint32_t pos = kept + (uint32_t)__popcll(m & below);
        out[1 + pos] = a.new_index ? a.new_index[nb] : nb;
        outd[1 + pos] = dv;
      }
      kept += (uint32_t)__popcll(m);
    }
    if (lane == 0) {
      out[0] = kept;
      if (a.dst_stamp) a.dst_stamp[r] = a.src_stamp[s];
      e_out += kept;
      emptied += (dead_row && cnt > 0 && !a.owner) ? 1 : 0;  // nodes, not rows: layer 0 only
    }
  }
  if (lane == 0) {
    if (e_out) atomicAdd(&a.counters[1], e_out);
    if (emptied) atomicAdd(&a.counters[2], emptied);
  }
}

// d4 = chunks of a row (dpad / 4); Chunk = four row elements (float4: f32 rows, float2: fp16 rows)
template <typename Chunk>
__global__ __launch_bounds__(256) void gm_move_kernel(const uint32_t* __restrict__ src_node, const Chunk* __restrict__ src, uint32_t src_rows,
                                                      uint32_t d4, uint32_t rows, Chunk* __restrict__ dst) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const uint32_t s = src_node[r];
  if (s >= src_rows) return;  // cannot happen; never read outside
  const Chunk* in = src + (size_t)s * d4;
  Chunk* out = dst + (size_t)r * d4;
  for (uint32_t c = lane; c < d4; c += 64) out[c] = in[c];
}

}  // namespace fvdb
