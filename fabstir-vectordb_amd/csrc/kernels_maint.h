// kernels_maint.h — re-partition of an inverted-list pool that never leaves HBM (compact, retrain, add_clusters,
// optimize_clusters; src/ivf/operations.rs:148-260 and :625-645).
//
// All four are one job.  The SEQUENCE ORDER of an index is: lists in ascending cluster id, each list in list-position
// order (what fvdb_ivf_list_export and the chunked save walk).  Every row of the sequence gets a destination list or
// is dropped; rows keep their sequence order inside the destination list; the row moves there in every representation
// the pool keeps.  Stages:
//   seq_map       sequence position -> source slot (block * 64 + lane); for a compact also the destination (own list, or
//                 drop when the live bit is clear)
//   gather        sequence rows -> dense row-major f32 (k-means input, nearest-centroid assignment)
//   rank          destination list per sequence row -> position in that list (stable) and the list totals
//   place         (list, position) -> destination slot; the inverse map "which source slot fills this destination slot"
//   move          one workgroup per DESTINATION block reads its 64 source rows and writes the block whole, tail lanes
//                 zero, so every store is a full 1 KiB wave-instruction whatever the permutation is
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kMaintNone = 0xFFFFFFFFu;  // destination: the row is dropped; inverse map: no source (tail lane)
// The rank kernels keep one 4-byte counter per destination list in LDS: 16384 lists = 64 KiB, two tiles per CU.
// More lists than that are refused by the host code (FVDB_E_UNSUPPORTED).
constexpr uint32_t kRankMaxLists = 16384;
constexpr uint32_t kMovePanel = 32;  // float4 chunks of a row transposed through LDS per pass (64 x 33 x 16 B = 33 KiB)

enum GatherMode : int { GATHER_ROW_MAJOR = 0, GATHER_BLOCKED_F32 = 1, GATHER_BLOCKED_F16 = 2 };

// One thread per (sequence block, lane).  sb_block[s] is the pool block behind the s-th block of the sequence,
// sb_seq0[s] the sequence position of its lane 0 (nsb + 1 entries), sb_list[s] the list it belongs to.
__global__ void seq_map_kernel(const uint32_t* __restrict__ sb_block, const uint32_t* __restrict__ sb_seq0,
                               const uint32_t* __restrict__ sb_list, uint32_t nsb, const uint64_t* __restrict__ valid,
                               uint32_t* __restrict__ seq_slot, uint32_t* __restrict__ dest /* nullable */) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t sb = (uint32_t)(t >> 6), lane = (uint32_t)(t & 63);
  if (sb >= nsb) return;
  const uint32_t s0 = sb_seq0[sb], rows = sb_seq0[sb + 1] - s0;
  if (lane >= rows) return;
  const uint32_t blk = sb_block[sb];
  seq_slot[s0 + lane] = blk * 64 + lane;
  if (dest) dest[s0 + lane] = ((valid[blk] >> lane) & 1) ? sb_list[sb] : kMaintNone;
}

// Sequence rows [0, n) of seq_slot -> out[n][d] f32.  f32 rows are bit copies, fp16 rows are widened exactly.
// `nch` = 16-byte chunks per row (d4 for f32, d8 for fp16).  Row-major source: consecutive threads read consecutive
// chunks of one row.  Blocked source: consecutive threads read the same chunk of consecutive sequence rows, which are
// consecutive lanes of one pool block, so the loads coalesce; the 16- or 32-byte stores land dpad*4 bytes apart and
// leave the merging of lines to L2 (this pass runs once per k-means, which costs thousands of times more).
__global__ void gather_seq_rows_kernel(const void* __restrict__ src, const uint32_t* __restrict__ seq_slot, uint32_t n,
                                       uint32_t d, uint32_t nch, int mode, float* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)n * nch) return;
  uint32_t i, c;
  if (mode == GATHER_ROW_MAJOR) {
    i = (uint32_t)(t / nch);
    c = (uint32_t)(t % nch);
  } else {
    c = (uint32_t)(t / n);
    i = (uint32_t)(t % n);
  }
  const uint32_t s = seq_slot[i];
  float* o = out + (size_t)i * d;
  if (mode == GATHER_BLOCKED_F16) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    const h8 v = ((const h8*)src)[((size_t)(s >> 6) * nch + c) * 64 + (s & 63)];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (8 * c + e < d) o[8 * c + e] = (float)v[e];
    return;
  }
  const float4 v = mode == GATHER_ROW_MAJOR ? ((const float4*)src)[(size_t)s * nch + c]
                                            : ((const float4*)src)[((size_t)(s >> 6) * nch + c) * 64 + (s & 63)];
  if (4 * c + 0 < d) o[4 * c + 0] = v.x;
  if (4 * c + 1 < d) o[4 * c + 1] = v.y;
  if (4 * c + 2 < d) o[4 * c + 2] = v.z;
  if (4 * c + 3 < d) o[4 * c + 3] = v.w;
}

// ids of the sequence rows (the host mirror looks for an id that would enter one list twice)
__global__ void gather_ids_kernel(const uint32_t* __restrict__ seq_slot, const uint64_t* __restrict__ src_ids, uint32_t n,
                                  uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = src_ids[seq_slot[i]];
}

// ---- stable destination ranks -----------------------------------------------------------------------------------
// rank[i] = number of sequence rows before i with the same destination.  The sequence is cut into tiles of T rows:
//   rank_hist    per tile, the count per destination list (LDS histogram, order does not matter for a count)
//   rank_scan    per list, the exclusive prefix of the tile counts in tile order, and the list total
//   rank_assign  per tile ONE wave walks its rows 64 at a time in order, the running counters of the tile in LDS
// Destinations >= nlist (kMaintNone) are dropped rows: not counted, rank kMaintNone.
__global__ __launch_bounds__(256) void rank_hist_kernel(const uint32_t* __restrict__ dest, uint32_t n, uint32_t T,
                                                        uint32_t nlist, uint32_t* __restrict__ tile_hist) {
  extern __shared__ uint32_t lds_cnt[];
  for (uint32_t L = threadIdx.x; L < nlist; L += 256) lds_cnt[L] = 0;
  __syncthreads();
  const uint64_t i0 = (uint64_t)blockIdx.x * T, i1 = i0 + T < n ? i0 + T : n;
  for (uint64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const uint32_t c = dest[i];
    if (c < nlist) atomicAdd(&lds_cnt[c], 1u);
  }
  __syncthreads();
  for (uint32_t L = threadIdx.x; L < nlist; L += 256) tile_hist[(size_t)blockIdx.x * nlist + L] = lds_cnt[L];
}

// in place: tile_hist[t][L] becomes the number of rows for list L in tiles before t
__global__ void rank_scan_kernel(uint32_t* __restrict__ tile_hist, uint32_t tiles, uint32_t nlist,
                                 uint32_t* __restrict__ total) {
  const uint32_t L = blockIdx.x * blockDim.x + threadIdx.x;
  if (L >= nlist) return;
  uint32_t run = 0;
  for (uint32_t t = 0; t < tiles; ++t) {
    const uint32_t v = tile_hist[(size_t)t * nlist + L];
    tile_hist[(size_t)t * nlist + L] = run;
    run += v;
  }
  total[L] = run;
}

__global__ __launch_bounds__(64) void rank_assign_kernel(const uint32_t* __restrict__ dest, uint32_t n, uint32_t T,
                                                         uint32_t nlist, const uint32_t* __restrict__ tile_base,
                                                         uint32_t* __restrict__ rank) {
  extern __shared__ uint32_t lds_cnt[];
  const uint32_t lane = threadIdx.x;
  for (uint32_t L = lane; L < nlist; L += 64) lds_cnt[L] = tile_base[(size_t)blockIdx.x * nlist + L];
  __syncthreads();
  const uint64_t i0 = (uint64_t)blockIdx.x * T, i1 = i0 + T < n ? i0 + T : n;
  for (uint64_t b = i0; b < i1; b += 64) {
    const uint64_t i = b + lane;
    uint32_t c = i < i1 ? dest[i] : kMaintNone;
    if (c >= nlist) c = kMaintNone;
    // among the 64 rows of this step: how many share my destination, how many of them come before me
    uint32_t same = 0, before = 0;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
      const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane((int)c, j);
      same += cj == c;
      before += (cj == c) & ((uint32_t)j < lane);
    }
    const uint32_t base = c != kMaintNone ? lds_cnt[c] : 0;
    __syncthreads();  // every lane has read its counter before the last row of each destination advances it
    if (c != kMaintNone) {
      rank[i] = base + before;
      if (before + 1 == same) lds_cnt[c] = base + same;
    } else if (i < i1) {
      rank[i] = kMaintNone;
    }
    __syncthreads();
  }
}

// (destination list, rank) -> destination slot.  list_block0[L] = first block of list L in the fresh pool (its blocks
// are consecutive), list_row0[L] = rows in the lists before L.  Writes the inverse map src_of_dst (preset to
// kMaintNone), the position of every sequence row (out_pos, kMaintNone = dropped) and the ids of the rows kept, dense
// in the sequence order of the NEW index (what the host mirror rebuilds its id -> position table from).
__global__ void place_rows_kernel(const uint32_t* __restrict__ dest, const uint32_t* __restrict__ rank,
                                  const uint32_t* __restrict__ seq_slot, uint32_t n, uint32_t nlist,
                                  const uint32_t* __restrict__ list_block0, const uint32_t* __restrict__ list_row0,
                                  const uint64_t* __restrict__ src_ids, uint32_t dst_slots, uint32_t rows_out,
                                  uint32_t* __restrict__ src_of_dst, uint32_t* __restrict__ out_pos /* nullable */,
                                  uint64_t* __restrict__ dense_ids /* nullable */) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = dest[i];
  if (c >= nlist) {
    if (out_pos) out_pos[i] = kMaintNone;
    return;
  }
  const uint32_t r = rank[i], s = seq_slot[i];
  const uint64_t slot = (uint64_t)list_block0[c] * 64 + r, row = (uint64_t)list_row0[c] + r;
  if (slot >= dst_slots || row >= rows_out) return;  // cannot happen while rank < total[c]; never write outside
  src_of_dst[slot] = s;
  if (out_pos) out_pos[i] = r;
  if (dense_ids) dense_ids[row] = src_ids[s];
}

// ids, norms and the live bit of destination block `blk`: one wave, lane = destination row.  Norms are copied, not
// recomputed; a soft-deleted row arrives soft-deleted.
__device__ inline void move_row_meta(uint32_t blk, uint32_t lane, uint32_t s, const uint64_t* __restrict__ src_ids,
                                     const float* __restrict__ src_norms, const uint64_t* __restrict__ src_valid,
                                     uint64_t* __restrict__ dst_ids, float* __restrict__ dst_norms,
                                     uint64_t* __restrict__ dst_valid) {
  uint64_t id = 0;
  float nrm = 0.0f;
  bool live = false;
  if (s != kMaintNone) {
    id = src_ids[s];
    nrm = src_norms[s];
    live = (src_valid[s >> 6] >> (s & 63)) & 1;
  }
  dst_ids[(size_t)blk * 64 + lane] = id;
  dst_norms[(size_t)blk * 64 + lane] = nrm;
  const uint64_t word = __ballot(live);
  if (lane == 0) dst_valid[blk] = word;
}

// f32 pool that keeps the row-major copy: a row is dpad*4 contiguous bytes there, in the blocked layout it is d4
// pieces of 16 bytes 1 KiB apart.  So the source is read through `rm` (whole rows, whatever the permutation), written
// to the destination's `rm` as it comes, and transposed through LDS, kMovePanel chunks of all 64 rows per pass, into
// the blocked layout and the fp16 mirror.  The mirror is the round-to-nearest-even image of the f32 row (the same
// conversion scatter_rows_kernel applies), so deriving it here gives the bits a copy would.
__global__ __launch_bounds__(256) void move_rows_rm_kernel(
    const uint32_t* __restrict__ src_of_dst, const float4* __restrict__ src_rm, const uint64_t* __restrict__ src_ids,
    const float* __restrict__ src_norms, const uint64_t* __restrict__ src_valid, uint32_t d4,
    float4* __restrict__ dst_data, float4* __restrict__ dst_rm, void* __restrict__ dst_half,
    uint64_t* __restrict__ dst_ids, float* __restrict__ dst_norms, uint64_t* __restrict__ dst_valid) {
  __shared__ float4 tile[64][kMovePanel + 1];  // + 1: a lane-per-row read of one chunk walks the banks
  __shared__ uint32_t srow[64];
  const uint32_t blk = blockIdx.x, tid = threadIdx.x;
  if (tid < 64) {
    const uint32_t s = src_of_dst[(size_t)blk * 64 + tid];
    srow[tid] = s;
    move_row_meta(blk, tid, s, src_ids, src_norms, src_valid, dst_ids, dst_norms, dst_valid);
  }
  __syncthreads();
  const float4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t p0 = 0; p0 < d4; p0 += kMovePanel) {
    const uint32_t pc = d4 - p0 < kMovePanel ? d4 - p0 : kMovePanel;
    for (uint32_t idx = tid; idx < 64 * pc; idx += 256) {
      const uint32_t row = idx / pc, cc = idx - row * pc;
      const uint32_t s = srow[row];
      const float4 v = s != kMaintNone ? src_rm[(size_t)s * d4 + p0 + cc] : zero;
      dst_rm[((size_t)blk * 64 + row) * d4 + p0 + cc] = v;
      tile[row][cc] = v;
    }
    __syncthreads();
    for (uint32_t idx = tid; idx < 64 * pc; idx += 256) {
      const uint32_t lane = idx & 63, cc = idx >> 6;
      dst_data[((size_t)blk * d4 + p0 + cc) * 64 + lane] = tile[lane][cc];
    }
    if (dst_half) {  // pools with the mirror have d4 % 4 == 0: p0 and pc are even
      typedef _Float16 h8 __attribute__((ext_vector_type(8)));
      for (uint32_t idx = tid; idx < 64 * (pc >> 1); idx += 256) {
        const uint32_t lane = idx & 63, k = idx >> 6;
        const float4 a = tile[lane][2 * k], b = tile[lane][2 * k + 1];
        const h8 hv = {(_Float16)a.x, (_Float16)a.y, (_Float16)a.z, (_Float16)a.w,
                       (_Float16)b.x, (_Float16)b.y, (_Float16)b.z, (_Float16)b.w};
        ((h8*)dst_half)[((size_t)blk * (d4 >> 1) + (p0 >> 1) + k) * 64 + lane] = hv;
      }
    }
    __syncthreads();
  }
}

// Pools without the row-major copy (fp16 rows; f32 rows whose padded d is not a multiple of 16): both are `nch`
// 16-byte chunks per row, [nch][64] per block.  Lane = destination row gathers its chunks from wherever the source
// row sits: 16 useful bytes of every 128-byte line under a random permutation, neighbouring lanes of one line under
// the almost-identity shift of a compact.  Stores are whole 1 KiB wave-instructions either way.
__global__ __launch_bounds__(256) void move_rows_blocked_kernel(
    const uint32_t* __restrict__ src_of_dst, const uint4* __restrict__ src_data, const uint64_t* __restrict__ src_ids,
    const float* __restrict__ src_norms, const uint64_t* __restrict__ src_valid, uint32_t nch,
    uint4* __restrict__ dst_data, uint64_t* __restrict__ dst_ids, float* __restrict__ dst_norms,
    uint64_t* __restrict__ dst_valid) {
  const uint32_t blk = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t s = src_of_dst[(size_t)blk * 64 + lane];
  if (w == 0) move_row_meta(blk, lane, s, src_ids, src_norms, src_valid, dst_ids, dst_norms, dst_valid);
  const uint4 zero = {0u, 0u, 0u, 0u};
  for (uint32_t c = w; c < nch; c += 4) {
    const uint4 v = s != kMaintNone ? src_data[((size_t)(s >> 6) * nch + c) * 64 + (s & 63)] : zero;
    dst_data[((size_t)blk * nch + c) * 64 + lane] = v;
  }
}

// an upper bound stays one: dst = max(dst, src) over float bits of non-negative values
__global__ void max_bits_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && *src > *dst) *dst = *src;
}

}  // namespace fvdb
