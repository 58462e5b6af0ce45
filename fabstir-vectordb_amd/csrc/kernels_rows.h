// kernels_rows.h — rows by location: the gather behind fvdb_ivf_get_rows (get_vector_by_id, src/ivf/core.rs:553-562;
// includeVectors, bindings/node/src/session.rs:266-281) and behind the migration that takes its rows from the graph's
// row store in HBM (fvdb_ivf_assign_from_store / fvdb_ivf_add_assigned_from_store; src/hybrid/core.rs:600-649).
//
// Both kernels give ONE WAVEFRONT to a row (four rows to a 256-thread workgroup) and write it f32, tightly packed with
// stride d: lane l takes the 16-byte chunks l, l + 64, ... of the row, so a row of up to 256 dims (f32) or 512 dims
// (fp16) is one load per lane.  The stores are scalar because out + i * d is 16-byte aligned only when d % 4 == 0;
// consecutive lanes still write consecutive addresses.  Dimensions past d (the padding up to a whole chunk) are never
// written.  Neither is a bandwidth kernel: a row is a few KB and a call moves tens to thousands of them.
//   f32 rows   read from the pool's row-major copy where it exists (consecutive lanes, consecutive 16 bytes), else
//              from the blocked layout [(blk * d4 + c) * 64 + lane] (every chunk of a row in another 1-KiB line)
//   fp16 rows  the blocked layout [(blk * d8 + c) * 64 + lane] of 8 halves is the only copy: the 16-byte chunks of one
//              row sit 1 KiB apart, so the read is strided by the layout itself
#pragma once
#include "common.h"
#include "row_types.h"

namespace fvdb {

constexpr uint32_t kRowsPerGroup = 4;  // wavefronts (rows) per workgroup of the two gathers

// slots[n] (pool block * 64 + lane) -> out[n][d].  ST = 0: f32 rows (nch = d4; `rm` = the row-major copy or nullptr),
// ST = 1: fp16 rows widened exactly (nch = d8).
template <int ST>
__global__ __launch_bounds__(256) void pool_gather_rows_kernel(const void* __restrict__ blocked, const float* __restrict__ rm,
                                                               const uint32_t* __restrict__ slots, uint32_t n, uint32_t d,
                                                               uint32_t nch, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * kRowsPerGroup + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const uint32_t s = slots[i];
  float* o = out + (size_t)i * d;
  if (ST == 1) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    const h8* src = (const h8*)blocked + (size_t)(s >> 6) * nch * 64 + (s & 63);
    for (uint32_t c = lane; c < nch; c += 64) {
      const h8 v = src[(size_t)c * 64];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (8 * c + e < d) o[8 * c + e] = (float)v[e];
    }
    return;
  }
  const float4* src = rm ? (const float4*)rm + (size_t)s * nch : (const float4*)blocked + (size_t)(s >> 6) * nch * 64 + (s & 63);
  const uint32_t step = rm ? 1u : 64u;
  for (uint32_t c = lane; c < nch; c += 64) {
    const float4 v = src[(size_t)c * step];
    if (4 * c + 0 < d) o[4 * c + 0] = v.x;
    if (4 * c + 1 < d) o[4 * c + 1] = v.y;
    if (4 * c + 2 < d) o[4 * c + 2] = v.z;
    if (4 * c + 3 < d) o[4 * c + 3] = v.w;
  }
}

// store rows [row][dpad] (dpad = d rounded up to 4) and rows[n] -> out[n][d]
template <typename RT>
__global__ __launch_bounds__(256) void store_gather_rows_kernel(const RT* __restrict__ data, uint32_t dpad,
                                                                const uint32_t* __restrict__ rows, uint32_t n, uint32_t d,
                                                                float* __restrict__ out) {
  const uint32_t i = blockIdx.x * kRowsPerGroup + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const typename RowVec<RT>::Quad* src = (const typename RowVec<RT>::Quad*)(data + (size_t)rows[i] * dpad);
  float* o = out + (size_t)i * d;
  for (uint32_t c = lane; c < dpad / 4; c += 64) {
    const float4 v = row_widen(src[c]);
    if (4 * c + 0 < d) o[4 * c + 0] = v.x;
    if (4 * c + 1 < d) o[4 * c + 1] = v.y;
    if (4 * c + 2 < d) o[4 * c + 2] = v.z;
    if (4 * c + 3 < d) o[4 * c + 3] = v.w;
  }
}

}  // namespace fvdb
