// kernels_rows.h — rows by location: the gather behind fvdb_ivf_get_rows (get_vector_by_id, src/ivf/core.rs:553-562;
// includeVectors, bindings/node/src/session.rs:266-281) and behind the migration that takes its rows from the graph's
// row store in HBM (fvdb_ivf_assign_from_store / fvdb_ivf_add_assigned_from_store; src/hybrid/core.rs:600-649).
//
// Both kernels give ONE WAVEFRONT to a row (four rows to a 256-thread workgroup) and write it f32 at out + i * ostride:
// ostride = d is the tightly packed form of the entry points above; a larger one is the staging block of the diverse
// selection, where dimensions d .. min(ostride, d rounded up to 4) are written as zeros.  A
// location of 0xFFFFFFFF (and a store row past the end) is skipped: its output row is left as it was.  Lane l takes the 16-byte chunks l, l + 64, ... of the row, so a row of up to 256 dims (f32) or 512 dims
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

// slots[n] (pool block * 64 + lane) -> out[n][ostride].  ST = 0: f32 rows (nch = d4; `rm` = the row-major copy or nullptr),
// ST = 1: fp16 rows widened exactly (nch = d8).
template <int ST>
__global__ __launch_bounds__(256) void pool_gather_rows_kernel(const void* __restrict__ blocked, const float* __restrict__ rm,
                                                               const uint32_t* __restrict__ slots, uint32_t n, uint32_t d,
                                                               uint32_t nch, float* __restrict__ out, uint32_t ostride) {
  const uint32_t i = blockIdx.x * kRowsPerGroup + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const uint32_t s = slots[i];
  if (s == 0xFFFFFFFFu) return;
  float* o = out + (size_t)i * ostride;
  const uint32_t dz = min(ostride, (d + 3u) & ~3u);  // zeros from d up to here
  if (ST == 1) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    const h8* src = (const h8*)blocked + (size_t)(s >> 6) * nch * 64 + (s & 63);
    for (uint32_t c = lane; c < nch; c += 64) {
      const h8 v = src[(size_t)c * 64];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (8 * c + e < d) o[8 * c + e] = (float)v[e];
        else if (8 * c + e < dz) o[8 * c + e] = 0.0f;
    }
    return;
  }
  const float4* src = rm ? (const float4*)rm + (size_t)s * nch : (const float4*)blocked + (size_t)(s >> 6) * nch * 64 + (s & 63);
  const uint32_t step = rm ? 1u : 64u;
  for (uint32_t c = lane; c < nch; c += 64) {
    const float4 v = src[(size_t)c * step];
    if (4 * c + 0 < d) o[4 * c + 0] = v.x;
    if (4 * c + 1 < d) o[4 * c + 1] = v.y;
    else if (4 * c + 1 < dz) o[4 * c + 1] = 0.0f;
    if (4 * c + 2 < d) o[4 * c + 2] = v.z;
    else if (4 * c + 2 < dz) o[4 * c + 2] = 0.0f;
    if (4 * c + 3 < d) o[4 * c + 3] = v.w;
    else if (4 * c + 3 < dz) o[4 * c + 3] = 0.0f;
  }
}

// store rows [row][dpad] (dpad = d rounded up to 4) and rows[n] -> out[n][ostride]; nrows: rows the store holds
template <typename RT>
__global__ __launch_bounds__(256) void store_gather_rows_kernel(const RT* __restrict__ data, uint32_t dpad,
                                                                const uint32_t* __restrict__ rows, uint32_t n, uint32_t d,
                                                                float* __restrict__ out, uint32_t ostride, uint32_t nrows) {
  const uint32_t i = blockIdx.x * kRowsPerGroup + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const uint32_t row = rows[i];
  if (row >= nrows) return;  // 0xFFFFFFFF included: the store holds fewer rows than that
  const typename RowVec<RT>::Quad* src = (const typename RowVec<RT>::Quad*)(data + (size_t)row * dpad);
  float* o = out + (size_t)i * ostride;
  const uint32_t dz = min(ostride, dpad);
  for (uint32_t c = lane; c < dpad / 4; c += 64) {
    const float4 v = row_widen(src[c]);
    if (4 * c + 0 < d) o[4 * c + 0] = v.x;
    if (4 * c + 1 < d) o[4 * c + 1] = v.y;
    else if (4 * c + 1 < dz) o[4 * c + 1] = 0.0f;
    if (4 * c + 2 < d) o[4 * c + 2] = v.z;
    else if (4 * c + 2 < dz) o[4 * c + 2] = 0.0f;
    if (4 * c + 3 < d) o[4 * c + 3] = v.w;
    else if (4 * c + 3 < dz) o[4 * c + 3] = 0.0f;
  }
}

}  // namespace fvdb
