// wave_ops.h — the cross-lane helpers of one wavefront (64 lanes), and the workgroup scan built on them.  Every kernel
// header takes them from here; the wave helpers touch no LDS, the workgroup scan uses 16 words its caller lends.
#pragma once
#include "common.h"

namespace fvdb {

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t rlane(uint32_t v, uint32_t l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float rlane_f(float v, uint32_t l) {
  return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), l));
}

__device__ __forceinline__ uint32_t dpp_wave_shr1(uint32_t v) {
  // lane i <- lane i-1 (lane 0 <- 0): one VALU op instead of an LDS-crossbar shuffle
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// lane `l` of `old` <- `value` (both wave-uniform): one compare and one select.  (v_writelane_b32 through inline asm cost
// more: the lane select has to travel in M0, the wait states around it are spelled out by hand, and the tied operand made
// the compiler copy the registers of the set around every call — ~100 instructions per admission in the replay loop.)
__device__ __forceinline__ uint32_t writelane_u(uint32_t value, uint32_t l, uint32_t old) {
  const uint32_t me = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  return me == l ? value : old;
}

// wave-wide max / min of a float, result in every lane (DPP row shifts + row broadcasts, no LDS)
__device__ __forceinline__ float wave_max_f(float v) {
  const int ninf = (int)0xFF800000u;
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(v), 0x111, 0xf, 0xf, false)));  // row_shr:1
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(v), 0x112, 0xf, 0xf, false)));  // row_shr:2
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(v), 0x114, 0xf, 0xf, false)));  // row_shr:4
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(v), 0x118, 0xf, 0xf, false)));  // row_shr:8
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(v), 0x142, 0xa, 0xf, false)));  // row_bcast:15
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(ninf, __float_as_int(v), 0x143, 0xc, 0xf, false)));  // row_bcast:31
  return rlane_f(v, 63);
}
__device__ __forceinline__ float wave_min_f(float v) {
  const int pinf = (int)0x7F800000u;
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(pinf, __float_as_int(v), 0x111, 0xf, 0xf, false)));
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(pinf, __float_as_int(v), 0x112, 0xf, 0xf, false)));
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(pinf, __float_as_int(v), 0x114, 0xf, 0xf, false)));
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(pinf, __float_as_int(v), 0x118, 0xf, 0xf, false)));
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(pinf, __float_as_int(v), 0x142, 0xa, 0xf, false)));
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(pinf, __float_as_int(v), 0x143, 0xc, 0xf, false)));
  return rlane_f(v, 63);
}

// the same on unsigned values (zero fill: max's identity; min = ~max(~v))
__device__ __forceinline__ uint32_t wave_max_u(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ uint32_t wave_min_u(uint32_t v) { return ~wave_max_u(~v); }

// sum over the wave, result in every lane (xor butterfly)
__device__ __forceinline__ uint32_t wave_sum_u(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// inclusive prefix sum over the wave: lane i gets v_0 + ... + v_i
__device__ __forceinline__ uint32_t wave_incl_scan_u(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(v, o);
    if (lane >= o) v += up;
  }
  return v;
}

// set bits of a ballot below this lane: the lane's rank among the lanes that voted
__device__ __forceinline__ uint32_t ballot_rank(uint64_t m, uint32_t lane) { return (uint32_t)__popcll(m & ((1ull << lane) - 1ull)); }

// The workgroup scan, once: the sum of the x of every thread before this one, and the workgroup's sum in `total`.  Every
// thread of a workgroup of `waves` whole waves (at most 16) calls it; s_wave is 16 words of LDS the caller lends, free
// again after the caller's next barrier.  One barrier inside.
__device__ __forceinline__ uint32_t block_excl_scan_u(uint32_t x, uint32_t* s_wave, uint32_t lane, uint32_t wave, uint32_t waves,
                                                      uint32_t& total) {
  const uint32_t incl = wave_incl_scan_u(x, (int)lane);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t w = 0; w < waves; ++w) {
    const uint32_t cw = s_wave[w];
    before += w < wave ? cw : 0u;
    all += cw;
  }
  total = all;
  return before + incl - x;
}

// exclusive prefix sum of v[0 .. m) in place, the total into *total; one workgroup of 1024
template <typename Total>
__global__ __launch_bounds__(1024) void block_excl_scan_kernel(uint32_t* __restrict__ v, uint32_t m, Total* __restrict__ total) {
  __shared__ uint32_t s_wave[16];
  uint32_t base = 0;  // uniform: every thread adds the same chunk totals
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t c0 = 0; c0 < m; c0 += 1024) {
    const uint32_t i = c0 + threadIdx.x;
    const uint32_t x = i < m ? v[i] : 0u;
    uint32_t chunk;
    const uint32_t before = block_excl_scan_u(x, s_wave, lane, wave, 16u, chunk);
    if (i < m) v[i] = base + before;
    base += chunk;
    __syncthreads();  // s_wave is written again by the next chunk
  }
  if (threadIdx.x == 0) *total = base;
}

}  // namespace fvdb
