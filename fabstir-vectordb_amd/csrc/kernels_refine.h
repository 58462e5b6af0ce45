// kernels_refine.h — the re-scoring pass the compressed indexes share (product quantization; SQ8,
// section 9x): one wave per query, the approximate search's candidates scored against f32 or fp16 rows with the shared
// row scorer (score_rows.h: t = a - b; s = s + t * t, ascending, sqrtf last) and the k smallest
// (bits(distance) << 32) | row kept.
#pragma once
#include "common.h"
#include "kernels_scan.h"
#include "score_rows.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace fvdb {

struct RefineArgs {
  const void* rows;          // [row][dpad] of RT: a store's rows, or (local != 0) one decoded row per candidate slot
  const float* queries;      // [B][dpad], zero beyond d
  const uint32_t* cand;      // [B][fk] index rows, the approximate search's answer
  const uint32_t* cand_cnt;  // [B]
  const uint64_t* ids;       // [rows]
  uint32_t dpad, B, fk, k;
  uint64_t* out_ids;
  float* out_dist;
  uint32_t* out_counts;
  uint32_t local;            // 0: candidate c of query q is rows[cand]; else it is rows[q * fk + c] (the key keeps cand)
};

// lane = candidate, 64 a pass (score_rows_wave: rounds of up to 16 rows through the shared scorer)
template <int KR, typename RT>
__device__ __forceinline__ void refine_wave(const RefineArgs& a, uint32_t q, float* tile, int lane) {
  const uint32_t cnt = min(rfl(a.cand_cnt[q]), a.fk);
  WaveTopK<KR> tk;
  tk.init();
  for (uint32_t base = 0; base < cnt; base += 64) {
    const uint32_t nn = min(64u, cnt - base);
    const bool mine = (uint32_t)lane < nn;
    const uint32_t row = mine ? a.cand[(size_t)q * a.fk + base + lane] : 0u;
    const uint32_t src = a.local ? q * a.fk + (mine ? base + (uint32_t)lane : 0u) : row;
    const float dist = score_rows_wave((const RT*)a.rows, a.dpad, a.queries + (size_t)q * a.dpad, src, nn, tile, lane);
    const uint32_t chi = mine ? __float_as_uint(dist) : kInf32;
    if (base == 0) {
      uint32_t shi = chi, slo = mine ? row : kInf32;
      wave_sort64(shi, slo, lane);
      tk.hi[0] = shi;
      tk.lo[0] = slo;
    } else {
      uint32_t th, tl;
      tk.kth(a.k, th, tl);
      offer<KR>(tk, a.k, chi, row, th, tl, lane);
    }
  }
  uint32_t count = 0;
#pragma unroll
  for (int rr = 0; rr < KR; ++rr) {
    const uint32_t e = rr * 64 + lane;
    const bool have = e < a.k && tk.hi[rr] != kInf32;
    count += __popcll(__ballot(have));
    if (e < a.k) {
      a.out_ids[(size_t)q * a.k + e] = have ? a.ids[tk.lo[rr]] : ~0ull;
      a.out_dist[(size_t)q * a.k + e] = have ? __uint_as_float(tk.hi[rr]) : __uint_as_float(0x7F800000u);
    }
  }
  if (lane == 0) a.out_counts[q] = count;
}

}  // namespace fvdb
