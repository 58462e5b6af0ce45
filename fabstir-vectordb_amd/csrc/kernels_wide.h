// kernels_wide.h — the list scan for 256 < k <= 4096 (and any smaller k): the same result as kernels_scan.h defines,
// selected another way.  Replaces IVFIndex::search_with_config's list scan, sort and truncate(k)
// (src/ivf/core.rs:626-681) where k outgrows the 64 x 4 register list of WaveTopK.
//
//   score   wide_score_kernel: the work items and the fold of scan_topk_kernel (lane = row, queries through the scalar
//           path), but each row's distance bits go to a per-query arena at the row's scan position `seq` instead of a
//           register list.  Dead rows, masked rows and block padding write kInf32.  The arena index IS the tie-break,
//           so this stage has no atomics and no ordering concern.  In the per-query form (PQ) the live word of a
//           block is the word of the query's own allow-set: one batch, one mask per query.
//   select  wide_select_kernel: one workgroup per query.  Radix select (8-bit digits, LDS histogram) of the k-th
//           smallest distance word — non-negative f32 bits are monotone as u32 — then the rows below the cut and the
//           first rows AT the cut in seq order are gathered as 64-bit keys into LDS, sorted there (bitonic; the keys
//           are unique) and resolved seq -> (probe rank, position) -> pool slot -> id as merge_topk_kernel does.
//           Everything up to the sorted keys is wide_select_keys, which flat_select_kernel (kernels_flat_wide.h) calls
//           too; the sort is lds_bitonic_sort_u64, which also serves kernels_rank.h and kernels_grid.h.
//
//   shards  on an index holding a shard of a larger one the selection is the same and only the keys written out change:
//           their low word becomes the LOGICAL index's seq (wide_gbase_kernel, GLOB_KEYS), unique across ranks, and
//           merge_keys_wide_kernel merges partial lists of up to kWideMaxK such keys.
//
// Arena of a query: 64 words per block of its probed lists, rank after rank; base[q][r] = blocks of the lists ranked
// before r (wide_base_kernel), so arena index == seq.
#pragma once
#include "kernels_scan.h"

#pragma clang fp contract(off)

namespace fvdb {

constexpr uint32_t kWideMaxK = 4096;       // FVDB_MAX_K_WIDE: the survivors' keys fill 32 KB of LDS
constexpr uint32_t kWideSelThreads = 512;  // 8 waves share one query's arena
constexpr uint32_t kWideMaxProbes = 256;   // FVDB_MAX_K: the rank bases of this many probes are staged in LDS

struct WideArgs {
  PoolView pool;
  ListTable lists;
  const uint32_t* probes;  // [B][nprobe] list ids in probe order
  const uint32_t* base;    // [B][nprobe + 1] blocks of earlier-ranked probed lists; [nprobe] = all of them
  const uint32_t* gbase;   // GLOB_KEYS only: [B][nprobe] the same count over the LOGICAL index (wide_gbase_kernel)
  uint32_t* arena;         // [B][stride] distance bits by seq
  uint64_t stride;         // words per query
  uint32_t B, k, nprobe;
  uint64_t* out_ids;       // any of the four may be null
  float* out_dist;
  uint32_t* out_counts;
  uint64_t* out_keys;
};

// base[q][0..np]: exclusive prefix of the block counts of query q's probed lists.  A list that would not fit the
// query's arena (cap_blocks) counts as empty here and is then skipped by the score stage: nothing writes past the end.
__global__ void wide_base_kernel(const uint32_t* __restrict__ probes, const uint32_t* __restrict__ list_off, uint32_t B,
                                 uint32_t np, uint32_t cap_blocks, uint32_t* __restrict__ base) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= B) return;
  uint32_t acc = 0;
  for (uint32_t r = 0; r < np; ++r) {
    base[(size_t)q * (np + 1) + r] = acc;
    const uint32_t L = probes[(size_t)q * np + r];
    const uint32_t nb = L == kInf32 ? 0u : list_off[L + 1] - list_off[L];
    if (nb <= cap_blocks - acc) acc += nb;
  }
  base[(size_t)q * (np + 1) + np] = acc;
}

// gbase[q][0..np): exclusive prefix of the LOGICAL index's block counts of query q's probed lists — the base of
// merge_topk_kernel's seq (kernels_scan.h), which is what makes a key unique across the ranks of a sharded index.
// "No list" entries count as empty, as they do there.
__global__ void wide_gbase_kernel(const uint32_t* __restrict__ probes, const uint32_t* __restrict__ glob_blocks, uint32_t B,
                                  uint32_t np, uint32_t* __restrict__ gbase) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= B) return;
  uint32_t acc = 0;
  for (uint32_t r = 0; r < np; ++r) {
    gbase[(size_t)q * np + r] = acc;
    const uint32_t L = probes[(size_t)q * np + r];
    acc += L == kInf32 ? 0u : glob_blocks[L];
  }
}

// One work item: rows of blocks [b0, b1) of a list against the ne (<= QQ) queries of a group.  The fold is
// scan_item's, statement for statement (kernels_scan.h): the two must round alike.
// PQ: liveness per query.  words[group[q]] are the live words query q sees (a mask's words are valid & allowed already;
// the table's last entry is the pool's own), pool_valid is not read.  The host has checked every group[] entry.
template <int QQ, int ST, bool PQ>
__device__ __forceinline__ void wide_score_item(const void* __restrict__ pool_data, const uint64_t* __restrict__ pool_valid,
                                                const uint64_t* const* __restrict__ words, const uint32_t* __restrict__ group,
                                                const uint32_t d4, const uint32_t* __restrict__ list_blocks,
                                                const u32x2* __restrict__ entries, const float* __restrict__ queries,
                                                const uint32_t dpad, const uint32_t nprobe,
                                                const uint32_t* __restrict__ base, uint32_t* __restrict__ arena,
                                                const uint64_t stride, const uint32_t b_begin, const uint32_t b0,
                                                const uint32_t b1, const uint32_t e0, const uint32_t ne, const int lane) {
  uint32_t qoff[QQ];
#pragma unroll
  for (int j = 0; j < QQ; ++j) qoff[j] = cload(entries + e0 + ((uint32_t)j < ne ? j : 0)).x * dpad;
  // where query j's distances go: lane j keeps (arena word of this list's first row, blocks owned there) and the store
  // below reads them back lane by lane — sixteen wave-uniform 64-bit offsets would not fit the scalar registers
  uint32_t room_l = 0;  // 0: no query j, or its list was left out of the arena
  uint64_t aoff_l = 0;
  const uint64_t* words_l = nullptr;  // PQ: the live words of query j, kept the same way
  if ((uint32_t)lane < ne) {
    const u32x2 e = entries[e0 + lane];
    const uint32_t* bp = base + (size_t)e.x * (nprobe + 1) + e.y;
    room_l = bp[1] - bp[0];
    aoff_l = (uint64_t)e.x * stride + (uint64_t)bp[0] * 64;
    if constexpr (PQ) words_l = words[group[e.x]];
  }

  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t blk = cload(list_blocks + b_begin + b);
    uint64_t word_l = 0;  // PQ: lane j loads its query's word of this block now; the fold hides the latency
    if constexpr (PQ)
      if ((uint32_t)lane < ne) word_l = words_l[blk];
    float acc[QQ];
#pragma unroll
    for (int j = 0; j < QQ; ++j) acc[j] = 0.0f;
    uint32_t c = 0;
    for (; c + 4 <= d4; c += 4) {
      float x[16];
      load_rows16<ST>(pool_data, blk, d4, c, lane, x);
      f32x16 qn = cload16(queries + qoff[0] + 4 * c);
#pragma unroll
      for (int j = 0; j < QQ; ++j) {
        const f32x16 qv = qn;
        if (j + 1 < QQ) qn = cload16(queries + qoff[j + 1] + 4 * c);
        __builtin_amdgcn_sched_barrier(0);
        float t, a = acc[j];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          t = x[i] - qv[i];
          a = a + t * t;
        }
        acc[j] = a;
      }
    }
    if (ST == 0) {
      const float4* xp = (const float4*)pool_data + (size_t)blk * d4 * 64 + lane;
      for (; c < d4; ++c) {
        const float4 xv = xp[(size_t)c * 64];
#pragma unroll
        for (int j = 0; j < QQ; ++j) {
          const f32x4 qv = cload((const f32x4*)(queries + qoff[j] + 4 * c));
          float t;
          t = xv.x - qv.x; acc[j] = acc[j] + t * t;
          t = xv.y - qv.y; acc[j] = acc[j] + t * t;
          t = xv.z - qv.z; acc[j] = acc[j] + t * t;
          t = xv.w - qv.w; acc[j] = acc[j] + t * t;
        }
      }
    }
    uint64_t vmask = 0;
    if constexpr (!PQ) vmask = cload(pool_valid + blk);
    bool live = (vmask >> lane) & 1ull;
#pragma unroll
    for (int j = 0; j < QQ; ++j) {
      const float dist = sqrtf(acc[j]);
      const uint32_t room = rlane(room_l, j);
      const uint64_t aoff = ((uint64_t)rlane((uint32_t)(aoff_l >> 32), j) << 32) | rlane((uint32_t)aoff_l, j);
      if constexpr (PQ) {
        const uint64_t word = ((uint64_t)rlane((uint32_t)(word_l >> 32), j) << 32) | rlane((uint32_t)word_l, j);
        live = (word >> lane) & 1ull;
      }
      if (b < room) arena[aoff + (size_t)b * 64 + lane] = live ? __float_as_uint(dist) : kInf32;
    }
  }
}

// Persistent waves pull (list segment, query group) items from the plan's work queue, as scan_topk_kernel does.
// wide_score_kernel<ST>: one live word per block, the pool's or one mask's for the whole batch (pool_valid).
// wide_score_kernel<ST, WideGroups>: one live word per (block, query) — the per-query form takes the table and the
// group array as one further argument and does not read pool_valid.
struct WideGroups {
  const uint64_t* const* words;  // [G + 1] live words per group; a mask's, or the pool's own for "no filter"
  const uint32_t* group;         // [B] of the sub-batch, every entry <= G (the host checks)
};
template <int ST, class... PerQuery>
__global__ __launch_bounds__(256) void wide_score_kernel(
    const void* __restrict__ pool_data, const uint64_t* __restrict__ pool_valid, const uint32_t d4,
    const uint32_t* __restrict__ list_off, const uint32_t* __restrict__ list_blocks, const uint32_t nlist,
    const uint32_t* __restrict__ entry_off, const uint32_t* __restrict__ item_off, const u32x2* __restrict__ entries,
    const uint32_t* __restrict__ n_items_p, uint32_t* __restrict__ head, const float* __restrict__ queries,
    const uint32_t dpad, const uint32_t segb, const uint32_t nprobe, const uint32_t* __restrict__ base,
    uint32_t* __restrict__ arena, const uint64_t stride, const PerQuery... per_query) {
  static_assert(sizeof...(PerQuery) <= 1, "wide_score_kernel<ST> or wide_score_kernel<ST, WideGroups>");
  constexpr bool PQ = sizeof...(PerQuery) != 0;
  const uint64_t* const* words = nullptr;
  const uint32_t* group = nullptr;
  if constexpr (PQ) {
    const WideGroups g = (per_query, ...);
    words = g.words;
    group = g.group;
  }
  constexpr uint32_t Q = 16;
  const int lane = threadIdx.x & 63;
  const uint32_t n_items = cload(n_items_p);
  for (;;) {
    uint32_t item = 0;
    if (lane == 0) item = atomicAdd(head, 1u);
    item = rfl(item);
    if (item >= n_items) return;

    uint32_t lo = 0, hi = nlist;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (cload(item_off + mid) <= item) lo = mid; else hi = mid;
    }
    const uint32_t L = lo;
    const uint32_t e_begin = cload(entry_off + L);
    const uint32_t cnt = cload(entry_off + L + 1) - e_begin;
    const uint32_t ngroups = (cnt + Q - 1) / Q;
    const uint32_t local = item - cload(item_off + L);
    const uint32_t seg = local / ngroups, g = local - seg * ngroups;
    const uint32_t b_begin = cload(list_off + L);
    const uint32_t nblk = cload(list_off + L + 1) - b_begin;
    const uint32_t b0 = seg * segb;
    const uint32_t b1 = min(b0 + segb, nblk);
    const uint32_t e0 = e_begin + g * Q;
    const uint32_t ne = min(Q, cnt - g * Q);

    if (ne <= 4)
      wide_score_item<4, ST, PQ>(pool_data, pool_valid, words, group, d4, list_blocks, entries, queries, dpad, nprobe, base,
                                 arena, stride, b_begin, b0, b1, e0, ne, lane);
    else if (ne <= 8)
      wide_score_item<8, ST, PQ>(pool_data, pool_valid, words, group, d4, list_blocks, entries, queries, dpad, nprobe, base,
                                 arena, stride, b_begin, b0, b1, e0, ne, lane);
    else
      wide_score_item<16, ST, PQ>(pool_data, pool_valid, words, group, d4, list_blocks, entries, queries, dpad, nprobe, base,
                                  arena, stride, b_begin, b0, b1, e0, ne, lane);
  }
}

// rank r with base[r] <= blk < base[r + 1] (lists of no blocks own no index): the last r with base[r] <= blk
__device__ __forceinline__ uint32_t wide_rank_of(const uint32_t* s_base, uint32_t np, uint32_t blk) {
  uint32_t lo = 0, hi = np;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (s_base[mid] <= blk) lo = mid; else hi = mid;
  }
  return lo;
}

// Bitonic sort, ascending, of the P (a power of two) 64-bit keys in LDS by the T threads of the workgroup, all of which
// call it after a barrier behind the last write of a key; on return the keys are sorted and visible to every thread
// (P == 1: no step and no barrier).  The one sort of the wide selection, rank_sort_kernel (kernels_rank.h) and
// grid_flags_kernel (kernels_grid.h).
__device__ __forceinline__ void lds_bitonic_sort_u64(uint64_t* keys, const uint32_t P, const uint32_t tid, const uint32_t T) {
  for (uint32_t kb = 2; kb <= P; kb <<= 1)
    for (uint32_t j = kb >> 1; j > 0; j >>= 1) {
      for (uint32_t t = tid; t < P / 2; t += T) {
        const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const uint64_t x = keys[lo], y = keys[hi];
        const bool up = (lo & kb) == 0;
        if ((x > y) == up) {
          keys[lo] = y;
          keys[hi] = x;
        }
      }
      __syncthreads();
    }
}

// The LDS of one selection: 33 840 bytes.  16-byte aligned: a lane reads its four histogram bins with one ds_read_b128.
struct alignas(16) WideSelectLds {
  uint64_t keys[kWideMaxK];
  uint32_t hist[256];
  uint32_t wties[kWideSelThreads / 64];
  uint32_t prefix, below, want, taken;
};

// The selection itself, once: the k smallest of the n (a multiple of 64) distance words ar[0, n) as keys (word << 32 |
// index), a word equal to the k-th taken in index order — the tie rule of wide_select_kernel and of flat_select_kernel
// (kernels_flat_wide.h) is this text.  kInf32 words are never taken.  Every thread of a workgroup of kWideSelThreads
// calls it; it owns `s` and asks nothing of its contents.  Returns the number of keys taken (<= k), s.keys[0, count)
// ascending and visible to every thread.
__device__ __forceinline__ uint32_t wide_select_keys(const uint32_t* __restrict__ ar, const uint32_t n, const uint32_t k,
                                                     WideSelectLds& s) {
  constexpr uint32_t T = kWideSelThreads, W = T / 64;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // each wave owns a contiguous run of whole 64-word blocks, in index order
  const uint32_t per = ((n / 64 + W - 1) / W) * 64;
  const uint32_t w0 = min(wave * per, n), w1 = min(w0 + per, n);

  // ---- the k-th smallest word: cut = its value, below = words smaller than it ----
  const uint32_t kk = min(k, n);  // n == 0: nothing to select
  uint32_t cut = 0, below = 0, want = 0;
  if (kk) {
    if (tid == 0) {  // read behind the first barrier of the first pass
      s.prefix = 0;
      s.below = 0;
      s.taken = 0;
      s.want = kk;
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (uint32_t b = tid; b < 256; b += T) s.hist[b] = 0;
      __syncthreads();
      const uint32_t prefix = s.prefix;
      const uint32_t himask = shift == 24 ? 0u : ~0u << (shift + 8);
      for (uint32_t i = w0 + lane; i < w1; i += 64) {  // whole blocks: all 64 lanes run every round
        const uint32_t v = ar[i];
        const bool in = (v & himask) == prefix;
        const uint32_t dg = (v >> shift) & 255u;
        // distances of one query share their leading bits: a wave whose words all fall in one bin adds once
        const uint32_t dg0 = rfl(dg);
        const uint64_t m_in = __ballot(in);
        if (__ballot(in && dg != dg0) == 0) {
          if (lane == 0 && m_in) atomicAdd(&s.hist[dg0], (uint32_t)__popcll(m_in));
        } else if (in) {
          atomicAdd(&s.hist[dg], 1u);
        }
      }
      __syncthreads();
      if (wave == 0) {  // the bin holding the s.want-th word of this round: 4 bins per lane, prefix across lanes
        const uint32_t h0 = s.hist[4 * lane], h1 = s.hist[4 * lane + 1], h2 = s.hist[4 * lane + 2], h3 = s.hist[4 * lane + 3];
        const uint32_t mine = h0 + h1 + h2 + h3;
        const uint32_t inc = wave_incl_scan_u(mine, (int)lane);
        const uint32_t wantr = s.want, exc = inc - mine;
        if (exc < wantr && wantr <= inc) {  // exactly one lane
          uint32_t bin = 4 * lane, acc = exc;
          if (acc + h0 < wantr) { acc += h0; ++bin;
            if (acc + h1 < wantr) { acc += h1; ++bin;
              if (acc + h2 < wantr) { acc += h2; ++bin; } } }
          s.prefix = prefix | (bin << shift);
          s.below += acc;
          s.want = wantr - acc;
        }
      }
      __syncthreads();
    }
    cut = s.prefix;
    below = s.below;
    want = s.want;  // words equal to `cut` still wanted: the first `want` of them in index order
    if (cut == kInf32) want = 0;  // fewer than k live rows: "no row" words are never results
  }

  // ---- words at the cut ahead of each wave ----
  uint32_t ties = 0;
  if (want)
    for (uint32_t i = w0 + lane; i < w1; i += 64) ties += (uint32_t)__popcll(__ballot(ar[i] == cut));
  if (lane == 0) s.wties[wave] = ties;
  __syncthreads();
  uint32_t tie_rank = 0;  // of the first word at the cut in this wave's run
  for (uint32_t w = 0; w < wave; ++w) tie_rank += s.wties[w];

  // ---- gather the survivors as (distance bits << 32 | index) ----
  if (kk)
    for (uint32_t i = w0 + lane; i < w1; i += 64) {
      const uint32_t v = ar[i];
      const uint64_t m_tie = __ballot(v == cut);
      const uint32_t my_tie = tie_rank + ballot_rank(m_tie, lane);
      tie_rank += (uint32_t)__popcll(m_tie);
      uint32_t at = kInf32;
      if (v < cut) at = atomicAdd(&s.taken, 1u);       // slots [0, below): any order, the sort follows
      else if (v == cut && my_tie < want) at = below + my_tie;
      if (at < kWideMaxK) s.keys[at] = ((uint64_t)v << 32) | i;
    }
  const uint32_t count = below + want;  // the selection found at least `want` words at the cut
  uint32_t P = 1;
  while (P < count) P <<= 1;
  __syncthreads();
  for (uint32_t e = count + tid; e < P; e += T) s.keys[e] = ~0ull;
  __syncthreads();
  lds_bitonic_sort_u64(s.keys, P, tid, T);
  return count;
}

// LDS_BASE: the query's rank bases are staged in LDS (nprobe <= kWideMaxProbes); otherwise they are read where
// wide_base_kernel left them — only the binary searches of the <= k winners touch them.
// GLOB_KEYS: a shard of a larger index (fvdb_ivf_search_shard_wide_dev_slot).  Selection is unchanged — by (distance
// bits, local arena index); the lists of other ranks are empty here, so that order restricted to this rank's rows is
// the logical index's order — and only the key written out carries the logical index's seq (a.gbase) in its low word.
template <bool LDS_BASE, bool GLOB_KEYS = false>
__global__ __launch_bounds__(kWideSelThreads) void wide_select_kernel(const WideArgs a) {
  constexpr uint32_t T = kWideSelThreads;
  __shared__ WideSelectLds s_sel;
  __shared__ uint32_t s_base_lds[LDS_BASE ? kWideMaxProbes + 1 : 1];

  const uint32_t tid = threadIdx.x;
  const uint32_t q = blockIdx.x, np = a.nprobe, k = a.k;
  const uint32_t* s_base = a.base + (size_t)q * (np + 1);
  if (LDS_BASE) {
    for (uint32_t r = tid; r <= np; r += T) s_base_lds[r] = a.base[(size_t)q * (np + 1) + r];
    s_base = s_base_lds;
    __syncthreads();
  }
  // the arena words of this query, in seq order: s_base[np] * 64 (dead rows and padding hold kInf32)
  const uint32_t count = wide_select_keys(a.arena + (size_t)q * a.stride, s_base[np] * 64, k, s_sel);
  const uint64_t* s_keys = s_sel.keys;

  // ---- seq -> (rank, position) -> pool slot -> id ----
  for (uint32_t e = tid; e < k; e += T) {
    const bool have = e < count;
    uint64_t key = ~0ull, id = ~0ull;
    if (have) {
      key = s_keys[e];
      const uint32_t seq = (uint32_t)key;
      const uint32_t r = wide_rank_of(s_base, np, seq >> 6);
      const uint32_t L = a.probes[(size_t)q * np + r];
      const uint32_t pos = seq - s_base[r] * 64;
      const uint32_t blk = a.lists.blocks[a.lists.off[L] + (pos >> 6)];
      id = a.pool.ids[(size_t)blk * 64 + (pos & 63)];
      if (GLOB_KEYS) key = (key & 0xFFFFFFFF00000000ull) | (a.gbase[(size_t)q * np + r] * 64u + pos);
    }
    const size_t o = (size_t)q * k + e;
    if (a.out_ids) a.out_ids[o] = id;
    if (a.out_dist) a.out_dist[o] = have ? __uint_as_float((uint32_t)(key >> 32)) : __uint_as_float(0x7F800000u);
    if (a.out_keys) a.out_keys[o] = key;
  }
  if (tid == 0 && a.out_counts) a.out_counts[q] = count;
}

// G-way merge of per-shard (key, id) partial lists of up to kWideMaxK entries each (fvdb_merge_keys_wide_dev): the
// result merge_keys_kernel defines, found without a sort.  Every partial list is ascending with ~0 tails and the keys
// are unique across the lists, so the place of an entry in the merged order is its own index plus, for every other
// list, the number of that list's keys below it (a lower bound).  Entries whose place is below k write themselves
// there; nothing is staged in LDS (G * k keys would be 256 KB at G = 8, k = 4096).  One workgroup per query.
__global__ __launch_bounds__(256) void merge_keys_wide_kernel(const uint64_t* __restrict__ keys,
                                                              const uint64_t* __restrict__ ids, uint32_t G, uint32_t B,
                                                              uint32_t k, uint64_t* __restrict__ out_ids,
                                                              float* __restrict__ out_dist,
                                                              uint32_t* __restrict__ out_counts) {
  __shared__ uint32_t s_valid;
  const uint32_t tid = threadIdx.x, q = blockIdx.x;
  if (tid == 0) s_valid = 0;
  __syncthreads();
  uint32_t valid = 0;
  const uint32_t total = G * k;  // <= 2^31: the host checks
  for (uint32_t t = tid; t < total; t += 256) {
    const uint32_t g = t / k, e = t - g * k;
    const size_t o = ((size_t)g * B + q) * k + e;
    const uint64_t key = keys[o];
    if ((uint32_t)(key >> 32) == kInf32) continue;  // "no result": the tail of a short list
    ++valid;
    uint32_t place = e;
    for (uint32_t g2 = 0; g2 < G && place < k; ++g2) {
      if (g2 == g) continue;
      const uint64_t* __restrict__ other = keys + ((size_t)g2 * B + q) * k;
      uint32_t lo = 0, hi = k;  // first index with other[i] >= key
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (other[mid] < key) lo = mid + 1; else hi = mid;
      }
      place += lo;
    }
    if (place < k) {
      out_ids[(size_t)q * k + place] = ids[o];
      out_dist[(size_t)q * k + place] = __uint_as_float((uint32_t)(key >> 32));
    }
  }
  if (valid) atomicAdd(&s_valid, valid);
  __syncthreads();
  const uint32_t count = min(k, s_valid);
  for (uint32_t e = count + tid; e < k; e += 256) {
    out_ids[(size_t)q * k + e] = ~0ull;
    out_dist[(size_t)q * k + e] = __uint_as_float(0x7F800000u);
  }
  if (tid == 0 && out_counts) out_counts[q] = count;
}

}  // namespace fvdb
