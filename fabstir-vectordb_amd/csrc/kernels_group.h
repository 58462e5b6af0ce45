// kernels_group.h — grouped selection: of the n <= 4096 candidates a search of fetch_k returned
// for one query, the first k groups by a key, each with its first group_size members.  No counterpart in the reference;
// the definition is this project's and is exact, per query, over candidates c = 0 .. n-1 (n = min(counts[b], fetch_k))
// in the order given — position order only, the distances are carried and never compared:
//
//   kept[c]   = !distinct || no c' < c has id[c'] == id[c]
//   key[c]    = none when tag[c] is not NULL / BOOL / INT / FLOAT / STRING or id[c] is FVDB_NO_ID, else (tag[c], val[c]);
//               two keys are the same iff both words are equal
//   a kept candidate whose key is none: dropped (missing = DROP), or a group of its own (missing = OWN)
//   groups    ordered by the position of their first member; members = the group's kept candidates in position order
//   output    the first k groups, each with its first group_size members
//
// ONE WORKGROUP per query, state in LDS, nothing quadratic in n:
//   1. ids into an open-addressing table of candidate POSITIONS (a probe compares the ids the positions stand for; the
//      cell of an id ends as the smallest position that carries it: compare-and-swap claims a cell, an atomic min
//      settles it).  kept[c] = the cell of id[c] holds c.  Which cell an id lands in depends on scheduling; what the
//      cell holds after the barrier does not, and only that is read.
//   2. the same table, cleared, over the keys of the kept candidates: first[c] = the smallest kept position with c's key.
//   3. words (first[c] << 32 | c) sorted by the one LDS sort (lds_bitonic_sort_u64): segments are groups, already in
//      group order, and the offset in a segment is the member rank.
//   4. the workgroup scan (block_excl_scan_u) over "first of its segment" in sorted order: the group rank; the first and
//      the last word of segment g leave its bounds in LDS.
//   5. output cell [g][m] is written by the thread that owns the CELL, from word start[g] + m or as a tail: every byte
//      of every output is written exactly once, and no atomic decides where.
#pragma once
#include "common.h"
#include "kernels_wide.h"
#include "wave_ops.h"

namespace fvdb {

constexpr uint32_t kGroupNone = 0xFFFFFFFFu;
constexpr uint32_t kGroupSmallMax = 256;   // candidates of the small instantiation (FVDB_MAX_K), 256 threads
constexpr uint32_t kGroupFullMax = 4096;   // of the full one (FVDB_MAX_K_WIDE), 1024 threads
constexpr uint8_t kGroupDropped = 0xFF;    // s.tag of a candidate `distinct` dropped
enum : uint32_t { kGroupMissingDrop = 0, kGroupMissingOwn = 1 };

// 6 464 bytes (PMAX = 256) / 102 464 bytes (PMAX = 4096) of dynamic LDS
template <uint32_t PMAX>
struct alignas(16) GroupLds {
  uint64_t word[PMAX];     // step 1: the ids; from step 2: the key words
  uint64_t keys[PMAX];     // the sort words
  uint32_t tab[2 * PMAX];  // the table of positions; from step 4: start[PMAX], end[PMAX] of the groups written
  uint8_t tag[PMAX];       // 0: kept, key none; 1..5: kept, the key's tag; kGroupDropped
  uint32_t wave[16];       // the scan's
};

struct GroupArgs {
  const uint64_t* ids;      // [B][fetch_k]
  const float* dist;        // [B][fetch_k]
  const uint32_t* counts;   // [B]
  const uint8_t* key_tag;   // [B][fetch_k]
  const uint64_t* key_val;  // [B][fetch_k]
  uint32_t fetch_k, k, group_size, distinct, missing;
  uint64_t* out_ids;        // [B][k][group_size]
  float* out_dist;
  uint32_t* out_rank;
  uint32_t* out_members;    // [B][k]
  uint32_t* out_total;
  uint8_t* out_key_tag;
  uint64_t* out_key_val;
  uint32_t* out_groups;     // [B]
  uint32_t* out_flags;
};

// the table position a word starts its probe at: the top bits of a 32-bit multiplicative hash (tests/_group_cases.py
// restates it to build keys that share a cell)
__device__ __forceinline__ uint32_t group_hash(uint64_t v, uint32_t tag, uint32_t shift) {
  const uint32_t x = (uint32_t)v ^ ((uint32_t)(v >> 32) * 0x85EBCA6Bu) ^ (tag * 0xC2B2AE35u);
  return (x * 0x9E3779B1u) >> shift;
}

template <bool KEYED, uint32_t PMAX>
__device__ __forceinline__ bool group_same(const GroupLds<PMAX>& s, uint32_t x, uint32_t y) {
  return s.word[x] == s.word[y] && (!KEYED || s.tag[x] == s.tag[y]);
}

// position c enters the table: the cell of its word ends as the smallest position entered with that word
template <bool KEYED, uint32_t PMAX>
__device__ __forceinline__ void group_insert(GroupLds<PMAX>& s, uint32_t c, uint32_t h, uint32_t mask) {
  for (;;) {
    const uint32_t old = atomicCAS(&s.tab[h], kGroupNone, c);
    if (old == kGroupNone) return;
    if (group_same<KEYED>(s, old, c)) {  // old is a position entered before: below n
      atomicMin(&s.tab[h], c);
      return;
    }
    h = (h + 1) & mask;
  }
}

// after the barrier behind the inserts: the smallest position entered with c's word (c was entered: the probe meets its
// cell before an empty one)
template <bool KEYED, uint32_t PMAX>
__device__ __forceinline__ uint32_t group_find(const GroupLds<PMAX>& s, uint32_t c, uint32_t h, uint32_t mask) {
  for (;;) {
    const uint32_t at = s.tab[h];
    if (at == kGroupNone) return c;
    if (group_same<KEYED>(s, at, c)) return at;
    h = (h + 1) & mask;
  }
}

template <uint32_t PMAX, uint32_t T>
__global__ __launch_bounds__(T) void group_select_kernel(const GroupArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_group_raw[];
  GroupLds<PMAX>& s = *reinterpret_cast<GroupLds<PMAX>*>(s_group_raw);
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t qb = (size_t)blockIdx.x;
  const uint32_t n = min(min(a.counts[qb], a.fetch_k), PMAX);  // fetch_k <= PMAX: checked on the host
  const uint64_t* ids = a.ids + qb * a.fetch_k;
  const float* dist = a.dist + qb * a.fetch_k;
  const uint8_t* ktag = a.key_tag + qb * a.fetch_k;
  const uint64_t* kval = a.key_val + qb * a.fetch_k;
  const uint32_t P = n <= 1 ? 1u : 1u << (32 - __clz(n - 1));  // sort width: a power of two, n <= P <= PMAX
  const uint32_t H = 2 * P, mask = H - 1, shift = (uint32_t)__clz(P);  // table of 2 P cells: 32 - log2(H) = clz(P)

  // ---- 1: distinct ----
  for (uint32_t c = tid; c < n; c += T) {
    s.word[c] = ids[c];
    s.tag[c] = 0;
  }
  for (uint32_t h = tid; h < H; h += T) s.tab[h] = kGroupNone;
  __syncthreads();
  if (a.distinct) {  // uniform
    for (uint32_t c = tid; c < n; c += T) group_insert<false>(s, c, group_hash(s.word[c], 0u, shift), mask);
    __syncthreads();
    for (uint32_t c = tid; c < n; c += T)
      if (group_find<false>(s, c, group_hash(s.word[c], 0u, shift), mask) != c) s.tag[c] = kGroupDropped;
    __syncthreads();
    for (uint32_t h = tid; h < H; h += T) s.tab[h] = kGroupNone;
  }
  // ---- 2: keys (thread tid owns the same positions in every loop: it reads its id before the key word replaces it) ----
  for (uint32_t c = tid; c < n; c += T) {
    const uint64_t id = s.word[c];
    const uint32_t tg = ktag[c];
    const bool none = tg < 1u || tg > 5u || id == ~0ull;
    s.word[c] = none ? 0ull : kval[c];
    if (s.tag[c] != kGroupDropped) s.tag[c] = none ? (uint8_t)0 : (uint8_t)tg;
  }
  __syncthreads();
  for (uint32_t c = tid; c < n; c += T) {
    const uint32_t tg = s.tag[c];
    if (tg != 0u && tg != kGroupDropped) group_insert<true>(s, c, group_hash(s.word[c], tg, shift), mask);
  }
  __syncthreads();
  // ---- 3: the sort words ----
  for (uint32_t c = tid; c < P; c += T) {
    uint64_t key = ~0ull;
    if (c < n) {
      const uint32_t tg = s.tag[c];
      if (tg == 0u) {
        if (a.missing == kGroupMissingOwn) key = ((uint64_t)c << 32) | c;
      } else if (tg != kGroupDropped) {
        key = ((uint64_t)group_find<true>(s, c, group_hash(s.word[c], tg, shift), mask) << 32) | c;
      }
    }
    s.keys[c] = key;
  }
  __syncthreads();  // the table is read no more: its words become start[] and end[]
  lds_bitonic_sort_u64(s.keys, P, tid, T);
  // ---- 4: group ranks in sorted order ----
  uint32_t* start = s.tab;
  uint32_t* end = s.tab + PMAX;
  uint32_t base = 0;  // uniform
  for (uint32_t i0 = 0; i0 < P; i0 += T) {
    const uint32_t i = i0 + tid;
    const uint64_t key = i < P ? s.keys[i] : ~0ull;
    const bool valid = key != ~0ull;
    const uint32_t first = (uint32_t)(key >> 32);
    const bool head = valid && (i == 0 || (uint32_t)(s.keys[i - 1] >> 32) != first);
    const bool last = valid && (i + 1 >= P || (uint32_t)(s.keys[i + 1] >> 32) != first);  // a pad's high word is no position
    uint32_t heads;
    const uint32_t before = block_excl_scan_u(head ? 1u : 0u, s.wave, lane, wave, T / 64, heads);
    const uint32_t g = base + before + (head ? 1u : 0u) - 1u;  // valid: a head stands at or before i
    if (head && g < a.k) start[g] = i;                         // g < n <= PMAX
    if (last && g < a.k) end[g] = i + 1;
    base += heads;
    __syncthreads();
  }
  const uint32_t G = min(base, a.k);
  // ---- 5: every output cell once ----
  const uint32_t gs = a.group_size, cells = a.k * gs;  // <= 4096: checked on the host
  const float pinf = __uint_as_float(0x7F800000u);
  for (uint32_t cell = tid; cell < cells; cell += T) {
    const uint32_t g = cell / gs, m = cell - g * gs;
    uint64_t oid = ~0ull;
    float od = pinf;
    uint32_t orank = kGroupNone;
    if (g < G) {
      const uint32_t st = start[g];
      if (m < end[g] - st) {
        orank = (uint32_t)s.keys[st + m];
        oid = ids[orank];
        od = dist[orank];
      }
    }
    a.out_ids[qb * cells + cell] = oid;
    a.out_dist[qb * cells + cell] = od;
    a.out_rank[qb * cells + cell] = orank;
  }
  for (uint32_t g = tid; g < a.k; g += T) {
    uint32_t members = 0, total = 0, tg = 0;
    uint64_t kw = 0;
    if (g < G) {
      const uint32_t st = start[g];
      total = end[g] - st;
      members = min(total, gs);
      const uint32_t c = (uint32_t)s.keys[st];
      tg = s.tag[c];  // 0 (FVDB_META_MISSING) for a group made by missing = OWN
      kw = s.word[c];
    }
    a.out_members[qb * a.k + g] = members;
    a.out_total[qb * a.k + g] = total;
    a.out_key_tag[qb * a.k + g] = (uint8_t)tg;
    a.out_key_val[qb * a.k + g] = kw;
  }
  if (tid == 0) {
    a.out_groups[qb] = G;
    a.out_flags[qb] = n == a.fetch_k ? 1u : 0u;
  }
}

}  // namespace fvdb
