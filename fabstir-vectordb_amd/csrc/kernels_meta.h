// kernels_meta.h — metadata filters over typed columns in HBM (include/fvdb.h, "metadata columns").
// One thread per slot runs a postfix program of three-valued leaves (EQUALS, IN, RANGE) and Kleene AND / OR.  The program,
// its constants and the column table are the same for every lane and are read through wave-uniform loads; the per-lane
// stack is two 32-bit words (a "true" bit and an "unknown" bit per entry).  A wave publishes two ballot words, the
// workgroup two counts; after the block scan of both count arrays a write pass places row ids and unknown slots by
// ballot rank, in ascending slot order.
#pragma once
#include "wave_ops.h"

namespace fvdb {

// cell and constant tags (FVDB_META_* of the header).  MISSING is 0: a zero-filled column is MISSING everywhere.
enum : uint32_t {
  kMetaMissing = 0, kMetaNull = 1, kMetaBool = 2, kMetaInt = 3, kMetaFloat = 4, kMetaString = 5, kMetaArray = 6, kMetaComplex = 7,
  kMetaNever = 15,  // constants only: equals no cell (a string the dictionary does not hold, a NaN)
};
enum : uint32_t { kMetaOpEquals = 1, kMetaOpIn = 2, kMetaOpRange = 3, kMetaOpAnd = 4, kMetaOpOr = 5 };
enum : uint32_t { kMetaInHasComplex = 1, kMetaInHasAny = 2 };                                   // IN flags
enum : uint32_t { kMetaHasLo = 1, kMetaLoInc = 2, kMetaHasHi = 4, kMetaHiInc = 8 };             // RANGE flags
enum : uint32_t { kMetaF = 0, kMetaT = 1, kMetaU = 2 };                                         // three-valued result
constexpr uint32_t kMetaStack = 16;      // FVDB_META_MAX_STACK: entries of the per-lane stack (bits of its two words)
constexpr uint32_t kMetaInLinear = 16;   // an IN of at most this many constants is a uniform linear scan, else a binary search

struct MetaColumn {
  const uint8_t* tag;    // [slots]
  const uint64_t* val;   // [slots]; ARRAY: offset (low 32 bits) and length (high 32 bits) into etag / eval
  const uint8_t* etag;   // elements of the column's ARRAY cells
  const uint64_t* eval;
};

struct MetaEvalArgs {
  const uint8_t* present;   // [slots]
  const MetaColumn* cols;
  const uint4* instr;       // x = op | flags << 8, y = column (leaf) or operand count (AND / OR), z = first constant, w = constants
  const uint32_t* ctag;     // constant pool: tag and ordered key (RANGE bounds: the f64's bits)
  const uint64_t* ckey;
  uint64_t* ballots;        // [waves][2]: match, unknown
  uint32_t* cnt_match;      // [workgroups]
  uint32_t* cnt_unknown;    // [workgroups]
  uint32_t slots, n_instr;
};

// The key two values of one tag are compared by: equal keys <=> equal values, and key order = value order, so a sorted
// constant list can be searched.  INT: the int64 biased to unsigned.  FLOAT: -0.0 folded onto 0.0, then the usual
// order-preserving map of the f64's bits; a NaN (nan = true) equals nothing.  BOOL / STRING: the payload.  NULL: 0.
__device__ __forceinline__ uint64_t meta_key(uint32_t tag, uint64_t v, bool& nan) {
  nan = false;
  if (tag == kMetaInt) return v ^ (1ull << 63);
  if (tag == kMetaFloat) {
    if ((v << 1) == 0ull) v = 0ull;
    nan = (v & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
    return (v >> 63) ? ~v : (v | (1ull << 63));
  }
  return (tag == kMetaBool || tag == kMetaString) ? v : 0ull;
}

__device__ __forceinline__ bool meta_scalar_eq(uint32_t tag, uint64_t v, uint32_t ct, uint64_t ck) {
  bool nan;
  const uint64_t key = meta_key(tag, v, nan);
  return tag == ct && key == ck && !nan;
}

// EQUALS against the constant (ct, ck).  A scalar cell is compared; an ARRAY cell is true if any element equals the
// constant (Kleene OR over the elements: a COMPLEX element leaves it unknown unless another element matches).
__device__ __forceinline__ uint32_t meta_leaf_equals(const MetaColumn c, uint32_t tag, uint64_t v, uint32_t ct, uint64_t ck) {
  if (tag == kMetaMissing) return kMetaF;
  if (tag == kMetaComplex) return kMetaU;
  if (tag != kMetaArray) return ct == kMetaComplex ? kMetaU : (meta_scalar_eq(tag, v, ct, ck) ? kMetaT : kMetaF);
  const uint32_t off = (uint32_t)v, len = (uint32_t)(v >> 32);
  if (len == 0) return kMetaF;
  if (ct == kMetaComplex) return kMetaU;
  uint32_t r = kMetaF;
  for (uint32_t e = off; e < off + len; ++e) {  // divergent: one lane per cell
    const uint32_t et = c.etag[e];
    if (et == kMetaComplex) {
      r = kMetaU;
    } else if (meta_scalar_eq(et, c.eval[e], ct, ck)) {
      r = kMetaT;
      break;
    }
  }
  return r;
}

// IN over the sorted, COMPLEX-free constants [first, first + n): the whole value is compared, an ARRAY cell is not
// looked into.
__device__ __forceinline__ uint32_t meta_leaf_in(uint32_t tag, uint64_t v, const uint32_t* __restrict__ ctag,
                                                 const uint64_t* __restrict__ ckey, uint32_t first, uint32_t n, uint32_t flags) {
  const uint32_t open = (flags & kMetaInHasComplex) ? kMetaU : kMetaF;  // what a comparison with a COMPLEX constant leaves
  if (tag == kMetaMissing) return kMetaF;
  if (tag == kMetaComplex) return (flags & kMetaInHasAny) ? kMetaU : kMetaF;
  if (tag == kMetaArray) return open;
  bool nan;
  const uint64_t key = meta_key(tag, v, nan);
  bool found = false;
  if (n <= kMetaInLinear) {
    for (uint32_t i = 0; i < n; ++i) found |= (ctag[first + i] == tag && ckey[first + i] == key);  // uniform loads
  } else {
    uint32_t lo = 0, hi = n;  // divergent: lower bound of (tag, key) by (ctag, ckey)
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      const uint32_t mt = ctag[first + mid];
      const uint64_t mk = ckey[first + mid];
      if (mt < tag || (mt == tag && mk < key)) lo = mid + 1; else hi = mid;
    }
    found = lo < n && ctag[first + lo] == tag && ckey[first + lo] == key;
  }
  return (found && !nan) ? kMetaT : open;
}

// RANGE: an INT cell goes to f64 first (to nearest even), the comparisons are f64; a NaN on either side compares false.
__device__ __forceinline__ uint32_t meta_leaf_range(uint32_t tag, uint64_t v, uint64_t lo_bits, uint64_t hi_bits, uint32_t flags) {
  if (tag == kMetaComplex) return kMetaU;
  if (tag != kMetaInt && tag != kMetaFloat) return kMetaF;
  const double x = tag == kMetaInt ? (double)(long long)v : __longlong_as_double((long long)v);
  const double lo = __longlong_as_double((long long)lo_bits), hi = __longlong_as_double((long long)hi_bits);
  const bool lo_ok = !(flags & kMetaHasLo) || ((flags & kMetaLoInc) ? x >= lo : x > lo);
  const bool hi_ok = !(flags & kMetaHasHi) || ((flags & kMetaHiInc) ? x <= hi : x < hi);
  return (lo_ok && hi_ok) ? kMetaT : kMetaF;
}

__global__ __launch_bounds__(256) void meta_eval_kernel(const MetaEvalArgs a) {
  __shared__ uint32_t s_cnt[8];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
  const bool live = slot < a.slots && a.present[slot] != 0;
  uint32_t st_t = 0, st_u = 0, sp = 0;  // entry i of the stack: bit i of st_t (true) / st_u (unknown), neither = false
  for (uint32_t pc = 0; pc < a.n_instr; ++pc) {
    const uint4 in = a.instr[pc];
    const uint32_t op = in.x & 0xFFu, flags = in.x >> 8;
    uint32_t r;
    if (op == kMetaOpAnd || op == kMetaOpOr) {
      const uint32_t n = in.y;
      const uint32_t mask = ((1u << n) - 1u) << (sp - n);  // n <= 16 <= sp's range: checked on the host
      const uint32_t t = st_t & mask, u = st_u & mask, f = ~(st_t | st_u) & mask;
      r = op == kMetaOpAnd ? (f ? kMetaF : (u ? kMetaU : kMetaT)) : (t ? kMetaT : (u ? kMetaU : kMetaF));
      sp -= n;
    } else {
      const MetaColumn c = a.cols[in.y];
      const uint32_t tag = live ? (uint32_t)c.tag[slot] : (uint32_t)kMetaMissing;  // once per leaf, coalesced
      const uint64_t v = live ? c.val[slot] : 0ull;
      if (op == kMetaOpEquals) r = meta_leaf_equals(c, tag, v, a.ctag[in.z], a.ckey[in.z]);
      else if (op == kMetaOpIn) r = meta_leaf_in(tag, v, a.ctag, a.ckey, in.z, in.w, flags);
      else r = meta_leaf_range(tag, v, a.ckey[in.z], a.ckey[in.z + 1], flags);
    }
    const uint32_t bit = 1u << sp;
    st_t = (st_t & ~bit) | (r == kMetaT ? bit : 0u);
    st_u = (st_u & ~bit) | (r == kMetaU ? bit : 0u);
    sp += 1;
  }
  const uint64_t m = __ballot(live && (st_t & 1u)), u = __ballot(live && (st_u & 1u));
  if (lane == 0) {
    const size_t gw = (size_t)blockIdx.x * 4 + wave;
    a.ballots[2 * gw] = m;
    a.ballots[2 * gw + 1] = u;
    s_cnt[wave] = (uint32_t)__popcll(m);
    s_cnt[4 + wave] = (uint32_t)__popcll(u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.cnt_match[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    a.cnt_unknown[blockIdx.x] = s_cnt[4] + s_cnt[5] + s_cnt[6] + s_cnt[7];
  }
}

// slot i of workgroup b: its row id to out_ids[off_match[b] + rank among the workgroup's matches]; an unknown slot to
// out_unknown[off_unknown[b] + rank among its unknowns], with the number of matches in front of it (where the host
// merges it in) beside it.  The ranks come from the ballots the evaluation left; no atomics.
__global__ __launch_bounds__(256) void meta_write_kernel(const uint64_t* __restrict__ ids, const uint64_t* __restrict__ ballots,
                                                         const uint32_t* __restrict__ off_match, const uint32_t* __restrict__ off_unknown,
                                                         uint64_t* __restrict__ out_ids, uint32_t* __restrict__ out_unknown,
                                                         uint32_t* __restrict__ out_rank) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
  const size_t gw0 = (size_t)blockIdx.x * 4;
  uint32_t base_m = off_match[blockIdx.x], base_u = off_unknown[blockIdx.x];
  for (uint32_t w = 0; w < wave; ++w) {
    base_m += (uint32_t)__popcll(ballots[2 * (gw0 + w)]);
    base_u += (uint32_t)__popcll(ballots[2 * (gw0 + w) + 1]);
  }
  const uint64_t m = ballots[2 * (gw0 + wave)], u = ballots[2 * (gw0 + wave) + 1];  // bits of live slots only
  const uint32_t at = base_m + ballot_rank(m, lane);
  if ((m >> lane) & 1ull) out_ids[at] = ids[slot];
  if ((u >> lane) & 1ull) {
    const uint32_t j = base_u + ballot_rank(u, lane);
    out_unknown[j] = slot;
    out_rank[j] = at;
  }
}

// cell i of the list goes to its slot (slots are distinct and inside the table: checked on the host)
__global__ __launch_bounds__(256) void meta_scatter_cells_kernel(const uint32_t* __restrict__ slots, const uint8_t* __restrict__ tags,
                                                                 const uint64_t* __restrict__ vals, uint64_t n, uint8_t* __restrict__ tag,
                                                                 uint64_t* __restrict__ val) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  tag[slots[i]] = tags[i];
  val[slots[i]] = vals[i];
}

__global__ __launch_bounds__(256) void meta_scatter_bytes_kernel(const uint32_t* __restrict__ slots, const uint8_t* __restrict__ bytes, uint64_t n,
                                                                 uint8_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[slots[i]] = bytes[i];
}

// ---- id -> slot: an open-addressing index in HBM, linear probing, `mask + 1` cells (a power of
// two of at least twice the slots, so a probe always meets an empty cell).  A cell is an id word and a slot word.  The
// empty id word is FVDB_NO_ID: a candidate with that id has no key by definition, so a slot that carries it is never
// entered and never looked up, and every other id, 0 among them, is an ordinary id.
constexpr uint64_t kMetaIndexEmpty = ~0ull;

__device__ __forceinline__ uint32_t meta_index_hash(uint64_t id, uint32_t mask) {
  id ^= id >> 33;
  id *= 0xFF51AFD7ED558CCDull;
  id ^= id >> 33;
  return (uint32_t)id & mask;
}

// both arrays start as all ones.  A 64-bit compare-and-swap claims the id word; an atomic min settles the slot word, so
// of the slots that carry one id the LOWEST wins whatever the order the threads arrive in.
__global__ __launch_bounds__(256) void meta_index_build_kernel(const uint64_t* __restrict__ ids, uint32_t slots, uint64_t* __restrict__ hid,
                                                               uint32_t* __restrict__ hslot, uint32_t mask) {
  const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= slots) return;
  const uint64_t id = ids[slot];
  if (id == kMetaIndexEmpty) return;
  uint32_t h = meta_index_hash(id, mask);
  for (uint32_t step = 0; step <= mask; ++step) {  // slots <= (mask + 1) / 2: ends at a cell of its own long before
    const unsigned long long old = atomicCAS((unsigned long long*)&hid[h], (unsigned long long)kMetaIndexEmpty, (unsigned long long)id);
    if (old == kMetaIndexEmpty || old == id) {
      atomicMin(&hslot[h], slot);
      return;
    }
    h = (h + 1) & mask;
  }
}

// the key of one id by the rule of section 9v: (MISSING, 0) when the id is FVDB_NO_ID, is in no slot, its slot is not
// present, or its cell is MISSING, ARRAY, COMPLEX or a FLOAT NaN; otherwise the cell's tag and its word as stored, a
// FLOAT -0.0 folded onto 0.0, a NULL as 0.  Presence and the cell are read now: only set_rows asks for a rebuild.
__global__ __launch_bounds__(256) void meta_keys_of_ids_kernel(const uint64_t* __restrict__ ids, uint64_t n, const uint64_t* __restrict__ hid,
                                                               const uint32_t* __restrict__ hslot, uint32_t mask, uint32_t slots,
                                                               const uint8_t* __restrict__ present, const uint8_t* __restrict__ ctag,
                                                               const uint64_t* __restrict__ cval, uint8_t* __restrict__ out_tag,
                                                               uint64_t* __restrict__ out_key) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t id = ids[i];
  uint32_t slot = 0xFFFFFFFFu;
  if (id != kMetaIndexEmpty && slots != 0) {
    uint32_t h = meta_index_hash(id, mask);
    for (uint32_t step = 0; step <= mask; ++step) {
      const uint64_t e = hid[h];
      if (e == kMetaIndexEmpty) break;
      if (e == id) {
        slot = hslot[h];
        break;
      }
      h = (h + 1) & mask;
    }
  }
  uint32_t tag = kMetaMissing;
  uint64_t key = 0;
  if (slot < slots && present[slot] != 0) {
    const uint32_t t = ctag[slot];
    uint64_t v = cval[slot];
    if (t == kMetaFloat && (v << 1) == 0ull) v = 0ull;
    const bool nan = t == kMetaFloat && (v & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
    if (t >= kMetaNull && t <= kMetaString && !nan) {
      tag = t;
      key = t == kMetaNull ? 0ull : v;
    }
  }
  out_tag[i] = (uint8_t)tag;
  out_key[i] = key;
}

}  // namespace fvdb
