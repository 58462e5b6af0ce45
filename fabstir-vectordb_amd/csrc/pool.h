// pool.h — a pool of 64-row blocks in HBM (layout: common.h PoolView) and the one routine that allocates its buffers.
// Host-only code.
#pragma once
#include "common.h"
#include "fvdb_internal.h"

struct Pool {
  enum Buf { DATA = 0, RM, HALF, NORMS, IDS, VALID, kBufs };  // in the order they are allocated
  uint32_t d4 = 0;      // 4-dim chunks per row (of the padded dimension)
  uint32_t esize = 4;   // bytes per stored element: 4 = f32, 2 = fp16
  uint32_t cap_blocks = 0, used_blocks = 0;
  bool mirror = false;  // f32 pools: keep an fp16 (round-to-nearest) copy of the rows for the matrix-core filter
  DBuf buf[kBufs];
  void* data() const { return buf[DATA].p; }
  uint64_t* ids() const { return buf[IDS].as<uint64_t>(); }
  uint64_t* valid() const { return buf[VALID].as<uint64_t>(); }
  float* norms() const { return buf[NORMS].as<float>(); }  // |x|^2 per row (matrix-core filter, kernels_mfma.h)
  void* half() const { return buf[HALF].p; }               // [blocks][d8][64] 8-half chunks, same lane = row layout
  // f32 pools with the mirror also keep the rows ROW-MAJOR ([blocks * 64][dpad] f32, bit copies): the select stage
  // scores some twenty single rows per query, and in the blocked layout every 16 bytes of a row sit in a different
  // cache line (12 KB fetched per 1.5 KB row)
  float* rm() const { return buf[RM].as<float>(); }
  size_t block_bytes() const { return (size_t)d4 * 4 * esize * 64; }
  // bytes of one block in buffer b; 0: a pool of this shape does not keep it
  size_t bytes_per_block(int b) const {
    switch (b) {
      case DATA: return block_bytes();
      case RM: return mirror && esize == 4 ? block_bytes() : 0;
      case HALF: return mirror ? block_bytes() / 2 : 0;
      case NORMS: return 64 * sizeof(float);
      case IDS: return 64 * sizeof(uint64_t);
      default: return sizeof(uint64_t);
    }
  }
  fvdb::PoolView view() const { return fvdb::PoolView{data(), ids(), valid(), d4}; }
  int reserve(fvdb_ctx* ctx, uint32_t blocks);
};
static_assert(!std::is_copy_constructible<Pool>::value && std::is_nothrow_move_constructible<Pool>::value, "Pool is move-only");

// A full set of buffers for `blocks` blocks, shaped like `like`: all of them or none.  With `carry` the set is what
// `like` grows into: cleared, its used blocks copied over (stream-ordered: synchronise before it takes like's place).
// Without, nothing is cleared and every block counts as used: the caller writes all 64 lanes of each.
inline hipError_t pool_buffers(const Pool& like, uint32_t blocks, bool carry, hipStream_t st, Pool* out) {
  Pool p;
  p.d4 = like.d4;
  p.esize = like.esize;
  p.mirror = like.mirror;
  p.cap_blocks = blocks;
  p.used_blocks = carry ? like.used_blocks : blocks;
  const size_t used = carry ? like.used_blocks : 0;
  auto copy_used = [&](int b) {
    return hipMemcpyAsync(p.buf[b].p, like.buf[b].p, used * p.bytes_per_block(b), hipMemcpyDeviceToDevice, st);
  };
  hipError_t e = hipSuccess;
  for (int b = 0; b < Pool::kBufs && e == hipSuccess; ++b) {
    const size_t bytes = (size_t)blocks * p.bytes_per_block(b);
    if (!bytes) continue;
    e = p.buf[b].exact(bytes);
    // rows never written (the tail of each list's last block) must be finite: they share MFMA instructions with
    // live rows, and 0 x NaN would poison those.  The ids of such rows are never read.
    if (e == hipSuccess && carry && b != Pool::IDS) e = hipMemsetAsync(p.buf[b].p, 0, bytes, st);
    if (e == hipSuccess && used && (b == Pool::RM || b == Pool::HALF) && like.buf[b].p) e = copy_used(b);
  }
  for (int b : {Pool::DATA, Pool::IDS, Pool::VALID, Pool::NORMS})
    if (e == hipSuccess && used) e = copy_used(b);
  if (e == hipSuccess) *out = std::move(p);
  return e;
}

// grow to at least `blocks` capacity, preserving contents
inline int Pool::reserve(fvdb_ctx* ctx, uint32_t blocks) {
  if (blocks <= cap_blocks) return FVDB_OK;
  const uint32_t ncap = std::max<uint32_t>(blocks, cap_blocks + cap_blocks / 2 + 16);
  Pool grown;
  HIPCHK(ctx, pool_buffers(*this, ncap, true, ctx->stream, &grown));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *this = std::move(grown);
  return FVDB_OK;
}
