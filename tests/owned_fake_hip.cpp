// owned_fake_hip.cpp — the engine's scoped owners (csrc/dev_owned.h) and the pool's buffer set (csrc/pool.h) against a
// fake HIP runtime defined here: it keeps the set of live handles, aborts on a free of something not live, records the
// sizes requested, and fails the n-th call of a chosen kind on demand.  Stand-alone: built with the host compiler,
// not linked against the HIP runtime (tests/test_owned_buffers.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../fabstir-vectordb_amd/csrc/pool.h"

#define REQUIRE(cond)                                                      \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: REQUIRE(%s)\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// ---- the fake runtime ------------------------------------------------------------------------------------------------
namespace fake {
enum Kind { MALLOC, HOST_MALLOC, EVENT, STREAM, MEMSET, MEMCPY, SYNC, KINDS };
struct Op {
  char what;  // 'M' device alloc, 'H' pinned alloc, 'F' device free, 'G' pinned free
  size_t bytes;
  void* p;
};
std::set<void*> live;
std::vector<Op> ops;      // allocations and frees, in order
int fail_in[KINDS] = {};  // n > 0: the n-th call of this kind from now on fails
int calls[KINDS] = {};
hipError_t sticky = hipSuccess;

bool trip(Kind k) {
  calls[k] += 1;
  return fail_in[k] > 0 && --fail_in[k] == 0;
}
void fail_nth(Kind k, int n) { fail_in[k] = n; }
void reset() {
  ops.clear();
  std::memset(fail_in, 0, sizeof fail_in);
  std::memset(calls, 0, sizeof calls);
}
hipError_t alloc(Kind k, char what, void** p, size_t bytes) {
  if (trip(k)) {
    *p = (void*)0x1;  // a failing call may leave rubbish behind: the owners must not keep it
    return sticky = hipErrorOutOfMemory;
  }
  *p = std::malloc(bytes ? bytes : 1);
  std::memset(*p, 0xAB, bytes);
  live.insert(*p);
  ops.push_back({what, bytes, *p});
  return hipSuccess;
}
hipError_t release(char what, void* p) {
  if (!p) return hipSuccess;
  if (!live.erase(p)) {
    std::fprintf(stderr, "free of %p, which is not live\n", p);
    std::abort();
  }
  ops.push_back({what, 0, p});
  std::free(p);
  return hipSuccess;
}
template <typename H>
hipError_t make_handle(Kind k, H* out) {
  if (trip(k)) {
    *out = (H)0x1;
    return hipErrorOutOfMemory;
  }
  void* p = std::malloc(1);
  live.insert(p);
  *out = (H)p;
  return hipSuccess;
}
std::vector<size_t> sizes(char what) {
  std::vector<size_t> v;
  for (const Op& o : ops)
    if (o.what == what) v.push_back(o.bytes);
  return v;
}
}  // namespace fake

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return fake::alloc(fake::MALLOC, 'M', p, bytes); }
hipError_t hipFree(void* p) { return fake::release('F', p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return fake::alloc(fake::HOST_MALLOC, 'H', p, bytes); }
hipError_t hipHostFree(void* p) { return fake::release('G', p); }
hipError_t hipEventCreate(hipEvent_t* e) { return fake::make_handle(fake::EVENT, e); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return fake::make_handle(fake::EVENT, e); }
hipError_t hipEventDestroy(hipEvent_t e) { return fake::release('e', (void*)e); }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { return fake::live.count((void*)e) ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipEventSynchronize(hipEvent_t e) { return fake::live.count((void*)e) ? hipSuccess : hipErrorInvalidHandle; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  if (!fake::live.count((void*)a) || !fake::live.count((void*)b)) return hipErrorInvalidHandle;
  *ms = 1.5f;
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { return fake::make_handle(fake::STREAM, s); }
hipError_t hipStreamDestroy(hipStream_t s) { return fake::release('s', (void*)s); }
hipError_t hipStreamSynchronize(hipStream_t) { return fake::trip(fake::SYNC) ? hipErrorUnknown : hipSuccess; }
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) {
  if (fake::trip(fake::MEMSET)) return hipErrorUnknown;
  std::memset(dst, value, bytes);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
  if (fake::trip(fake::MEMCPY)) return hipErrorUnknown;
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipGetLastError(void) {
  const hipError_t e = fake::sticky;
  fake::sticky = hipSuccess;
  return e;
}
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake error"; }
}

// ---- 1. scope exit, move, swap ---------------------------------------------------------------------------------------
template <typename Buf>
void scope_exit_case(char alloc_op, char free_op) {
  fake::reset();
  const std::set<void*> before = fake::live;
  {
    Buf a, b;
    REQUIRE(a.exact(100) == hipSuccess && b.exact(200) == hipSuccess);
    void *pa = a.p, *pb = b.p;
    REQUIRE(fake::live.size() == before.size() + 2);
    Buf c(std::move(a));  // the source of a move is empty and frees nothing
    REQUIRE(a.p == nullptr && a.cap == 0 && c.p == pa && c.cap == 100);
    std::swap(b, c);      // swap frees nothing
    REQUIRE(b.p == pa && b.cap == 100 && c.p == pb && c.cap == 200);
    REQUIRE(fake::live.size() == before.size() + 2);
    b = std::move(c);     // move-assignment onto a non-empty owner frees the block it held, not the one it takes
    REQUIRE(b.p == pb && c.p == nullptr && !fake::live.count(pa) && fake::live.count(pb));
    Buf& self = b;
    b = std::move(self);  // self-move is harmless
    REQUIRE(b.p == pb && b.cap == 200 && fake::live.count(pb));
    b.release();
    b.release();          // an explicit early release, then nothing more to free
    REQUIRE(b.p == nullptr && b.cap == 0 && fake::live == before);
    REQUIRE(a.exact(64) == hipSuccess);  // left to the destructor
  }
  REQUIRE(fake::live == before);
  size_t allocs = 0, frees = 0;
  for (const fake::Op& o : fake::ops) {
    allocs += o.what == alloc_op;
    frees += o.what == free_op;
  }
  REQUIRE(allocs == 3 && frees == 3);  // each block exactly once
}

// ---- 2. ensure / exact ------------------------------------------------------------------------------------------------
template <typename Buf>
void ensure_case(fake::Kind kind, char alloc_op, char free_op, size_t floor) {
  fake::reset();
  const std::set<void*> before = fake::live;
  {
    Buf b;
    REQUIRE(b.ensure(1) == hipSuccess && b.cap == floor);  // the floor
    REQUIRE(b.ensure(floor) == hipSuccess && fake::calls[kind] == 1);  // fits: no call
    void* first = b.p;
    REQUIRE(b.ensure(10000) == hipSuccess && b.cap == 12500);  // bytes + bytes / 4
    REQUIRE(b.ensure(12500) == hipSuccess && b.ensure(0) == hipSuccess && fake::calls[kind] == 2);
    REQUIRE((fake::sizes(alloc_op) == std::vector<size_t>{floor, 12500}));
    // the old block went before the new one was asked for
    REQUIRE(fake::ops.size() == 3 && fake::ops[1].what == free_op && fake::ops[1].p == first && fake::ops[2].what == alloc_op);
    fake::fail_nth(kind, 1);
    REQUIRE(b.ensure(20000) == hipErrorOutOfMemory);  // the error comes back, the owner is empty
    REQUIRE(b.p == nullptr && b.cap == 0 && fake::live == before);
    REQUIRE(hipGetLastError() == hipSuccess);  // and is not left for the next launch check to find
    REQUIRE(b.exact(777) == hipSuccess && b.cap == 777 && fake::sizes(alloc_op).back() == 777);  // exactly that size
    REQUIRE(b.exact(5) == hipSuccess && b.cap == 5 && fake::sizes(alloc_op).back() == 5);
    fake::fail_nth(kind, 1);
    REQUIRE(b.exact(9) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0);
  }
  REQUIRE(fake::live == before);
}

// ---- 3. growth that keeps contents ------------------------------------------------------------------------------------
void grow_case() {
  fake::reset();
  const std::set<void*> before = fake::live;
  {
    DBuf b;
    REQUIRE(b.exact(64) == hipSuccess);
    for (int i = 0; i < 64; ++i) b.as<unsigned char>()[i] = (unsigned char)i;
    const std::set<void*> with_b = fake::live;
    void* old = b.p;
    const fake::Kind steps[] = {fake::MALLOC, fake::MEMCPY, fake::MEMSET, fake::SYNC};
    for (fake::Kind k : steps) {  // the allocation, the copy, the memset, the synchronise failing in turn
      fake::fail_nth(k, 1);
      REQUIRE(grow_keeping(b, 256, 48, /*zero_rest=*/true, nullptr) != hipSuccess);
      REQUIRE(fake::live == with_b && b.p == old && b.cap == 64);
      REQUIRE(fake::fail_in[k] == 0);  // (the failure was really reached)
    }
    REQUIRE(grow_keeping(b, 256, 48, /*zero_rest=*/true, nullptr) == hipSuccess);
    REQUIRE(b.p != old && b.cap == 256 && !fake::live.count(old) && fake::live.size() == with_b.size());
    for (int i = 0; i < 256; ++i) REQUIRE(b.as<unsigned char>()[i] == (i < 48 ? i : 0));
    const int memsets = fake::calls[fake::MEMSET];
    REQUIRE(grow_keeping(b, 512, 256, /*zero_rest=*/false, nullptr) == hipSuccess);  // the store's growth: nothing zeroed
    REQUIRE(b.cap == 512 && fake::calls[fake::MEMSET] == memsets);
    for (int i = 0; i < 256; ++i) REQUIRE(b.as<unsigned char>()[i] == (i < 48 ? i : 0));
    DBuf empty;
    REQUIRE(grow_keeping(empty, 32, 0, true, nullptr) == hipSuccess && empty.cap == 32);  // from nothing: no copy
    for (int i = 0; i < 32; ++i) REQUIRE(empty.as<unsigned char>()[i] == 0);
  }
  REQUIRE(fake::live == before);
}

// ---- 4. the pool's set ------------------------------------------------------------------------------------------------
struct Shape {
  const char* name;
  uint32_t esize;
  bool mirror;
  int n_bufs;
};

std::vector<size_t> pool_sizes(const Shape& sh, uint32_t d4, size_t blocks) {
  const size_t bb = (size_t)d4 * 4 * sh.esize * 64;
  std::vector<size_t> v{blocks * bb};                      // data
  if (sh.mirror && sh.esize == 4) v.push_back(blocks * bb);  // rm
  if (sh.mirror) v.push_back(blocks * bb / 2);             // half
  v.push_back(blocks * 64 * sizeof(float));                // norms
  v.push_back(blocks * 64 * sizeof(uint64_t));             // ids
  v.push_back(blocks * sizeof(uint64_t));                  // valid
  return v;
}

std::vector<void*> pool_ptrs(const Pool& p) {
  std::vector<void*> v;
  for (const DBuf& b : p.buf) v.push_back(b.p);
  return v;
}

void pool_case(const Shape& sh) {
  const uint32_t d4 = 4, blocks = 3;
  fvdb_ctx ctx;
  const std::set<void*> before = fake::live;
  {
    Pool like;
    like.d4 = d4;
    like.esize = sh.esize;
    like.mirror = sh.mirror;
    // a fresh set of exactly 3 blocks (the re-partition's): all or none
    for (int i = 1; i <= sh.n_bufs; ++i) {
      fake::reset();
      fake::fail_nth(fake::MALLOC, i);
      Pool out;
      REQUIRE(pool_buffers(like, blocks, /*carry=*/false, nullptr, &out) == hipErrorOutOfMemory);
      REQUIRE(fake::live == before && out.cap_blocks == 0 && out.data() == nullptr);
      REQUIRE(fake::calls[fake::MALLOC] == i);
    }
    fake::reset();
    Pool pool;
    REQUIRE(pool_buffers(like, blocks, /*carry=*/false, nullptr, &pool) == hipSuccess);
    REQUIRE(fake::sizes('M') == pool_sizes(sh, d4, blocks));
    REQUIRE(pool.cap_blocks == blocks && pool.used_blocks == blocks && pool.d4 == d4 && pool.esize == sh.esize && pool.mirror == sh.mirror);
    REQUIRE(fake::calls[fake::MEMSET] == 0 && fake::calls[fake::MEMCPY] == 0);  // nothing is cleared, nothing copied
    REQUIRE((pool.rm() != nullptr) == (sh.mirror && sh.esize == 4) && (pool.half() != nullptr) == sh.mirror);
    REQUIRE(fake::live.size() == before.size() + (size_t)sh.n_bufs);
    // growth: the 3 used blocks carried over into max(blocks, cap + cap / 2 + 16) = 20
    const size_t bb = pool.block_bytes();
    std::memset(pool.data(), 0x11, blocks * bb);
    std::memset(pool.ids(), 0x22, blocks * 512);
    std::memset(pool.valid(), 0x33, blocks * 8);
    std::memset(pool.norms(), 0x44, blocks * 256);
    if (pool.rm()) std::memset(pool.rm(), 0x55, blocks * bb);
    if (pool.half()) std::memset(pool.half(), 0x66, blocks * bb / 2);
    const std::set<void*> with_pool = fake::live;
    const std::vector<void*> old = pool_ptrs(pool);
    for (int i = 1; i <= sh.n_bufs; ++i) {
      fake::reset();
      fake::fail_nth(fake::MALLOC, i);
      REQUIRE(pool.reserve(&ctx, blocks + 1) == FVDB_E_OOM);
      REQUIRE(fake::live == with_pool && pool_ptrs(pool) == old && pool.cap_blocks == blocks && pool.used_blocks == blocks);
      REQUIRE(fake::calls[fake::MALLOC] == i);
    }
    for (fake::Kind k : {fake::MEMSET, fake::MEMCPY, fake::SYNC}) {  // a HIP error behind the allocations
      fake::reset();
      fake::fail_nth(k, k == fake::SYNC ? 1 : 2);
      REQUIRE(pool.reserve(&ctx, blocks + 1) == FVDB_E_HIP);
      REQUIRE(fake::live == with_pool && pool_ptrs(pool) == old && pool.cap_blocks == blocks);
    }
    fake::reset();
    REQUIRE(pool.reserve(&ctx, blocks) == FVDB_OK && fake::calls[fake::MALLOC] == 0);  // fits: nothing happens
    REQUIRE(pool.reserve(&ctx, blocks + 1) == FVDB_OK);
    REQUIRE(fake::sizes('M') == pool_sizes(sh, d4, 20));
    REQUIRE(pool.cap_blocks == 20 && pool.used_blocks == blocks && fake::live.size() == with_pool.size());
    REQUIRE(fake::calls[fake::SYNC] == 1);  // the single synchronise before the swap
    REQUIRE(fake::calls[fake::MEMSET] == sh.n_bufs - 1 && fake::calls[fake::MEMCPY] == sh.n_bufs);  // ids are not cleared
    for (void* p : old) REQUIRE(!p || !fake::live.count(p));
    auto kept = [&](const void* p, int byte, size_t used, size_t all, bool cleared) {
      const unsigned char* c = (const unsigned char*)p;
      for (size_t i = 0; i < used; ++i) REQUIRE(c[i] == byte);
      for (size_t i = used; cleared && i < all; ++i) REQUIRE(c[i] == 0);  // tail rows must be finite
    };
    kept(pool.data(), 0x11, blocks * bb, 20 * bb, true);
    kept(pool.ids(), 0x22, blocks * 512, 20 * 512, false);
    kept(pool.valid(), 0x33, blocks * 8, 20 * 8, true);
    kept(pool.norms(), 0x44, blocks * 256, 20 * 256, true);
    if (pool.rm()) kept(pool.rm(), 0x55, blocks * bb, 20 * bb, true);
    if (pool.half()) kept(pool.half(), 0x66, blocks * bb / 2, 20 * bb / 2, true);
    Pool moved = std::move(pool);  // a move leaves the source without buffers
    REQUIRE(pool.data() == nullptr && moved.cap_blocks == 20 && fake::live.size() == with_pool.size());
  }
  REQUIRE(fake::live == before);
}

// ---- 5. events, streams, the stage timer ------------------------------------------------------------------------------
void handle_case() {
  fake::reset();
  const std::set<void*> before = fake::live;
  {
    DevEvent e, f;
    REQUIRE(e.create() == hipSuccess && f.create(hipEventDisableTiming) == hipSuccess);
    hipEvent_t he = e;
    REQUIRE(e.create() == hipSuccess && (hipEvent_t)e == he && fake::calls[fake::EVENT] == 2);  // exists already
    DevEvent g(std::move(e));
    REQUIRE((hipEvent_t)e == nullptr && (hipEvent_t)g == he);
    f = std::move(g);  // the event f held is destroyed
    REQUIRE(fake::live.size() == before.size() + 1);
    DevEvent bad;
    fake::fail_nth(fake::EVENT, 1);
    REQUIRE(bad.create() != hipSuccess && (hipEvent_t)bad == nullptr);
    fake::fail_nth(fake::EVENT, 1);
    REQUIRE(bad.create(hipEventDisableTiming) != hipSuccess && (hipEvent_t)bad == nullptr);
    DevStream s, t;
    REQUIRE(s.create(hipStreamNonBlocking) == hipSuccess);
    hipStream_t hs = s;
    t = std::move(s);
    REQUIRE((hipStream_t)s == nullptr && (hipStream_t)t == hs);
    fake::fail_nth(fake::STREAM, 1);
    REQUIRE(s.create(hipStreamNonBlocking) != hipSuccess && (hipStream_t)s == nullptr);
  }
  REQUIRE(fake::live == before);
  for (int i = 1; i <= 6; ++i) {  // creation i of the timer's six failing
    fake::reset();
    {
      StageTimer<6> timer;
      fake::fail_nth(fake::EVENT, i);
      REQUIRE(timer.create() != hipSuccess);  // reported
      REQUIRE(fake::live.size() == before.size() + (size_t)(i - 1));
    }
    REQUIRE(fake::live == before);  // and what it had created is destroyed
  }
  {
    StageTimer<2> clock;
    REQUIRE(clock.create() == hipSuccess);
    clock.begin(nullptr);
    REQUIRE(clock.end(nullptr) == 1.5f && clock.ms(0, 1) == 1.5f);
    StageTimer<2> never;  // never created: its marks fail, its times are 0
    REQUIRE(never.mark(0, nullptr) != hipSuccess && never.end(nullptr) == 0.0f && never.ms(0, 1) == 0.0f);
  }
  REQUIRE(fake::live == before);
}

int main() {
  scope_exit_case<DBuf>('M', 'F');
  scope_exit_case<HBuf>('H', 'G');
  ensure_case<DBuf>(fake::MALLOC, 'M', 'F', 256);
  ensure_case<HBuf>(fake::HOST_MALLOC, 'H', 'G', 4096);
  grow_case();
  const Shape shapes[] = {{"f32 with mirror", 4, true, 6}, {"f32 without", 4, false, 4}, {"fp16", 2, false, 4}};
  for (const Shape& sh : shapes) pool_case(sh);
  handle_case();
  REQUIRE(fake::live.empty());  // end of main: nothing is live
  std::printf("owned buffers ok\n");
  return 0;
}
