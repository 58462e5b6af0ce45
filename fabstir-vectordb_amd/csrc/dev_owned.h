// dev_owned.h — scoped owners of what the HIP runtime hands out: device memory (DBuf), pinned host memory (HBuf),
// events (DevEvent), streams (DevStream), and a stage timer over events.  Host-only code, and the one place in the
// engine that calls hipMalloc / hipFree / hipHostMalloc / hipHostFree / hipEventCreate* / hipEventDestroy /
// hipStreamCreate* / hipStreamDestroy.  Every owner is move-only and frees on scope exit.  None has static storage
// duration (a destructor would then run after the runtime has shut down): they live in the heap objects behind the
// C ABI's handles, or on the stack of a call.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <utility>

// alloc / free by themselves serve the C ABI's fvdb_dev_alloc and fvdb_host_alloc, whose blocks the caller owns
struct DeviceMem {
  static constexpr size_t kFloor = 256;
  static hipError_t alloc(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
  static hipError_t free(void* p) { return hipFree(p); }
};
struct PinnedMem {
  static constexpr size_t kFloor = 4096;
  static hipError_t alloc(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
  static hipError_t free(void* p) { return hipHostFree(p); }
};

template <typename Mem>
struct OwnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  OwnedBuf(OwnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  OwnedBuf& operator=(OwnedBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~OwnedBuf() { release(); }
  // scratch that only grows: a no-op when it fits, else the old block goes and a quarter more than asked is taken.
  // Contents are not preserved.
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    return exact(std::max<size_t>(bytes + bytes / 4, Mem::kFloor));
  }
  // the old block goes, then exactly `bytes` are taken (flags: hipHostMalloc's, pinned memory only).  On failure the
  // owner is empty.
  hipError_t exact(size_t bytes, unsigned flags = 0) {
    release();
    const hipError_t e = Mem::alloc(&p, bytes, flags);
    if (e == hipSuccess) {
      cap = bytes;
    } else {
      p = nullptr;
      (void)hipGetLastError();  // reported here: it must not surface again at the next launch check
    }
    return e;
  }
  void release() {
    if (p) (void)Mem::free(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const { return (T*)p; }
};
using DBuf = OwnedBuf<DeviceMem>;
using HBuf = OwnedBuf<PinnedMem>;  // pinned host staging (exact(): pass hipHostMallocMapped for a mapped block)
static_assert(hipHostMallocDefault == 0, "OwnedBuf::exact's default flags");
static_assert(!std::is_copy_constructible<DBuf>::value && std::is_nothrow_move_constructible<DBuf>::value, "DBuf is move-only");
static_assert(!std::is_copy_constructible<HBuf>::value && std::is_nothrow_move_constructible<HBuf>::value, "HBuf is move-only");

// Grow `b` to exactly `new_bytes` keeping its first `keep` bytes (stream-ordered copy), the rest zeroed when asked.
// The stream is synchronised before the new block takes the old one's place; on any failure the new block is freed and
// `b` is as it was.
inline hipError_t grow_keeping(DBuf& b, size_t new_bytes, size_t keep, bool zero_rest, hipStream_t st) {
  DBuf nb;
  hipError_t e = nb.exact(new_bytes);
  if (e == hipSuccess && keep) e = hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && zero_rest && new_bytes > keep) e = hipMemsetAsync((char*)nb.p + keep, 0, new_bytes - keep, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return e;
  std::swap(b, nb);
  return hipSuccess;
}

template <typename H, hipError_t (*Destroy)(H)>
struct OwnedHandle {
  H h = nullptr;
  OwnedHandle() = default;
  OwnedHandle(const OwnedHandle&) = delete;
  OwnedHandle& operator=(const OwnedHandle&) = delete;
  OwnedHandle(OwnedHandle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  OwnedHandle& operator=(OwnedHandle&& o) noexcept {
    if (this != &o) {
      release();
      h = std::exchange(o.h, nullptr);
    }
    return *this;
  }
  ~OwnedHandle() { release(); }
  void release() {
    if (h) (void)Destroy(h);
    h = nullptr;
  }
  operator H() const { return h; }
};
struct DevEvent : OwnedHandle<hipEvent_t, hipEventDestroy> {
  // a no-op when the event exists already (flags 0: hipEventCreate's timing event)
  hipError_t create(unsigned flags = 0) {
    if (h) return hipSuccess;
    const hipError_t rc = flags ? hipEventCreateWithFlags(&h, flags) : hipEventCreate(&h);
    if (rc != hipSuccess) h = nullptr;
    return rc;
  }
};
struct DevStream : OwnedHandle<hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags) {
    release();
    const hipError_t rc = hipStreamCreateWithFlags(&h, flags);
    if (rc != hipSuccess) h = nullptr;
    return rc;
  }
};
static_assert(!std::is_copy_constructible<DevEvent>::value && std::is_nothrow_move_constructible<DevEvent>::value, "DevEvent is move-only");
static_assert(!std::is_copy_constructible<DevStream>::value && std::is_nothrow_move_constructible<DevStream>::value, "DevStream is move-only");

// Stream time of the stages of one job: N marks, ms(a, b) between two of them once both have completed.  A job with a
// single stage at a time uses begin() .. end() (end waits for the stage).
template <int N>
struct StageTimer {
  DevEvent ev[N];
  hipError_t create() {
    for (auto& x : ev) {
      const hipError_t rc = x.create();
      if (rc != hipSuccess) return rc;  // what was created goes with the timer
    }
    return hipSuccess;
  }
  hipError_t mark(int i, hipStream_t st) { return hipEventRecord(ev[i], st); }
  float ms(int a, int b) const {
    float v = 0.0f;
    return hipEventElapsedTime(&v, ev[a], ev[b]) == hipSuccess ? v : 0.0f;
  }
  void begin(hipStream_t st) { (void)mark(0, st); }
  float end(hipStream_t st) {
    static_assert(N >= 2, "begin() .. end() takes two marks");
    if (mark(1, st) != hipSuccess || hipEventSynchronize(ev[1]) != hipSuccess) return 0.0f;
    return ms(0, 1);
  }
};
