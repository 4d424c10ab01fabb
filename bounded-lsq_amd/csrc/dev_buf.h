// Owning buffers of the host side: device memory (DevBuf) and page-locked host memory (PinnedBuf).  Both free
// themselves in their destructor and cannot be copied, so a structure that holds one needs no release list: a new
// buffer is a new member and nothing else.  Needs hipMalloc / hipFree / hipHostMalloc / hipHostFree only (a host-only
// program that supplies those four can include it: tests/dev_buf_host).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <initializer_list>
#include <type_traits>

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
    return *this;
  }
  ~DevBuf() { release(); }
  // (a live buffer is freed first — hipFree waits for the device —; b == 0: empty, no allocation)
  hipError_t alloc(size_t b) {
    release();
    if (b == 0) return hipSuccess;
    const hipError_t e = hipMalloc(&p, b);
    if (e == hipSuccess) bytes = b; else p = nullptr;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
static_assert(!std::is_copy_constructible<DevBuf>::value, "a DevBuf has one owner");

// The buffers of a list, allocated in turn; 0, or the first failure recorded under its `what` by ctx->fail(e, what)
struct AllocReq { DevBuf* buf; size_t bytes; const char* what; };
template <class Ctx>
int alloc_all(Ctx* ctx, std::initializer_list<AllocReq> reqs) {
  for (const AllocReq& r : reqs) {
    const hipError_t e = r.buf->alloc(r.bytes);
    if (e != hipSuccess) return ctx->fail(e, r.what);
  }
  return 0;
}

// `count` zeroed T in page-locked host memory; reads as the T* it owns
template <class T>
struct PinnedBuf {
  T* p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { release(); }
  hipError_t alloc(size_t count, unsigned flags) {
    release();
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), count * sizeof(T), flags);
    if (e != hipSuccess) { p = nullptr; return e; }
    for (size_t i = 0; i < count; ++i) p[i] = T();
    return hipSuccess;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; }
  operator T*() const { return p; }
};
