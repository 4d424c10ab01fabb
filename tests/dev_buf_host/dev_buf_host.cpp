// Host-only check of csrc/dev_buf.h: the four HIP allocation calls it needs are defined here on top of malloc / free
// with a live-allocation counter, so the ownership rules run — under the address and undefined-behaviour sanitizers —
// without a GPU and without the HIP runtime.  Exit status 0: every check held and nothing is live.
#include "dev_buf.h"

#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

static long g_live = 0, g_host_live = 0;
static long g_mallocs = 0, g_fail_at = -1;           // hipMalloc number g_fail_at (counted from 0) fails

extern "C" hipError_t hipMalloc(void** ptr, size_t size) {
  if (g_mallocs++ == g_fail_at) { *ptr = nullptr; return hipErrorOutOfMemory; }
  *ptr = malloc(size);
  ++g_live;
  return hipSuccess;
}
extern "C" hipError_t hipFree(void* ptr) {
  if (ptr) { free(ptr); --g_live; }
  return hipSuccess;
}
extern "C" hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) {
  *ptr = malloc(size);
  ++g_host_live;
  return hipSuccess;
}
extern "C" hipError_t hipHostFree(void* ptr) {
  if (ptr) { free(ptr); --g_host_live; }
  return hipSuccess;
}

static int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failed; } \
  } while (0)

struct Holder { int tag; DevBuf buf; };              // as Level in blsq_host.h
struct Ctx {                                         // what alloc_all asks of a context
  const char* where = nullptr;
  int fail(hipError_t e, const char* what) { where = what; return (int)e; }
};

int main() {
  {  // a vector of holders grows through several reallocations
    std::vector<Holder> v;
    size_t caps = 0, last_cap = 0;
    for (int i = 0; i < 40; ++i) {
      Holder h{i, {}};
      CHECK(h.buf.alloc(64 + i) == hipSuccess);
      v.push_back(std::move(h));
      CHECK(h.buf.p == nullptr && h.buf.bytes == 0);
      if (v.capacity() != last_cap) { ++caps; last_cap = v.capacity(); }
    }
    CHECK(caps >= 4);
    CHECK(g_live == 40);
    for (int i = 0; i < 40; ++i) {
      CHECK(v[i].tag == i && v[i].buf.bytes == (size_t)(64 + i));
      v[i].buf.as<unsigned char>()[63 + i] = 1;      // (the last byte: the sanitizer watches the bounds)
    }
  }
  CHECK(g_live == 0);
  {  // move construction, move assignment, self-move
    DevBuf a;
    CHECK(a.alloc(128) == hipSuccess);
    void* pa = a.p;
    DevBuf b(std::move(a));
    CHECK(a.p == nullptr && a.bytes == 0 && b.p == pa && b.bytes == 128 && g_live == 1);
    DevBuf c;
    CHECK(c.alloc(32) == hipSuccess && g_live == 2);
    c = std::move(b);                                // (frees c's own 32 bytes)
    CHECK(b.p == nullptr && b.bytes == 0 && c.p == pa && c.bytes == 128 && g_live == 1);
    DevBuf& same = c;
    c = std::move(same);
    CHECK(c.p == pa && c.bytes == 128 && g_live == 1);
  }
  CHECK(g_live == 0);
  {  // alloc on a live buffer, alloc(0), double release
    DevBuf a;
    CHECK(a.alloc(16) == hipSuccess && g_live == 1);
    CHECK(a.alloc(48) == hipSuccess && g_live == 1 && a.bytes == 48);
    a.as<unsigned char>()[47] = 1;
    CHECK(a.alloc(0) == hipSuccess && a.p == nullptr && a.bytes == 0 && g_live == 0);
    CHECK(a.alloc(8) == hipSuccess && g_live == 1);
    a.release();
    CHECK(a.p == nullptr && a.bytes == 0 && g_live == 0);
    a.release();
    CHECK(g_live == 0);
  }
  {  // alloc_all whose third request fails: the failure is reported, nothing stays live after the scope
    Ctx ctx;
    {
      DevBuf a, b, c, d;
      g_fail_at = g_mallocs + 2;
      const int rc = alloc_all(&ctx, {{&a, 8, "first"}, {&b, 8, "second"}, {&c, 8, "third"}, {&d, 8, "fourth"}});
      g_fail_at = -1;
      CHECK(rc == (int)hipErrorOutOfMemory && ctx.where && ctx.where[0] == 't');
      CHECK(a.p && b.p && !c.p && !d.p && g_live == 2);
    }
    CHECK(g_live == 0);
  }
  {  // the pinned counterpart: zeroed, reads as its pointer, frees itself; alloc on a live one
    PinnedBuf<int> pin;
    CHECK(!pin);
    CHECK(pin.alloc(4, 0) == hipSuccess && g_host_live == 1);
    int* q = pin;
    CHECK(q[0] == 0 && q[3] == 0 && pin[3] == 0);
    CHECK(pin.alloc(128, 0) == hipSuccess && g_host_live == 1);
    pin[127] = 7;
  }
  CHECK(g_host_live == 0 && g_live == 0);
  if (g_failed) return 1;
  printf("dev_buf_host ok\n");
  return 0;
}
