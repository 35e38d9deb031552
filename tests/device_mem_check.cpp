// Stand-alone check of helicon_amd/csrc/device_mem.h on the host: hipMalloc / hipFree are the stubs below (malloc / free
// with a live-allocation counter and a switch that makes the n-th allocation fail), hipEventCreate / hipEventDestroy
// likewise, so no HIP runtime is linked.  Built
// with -fsanitize=address,undefined and run as a child process by tests/test_device_mem_host.py.
#include "device_mem.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

static int g_live = 0, g_peak = 0, g_mallocs = 0, g_frees = 0;
static int g_fail_at = 0;          // > 0: that allocation from now (1 = the next one) fails, once
static size_t g_last_bytes = 0;

extern "C" hipError_t hipMalloc(void** ptr, size_t size) {
  if (g_fail_at > 0 && --g_fail_at == 0) {
    *ptr = nullptr;
    return hipErrorOutOfMemory;
  }
  ++g_mallocs;
  g_last_bytes = size;
  if (size == 0) {                 // as the runtime: success and a null pointer
    *ptr = nullptr;
    return hipSuccess;
  }
  *ptr = std::malloc(size);
  std::memset(*ptr, 0xab, size);   // fresh memory is recognisable: growth must not carry the old contents over
  ++g_live;
  if (g_live > g_peak) g_peak = g_live;
  return hipSuccess;
}

extern "C" hipError_t hipFree(void* ptr) {
  if (ptr) {
    --g_live;
    ++g_frees;
    std::free(ptr);
  }
  return hipSuccess;
}

static int g_events = 0, g_event_fail_at = 0;   // live events; > 0: that creation from now fails, once

extern "C" hipError_t hipEventCreate(hipEvent_t* event) {
  if (g_event_fail_at > 0 && --g_event_fail_at == 0) return hipErrorOutOfMemory;
  *event = reinterpret_cast<hipEvent_t>(std::malloc(1));
  ++g_events;
  return hipSuccess;
}

extern "C" hipError_t hipEventDestroy(hipEvent_t event) {
  --g_events;
  std::free(event);
  return hipSuccess;
}

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<DevBuf<int>>::value, "DevBuf must not copy");
static_assert(std::is_nothrow_move_constructible<DevBuf<int>>::value && std::is_nothrow_move_assignable<DevBuf<int>>::value, "DevBuf moves");
static_assert(!std::is_copy_constructible<DevArena>::value && !std::is_copy_assignable<DevArena>::value, "DevArena must not copy");

static void buf_keeps_and_grows() {
  DevBuf<double> b;
  CHECK(b.get() == nullptr && b.size() == 0 && b.bytes() == 0);
  CHECK(b.ensure(10) && b.size() == 10 && b.bytes() == 80 && g_last_bytes == 80);
  double* const first = b.get();
  CHECK(first != nullptr && static_cast<double*>(b) == first && b + 3 == first + 3);
  const int mallocs = g_mallocs;
  CHECK(b.ensure(10) && b.get() == first);           // at capacity: kept
  CHECK(b.ensure(4) && b.get() == first && b.size() == 10);   // below: kept, and the size stays the buffer's own
  CHECK(g_mallocs == mallocs);
  std::memset(first, 0, 80);
  g_peak = g_live;
  CHECK(b.ensure(11) && b.size() == 11 && g_last_bytes == 88);   // exactly what was asked for: no geometric growth
  CHECK(g_peak == 1);                                // freed first, then allocated
  const unsigned char* raw = reinterpret_cast<const unsigned char*>(b.get());
  bool fresh = true;
  for (size_t i = 0; i < b.bytes(); ++i) fresh = fresh && raw[i] == 0xab;
  CHECK(fresh);                                      // no copy of the old contents
  b.reset();
  CHECK(b.get() == nullptr && b.size() == 0 && g_live == 0);
  b.reset();                                         // twice is harmless
}

static void buf_failed_growth() {
  DevBuf<int> b;
  CHECK(b.ensure(8));
  g_fail_at = 1;
  CHECK(!b.ensure(16));
  CHECK(b.get() == nullptr && b.size() == 0 && b.bytes() == 0 && g_live == 0);
  CHECK(DevBuf<int>::bytes_for(16) == 64);
  CHECK(dev_alloc_failed(64) == "device allocation of 64 bytes failed");
  CHECK(b.ensure(16) && b.size() == 16 && g_live == 1);   // a later ensure succeeds
  g_fail_at = 1;
  DevBuf<int> never;
  CHECK(!never.ensure(1) && never.get() == nullptr && never.size() == 0);
}

static void buf_moves() {
  DevBuf<float> a;
  CHECK(a.ensure(5));
  float* const p = a.get();
  DevBuf<float> b(std::move(a));
  CHECK(a.get() == nullptr && a.size() == 0 && b.get() == p && b.size() == 5 && g_live == 1);
  DevBuf<float> c;
  CHECK(c.ensure(7) && g_live == 2);
  c = std::move(b);                                   // the target's own buffer is freed, the source is left empty
  CHECK(c.get() == p && c.size() == 5 && b.get() == nullptr && b.size() == 0 && g_live == 1);
  DevBuf<float>& self = c;
  c = std::move(self);
  CHECK(c.get() == p && c.size() == 5 && g_live == 1);
}

static void arena_scopes() {
  {
    DevArena mem;
    int* a = mem.get<int>(3);
    CHECK(a != nullptr && g_last_bytes == 16);        // never below 16 bytes
    double* z = mem.get<double>(0);
    CHECK(z != nullptr && g_last_bytes == 16);        // a zero-sized request still gives a pointer
    char* c = mem.get<char>(100);
    CHECK(c != nullptr && g_last_bytes == 100 && mem.ok() && g_live == 3);
    struct Wide { double v[5]; };
    CHECK(mem.get<Wide>(0) != nullptr && g_last_bytes == sizeof(Wide));   // ... nor below one element
  }
  CHECK(g_live == 0);
  {
    DevArena mem;
    CHECK(mem.get<int>(4) != nullptr);
    g_fail_at = 1;
    CHECK(mem.get<float>(1000) == nullptr);           // the failure in the middle
    CHECK(!mem.ok() && mem.failed_bytes() == 4000);
    const int mallocs = g_mallocs;
    CHECK(mem.get<int>(4) == nullptr && g_mallocs == mallocs);   // ... stops the run of requests
    CHECK(g_live == 1);
  }
  CHECK(g_live == 0);
  {
    DevArena mem;
    CHECK(mem.get<int>(4) != nullptr && mem.get<int>(4) != nullptr && g_live == 2);
    mem.release();                                    // frees now, and the arena serves again
    CHECK(g_live == 0 && mem.ok());
    CHECK(mem.get<int>(4) != nullptr && g_live == 1);
  }
  CHECK(g_live == 0);
}

static_assert(!std::is_copy_constructible<DevEvents<2>>::value && !std::is_copy_assignable<DevEvents<2>>::value, "DevEvents must not copy");

static void events_on_demand() {
  {
    DevEvents<3> ev;
    CHECK(g_events == 0 && ev[0] == nullptr && ev[2] == nullptr);   // nothing until create()
    CHECK(ev.create() == hipSuccess && g_events == 3 && ev[0] && ev[1] && ev[2] && ev[0] != ev[1]);
    const hipEvent_t first = ev[0];
    CHECK(ev.create() == hipSuccess && g_events == 3 && ev[0] == first);   // a second call keeps them
  }
  CHECK(g_events == 0);
  {
    DevEvents<2> ev;
    g_event_fail_at = 2;
    CHECK(ev.create() == hipErrorOutOfMemory && g_events == 1 && ev[0] && ev[1] == nullptr);
    CHECK(ev.create() == hipSuccess && g_events == 2 && ev[1]);   // a later call creates only what is missing
  }
  CHECK(g_events == 0);
  { DevEvents<2> never; }   // never created: nothing to destroy
  CHECK(g_events == 0);
}

struct Holder {   // what the library's long-lived objects look like: freed by delete
  DevBuf<int> a;
  DevBuf<double> b;
};

int main() {
  buf_keeps_and_grows();
  CHECK(g_live == 0);
  buf_failed_growth();
  CHECK(g_live == 0);
  buf_moves();
  CHECK(g_live == 0);
  arena_scopes();
  events_on_demand();
  Holder* h = new Holder;
  CHECK(h->a.ensure(3) && h->b.ensure(3) && g_live == 2);
  delete h;
  CHECK(g_live == 0 && g_mallocs == g_frees);        // the live counter is 0 at exit: every allocation was freed once
  std::printf(g_failed ? "device_mem_check: %d check(s) failed\n" : "device_mem_check: ok (live %d)\n", g_failed ? g_failed : g_live);
  return g_failed ? 1 : 0;
}
