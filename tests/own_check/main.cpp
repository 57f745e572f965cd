// own_check — the four holders of csrc/smpc_own.h against counting stand-ins for the eight runtime
// calls they make: malloc / free underneath, a live count per kind, and a switch that makes the next
// allocation fail.  No GPU and no HIP runtime: this file defines the calls itself.  Built with
// -fsanitize=address,undefined by tests/test_own_cpu.py, so a double free or a leak of the
// stand-ins' blocks fails the run as well.  Exit status 0: every check held.
#include "../../mpcholonavigation_amd/csrc/smpc_own.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

namespace {

struct Kind {
  const char* name;
  int live = 0, made = 0, freed = 0;
};
Kind g_dev{"device"}, g_pin{"pinned"}, g_ev{"event"}, g_st{"stream"};
bool g_fail_next = false;   // the next allocation of either buffer kind fails, once
unsigned int g_last_flags = 0;

hipError_t make(Kind& k, void** out, size_t bytes)
{
  if (g_fail_next) {
    g_fail_next = false;
    return hipErrorOutOfMemory;
  }
  *out = malloc(bytes ? bytes : 1);
  if (!*out) return hipErrorOutOfMemory;
  k.live++; k.made++;
  return hipSuccess;
}
hipError_t drop(Kind& k, void* p)
{
  if (!p) return hipErrorInvalidValue;
  free(p);   // (a block freed twice: the sanitizer reports it)
  k.live--; k.freed++;
  return hipSuccess;
}

int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      g_failed++;                                                          \
    }                                                                      \
  } while (0)

}  // namespace

extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) {return make(g_dev, ptr, size);}
hipError_t hipFree(void* ptr) {return drop(g_dev, ptr);}
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int flags)
{
  g_last_flags = flags;
  return make(g_pin, ptr, size);
}
hipError_t hipHostFree(void* ptr) {return drop(g_pin, ptr);}
hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned flags)
{
  g_last_flags = flags;
  return make(g_ev, reinterpret_cast<void**>(event), 1);
}
hipError_t hipEventDestroy(hipEvent_t event) {return drop(g_ev, event);}
hipError_t hipStreamCreateWithFlags(hipStream_t* stream, unsigned int flags)
{
  g_last_flags = flags;
  return make(g_st, reinterpret_cast<void**>(stream), 1);
}
hipError_t hipStreamDestroy(hipStream_t stream) {return drop(g_st, stream);}
}

using smpc_impl::DevBuf;
using smpc_impl::Event;
using smpc_impl::PinnedBuf;
using smpc_impl::Stream;

// what the two buffers share; `ensure` allocates a buffer of `count` elements with the kind's defaults
template <typename Buf>
static void check_buffer(Kind& k)
{
  CHECK(k.live == 0);
  k = Kind{k.name};   // the counts below are this call's
  {
    Buf a;
    CHECK(!a && a.get() == nullptr && a.capacity() == 0);
    CHECK(a.ensure(100) == hipSuccess);
    CHECK(a && a.get() != nullptr && a.capacity() == 100 && k.live == 1);
    // ---- a smaller or equal count keeps the pointer
    auto* const p = a.get();
    CHECK(a.ensure(100) == hipSuccess && a.get() == p && a.capacity() == 100);
    CHECK(a.ensure(7) == hipSuccess && a.get() == p && a.capacity() == 100);
    CHECK(k.made == 1 && k.freed == 0);
    // ---- a larger count frees once and allocates once
    CHECK(a.ensure(101) == hipSuccess);
    CHECK(a.capacity() == 101 && k.made == 2 && k.freed == 1 && k.live == 1);
    // ---- a moved-from holder is empty and frees nothing
    auto* const q = a.get();
    Buf b(std::move(a));
    CHECK(!a && a.get() == nullptr && a.capacity() == 0);
    CHECK(b.get() == q && b.capacity() == 101 && k.live == 1 && k.freed == 1);
    {
      Buf gone(std::move(a));   // (empty from empty)
      CHECK(!gone);
    }
    CHECK(k.freed == 1 && k.live == 1);
    // ---- move-assigning over a held resource frees it exactly once
    Buf c;
    CHECK(c.ensure(5) == hipSuccess && k.live == 2);
    auto* const held = b.get();
    c = std::move(b);
    CHECK(c.get() == held && c.capacity() == 101 && !b && b.capacity() == 0);
    CHECK(k.live == 1 && k.freed == 2);
    // ---- a failed ensure leaves the holder empty with capacity 0, and a later ensure succeeds
    g_fail_next = true;
    CHECK(c.ensure(1000) == hipErrorOutOfMemory);
    CHECK(!c && c.get() == nullptr && c.capacity() == 0 && k.live == 0 && k.freed == 3);
    CHECK(c.ensure(3) == hipSuccess && c && c.capacity() == 3 && k.live == 1);
    g_fail_next = true;
    Buf d;
    CHECK(d.ensure(1) == hipErrorOutOfMemory && !d && d.capacity() == 0);
    CHECK(d.ensure(1) == hipSuccess && d && k.live == 2);
    // ---- release() hands the resource over, and the destructor then frees nothing
    const int freed = k.freed;
    auto* mine = static_cast<void*>(nullptr);
    {
      Buf e;
      CHECK(e.ensure(9) == hipSuccess && k.live == 3);
      mine = e.release();
      CHECK(mine != nullptr && !e && e.capacity() == 0);
    }
    CHECK(k.freed == freed && k.live == 3);
    CHECK(drop(k, mine) == hipSuccess);
  }
  // c and d went at the end of the scope
  CHECK(k.live == 0 && k.made == k.freed);
}

template <typename H>
static void check_handle(Kind& k, unsigned int flags)
{
  CHECK(k.live == 0);
  k = Kind{k.name};
  {
    H a;
    CHECK(!a && a.get() == nullptr);
    CHECK(a.ensure(flags) == hipSuccess && a && k.live == 1 && g_last_flags == flags);
    auto const h = a.get();
    CHECK(a.ensure(flags) == hipSuccess && a.get() == h && k.made == 1);   // held: kept
    H b(std::move(a));
    CHECK(!a && a.get() == nullptr && b.get() == h && k.live == 1 && k.freed == 0);
    H c;
    CHECK(c.ensure(flags) == hipSuccess && k.live == 2);
    c = std::move(b);
    CHECK(c.get() == h && !b && k.live == 1 && k.freed == 1);
    g_fail_next = true;
    H d;
    CHECK(d.ensure(flags) != hipSuccess && !d && d.get() == nullptr);
    CHECK(d.ensure(flags) == hipSuccess && d && k.live == 2);
    const int freed = k.freed;
    auto mine = h;
    {
      H e;
      CHECK(e.ensure(flags) == hipSuccess && k.live == 3);
      mine = e.release();
      CHECK(mine != nullptr && !e);
    }
    CHECK(k.freed == freed && k.live == 3);
    CHECK(drop(k, mine) == hipSuccess);
  }
  CHECK(k.live == 0 && k.made == k.freed);
}

int main()
{
  check_buffer<DevBuf<float>>(g_dev);
  check_buffer<DevBuf<unsigned char>>(g_dev);
  check_buffer<PinnedBuf<double>>(g_pin);
  {
    // the flags reach the runtime; the default is hipHostMallocDefault
    PinnedBuf<float> p;
    CHECK(p.ensure(4, hipHostMallocMapped) == hipSuccess && g_last_flags == hipHostMallocMapped);
    PinnedBuf<float> q;
    CHECK(q.ensure(4) == hipSuccess && g_last_flags == hipHostMallocDefault);
    // a block allocated elsewhere: the holder's from adopt() on, the one it held before freed
    DevBuf<int> a;
    CHECK(a.ensure(2) == hipSuccess);
    void* other = nullptr;
    CHECK(make(g_dev, &other, 64) == hipSuccess && g_dev.live == 2);
    a.adopt(static_cast<int*>(other), 16);
    CHECK(a.get() == other && a.capacity() == 16 && g_dev.live == 1);
  }
  check_handle<Event>(g_ev, hipEventDisableTiming);
  check_handle<Stream>(g_st, hipStreamNonBlocking);
  {
    Event e;
    CHECK(e.ensure() == hipSuccess && g_last_flags == hipEventDefault);
  }
  // ---- at exit every live count is 0
  for (const Kind* k : {&g_dev, &g_pin, &g_ev, &g_st}) {
    if (k->live != 0) {
      fprintf(stderr, "%s: %d still live\n", k->name, k->live);
      g_failed++;
    }
    CHECK(k->made > 0 && k->made == k->freed);
  }
  return g_failed ? 1 : 0;
}
