// Stand-alone check of the owner types in khronos_amd/csrc/khr_owned.h (tests/test_cpu_owned.py compiles and runs it).
// It passes with and without a HIP device: without one every allocation fails, which is the path a context's teardown after a
// failed khr_create depends on; with one the same statements exercise the real allocate / move / release path.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

#include "../khronos_amd/csrc/khr_owned.h"

static std::string g_err;
extern "C" void khr_set_last_error(const char* text) { g_err = text ? text : ""; }

using namespace khr;

static int g_checks = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static int64_t live(LiveKind k) { return g_live[k].load(std::memory_order_relaxed); }
static bool allZero() { return live(LIVE_DEVICE) == 0 && live(LIVE_PINNED) == 0 && live(LIVE_EVENT) == 0 && live(LIVE_STREAM) == 0; }

// alloc / reserve / move / reset of one buffer kind
template <typename B>
static void checkBuffer(LiveKind kind, const char* name) {
  CHECK(allZero());
  {
    B b;
    CHECK(!b && b.get() == nullptr && b.count() == 0);
    b.reset();  // reset of an empty object
    b.reset();
    CHECK(allZero());
    g_err.clear();
    const int rc = b.alloc(1000);
    if (rc != KHR_OK) {  // a failure: the code, the text, an empty object, nothing counted
      CHECK(rc == KHR_ENOMEM);
      CHECK(!g_err.empty());
      CHECK(!b && b.count() == 0);
      CHECK(allZero());
      g_err.clear();
      CHECK(b.reserve(2000) == KHR_ENOMEM && !g_err.empty() && !b && b.count() == 0 && allZero());
    } else {
      CHECK(b && b.count() == 1000 && live(kind) == 1);
      auto* const p0 = b.get();
      CHECK(b.reserve(500) == KHR_OK && b.get() == p0 && b.count() == 1000);  // grow-only: a smaller request changes nothing
      CHECK(b.reserve(2000) == KHR_OK && b.count() == 2000 && live(kind) == 1);  // exact size, the old block is gone
    }
    CHECK(b.reserve(0) == KHR_OK);
    {  // a zero-size request is an empty success
      B z;
      CHECK(z.alloc(0) == KHR_OK && !z && z.count() == 0 && live(kind) == (b ? 1 : 0));
    }
    // moves transfer what is held (whatever that is) and leave the source empty; nothing is counted twice
    auto* const p = b.get();
    const size_t n = b.count();
    const int64_t held = live(kind);
    B c(std::move(b));
    CHECK(!b && b.count() == 0 && c.get() == p && c.count() == n && live(kind) == held);
    B d;
    d = std::move(c);
    CHECK(!c && c.count() == 0 && d.get() == p && d.count() == n && live(kind) == held);
    B& self = d;
    d = std::move(self);  // self-assignment keeps the block
    CHECK(d.get() == p && d.count() == n && live(kind) == held);
    d.reset();
    d.reset();  // a second reset is harmless
    CHECK(!d && d.count() == 0 && allZero());
  }
  CHECK(allZero());
  std::printf("%s ok\n", name);
}

int main() {
  checkBuffer<DevBuf<uint32_t>>(LIVE_DEVICE, "DevBuf");
  checkBuffer<DevBuf<uint8_t>>(LIVE_DEVICE, "DevBuf<uint8_t>");
  checkBuffer<PinnedBuf<uint32_t>>(LIVE_PINNED, "PinnedBuf");
  checkBuffer<PinnedBuf<void>>(LIVE_PINNED, "PinnedBuf<void>");
  {  // the device view of a page-locked block exists exactly while the block does
    PinnedBuf<uint32_t> h;
    CHECK(h.dev() == nullptr);
    if (h.alloc(16) == KHR_OK) CHECK(h.dev() != nullptr);
    else CHECK(h.dev() == nullptr);
    h.reset();
    CHECK(h.dev() == nullptr && allZero());
  }
  {  // Event: created by the first ensure() only
    Event e;
    CHECK(!e);
    e.reset();
    g_err.clear();
    const int rc = e.ensure();
    if (rc != KHR_OK) {
      CHECK(rc == KHR_EDEVICE && !g_err.empty() && !e && allZero());
    } else {
      hipEvent_t h = e;
      CHECK(h != nullptr && live(LIVE_EVENT) == 1);
      CHECK(e.ensure() == KHR_OK && e.get() == h && live(LIVE_EVENT) == 1);
    }
    const int64_t held = live(LIVE_EVENT);
    hipEvent_t h = e.get();
    Event f(std::move(e));
    CHECK(!e && f.get() == h && live(LIVE_EVENT) == held);
    Event g;
    g = std::move(f);
    CHECK(!f && g.get() == h && live(LIVE_EVENT) == held);
    g.reset();
    g.reset();
    CHECK(!g && allZero());
  }
  {  // Stream: one of its own ...
    Stream s;
    CHECK(!s && !s.owns());
    s.reset();
    g_err.clear();
    const int rc = s.create(hipStreamNonBlocking);
    if (rc != KHR_OK) CHECK(rc == KHR_EDEVICE && !g_err.empty() && !s && !s.owns() && allZero());
    else CHECK(s && s.owns() && live(LIVE_STREAM) == 1);
    // ... replaced by a caller's stream: referred to, not counted, never destroyed (this handle is not even a stream: destroying or
    // using it would fault)
    alignas(64) static char not_a_stream[64];
    hipStream_t callers = reinterpret_cast<hipStream_t>(not_a_stream);
    s.refer(callers);
    CHECK(s.get() == callers && !s.owns() && allZero());
    Stream t(std::move(s));
    CHECK(!s && t.get() == callers && !t.owns() && allZero());
    Stream u;
    u = std::move(t);
    CHECK(!t && u.get() == callers && !u.owns() && allZero());
    u.reset();
    u.reset();
    CHECK(!u && allZero());
    u.refer(callers);  // (and left to the destructor)
  }
  CHECK(allZero());
  std::printf("owned selftest ok (%d checks)\n", g_checks);
  return 0;
}
