// bufcheck.cpp -- chomp_buffers.h on the host, with counting stand-ins for the four allocation
// calls: what the owning types allocate, free, park and refuse.  A program of its own (built and
// run by tests/test_buffers_cpu.py with the address and undefined-behaviour sanitizers); exits 0
// when every check holds.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#define CHOMP_BUFFERS_STANDIN

namespace {
struct Space {
  std::map<void*, size_t> live;      // block -> bytes
  std::vector<size_t> sizes;         // bytes of every allocation, in order
  int frees = 0, double_frees = 0;
  int alloc(void** p, size_t bytes) {
    *p = std::malloc(bytes ? bytes : 1);
    live[*p] = bytes;
    sizes.push_back(bytes);
    return 0;
  }
  int release(void* p) {
    if (!live.count(p)) { ++double_frees; return 1; }
    live.erase(p);
    ++frees;
    std::free(p);
    return 0;
  }
};
Space device, pinned;
}  // namespace

namespace chomp {
int buf_dev_malloc(void** p, size_t bytes) { return device.alloc(p, bytes); }
int buf_dev_free(void* p) { return device.release(p); }
int buf_host_malloc(void** p, size_t bytes) { return pinned.alloc(p, bytes); }
int buf_host_free(void* p) { return pinned.release(p); }
}  // namespace chomp

#include "../../chomp_amd/csrc/chomp_buffers.h"

using namespace chomp;

static int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

struct Shadow {
  bool holds = true;
  void reset() { holds = false; }
};

// Growth 0 -> 8 -> 4 -> 16: blocks of exactly 8 and 16 elements, each old block freed once, "moved"
// twice.
template <class B>
static void growth(Space& S) {
  S = Space();
  {
    BufferHome home;
    B b;
    CHECK(b.get() == nullptr && b.cap() == 0 && !b.fits(0));
    CHECK(b.ensure(home, 8) == BufferGrowth::moved);
    double* first = b;
    CHECK(first && b.cap() == 8 && S.live.size() == 1);
    first[7] = 1.0;                                 // (the whole block is the buffer's)
    CHECK(b.ensure(home, 4) == BufferGrowth::kept);
    CHECK(b.get() == first && b.cap() == 8 && S.frees == 0);
    CHECK(b.ensure(home, 16) == BufferGrowth::moved);
    CHECK(b.cap() == 16 && S.frees == 1 && S.live.size() == 1 && !S.live.count(first));
    b[15] = 2.0;
    CHECK(b + 3 == b.get() + 3);                    // (pointer arithmetic through the conversion)
    CHECK(S.sizes.size() == 2 && S.sizes[0] == 8 * sizeof(double) && S.sizes[1] == 16 * sizeof(double));
    CHECK(home.graveyard.empty() && home.host_graveyard.empty());
  }
  CHECK(S.live.empty() && S.frees == 2 && S.double_frees == 0);
}

// With graph_seen the old block stays live until teardown, and is freed once there.
template <class B>
static void graveyard(Space& S, bool pinned_kind) {
  S = Space();
  {
    BufferHome home;
    B b;
    CHECK(b.ensure(home, 8) == BufferGrowth::moved);
    double* old = b;
    home.graph_seen = true;
    CHECK(b.ensure(home, 16) == BufferGrowth::moved);
    CHECK(S.live.count(old) == 1 && S.live.size() == 2 && S.frees == 0);
    old[7] = 3.0;                                   // (a graph may still write there)
    const std::vector<void*>& yard = pinned_kind ? home.host_graveyard : home.graveyard;
    const std::vector<void*>& other = pinned_kind ? home.graveyard : home.host_graveyard;
    CHECK(yard.size() == 1 && yard[0] == old && other.empty());
    CHECK(b.renew(home, 16) == BufferGrowth::moved && yard.size() == 2 && S.live.size() == 3);
  }
  CHECK(S.live.empty() && S.frees == 3 && S.double_frees == 0);
}

// Under capture growth is refused and the buffer untouched; a request that fits is accepted.
template <class B>
static void capture(Space& S) {
  S = Space();
  {
    BufferHome home;
    B b;
    home.capture = true;
    CHECK(b.ensure(home, 8) == BufferGrowth::refused && b.get() == nullptr && S.sizes.empty());
    home.capture = false;
    CHECK(b.ensure(home, 8) == BufferGrowth::moved);
    double* p = b;
    home.capture = true;
    CHECK(b.ensure(home, 8) == BufferGrowth::kept && b.ensure(home, 1) == BufferGrowth::kept);
    CHECK(b.ensure(home, 9) == BufferGrowth::refused);
    CHECK(b.get() == p && b.cap() == 8 && S.frees == 0 && S.sizes.size() == 1);
    CHECK(home.graveyard.empty() && home.host_graveyard.empty());
  }
  CHECK(S.live.empty() && S.frees == 1 && S.double_frees == 0);
}

// A fed buffer loses its shadow when it moves and keeps it when it does not.
static void fed() {
  device = Space();
  {
    BufferHome home;
    FedBuffer<int, Shadow> f;
    CHECK(f.ensure(home, 8) == BufferGrowth::moved && !f.sh.holds);
    f.sh.holds = true;
    CHECK(f.ensure(home, 8) == BufferGrowth::kept && f.ensure(home, 3) == BufferGrowth::kept && f.sh.holds);
    home.capture = true;
    CHECK(f.ensure(home, 9) == BufferGrowth::refused && f.sh.holds);
    home.capture = false;
    int* before = f;
    CHECK(f.ensure(home, 9) == BufferGrowth::moved && !f.sh.holds && f.dev.cap() == 9);
    CHECK(!device.live.count(before));
    f.sh.holds = true;
    CHECK(f.renew(home, 9) == BufferGrowth::moved && !f.sh.holds);
  }
  CHECK(device.live.empty() && device.frees == 3 && device.double_frees == 0);
}

// Allocate once: the first size stays.
static void once() {
  device = Space();
  {
    DeviceBuffer<double> b;
    CHECK(b.once(5) == 0 && b.cap() == 5);
    double* p = b;
    CHECK(b.once(50) == 0 && b.get() == p && b.cap() == 5 && device.sizes.size() == 1);
  }
  CHECK(device.live.empty() && device.frees == 1 && device.double_frees == 0);
}

int main() {
  growth<DeviceBuffer<double>>(device);
  growth<PinnedBuffer<double>>(pinned);
  graveyard<DeviceBuffer<double>>(device, false);
  graveyard<PinnedBuffer<double>>(pinned, true);
  capture<DeviceBuffer<double>>(device);
  capture<PinnedBuffer<double>>(pinned);
  fed();
  once();
  CHECK(device.live.empty() && pinned.live.empty());
  CHECK(device.double_frees == 0 && pinned.double_frees == 0);
  if (failures) { std::printf("bufcheck: %d checks failed\n", failures); return 1; }
  std::printf("bufcheck ok\n");
  return 0;
}
