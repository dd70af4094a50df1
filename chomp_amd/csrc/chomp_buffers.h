// chomp_buffers.h -- the owning types of a context's device and pinned host memory.
//
// A buffer is a pointer and a capacity in elements; it frees itself when the context goes.  It
// converts to T*, so launches, pointer arithmetic and copies read as they would with a raw
// pointer.  Growth never keeps contents, allocates exactly what was asked for, refuses while the
// context's stream is being captured, and parks (not frees) the old block once a call of the
// context has been captured: a graph may still hold its address (include/chomp_mi355x.h, "HIP
// graphs").  It says whether the block moved, so the caller can drop what described the old one.
//
// The four allocation calls come from outside: the HIP runtime's, unless CHOMP_BUFFERS_STANDIN is
// defined, in which case the including program defines chomp::buf_dev_malloc, buf_dev_free,
// buf_host_malloc and buf_host_free itself (tests/hostcheck/bufcheck.cpp; 0 is success).
#pragma once

#include <cstddef>
#include <vector>

#ifndef CHOMP_BUFFERS_STANDIN
#include <hip/hip_runtime.h>
namespace chomp {
inline int buf_dev_malloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
inline int buf_dev_free(void* p) { return (int)hipFree(p); }
inline int buf_host_malloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
inline int buf_host_free(void* p) { return (int)hipHostFree(p); }
}  // namespace chomp
#endif

namespace chomp {

// What growth has to know of the context; the graveyards are drained when it goes.
struct BufferHome {
  bool capture = false;      // the context's stream is being captured (as of the last look)
  bool graph_seen = false;   // a call of this context has been captured at least once
  std::vector<void*> graveyard;        // device blocks a captured graph may still reference
  std::vector<void*> host_graveyard;   // (pinned words a graph's kernels or copies may write)
  int error = 0;             // the allocation call's code of the last BufferGrowth::failed
  BufferHome() = default;
  BufferHome(const BufferHome&) = delete;
  BufferHome& operator=(const BufferHome&) = delete;
  ~BufferHome() {
    for (void* p : graveyard) (void)buf_dev_free(p);
    for (void* p : host_graveyard) (void)buf_host_free(p);
  }
};

enum class BufferGrowth { kept, moved, refused, failed };

template <class T, bool Pinned>
class Buffer {
 public:
  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() { if (p_) (void)(Pinned ? buf_host_free(p_) : buf_dev_free(p_)); }

  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t cap() const { return cap_; }
  bool fits(size_t n) const { return n <= cap_ && p_; }

  // Room for n elements.  kept: there was (nothing is touched).
  BufferGrowth ensure(BufferHome& home, size_t n) {
    if (fits(n)) return BufferGrowth::kept;
    if (home.capture) return BufferGrowth::refused;
    return renew(home, n);
  }
  // A new block of exactly n elements in place of the old one, whatever its size (for callers
  // that decide about growth and capture themselves).
  BufferGrowth renew(BufferHome& home, size_t n) {
    if (p_) {
      if (home.graph_seen) (Pinned ? home.host_graveyard : home.graveyard).push_back(p_);
      else if ((home.error = Pinned ? buf_host_free(p_) : buf_dev_free(p_))) return BufferGrowth::failed;
    }
    p_ = nullptr;
    cap_ = 0;
    if ((home.error = once(n))) return BufferGrowth::failed;
    return BufferGrowth::moved;
  }
  // Allocate once, n elements for good: nothing happens when the block is there.  The
  // allocation call's code (0: fine).
  int once(size_t n) {
    if (p_) return 0;
    void* q = nullptr;
    const int e = Pinned ? buf_host_malloc(&q, n * sizeof(T)) : buf_dev_malloc(&q, n * sizeof(T));
    if (e) return e;
    p_ = static_cast<T*>(q);
    cap_ = n;
    return 0;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};
template <class T> using DeviceBuffer = Buffer<T, false>;
template <class T> using PinnedBuffer = Buffer<T, true>;

// A device buffer fed through a staging shadow (anything with reset(): the shadow says what the
// device holds).  The two travel together: a buffer that moved holds nothing, so its shadow goes.
template <class T, class Shadow>
struct FedBuffer {
  DeviceBuffer<T> dev;
  Shadow sh;
  operator T*() const { return dev; }
  bool fits(size_t n) const { return dev.fits(n); }
  BufferGrowth ensure(BufferHome& home, size_t n) { return dropped(dev.ensure(home, n)); }
  BufferGrowth renew(BufferHome& home, size_t n) { return dropped(dev.renew(home, n)); }

 private:
  BufferGrowth dropped(BufferGrowth g) {
    if (g == BufferGrowth::moved || g == BufferGrowth::failed) sh.reset();
    return g;
  }
};

#ifndef CHOMP_BUFFERS_STANDIN
// A parameter block on its way to the device: the host shadow says what the device holds (an
// unchanged block is not uploaded again -- MCMC-style loops re-run the set-up with mostly
// identical inputs); a changed block goes through one of two pinned staging buffers, each guarded
// by an event, so the copy is a true asynchronous DMA and the host never drains the stream
// (SimulationDesign / MCMC loops change a block on every call).  Filled by upload() of
// chomp_capi.hip.
struct StagedBlock {
  std::vector<char> shadow;
  void* pin[2] = {nullptr, nullptr};
  hipEvent_t done[2] = {nullptr, nullptr};
  bool used[2] = {false, false};
  size_t cap = 0;
  int turn = 0;
  StagedBlock() = default;
  StagedBlock(const StagedBlock&) = delete;
  StagedBlock& operator=(const StagedBlock&) = delete;
  ~StagedBlock() {
    for (int i = 0; i < 2; ++i) {
      if (pin[i]) (void)hipHostFree(pin[i]);
      if (done[i]) (void)hipEventDestroy(done[i]);
    }
  }
  void reset() { shadow.clear(); }
};
template <class T> using StagedBuffer = FedBuffer<T, StagedBlock>;
#endif

}  // namespace chomp
