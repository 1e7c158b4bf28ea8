// host_owners.h -- what the host code of the library's three translation units (uvaia_gpu.hip through host_ctx.inc, uvaia_cluster.hip,
// uvaia_align.hip) owns on the device: device buffers, pinned blocks, events and streams behind move-only handles.  Host code only.
//
// A failed HIP call is reported through a hook the including unit declares BEFORE this header, one overload per context type:
//   int hip_failed(Ctx *c, hipError_t e, const char *call, const char *file, int line);   // records the message, returns the unit's error code
// (c may be null: the unit's open function has no context to report to yet).  The handles live in an unnamed namespace because their member
// templates name that hook: every unit gets handles of its own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>

// One check for every HIP call inside a function that returns the unit's error code
#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_failed((c), e_, #call, __FILE__, __LINE__); } while (0)

namespace {

// Device memory of `cap` elements.  reserve() is the one grow step: nothing happens while the capacity suffices; otherwise what was held
// goes (contents are not kept), and the capacity is recorded only once the new array exists -- a failure leaves the buffer empty.
// Whoever calls it has waited for the work that may still read the old array.
template <class T> struct DevBuf {
  T *p = nullptr; size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
  ~DevBuf() { release(); }
  void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
  template <class C> int reserve(C c, size_t n)
  {
    if (n <= cap) return 0;
    release();
    HIPCHK(c, hipMalloc(&p, n * sizeof(T)));
    cap = n;
    return 0;
  }
  // The grow step that keeps contents: a new array of n elements takes the first `keep` of the old one by a copy on `stream`, the host
  // waits for the stream (the copy, and every kernel queued before it that reads the old array), then the old array goes.  A failure
  // leaves the buffer as it was.
  template <class C> int grow_keeping(C c, size_t n, size_t keep, hipStream_t stream)
  {
    DevBuf nb;
    if (int rc = nb.reserve(c, n)) return rc;
    if (keep) HIPCHK(c, hipMemcpyAsync(nb.p, p, keep * sizeof(T), hipMemcpyDeviceToDevice, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
    *this = std::move(nb);
    return 0;
  }
  operator T *() const { return p; }
};

// a pinned host block
struct PinnedBuf {
  uint8_t *p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete; PinnedBuf &operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() { if (p) hipHostFree(p); }
  template <class C> int alloc(C c, size_t bytes) { HIPCHK(c, hipHostMalloc(&p, bytes, hipHostMallocDefault)); return 0; }
  operator uint8_t *() const { return p; }
};

// an event, made by the first make() (later ones do nothing): with timing by default, or with the flags given
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event &) = delete; Event &operator=(const Event &) = delete;
  Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
  Event &operator=(Event &&o) noexcept { if (this != &o) { if (e) hipEventDestroy(e); e = o.e; o.e = nullptr; } return *this; }
  ~Event() { if (e) hipEventDestroy(e); }
  template <class C> int make(C c, unsigned flags = 0)
  {
    if (e) return 0;
    if (flags) HIPCHK(c, hipEventCreateWithFlags(&e, flags)); else HIPCHK(c, hipEventCreate(&e));
    return 0;
  }
  operator hipEvent_t() const { return e; }
};

// a stream the holder created (s is filled by the hipStreamCreate* call that suits it); the holder waits for it before it goes
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream &) = delete; Stream &operator=(const Stream &) = delete;
  ~Stream() { if (s) hipStreamDestroy(s); }
  operator hipStream_t() const { return s; }
};

}  // namespace
