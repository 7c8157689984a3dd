// cassie_host.h -- host-only plumbing of the C-ABI units (cassie_cabi.hip, cassie3d_cabi.hip): owners of the HIP resources a handle holds,
// the handles' common base with its error reporting, the two-stream fork / join, and the helpers both ABIs spell the same way.
// hipFree, hipHostFree, hipStreamDestroy and hipEventDestroy appear here and nowhere else: a handle's members release themselves, so a
// handle declares its buffers BEFORE its events and streams (members go in reverse order: a stream is drained and destroyed before the
// buffers its kernels use are released).
#ifndef CASSIE_HOST_H_
#define CASSIE_HOST_H_
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <memory>
#include <string>
#include <type_traits>

#include "../../include/cassie_vec.h"

// Nothing here, and no handle type built from it, is part of what the library exports: CASSIE_HOST_PRIVATE_BEGIN / _END bracket the
// definitions (inline functions and implicit destructors would otherwise appear as weak symbols of libcassie2d.so).
#define CASSIE_HOST_PRIVATE_BEGIN _Pragma("GCC visibility push(hidden)")
#define CASSIE_HOST_PRIVATE_END _Pragma("GCC visibility pop")

CASSIE_HOST_PRIVATE_BEGIN
namespace cassie_host {

// ---- owners: move-only (a std::unique_ptr with a releasing deleter inside), get(), released by the destructor
struct FreeDevice { void operator()(void* p) const { (void)hipFree(p); } };
struct FreeHost { void operator()(void* p) const { (void)hipHostFree(p); } };
struct DestroyStream { void operator()(hipStream_t s) const { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } };   // queued work first
struct DestroyEvent { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };

template <class T> class DeviceBuffer {
  std::unique_ptr<T, FreeDevice> p_;
 public:
  T* get() const { return p_.get(); }
  explicit operator bool() const { return bool(p_); }
  void reset() { p_.reset(); }
  // `count` elements in place of what was held (released first); fill >= 0: every byte set to it before the call returns
  hipError_t alloc(size_t count, int fill = -1) {
    reset();
    T* p = nullptr;
    const hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e != hipSuccess) return e;
    p_.reset(p);
    return fill < 0 ? hipSuccess : hipMemset(p, fill, count * sizeof(T));
  }
  hipError_t ensure(size_t count, int fill = -1) { return p_ ? hipSuccess : alloc(count, fill); }   // allocate on first use
};

// pinned host words the device can write (mapped): get() the host address, dev() the device's; zeroed
template <class T> class MappedHost {
  std::unique_ptr<T, FreeHost> p_;
  T* dev_ = nullptr;
 public:
  T* get() const { return p_.get(); }
  T* dev() const { return p_ ? dev_ : nullptr; }
  hipError_t alloc(size_t count) {
    T* p = nullptr;
    const hipError_t e = hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocMapped);
    if (e != hipSuccess) return e;
    p_.reset(p);
    for (size_t k = 0; k < count; k++) p[k] = T();
    return hipHostGetDevicePointer((void**)&dev_, p, 0);
  }
};

// a stream (flags 0: default, hipStreamNonBlocking), synchronised before it is destroyed / an event (flags 0: timing, hipEventDisableTiming)
template <class H, hipError_t (*Create)(H*, unsigned), class Destroy> class Created {
  std::unique_ptr<std::remove_pointer_t<H>, Destroy> h_;
 public:
  H get() const { return h_.get(); }
  hipError_t create(unsigned flags = 0) {
    H h = nullptr;
    const hipError_t e = Create(&h, flags);
    if (e == hipSuccess) h_.reset(h);
    return e;
  }
};
using Stream = Created<hipStream_t, hipStreamCreateWithFlags, DestroyStream>;
using Event = Created<hipEvent_t, hipEventCreateWithFlags, DestroyEvent>;
inline void sync(const Stream& s) { if (s.get()) (void)hipStreamSynchronize(s.get()); }   // (a stream that was never created: nothing)

// ---- what both handle types are: CassieVec and Cassie3dVec derive from this
struct Handle {
  int n = 0, device = 0;
  hipStream_t stream = nullptr;               // the caller's stream (CassieVecSetStream): kernels run here; not owned
  unsigned long long substeps_requested = 0;  // host: env-substeps asked for since the counters were last cleared
  std::string err;
};

inline int fail(Handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->err = buf;
  return code;
}

#define HIPCHK(h, call)                                                                                          \
  do {                                                                                                           \
    hipError_t e_ = (call);                                                                                      \
    if (e_ != hipSuccess) return cassie_host::fail(h, CASSIE_EHIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// ---- two streams side by side
// fork: every stream of `to` waits for what is queued on `from` so far.  false: the fork could not be set up -- the caller then runs that
// work on `from` itself rather than let it race with what `from` still has queued.
inline bool fork(hipStream_t from, hipEvent_t ev, std::initializer_list<hipStream_t> to) {
  if (hipEventRecord(ev, from) != hipSuccess) return false;
  for (hipStream_t s : to)
    if (hipStreamWaitEvent(s, ev, 0) != hipSuccess) return false;
  return true;
}
// join: `into` continues behind what is queued on `from`.  If the event cannot be recorded / waited for, the hard way: the host waits for
// `from`; false then (the caller stops forking).
inline bool join(hipStream_t into, hipEvent_t ev, hipStream_t from) {
  if (hipEventRecord(ev, from) == hipSuccess && hipStreamWaitEvent(into, ev, 0) == hipSuccess) return true;
  (void)hipStreamSynchronize(from);
  return false;
}

// ---- shared by the two ABIs
// the opening of a Create: CASSIE_OK with `device` current, else the code to return
inline int open_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    fprintf(stderr, "libcassie2d: no HIP device available; this library has no CPU path\n");
    return CASSIE_ENODEVICE;
  }
  if (device < 0 || device >= ndev) return CASSIE_EINVAL;
  return hipSetDevice(device) == hipSuccess ? CASSIE_OK : CASSIE_EHIP;
}

inline int synchronize(Handle* h) {
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return CASSIE_OK;
}
// the copies of the *Host conveniences, `count` elements on the handle's stream (followed by synchronize()); a null host destination is skipped
template <class T> int to_device(Handle* h, T* dev, const T* host, size_t count) {
  HIPCHK(h, hipMemcpyAsync(dev, host, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
  return CASSIE_OK;
}
template <class T> int to_host(Handle* h, T* host, const T* dev, size_t count) {
  if (host) HIPCHK(h, hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, h->stream));
  return CASSIE_OK;
}

// device event counters: N words to the host (synchronises the stream) / cleared with the host's count of requested substeps
template <int N> int read_counters(Handle* h, const unsigned long long* stats, unsigned long long (&host)[N]) {
  HIPCHK(h, hipSetDevice(h->device));
  if (int rc = to_host(h, host, stats, N)) return rc;
  return synchronize(h);
}
inline int reset_counters(Handle* h, unsigned long long* stats, int n_words) {
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemsetAsync(stats, 0, n_words * sizeof(unsigned long long), h->stream));
  h->substeps_requested = 0;
  return CASSIE_OK;
}

// average device time (ms, events on the handle's stream) of `steps` calls of step() back to back
template <class Step> int timed_steps(Handle* h, hipEvent_t ev0, hipEvent_t ev1, int steps, float* avg_ms, Step step) {
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventRecord(ev0, h->stream));
  for (int i = 0; i < steps; i++)
    if (int rc = step()) return rc;
  HIPCHK(h, hipEventRecord(ev1, h->stream));
  HIPCHK(h, hipEventSynchronize(ev1));
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, ev0, ev1));
  *avg_ms = ms / steps;
  return CASSIE_OK;
}

// an on / off environment variable: 0 or 1 by its first character, -1 when unset or anything else
inline int env_switch(const char* name) {
  const char* e = getenv(name);
  return e && (e[0] == '0' || e[0] == '1') ? e[0] - '0' : -1;
}

}  // namespace cassie_host
CASSIE_HOST_PRIVATE_END
#endif
