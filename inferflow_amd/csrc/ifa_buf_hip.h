// ifa_buf_hip.h -- the worker's buffer types (ifa_buf.h) over HIP device memory and pinned host memory.
//
// Both spaces count what they hand out and can be told to fail: ifa_debug_alloc_fail_at / ifa_debug_live_allocs
// (include/inferflow_amd.h) are test hooks over that counter and countdown; nothing else reads them.  A failed allocation records
// "hipMalloc(N bytes) failed: <error>" (hipHostMalloc for the pinned space) and returns IFA_ERR_HIP.  Definitions: ifa_engine.hip.
#pragma once
#include "ifa_host.h"
#include "ifa_buf.h"

namespace ifa {

struct DevSpace { static int alloc(void **p, size_t bytes); static void free(void *p); };
struct PinSpace { static int alloc(void **p, size_t bytes); static void free(void *p); };

template <class T> using DevBuf = Buf<T, DevSpace>;
template <class T> using PinBuf = Buf<T, PinSpace>;
template <class T> using DevPin = Staged<T, DevSpace, PinSpace>;

// an event the worker creates on first use and keeps until it goes
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};

} // namespace ifa
