// ifa_buf.h -- the two owning buffer types of the per-device worker (ifa_engine_state.h).  No HIP here: a memory space is a policy
//   struct Space { static int alloc(void **p, size_t bytes); static void free(void *p); };
// whose alloc returns 0 or an ifa_fail code (message recorded: the failing call and its error).  ifa_buf_hip.h has the device and
// pinned spaces; tests/buf_selftest.cc runs the types over malloc.
#pragma once
#include <cstddef>

namespace ifa {

template <class T> struct buf_elem { static constexpr size_t bytes = sizeof(T); };
template <> struct buf_elem<void> { static constexpr size_t bytes = 1; };      // Buf<void, ...>: a capacity in bytes

// One block of `cap()` elements.  Move-only; reads as a T * wherever one is expected (kernel parameters, pointer arithmetic, tests
// for null), so the code that uses a buffer does not know it is owned.
template <class T, class Space> class Buf {
    T *p_ = nullptr;
    size_t cap_ = 0;
public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~Buf() { reset(); }
    // frees what it holds, then allocates n elements; on failure: empty, capacity 0, the space's error code
    int alloc(size_t n)
    {
        reset();
        void *q = nullptr;
        const int rc = Space::alloc(&q, n * buf_elem<T>::bytes);
        if (rc) return rc;
        p_ = static_cast<T *>(q); cap_ = q ? n : 0;
        return 0;
    }
    void reset()
    {
        if (p_) Space::free(p_);
        p_ = nullptr; cap_ = 0;
    }
    operator T *() const { return p_; }
    template <class U> explicit operator U *() const { return (U *)p_; }      // (const half_t *)buf, as with the raw pointer
    T *get() const { return p_; }
    size_t cap() const { return cap_; }
};

// A device block and its pinned staging block, one capacity: both at >= n elements, or nothing.  reserve() does not wait for any
// stream: a caller whose old pair may still be in use synchronises first.
template <class T, class DevSpace, class PinSpace> struct Staged {
    Buf<T, DevSpace> dev;
    Buf<T, PinSpace> pin;
    size_t cap() const { return pin.cap(); }
    int reserve(size_t n)
    {
        if (n <= cap()) return 0;
        int rc = dev.alloc(n);
        if (!rc) rc = pin.alloc(n);
        if (rc) reset();
        return rc;
    }
    void reset() { dev.reset(); pin.reset(); }
};

} // namespace ifa
