// Shared host-side plumbing of libscaldpc (error string, HIP check macro).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../include/scaldpc.h"

namespace scaldpc {

std::string &last_error();
int fail(int code, const char *fmt, ...);

#define SC_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return ::scaldpc::fail(e__ == hipErrorOutOfMemory ? SCALDPC_ENOMEM : SCALDPC_EHIP, \
                                   "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__),   \
                                   __FILE__, __LINE__);                                      \
    } while (0)

#define SC_TRY(expr)            \
    do {                        \
        int rc__ = (expr);      \
        if (rc__) return rc__;  \
    } while (0)

// Device / pinned-host memory through a small per-process cache of released blocks
// (scaldpc_bp.hip): the reference builds a NEW decoder for every decode (hqc.py:694), and a
// handle's ~20 hipMalloc / hipFree pairs (hipFree synchronises the device) cost several times
// the decode itself.  Blocks up to 64 MiB are parked on release (at most 512 MiB in total,
// scaldpc_trim() returns them to the driver, SCALDPC_NO_CACHE=1 disables the cache); larger
// ones go straight to hipMalloc / hipFree.  Memory comes back uninitialised either way.
int cached_alloc(void **p, size_t bytes, bool pinned_host);
void cached_free(void *p);
// While alive on a thread, released blocks go to hipFree / hipHostFree (which wait for the
// device) instead of the cache: used when a handle may have asynchronous work in flight.
struct CacheBypass {
    explicit CacheBypass(bool on);
    ~CacheBypass();
    bool prev;
};

// Every entry point that takes a handle runs on the handle's device whatever the calling thread's
// current device is (allocations, streams and launches all follow the current device), and puts
// the caller's device back on return.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int device)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// Streams of destroyed handles are parked per device and handed to the next handle created there.
int stream_acquire(hipStream_t *out, int *device);
void stream_release(hipStream_t s, int device);

// Host memory for a handle's graph mirrors and tables, through a small per-process pool of released blocks.  The
// reference builds a NEW decoder for every decode (hqc.py:694), i.e. a few multi-megabyte std::vectors are allocated and
// freed per decode; glibc hands such sizes to mmap / trims the heap top on free, so the next decoder page-faults every
// byte again -- and depending on what else the process (Python, NumPy) has on the heap this flips between 0.45 ms and
// 2-8 ms per construction plus 1.5 ms per destroy (measured: profiles/r03/rebuild_probe.log).  Blocks of at least 32 KiB
// are parked on release (at most 256 MiB in total; scaldpc_trim() returns them); smaller requests go to operator new.
void *host_pool_alloc(size_t bytes);
void host_pool_free(void *p, size_t bytes) noexcept;

template <typename T>
struct PoolAlloc {
    using value_type = T;
    PoolAlloc() noexcept = default;
    template <typename U>
    PoolAlloc(const PoolAlloc<U> &) noexcept {}
    T *allocate(size_t n) { return static_cast<T *>(host_pool_alloc(n * sizeof(T))); }
    void deallocate(T *p, size_t n) noexcept { host_pool_free(p, n * sizeof(T)); }
    template <typename U>
    bool operator==(const PoolAlloc<U> &) const noexcept { return true; }
    template <typename U>
    bool operator!=(const PoolAlloc<U> &) const noexcept { return false; }
};
template <typename T>
using pvec = std::vector<T, PoolAlloc<T>>;

// One block of cached_alloc, owned: released (cached_free) by reset() and the destructor.  cap() is the element count
// last requested; a request for 0 elements still takes one.  A failed request leaves the buffer empty with capacity 0, so
// the next call retries.  Nothing here zeroes the memory or synchronises.  The buffer converts to T *, so kernel
// launches and pointer arithmetic read as with a plain pointer.
template <typename T, bool Pinned = false>
class Buf {
public:
    Buf() = default;
    Buf(Buf &&o) noexcept : p_(o.p_), cap_(o.cap_)
    {
        o.p_ = nullptr;
        o.cap_ = 0;
    }
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(cap_, o.cap_);
        }
        return *this;
    }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { reset(); }

    operator T *() const { return p_; }
    T *get() const { return p_; }
    size_t cap() const { return cap_; }

    void reset()
    {
        if (p_) cached_free((void *)p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // room for `need` elements; else the block is released and `alloc` (>= need) elements are requested
    int ensure(size_t need, size_t alloc)
    {
        if (p_ && need <= cap_) return 0;
        reset();
        return request(alloc, &p_, &cap_);
    }
    int ensure(size_t need) { return ensure(need, need); }
    // room for `need` elements with the first `used` kept: the new block of `alloc` elements is requested and filled
    // before the old one is released; a failed request or copy leaves the old block in place
    int grow_keep(size_t used, size_t need, size_t alloc)
    {
        if (need <= cap_) return 0;
        Buf q;
        SC_TRY(request(alloc, &q.p_, &q.cap_));
        if (used) {
            const hipError_t e = hipMemcpy(q.p_, p_, used * sizeof(T), hipMemcpyDeviceToDevice);
            if (e != hipSuccess) return fail(SCALDPC_EHIP, "copy into the grown buffer failed: %s", hipGetErrorString(e));
        }
        *this = std::move(q);
        return 0;
    }

private:
    static int request(size_t count, T **p, size_t *cap)
    {
        void *q = nullptr;
        SC_TRY(cached_alloc(&q, std::max<size_t>(count, 1) * sizeof(T), Pinned));
        *p = (T *)q;
        *cap = count;
        return 0;
    }
    T *p_ = nullptr;
    size_t cap_ = 0;
};
template <typename T>
using PinnedBuf = Buf<T, true>;

}  // namespace scaldpc
