// A device buffer that owns its allocation (host API only: no kernels_common.h, so that a host program can include it).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace viprs {

// `n` is the capacity of `p` in elements, never a request: a failed allocation leaves the buffer EMPTY (p null, n 0), so
// that "n >= need" never vouches for a null pointer when the caller tries again with the same object.
template <typename V> struct DevBuf {
    V* p = nullptr;
    size_t n = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    // `dev_malloc(void**, bytes)`: hipMalloc, or a stand-in (tests/dev_buf_state.cpp)
    template <typename Malloc> hipError_t alloc_with(size_t count, Malloc&& dev_malloc) {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        if (count == 0) return hipSuccess;
        void* q = nullptr;
        const hipError_t e = dev_malloc(&q, count * sizeof(V));
        if (e != hipSuccess || !q) return e != hipSuccess ? e : hipErrorOutOfMemory;
        p = static_cast<V*>(q);
        n = count;
        return hipSuccess;
    }
    hipError_t alloc(size_t count) {
        return alloc_with(count, [](void** q, size_t bytes) { return hipMalloc(q, bytes); });
    }
    // room for at least `count` elements: a buffer that is large enough stays as it is
    template <typename Malloc> hipError_t reserve_with(size_t count, Malloc&& dev_malloc) {
        if (count == 0 || (p && n >= count)) return hipSuccess;
        return alloc_with(count, dev_malloc);
    }
    hipError_t reserve(size_t count) {
        return reserve_with(count, [](void** q, size_t bytes) { return hipMalloc(q, bytes); });
    }
};

}  // namespace viprs
