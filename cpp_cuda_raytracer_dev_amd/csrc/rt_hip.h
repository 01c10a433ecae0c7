// rt_hip.h -- the host code's HIP helpers (rt_api.cpp, tile_order.cpp): error
// mapping, device allocations, the current-device guard.
#pragma once

#include "rt_internal.h"

namespace rt {

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

inline int hip_check(hipError_t e, const char* what) {
    if (e == hipSuccess) return RT_OK;
    return fail(e == hipErrorOutOfMemory ? RT_ERR_NOMEM : RT_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

template <class T>
int dev_alloc(T** p, size_t count, const char* what) {
    *p = nullptr;
    if (count == 0) count = 1;
    return hip_check(hipMalloc((void**)p, sizeof(T) * count), what);
}

template <class T>
void dev_free(T*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}

}  // namespace rt
