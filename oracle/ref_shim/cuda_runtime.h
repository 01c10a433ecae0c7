/*
 * oracle/ref_shim/cuda_runtime.h -- a host stand-in for the CUDA runtime.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/ref_build.py).  With it the reference's
 * .cu and .cpp files compile as plain C++ and run on the CPU: a kernel is an
 * ordinary function of the thread-local threadIdx / blockIdx, a launch is a
 * loop over the grid, device memory is host memory.  The reference's kernels
 * use no shared memory, no atomics and no warp intrinsics, and no thread
 * reads what another thread of the same launch writes, so the order in which
 * the "threads" run does not matter.
 *
 * Every standard header the reference or this shim needs is included here,
 * before windows.h (this directory) defines the min / max macros.
 */
#ifndef REF_SHIM_CUDA_RUNTIME_H
#define REF_SHIM_CUDA_RUNTIME_H

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <typeinfo>
#include <vector>

#define __global__
#define __device__
#define __host__

typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind {
    cudaMemcpyHostToHost = 0,
    cudaMemcpyHostToDevice = 1,
    cudaMemcpyDeviceToHost = 2,
    cudaMemcpyDeviceToDevice = 3,
    cudaMemcpyDefault = 4
};

struct uint3 {
    unsigned x, y, z;
};
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};

/* defined once, in oracle/ref_harness.cpp */
extern thread_local uint3 threadIdx, blockIdx;
extern thread_local dim3 blockDim, gridDim;

/* cudaMalloc: exactly `size` zeroed bytes, so that a host AddressSanitizer
 * build sees the same bounds a device allocation has. */
inline cudaError_t cudaMalloc(void** p, size_t size) {
    *p = calloc(1, size);
    return cudaSuccess;
}
inline cudaError_t cudaFree(void* p) {
    free(p);
    return cudaSuccess;
}
inline cudaError_t cudaMemcpy(void* dst, const void* src, size_t n, cudaMemcpyKind) {
    memmove(dst, src, n);
    return cudaSuccess;
}
inline cudaError_t cudaSetDevice(int) { return cudaSuccess; }
inline cudaError_t cudaGetLastError() { return cudaSuccess; }
inline cudaError_t cudaPeekAtLastError() { return cudaSuccess; }
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline cudaError_t cudaDeviceReset() { return cudaSuccess; }
inline const char* cudaGetErrorString(cudaError_t) { return "no error"; }

namespace ref_shim {

/* Worker threads of a launch: REF_SHIM_THREADS, else min(16, cores). */
inline unsigned max_threads() {
    static const unsigned n = [] {
        if (const char* e = getenv("REF_SHIM_THREADS")) {
            const int v = atoi(e);
            if (v > 0) return (unsigned)v;
        }
        const unsigned hc = std::thread::hardware_concurrency();
        return hc == 0 ? 1u : (hc > 16u ? 16u : hc);
    }();
    return n;
}

/* A launch: every block of the grid, every thread of the block, one after
 * another.  Large grids are cut into runs of consecutive blocks, one host
 * thread each; the indices are thread-local, so the kernels cannot tell. */
template <class K>
struct launch {
    K kernel;
    dim3 grid, block;

    template <class... A>
    void run(unsigned long long lo, unsigned long long hi, A&... a) const {
        gridDim = grid;
        blockDim = block;
        for (unsigned long long b = lo; b < hi; b++) {
            blockIdx.x = (unsigned)(b % grid.x);
            blockIdx.y = (unsigned)((b / grid.x) % grid.y);
            blockIdx.z = (unsigned)(b / ((unsigned long long)grid.x * grid.y));
            for (unsigned tz = 0; tz < block.z; tz++)
                for (unsigned ty = 0; ty < block.y; ty++)
                    for (unsigned tx = 0; tx < block.x; tx++) {
                        threadIdx.x = tx;
                        threadIdx.y = ty;
                        threadIdx.z = tz;
                        kernel(a...);  /* by value, as a kernel receives its arguments */
                    }
        }
    }

    template <class... A>
    void operator()(A... a) const {
        const unsigned long long blocks = (unsigned long long)grid.x * grid.y * grid.z;
        unsigned long long nt = max_threads();
        if (nt > blocks / 4) nt = blocks / 4;  /* at least four blocks a thread */
        if (nt <= 1) {
            run(0, blocks, a...);
            return;
        }
        std::vector<std::thread> pool;
        for (unsigned long long t = 0; t < nt; t++)
            pool.emplace_back([&, t] { run(blocks * t / nt, blocks * (t + 1) / nt, a...); });
        for (auto& th : pool) th.join();
    }
};

template <class K>
launch<K> make_launch(K k, dim3 g, dim3 b) {
    return launch<K>{k, g, b};
}

}  // namespace ref_shim

/* oracle/ref_build.py rewrites `k <<< g, b >>> (args)` to REF_LAUNCH(k, g, b)(args). */
#define REF_LAUNCH(k, g, b) ref_shim::make_launch((k), dim3(g), dim3(b))

#endif
