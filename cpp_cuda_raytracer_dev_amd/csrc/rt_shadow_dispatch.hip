// rt_shadow_dispatch.hip -- the instances of k_shadow_kd3 (rt_shadow_over's
// deferred shadow pass; count x push order) and their launcher, in a
// translation unit of their own so they compile beside the KD kernels'
// (build.py).
// the header's other kernels are launched from rt_kernels.hip; unused here
#pragma clang diagnostic ignored "-Wunused-function"
#include "rt_kernels_impl.h"

namespace rt {

int launch_shadow_over(const TraceParams& p, bool count, void* stream) {
    const unsigned grid = (unsigned)(p.tiles_x * p.block_rows);
    if (grid == 0) return RT_OK;
    TraceFn fn = count ? shadow_kernel<true>(p.any_order) : shadow_kernel<false>(p.any_order);
    fn<<<grid, 64u * (unsigned)kd3_waves(16), 0, (hipStream_t)stream>>>(p);
    return check_launch<void>("k_shadow_kd3");
}

}  // namespace rt
