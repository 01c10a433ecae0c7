// rt_light_dispatch.hip -- the instances of k_light_kd3 (rt_light_over's
// visibility pass for a list of lights; count x push order) and of
// k_shade_lights (rt_shade_lights), with their launchers, in a translation
// unit of their own so they compile beside the KD kernels' (build.py).
// the header's other kernels are launched from rt_kernels.hip; unused here
#pragma clang diagnostic ignored "-Wunused-function"
#include "rt_kernels_impl.h"

namespace rt {

int launch_light_over(const TraceParams& p, bool count, void* stream) {
    const unsigned grid = (unsigned)(p.tiles_x * p.block_rows);
    if (grid == 0) return RT_OK;
    TraceFn fn = count ? light_kernel<true>(p.any_order) : light_kernel<false>(p.any_order);
    fn<<<grid, 64u * (unsigned)kd3_waves(16), 0, (hipStream_t)stream>>>(p);
    return check_launch<void>("k_light_kd3");
}

int launch_shade_lights(const TraceParams& p, void* stream) {
    const unsigned grid = (unsigned)(p.tiles_x * p.block_rows);
    if (grid == 0) return RT_OK;
    k_shade_lights<kTileH><<<grid, 8u * kTileH, 0, (hipStream_t)stream>>>(p);
    return check_launch<void>("k_shade_lights");
}

}  // namespace rt
