// frame_geom.h -- the launch geometry of a frame: which walks may take the
// kFast forms, the tiling, the fine / coarse split with its far rectangle,
// the rays per wave, and the gather rectangle every rank derives alike.  Pure
// host arithmetic over a FrameGeom, no HIP and no camera, so a CPU program
// (tests/frame_geom_main.cpp) runs it under a sanitizer.  The camera's side
// (camera_geom, the caches, fill_params) is rt_api.cpp's.
#pragma once

#include <stdint.h>

#include <utility>
#include <vector>

#include "rt_params.h"
#include "tile_order_host.h"

namespace rt {

// The identity object transform (a null xform).
extern const float kIdentXf[12];

// Everything the launch geometry (tiling, fine region, frame rectangle)
// depends on: a device camera's fields (camera_geom) or the host-only inputs
// of rt_frame_rect_host, so both derive the same rectangle by one code path.
struct FrameGeom {
    int32_t w = 0, h = 0;
    const float* n_mod = nullptr;
    const float* u_mod = nullptr;
    const float* v_mod = nullptr;
    float root_box[6] = {0, 0, 0, 0, 0, 0};  // camera-relative root box
    bool root_leaf = false;
    int kernel = 3, rays = 0, coarse = 8, debug = 0;
    bool multiframe = false;  // renders of rt_run_frames' multi-frame launches (auto_rays)
    // groups holding a pixel with a tiny ray component (find_tiny_groups):
    // the camera's cached list, or computed by the caller
    const std::vector<std::pair<int32_t, int32_t>>* tiny = nullptr;
    // renders only (fill_params): the fine region the camera holds for this
    // tiling (hold_region), or null for the exact region
    Hold* hold = nullptr;
    int32_t cam_flags = kCamUnordered;  // k_cam_nodes' flags of the camera's records (renders only)
};

// The geometry inputs of rt_frame_rect_host: `in`'s fields (g points into
// it) and its tiny-ray groups, computed into `tiny`.
FrameGeom host_geom(const rt_frame_geometry& in, std::vector<std::pair<int32_t, int32_t>>& tiny);

// Groups with a pixel whose unnormalised primary ray q = n + u*x + v*y (the
// kernels' float expression) has a component of magnitude <= 1e-30: their
// slab tests may see 0/0 = NaN, so they never take the far-group shortcut.
void tiny_groups_of(int32_t w, int32_t h, const float* n, const float* u, const float* v,
                    std::vector<std::pair<int32_t, int32_t>>& out);

// The launch geometry of one render: camera basis, transform, tiling, and
// the fine / far split (set_fine_region).  Returns whether the far groups
// are fused into the fine kernel (every pixel outside the fine region is
// then provably background: a far wave that finds otherwise sets error 4).
bool frame_geometry(const FrameGeom& g, const float* xform, const rt_tile* tile, uint32_t mode, TraceParams& p);

// The rectangle from the geometry inputs alone (the device camera's, or the
// host-only ones of rt_frame_rect_host): every rank's tiling, as its render
// would derive it.
void frame_rect_geom(const FrameGeom& g, bool kd_tree, const float* xform, uint32_t mode, int32_t nranks,
                     int32_t rect[4]);

}  // namespace rt
