// rt_internal.h -- shared between the host C++ (scene_host.cpp, rt_api.cpp, tile_order.cpp)
// and the HIP kernels (rt_kernels.hip).  Device-side data layouts live here
// and in rt_params.h (TraceParams).
#pragma once

// (before rt_params.h, which then uses HIP's float4 / float2)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_params.h"
#include "rt_tile_consts.h"

namespace rt {

// Error plumbing for rt_last_error_string (thread-local message).
int fail(int code, const char* fmt, ...);

// Leaf references in the traversal: a set top bit means "leaf; the low bits
// are a triangle index", otherwise the low bits index the dense interior-node
// array.  Trees are limited to < 2^31 triangles.
constexpr uint32_t kLeafBit = 0x80000000u;

// Traversal stack entries per lane kept in LDS.  The reference sizes the
// per-pixel stack ceil(log2(nvox)) (TD/Camera.cpp:202-203), which is exactly
// the maximum DFS occupancy of its balanced median tree; 24 covers 2^23 tris.
constexpr int kMaxDepth = 24;

// Interior record (64 B) of the KD layout: the two children's
// camera-relative boxes plus this node's split thresholds and child references.
//   r0 = (L.t0x, L.t1x, L.t0y, L.t1y)   r1 = (L.t0z, L.t1z, R.t0x, R.t1x)
//   r2 = (R.t0y, R.t1y, R.t0z, R.t1z)   r3 = (S_gt, S_lt, Lref | axis << 29, Rref | tiny_s1 << 29)
// (k_cam_nodes: S_gt / S_lt are the exact float forms of the reference's
// double tests against s2; s1 = L's high and s2 = R's low bound on the axis.)
constexpr uint32_t kRefMask = 0x1FFFFFFFu;
constexpr uint32_t kAxisShift = 29;
constexpr uint32_t kTinyS1Bit = 1u << 29;
// (k_cam_nodes' flags of a camera's records, kCam*: rt_tile_consts.h)

// rt_camera_set_option keys.
enum Option : int32_t {
    kOptKernel = 1,     // KD kernel: 2 (per-lane DFS in the reference's order) or 3 (item pool, default)
    kOptTileOrder = 2,  // 0 XCD-contiguous, 1 natural, 2 centre-out, 3 by measured cost (kernel 3)
    kOptRays = 3,       // kernel 3 pixels per wave: 32, 16 or 8 (0 = auto)
    kOptItems = 4,      // kernel 3 items popped per lane per iteration: 1 or 2
    kOptCoarse = 5,     // kernel 3 coarse groups per wave outside the root box's rectangle (0 = off)
    kOptShadowOrder = 6,  // kernel 3 any-hit push order 0..3, -1 = timed choice (default)
    kOptFlat = 7,       // flat-list kernel: 9 one pass, 12 the list in 16 chunks (default)
    kOptRaysUsed = 8,   // get only: pixels per wave of the last kernel-3 render
    kOptSplitUsed = 9,  // get only: split tiles at the head of the current cost order (kernel 3)
    // 10, 11: retired (ABI 2; round 4's coop-used and frame-group keys)
    kOptFastUsed = 12,  // get only: which walks of the last kernel-3 render took the kFast forms (bit mask)
    kOptOrderRestores = 13,  // get only: kept cost orders restored (TileOrder::restore_order)
    kOptFineTiles = 14,  // get only: fine tiles (one kRays unit per wave) of the last kernel-3 render
    kOptDebug = 100,    // diagnostics: 1 = skip traversal, 2 = per-wave timestamps, 4 = every group
                        // coarse, 8 = coarse kernel on a side stream beside the fine one,
                        // 16 = counted shadow walks stop at occluders (the timed walk's work),
                        // 32 = counting renders stop after the root test, 64 = order / cost
                        // buffers sized for the current grid only, 256 = no held fine region,
                        // 512 = no split tiles, 1024 = no two-level iterations, 2048 = no kFast walks,
                        // 8192 = no clipped rectangle for a root box at the eye's depth,
                        // 16384 = record-load statistics (diagnostic builds, RT_VMEM_STATS)
    kOptPoolCap = 101,  // tests: shrink kernel 3's item pool (66..kPoolCap) to force its fallback
};
constexpr int kPoolCapMax = 640;

// ---------------------------------------------------------------------------
// Device layouts (all 16-byte aligned, read with dwordx4 loads).
//
// Interior records: above (kRefMask, kAxisShift), camera-relative, one per
// interior node (init_cam_voxel_mem_cuda, TD/Camera.cu:137-162).
//
// TriRecord (64 B), camera-relative, one per triangle, indexed by
// tri_list_index (init_tri_mem_cuda + init_cam_tri_mem_cuda,
// TD/Trixel.cu:11-36):
//   (e1x, e1y, e1z, e2x) (e2y, e2z, dtx, dty) (dtz, dqx, dqy, dqz) (dw, 0, 0, 0)
//
// Shade (32 B), one per triangle: (nx, ny, nz, 0) (r, g, b, 0)
// ---------------------------------------------------------------------------

}  // namespace rt

// Kernel launchers (rt_kernels.hip), all stream-ordered.
namespace rt {
int launch_tri_world(const float* points9, const float* rad3, uint32_t ntri,
                     float4* tri_world, float4* shade, void* stream);
int launch_cam_tri(const float4* tri_world, uint32_t ntri, const float pos[3],
                   float4* trec, void* stream);
int launch_pair_tri(const float4* trec, uint32_t ntri, float4* tpair, void* stream);
int launch_cam_nodes(const rt_kd_node* nodes, const int32_t* interior_ids,
                     const uint32_t* node_ref, int64_t ninterior, const float pos[3],
                     float4* inode, int32_t* flags, float2* split_planes, void* stream);
// part: the coarse groups then the fine tiles (kPartAll), or one of them.
enum LaunchPart : int { kPartAll = 0, kPartFine = 1, kPartCoarse = 2 };
int launch_trace(const TraceParams& p, uint32_t mode, uint32_t flags, int kernel_version,
                 void* stream, int part);
// rt_shadow_over's pass (rt_shadow_dispatch.hip): k_shadow_kd3 over the
// tiles_x * block_rows tiles of p, push order p.any_order.
int launch_shadow_over(const TraceParams& p, bool count, void* stream);
// rt_light_over's pass (rt_light_dispatch.hip): k_light_kd3 over the same
// grid for p.nlights lights; and rt_shade_lights' k_shade_lights, one 8 x 8
// tile per 64-thread block over the tiles_x * block_rows tiles of p.
int launch_light_over(const TraceParams& p, bool count, void* stream);
int launch_shade_lights(const TraceParams& p, void* stream);
// Camera-relative box of one world node, exactly as init_cam_voxel_mem_cuda.
void camera_relative_box(const rt_kd_node& nd, const float pos[3], float out[6]);
// KD build on the GPU (kd_build_gpu.hip).  The median tree's shape depends
// on the triangle count alone: per node its position range [l, r], median m,
// first child (-1 for a leaf) and parent; level k = nodes [level[k], level[k+1]).
struct KdShape {
    std::vector<int32_t> l, m, r, left, parent;
    std::vector<int64_t> level;
    int32_t height = 0;
};
void kd_shape(uint32_t n, KdShape& out);
// The node array of rt_kd_build, built on the current device into d_nodes
// (2n-1 entries); synchronises `stream`.
int kd_build_device(const rt_leaf_aabb* h_leafs, uint32_t n, const KdShape& shape, rt_kd_node* d_nodes, void* stream);
// Traversal refs: kLeafBit | tri for leaves, record position for interior ids.
int launch_node_ref(const rt_kd_node* d_nodes, int64_t nnode, const int32_t* d_ids, int64_t ninterior,
                    uint32_t* d_ref, void* stream);
// rt_kd_build's input checks: tri indices a permutation of [0, n), no NaN bound.
int validate_leafs(const rt_leaf_aabb* leafs, uint32_t n, const char* what);
int launch_unpack(int32_t w, int32_t h, int32_t nranks, const uint32_t* gathered,
                  uint32_t* frame, void* stream);
// rt_render_clear: the miss state (background, hit -1, d = 400, zeros) into
// the pixels a render of (nranks, rank, frame_out) addresses; hit may be null.
int launch_clear(int32_t w, int32_t h, int32_t nranks, int32_t rank, bool frame_out, uint32_t* argb, int64_t* hit,
                 float* aov, int64_t aov_stride, void* stream);
// Slots s of `rank` whose band rank + s*nranks lies in [b0, b1): [s0, s1).
__host__ __device__ inline void rect_slots(int32_t b0, int32_t b1, int32_t nranks, int32_t rank,
                                           int32_t& s0, int32_t& s1) {
    s0 = b0 <= rank ? 0 : (b0 - rank + nranks - 1) / nranks;
    s1 = b1 <= rank ? 0 : (b1 - 1 - rank) / nranks + 1;
    if (s1 < s0) s1 = s0;
}
// rect = (x0, x1, b0, b1): columns [x0, x1) of bands [b0, b1) (rt_frame_rect).
int launch_pack_rect(int32_t w, int32_t h, int32_t nranks, int32_t rank, const int32_t rect[4],
                     const uint32_t* local, uint32_t* out, void* stream);
int launch_unpack_rect(int32_t w, int32_t h, int32_t nranks, const int32_t rect[4], const uint32_t* local0,
                       const uint32_t* peers, uint32_t* frame, void* stream,
                       bool rect_only = false);
// rt_comm_gather_frame; rect_only: d_frame already holds this rectangle's
// background (an earlier gather of the same rectangle into it), so rank 0
// writes the rectangle alone.
int comm_gather_frame(rt_comm* c, rt_camera* cam, const float* xform, uint32_t mode, const uint32_t* d_local,
                      uint32_t* d_scratch, uint32_t* d_frame, void* stream, bool rect_only, int32_t rect_out[4]);
}  // namespace rt
