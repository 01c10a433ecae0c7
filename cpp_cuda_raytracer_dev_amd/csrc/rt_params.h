// rt_params.h -- TraceParams, the kernels' argument block, which the launch
// geometry (frame_geom.cpp) fills on the host.  No HIP include: a translation
// unit that has seen HIP's headers (rt_internal.h includes them first) gets
// their float4 / float2; a plain C++ one (frame_geom.cpp,
// tests/frame_geom_main.cpp) only ever holds pointers to them, so the two
// types are declared opaque there.
#pragma once

#include <stdint.h>

#include "../../include/rt_mi355x.h"
#include "rt_tile_consts.h"

#ifndef HIP_INCLUDE_HIP_HIP_RUNTIME_H
struct float2;
struct float4;
#endif

namespace rt {

struct TraceParams {
    const float4* inode;
    const float4* trec;
    const float4* tpair;           // flat variant 2: triangle pairs (k_pair_tri), or null
    const float4* shade;
    uint32_t* argb;
    int64_t* hit;
    // rt_render_display: the frame the reference's window shows
    // (TD/WinMain.cpp:212-237), or null: argb holds the previous frame's
    // clean buffer on entry; a hit pixel shows this frame's Phong, a miss
    // keeps the previous clean value (color_cam_cuda writes rmi >= 0 only)
    uint32_t* display;
    unsigned long long* counters;  // 5 x u64 or null
    int32_t* err;                  // device error word
    float n_mod[3], u_mod[3], v_mod[3];
    float xf[12];
    int32_t w, h;
    int32_t nranks, rank;
    int32_t frame_out;             // RT_FLAG_FRAME_OUT: tile pixels at their frame rows
    int32_t tiles_x, block_rows;   // fine grid = tiles_x * block_rows blocks
    // Fine region (kernel 3): the tiles covering the root box's screen
    // rectangle start at tile column fine_tx0 and band slot fine_s0; every
    // other 8x8 group of this rank's bands is a coarse group, handled
    // `coarse_per_wave` to a wave after the fine blocks (exact either way:
    // a coarse group runs the same root test and traces what passes).
    int32_t fine_tx0, fine_s0;
    int32_t groups_x, nslots;      // 8-px groups per row, band slots of this rank
    int32_t cg_x0, cg_x1;          // fine region in 8-px groups [x0, x1)
    int32_t cs0, cs1;              // fine region in slots [s0, s1)
    int32_t coarse_per_wave;       // coarse groups per wave
    int32_t any_order;             // push order of any-hit (shadow) walks 0..3, +4: counted walks stop at occluders
    int32_t coarse_blocks;         // blocks of k_coarse_kd3
    int32_t fill_blocks;           // blocks after the fine grid filling far groups (fused mode)
    int64_t coarse_groups;         // total coarse groups
    int32_t plain_xf;              // object transform is the identity (rotation 1, offset 0)
    // kernel 3's kFast walks apply (frame_geom.cpp fast_proof): ordered boxes,
    // and every box's entry parameter >= 2^-20 for every ray of the frame
    // (any rotation; with an offset the translated walks take xfast_slot)
    int32_t fast;
    // shadow walks (round 6): the translated kFast slots apply to a shadow
    // ray that points to side sh_neg (1: negative) of axis sh_axis with
    // normal, nonzero components (frame_geom.cpp fast_proof_shadow)
    int32_t fast_sh, sh_axis, sh_neg;
    uint32_t leaf_off;             // byte offset of trec from inode (one allocation; rt_api.cpp prepare_camera_object)
    // bytes of that allocation's records (inode + trec; < 4 GiB when leaf_off is
    // set).  No kernel reads it; it keeps its slot because the fields after it
    // moving up changes the register allocation of the untranslated KD kernels
    uint32_t rec_bytes;
    int32_t tiny_s1;               // some interior record of the camera has the tiny-s1 flag
    int32_t far_rect[4];           // root box's screen rectangle + 2 px (x0, x1, y0, y1; frame pixels)
    int32_t far_all;               // every group background: the box lies behind the eye (box_behind)
    int32_t tile_w, tile_h;        // pixels per block (tile_h divides the 8-row band)
    int32_t rays;                  // pixels (rays) per wave: 32, 16 or 8
    int32_t tile_order;            // Option kOptTileOrder
    const int32_t* order;          // tile permutation (tile_order 2: centre-out, 3: by cost)
    // kernel 3, tile order 3 (16- and 8-ray units): order[0..split) render as
    // two halves (2 blocks per tile)
    int32_t split;
    uint32_t* cost;                // tile_order 3: pool iterations per fine unit [tile][kCostSlots], or null
    float root_box[6];             // camera-relative root AABB (t0x,t1x,t0y,t1y,t0z,t1z)
    int32_t pool_cap;              // kernel 3 item-pool capacity in use (<= kPoolCap)
    int32_t items;                 // kernel 3 items per lane per iteration (1 or 2)
    int32_t debug;                 // diagnostic builds only: 1 = skip traversal
    unsigned long long* dbg;       // per-wave (t_start, t_end, visits) when non-null
    // diagnostic builds (-DRT_VMEM_STATS=1) with debug bit 16384: record-load
    // statistics per walk form (rt_kernels_impl.h vmem_stat), or null
    unsigned long long* vstat;
    // A multi-frame launch (kernel 3; pf_frames > 0): pf_frames frames of
    // pf_blocks blocks each in one grid, frame-major; frame f writes
    // pf_argb[(pf_seq0 + f) % pf_nbuf].
    int32_t pf_frames, pf_blocks, pf_seq0, pf_nbuf;
    uint32_t* pf_argb[RT_LOOP_MAX_BUF];
    uint32_t root_ref;
    uint32_t ntri;
    int32_t max_depth;
    int32_t tree_height;           // the scene tree's height (kernel 3's pool slack is height + 1)
    // kernel 3's two-level iterations: the deepest node depth whose children
    // are interior records at positions 2i + 1, 2i + 2 (-1: off)
    int32_t two_depth;
    int32_t flat_variant;          // Option kOptFlat: flat-list kernel form (9 or 12)
    // the chunked flat form (12, non-counting renders): per-pixel (w bits,
    // triangle) minima of the chunks, all ones between frames; and the chunk count
    unsigned long long* flat_key;
    int32_t flat_chunks;
    // RT_FLAG_WRITE_AOV: ten float planes of aov_stride pixels each (d, pnt,
    // norm, rad of the nearest hit: Camera::pixel_memory, TD/Camera.h:50-59),
    // written by the write-hit instances next to the hit index; null = off.
    // Last in the struct, so every earlier member keeps its kernel-argument
    // offset and the instances that never read it stay as they were.
    float* aov;
    int64_t aov_stride;
    // rt_render_over (after the planes for the same reason): a pixel is
    // written only where it is a hit nearer than plane 0's d, with hit_base
    // added to its triangle index; every other pixel gets no store.  Read by
    // the write-hit instances alone (hit_base is 0 in every other render).
    int32_t over;
    int64_t hit_base;
    // A tree whose s1 / s2 fields are not its children's bounds on the cut
    // axis (k_cam_nodes' kCamSplitFields; no builder makes one): the fields,
    // camera-relative, per interior record, for the walks that otherwise read
    // the split planes from the record's child boxes; null for every other
    // tree.  Last for the same reason as the planes.
    const float2* split_planes;
    // rt_shadow_over (k_shadow_kd3 alone reads it; last for the same reason):
    // the object's own pixels, hit_base <= hit < hit_base + ntri, are not tested
    int32_t shadow_skip_own;
    // rt_light_over / rt_shade_lights (k_light_kd3 and k_shade_lights alone
    // read them; last for the same reason): the camera's light list on the
    // device, nlights x (Lx, Ly, Lz, I), 1 <= nlights <= RT_LIGHTS_MAX
    const float* lights;
    int32_t nlights;
};

// Blocks of k_trace_kd3's grid (fine tiles, split extras, far fill).
inline unsigned fine_grid_blocks(const TraceParams& p) {
    return (unsigned)(p.tiles_x * p.block_rows) + (unsigned)p.split + (unsigned)p.fill_blocks;
}

}  // namespace rt
