// rt_api.cpp -- the C ABI (include/rt_mi355x.h) over the HIP runtime.
//
// Handles own every device buffer they allocate and free it in rt_*_destroy
// (the reference never frees: TD/Camera.cpp:143-210, TD/Trixel.h:90-124).
// Every launch is stream-ordered and checked with hipGetLastError; nothing on
// the render path synchronises or allocates, so a caller may capture
// rt_render_into in a hipGraph.
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "rt_hip.h"
#include "rt_internal.h"
#include "tile_order.h"
// (after rt_internal.h: HIP's headers come before rt_params.h)
#include "frame_geom.h"

using namespace rt;

struct rt_scene {
    int device = 0;
    uint32_t ntri = 0;
    float4* d_tri_world = nullptr;   // (p1, e1, e2, n) per triangle
    float4* d_shade = nullptr;       // (n, rad) per triangle
    rt_kd_node* d_nodes = nullptr;   // world-space tree as uploaded
    int32_t* d_interior_ids = nullptr;
    uint32_t* d_node_ref = nullptr;
    int64_t nnode = 0, ninterior = 0;
    uint32_t root_ref = 0;
    int32_t height = 0;
    uint64_t tree_version = 0;
    rt_kd_node root{};               // host copy of node 0 (root box)
    // host shape of the tree (left child or -1 for a leaf), kept to re-lay
    // the interior records out (rt_scene_set_option)
    std::vector<int32_t> h_left;
    int record_order = 0;            // RT_SCENE_ORDER: 0 BFS, 1 DFS preorder, 2 treelets
    int treelet_height = 3;          // RT_SCENE_TREELET_HEIGHT
    // kernel 3's two-level iterations (two_level_depth): the deepest node
    // depth whose children are interior records at 2i + 1, 2i + 2, or -1
    int32_t two_depth = -1;
};

struct rt_camera {
    int device = 0;
    int32_t w = 0, h = 0;
    float pos[3] = {0, 0, 0};
    rt_camera_basis_t basis{};
    uint32_t* d_argb = nullptr;
    int64_t* d_hit = nullptr;
    // RT_FLAG_WRITE_AOV: the caller's planes (rt_camera_set_aov) or the
    // camera's own, allocated by the first render that needs them; and the
    // hit target of such a render whose caller passed none (the planes ride
    // on the write-hit kernel instances)
    float* aov_bound = nullptr;
    int64_t aov_bound_stride = 0;
    float* d_aov = nullptr;
    bool aov_filled = false;         // a flagged render wrote d_aov (rt_read_aov)
    int64_t* d_aov_hit = nullptr;
    unsigned long long* d_counters = nullptr;
    int32_t* d_err = nullptr;
    // rt_camera_set_lights: the light list (Lx, Ly, Lz, I) x nlights, its host
    // copy and the device copy rt_light_over / rt_shade_lights read; no other
    // entry point looks at it (their light is the literal (2, 2, 2))
    float lights[4 * RT_LIGHTS_MAX] = {2.0f, 2.0f, 2.0f, 1.0f};
    int32_t nlights = 1;
    float* d_lights = nullptr;
    rt_scene* obj = nullptr;
    uint64_t prepared_version = 0;
    float4* d_trec = nullptr;        // camera-relative triangle records
    float4* d_inode = nullptr;       // camera-relative interior nodes
    float2* d_split = nullptr;       // a tree with kCamSplitFields: its s1 / s2 fields per interior record
    int64_t split_cap = 0;
    int32_t* d_cam_flags = nullptr;  // k_cam_nodes' flags (kCamTinyS1, kCamUnordered) ...
    int32_t cam_flags = kCamUnordered;  // ... read back once the records are built
    float4* d_tpair = nullptr;       // flat variant 2: camera-relative triangle pairs
    uint32_t trec_cap = 0;
    // d_inode and d_trec are one allocation, the interior records first, so
    // kernel 3's kFast walks address both from d_inode with a 32-bit byte
    // offset (leaf_off: the byte offset of d_trec; 0 when the records exceed
    // 4 GiB, and then no kFast walk runs)
    float4* d_rec = nullptr;
    int64_t rec_cap = 0;             // in float4
    uint32_t leaf_off = 0;
    // kOptKernel: the KD kernel a render runs.  Every kernel handles any tree
    // the LDS stack admits (height <= kMaxDepth; rt_scene_set_kd rejects
    // taller ones): kernel 3's marked path codes take height + 1 <= 25 bits.
    int kernel_version = 3;
    int tile_order = 3;              // kOptTileOrder
    // kOptDebug (diagnostics): 1 skip traversal, 2 per-wave stamps, 4 every
    // group coarse, 8 coarse kernel on a side stream, 16 counted shadow walks
    // stop at occluders, 32 counting renders of kernel 3 stop after the root
    // test, 64 order / cost buffers sized for the current grid only
    int debug = 0;
    int pool_cap = kPoolCapMax;      // kOptPoolCap
    unsigned long long* d_dbg = nullptr;
    int64_t dbg_cap = 0;             // in u64
    TileOrder order;                 // tile dispatch orders, cost feedback, the held fine region
    int coarse = 8;                  // kOptCoarse: coarse groups per wave (0 = off)
    bool multiframe = false;         // inside rt_run_frames' multi-frame launches (auto_rays)
    // 8x8 groups (x / 8, y / 8) holding a pixel whose primary ray has a zero
    // or tiny component (computed once, as the kernels compute the rays)
    std::vector<std::pair<int32_t, int32_t>> tiny_groups;
    bool tiny_done = false;
    // kernel 3: the coarse groups run on a side stream beside the fine tiles
    // (disjoint pixels), forked from and joined back into the caller's stream
    hipStream_t side = nullptr;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    int rays = 0;                    // kOptRays: pixels per wave of kernel 3 (0: auto_rays)
    int last_rays = 0;               // the pixels per wave the last kernel-3 render used
    int last_fast = 0;               // whether it took the kFast walks (fast_proof)
    int64_t last_fine = 0;           // kOptFineTiles: fine tiles of the last kernel-3 render
    int items = 2;                   // kOptItems: items per lane per pool iteration
    int flat_variant = 12;           // kOptFlat: flat-list kernel form
    // chunked flat forms: one per-pixel key buffer per stream that renders
    // (frames in flight use several), all ones between frames
    struct FlatKeys {
        hipStream_t stream = nullptr;
        unsigned long long* d = nullptr;
        int64_t cap = 0;
    };
    FlatKeys flat_keys[8];
    // shadow renders: the any-hit push order, fixed (kOptShadowOrder 0..3)
    // or timed (-1): a round of trial frames runs each order kTuneReps times,
    // interleaved, bracketed by events; the fastest is kept for kTunePeriod
    // frames, then the next round starts (the view may have changed).
    int shadow_order = -1;
    int any_best = 1;
    int tune_next = 0;               // next trial frame of the round; kTuneTrials = round queued
    int tune_frames = 0;             // frames since the last round's result
    bool tune_pending = false;
    hipEvent_t tune_ev[2 * 12] = {};
    // Frame loops render the same (transform, tile, buffers) frame after
    // frame: its launch geometry is kept and reused while nothing it depends
    // on changed.  The one rule: whatever changes an input of the geometry
    // other than the key's own terms bumps geom_gen before a cache is next
    // consulted -- rt_camera_set_option, the multi-frame rays rule
    // (run_frames_multiframe), and prepare_camera_object, which every render
    // and rt_frame_rect call first and which bumps it whenever the object or
    // its tree (tree_version) is not the one it last prepared.  So the key
    // carries no tree term, and rt_camera_add_object bumps nothing itself.
    uint64_t geom_gen = 1;
    struct GeomKey {
        bool valid = false;
        uint64_t gen = 0;
        float xf[12];
        uint32_t mode = 0;
        int32_t nranks = 0;
        bool matches(uint64_t g, const float* x, uint32_t m, int32_t nr) const {
            return valid && gen == g && mode == m && nranks == nr && !memcmp(xf, x, sizeof xf);
        }
        void set(uint64_t g, const float* x, uint32_t m, int32_t nr) {
            valid = true;
            gen = g;
            memcpy(xf, x, sizeof xf);
            mode = m;
            nranks = nr;
        }
    };
    struct ParamCache {
        GeomKey key;
        int32_t rank = 0;
        TraceParams p;               // its argb / hit are set per call
    } pcache;
    // rt_run_frames with frames in flight: the library's own render lanes
    // (and, with a gather, its comm lane), each a stream created after the
    // caller's, so on hardware queues of its own while queues are free.
    // While a loop runs, `active` lists the lanes frames are issued to: a
    // timed trial frame of the shadow push order then waits for all of them
    // and they wait for it (render_common).  (A cost-order upload waits for
    // the streams that launched with its slot, which TileOrder records.)
    hipStream_t lanes[RT_LOOP_MAX_LANES + 1] = {};
    hipEvent_t lane_ev[RT_LOOP_MAX_LANES + 1] = {};
    int nactive = 0;
    hipStream_t active[RT_LOOP_MAX_LANES] = {};
    // rt_run_frames: events kept across calls (the timed call reuses the
    // warm-up call's), pairs bracketing sampled frames' renders
    std::vector<hipEvent_t> loop_ev;
    struct RectCache {
        GeomKey key;
        int32_t rect[4];
    } rcache;
};

namespace {

int prepare_camera_object(rt_camera* c) {
    rt_scene* s = c->obj;
    if (!s) return fail(RT_ERR_STATE, "camera has no object (rt_camera_add_object)");
    if (c->prepared_version == s->tree_version + 1) return RT_OK;
    int rc;
    // The records are rewritten in place (on the null stream) whenever they
    // fit the buffers the camera has: frames of the previous object or tree
    // still in flight on the caller's streams would walk them half written
    // (a smaller scene after a larger one; hipFree waits only when they grow)
    if ((rc = hip_check(hipDeviceSynchronize(), "camera object prep: frames in flight"))) return rc;
    const int64_t nint4 = std::max<int64_t>(s->d_nodes ? s->ninterior : 0, 1) * 4, ntri4 = (int64_t)s->ntri * 4;
    if (c->rec_cap < nint4 + ntri4) {
        dev_free(c->d_rec);
        c->d_rec = c->d_inode = c->d_trec = nullptr;
        c->rec_cap = 0;
        if ((rc = dev_alloc(&c->d_rec, (size_t)(nint4 + ntri4), "hipMalloc(records)"))) return rc;
        c->rec_cap = nint4 + ntri4;
    }
    c->d_inode = c->d_rec;
    c->d_trec = c->d_rec + nint4;
    c->leaf_off = (nint4 + ntri4) * 16 < (int64_t)UINT32_MAX ? (uint32_t)(nint4 * 16) : 0u;
    if (c->trec_cap < s->ntri) {
        dev_free(c->d_tpair);
        if ((rc = dev_alloc(&c->d_tpair, (size_t)((s->ntri + 1) / 2) * 8, "hipMalloc(tpair)"))) return rc;
        c->trec_cap = s->ntri;
    }
    // init_camera_trixel_device_memory (TD/Trixel.cu:244-264), plus its pair
    // layout for the packed flat-list kernel
    if ((rc = launch_cam_tri(s->d_tri_world, s->ntri, c->pos, c->d_trec, nullptr)) ||
        (rc = launch_pair_tri(c->d_trec, s->ntri, c->d_tpair, nullptr)))
        return rc;
    if (s->d_nodes) {
        if (!c->d_cam_flags && (rc = dev_alloc(&c->d_cam_flags, 1, "hipMalloc(cam flags)"))) return rc;
        // init_camera_voxel_device_memory (TD/Camera.cu:163-187)
        if ((rc = hip_check(hipMemset(c->d_cam_flags, 0, sizeof(int32_t)), "memset cam flags")) ||
            (rc = launch_cam_nodes(s->d_nodes, s->d_interior_ids, s->d_node_ref, s->ninterior, c->pos,
                                   c->d_inode, c->d_cam_flags, nullptr, nullptr)))
            return rc;
    }
    if ((rc = hip_check(hipDeviceSynchronize(), "camera object prep"))) return rc;
    c->cam_flags = 0;
    if (s->d_nodes && s->ninterior > 0 &&
        (rc = hip_check(hipMemcpy(&c->cam_flags, c->d_cam_flags, sizeof(int32_t), hipMemcpyDeviceToHost), "D2H cam flags")))
        return rc;
    if (c->cam_flags & kCamSplitFields) {
        // the fields of a tree whose split planes are not its boxes' bounds: a
        // second pass writes them beside the records (TraceParams::split_planes)
        if (c->split_cap < s->ninterior) {
            dev_free(c->d_split);
            c->d_split = nullptr;
            c->split_cap = 0;
            if ((rc = dev_alloc(&c->d_split, (size_t)s->ninterior, "hipMalloc(split planes)"))) return rc;
            c->split_cap = s->ninterior;
        }
        if ((rc = launch_cam_nodes(s->d_nodes, s->d_interior_ids, s->d_node_ref, s->ninterior, c->pos, c->d_inode,
                                   c->d_cam_flags, c->d_split, nullptr)) ||
            (rc = hip_check(hipDeviceSynchronize(), "camera split planes")))
            return rc;
    }
    c->geom_gen++;  // cached launch parameters carry the flags
    // kept cost orders measured another object or tree: a grid
    // of the same key must not restart from them (the camera's position is
    // fixed at rt_camera_create, so this covers every input of a cost order)
    c->order.forget_kept();
    c->prepared_version = s->tree_version + 1;
    return RT_OK;
}

constexpr int kAnyOrders = 4, kTuneReps = 3, kTuneTrials = kAnyOrders * kTuneReps;
constexpr int kTunePeriod = 2048;  // frames between timing rounds of the shadow push order

void find_tiny_groups(rt_camera* c) {
    if (c->tiny_done) return;
    tiny_groups_of(c->w, c->h, c->basis.n_mod, c->basis.u_mod, c->basis.v_mod, c->tiny_groups);
    c->tiny_done = true;
}

// The geometry inputs of a device camera (its object prepared).
FrameGeom camera_geom(rt_camera* c) {
    FrameGeom g;
    g.w = c->w;
    g.h = c->h;
    g.n_mod = c->basis.n_mod;
    g.u_mod = c->basis.u_mod;
    g.v_mod = c->basis.v_mod;
    camera_relative_box(c->obj->root, c->pos, g.root_box);
    g.root_leaf = (c->obj->root_ref & kLeafBit) != 0;
    g.kernel = c->kernel_version;
    g.rays = c->rays;
    g.multiframe = c->multiframe;
    g.coarse = c->coarse;
    g.debug = c->debug;
    find_tiny_groups(c);
    g.tiny = &c->tiny_groups;
    g.cam_flags = c->cam_flags;
    return g;
}

bool frame_geometry(rt_camera* c, const float* xform, const rt_tile* tile, uint32_t mode, TraceParams& p) {
    FrameGeom g = camera_geom(c);
    g.hold = &c->order.hold;  // renders keep a held fine region (rt_frame_rect does not)
    return frame_geometry(g, xform, tile, mode, p);
}

int fill_params(rt_camera* c, const float* xform, const rt_tile* tile, uint32_t* argb, int64_t* hit,
                uint32_t mode, TraceParams& p, hipStream_t st) {
    const rt_scene* s = c->obj;
    p.inode = c->d_inode;
    p.split_planes = (c->cam_flags & kCamSplitFields) ? c->d_split : nullptr;
    p.trec = c->d_trec;
    p.leaf_off = c->leaf_off;
    p.rec_bytes = c->leaf_off ? (uint32_t)(c->leaf_off + 64 * (uint64_t)c->obj->ntri) : 0u;
    p.tpair = c->d_tpair;
    p.flat_variant = c->flat_variant;
    p.shade = s->d_shade;
    p.argb = argb;
    p.hit = hit;
    p.counters = c->d_counters;
    p.err = c->d_err;
    const int kernel = mode == RT_MODE_KD ? c->kernel_version : 0;
    (void)frame_geometry(c, xform, tile, mode, p);
    p.root_ref = s->root_ref;
    p.ntri = s->ntri;
    p.max_depth = kMaxDepth;
    p.tree_height = s->height;
    // debug bit 1024: one-level iterations only
    p.two_depth = (c->debug & 1024) ? -1 : s->two_depth;
    p.tile_order = c->tile_order;
    p.split = 0;
    p.debug = c->debug;
    p.pool_cap = c->pool_cap;
    p.items = c->items;
    p.dbg = nullptr;
    p.vstat = nullptr;
    if ((c->debug & 16384) && !(c->debug & 2)) {
        // record-load statistics (diagnostic builds): 32 counters, read with
        // rt_camera_debug_read; they accumulate until the option is set again
        if (c->dbg_cap < 32) {
            dev_free(c->d_dbg);
            int rc = dev_alloc(&c->d_dbg, 32, "hipMalloc(dbg)");
            if (rc) return rc;
            c->dbg_cap = 32;
            if ((rc = hip_check(hipMemset(c->d_dbg, 0, sizeof(uint64_t) * 32), "memset vstat"))) return rc;
        }
        p.vstat = c->d_dbg;
    }
    if (c->debug & 2) {
        // (fine tiles twice: a split tile adds a block)
        const int64_t need = (2 * (int64_t)p.tiles_x * p.block_rows + p.coarse_blocks + p.fill_blocks) * 4 * 3;
        if (c->dbg_cap < need) {
            dev_free(c->d_dbg);
            int rc = dev_alloc(&c->d_dbg, (size_t)need, "hipMalloc(dbg)");
            if (rc) return rc;
            c->dbg_cap = need;
        }
        p.dbg = c->d_dbg;
        int rc = hip_check(hipMemset(c->d_dbg, 0, sizeof(uint64_t) * (size_t)need), "memset dbg");
        if (rc) return rc;
    }
    return c->order.prepare(p, kernel, st, &p.order, &p.cost);
}

int check_tile(const rt_tile* tile) {
    if (tile && (tile->nranks < 1 || tile->rank < 0 || tile->rank >= tile->nranks))
        return fail(RT_ERR_INVALID, "rt_tile: rank %d of %d", tile->rank, tile->nranks);
    return RT_OK;
}

// The device error word: 1 = DFS stack overflow (kernels 1-2), 2 = item pool
// overflow (kernel 3), 4 = a fused far group that was not far (kernel 3),
// 8 = a tile order entry outside the fine grid (kernel 3; the block skipped).
int device_error(int32_t err) {
    return fail(RT_ERR_OVERFLOW, "device reported %s%s%s%s", (err & 1) ? "[traversal stack overflow]" : "",
                (err & 2) ? "[item pool overflow]" : "", (err & 4) ? "[far-group check failed]" : "",
                (err & 8) ? "[tile order out of range]" : "");
}

}  // namespace

extern "C" int rt_device_count(int* count) {
    if (!count) return fail(RT_ERR_INVALID, "rt_device_count: null");
    return hip_check(hipGetDeviceCount(count), "hipGetDeviceCount");
}

extern "C" int rt_scene_create(int device, const float* points9, const float* rad3, uint32_t ntri,
                               rt_scene** out) {
    if (!out || (ntri && (!points9 || !rad3))) return fail(RT_ERR_INVALID, "rt_scene_create: null argument");
    if (ntri > kRefMask) return fail(RT_ERR_INVALID, "rt_scene_create: more than 2^29 triangles");
    *out = nullptr;
    DeviceGuard g(device);
    if (!g.ok) return fail(RT_ERR_HIP, "rt_scene_create: hipSetDevice(%d) failed", device);
    rt_scene* s = new rt_scene();
    s->device = device;
    s->ntri = ntri;
    float *d_pts = nullptr, *d_rad = nullptr;
    int rc;
    if ((rc = dev_alloc(&s->d_tri_world, (size_t)ntri * 3, "hipMalloc(tri_world)")) ||
        (rc = dev_alloc(&s->d_shade, (size_t)ntri * 2, "hipMalloc(shade)")) ||
        (rc = dev_alloc(&d_pts, (size_t)ntri * 9, "hipMalloc(points)")) ||
        (rc = dev_alloc(&d_rad, (size_t)ntri * 3, "hipMalloc(rad)")) ||
        (rc = hip_check(hipMemcpy(d_pts, points9, sizeof(float) * 9 * ntri, hipMemcpyHostToDevice), "H2D points")) ||
        (rc = hip_check(hipMemcpy(d_rad, rad3, sizeof(float) * 3 * ntri, hipMemcpyHostToDevice), "H2D rad")) ||
        (rc = launch_tri_world(d_pts, d_rad, ntri, s->d_tri_world, s->d_shade, nullptr)) ||
        (rc = hip_check(hipDeviceSynchronize(), "init_tri_mem"))) {
        dev_free(d_pts);
        dev_free(d_rad);
        rt_scene_destroy(s);
        return rc;
    }
    dev_free(d_pts);
    dev_free(d_rad);
    *out = s;
    return RT_OK;
}

namespace {

// The order of the dense interior records.  Internal: a record names its
// children by position, the traversal's tie rule uses DFS path codes, so the
// frame never depends on it; only the cache locality of the walk does.
//   0  BFS (node index order, as the reference stores kd_tree_node)
//   1  DFS preorder, left child first: a node's first child is the next record
//   2  treelets of height H: a node and its descendants down to H-1 levels
//      below it are consecutive (BFS inside), treelets in DFS order
std::vector<int32_t> interior_order(const std::vector<int32_t>& left, int order, int h) {
    std::vector<int32_t> ids;
    const int64_t n = (int64_t)left.size();
    if (n == 0 || left[0] < 0) return ids;
    ids.reserve((size_t)(n / 2));
    if (order == 0) {
        for (int64_t i = 0; i < n; i++)
            if (left[(size_t)i] >= 0) ids.push_back((int32_t)i);
        return ids;
    }
    if (order == 1) {
        std::vector<int32_t> st{0};
        while (!st.empty()) {
            const int32_t i = st.back();
            st.pop_back();
            if (left[(size_t)i] < 0) continue;
            ids.push_back(i);
            st.push_back(left[(size_t)i] + 1);
            st.push_back(left[(size_t)i]);
        }
        return ids;
    }
    std::vector<int32_t> roots{0}, level, next, below;
    while (!roots.empty()) {
        const int32_t r = roots.back();
        roots.pop_back();
        level.assign(1, r);
        below.clear();
        for (int d = 0; d < h && !level.empty(); d++) {
            next.clear();
            for (int32_t i : level) {
                ids.push_back(i);
                for (int32_t c : {left[(size_t)i], left[(size_t)i] + 1})
                    if (left[(size_t)c] >= 0) (d + 1 < h ? next : below).push_back(c);
            }
            level.swap(next);
        }
        // child treelets left to right: push in reverse so the leftmost pops first
        for (auto it = below.rbegin(); it != below.rend(); ++it) roots.push_back(*it);
    }
    return ids;
}

// Kernel 3's two-level iterations load a node's children's records before
// its own record has arrived, at interior positions 2i + 1 and 2i + 2 of the
// node's position i.  Returns the deepest depth d such that every interior
// node at depth <= d has two interior children at exactly those positions
// (true for the top levels of the reference's tree in BFS record order: its
// shape depends on n alone, a range of s triangles splitting into ceil(s/2)
// and floor(s/2), so every node above depth floor(log2 n) - 1 is interior),
// or -1 when the root's children are not (DFS or treelet orders, tiny trees).
int32_t two_level_depth(const std::vector<int32_t>& left, const std::vector<int32_t>& ids) {
    const int64_t n = (int64_t)left.size();
    if (n == 0 || left[0] < 0) return -1;
    std::vector<int32_t> pos((size_t)n, -1), depth((size_t)n, 0);
    for (size_t k = 0; k < ids.size(); k++) pos[(size_t)ids[k]] = (int32_t)k;
    int32_t bad = INT32_MAX, height = 0;
    for (int64_t i = 0; i < n; i++) {
        const int32_t L = left[(size_t)i];
        if (L < 0) continue;
        const int32_t R = L + 1, d = depth[(size_t)i];
        depth[(size_t)L] = depth[(size_t)R] = d + 1;
        height = std::max(height, d + 1);
        const bool ok = left[(size_t)L] >= 0 && left[(size_t)R] >= 0 &&
                        (int64_t)pos[(size_t)L] == 2 * (int64_t)pos[(size_t)i] + 1 &&
                        (int64_t)pos[(size_t)R] == 2 * (int64_t)pos[(size_t)i] + 2;
        if (!ok) bad = std::min(bad, d);
    }
    return bad == INT32_MAX ? height : bad - 1;
}

// (Re)builds the interior record order and the node -> ref table (on the
// device, from the uploaded nodes).
int relabel(rt_scene* s) {
    const int64_t n = (int64_t)s->h_left.size();
    const std::vector<int32_t> ids = interior_order(s->h_left, s->record_order, s->treelet_height);
    DeviceGuard g(s->device);
    dev_free(s->d_interior_ids);
    dev_free(s->d_node_ref);
    int rc;
    if ((rc = dev_alloc(&s->d_interior_ids, ids.size(), "hipMalloc(ids)")) ||
        (rc = dev_alloc(&s->d_node_ref, (size_t)n, "hipMalloc(node_ref)")) ||
        (!ids.empty() && (rc = hip_check(hipMemcpy(s->d_interior_ids, ids.data(), sizeof(int32_t) * ids.size(),
                                                   hipMemcpyHostToDevice), "H2D ids"))) ||
        (rc = launch_node_ref(s->d_nodes, n, s->d_interior_ids, (int64_t)ids.size(), s->d_node_ref, nullptr)) ||
        (rc = hip_check(hipMemcpy(&s->root_ref, s->d_node_ref, sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H root ref")))
        return rc;
    s->ninterior = (int64_t)ids.size();
    s->two_depth = two_level_depth(s->h_left, ids);
    s->tree_version++;
    return RT_OK;
}

}  // namespace

extern "C" int rt_scene_set_kd(rt_scene* s, const rt_kd_node* nodes, uint64_t nnode) {
    if (!s || !nodes) return fail(RT_ERR_INVALID, "rt_scene_set_kd: null argument");
    const int64_t n = (int64_t)nnode;
    if (s->ntri == 0 || n != 2 * (int64_t)s->ntri - 1)
        return fail(RT_ERR_INVALID, "rt_scene_set_kd: %lld nodes for %u triangles", (long long)n, s->ntri);
    // Validate: BFS order with right = left + 1 (so every DFS terminates),
    // leaves cover every triangle exactly once, bounded height.
    std::vector<int32_t> left((size_t)n, -1);
    std::vector<uint8_t> seen(s->ntri, 0);
    std::vector<int32_t> depth((size_t)n, 0);
    int32_t height = 0;
    for (int64_t i = 0; i < n; i++) {
        const rt_kd_node& nd = nodes[i];
        if (nd.is_leaf) {
            if (nd.tri_index < 0 || nd.tri_index >= (int64_t)s->ntri || seen[(size_t)nd.tri_index])
                return fail(RT_ERR_INVALID, "rt_scene_set_kd: leaf %lld has bad/duplicate triangle", (long long)i);
            seen[(size_t)nd.tri_index] = 1;
        } else {
            if (nd.left <= i || nd.right != nd.left + 1 || nd.right >= n)
                return fail(RT_ERR_INVALID, "rt_scene_set_kd: node %lld children %lld/%lld not BFS", (long long)i,
                            (long long)nd.left, (long long)nd.right);
            if (nd.cut_flag < 0 || nd.cut_flag > 5)
                return fail(RT_ERR_INVALID, "rt_scene_set_kd: node %lld cut_flag %d", (long long)i, nd.cut_flag);
            depth[(size_t)nd.left] = depth[(size_t)i] + 1;
            depth[(size_t)nd.right] = depth[(size_t)i] + 1;
            height = std::max(height, depth[(size_t)i] + 1);
            left[(size_t)i] = (int32_t)nd.left;
        }
    }
    if (height > kMaxDepth)
        return fail(RT_ERR_INVALID, "rt_scene_set_kd: tree height %d exceeds the %d-entry LDS stack", height, kMaxDepth);
    DeviceGuard g(s->device);
    dev_free(s->d_nodes);
    int rc;
    if ((rc = dev_alloc(&s->d_nodes, (size_t)n, "hipMalloc(nodes)")) ||
        (rc = hip_check(hipMemcpy(s->d_nodes, nodes, sizeof(rt_kd_node) * (size_t)n, hipMemcpyHostToDevice), "H2D nodes"))) {
        dev_free(s->d_nodes);
        return rc;
    }
    s->nnode = n;
    s->root = nodes[0];
    s->height = height;
    s->h_left.swap(left);
    if ((rc = relabel(s))) {
        dev_free(s->d_nodes);
        return rc;
    }
    return RT_OK;
}

extern "C" int rt_kd_build_gpu(int device, const rt_leaf_aabb* leafs, uint32_t ntri, rt_kd_node* nodes, void* stream) {
    if (!nodes) return fail(RT_ERR_INVALID, "rt_kd_build_gpu: null nodes");
    int rc = validate_leafs(leafs, ntri, "rt_kd_build_gpu");
    if (rc) return rc;
    DeviceGuard g(device);
    if (!g.ok) return fail(RT_ERR_HIP, "rt_kd_build_gpu: hipSetDevice(%d) failed", device);
    KdShape shape;
    kd_shape(ntri, shape);
    const int64_t nnode = 2 * (int64_t)ntri - 1;
    rt_kd_node* d = nullptr;
    if ((rc = dev_alloc(&d, (size_t)nnode, "hipMalloc(kd nodes)"))) return rc;
    rc = kd_build_device(leafs, ntri, shape, d, stream);
    if (!rc)
        rc = hip_check(hipMemcpy(nodes, d, sizeof(rt_kd_node) * (size_t)nnode, hipMemcpyDeviceToHost), "D2H kd nodes");
    dev_free(d);
    return rc;
}

extern "C" int rt_scene_build_kd(rt_scene* s, const rt_leaf_aabb* leafs, uint32_t ntri, void* stream) {
    if (!s) return fail(RT_ERR_INVALID, "rt_scene_build_kd: null scene");
    if (ntri != s->ntri)
        return fail(RT_ERR_INVALID, "rt_scene_build_kd: %u leaf boxes for %u triangles", ntri, s->ntri);
    int rc = validate_leafs(leafs, ntri, "rt_scene_build_kd");
    if (rc) return rc;
    KdShape shape;
    kd_shape(ntri, shape);
    if (shape.height > kMaxDepth)
        return fail(RT_ERR_INVALID, "rt_scene_build_kd: tree height %d exceeds the %d-entry LDS stack", shape.height,
                    kMaxDepth);
    DeviceGuard g(s->device);
    const int64_t nnode = 2 * (int64_t)ntri - 1;
    dev_free(s->d_nodes);
    if ((rc = dev_alloc(&s->d_nodes, (size_t)nnode, "hipMalloc(nodes)")) ||
        (rc = kd_build_device(leafs, ntri, shape, s->d_nodes, stream)) ||
        (rc = hip_check(hipMemcpy(&s->root, s->d_nodes, sizeof(rt_kd_node), hipMemcpyDeviceToHost), "D2H root"))) {
        dev_free(s->d_nodes);
        return rc;
    }
    s->nnode = nnode;
    s->height = shape.height;
    s->h_left.swap(shape.left);
    if ((rc = relabel(s))) {
        dev_free(s->d_nodes);
        return rc;
    }
    return RT_OK;
}

extern "C" int rt_scene_read_kd(rt_scene* s, rt_kd_node* nodes, uint64_t nnode) {
    if (!s || !nodes) return fail(RT_ERR_INVALID, "rt_scene_read_kd: null argument");
    if (!s->d_nodes || (int64_t)nnode != s->nnode)
        return fail(RT_ERR_INVALID, "rt_scene_read_kd: scene has %lld nodes, %llu requested", (long long)s->nnode,
                    (unsigned long long)nnode);
    DeviceGuard g(s->device);
    return hip_check(hipMemcpy(nodes, s->d_nodes, sizeof(rt_kd_node) * (size_t)nnode, hipMemcpyDeviceToHost), "D2H nodes");
}

extern "C" int rt_scene_set_option(rt_scene* s, int32_t key, int32_t value) {
    if (!s) return fail(RT_ERR_INVALID, "rt_scene_set_option: null scene");
    switch (key) {
    case RT_SCENE_ORDER:
        if (value < 0 || value > 2) return fail(RT_ERR_INVALID, "interior record order %d (0..2)", value);
        s->record_order = value;
        break;
    case RT_SCENE_TREELET_HEIGHT:
        if (value < 1 || value > 12) return fail(RT_ERR_INVALID, "treelet height %d (1..12)", value);
        s->treelet_height = value;
        break;
    default:
        return fail(RT_ERR_INVALID, "rt_scene_set_option: unknown key %d", key);
    }
    return s->h_left.empty() ? RT_OK : relabel(s);
}

extern "C" int rt_scene_get_option(const rt_scene* s, int32_t key, int32_t* value) {
    if (!s || !value) return fail(RT_ERR_INVALID, "rt_scene_get_option: null argument");
    switch (key) {
    case RT_SCENE_ORDER: *value = s->record_order; return RT_OK;
    case RT_SCENE_TREELET_HEIGHT: *value = s->treelet_height; return RT_OK;
    case RT_SCENE_TWO_LEVEL_DEPTH: *value = s->two_depth; return RT_OK;
    default: return fail(RT_ERR_INVALID, "rt_scene_get_option: unknown key %d", key);
    }
}

extern "C" int rt_camera_create(int device, int32_t w, int32_t h, float f_w, float f_h, float focal,
                                const float pos[3], const float look_at[3], const float up[3],
                                rt_camera** out) {
    if (!out) return fail(RT_ERR_INVALID, "rt_camera_create: null out");
    *out = nullptr;
    if (w <= 0 || h <= 0 || (int64_t)w * h > (int64_t)1 << 31)
        return fail(RT_ERR_INVALID, "rt_camera_create: bad resolution %dx%d", w, h);
    rt_camera_basis_t basis;
    int rc = rt_camera_basis(w, h, f_w, f_h, focal, pos, look_at, up, &basis);
    if (rc) return rc;
    DeviceGuard g(device);
    if (!g.ok) return fail(RT_ERR_HIP, "rt_camera_create: hipSetDevice(%d) failed", device);
    rt_camera* c = new rt_camera();
    c->device = device;
    c->w = w;
    c->h = h;
    for (int k = 0; k < 3; k++) c->pos[k] = pos[k];
    c->basis = basis;
    const size_t npix = (size_t)w * h;
    if ((rc = dev_alloc(&c->d_argb, npix, "hipMalloc(argb)")) ||
        (rc = dev_alloc(&c->d_hit, npix, "hipMalloc(hit)")) ||
        (rc = dev_alloc(&c->d_counters, 5, "hipMalloc(counters)")) ||
        (rc = dev_alloc(&c->d_err, 1, "hipMalloc(err)")) ||
        (rc = dev_alloc(&c->d_lights, 4 * RT_LIGHTS_MAX, "hipMalloc(lights)")) ||
        (rc = hip_check(hipMemcpy(c->d_lights, c->lights, sizeof c->lights, hipMemcpyHostToDevice), "H2D lights")) ||
        // init_cam_mem_cuda (TD/Camera.cu:97-110): frame zeroed, rmi = -1
        (rc = hip_check(hipMemset(c->d_argb, 0, npix * sizeof(uint32_t)), "memset argb")) ||
        (rc = hip_check(hipMemset(c->d_hit, 0xFF, npix * sizeof(int64_t)), "memset hit")) ||
        (rc = hip_check(hipMemset(c->d_counters, 0, 5 * sizeof(unsigned long long)), "memset counters")) ||
        (rc = hip_check(hipMemset(c->d_err, 0, sizeof(int32_t)), "memset err"))) {
        rt_camera_destroy(c);
        return rc;
    }
    *out = c;
    return RT_OK;
}

extern "C" int rt_camera_add_object(rt_camera* c, rt_scene* s) {
    if (!c || !s) return fail(RT_ERR_INVALID, "rt_camera_add_object: null argument");
    if (c->device != s->device) return fail(RT_ERR_INVALID, "rt_camera_add_object: camera and scene on different devices");
    DeviceGuard g(c->device);
    c->obj = s;
    c->prepared_version = 0;
    return prepare_camera_object(c);
}

// The any-hit push order of a shadow frame (TraceParams::any_order) and, on
// a trial frame, its index in the round (else -1).  Never blocks: the round's
// events are only queried, and nothing is timed while the stream is captured
// or when counting (the counting walk does not stop at occluders).
static int any_order_for(rt_camera* c, uint32_t flags, void* stream, int& trial) {
    trial = -1;
    if (!(flags & RT_FLAG_SHADOW)) return 0;
    if (c->shadow_order >= 0) return c->shadow_order;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if ((flags & RT_FLAG_COUNT) ||
        (hipStreamIsCapturing((hipStream_t)stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone))
        return c->any_best;
    if (c->tune_pending) {
        if (hipEventQuery(c->tune_ev[2 * kTuneTrials - 1]) != hipSuccess) return c->any_best;
        float best[kAnyOrders];
        for (int o = 0; o < kAnyOrders; o++) best[o] = 1e30f;
        for (int t = 0; t < kTuneTrials; t++) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, c->tune_ev[2 * t], c->tune_ev[2 * t + 1]) == hipSuccess)
                best[t % kAnyOrders] = std::min(best[t % kAnyOrders], ms);
        }
        int b = 0;
        for (int o = 1; o < kAnyOrders; o++)
            if (best[o] < best[b]) b = o;
        c->any_best = b;
        c->tune_pending = false;
        c->tune_frames = 0;
        c->tune_next = kTuneTrials;
        return c->any_best;
    }
    if (c->tune_next >= kTuneTrials) {
        if (++c->tune_frames < kTunePeriod) return c->any_best;
        c->tune_next = 0;
    }
    for (int k = 0; k < 2 * kTuneTrials; k++)
        if (!c->tune_ev[k] && hipEventCreate(&c->tune_ev[k]) != hipSuccess) return c->any_best;
    trial = c->tune_next++;
    return trial % kAnyOrders;
}

// The trace launches of one frame: the coarse kernel, then the fine one, on
// the caller's stream.  Debug bit 8 instead runs the coarse kernel on the
// camera's side stream beside the fine one (forked after the caller's
// earlier work, joined before its later work); measured slower, since its
// waves take the slots the heaviest fine tiles need.
static int launch_split(rt_camera* c, const TraceParams& p, uint32_t mode, uint32_t flags, void* stream) {
    const int kernel = c->kernel_version;
    if (p.coarse_blocks == 0 || p.tiles_x * p.block_rows == 0 || !(c->debug & 8))
        return launch_trace(p, mode, flags, kernel, stream, kPartAll);
    int rc;
    if (!c->side &&
        (rc = hip_check(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking), "side stream")))
        return rc;
    if (!c->fork_ev && (rc = hip_check(hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming), "fork event")))
        return rc;
    if (!c->join_ev && (rc = hip_check(hipEventCreateWithFlags(&c->join_ev, hipEventDisableTiming), "join event")))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = hip_check(hipEventRecord(c->fork_ev, st), "fork record")) ||
        (rc = launch_trace(p, mode, flags, kernel, stream, kPartFine)) ||
        (rc = hip_check(hipStreamWaitEvent(c->side, c->fork_ev, 0), "fork wait")) ||
        (rc = launch_trace(p, mode, flags, kernel, c->side, kPartCoarse)) ||
        (rc = hip_check(hipEventRecord(c->join_ev, c->side), "join record")) ||
        (rc = hip_check(hipStreamWaitEvent(st, c->join_ev, 0), "join wait")))
        return rc;
    return RT_OK;
}

// The key buffer of the chunked flat forms for renders on `stream` (at least
// `npix` keys): allocated all ones once, reset by every frame's shading.
static int flat_keys_for(rt_camera* c, hipStream_t stream, int64_t npix, unsigned long long** out) {
    rt_camera::FlatKeys* slot = nullptr;
    for (auto& k : c->flat_keys)
        if (k.d && k.stream == stream) slot = &k;
    if (!slot)
        for (auto& k : c->flat_keys)
            if (!k.d) {
                slot = &k;
                break;
            }
    if (!slot) {  // more streams than slots: start over once nothing uses them
        int rc = hip_check(hipDeviceSynchronize(), "flat keys sync");
        if (rc) return rc;
        for (auto& k : c->flat_keys) {
            dev_free(k.d);
            k = rt_camera::FlatKeys{};
        }
        slot = &c->flat_keys[0];
    }
    if (slot->cap < npix) {
        if (slot->d) {  // the stream's earlier frames may still use it
            int rc = hip_check(hipStreamSynchronize(stream), "flat keys sync");
            if (rc) return rc;
        }
        dev_free(slot->d);
        slot->d = nullptr;
        int rc = dev_alloc(&slot->d, (size_t)npix, "hipMalloc(flat keys)");
        if (!rc) rc = hip_check(hipMemsetAsync(slot->d, 0xFF, sizeof(unsigned long long) * (size_t)npix, stream),
                                "flat keys init");
        if (rc) return rc;
        slot->cap = npix;
    }
    slot->stream = stream;
    *out = slot->d;
    return RT_OK;
}

// rt_run_frames' multi-frame launches: `frames` frames in one grid, frame f
// into argb[(seq0 + f) % nbuf].
struct PersistArgs {
    int32_t frames, seq0, nbuf;
    uint32_t* const* argb;
};

// The planes of a RT_FLAG_WRITE_AOV render split over nranks: the bound
// buffer, which must hold the pixels such a render addresses (the packed band
// buffer under a tile of several ranks, else the frame), or the camera's own,
// whose stride holds the frame and any packed tile (every band, 8 rows each).
static int aov_target(rt_camera* c, int32_t nranks, bool frame_out, float** aov, int64_t* stride) {
    const int64_t npix = (int64_t)c->w * c->h;
    if (c->aov_bound) {
        const int64_t need = nranks > 1 && !frame_out ? rt_tile_packed_pixels(c->w, c->h, nranks) : npix;
        if (c->aov_bound_stride < need)
            return fail(RT_ERR_INVALID, "rt_render: plane stride %lld is below the %lld pixels this render writes",
                        (long long)c->aov_bound_stride, (long long)need);
        *aov = c->aov_bound;
        *stride = c->aov_bound_stride;
        return RT_OK;
    }
    *stride = rt_tile_packed_pixels(c->w, c->h, 1);
    if (!c->d_aov) {
        int rc = dev_alloc(&c->d_aov, (size_t)(RT_AOV_PLANES * *stride), "hipMalloc(aov)");
        if (rc) return rc;
    }
    c->aov_filled = true;
    *aov = c->d_aov;
    return RT_OK;
}

static int render_common(rt_camera* c, const float* xform, uint32_t mode, uint32_t flags, const rt_tile* tile,
                         uint32_t* argb, int64_t* hit, void* stream, uint32_t* display = nullptr,
                         const PersistArgs* pf = nullptr, int32_t* rendered = nullptr, const int64_t* over_base = nullptr) {
    if (rendered) *rendered = 1;
    if (!c) return fail(RT_ERR_INVALID, "rt_render: null camera");
    if (mode != RT_MODE_KD && mode != RT_MODE_FLAT) return fail(RT_ERR_INVALID, "rt_render: mode %u", mode);
    int rc = check_tile(tile);
    if (rc) return rc;
    if (!argb || ((flags & RT_FLAG_WRITE_HIT) && !hit)) return fail(RT_ERR_INVALID, "rt_render: null output buffer");
    DeviceGuard g(c->device);
    if ((rc = prepare_camera_object(c))) return rc;
    if (mode == RT_MODE_KD && !c->obj->d_nodes)
        return fail(RT_ERR_STATE, "rt_render: KD mode needs rt_scene_set_kd (Trixel::create_kd) first");
    if (c->obj->ntri == 0) return fail(RT_ERR_STATE, "rt_render: empty scene");
    if (flags & ~(RT_FLAG_WRITE_HIT | RT_FLAG_COUNT | RT_FLAG_SHADOW | RT_FLAG_FRAME_OUT | RT_FLAG_WRITE_AOV))
        return fail(RT_ERR_INVALID, "rt_render: unknown flags 0x%x", flags);
    if (flags & RT_FLAG_SHADOW) {
        if (mode != RT_MODE_KD) return fail(RT_ERR_INVALID, "rt_render: RT_FLAG_SHADOW needs RT_MODE_KD");
        if (c->kernel_version != 3)
            return fail(RT_ERR_STATE, "rt_render: shadow rays run in the wave-cooperative kernel (3); kernel %d",
                        c->kernel_version);
    }
    const float* xf = xform ? xform : kIdentXf;
    const int32_t nr = tile ? tile->nranks : 1, rk = tile ? tile->rank : 0;
    float* aov = nullptr;
    int64_t aov_stride = 0;
    // rt_render_over reads the d it tests against: the camera's own planes
    // must hold a frame (a bound buffer is the caller's to fill)
    if (over_base && !c->aov_bound && !c->aov_filled)
        return fail(RT_ERR_STATE, "rt_render_over: the camera's own planes hold no frame (render with "
                                  "RT_FLAG_WRITE_AOV or rt_render_clear first)");
    if (flags & RT_FLAG_WRITE_AOV) {
        if ((rc = aov_target(c, nr, (flags & RT_FLAG_FRAME_OUT) != 0, &aov, &aov_stride))) return rc;
        // the planes ride on the write-hit instances: those need a hit target
        if (!hit) {
            if (!c->d_aov_hit && (rc = dev_alloc(&c->d_aov_hit, (size_t)c->w * c->h, "hipMalloc(aov hit)"))) return rc;
            hit = c->d_aov_hit;
        }
        flags |= RT_FLAG_WRITE_HIT;
    }
    auto& pc = c->pcache;
    TraceParams p;
    if (!(c->debug & 2) && pc.key.matches(c->geom_gen, xf, mode, nr) && pc.rank == rk) {
        p = pc.p;  // the same frame as the last one: its geometry stands
        p.argb = argb;
        p.hit = hit;
    } else {
        if ((rc = fill_params(c, xform, tile, argb, hit, mode, p, (hipStream_t)stream))) return rc;
        pc.key.set(c->geom_gen, xf, mode, nr);
        pc.key.valid = !(c->debug & 2);
        pc.rank = rk;
        pc.p = p;
    }
    p.frame_out = (flags & RT_FLAG_FRAME_OUT) ? 1 : 0;
    p.display = display;
    p.aov = aov;
    p.aov_stride = aov_stride;
    p.over = over_base ? 1 : 0;
    p.hit_base = over_base ? *over_base : 0;
    p.flat_key = nullptr;
    p.flat_chunks = 0;
    if (mode == RT_MODE_FLAT && c->flat_variant >= 10 && !(flags & RT_FLAG_COUNT)) {
        const int64_t npix = std::max<int64_t>((int64_t)c->w * c->h, rt_tile_packed_pixels(c->w, c->h, nr));
        if ((rc = flat_keys_for(c, (hipStream_t)stream, npix, &p.flat_key))) return rc;
        p.flat_chunks = c->flat_variant == 10 ? 8 : c->flat_variant == 11 ? 4 : c->flat_variant == 12 ? 16 : 32;
        const int64_t npair = (c->obj->ntri + 1) / 2;
        if (p.flat_chunks > npair) p.flat_chunks = (int32_t)npair;
    }
    if (mode == RT_MODE_KD && c->kernel_version == 3) {
        c->last_rays = p.rays;
        // bit 0: the nearest-hit walk's proof, bit 1: the shadow walk's (a
        // shadow render), bit 2: under an object transform
        c->last_fast = (p.fast ? 1 : 0) | ((p.fast_sh && (flags & RT_FLAG_SHADOW)) ? 2 : 0) |
                       ((p.fast && !p.plain_xf) ? 4 : 0);
        c->last_fine = (int64_t)p.tiles_x * p.block_rows;
    }
    int trial;
    p.any_order = any_order_for(c, flags, stream, trial) | ((c->debug & 16) ? 4 : 0);
    hipStream_t st = (hipStream_t)stream;
    // a trial frame is timed alone: with frames in flight on other lanes it
    // starts after theirs and their later frames start after it
    const bool solo = trial >= 0 && c->nactive > 1;
    for (int l = 0; solo && l < c->nactive; l++) {
        if (c->active[l] == st) continue;
        if ((rc = hip_check(hipEventRecord(c->lane_ev[l], c->active[l]), "trial join")) ||
            (rc = hip_check(hipStreamWaitEvent(st, c->lane_ev[l], 0), "trial join wait")))
            return rc;
    }
    if (trial >= 0 && (rc = hip_check(hipEventRecord(c->tune_ev[2 * trial], st), "order trial start"))) return rc;
    const bool order3 = p.cost != nullptr;
    // a multi-frame launch (KD kernel 3, fused far fill, no per-frame
    // outputs beyond the frame): one launch for pf->frames frames, no cost
    // sample inside it
    const bool persist = pf && pf->frames > 1 && mode == RT_MODE_KD && c->kernel_version == 3 && p.coarse_blocks == 0 &&
                         flags == 0 && !display;
    bool sampled = false;
    if ((rc = c->order.before_launch(p, st, persist, &sampled))) return rc;
    p.pf_frames = 0;
    if (persist) {
        p.pf_blocks = (int32_t)fine_grid_blocks(p);
        // the XCD-mapped orders (0, 4, 5): every frame's grid a multiple of
        // 8 blocks, so a frame's block b runs on XCD b % 8 (blocks are
        // dispatched to the 8 XCDs round robin); the padding blocks exit
        if (c->tile_order == 0 || c->tile_order == 4 || c->tile_order == 5) p.pf_blocks = (p.pf_blocks + 7) & ~7;
        // one dispatch holds at most 2^32 - 1 work-items (and 2^31 - 1
        // blocks): fewer frames per launch for large frames (a
        // 4K frame of 8-ray units is ~259k blocks of 256 threads)
        const int64_t threads = 64 * (int64_t)kd3_waves(p.rays);
        const int64_t max_blocks = std::min<int64_t>(0xFFFFFFFFll / threads, 0x7FFFFFFFll);
        p.pf_frames = (int32_t)std::max<int64_t>(1, std::min<int64_t>(pf->frames, max_blocks / std::max(1, p.pf_blocks)));
        p.pf_nbuf = pf->nbuf;
        p.pf_seq0 = pf->seq0 % pf->nbuf;
        for (int k = 0; k < RT_LOOP_MAX_BUF; k++) p.pf_argb[k] = k < pf->nbuf ? pf->argb[k] : nullptr;
        if (rendered) *rendered = p.pf_frames;
    }
    if ((rc = launch_split(c, p, mode, flags, stream))) return rc;
    if (trial >= 0) {
        if ((rc = hip_check(hipEventRecord(c->tune_ev[2 * trial + 1], st), "order trial stop"))) return rc;
        c->tune_pending = c->tune_next == kTuneTrials;
        for (int l = 0; solo && l < c->nactive; l++)
            if (c->active[l] != st &&
                (rc = hip_check(hipStreamWaitEvent(c->active[l], c->tune_ev[2 * trial + 1], 0), "trial fork wait")))
                return rc;
    }
    return c->order.after_launch(p, st, (c->debug & 8) ? c->side : nullptr, order3, sampled);
}

extern "C" int rt_render(rt_camera* c, const float* xform, uint32_t mode, uint32_t flags, const rt_tile* tile,
                         void* stream) {
    if (!c) return fail(RT_ERR_INVALID, "rt_render: null camera");
    if (tile && tile->nranks != 1)
        return fail(RT_ERR_INVALID, "rt_render: the camera's own buffer holds a full frame; use rt_render_into for tiles");
    return render_common(c, xform, mode, flags, tile, c->d_argb, c->d_hit, stream);
}

extern "C" int rt_render_display(rt_camera* c, const float* xform, uint32_t mode, uint32_t flags, const rt_tile* tile,
                                 uint32_t* d_clean, uint32_t* d_display, int64_t* d_hit, void* stream) {
    if (!d_clean || !d_display || d_clean == d_display)
        return fail(RT_ERR_INVALID, "rt_render_display: needs distinct clean and display buffers");
    return render_common(c, xform, mode, flags, tile, d_clean, d_hit, stream, d_display);
}

extern "C" int rt_render_into(rt_camera* c, const float* xform, uint32_t mode, uint32_t flags, const rt_tile* tile,
                              uint32_t* d_argb, int64_t* d_hit, void* stream) {
    return render_common(c, xform, mode, flags, tile, d_argb, d_hit, stream);
}

extern "C" int rt_render_over(rt_camera* c, const float* xform, uint32_t mode, uint32_t flags, const rt_tile* tile,
                              uint32_t* d_argb, int64_t* d_hit, int64_t hit_base, void* stream) {
    if (!c) return fail(RT_ERR_INVALID, "rt_render_over: null camera");
    if (flags & ~(RT_FLAG_WRITE_HIT | RT_FLAG_COUNT | RT_FLAG_SHADOW | RT_FLAG_FRAME_OUT | RT_FLAG_WRITE_AOV))
        return fail(RT_ERR_INVALID, "rt_render_over: unknown flags 0x%x", flags);
    if (hit_base < 0) return fail(RT_ERR_INVALID, "rt_render_over: hit_base %lld", (long long)hit_base);
    // no targets: the camera's own frame and hit buffers; a frame alone:
    // no hit index is kept (render_common's scratch takes the stores)
    if (!d_argb) {
        d_argb = c->d_argb;
        if (!d_hit) d_hit = c->d_hit;
    }
    // RT_FLAG_WRITE_AOV brings the write-hit instances (and that scratch) with it
    return render_common(c, xform, mode, (flags & ~RT_FLAG_WRITE_HIT) | RT_FLAG_WRITE_AOV, tile, d_argb, d_hit, stream,
                         nullptr, nullptr, nullptr, &hit_base);
}

extern "C" int rt_render_clear(rt_camera* c, uint32_t flags, const rt_tile* tile, uint32_t* d_argb, int64_t* d_hit,
                               void* stream) {
    if (!c) return fail(RT_ERR_INVALID, "rt_render_clear: null camera");
    if (flags & ~RT_FLAG_FRAME_OUT) return fail(RT_ERR_INVALID, "rt_render_clear: unknown flags 0x%x", flags);
    int rc = check_tile(tile);
    if (rc) return rc;
    if (!d_argb) {
        d_argb = c->d_argb;
        if (!d_hit) d_hit = c->d_hit;
    }
    DeviceGuard g(c->device);
    const int32_t nr = tile ? tile->nranks : 1, rk = tile ? tile->rank : 0;
    const bool frame_out = (flags & RT_FLAG_FRAME_OUT) != 0;
    float* aov = nullptr;
    int64_t stride = 0;
    if ((rc = aov_target(c, nr, frame_out, &aov, &stride))) return rc;  // marks the camera's own planes filled
    return launch_clear(c->w, c->h, nr, rk, frame_out, d_argb, d_hit, aov, stride, stream);
}

// The deferred shadow pass (k_shadow_kd3).  Its launch parameters are built
// here from the camera alone, beside the renders' machinery rather than
// through it: the pass has no fine region, cost order, held region or cached
// geometry, and must leave the camera's (fill_params' caches, TileOrder) as
// the renders left them.
extern "C" int rt_shadow_over(rt_camera* c, const float* xform, uint32_t flags, const rt_tile* tile, uint32_t* d_argb,
                              int64_t* d_hit, int64_t hit_base, int32_t skip_own, void* stream) {
    if (!c) return fail(RT_ERR_INVALID, "rt_shadow_over: null camera");
    if (flags & ~(RT_FLAG_COUNT | RT_FLAG_FRAME_OUT))
        return fail(RT_ERR_INVALID, "rt_shadow_over: flags 0x%x (RT_FLAG_COUNT and RT_FLAG_FRAME_OUT are accepted)", flags);
    if (hit_base < 0) return fail(RT_ERR_INVALID, "rt_shadow_over: hit_base %lld", (long long)hit_base);
    int rc = check_tile(tile);
    if (rc) return rc;
    if (d_argb && !d_hit) return fail(RT_ERR_INVALID, "rt_shadow_over: a frame without its hit buffer (the owner is needed)");
    if (!d_argb) {
        d_argb = c->d_argb;
        if (!d_hit) d_hit = c->d_hit;
    }
    if (c->kernel_version != 3)
        return fail(RT_ERR_INVALID, "rt_shadow_over: shadow rays run in the wave-cooperative kernel (3); kernel %d",
                    c->kernel_version);
    if (!c->obj) return fail(RT_ERR_STATE, "camera has no object (rt_camera_add_object)");
    if (!c->obj->d_nodes) return fail(RT_ERR_STATE, "rt_shadow_over: needs rt_scene_set_kd (Trixel::create_kd) first");
    if (c->obj->ntri == 0) return fail(RT_ERR_STATE, "rt_shadow_over: empty scene");
    const int32_t nr = tile ? tile->nranks : 1, rk = tile ? tile->rank : 0;
    const bool frame_out = (flags & RT_FLAG_FRAME_OUT) != 0;
    // plane 0 is read, never written: the bound planes (the caller's to fill,
    // and to size) or the camera's own once something filled them
    float* aov = c->aov_bound;
    int64_t stride = c->aov_bound_stride;
    if (aov) {
        const int64_t need = nr > 1 && !frame_out ? rt_tile_packed_pixels(c->w, c->h, nr) : (int64_t)c->w * c->h;
        if (stride < need)
            return fail(RT_ERR_INVALID, "rt_shadow_over: plane stride %lld is below the %lld pixels this pass reads",
                        (long long)stride, (long long)need);
    } else {
        if (!c->d_aov || !c->aov_filled)
            return fail(RT_ERR_STATE, "rt_shadow_over: the camera's own planes hold no frame (render with "
                                      "RT_FLAG_WRITE_AOV or rt_render_clear first)");
        aov = c->d_aov;
        stride = rt_tile_packed_pixels(c->w, c->h, 1);
    }
    DeviceGuard g(c->device);
    if ((rc = prepare_camera_object(c))) return rc;
    const rt_scene* s = c->obj;
    TraceParams p{};
    p.inode = c->d_inode;
    p.trec = c->d_trec;
    p.split_planes = (c->cam_flags & kCamSplitFields) ? c->d_split : nullptr;
    p.leaf_off = c->leaf_off;
    p.rec_bytes = c->leaf_off ? (uint32_t)(c->leaf_off + 64 * (uint64_t)s->ntri) : 0u;
    p.shade = s->d_shade;
    p.argb = d_argb;
    p.hit = d_hit;
    p.counters = c->d_counters;
    p.err = c->d_err;
    for (int k = 0; k < 3; k++) {
        p.n_mod[k] = c->basis.n_mod[k];
        p.u_mod[k] = c->basis.u_mod[k];
        p.v_mod[k] = c->basis.v_mod[k];
    }
    memcpy(p.xf, xform ? xform : kIdentXf, sizeof p.xf);
    p.w = c->w;
    p.h = c->h;
    p.nranks = nr;
    p.rank = rk;
    p.frame_out = frame_out ? 1 : 0;
    // every tile of the rank's bands: 8 x 8 pixels, four 16-pixel units
    p.rays = 16;
    p.tile_w = 8;
    p.tile_h = kd3_waves(16) * 2;
    const int32_t nbands = (c->h + kTileH - 1) / kTileH;
    p.tiles_x = (c->w + p.tile_w - 1) / p.tile_w;
    p.block_rows = ((nbands + nr - 1) / nr) * (kTileH / p.tile_h);
    // natural order unless the camera asks for XCD-contiguous runs (RT_OPT_TILE_ORDER 0):
    // the grid is the whole frame and the work sits where the hits are, so a
    // contiguous run per XCD leaves most XCDs idle (knot 1080p: 325 against 132 us)
    p.tile_order = c->tile_order == 0 ? 0 : 1;
    camera_relative_box(s->root, c->pos, p.root_box);
    p.root_ref = s->root_ref;
    p.ntri = s->ntri;
    p.max_depth = kMaxDepth;
    p.tree_height = s->height;
    p.two_depth = -1;
    p.tiny_s1 = (c->cam_flags & kCamTinyS1) ? 1 : 0;
    p.plain_xf = 0;
    p.fast = p.fast_sh = 0;  // the double forms (k_shadow_kd3's comment)
    p.debug = c->debug;
    p.pool_cap = c->pool_cap;
    p.items = c->items;
    // a fixed push order as given; timed (-1): the order in use, no timing frames here
    p.any_order = (c->shadow_order >= 0 ? c->shadow_order : c->any_best) | ((c->debug & 16) ? 4 : 0);
    p.aov = aov;
    p.aov_stride = stride;
    p.hit_base = hit_base;
    p.shadow_skip_own = skip_own ? 1 : 0;
    return launch_shadow_over(p, (flags & RT_FLAG_COUNT) != 0, stream);
}

// The light list (rt_light_over, rt_shade_lights).  Not stream-ordered: the
// device copy is rewritten after the device has drained, so no pass in flight
// reads a half-written list.
extern "C" int rt_camera_set_lights(rt_camera* c, const float* lights4, int32_t n) {
    if (!c) return fail(RT_ERR_INVALID, "rt_camera_set_lights: null camera");
    if (!lights4 || n < 1 || n > RT_LIGHTS_MAX)
        return fail(RT_ERR_INVALID, "rt_camera_set_lights: %d lights (1..%d)", n, RT_LIGHTS_MAX);
    for (int k = 0; k < 4 * n; k++)
        if (!std::isfinite(lights4[k]))
            return fail(RT_ERR_INVALID, "rt_camera_set_lights: light %d has a non-finite component", k / 4);
    DeviceGuard g(c->device);
    float next[4 * RT_LIGHTS_MAX] = {};
    memcpy(next, lights4, sizeof(float) * 4 * (size_t)n);
    int rc;
    if ((rc = hip_check(hipDeviceSynchronize(), "rt_camera_set_lights: synchronize")) ||
        (rc = hip_check(hipMemcpy(c->d_lights, next, sizeof next, hipMemcpyHostToDevice), "H2D lights")))
        return rc;
    memcpy(c->lights, next, sizeof next);
    c->nlights = n;
    return RT_OK;
}

extern "C" int rt_camera_get_lights(rt_camera* c, float* lights4, int32_t* n) {
    if (!c) return fail(RT_ERR_INVALID, "rt_camera_get_lights: null camera");
    if (lights4) memcpy(lights4, c->lights, sizeof(float) * 4 * (size_t)c->nlights);
    if (n) *n = c->nlights;
    return RT_OK;
}

// What rt_light_over and rt_shade_lights share with rt_shadow_over: the
// targets' defaults, the plane target's checks, and the launch parameters of
// a pass over every tile of the rank's frame (the camera's caches stay as the
// renders left them).  tile_h: rows of a block's tile.
static int light_pass_params(rt_camera* c, const char* who, const float* xform, const rt_tile* tile, bool frame_out,
                             uint32_t*& d_argb, int64_t*& d_hit, int32_t tile_h, TraceParams& p) {
    int rc = check_tile(tile);
    if (rc) return rc;
    if (d_argb && !d_hit) return fail(RT_ERR_INVALID, "%s: a frame without its hit buffer (the owner is needed)", who);
    if (!d_argb) {
        d_argb = c->d_argb;
        if (!d_hit) d_hit = c->d_hit;
    }
    const int32_t nr = tile ? tile->nranks : 1, rk = tile ? tile->rank : 0;
    // the planes are read, never written: the bound ones (the caller's to
    // fill, and to size) or the camera's own once something filled them
    float* aov = c->aov_bound;
    int64_t stride = c->aov_bound_stride;
    if (aov) {
        const int64_t need = nr > 1 && !frame_out ? rt_tile_packed_pixels(c->w, c->h, nr) : (int64_t)c->w * c->h;
        if (stride < need)
            return fail(RT_ERR_INVALID, "%s: plane stride %lld is below the %lld pixels this pass reads", who,
                        (long long)stride, (long long)need);
    } else {
        if (!c->d_aov || !c->aov_filled)
            return fail(RT_ERR_STATE, "%s: the camera's own planes hold no frame (render with RT_FLAG_WRITE_AOV or "
                                      "rt_render_clear first)", who);
        aov = c->d_aov;
        stride = rt_tile_packed_pixels(c->w, c->h, 1);
    }
    p.argb = d_argb;
    p.hit = d_hit;
    p.counters = c->d_counters;
    p.err = c->d_err;
    for (int k = 0; k < 3; k++) {
        p.n_mod[k] = c->basis.n_mod[k];
        p.u_mod[k] = c->basis.u_mod[k];
        p.v_mod[k] = c->basis.v_mod[k];
    }
    memcpy(p.xf, xform ? xform : kIdentXf, sizeof p.xf);
    p.w = c->w;
    p.h = c->h;
    p.nranks = nr;
    p.rank = rk;
    p.frame_out = frame_out ? 1 : 0;
    p.tile_w = 8;
    p.tile_h = tile_h;
    const int32_t nbands = (c->h + kTileH - 1) / kTileH;
    p.tiles_x = (c->w + p.tile_w - 1) / p.tile_w;
    p.block_rows = ((nbands + nr - 1) / nr) * (kTileH / p.tile_h);
    p.tile_order = c->tile_order == 0 ? 0 : 1;  // as rt_shadow_over
    p.two_depth = -1;
    p.debug = c->debug;
    p.aov = aov;
    p.aov_stride = stride;
    p.lights = c->d_lights;
    p.nlights = c->nlights;
    return RT_OK;
}

// The visibility pass of the light list (k_light_kd3): rt_shadow_over's
// launch with the camera's lights, every hit pixel tested.
extern "C" int rt_light_over(rt_camera* c, const float* xform, uint32_t flags, const rt_tile* tile, uint32_t* d_argb,
                             int64_t* d_hit, int64_t hit_base, void* stream) {
    if (!c) return fail(RT_ERR_INVALID, "rt_light_over: null camera");
    if (flags & ~(RT_FLAG_COUNT | RT_FLAG_FRAME_OUT))
        return fail(RT_ERR_INVALID, "rt_light_over: flags 0x%x (RT_FLAG_COUNT and RT_FLAG_FRAME_OUT are accepted)", flags);
    if (hit_base < 0) return fail(RT_ERR_INVALID, "rt_light_over: hit_base %lld", (long long)hit_base);
    int rc = check_tile(tile);
    if (rc) return rc;
    if (d_argb && !d_hit) return fail(RT_ERR_INVALID, "rt_light_over: a frame without its hit buffer (the owner is needed)");
    if (c->kernel_version != 3)
        return fail(RT_ERR_INVALID, "rt_light_over: shadow rays run in the wave-cooperative kernel (3); kernel %d",
                    c->kernel_version);
    if (!c->obj) return fail(RT_ERR_STATE, "camera has no object (rt_camera_add_object)");
    if (!c->obj->d_nodes) return fail(RT_ERR_STATE, "rt_light_over: needs rt_scene_set_kd (Trixel::create_kd) first");
    if (c->obj->ntri == 0) return fail(RT_ERR_STATE, "rt_light_over: empty scene");
    TraceParams p{};
    if ((rc = light_pass_params(c, "rt_light_over", xform, tile, (flags & RT_FLAG_FRAME_OUT) != 0, d_argb, d_hit,
                                kd3_waves(16) * 2, p)))
        return rc;
    DeviceGuard g(c->device);
    if ((rc = prepare_camera_object(c))) return rc;
    const rt_scene* s = c->obj;
    p.inode = c->d_inode;
    p.trec = c->d_trec;
    p.split_planes = (c->cam_flags & kCamSplitFields) ? c->d_split : nullptr;
    p.leaf_off = c->leaf_off;
    p.rec_bytes = c->leaf_off ? (uint32_t)(c->leaf_off + 64 * (uint64_t)s->ntri) : 0u;
    p.shade = s->d_shade;
    p.rays = 16;  // four 16-pixel units per 8 x 8 tile
    camera_relative_box(s->root, c->pos, p.root_box);
    p.root_ref = s->root_ref;
    p.ntri = s->ntri;
    p.max_depth = kMaxDepth;
    p.tree_height = s->height;
    p.tiny_s1 = (c->cam_flags & kCamTinyS1) ? 1 : 0;
    p.plain_xf = 0;
    p.fast = p.fast_sh = 0;  // the double forms (k_light_kd3's comment)
    p.pool_cap = c->pool_cap;
    p.items = c->items;
    // a fixed push order as given; timed (-1): the order in use, no timing frames here
    p.any_order = (c->shadow_order >= 0 ? c->shadow_order : c->any_best) | ((c->debug & 16) ? 4 : 0);
    p.hit_base = hit_base;
    return launch_light_over(p, (flags & RT_FLAG_COUNT) != 0, stream);
}

// The shading pass of the light list (k_shade_lights): no tree, no object.
extern "C" int rt_shade_lights(rt_camera* c, uint32_t flags, const rt_tile* tile, uint32_t* d_argb, int64_t* d_hit,
                               void* stream) {
    if (!c) return fail(RT_ERR_INVALID, "rt_shade_lights: null camera");
    if (flags & ~RT_FLAG_FRAME_OUT)
        return fail(RT_ERR_INVALID, "rt_shade_lights: flags 0x%x (RT_FLAG_FRAME_OUT is accepted)", flags);
    TraceParams p{};
    int rc = light_pass_params(c, "rt_shade_lights", nullptr, tile, (flags & RT_FLAG_FRAME_OUT) != 0, d_argb, d_hit,
                               kTileH, p);
    if (rc) return rc;
    DeviceGuard g(c->device);
    p.rays = 8 * kTileH;  // one pixel per lane: an 8 x 8 tile per wave
    return launch_shade_lights(p, stream);
}

extern "C" int rt_camera_targets(rt_camera* c, uint32_t** d_argb, int64_t** d_hit, float** d_aov, int64_t* plane_stride) {
    if (!c) return fail(RT_ERR_INVALID, "rt_camera_targets: null camera");
    const int64_t stride = rt_tile_packed_pixels(c->w, c->h, 1);
    if (d_aov && !c->d_aov) {
        DeviceGuard g(c->device);
        int rc = dev_alloc(&c->d_aov, (size_t)(RT_AOV_PLANES * stride), "hipMalloc(aov)");
        if (rc) return rc;
    }
    if (d_argb) *d_argb = c->d_argb;
    if (d_hit) *d_hit = c->d_hit;
    if (d_aov) *d_aov = c->d_aov;
    if (plane_stride) *plane_stride = stride;
    return RT_OK;
}

extern "C" int64_t rt_tile_packed_pixels(int32_t w, int32_t h, int32_t nranks) {
    if (w <= 0 || h <= 0 || nranks < 1) return -1;
    const int64_t nbands = (h + kTileH - 1) / kTileH;
    const int64_t slots = (nbands + nranks - 1) / nranks;
    return slots * kTileH * (int64_t)w;
}

extern "C" int rt_unpack_bands(int device, int32_t w, int32_t h, int32_t nranks, const uint32_t* d_gathered,
                               uint32_t* d_frame, void* stream) {
    if (!d_gathered || !d_frame || w <= 0 || h <= 0 || nranks < 1) return fail(RT_ERR_INVALID, "rt_unpack_bands: bad argument");
    DeviceGuard g(device);
    return launch_unpack(w, h, nranks, d_gathered, d_frame, stream);
}

extern "C" int rt_frame_rect(rt_camera* c, const float* xform, uint32_t mode, int32_t nranks, int32_t rect[4]) {
    if (!c || !rect || nranks < 1) return fail(RT_ERR_INVALID, "rt_frame_rect: bad argument");
    if (mode != RT_MODE_KD && mode != RT_MODE_FLAT) return fail(RT_ERR_INVALID, "rt_frame_rect: mode %u", mode);
    DeviceGuard g(c->device);
    int rc;
    if ((rc = prepare_camera_object(c))) return rc;
    const float* xf = xform ? xform : kIdentXf;
    auto& rcx = c->rcache;
    if (rcx.key.matches(c->geom_gen, xf, mode, nranks)) {
        memcpy(rect, rcx.rect, sizeof rcx.rect);
        return RT_OK;
    }
    frame_rect_geom(camera_geom(c), c->obj->d_nodes != nullptr, xform, mode, nranks, rect);
    rcx.key.set(c->geom_gen, xf, mode, nranks);
    memcpy(rcx.rect, rect, sizeof rcx.rect);
    return RT_OK;
}

extern "C" int rt_camera_frame_geometry(rt_camera* c, rt_frame_geometry* out) {
    if (!c || !out) return fail(RT_ERR_INVALID, "rt_camera_frame_geometry: bad argument");
    DeviceGuard g(c->device);
    int rc;
    if ((rc = prepare_camera_object(c))) return rc;
    // the host rectangle (rt_frame_rect_host) assumes a KD tree, as the
    // device rectangle does only when the scene has one
    if (!c->obj->d_nodes) return fail(RT_ERR_STATE, "rt_camera_frame_geometry: the scene has no KD tree");
    const FrameGeom f = camera_geom(c);
    out->w = f.w;
    out->h = f.h;
    for (int k = 0; k < 3; k++) {
        out->n_mod[k] = f.n_mod[k];
        out->u_mod[k] = f.u_mod[k];
        out->v_mod[k] = f.v_mod[k];
    }
    memcpy(out->root_box, f.root_box, sizeof out->root_box);
    out->root_is_leaf = f.root_leaf ? 1 : 0;
    out->kernel = f.kernel;
    out->rays = f.rays;
    out->coarse = f.coarse;
    out->debug = f.debug;
    return RT_OK;
}

extern "C" int rt_frame_rect_host(const rt_frame_geometry* in, const float* xform, uint32_t mode, int32_t nranks,
                                  int32_t rect[4]) {
    if (!in || !rect || nranks < 1 || in->w <= 0 || in->h <= 0) return fail(RT_ERR_INVALID, "rt_frame_rect_host: bad argument");
    if (mode != RT_MODE_KD && mode != RT_MODE_FLAT) return fail(RT_ERR_INVALID, "rt_frame_rect_host: mode %u", mode);
    if (in->kernel < 1 || in->kernel > 3 || (in->rays != 0 && in->rays != 8 && in->rays != 16 && in->rays != 32 &&
                                              in->rays != 64) || in->coarse < 0 || in->coarse > 32)
        return fail(RT_ERR_INVALID, "rt_frame_rect_host: bad kernel options");
    std::vector<std::pair<int32_t, int32_t>> tiny;
    frame_rect_geom(host_geom(*in, tiny), true, xform, mode, nranks, rect);
    return RT_OK;
}

static int check_rect(int32_t w, int32_t h, int32_t nranks, const int32_t rect[4], const char* what) {
    const int32_t nbands = (h + kTileH - 1) / kTileH;
    if (w <= 0 || h <= 0 || nranks < 1 || !rect || rect[0] < 0 || rect[1] > w || rect[0] > rect[1] || rect[2] < 0 ||
        rect[3] > nbands || rect[2] > rect[3])
        return fail(RT_ERR_INVALID, "%s: bad frame geometry or rectangle", what);
    return RT_OK;
}

extern "C" int64_t rt_rect_pixels(int32_t w, int32_t h, int32_t nranks, int32_t rank, const int32_t rect[4]) {
    if (check_rect(w, h, nranks, rect, "rt_rect_pixels") || rank < 0 || rank >= nranks) return -1;
    int32_t s0, s1;
    rect_slots(rect[2], rect[3], nranks, rank, s0, s1);
    return (int64_t)(s1 - s0) * kTileH * (rect[1] - rect[0]);
}

extern "C" int rt_pack_rect(int device, int32_t w, int32_t h, int32_t nranks, int32_t rank, const int32_t rect[4],
                            const uint32_t* d_local, uint32_t* d_out, void* stream) {
    int rc;
    if ((rc = check_rect(w, h, nranks, rect, "rt_pack_rect"))) return rc;
    if (rank < 0 || rank >= nranks || !d_local || !d_out) return fail(RT_ERR_INVALID, "rt_pack_rect: bad argument");
    DeviceGuard g(device);
    return launch_pack_rect(w, h, nranks, rank, rect, d_local, d_out, stream);
}

// Host-memory forms of the rectangle gather's pack and assembly (the same
// index maps as k_pack_rect / k_unpack_rect), for a gather over host buffers
// (distributed.HostRectGather: the protocol over gloo, tests on CPU).
extern "C" int rt_pack_rect_host(int32_t w, int32_t h, int32_t nranks, int32_t rank, const int32_t rect[4],
                                 const uint32_t* local, uint32_t* out) {
    int rc;
    if ((rc = check_rect(w, h, nranks, rect, "rt_pack_rect_host"))) return rc;
    if (rank < 0 || rank >= nranks || !local || !out) return fail(RT_ERR_INVALID, "rt_pack_rect_host: bad argument");
    int32_t s0, s1;
    rect_slots(rect[2], rect[3], nranks, rank, s0, s1);
    const int32_t cw = rect[1] - rect[0];
    for (int32_t row = 0; row < (s1 - s0) * kTileH; row++) {
        const int32_t s = s0 + row / kTileH, r = row % kTileH;
        memcpy(out + (int64_t)row * cw, local + ((int64_t)s * kTileH + r) * w + rect[0], sizeof(uint32_t) * (size_t)cw);
    }
    return RT_OK;
}

extern "C" int rt_unpack_rect_host(int32_t w, int32_t h, int32_t nranks, const int32_t rect[4], const uint32_t* local0,
                                   const uint32_t* peers, uint32_t* frame) {
    int rc;
    if ((rc = check_rect(w, h, nranks, rect, "rt_unpack_rect_host"))) return rc;
    if (!local0 || !frame || (nranks > 1 && !peers)) return fail(RT_ERR_INVALID, "rt_unpack_rect_host: bad argument");
    const int32_t x0 = rect[0], x1 = rect[1], b0 = rect[2], b1 = rect[3], cw = x1 - x0;
    std::vector<int64_t> off((size_t)nranks + 1, 0);  // each peer's part, back to back
    for (int32_t q = 1; q < nranks; q++) {
        int32_t s0, s1;
        rect_slots(b0, b1, nranks, q, s0, s1);
        off[(size_t)q + 1] = off[(size_t)q] + (int64_t)(s1 - s0) * kTileH * cw;
    }
    for (int32_t y = 0; y < h; y++) {
        const int32_t band = y / kTileH, r = y - band * kTileH;
        const int32_t rank = band % nranks, slot = band / nranks;
        uint32_t* dst = frame + (int64_t)y * w;
        for (int32_t x = 0; x < w; x++) dst[x] = 0x00F08200u;  // the background, TD/Camera.cpp:72
        if (band < b0 || band >= b1 || cw <= 0) continue;
        const uint32_t* src;
        if (rank == 0) {
            src = local0 + ((int64_t)slot * kTileH + r) * w + x0;
        } else {
            int32_t s0, s1;
            rect_slots(b0, b1, nranks, rank, s0, s1);
            src = peers + off[(size_t)rank] + ((int64_t)(slot - s0) * kTileH + r) * cw;
        }
        memcpy(dst + x0, src, sizeof(uint32_t) * (size_t)cw);
    }
    return RT_OK;
}

extern "C" int rt_unpack_rect(int device, int32_t w, int32_t h, int32_t nranks, const int32_t rect[4],
                              const uint32_t* d_local0, const uint32_t* d_peers, uint32_t* d_frame, void* stream) {
    int rc;
    if ((rc = check_rect(w, h, nranks, rect, "rt_unpack_rect"))) return rc;
    if (!d_local0 || !d_frame || (nranks > 1 && !d_peers)) return fail(RT_ERR_INVALID, "rt_unpack_rect: bad argument");
    DeviceGuard g(device);
    // d_local0 == d_frame: rank 0's bands were rendered into the frame (RT_FLAG_FRAME_OUT)
    return launch_unpack_rect(w, h, nranks, rect, d_local0 == d_frame ? nullptr : d_local0, d_peers, d_frame, stream);
}

extern "C" int rt_read_frame(rt_camera* c, uint32_t* argb, int64_t* hit) {
    if (!c || !argb) return fail(RT_ERR_INVALID, "rt_read_frame: null argument");
    DeviceGuard g(c->device);
    int rc;
    if ((rc = hip_check(hipDeviceSynchronize(), "rt_read_frame sync"))) return rc;
    int32_t err = 0;
    if ((rc = hip_check(hipMemcpy(&err, c->d_err, sizeof err, hipMemcpyDeviceToHost), "D2H err"))) return rc;
    const size_t npix = (size_t)c->w * c->h;
    if ((rc = hip_check(hipMemcpy(argb, c->d_argb, npix * sizeof(uint32_t), hipMemcpyDeviceToHost), "D2H argb")))
        return rc;
    if (hit && (rc = hip_check(hipMemcpy(hit, c->d_hit, npix * sizeof(int64_t), hipMemcpyDeviceToHost), "D2H hit")))
        return rc;
    if (err) return device_error(err);
    return RT_OK;
}

extern "C" int rt_camera_set_aov(rt_camera* c, float* d_aov, int64_t plane_stride) {
    if (!c) return fail(RT_ERR_INVALID, "rt_camera_set_aov: null camera");
    if (d_aov && plane_stride <= 0) return fail(RT_ERR_INVALID, "rt_camera_set_aov: plane stride %lld", (long long)plane_stride);
    c->aov_bound = d_aov;
    c->aov_bound_stride = d_aov ? plane_stride : 0;
    return RT_OK;
}

extern "C" int rt_read_aov(rt_camera* c, float* aov) {
    if (!c || !aov) return fail(RT_ERR_INVALID, "rt_read_aov: null argument");
    if (!c->aov_filled)
        return fail(RT_ERR_STATE, "rt_read_aov: no RT_FLAG_WRITE_AOV render has filled the camera's own planes");
    DeviceGuard g(c->device);
    int rc;
    if ((rc = hip_check(hipDeviceSynchronize(), "rt_read_aov sync"))) return rc;
    // the planes of w*h floats out of the buffer's wider stride
    const size_t row = (size_t)c->w * c->h * sizeof(float);
    const size_t pitch = (size_t)rt_tile_packed_pixels(c->w, c->h, 1) * sizeof(float);
    return hip_check(hipMemcpy2D(aov, row, c->d_aov, pitch, row, RT_AOV_PLANES, hipMemcpyDeviceToHost), "D2H aov");
}

extern "C" int rt_pinned_alloc(size_t bytes, void** out) {
    if (!out) return fail(RT_ERR_INVALID, "rt_pinned_alloc: null out");
    *out = nullptr;
    return hip_check(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault), "hipHostMalloc");
}

extern "C" void rt_pinned_free(void* p) {
    if (p) (void)hipHostFree(p);
}

extern "C" int rt_frame_copy_async(int device, const uint32_t* d_argb, uint32_t* h_argb, int64_t npix, void* stream) {
    if (!d_argb || !h_argb || npix < 0) return fail(RT_ERR_INVALID, "rt_frame_copy_async: bad argument");
    if (npix == 0) return RT_OK;
    DeviceGuard g(device);
    return hip_check(hipMemcpyAsync(h_argb, d_argb, sizeof(uint32_t) * (size_t)npix, hipMemcpyDeviceToHost,
                                    (hipStream_t)stream), "D2H frame");
}

extern "C" int rt_camera_counters(rt_camera* c, uint64_t out[5], int reset) {
    if (!c || !out) return fail(RT_ERR_INVALID, "rt_camera_counters: null argument");
    DeviceGuard g(c->device);
    int rc;
    if ((rc = hip_check(hipDeviceSynchronize(), "counters sync"))) return rc;
    unsigned long long tmp[5];
    if ((rc = hip_check(hipMemcpy(tmp, c->d_counters, sizeof tmp, hipMemcpyDeviceToHost), "D2H counters"))) return rc;
    for (int k = 0; k < 5; k++) out[k] = tmp[k];
    if (reset && (rc = hip_check(hipMemset(c->d_counters, 0, sizeof tmp), "reset counters"))) return rc;
    int32_t err = 0;
    if ((rc = hip_check(hipMemcpy(&err, c->d_err, sizeof err, hipMemcpyDeviceToHost), "D2H err"))) return rc;
    if (err) return device_error(err);
    return RT_OK;
}

extern "C" int rt_camera_error(rt_camera* c, int32_t* err, int reset) {
    if (!c || !err) return fail(RT_ERR_INVALID, "rt_camera_error: null argument");
    DeviceGuard g(c->device);
    int rc;
    if ((rc = hip_check(hipDeviceSynchronize(), "rt_camera_error sync"))) return rc;
    if ((rc = hip_check(hipMemcpy(err, c->d_err, sizeof *err, hipMemcpyDeviceToHost), "D2H err"))) return rc;
    if (reset && (rc = hip_check(hipMemset(c->d_err, 0, sizeof(int32_t)), "reset err"))) return rc;
    return RT_OK;
}

extern "C" int rt_camera_info(const rt_camera* c, int32_t* w, int32_t* h, int32_t* max_depth) {
    if (!c) return fail(RT_ERR_INVALID, "rt_camera_info: null camera");
    if (w) *w = c->w;
    if (h) *h = c->h;
    if (max_depth) *max_depth = c->obj ? c->obj->height : 0;
    return RT_OK;
}

extern "C" void rt_scene_destroy(rt_scene* s) {
    if (!s) return;
    DeviceGuard g(s->device);
    dev_free(s->d_tri_world);
    dev_free(s->d_shade);
    dev_free(s->d_nodes);
    dev_free(s->d_interior_ids);
    dev_free(s->d_node_ref);
    delete s;
}

extern "C" void rt_camera_destroy(rt_camera* c) {
    if (!c) return;
    DeviceGuard g(c->device);
    dev_free(c->d_argb);
    dev_free(c->d_hit);
    dev_free(c->d_aov);
    dev_free(c->d_aov_hit);
    dev_free(c->d_counters);
    dev_free(c->d_err);
    dev_free(c->d_lights);
    dev_free(c->d_cam_flags);
    dev_free(c->d_split);
    dev_free(c->d_rec);
    dev_free(c->d_tpair);
    dev_free(c->d_dbg);
    for (auto& k : c->flat_keys) dev_free(k.d);
    for (hipEvent_t e : c->tune_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->join_ev) (void)hipEventDestroy(c->join_ev);
    for (hipEvent_t e : c->loop_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->side) (void)hipStreamDestroy(c->side);
    for (int k = 0; k <= RT_LOOP_MAX_LANES; k++) {
        if (c->lanes[k]) (void)hipStreamDestroy(c->lanes[k]);
        if (c->lane_ev[k]) (void)hipEventDestroy(c->lane_ev[k]);
    }
    delete c;  // (its TileOrder frees its own, under the guard)
}

extern "C" int rt_camera_set_option(rt_camera* c, int32_t key, int32_t value) {
    if (!c) return fail(RT_ERR_INVALID, "rt_camera_set_option: null camera");
    c->geom_gen++;  // cached launch geometry is stale
    switch (key) {
    case kOptKernel:
        // kernel 1 (round 1's per-lane DFS over own-box records, 1.8 ms per
        // 1080p frame) is gone; 2 is the reference-order per-lane DFS
        if (value < 2 || value > 3) return fail(RT_ERR_INVALID, "kernel version %d (2, 3)", value);
        c->kernel_version = value;
        return RT_OK;
    case kOptRays:
        // (64 rays per wave measured slower everywhere, r04u-w, and is gone)
        if (value != 0 && value != 8 && value != 16 && value != 32)
            return fail(RT_ERR_INVALID, "rays per wave %d (0 auto, 8, 16, 32)", value);
        c->rays = value;
        return RT_OK;
    case kOptItems:
        if (value != 1 && value != 2 && !(value >= 65 && value <= 128))
            return fail(RT_ERR_INVALID, "items per lane %d (1, 2, or 65..128: two when the pool holds that many)", value);
        c->items = value;
        return RT_OK;
    case kOptCoarse:
        if (value < 0 || value > 32) return fail(RT_ERR_INVALID, "coarse groups per wave %d (0..32)", value);
        c->coarse = value;
        return RT_OK;
    case kOptPoolCap:
        // the 64 root items plus a DFS run of height <= 24 must fit
        if (value < 64 + kMaxDepth + 1 || value > kPoolCapMax)
            return fail(RT_ERR_INVALID, "pool cap %d (%d..%d)", value, 64 + kMaxDepth + 1, kPoolCapMax);
        c->pool_cap = value;
        return RT_OK;
    case kOptDebug:
        // the record-load statistics accumulate until the option is set again:
        // they share d_dbg with the per-wave stamps (bit 2), whose records an
        // earlier render may have left there, and start from zero here (a buffer
        // of fewer than 32 words is replaced, zeroed, by the next render)
        if ((value & 16384) && c->d_dbg && c->dbg_cap >= 32) {
            DeviceGuard g(c->device);
            int rc;
            if ((rc = hip_check(hipDeviceSynchronize(), "debug option sync")) ||
                (rc = hip_check(hipMemset(c->d_dbg, 0, sizeof(uint64_t) * 32), "memset vstat")))
                return rc;
        }
        c->debug = value;
        return RT_OK;
    case kOptShadowOrder:
        if (value < -1 || value > 3) return fail(RT_ERR_INVALID, "shadow push order %d (-1 timed, 0..3)", value);
        c->shadow_order = value;
        c->tune_next = 0;
        c->tune_frames = 0;
        c->tune_pending = false;
        return RT_OK;
    case kOptFlat:
        // forms 0-8, 10, 11, 13 of rounds 1-2 measured slower and are gone
        if (value != 9 && value != 12) return fail(RT_ERR_INVALID, "flat kernel form %d (9 or 12)", value);
        c->flat_variant = value;
        return RT_OK;
    case kOptTileOrder:
        if (value < 0 || value > 5) return fail(RT_ERR_INVALID, "tile order %d (0..5)", value);
        c->tile_order = value;
        return RT_OK;
    case 10:
    case 11:
        return fail(RT_ERR_INVALID, "rt_camera_set_option: key %d is retired (ABI 2)", key);
    default:
        return fail(RT_ERR_INVALID, "rt_camera_set_option: unknown key %d", key);
    }
}

extern "C" int rt_camera_get_option(const rt_camera* c, int32_t key, int32_t* value) {
    if (!c || !value) return fail(RT_ERR_INVALID, "rt_camera_get_option: null argument");
    switch (key) {
    case kOptKernel: *value = c->kernel_version; return RT_OK;
    case kOptTileOrder: *value = c->tile_order; return RT_OK;
    case kOptRays: *value = c->rays; return RT_OK;
    case kOptItems: *value = c->items; return RT_OK;
    case kOptCoarse: *value = c->coarse; return RT_OK;
    case kOptFlat: *value = c->flat_variant; return RT_OK;
    case kOptRaysUsed: *value = c->last_rays; return RT_OK;
    case kOptDebug: *value = c->debug; return RT_OK;
    case kOptSplitUsed: *value = c->order.split(); return RT_OK;
    case kOptFastUsed: *value = c->last_fast; return RT_OK;
    case kOptOrderRestores: *value = (int32_t)std::min<uint64_t>(c->order.restores(), INT32_MAX); return RT_OK;
    case kOptFineTiles: *value = (int32_t)std::min<int64_t>(c->last_fine, INT32_MAX); return RT_OK;
    case kOptShadowOrder: *value = c->shadow_order >= 0 ? c->shadow_order : c->any_best; return RT_OK;
    case 10:
    case 11: return fail(RT_ERR_INVALID, "rt_camera_get_option: key %d is retired (ABI 2)", key);
    default: return fail(RT_ERR_INVALID, "rt_camera_get_option: unknown key %d", key);
    }
}

namespace rt {
void camera_relative_box(const rt_kd_node& nd, const float pos[3], float b[6]) {
    // init_cam_voxel_mem_cuda, TD/Camera.cu:142-147 (obj_center = 0); the
    // same IEEE operations as the device-side rel_box
    const float oc = 0.0f;
    b[0] = nd.x0 - pos[0] + oc; b[1] = nd.x1 - pos[0] + oc;
    b[2] = nd.y0 - pos[1] + oc; b[3] = nd.y1 - pos[1] + oc;
    b[4] = nd.z0 - pos[2] + oc; b[5] = nd.z1 - pos[2] + oc;
}
}  // namespace rt

extern "C" int64_t rt_camera_debug_read(rt_camera* c, uint64_t* out, int64_t n) {
    if (!c || !out || !c->d_dbg) return fail(RT_ERR_STATE, "rt_camera_debug_read: no diagnostic buffer");
    DeviceGuard g(c->device);
    const int64_t m = std::min(n, c->dbg_cap);
    if (hip_check(hipDeviceSynchronize(), "debug sync") ||
        hip_check(hipMemcpy(out, c->d_dbg, sizeof(uint64_t) * (size_t)m, hipMemcpyDeviceToHost), "D2H dbg"))
        return RT_ERR_HIP;
    return m;
}

// The frame loop in native code (bench.py, a headless viewer): per frame one
// render into buffer set k = seq % nbuf and, with a communicator, its gather
// on the comm stream while the next frame renders; a buffer set is reused
// only after its gather has read it (events).  The host work per frame is the
// cached launch (render_common) plus, with comm, the cached-rectangle gather:
// a Python loop around the same calls costs tens of microseconds per frame.
// The camera's lanes for a loop of L frames in flight: L render lanes and,
// with a gather, one comm lane (index RT_LOOP_MAX_LANES), created on first
// use, each with an event.
static int ensure_lanes(rt_camera* c, int L, bool comm) {
    int rc;
    for (int k = 0; k <= RT_LOOP_MAX_LANES; k++) {
        if (k >= L && !(comm && k == RT_LOOP_MAX_LANES)) continue;
        if (!c->lanes[k] && (rc = hip_check(hipStreamCreateWithFlags(&c->lanes[k], hipStreamNonBlocking), "lane stream")))
            return rc;
        if (!c->lane_ev[k] && (rc = hip_check(hipEventCreateWithFlags(&c->lane_ev[k], hipEventDisableTiming), "lane event")))
            return rc;
    }
    return RT_OK;
}

// rt_run_frames with RT_LOOP_MULTIFRAME: frames in launches of up to
// kPersistChunk frames, each one k_trace_kd3 grid of every frame's blocks,
// frame-major (render_common's PersistArgs).
// Until a cost order exists (tile order 3) frames launch one at a time, so
// that cost samples are taken; multi-frame launches take none.
constexpr int32_t kPersistChunk = 128;
// Each chunk of 4 or more frames as two concurrent launches of half the
// frames, on the render stream and a second lane, when the launches take
// 16-ray units (large fine regions): the driver's knot 1080p window 11.95-12.02k
// -> 12.31-12.38k FPS, 1,000 frames 12.20k -> 12.82k, dragon 1080p 20.21k ->
// 20.76k; 32-ray launches (960x540) lose 5 % and stay one launch (r05al).
#ifndef RT_MF_SPLIT
#define RT_MF_SPLIT 1
#endif

static int run_frames_multiframe(rt_camera* c, const rt_frame_loop* a, int32_t nframes, int64_t* seq,
                                 double* kernel_ms_avg, int32_t* kernel_ms_frames, double* host_ms) {
    // the frames of this call take the multi-frame rays-per-wave rule
    // (auto_rays); a change of rule is a change of launch geometry
    struct MfScope {
        rt_camera* c;
        explicit MfScope(rt_camera* cam) : c(cam) {
            if (!c->multiframe) { c->multiframe = true; c->geom_gen++; }
        }
        ~MfScope() { c->multiframe = false; c->geom_gen++; }
    } mf_scope(c);
    hipStream_t rs = (hipStream_t)a->render_stream;
    const rt_tile* tile = a->tile.nranks > 0 ? &a->tile : nullptr;
    // bracketed launches reuse a ring of kRing event pairs (single-frame
    // launches before a cost order exists would otherwise take a pair per
    // frame): a pair is read back before it is recorded again
    constexpr int kRing = 32;
    int32_t ring_frames[kRing] = {};
    int64_t nbracket = 0;
    double sum = 0.0;
    int32_t cnt = 0;
    auto harvest = [&](int slot) {
        float ms = 0.0f;
        if (hipEventSynchronize(c->loop_ev[(size_t)(2 * slot + 1)]) == hipSuccess &&
            hipEventElapsedTime(&ms, c->loop_ev[(size_t)(2 * slot)], c->loop_ev[(size_t)(2 * slot + 1)]) == hipSuccess) {
            sum += ms;
            cnt += ring_frames[slot];
        }
    };
    int rc = RT_OK;
    const int every = a->event_every;
    // the split (RT_MF_SPLIT) for launches of 16-ray units: the rays per
    // wave this call's launches take (the multi-frame rule of auto_rays, or
    // RT_OPT_RAYS), from the frame's geometry (static within the call)
    bool split_ok = false;
    if (RT_MF_SPLIT && a->mode == RT_MODE_KD && c->kernel_version == 3 && c->obj) {
        TraceParams tp{};
        split_ok = frame_geometry(camera_geom(c), a->xform, tile, a->mode, tp) && tp.rays != 32;
    }
    const auto h0 = std::chrono::steady_clock::now();
    for (int32_t j = 0; j < nframes && !rc;) {
        const bool have_order = c->tile_order < 3 || c->order.has_cost_order();
        const int32_t chunk = have_order ? std::min(nframes - j, kPersistChunk) : 1;
        const bool time_it = every > 0;
        const int pair = (int)(nbracket % kRing);
        if (time_it && (int64_t)c->loop_ev.size() < 2 * (pair + 1)) {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            if ((rc = hip_check(hipEventCreate(&e0), "loop timing event")) ||
                (rc = hip_check(hipEventCreate(&e1), "loop timing event")))
                break;
            c->loop_ev.push_back(e0);
            c->loop_ev.push_back(e1);
        }
        if (time_it && nbracket >= kRing) harvest(pair);
        if (time_it && (rc = hip_check(hipEventRecord(c->loop_ev[(size_t)(2 * pair)], rs), "loop timing"))) break;
        const int k = (int)((*seq) % a->nbuf);
        int32_t done = 1;
        if (split_ok && chunk >= 4 && (rc = ensure_lanes(c, 2, false)) == RT_OK) {
            // two launches of half the frames each, on the render stream and
            // a second lane at the same time (the two-lane loop's overlap of
            // one grid's tail with another's head, with multi-frame launches).
            // Both halves write the ring of buffer sets ((seq + f) % nbuf,
            // nbuf <= RT_LOOP_MAX_BUF, chunks of up to 128 frames), so two
            // concurrent frames can write the same set: correct only because
            // every frame of a multi-frame call is the same static frame --
            // rt_run_frames rejects per-frame transforms (nxforms > 0) and a
            // gather for RT_LOOP_MULTIFRAME, and this call passes the one
            // a->xform to both launches.
            const int32_t h1 = chunk / 2;
            hipStream_t s2 = c->lanes[1];
            if ((rc = hip_check(hipEventRecord(c->lane_ev[1], rs), "split fork")) ||
                (rc = hip_check(hipStreamWaitEvent(s2, c->lane_ev[1], 0), "split fork wait")))
                break;
            const PersistArgs p1{h1, (int32_t)((*seq) % a->nbuf), a->nbuf, a->d_local};
            rc = render_common(c, a->xform, a->mode, a->flags, tile, a->d_local[k], nullptr, rs, nullptr, &p1, &done);
            if (rc) break;
            if (done == h1) {
                const PersistArgs p2{chunk - h1, (int32_t)((*seq + h1) % a->nbuf), a->nbuf, a->d_local};
                int32_t done2 = 1;
                rc = render_common(c, a->xform, a->mode, a->flags, tile, a->d_local[(*seq + h1) % a->nbuf], nullptr, s2,
                                   nullptr, &p2, &done2);
                if (rc) break;
                done += done2;
            }
            if ((rc = hip_check(hipEventRecord(c->lane_ev[1], s2), "split join")) ||
                (rc = hip_check(hipStreamWaitEvent(rs, c->lane_ev[1], 0), "split join wait")))
                break;
        } else {
            if (rc) break;
            const PersistArgs pf{chunk, (int32_t)((*seq) % a->nbuf), a->nbuf, a->d_local};
            rc = render_common(c, a->xform, a->mode, a->flags, tile, a->d_local[k], nullptr, rs, nullptr,
                               chunk > 1 ? &pf : nullptr, &done);
        }
        if (rc) break;
        if (time_it) {
            if ((rc = hip_check(hipEventRecord(c->loop_ev[(size_t)(2 * pair + 1)], rs), "loop timing"))) break;
            ring_frames[pair] = done;
            nbracket++;
        }
        j += done;
        *seq += done;
    }
    if (host_ms) *host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
    c->nactive = 0;
    if (!rc) rc = hip_check(hipStreamSynchronize(rs), "loop sync");
    if (rc) {
        (void)hipDeviceSynchronize();
        return rc;
    }
    for (int64_t b = std::max<int64_t>(0, nbracket - kRing); b < nbracket; b++) harvest((int)(b % kRing));
    // per frame: the launches' bracketed time over the frames they rendered
    if (kernel_ms_avg) *kernel_ms_avg = cnt ? sum / cnt : 0.0;
    if (kernel_ms_frames) *kernel_ms_frames = cnt;
    return RT_OK;
}

extern "C" int rt_run_frames(rt_camera* c, rt_comm* comm, const rt_frame_loop* a, int32_t nframes, int64_t* seq,
                             double* kernel_ms_avg, int32_t* kernel_ms_frames, double* host_ms) {
    if (!c || !a || !seq || nframes < 0 || a->nbuf < 1 || a->nbuf > RT_LOOP_MAX_BUF ||
        (a->inflight < 0 && a->inflight != RT_LOOP_MULTIFRAME) || a->inflight > RT_LOOP_MAX_LANES)
        return fail(RT_ERR_INVALID, "rt_run_frames: bad argument");
    if (a->flags & RT_FLAG_WRITE_AOV)
        return fail(RT_ERR_INVALID, "rt_run_frames: RT_FLAG_WRITE_AOV is not available in frame loops");
    if (a->inflight == RT_LOOP_MULTIFRAME) {
        if (comm || a->nxforms > 0)
            return fail(RT_ERR_INVALID, "rt_run_frames: multi-frame launches render a static scene without a gather");
        for (int k = 0; k < a->nbuf; k++)
            if (!a->d_local[k]) return fail(RT_ERR_INVALID, "rt_run_frames: missing buffer of set %d", k);
        DeviceGuard g(c->device);
        return run_frames_multiframe(c, a, nframes, seq, kernel_ms_avg, kernel_ms_frames, host_ms);
    }
    if (a->nxforms < 0 || (a->nxforms > 0 && !a->xforms))
        return fail(RT_ERR_INVALID, "rt_run_frames: bad transform sequence");
    const int L = std::max(1, (int)a->inflight);
    // a set is rendered by one lane only: frames j and j + nbuf share a set,
    // and with nbuf a multiple of L they also share a lane, so they are
    // ordered (without a gather, and on rank 0's direct path, no event orders
    // two lanes' renders of one set: ADVICE r02)
    if (L > 1 && a->nbuf % L)
        return fail(RT_ERR_INVALID, "rt_run_frames: %d buffer sets for %d frames in flight (need a multiple)", a->nbuf, L);
    for (int k = 0; k < a->nbuf; k++)
        if (!a->d_local[k] || (comm && (!a->d_scratch[k] || !a->comm_stream)))
            return fail(RT_ERR_INVALID, "rt_run_frames: missing buffer of set %d", k);
    DeviceGuard g(c->device);
    hipStream_t rs = (hipStream_t)a->render_stream, cs = (hipStream_t)a->comm_stream;
    int rc;
    if (L > 1 && (rc = ensure_lanes(c, L, comm != nullptr))) return rc;
    // the streams frames are issued to: the caller's, or the camera's lanes
    hipStream_t lane[RT_LOOP_MAX_LANES];
    for (int l = 0; l < L; l++) lane[l] = L > 1 ? c->lanes[l] : rs;
    const hipStream_t gs = L > 1 && comm ? c->lanes[RT_LOOP_MAX_LANES] : cs;
    hipEvent_t rendered[RT_LOOP_MAX_BUF] = {}, sent[RT_LOOP_MAX_BUF] = {};
    bool used[RT_LOOP_MAX_BUF] = {};
    // the rectangle each set's frame was last assembled with in this call:
    // its background stands, so a frame with the same rectangle writes the
    // rectangle alone (the frame buffers are the loop's during the call)
    int32_t set_rect[RT_LOOP_MAX_BUF][4];
    auto cleanup = [&]() {
        c->nactive = 0;
        for (int k = 0; k < RT_LOOP_MAX_BUF; k++) {
            if (rendered[k]) (void)hipEventDestroy(rendered[k]);
            if (sent[k]) (void)hipEventDestroy(sent[k]);
        }
    };
    for (int k = 0; k < a->nbuf && comm; k++) {
        if ((rc = hip_check(hipEventCreateWithFlags(&rendered[k], hipEventDisableTiming), "loop event")) ||
            (rc = hip_check(hipEventCreateWithFlags(&sent[k], hipEventDisableTiming), "loop event"))) {
            cleanup();
            return rc;
        }
    }
    const int every = a->event_every;
    const int64_t ntimed = every > 0 ? (nframes + every - 1) / every : 0;
    while ((int64_t)c->loop_ev.size() < 2 * ntimed) {
        hipEvent_t e = nullptr;
        if ((rc = hip_check(hipEventCreate(&e), "loop timing event"))) {
            cleanup();
            return rc;
        }
        c->loop_ev.push_back(e);
    }
    // lanes start after the caller's queued work (fork) ...  A stream with
    // nothing queued needs no fork: its marker and the lanes' waits on it
    // would only delay the first frame by a cross-queue hop (~10 us).
    // (The second lane's first frame often starts only when the first lane's
    // first frame ends, 9-129 us after it in kernel traces; holding both
    // behind one event after a short sleep did not change that, r04n.)
    if (L > 1) {
        hipEvent_t fork = c->lane_ev[0];
        rc = RT_OK;
        if (hipStreamQuery(rs) != hipSuccess) {
            rc = hip_check(hipEventRecord(fork, rs), "lane fork");
            for (int l = 0; !rc && l < L; l++) rc = hip_check(hipStreamWaitEvent(lane[l], fork, 0), "lane fork wait");
        }
        if (!rc && comm && hipStreamQuery(cs) != hipSuccess &&
            (rc = hip_check(hipEventRecord(fork, cs), "lane fork")) == RT_OK)
            rc = hip_check(hipStreamWaitEvent(gs, fork, 0), "lane fork wait");
        if (rc) {
            cleanup();
            return rc;
        }
        c->nactive = L;
        for (int l = 0; l < L; l++) c->active[l] = lane[l];
    }
    // (a dispatch gate holding a lane's frame until the other lane's had
    // started a share of its blocks, and a sleep staggering the lanes,
    // measured slower at every setting: round 4, r04e-r04h)
    const rt_tile* tile = a->tile.nranks > 0 ? &a->tile : nullptr;
    // rank 0 renders its bands straight into the frame it assembles (its
    // part of the frame is never copied); the gather places the peers' parts
    int32_t crank = -1;
    if (comm && (rc = rt_comm_info(comm, nullptr, &crank))) {
        cleanup();
        return rc;
    }
    const bool direct = comm && crank == 0 && tile;
    // a peer's gather packs what its render wrote (render -> gather), and its
    // next render into the set waits for that pack (gather -> render); rank
    // 0's gather writes the peers' rows beside the rows its render writes,
    // so its lanes need no cross-queue events (each lane keeps frame order,
    // and the loop's end joins them)
    const bool linked = comm && !direct;
    for (int k = 0; direct && k < a->nbuf; k++)
        if (!a->d_frame[k]) {
            cleanup();
            return fail(RT_ERR_INVALID, "rt_run_frames: rank 0 has no frame buffer in set %d", k);
        }
    const auto h0 = std::chrono::steady_clock::now();
    for (int32_t j = 0; j < nframes && !rc; j++) {
        const int k = (int)((*seq) % a->nbuf);
        const float* xf = a->nxforms > 0 ? a->xforms + 12 * (size_t)((*seq) % a->nxforms) : a->xform;
        ++*seq;
        hipStream_t ls = lane[j % L];
        // set k is rendered again once the gather that last read it is done
        // (no barrier packet when that gather has already finished)
        if (linked && used[k] && hipEventQuery(sent[k]) != hipSuccess &&
            (rc = hip_check(hipStreamWaitEvent(ls, sent[k], 0), "render wait")))
            break;
        const bool timed = every > 0 && j % every == 0;
        const int64_t t = every > 0 ? j / every : 0;
        rc = timed ? hip_check(hipEventRecord(c->loop_ev[(size_t)(2 * t)], ls), "loop timing") : RT_OK;
        uint32_t* target = direct ? a->d_frame[k] : a->d_local[k];
        if (!rc)
            rc = render_common(c, xf, a->mode, a->flags | (direct ? RT_FLAG_FRAME_OUT : 0u), tile, target, nullptr, ls);
        if (!rc && timed) rc = hip_check(hipEventRecord(c->loop_ev[(size_t)(2 * t + 1)], ls), "loop timing");
        if (!rc && comm) {
            if (linked) {
                rc = hip_check(hipEventRecord(rendered[k], ls), "rendered");
                if (!rc) rc = hip_check(hipStreamWaitEvent(gs, rendered[k], 0), "comm wait");
            }
            int32_t rect[4] = {0, 0, 0, 0};
            bool rect_only = false;
            if (!rc && used[k]) {
                int32_t nranks = 1;
                rc = rt_comm_info(comm, &nranks, nullptr);
                if (!rc) rc = rt_frame_rect(c, xf, a->mode, nranks, rect);
                rect_only = !memcmp(rect, set_rect[k], sizeof rect);
            }
            if (!rc)
                rc = comm_gather_frame(comm, c, xf, a->mode, target, a->d_scratch[k], a->d_frame[k], gs,
                                       rect_only, set_rect[k]);
            if (!rc && linked) rc = hip_check(hipEventRecord(sent[k], gs), "sent");
        }
        used[k] = true;
    }
    if (host_ms) *host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
    // ... and the call returns once every lane has drained: the lanes
    // themselves are synchronised (a join into the caller's streams and a
    // wait on those would add a cross-queue hop to the last frame), so the
    // caller's later work is ordered after the loop
    c->nactive = 0;
    for (int l = 0; !rc && l < L; l++) rc = hip_check(hipStreamSynchronize(lane[l]), "loop sync");
    if (!rc && comm) rc = hip_check(hipStreamSynchronize(gs), "loop sync");
    if (!rc && L > 1) rc = hip_check(hipStreamSynchronize(rs), "loop sync");  // the fork's marker, if any
    if (!rc && L > 1 && comm) rc = hip_check(hipStreamSynchronize(cs), "loop sync");
    if (rc) (void)hipDeviceSynchronize();  // nothing of this loop may still use the events
    cleanup();
    if (rc) return rc;
    double sum = 0.0;
    int32_t cnt = 0;
    for (int64_t t = 0; t < ntimed; t++) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->loop_ev[(size_t)(2 * t)], c->loop_ev[(size_t)(2 * t + 1)]) == hipSuccess) {
            sum += ms;
            cnt++;
        }
    }
    if (kernel_ms_avg) *kernel_ms_avg = cnt ? sum / cnt : 0.0;
    if (kernel_ms_frames) *kernel_ms_frames = cnt;
    return RT_OK;
}
