// tile_order.cpp -- TileOrder (tile_order.h): the order slots, the cost
// samples and the uploads behind the caller's streams.
#include "tile_order.h"

#include <string.h>

#include "rt_hip.h"

namespace rt {

namespace {

constexpr int kOrderSlots = 8;
constexpr int kCostPeriod = 16;  // frames between cost samples (tile order 3)

TileGrid grid_of(const TraceParams& p) {
    TileGrid g;
    g.tile_w = p.tile_w; g.tile_h = p.tile_h;
    g.tiles_x = p.tiles_x; g.block_rows = p.block_rows;
    g.nranks = p.nranks; g.rank = p.rank;
    g.fine_tx0 = p.fine_tx0; g.fine_s0 = p.fine_s0;
    g.rays = p.rays;
    g.w = p.w; g.h = p.h; g.nslots = p.nslots;
    return g;
}

bool capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

}  // namespace

TileOrder::~TileOrder() {
    for (auto& o : oslot) {
        dev_free(o.d);
        if (o.h) (void)hipHostFree(o.h);
        for (hipEvent_t e : o.ev)
            if (e) (void)hipEventDestroy(e);
        if (o.up_ev) (void)hipEventDestroy(o.up_ev);
    }
    d_order = nullptr;
    for (hipEvent_t e : slot_join_ev)
        if (e) (void)hipEventDestroy(e);
    if (h_cost) (void)hipHostFree(h_cost);
    if (h_order) (void)hipHostFree(h_order);
    if (cost_ev) (void)hipEventDestroy(cost_ev);
    if (order_ev) (void)hipEventDestroy(order_ev);
}

void TileOrder::forget_kept() {
    for (auto& e : kept) e = KeptOrder();
    kept_next = 0;
}

int TileOrder::prepare(const TraceParams& p, int kernel, hipStream_t st, const int32_t** order, uint32_t** cost) {
    *order = nullptr;
    *cost = nullptr;
    if (p.tile_order >= 2 && p.tiles_x * p.block_rows > 0) {
        const TileGrid g = grid_of(p);
        int rc = ensure_order(g, p.debug, st);
        if (rc) return rc;
        *order = d_order;
        if (p.tile_order >= 3 && kernel == 3) {
            if ((rc = ensure_cost(std::max<int64_t>(all_tiles(g, p.debug), g.tiles()))) ||
                (rc = restore_order(g.tiles(), st)))
                return rc;
            *cost = d_cost_host;  // (marks tile order 3; before_launch passes it to sampled frames only)
        }
    }
    return RT_OK;
}

int TileOrder::before_launch(TraceParams& p, hipStream_t st, bool persist, bool* sampled) {
    int rc;
    // a slot (or its cost order) uploaded on another stream: this frame's
    // launch waits for it (no barrier packet once the upload has landed)
    for (int k = 0; p.order && k < kOrderSlots; k++) {
        auto& o = oslot[k];
        if (o.d != p.order || !o.up_valid || o.up_stream == st) continue;
        if (hipEventQuery(o.up_ev) == hipSuccess) o.up_valid = false;
        else if ((rc = hip_check(hipStreamWaitEvent(st, o.up_ev, 0), "order upload wait"))) return rc;
    }
    if (p.order && p.order == d_order && cost_up_valid && cost_up_stream != st) {
        if (hipEventQuery(order_ev) == hipSuccess) cost_up_valid = false;
        else if ((rc = hip_check(hipStreamWaitEvent(st, order_ev, 0), "cost order wait"))) return rc;
    }
    // split tiles of the cost order in d_order (launches are stream-ordered
    // behind its upload; other streams wait for it above)
    p.split = (p.order && p.order == d_order && p.cost && (p.rays == 16 || (p.rays == 8 && RT_SPLIT8)) &&
               !(p.debug & 512)) ? order_split : 0;
    *sampled = p.cost != nullptr && !persist && cost_sample_now(st);
    if (*sampled) {
        p.cost = d_cost_host;
        // the kernel writes this frame's costs into the pinned host buffer;
        // slots a tile does not write (missing waves) read 0
        memset(h_cost, 0, sizeof(uint32_t) * kCostSlots * (size_t)p.tiles_x * p.block_rows);
    } else {
        p.cost = nullptr;
    }
    return RT_OK;
}

int TileOrder::after_launch(const TraceParams& p, hipStream_t st, hipStream_t side, bool cost_ordered, bool sampled) {
    if (p.order) {  // the streams that read the current order slot
        note_order_stream(st);
        if (side) note_order_stream(side);
    }
    return cost_ordered ? cost_feedback(p, st, sampled) : RT_OK;
}

// The current slot was launched with on `st`.
void TileOrder::note_order_stream(hipStream_t st) {
    for (int i = 0; i < noused; i++)
        if (oused[i] == st) return;
    if (noused < 8) oused[noused++] = st;
    else oused_overflow = true;
}

int TileOrder::ensure_order(const TileGrid& p, int debug, hipStream_t st) {
    int64_t key[kOrderKey];
    p.key(key);
    if (std::equal(key, key + kOrderKey, order_key)) return RT_OK;
    const int64_t n = p.tiles();
    std::vector<int32_t> order = centre_order(p);
    int rc;
    // retire the current slot: an event on each stream that launched with it
    // (a pending cost-order upload into it was issued on one of them)
    if (ocur >= 0) {
        auto& o = oslot[ocur];
        o.nev = 0;
        o.device_sync = oused_overflow;
        for (int i = 0; i < noused && !o.device_sync; i++) {
            if (!o.ev[i] && (rc = hip_check(hipEventCreateWithFlags(&o.ev[i], hipEventDisableTiming), "order event")))
                return rc;
            if ((rc = hip_check(hipEventRecord(o.ev[i], oused[i]), "order retire"))) return rc;
            o.nev++;
        }
    }
    noused = 0;
    oused_overflow = false;
    // the next slot, once every launch that read it (and its upload) is done
    const int sl = (ocur + 1) % kOrderSlots;
    auto& o = oslot[sl];
    rc = RT_OK;
    if (o.device_sync) rc = hip_check(hipDeviceSynchronize(), "order slot sync");
    for (int i = 0; !rc && i < o.nev; i++) rc = hip_check(hipEventSynchronize(o.ev[i]), "order slot wait");
    if (rc) return rc;
    o.nev = 0;
    o.device_sync = false;
    if (o.cap < n) {
        const int64_t want = std::max(n, all_tiles(p, debug));
        dev_free(o.d);
        if (o.h) (void)hipHostFree(o.h);
        o.h = nullptr;
        o.cap = 0;
        if ((rc = dev_alloc(&o.d, (size_t)want, "hipMalloc(order)")) ||
            (rc = hip_check(hipHostMalloc((void**)&o.h, sizeof(int32_t) * (size_t)want, 0), "hipHostMalloc(order)")))
            return rc;
        o.cap = want;
    }
    std::copy(order.begin(), order.end(), o.h);
    if ((rc = hip_check(hipMemcpyAsync(o.d, o.h, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st), "H2D order")))
        return rc;
    // frames in flight on other lanes that render with this slot wait for
    // the upload (order_wait); a moving object's next grid, on the other
    // lane, has a slot of its own and does not (a wait on every lane here
    // tied each lane's next frame to the other's previous one)
    // (always recorded: a caller that renders on several streams of its own
    // needs the wait as much as the library's lanes do)
    o.up_valid = false;
    if (!o.up_ev && (rc = hip_check(hipEventCreateWithFlags(&o.up_ev, hipEventDisableTiming), "order event")))
        return rc;
    if ((rc = hip_check(hipEventRecord(o.up_ev, st), "order upload event"))) return rc;
    o.up_stream = st;
    o.up_valid = true;
    cost_up_valid = false;  // a cost order of the previous slot
    ocur = sl;
    d_order = o.d;
    order_gen = ~0ull;  // no cost order for this grid yet
    order_split = 0;    // nor split tiles
    std::copy(key, key + kOrderKey, order_key);
    centre.swap(order);
    layout_gen++;
    // tile order 3: sample the new grid's costs once it has held for two
    // frames (a moving object changes it every frame; its samples would
    // always be stale)
    frames_since = kCostPeriod - 2;
    return RT_OK;
}

// Buffers of tile order 3 for n fine tiles (allocated when the grid grows).
int TileOrder::ensure_cost(int64_t n) {
    int rc;
    if (host_cap < n) {
        // copies in flight may still use the pinned buffers
        if (cost_pending) (void)hipEventSynchronize(cost_ev);
        if (order_pending) (void)hipEventSynchronize(order_ev);
        if (h_cost) (void)hipHostFree(h_cost);
        if (h_order) (void)hipHostFree(h_order);
        h_cost = nullptr;
        d_cost_host = nullptr;
        h_order = nullptr;
        host_cap = 0;
        cost_pending = order_pending = false;
        if ((rc = hip_check(hipHostMalloc((void**)&h_cost, sizeof(uint32_t) * kCostSlots * (size_t)n, 0), "hipHostMalloc(cost)")) ||
            (rc = hip_check(hipHostMalloc((void**)&h_order, sizeof(int32_t) * (size_t)n, 0), "hipHostMalloc(order)")) ||
            (rc = hip_check(hipHostGetDevicePointer((void**)&d_cost_host, h_cost, 0), "cost device pointer")))
            return rc;
        host_cap = n;
    }
    if (!cost_ev && (rc = hip_check(hipEventCreateWithFlags(&cost_ev, hipEventDisableTiming), "cost event")))
        return rc;
    if (!order_ev && (rc = hip_check(hipEventCreateWithFlags(&order_ev, hipEventDisableTiming), "order event")))
        return rc;
    return RT_OK;
}

// Whether the frame about to launch on `st` is a cost sample: its kernel then
// writes its units' costs into h_cost (zeroed by before_launch) instead of
// nothing.
bool TileOrder::cost_sample_now(hipStream_t st) {
    if (cost_pending || frames_since + 1 < kCostPeriod || !h_cost) return false;
    return !capturing(st);
}

void TileOrder::keep_order(const std::vector<int32_t>& ord, int32_t split) {
    KeptOrder* k = nullptr;
    for (auto& e : kept)
        if (std::equal(e.key, e.key + kOrderKey, order_key)) k = &e;
    if (!k) {
        k = &kept[kept_next];
        kept_next ^= 1;
    }
    std::copy(order_key, order_key + kOrderKey, k->key);
    k->ord = ord;
    k->mem = cost_mem;
    k->split = split;
}

// A fresh grid (no cost order yet) that held a cost order before: upload it
// (on st, behind ensure_order's centre order; frames on other streams wait
// for it as for cost_feedback's uploads).
int TileOrder::restore_order(int64_t n, hipStream_t st) {
    if (order_gen == layout_gen || n > host_cap) return RT_OK;
    // the previous grid's last cost-order upload reads h_order: wait for it
    // by query only (cost_feedback clears the flag at its next sample)
    if (order_pending) {
        if (hipEventQuery(order_ev) != hipSuccess) return RT_OK;
        order_pending = false;
    }
    if (capturing(st)) return RT_OK;
    const KeptOrder* k = nullptr;
    for (const auto& e : kept)
        if ((int64_t)e.ord.size() == n && std::equal(e.key, e.key + kOrderKey, order_key)) k = &e;
    if (!k || noused > 0) return RT_OK;  // (only before the grid's first launch)
    std::copy(k->ord.begin(), k->ord.end(), h_order);
    int rc;
    if ((rc = hip_check(hipMemcpyAsync(d_order, h_order, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st),
                        "H2D kept cost order")) ||
        (rc = hip_check(hipEventRecord(order_ev, st), "order event")))
        return rc;
    cost_up_stream = st;
    cost_up_valid = true;
    order_pending = true;
    order_split = k->split;
    order_gen = layout_gen;
    restores_++;
    if ((int64_t)k->mem.size() == n) {
        cost_mem = k->mem;
        mem_gen = layout_gen;
    }
    return RT_OK;
}

// After a tile-order-3 frame: when an earlier cost sample has arrived, order
// the tiles by it (heaviest unit first, centre-out among equals) and upload
// the order behind this frame.  Every kCostPeriod frames one frame is the
// sample: its kernel writes its units' costs straight into pinned host memory
// (cost_sample_now / h_cost; no copy kernel, and the other frames write
// no costs), and an event after it says when the sample has arrived.
// Non-blocking (events are only queried); skipped while the stream is being
// captured into a graph.
int TileOrder::cost_feedback(const TraceParams& p, hipStream_t st, bool sampled) {
    if (capturing(st)) return RT_OK;
    const int64_t n = (int64_t)p.tiles_x * p.block_rows;
    if (cost_pending) {
        if (hipEventQuery(cost_ev) != hipSuccess) return RT_OK;
        if (order_pending && hipEventQuery(order_ev) != hipSuccess) return RT_OK;
        cost_pending = order_pending = false;
        frames_since = 0;
        if (cost_gen != layout_gen || (int64_t)centre.size() != n) return RT_OK;  // stale sample
        // the sampled costs, with the remembered unsplit cost of each tile the
        // sampled frame rendered split (effective_costs)
        if (mem_gen != layout_gen || (int64_t)cost_mem.size() != n) {
            cost_mem.assign((size_t)n, 0u);
            mem_gen = layout_gen;
        }
        std::vector<uint32_t> eff(h_cost, h_cost + kCostSlots * (size_t)n);
        effective_costs(eff, sample_split, cost_mem);
        const std::vector<int32_t> ord =
            cost_order(grid_of(p), centre.data(), p.tile_order == 4 ? 1 : p.tile_order == 5 ? 2 : 0, eff.data());
        bool same = true;
        for (int64_t k = 0; k < n; k++) {
            same = same && h_order[k] == ord[(size_t)k];
            h_order[k] = ord[(size_t)k];
        }
        const int32_t split = split_count(n, ord.data(), eff.data(), p.tile_order, p.rays, p.debug);
        same = same && split == order_split;
        if (same && order_gen == layout_gen) return RT_OK;  // d_order already holds it
        int rc;
        // frames on other streams (frames in flight on the library's lanes,
        // or a caller's own streams) read d_order: the upload waits for every
        // stream that launched with this slot, and a later frame on another
        // stream waits for the upload (before_launch)
        if (oused_overflow && (rc = hip_check(hipDeviceSynchronize(), "cost order sync"))) return rc;
        for (int i = 0; i < noused && !oused_overflow; i++) {
            if (oused[i] == st) continue;
            if (!slot_join_ev[i] &&
                (rc = hip_check(hipEventCreateWithFlags(&slot_join_ev[i], hipEventDisableTiming), "join event")))
                return rc;
            if ((rc = hip_check(hipEventRecord(slot_join_ev[i], oused[i]), "slot join")) ||
                (rc = hip_check(hipStreamWaitEvent(st, slot_join_ev[i], 0), "slot join wait")))
                return rc;
        }
        if ((rc = hip_check(hipMemcpyAsync(d_order, h_order, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st),
                            "H2D cost order")) ||
            (rc = hip_check(hipEventRecord(order_ev, st), "order event")))
            return rc;
        cost_up_stream = st;
        cost_up_valid = true;
        order_pending = true;
        order_split = split;  // launches after this upload (stream order) use it
        order_gen = layout_gen;
        keep_order(ord, split);
        return RT_OK;
    }
    if (!sampled) {
        ++frames_since;
        return RT_OK;
    }
    int rc;
    if ((rc = hip_check(hipEventRecord(cost_ev, st), "cost event"))) return rc;
    cost_pending = true;
    cost_gen = layout_gen;
    // which tiles the order this frame launched with rendered split
    // (before_launch: order[0..split))
    sample_split.assign((size_t)n, 0);
    if (order_gen == layout_gen)
        for (int32_t k = 0; k < p.split && k < n; k++) {
            const int32_t t = h_order[k];
            if (t >= 0 && t < n) sample_split[(size_t)t] = 1;
        }
    return RT_OK;
}

}  // namespace rt
