// tile_order.h -- a camera's tile dispatch orders: the centre-out permutation
// of each fine grid in a ring of device slots, the cost samples and cost
// orders of tile orders 3, 4 and 5, the split tiles at a cost order's head,
// the cost orders kept for the last two grids, and the waits that keep frames
// on other streams behind an order's upload.  The arithmetic is
// tile_order_host.h's; this is its state and its HIP resources.
//
// A render calls prepare (when its launch geometry is derived), then
// before_launch and after_launch around its launch.  Nothing is sampled,
// restored or uploaded behind a stream that is being captured into a graph.
#pragma once

#include "rt_internal.h"
#include "tile_order_host.h"

namespace rt {

struct TileOrder {
    TileOrder() = default;
    TileOrder(const TileOrder&) = delete;
    TileOrder& operator=(const TileOrder&) = delete;
    ~TileOrder();  // (with the camera's device current)

    // The order of p's fine grid for a render on st (a new grid: a new
    // slot, uploaded behind st) and, for a cost-ordered render (tile order
    // 3, 4 or 5 of kernel 3), the cost buffers and a kept order of this grid.
    // *order: the device permutation, or null (tile orders 0 and 1, an empty
    // grid).  *cost: non-null marks a cost-ordered render (before_launch
    // passes it to the kernel of sampled frames only).
    int prepare(const TraceParams& p, int kernel, hipStream_t st, const int32_t** order, uint32_t** cost);
    // Before the launch on st: waits for an upload of p.order on another
    // stream, p.split, and whether this frame is a cost sample (never one of
    // a multi-frame launch, `persist`): p.cost is then the zeroed sample
    // buffer, and null otherwise.
    int before_launch(TraceParams& p, hipStream_t st, bool persist, bool* sampled);
    // After it: st (and the side stream of debug bit 8, or null) read the
    // current slot; a cost-ordered render then turns an arrived sample into
    // the next order, or queues the sample's event.
    int after_launch(const TraceParams& p, hipStream_t st, hipStream_t side, bool cost_ordered, bool sampled);
    // Kept cost orders measured another object or tree.
    void forget_kept();

    bool has_cost_order() const { return order_gen == layout_gen; }  // the current grid renders in one
    int32_t split() const { return order_split; }
    uint64_t restores() const { return restores_; }
    Hold hold;  // the fine region renders keep (hold_region)

private:
    int ensure_order(const TileGrid& g, int debug, hipStream_t st);
    int ensure_cost(int64_t n);
    int restore_order(int64_t n, hipStream_t st);
    int cost_feedback(const TraceParams& p, hipStream_t st, bool sampled);
    void keep_order(const std::vector<int32_t>& ord, int32_t split);
    bool cost_sample_now(hipStream_t st);
    void note_order_stream(hipStream_t st);

    int32_t* d_order = nullptr;      // the current tile permutation (a slot's buffer)
    int64_t order_key[kOrderKey] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};
    // Tile permutations live in a ring of slots: a new fine grid (a moving
    // object changes it every frame) writes the next slot behind the
    // caller's stream instead of rewriting the buffer earlier frames still
    // read.  A slot is retired with an event on every stream that used it,
    // and written again kOrderSlots grids later, once those have fired.
    struct OrderSlot {
        int32_t* d = nullptr;        // device permutation
        int32_t* h = nullptr;        // pinned source of its upload
        int64_t cap = 0;
        hipEvent_t ev[8] = {};
        int nev = 0;
        bool device_sync = false;    // used by more streams than ev holds
        // frames in flight: the upload's event and stream; a frame on
        // another lane waits for it only when it renders with this slot
        hipEvent_t up_ev = nullptr;
        hipStream_t up_stream = nullptr;
        bool up_valid = false;
    } oslot[8];
    int ocur = -1;
    hipStream_t oused[8] = {};       // streams that launched with the current slot
    int noused = 0;
    bool oused_overflow = false;
    std::vector<int32_t> centre;     // centre-out permutation of the current fine grid (host copy)
    // tile order 3: each frame's per-unit pool iterations feed the next
    // frames' dispatch order, read back asynchronously (never a sync).
    // one buffer per stream that renders (cost_set): a sample copies the
    // buffer of the stream that queues it, which only that stream's frames
    // write, so frames in flight on other lanes (under motion, with another
    // fine grid) never tear it
    hipEvent_t slot_join_ev[8] = {};  // cost-order upload: joins the streams that read the slot
    hipStream_t cost_up_stream = nullptr;   // the last cost-order upload's stream ...
    bool cost_up_valid = false;             // ... while it may be pending
    uint32_t* h_cost = nullptr;      // pinned: [tile][kCostSlots] pool iterations, written by a sampled frame
    uint32_t* d_cost_host = nullptr; // its device address
    int32_t* h_order = nullptr;      // pinned H2D source
    int64_t host_cap = 0;            // tiles h_cost / h_order hold
    hipEvent_t cost_ev = nullptr, order_ev = nullptr;
    bool cost_pending = false, order_pending = false;
    int frames_since = 0;
    uint64_t layout_gen = 0, cost_gen = 0;   // fine-grid generation, and the one h_cost was read for
    // The order ranks tiles by the cost of one wave per unit (pool
    // iterations).  Split halves report an estimate, so each tile's cost as
    // last measured unsplit is remembered (per grid) and used while it
    // renders split: sample_split holds, per tile, whether the sampled frame
    // rendered it split (taken when the sample is queued).
    std::vector<uint8_t> sample_split;
    std::vector<uint32_t> cost_mem;
    uint64_t mem_gen = ~0ull;
    uint64_t order_gen = ~0ull;              // generation whose cost order d_order holds
    int32_t order_split = 0;                 // split tiles at the head of that cost order
    // the last cost orders of two grids (order_key): a camera that
    // alternates between two tilings -- rt_run_frames' multi-frame rays rule
    // against the per-frame one on a small frame -- starts each
    // switch with the order it last measured there, not the centre order
    struct KeptOrder {
        int64_t key[kOrderKey] = {};
        std::vector<int32_t> ord;
        std::vector<uint32_t> mem;  // cost_mem with it
        int32_t split = 0;
    };
    KeptOrder kept[2];
    int kept_next = 0;
    uint64_t restores_ = 0;          // kOptOrderRestores: kept orders restored
};

}  // namespace rt
