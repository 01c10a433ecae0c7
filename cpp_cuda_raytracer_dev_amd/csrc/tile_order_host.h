// tile_order_host.h -- the arithmetic of the tile dispatch orders: plain
// functions over a grid description, no HIP and no camera, so a CPU program
// (tests/tile_order_main.cpp) can run them under a sanitizer.  The state and
// the HIP resources around them are tile_order.h's TileOrder.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rt_tile_consts.h"

namespace rt {

// A tile grid's cost-order key (TileGrid::key): tile shape, grid size, ranks,
// fine-region origin, rays per wave.
constexpr int kOrderKey = 9;

// One fine grid of a camera: the key's values, the frame and this rank's
// band slots.
struct TileGrid {
    int32_t tile_w = 0, tile_h = 0, tiles_x = 0, block_rows = 0, nranks = 1, rank = 0, fine_tx0 = 0, fine_s0 = 0;
    int32_t rays = 0;
    int32_t w = 0, h = 0, nslots = 0;
    int64_t tiles() const { return (int64_t)tiles_x * block_rows; }
    // (the rays per wave too: 16- and 32-ray units both tile 8 x 8, and a cost
    // order measured with one is kept for it, keep_order / restore_order)
    void key(int64_t k[kOrderKey]) const {
        const int64_t v[kOrderKey] = {tile_w, tile_h, tiles_x, block_rows, nranks, rank, fine_tx0, fine_s0, rays};
        std::copy(v, v + kOrderKey, k);
    }
};

// Tiles of this rank's whole frame in g's tiling: the most any fine grid of
// this camera and tiling holds.  Order slots and cost buffers are sized for
// it, so a moving object's growing grid never reallocates them (each
// reallocation freed device memory, a device-wide synchronisation, and
// re-pinned host memory).
inline int64_t all_tiles(const TileGrid& g, int debug) {
    if (debug & 64) return 0;  // A/B: sized for the current grid only
    return (int64_t)((g.w + g.tile_w - 1) / g.tile_w) * g.nslots * (kTileH / g.tile_h);
}

// Centre-out permutation of the launch's tiles: blocks are dispatched in
// index order, so the expensive tiles (the object sits mid-frame) start
// first and the cheap background tiles fill in behind them.
inline std::vector<int32_t> centre_order(const TileGrid& p) {
    const int64_t n = (int64_t)p.tiles_x * p.block_rows;
    const int64_t per_band = kTileH / p.tile_h;
    // centre-out: a counting sort of the tiles by their distance from the
    // frame centre in 2-pixel rings, index order within a ring (O(n): a
    // moving object changes the grid every frame, and a comparison sort of
    // the 13k tiles of a 1080p frame took ~0.3 ms of host time per frame)
    std::vector<int32_t> order((size_t)n), ring((size_t)n);
    const double cx = 0.5 * p.w, cy = 0.5 * p.h;
    const int32_t nring = (int32_t)(0.5 * std::sqrt(cx * cx + cy * cy)) + 2;
    std::vector<int32_t> start((size_t)nring + 1, 0);
    // row by row, the column terms once (a moving object recomputes this
    // every frame: four 64-bit divisions per tile cost ~100 us of host time
    // per 1080p frame)
    std::vector<double> dx2((size_t)p.tiles_x);
    for (int64_t c0 = 0; c0 < p.tiles_x; c0++) {
        const double x = ((c0 + p.fine_tx0) + 0.5) * p.tile_w;
        dx2[(size_t)c0] = (x - cx) * (x - cx);
    }
    for (int64_t row = 0, t = 0; row < p.block_rows; row++) {
        const int64_t slot = row / per_band + p.fine_s0, yin = (row % per_band) * p.tile_h;
        const double y = (double)((p.rank + slot * (int64_t)p.nranks) * kTileH + yin) + 0.5 * p.tile_h;
        const double dy2 = (y - cy) * (y - cy);
        for (int64_t c0 = 0; c0 < p.tiles_x; c0++, t++) {
            const int32_t k = std::min(nring - 1, (int32_t)(0.5 * std::sqrt(dx2[(size_t)c0] + dy2)));
            ring[(size_t)t] = k;
            start[(size_t)k + 1]++;
        }
    }
    for (int32_t k = 0; k < nring; k++) start[(size_t)k + 1] += start[(size_t)k];
    for (int64_t t = 0; t < n; t++) order[(size_t)start[(size_t)ring[(size_t)t]]++] = (int32_t)t;
    return order;
}

// Dispatch order from the sampled costs (pool iterations of each tile's
// waves).  Order 3: heaviest tile first (counting sort, stable over the
// centre-out order).  Order 4: the tiles in Morton order are cut into 8 runs
// of equal total cost, one per XCD (blocks b and b + 8 share an XCD), each
// run heaviest first, interleaved so block b takes the next tile of run b % 8:
// the XCDs finish together and each L2 serves one screen region's subtrees.
// Order 5 (round 6, verdict r05 item 5): order 0's XCD mapping (8 runs of
// equal tile count, contiguous in row-major order: each XCD a band of the
// fine region's rows), each run heaviest first, interleaved the same way.
// Multi-frame launches pad every frame's grid to a multiple of 8 blocks for
// orders 0, 4 and 5 (render_common), so block b of every frame lands on XCD
// b % 8; these orders render no split tiles.
// xcd_mode 0 / 1 / 2: tile orders 3 / 4 / 5; centre: centre_order(p).
inline std::vector<int32_t> cost_order(const TileGrid& p, const int32_t* centre, int xcd_mode, const uint32_t* cost) {
    const bool xcd_split = xcd_mode != 0;
    const int64_t n = (int64_t)p.tiles_x * p.block_rows;
    uint32_t mx = 0;
    auto wave_max = [&](int64_t t) {
        uint32_t m = 0;
        for (int k = 0; k < kCostSlots; k++) m = std::max(m, cost[kCostSlots * (size_t)t + k]);
        return m;
    };
    auto wave_sum = [&](int64_t t) {
        double m = 0;
        for (int k = 0; k < kCostSlots; k++) m += cost[kCostSlots * (size_t)t + k];
        return m;
    };
    for (int64_t t = 0; t < n; t++) mx = std::max(mx, wave_max(t));
    mx = std::min<uint32_t>(mx, 1u << 16);
    auto cost_of = [&](int32_t t) { return std::min<uint32_t>(wave_max(t), mx); };
    // stable counting sort of `in` by cost, descending, appended to `out`
    std::vector<int64_t> start((size_t)mx + 2);
    auto sort_desc = [&](const int32_t* in, int64_t m, int32_t* out) {
        std::fill(start.begin(), start.end(), 0);
        for (int64_t k = 0; k < m; k++) start[(size_t)(mx - cost_of(in[k])) + 1]++;
        for (size_t k = 1; k < start.size(); k++) start[k] += start[k - 1];
        for (int64_t k = 0; k < m; k++) out[start[(size_t)(mx - cost_of(in[k]))]++] = in[k];
    };
    std::vector<int32_t> ord((size_t)n);
    if (!xcd_split) {
        sort_desc(centre, n, ord.data());
        return ord;
    }
    // Morton order of the tiles (pixel-proportional coordinates)
    std::vector<std::pair<uint64_t, int32_t>> mk((size_t)n);
    auto spread = [](uint64_t v) {
        v &= 0xFFFFFFFFull;
        v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
        v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
        v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
        v = (v | (v << 2)) & 0x3333333333333333ull;
        v = (v | (v << 1)) & 0x5555555555555555ull;
        return v;
    };
    for (int64_t t = 0; t < n; t++) {
        const uint64_t x = (uint64_t)(t % p.tiles_x) * (uint64_t)p.tile_w, y = (uint64_t)(t / p.tiles_x) * (uint64_t)p.tile_h;
        // order 5: row-major (the tile index itself)
        mk[(size_t)t] = {xcd_mode == 2 ? (uint64_t)t : (spread(x) | (spread(y) << 1)), (int32_t)t};
    }
    std::sort(mk.begin(), mk.end());
    double total = 0.0;
    for (int64_t t = 0; t < n; t++) total += 1.0 + wave_sum(t);
    constexpr int kXcd = 8;
    std::vector<int32_t> runs((size_t)n);
    int64_t cut[kXcd + 1] = {0};
    int r = 1;
    if (xcd_mode == 2) {
        // equal tile counts: block b (XCD b % 8) takes tile k = b / 8 of run
        // b % 8, as order 0 does
        for (; r < kXcd; r++) cut[r] = (n * r) / kXcd;
    } else {
        double acc = 0.0;
        for (int64_t k = 0; k < n && r < kXcd; k++) {
            const int32_t t = mk[(size_t)k].second;
            acc += 1.0 + wave_sum(t);
            while (r < kXcd && acc >= total * r / kXcd) cut[r++] = k + 1;
        }
    }
    while (r <= kXcd) cut[r++] = n;
    std::vector<int32_t> in((size_t)n);
    for (int64_t k = 0; k < n; k++) in[(size_t)k] = mk[(size_t)k].second;
    for (int x = 0; x < kXcd; x++) sort_desc(in.data() + cut[x], cut[x + 1] - cut[x], runs.data() + cut[x]);
    int64_t pos[kXcd];
    for (int x = 0; x < kXcd; x++) pos[x] = cut[x];
    for (int64_t b = 0; b < n; b++) {
        int x = (int)(b % kXcd);
        if (pos[x] == cut[x + 1]) {  // run exhausted: the run with most tiles left
            int best = -1;
            for (int y = 0; y < kXcd; y++)
                if (pos[y] < cut[y + 1] && (best < 0 || cut[y + 1] - pos[y] > cut[best + 1] - pos[best])) best = y;
            x = best;
        }
        ord[(size_t)b] = runs[(size_t)pos[x]++];
    }
    return ord;
}

// The sampled costs `eff` ([tile][kCostSlots], edited in place), with the
// remembered unsplit cost (cost_mem, one per tile) of each tile the sampled
// frame rendered split (sample_split, per tile, or of another size: none
// did): a half reports an estimate.  A tile sampled unsplit is remembered.
inline void effective_costs(std::vector<uint32_t>& eff, const std::vector<uint8_t>& sample_split,
                            std::vector<uint32_t>& cost_mem) {
    const int64_t n = (int64_t)cost_mem.size();
    const bool have_flags = (int64_t)sample_split.size() == n;
    for (int64_t t = 0; t < n; t++) {
        uint32_t* e = eff.data() + kCostSlots * (size_t)t;
        uint32_t m = 0;
        for (int k = 0; k < kCostSlots; k++) m = std::max(m, e[k]);
        const uint8_t mode = have_flags ? sample_split[(size_t)t] : 0;
        if (mode && cost_mem[(size_t)t] > 0) {
            for (int k = 0; k < kCostSlots; k++) e[k] = 0u;
            e[0] = cost_mem[(size_t)t];
        } else if (!mode) {
            cost_mem[(size_t)t] = m;
        }
    }
}

// Grids of fewer than this many 16-ray tiles (4 units each) split the tiles
// above RT_SPLIT_PCT % of the heaviest, larger ones only those above
// RT_SPLIT_PCT_LARGE %: at 1080p (3.4k tiles) splitting half the top measured
// slower with two frames in flight (dragon 16.2k -> 15.6k FPS, knot 10.19k ->
// 10.08k), at 960x540 (850 tiles) much faster (dragon 33.7k -> 44.5k, r03g).
#ifndef RT_SPLIT_MAX_TILES
#define RT_SPLIT_MAX_TILES 2048
#endif
constexpr int64_t kSplitMaxTiles = RT_SPLIT_MAX_TILES;
// which tiles split: cost > RT_SPLIT_PCT % of the top, at most n / RT_SPLIT_CAP_DIV
#ifndef RT_SPLIT_PCT
#define RT_SPLIT_PCT 50
#endif
// grids of kSplitMaxTiles or more: only tiles above RT_SPLIT_PCT_LARGE % of
// the top (with deterministic split costs, r03zf: dragon 1080p solo 74.0 ->
// 71.7 us, knot 107.1 -> 104.7 us, FPS unchanged; 0: no split there)
#ifndef RT_SPLIT_PCT_LARGE
#define RT_SPLIT_PCT_LARGE 75
#endif
#ifndef RT_SPLIT_CAP_DIV
#define RT_SPLIT_CAP_DIV 4
#endif
// 8-ray units split into 4-pixel halves as well (with two-level iterations:
// ranks of 8 at 1080p, dragon 16.8-19.4 -> 16.3-19.0 us per rank, knot max
// 26.7 -> 21.9 us, r03z)
#ifndef RT_SPLIT8
#define RT_SPLIT8 1
#endif

// Split tiles (order 3, 16-ray units): the tiles costlier than half
// the heaviest render as two 8-ray halves, so the heaviest chains
// end near the unsplit ones' (a unit's chain is mostly its items:
// half the rays, about half the pool iterations); at most a quarter
// of the tiles.  Debug bit 512: none.
// ord: the cost order of the n tiles, eff: their effective costs.
inline int32_t split_count(int64_t n, const int32_t* ord, const uint32_t* eff, int tile_order, int rays, int debug) {
    int32_t split = 0;
    auto cost_of = [&](int64_t t) {
        uint32_t m = 0;
        for (int k = 0; k < kCostSlots; k++) m = std::max(m, eff[kCostSlots * (size_t)t + k]);
        return m;
    };
    const uint32_t top = n > 0 ? cost_of(ord[0]) : 0;
    if (tile_order == 3 && (rays == 16 || (rays == 8 && RT_SPLIT8)) && kd3_waves(rays) == 4 &&
        !(debug & 512) && n > 0 && (n < kSplitMaxTiles || RT_SPLIT_PCT_LARGE > 0)) {
        const uint64_t pct = n < kSplitMaxTiles ? RT_SPLIT_PCT : RT_SPLIT_PCT_LARGE;
        while (split < n / RT_SPLIT_CAP_DIV && 100ull * cost_of(ord[(size_t)split]) > pct * top && top >= 24)
            split++;
    }
    return split;
}

// A moving object's screen rectangle changes every frame, so its fine grid
// did too: every frame got a new tile order slot, and the cost order (tile
// order 3) never applied (its samples were always of a stale grid).  Renders
// of a transformed object (an identity transform keeps its exact region:
// nothing moves, and the margin would turn fused far groups into fine tiles)
// keep the fine region the camera last chose while the exact one stays
// inside it and covers at least half of it; a new region is chosen with a
// margin of 1/8 of its size (at least 2 tile columns and 1 band slot) on
// every side.  Any region that contains the exact one renders the same frame
// (a fine tile runs the exact root test; the far groups outside it are the
// same proof, set_fine_region).  rt_frame_rect derives the gather rectangle
// without it (every rank alone, no state).  Debug bit 256: off.
struct Hold {
    bool valid = false;
    int32_t key[6] = {0, 0, 0, 0, 0, 0};  // tile_w, tile_h, nranks, rank, groups_x, nslots
    int32_t tx0 = 0, tx1 = -1, s0 = 0, s1 = -1;
};

// The region to render for the exact (non-empty) region (tx0..tx1, s0..s1)
// of a grid of ntx tile columns and nslots band slots: the held one, or a
// new one with its margin, which H then holds.
inline void hold_region(Hold& H, const int32_t key[6], int32_t ntx, int32_t nslots, int32_t& tx0, int32_t& tx1,
                        int32_t& s0, int32_t& s1) {
    const int64_t area = (int64_t)(tx1 - tx0 + 1) * (s1 - s0 + 1);
    const int64_t held = (int64_t)(H.tx1 - H.tx0 + 1) * (H.s1 - H.s0 + 1);
    if (H.valid && std::equal(key, key + 6, H.key) && tx0 >= H.tx0 && tx1 <= H.tx1 && s0 >= H.s0 &&
        s1 <= H.s1 && 2 * area >= held) {
        tx0 = H.tx0; tx1 = H.tx1; s0 = H.s0; s1 = H.s1;
    } else {
        const int32_t mx = std::max(2, (tx1 - tx0 + 1) / 8), ms = std::max(1, (s1 - s0 + 1) / 8);
        tx0 = std::max(0, tx0 - mx); tx1 = std::min(ntx - 1, tx1 + mx);
        s0 = std::max(0, s0 - ms); s1 = std::min(nslots - 1, s1 + ms);
        H.valid = true;
        std::copy(key, key + 6, H.key);
        H.tx0 = tx0; H.tx1 = tx1; H.s0 = s0; H.s1 = s1;
    }
}

}  // namespace rt
