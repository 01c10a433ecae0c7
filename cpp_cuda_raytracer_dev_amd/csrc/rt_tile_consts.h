// rt_tile_consts.h -- the constants shared by the kernels (through
// rt_internal.h), the tile-order arithmetic (tile_order_host.h) and the
// launch geometry (frame_geom.cpp).  No HIP include: tests/tile_order_main.cpp
// and tests/frame_geom_main.cpp compile it with a plain C++ compiler.
#pragma once

#include <stdint.h>

namespace rt {

// Per-pixel kernels: a block is a tile_w x 8 pixel tile made of 8x8-pixel
// wave64s (tile_w = 32 for the flat kernel, 16 for the KD kernel, whose LDS
// stack is three words per entry).
constexpr int kTileH = 8;
constexpr int kTileWFlat = 32;
constexpr int kTileWKd = 16;
constexpr int kBlockMax = 256;

// k_cam_nodes' flags of a camera's records
constexpr int32_t kCamTinyS1 = 1, kCamUnordered = 2, kCamSplitFields = 4;

// Waves per block of the wave-cooperative kernel: a block is one fine tile,
// each wave one kRays-pixel unit of it.  16- and 8-ray units may run
// RT_KD3_WAVES per block (2 or 4; the tile's waves share the CU's L1), 32-
// and 64-ray units run 2.  The per-unit cost slots hold up to 4 waves.
#ifndef RT_KD3_WAVES
#define RT_KD3_WAVES 4
#endif
// (constexpr: callable from host and device code alike)
constexpr int kd3_waves(int rays) { return rays <= 16 ? RT_KD3_WAVES : 2; }
// Kernel 3's per-tile cost slots (pool iterations): slots 0-3 the waves of a
// tile, 4-7 the second half's waves of a split tile (zero otherwise), so a
// split tile's cost is the max over both halves, not whichever half wrote
// last (that race reordered the heavy tiles at random between samples).
constexpr int kCostSlots = 8;

}  // namespace rt
