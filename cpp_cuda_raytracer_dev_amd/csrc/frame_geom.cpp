// frame_geom.cpp -- the launch geometry of a frame (frame_geom.h): the kFast
// proofs, the root box's screen rectangles, the fine / coarse split, the rays
// per wave and the gather rectangle.  Host arithmetic only, no HIP.
#include "frame_geom.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

namespace rt {

const float kIdentXf[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

namespace {

// kFast walks of kernel 3 (rt_kernels_impl.h fast_slot, xfast_slot): ordered
// child boxes inside their parents' (k_cam_nodes), and a proof that every
// box's entry parameter maxt0 is at least 2^-20 for every ray of the frame,
// so that the reference's double entry test (TD/Trixel.cu:146) is the float
// mint1 >= maxt0.  The proof: an axis k along which every pixel's
// object-space direction has one sign -- the direction is X3 (n + u x + v y)
// up to a positive factor (TD/Camera.cu:103-104, TD/Trixel.cu:64-66), so its
// component k is affine in the pixel, and its sign is fixed when it has that
// sign at the frame's four corners by a margin of 1e-5 of its terms'
// magnitudes (which covers the float evaluation of the ray and the
// rotation) -- and the root box, shifted by the object offset od (the slab
// test sees b + od, TD/Trixel.cu:94-95), lies beyond the eye on that side by
// a margin.  Every box lies inside the root box, so along axis k each box's
// near bound b has (b + od_k) / |r_k| >= that margin / |r_k|; the float
// t_k = fl(fl(b * fl(1/r_k)) + fl(od_k / r_k)) is within 2^-23 (|b| + |od_k|)
// / |r_k| of it, so a margin of 2^-19 max(1, rmax_k) + 2^-22 (M + |od_k|)
// (M = the root box's largest |bound| on k, rmax_k >= |r_k|) makes t_k, and
// maxt0 >= t_k, at least 2^-19 (1 - 2^-24) >= 2^-20.  Without an offset the
// sum is exact (od / r is a signed zero) and the margin is 2^-19 max(1,
// rmax_k).  The default view (the eye at z = -1 looking +z, the object at
// z > -0.1) proves it along z; a rotation or offset of the object keeps it
// wherever the object stays in front of the eye on some axis (verdict r05
// item 3: the reference's keyboard path).
bool fast_proof(const FrameGeom& g, const TraceParams& p) {
    if ((g.cam_flags & kCamUnordered) || g.root_leaf || !p.leaf_off) return false;
    const float* X = p.xf;
    const double fx = g.w - 1, fy = g.h - 1;
    for (int k = 0; k < 3; k++) {
        double n = 0, u = 0, v = 0, mag = 0, rmax = 0;
        for (int j = 0; j < 3; j++) {
            const double x = X[4 * k + j];
            n += x * g.n_mod[j];
            u += x * g.u_mod[j];
            v += x * g.v_mod[j];
            mag += std::fabs(x) * (std::fabs(g.n_mod[j]) + std::fabs(g.u_mod[j]) * fx + std::fabs(g.v_mod[j]) * fy);
            rmax += std::fabs(x);
        }
        rmax *= 1.0 + 0x1p-20;  // |r_k| <= sum_j |X_kj| |cam_j|, |cam_j| <= 1 + 2^-22
        const double c0 = n, c1 = n + u * fx, c2 = n + v * fy, c3 = n + u * fx + v * fy;
        const double e = 1e-5 * mag;
        const double lo = std::min(std::min(c0, c1), std::min(c2, c3)), hi = std::max(std::max(c0, c1), std::max(c2, c3));
        const double od = X[4 * k + 3];
        const double blo = (double)g.root_box[2 * k] + od, bhi = (double)g.root_box[2 * k + 1] + od;
        const double M = std::max(std::fabs((double)g.root_box[2 * k]), std::fabs((double)g.root_box[2 * k + 1]));
        const double margin = 0x1p-19 * std::max(1.0, rmax) + (od != 0.0 ? 0x1p-22 * (M + std::fabs(od)) : 0.0);
        if (!(std::isfinite(blo) && std::isfinite(bhi))) continue;
        if (lo > e && blo >= margin) return true;
        if (hi < -e && bhi <= -margin) return true;
    }
    return false;
}

// The shadow walks' proof (round 6, verdict r05 item 2): a shadow ray starts
// at the light (2, 2, 2) of TD/Camera.cu:32 (od = (-2, -2, -2)) and points
// at its hit, so if the root box lies below the light's plane on axis k with
// a margin, every shadow ray that points to -k (checked per wave in
// trace_unit, with normal nonzero components) sees every box on axis k at
// t_k = (2 - b) / |r_k| >= the margin (the same rounding bound as
// fast_proof, with od = -2 and |r_k| <= 1 + 2^-22); likewise above it.  Any
// object transform: the shadow walk runs on the records as they are, with the
// light's offset.  Sets sh_axis / sh_neg; false when no axis qualifies (a
// light inside the root box on every axis: tester.ply).
bool fast_proof_shadow(const FrameGeom& g, TraceParams& p) {
    if ((g.cam_flags & kCamUnordered) || g.root_leaf || !p.leaf_off) return false;
    for (int k = 0; k < 3; k++) {
        const double lo = g.root_box[2 * k], hi = g.root_box[2 * k + 1];
        const double M = std::max(std::fabs(lo), std::fabs(hi));
        const double margin = 0x1p-19 * (1.0 + 0x1p-20) + 0x1p-22 * (M + 2.0);
        if (!(std::isfinite(lo) && std::isfinite(hi))) continue;
        if (2.0 - hi >= margin) {
            p.sh_axis = k;
            p.sh_neg = 1;
            return true;
        }
        if (lo - 2.0 >= margin) {
            p.sh_axis = k;
            p.sh_neg = 0;
            return true;
        }
    }
    return false;
}

// The root box's corners shifted by the object offset, in the pixel frame:
// q = A^-1 (c + od) = (a, b, s), the pixel of a point being (a / s, b / s)
// and s its depth along the rays (s > 0 in front of the eye).  False when A
// is singular.
bool root_corners(const FrameGeom& g, const TraceParams& p, double q[8][3]) {
    const float* X = p.xf;
    const float* cols[3] = {g.u_mod, g.v_mod, g.n_mod};
    double A[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            A[i][j] = (double)X[4 * i] * cols[j][0] + (double)X[4 * i + 1] * cols[j][1] + (double)X[4 * i + 2] * cols[j][2];
    const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                       A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    double scale = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) scale = std::max(scale, fabs(A[i][j]));
    if (!(fabs(det) > 1e-12 * scale * scale * scale)) return false;
    double inv[3][3];
    inv[0][0] = (A[1][1] * A[2][2] - A[1][2] * A[2][1]) / det;
    inv[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det;
    inv[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det;
    inv[1][0] = (A[1][2] * A[2][0] - A[1][0] * A[2][2]) / det;
    inv[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det;
    inv[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det;
    inv[2][0] = (A[1][0] * A[2][1] - A[1][1] * A[2][0]) / det;
    inv[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det;
    inv[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det;
    const double od[3] = {X[3], X[7], X[11]};
    for (int k = 0; k < 8; k++) {
        const double cc[3] = {p.root_box[(k & 1) ? 1 : 0] + od[0], p.root_box[(k & 2) ? 3 : 2] + od[1],
                              p.root_box[(k & 4) ? 5 : 4] + od[2]};
        for (int i = 0; i < 3; i++) q[k][i] = inv[i][0] * cc[0] + inv[i][1] * cc[1] + inv[i][2] * cc[2];
    }
    return true;
}

// Screen rectangle (inclusive pixel bounds, row 0 = bottom) that the root
// box projects to, widened by a pixel.  Ray (ix, iy) points along
// X3 * (u_mod*ix + v_mod*iy + n_mod) and the slab test of TD/Trixel.cu:76-95
// sees the box shifted by the object translation od, so each corner c solves
// A (a, b, s) = c with A = X3 [u v n]; pixel = (a/s, b/s).  Returns false when
// the projection is not a bounded rectangle in front of the camera (a corner
// at or behind the eye plane, a singular A): the whole frame is then fine.
// The rectangle is a work-packing hint only -- pixels outside it still run the
// exact root test (coarse groups), so it need not be conservative.
bool root_rect(const FrameGeom& g, const TraceParams& p, double r[4]) {
    double q[8][3];
    if (!root_corners(g, p, q)) return false;
    r[0] = r[2] = INFINITY;
    r[1] = r[3] = -INFINITY;
    for (int k = 0; k < 8; k++) {
        if (!(q[k][2] > 1e-9 * (fabs(q[k][0]) + fabs(q[k][1]) + fabs(q[k][2])))) return false;
        const double x = q[k][0] / q[k][2], y = q[k][1] / q[k][2];
        if (!std::isfinite(x) || !std::isfinite(y)) return false;
        r[0] = std::min(r[0], x); r[1] = std::max(r[1], x);
        r[2] = std::min(r[2], y); r[3] = std::max(r[3], y);
    }
    r[0] = floor(r[0]) - 1; r[1] = ceil(r[1]) + 1;
    r[2] = floor(r[2]) - 1; r[3] = ceil(r[3]) + 1;
    return true;
}

// The screen rectangle of a root box that straddles the eye plane (round 6:
// an object moved to the camera's depth, `--animate`), a work-packing hint
// for the unfused (coarse-group) path only.  The pixels whose rays meet the
// box in front of the eye are the images (a/s, b/s) of the box's part with
// s > 0, a polytope whose vertices are the corners with s > 0 and the edges'
// crossings of s = 0; a/s and b/s are linear-fractional, so their extremes
// over it lie at the corners with s > 0, or are unbounded towards the sign of
// a (b) at a crossing.  Returns 0 when no rectangle helps (singular A, a
// crossing at a = 0 or b = 0); 1 with the (possibly half-unbounded)
// rectangle; 2 when the eye lies inside the box, where every ray's entry
// parameter maxt0 is negative (TD/Trixel.cu:95 fails), or no corner lies in
// front of the eye (a box behind the eye plane that box_behind's margins do
// not cover): the whole frame goes to coarse groups, whose certain-miss and
// root tests are exact.
int root_rect_clipped(const FrameGeom& g, const TraceParams& p, double r[4]) {
    const double od[3] = {p.xf[3], p.xf[7], p.xf[11]};
    bool inside = true;
    for (int k = 0; k < 3; k++) {
        const double lo = (double)p.root_box[2 * k] + od[k], hi = (double)p.root_box[2 * k + 1] + od[k];
        const double m = 1e-6 * std::max(1.0, std::max(fabs(lo), fabs(hi)));
        inside = inside && lo < -m && hi > m;
    }
    if (inside) {
        r[0] = r[2] = 1.0;
        r[1] = r[3] = -1.0;  // empty
        return 2;
    }
    double q[8][3];
    if (!root_corners(g, p, q)) return 0;
    r[0] = r[2] = INFINITY;
    r[1] = r[3] = -INFINITY;
    bool front = false;
    for (int k = 0; k < 8; k++) {
        if (q[k][2] > 0.0) {
            front = true;
            const double x = q[k][0] / q[k][2], y = q[k][1] / q[k][2];
            if (!std::isfinite(x) || !std::isfinite(y)) return 0;
            r[0] = std::min(r[0], x); r[1] = std::max(r[1], x);
            r[2] = std::min(r[2], y); r[3] = std::max(r[3], y);
        }
        for (int bit = 1; bit < 8; bit <<= 1) {  // each edge once, from its corner with the bit clear
            const int n = k | bit;
            if (n == k) continue;
            const double s0 = q[k][2], s1 = q[n][2];
            if (!((s0 > 0.0) != (s1 > 0.0))) continue;
            const double f = s0 / (s0 - s1);
            const double a = q[k][0] + (q[n][0] - q[k][0]) * f, b = q[k][1] + (q[n][1] - q[k][1]) * f;
            if (!(a != 0.0 && b != 0.0) || !std::isfinite(a) || !std::isfinite(b)) return 0;
            if (a > 0.0) r[1] = INFINITY; else r[0] = -INFINITY;
            if (b > 0.0) r[3] = INFINITY; else r[2] = -INFINITY;
        }
    }
    if (!front) {
        r[0] = r[2] = 1.0;
        r[1] = r[3] = -1.0;  // empty
        return 2;
    }
    r[0] = floor(r[0]) - 1; r[1] = ceil(r[1]) + 1;
    r[2] = floor(r[2]) - 1; r[3] = ceil(r[3]) + 1;
    return 1;
}

// Whether the (translated) root box lies behind the eye for every pixel's ray
// (a moving object carried past the camera).  A pixel's
// ray is R = X3 (n_mod + u_mod x + v_mod y), normalised by a positive factor,
// and the slab test of TD/Trixel.cu:76-95 sees the box B + od from the
// origin; if every corner c of B + od has c . R < 0, the whole box lies in
// the half-space x . R < 0, so any t with t R in the box has t |R|^2 < 0: the
// exact entry and exit parameters are negative and the test (maxt0 > -1e-16
// and mint1 >= maxt0 - 1e-16) fails.  An axis the reference drops (0/0 = NaN
// when a component of R is zero) leaves the projections on the other axes,
// for which the same holds since R has no component on the dropped one.
// R over the frame's pixels is a convex combination of the four corner
// pixels' directions (affine in x, y, then linear), so testing the 8 x 4
// corner pairs with a relative margin of 1e-4 (the kernel's rays deviate
// from these by ~1e-6) covers every pixel.
bool box_behind(const FrameGeom& g, const TraceParams& p) {
    const float* X = p.xf;
    double D[4][3];
    for (int k = 0; k < 4; k++) {
        const double fx = (k & 1) ? (double)(g.w - 1) : 0.0, fy = (k & 2) ? (double)(g.h - 1) : 0.0;
        double cam[3];
        for (int j = 0; j < 3; j++) cam[j] = (double)g.n_mod[j] + (double)g.u_mod[j] * fx + (double)g.v_mod[j] * fy;
        for (int i = 0; i < 3; i++)
            D[k][i] = (double)X[4 * i] * cam[0] + (double)X[4 * i + 1] * cam[1] + (double)X[4 * i + 2] * cam[2];
    }
    const double od[3] = {X[3], X[7], X[11]};
    for (int m = 0; m < 8; m++) {
        const double cc[3] = {p.root_box[(m & 1) ? 1 : 0] + od[0], p.root_box[(m & 2) ? 3 : 2] + od[1],
                              p.root_box[(m & 4) ? 5 : 4] + od[2]};
        const double cn = sqrt(cc[0] * cc[0] + cc[1] * cc[1] + cc[2] * cc[2]);
        for (int k = 0; k < 4; k++) {
            const double dn = sqrt(D[k][0] * D[k][0] + D[k][1] * D[k][1] + D[k][2] * D[k][2]);
            const double dot = cc[0] * D[k][0] + cc[1] * D[k][1] + cc[2] * D[k][2];
            if (!(dot < -1e-4 * cn * dn) || !std::isfinite(dot)) return false;
        }
    }
    return true;
}

// What set_fine_region lays the fine region out from (choose_rect).
enum class Region {
    kWholeFrame,  // no rectangle: every tile fine
    kBehind,      // the box behind the eye for every pixel: no fine tiles, every group background
    kProjected,   // the box's projection (root_rect); the groups 2 pixels outside it are far
    kClipped,     // the clipped rectangle of a box at the eye's depth: unfused, no far groups
};

// The rectangle r the fine region is laid out from, and of which kind.
// behind_ok: a box at or behind the eye may be proven so (kernel 3, an
// interior root, no diagnostics).
Region choose_rect(const FrameGeom& c, const TraceParams& p, bool behind_ok, double r[4]) {
    if (root_rect(c, p, r)) return Region::kProjected;
    if (!behind_ok) return Region::kWholeFrame;
    if (box_behind(c, p)) return Region::kBehind;
    // a box at the eye's depth (not wholly behind it): the clipped
    // rectangle on the unfused path, or every group coarse when the eye
    // is inside the box (round 6: such poses of a moving object ran the
    // whole frame as fine units, 73-87 us for an empty frame)
    if (!(c.debug & 8192) && root_rect_clipped(c, p, r) > 0) return Region::kClipped;  // (debug bit 8192: off)
    return Region::kWholeFrame;
}

// The fine region around rectangle r0 (projected, or clipped) and the coarse
// groups outside it.  fused: the far groups go to the fine kernel's extra
// blocks, and the region covers every group that is not far; returns false
// when a tiny-ray group of this rank would then fall outside it (the caller
// lays the region out again unfused, which rewrites every field set here).
bool lay_out_region(const FrameGeom& c, TraceParams& p, int per_wave, const double r0[4], bool clipped, bool fused) {
    const int32_t per_band = kTileH / p.tile_h;
    double r[4] = {r0[0], r0[1], r0[2], r0[3]};
    // r is the projection widened by a pixel; far groups lie 2 more outside
    // (not for a clipped rectangle: its groups outside keep the coarse
    // kernel's certain-miss and exact tests)
    auto clampi = [](double v) { return (int32_t)std::max(-1e9, std::min(1e9, v)); };
    if (!clipped) {
        p.far_rect[0] = clampi(r[0] - 2); p.far_rect[1] = clampi(r[1] + 2);
        p.far_rect[2] = clampi(r[2] - 2); p.far_rect[3] = clampi(r[3] + 2);
    }
    if (fused) {  // fine tiles over everything within the far rectangle
        r[0] -= 2; r[1] += 2; r[2] -= 2; r[3] += 2;
    }
    if (c.debug & 4) r[0] = r[1] = r[2] = r[3] = -8.0;  // tests: every group coarse
    const double x0 = std::max(r[0], 0.0), x1 = std::min(r[1], (double)c.w - 1);
    const double y0 = std::max(r[2], 0.0), y1 = std::min(r[3], (double)c.h - 1);
    int32_t tx0 = 0, tx1 = -1, s0 = 0, s1 = -1;
    if (x0 <= x1 && y0 <= y1) {
        tx0 = (int32_t)x0 / p.tile_w;
        tx1 = (int32_t)x1 / p.tile_w;
        const int32_t b0 = (int32_t)y0 / kTileH, b1 = (int32_t)y1 / kTileH;
        // slots s of this rank with b0 <= rank + s*N <= b1
        s0 = b0 <= p.rank ? 0 : (b0 - p.rank + p.nranks - 1) / p.nranks;
        s1 = b1 < p.rank ? -1 : (b1 - p.rank) / p.nranks;
        s1 = std::min(s1, p.nslots - 1);
    }
    if (tx1 < tx0 || s1 < s0) {  // nothing of the box on this rank: all coarse
        tx0 = 0; tx1 = -1; s0 = 0; s1 = -1;
    } else if (c.hold && !p.plain_xf && !(c.debug & (4 | 256))) {
        const int32_t key[6] = {p.tile_w, p.tile_h, p.nranks, p.rank, p.groups_x, p.nslots};
        hold_region(*c.hold, key, (c.w + p.tile_w - 1) / p.tile_w, p.nslots, tx0, tx1, s0, s1);
    }
    p.fine_tx0 = tx0;
    p.fine_s0 = s0;
    p.tiles_x = tx1 - tx0 + 1;
    p.block_rows = (s1 - s0 + 1) * per_band;
    p.cg_x0 = std::min(tx0 * p.tile_w / 8, p.groups_x);
    p.cg_x1 = std::min((tx1 + 1) * p.tile_w / 8, p.groups_x);
    p.cs0 = s0;
    p.cs1 = s1 + 1;
    if (p.tiles_x <= 0 || p.block_rows <= 0) {
        p.tiles_x = p.block_rows = 0;
        p.cg_x0 = p.cg_x1 = 0;
        p.cs0 = p.cs1 = 0;
    }
    p.coarse_per_wave = per_wave;
    p.coarse_groups = (int64_t)p.nslots * p.groups_x - (int64_t)(p.cs1 - p.cs0) * (p.cg_x1 - p.cg_x0);
    const int64_t waves = (p.coarse_groups + per_wave - 1) / per_wave;
    p.coarse_blocks = (int32_t)((waves + 1) / 2);  // kernel 3 runs two waves per block
    if (fused) {
        for (const auto& g : *c.tiny) {
            const int32_t band = g.second;
            if ((band - p.rank) % p.nranks != 0 || band < p.rank) continue;  // not this rank's band
            const int32_t slot = (band - p.rank) / p.nranks;
            if (g.first < p.cg_x0 || g.first >= p.cg_x1 || slot < p.cs0 || slot >= p.cs1) return false;
        }
        // appended to the fine kernel's grid, kd3_waves(rays) waves per block
        p.fill_blocks = (int32_t)((waves + kd3_waves(p.rays) - 1) / kd3_waves(p.rays));
        p.coarse_blocks = 0;
    }
    return true;
}

// Splits this rank's tiles into the fine region (one kRays unit per wave)
// around the root box's screen rectangle and coarse 8x8 groups elsewhere
// (`per_wave` to a wave; 0 = everything fine).
// fused: the caller wants the far groups filled by the fine kernel's extra
// blocks; the fine region then covers every group that is not far, and
// fusion is refused (returns false, region set as unfused) when a tiny-ray
// group would fall outside it, or the rectangle is a clipped one.
bool set_fine_region(const FrameGeom& c, TraceParams& p, int per_wave, bool fused, bool behind_ok) {
    const int32_t nbands = (c.h + kTileH - 1) / kTileH;
    p.groups_x = (c.w + 7) / 8;
    p.nslots = (nbands + p.nranks - 1) / p.nranks;
    p.fine_tx0 = p.fine_s0 = 0;
    p.cg_x0 = 0; p.cg_x1 = p.groups_x;
    p.cs0 = 0; p.cs1 = p.nslots;
    p.coarse_per_wave = 1;
    p.coarse_groups = 0;
    p.coarse_blocks = 0;
    // no group is "far" unless the projection below succeeds
    p.far_rect[0] = p.far_rect[2] = INT32_MIN / 2;
    p.far_rect[1] = p.far_rect[3] = INT32_MAX / 2;
    p.fill_blocks = 0;
    p.far_all = 0;
    // coarse groups are indexed in 32 bits (k_coarse_kd3)
    if (per_wave <= 0 || (int64_t)p.nslots * p.groups_x >= ((int64_t)1 << 31)) return false;
    double r[4];
    switch (choose_rect(c, p, behind_ok, r)) {
    case Region::kWholeFrame:
        return false;
    case Region::kBehind: {
        // no fine tiles, every group background (far_all), filled by the
        // fine kernel's blocks under any transform
        p.tiles_x = p.block_rows = 0;
        p.cg_x0 = p.cg_x1 = 0;
        p.cs0 = p.cs1 = 0;
        p.coarse_per_wave = per_wave;
        p.coarse_groups = (int64_t)p.nslots * p.groups_x;
        const int64_t waves = (p.coarse_groups + per_wave - 1) / per_wave;
        p.fill_blocks = (int32_t)((waves + kd3_waves(p.rays) - 1) / kd3_waves(p.rays));
        p.far_all = 1;
        return true;
    }
    case Region::kClipped:
        lay_out_region(c, p, per_wave, r, true, false);
        return false;
    case Region::kProjected:
        break;
    }
    if (fused && lay_out_region(c, p, per_wave, r, false, true)) return true;
    lay_out_region(c, p, per_wave, r, false, false);
    return false;
}

// Kernel 3's pixels per wave when RT_OPT_RAYS is 0 (auto): 16, unless this
// rank's fine region (the root box's screen rectangle) holds too few 16-ray
// units to fill the GPU -- then 8, which doubles the waves and halves the
// heaviest unit's pool chain.  Measured on the dragon stand-in (one GPU):
// 960x540 (3.4k 16-ray units) 67.7 -> 52.7 us with 8 rays, 1920x1080 (13.4k
// units) 88 -> 130 us, one frame at a time.  With two frames in flight
// (tools/project_ranks.py --inflight 2, frame period per rank, 16 vs 8
// rays): 1920x1080 whole 74 vs 139 us, a rank of 2 (6.7k units) 43 vs 70,
// of 4 (3.4k) 42 vs 36, of 8 (1.7k) 41 vs 24; 960x540 whole (3.4k) 35 vs 38,
// a rank of 2 34 vs 22.  The 16-ray floor near 41 us is the heaviest unit's
// chain; 8 rays scale with the work.  Round 3 (split tiles, below, shorten
// the 16-ray chains where few units fill the GPU): 960x540 whole 44.5k FPS
// with 16 rays + split vs 34.9k with 8 (solo 35.4 vs 38.1 us; knot 30.7k vs
// 26.3k); per-rank periods at 1080p, two in flight: a rank of 4 (3.4k units)
// 23.8 us (16 + split) vs 27.9 (8), of 8 (1.7k) 23.6 vs 20.9 (r03g).  So 8
// rays below 2,048 units.
constexpr int64_t kAutoRaysMinUnits = 2048;
// Multi-frame launches (round 4): frames overlap inside one grid, so the
// per-wave work counts for more than the heaviest unit's chain, and fine
// regions of fewer than this many 16-ray units render 32 rays per wave.
// Measured (r04u, r04v, 1,000 frames, one box; 16 -> 32 rays): dragon
// 960x540 (3.4k units) 54.3k -> 65.9k FPS, knot 960x540 36.3k -> 37.3k;
// at 1920x1080 (13.4k units) dragon 16.5k -> 17.7k, fill 1,351 -> 1,396,
// but knot 10.43k -> 9.91k; 64 rays lose everywhere (C3 55.5k, knot
// 960x540 29.5k, knot 1080p 8.1k).
constexpr int64_t kAutoRaysMfMaxUnits = 8192;

int auto_rays(const FrameGeom& c, const TraceParams& p) {
    double r[4];
    if (!root_rect(c, p, r)) return 16;  // no bounded rectangle: the whole frame is fine
    const double x0 = std::max(r[0] - 2, 0.0), x1 = std::min(r[1] + 2, (double)c.w - 1);
    const double y0 = std::max(r[2] - 2, 0.0), y1 = std::min(r[3] + 2, (double)c.h - 1);
    if (x1 < x0 || y1 < y0) return 16;
    const double px = (x1 - x0 + 1) * (y1 - y0 + 1) / p.nranks;
    if (c.multiframe) return px / 16 < (double)kAutoRaysMfMaxUnits ? 32 : 16;
    return px / 16 < (double)kAutoRaysMinUnits ? 8 : 16;
}

}  // namespace

FrameGeom host_geom(const rt_frame_geometry& in, std::vector<std::pair<int32_t, int32_t>>& tiny) {
    FrameGeom g;
    g.w = in.w;
    g.h = in.h;
    g.n_mod = in.n_mod;
    g.u_mod = in.u_mod;
    g.v_mod = in.v_mod;
    memcpy(g.root_box, in.root_box, sizeof g.root_box);
    g.root_leaf = in.root_is_leaf != 0;
    g.kernel = in.kernel;
    g.rays = in.rays;
    g.coarse = in.coarse;
    g.debug = in.debug;
    tiny_groups_of(g.w, g.h, g.n_mod, g.u_mod, g.v_mod, tiny);
    g.tiny = &tiny;
    return g;
}

void tiny_groups_of(int32_t w, int32_t h, const float* n, const float* u, const float* v,
                    std::vector<std::pair<int32_t, int32_t>>& out) {
    out.clear();
    for (int32_t y = 0; y < h; y++) {
        const float fy = (float)(uint32_t)y;
        for (int32_t x = 0; x < w; x++) {
            const float fx = (float)(uint32_t)x;
            const float qx = n[0] + u[0] * fx + v[0] * fy;
            const float qy = n[1] + u[1] * fx + v[1] * fy;
            const float qz = n[2] + u[2] * fx + v[2] * fy;
            if (!(fabsf(qx) > 1e-30f && fabsf(qy) > 1e-30f && fabsf(qz) > 1e-30f)) {
                const std::pair<int32_t, int32_t> g{x / 8, y / kTileH};
                if (out.empty() || out.back() != g) out.push_back(g);
            }
        }
    }
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
}

bool frame_geometry(const FrameGeom& g, const float* xform, const rt_tile* tile, uint32_t mode, TraceParams& p) {
    for (int k = 0; k < 3; k++) {
        p.n_mod[k] = g.n_mod[k];
        p.u_mod[k] = g.u_mod[k];
        p.v_mod[k] = g.v_mod[k];
    }
    memcpy(p.xf, xform ? xform : kIdentXf, sizeof p.xf);
    p.w = g.w;
    p.h = g.h;
    p.nranks = tile ? tile->nranks : 1;
    p.rank = tile ? tile->rank : 0;
    memcpy(p.root_box, g.root_box, sizeof p.root_box);
    const int32_t nbands = (g.h + kTileH - 1) / kTileH;
    const int kernel = mode == RT_MODE_KD ? g.kernel : 0;
    p.rays = kernel == 3 ? (g.rays > 0 ? g.rays : auto_rays(g, p)) : 64;
    if (kernel == 0) {                       // flat: 32x8 tiles, four 8x8 waves
        p.tile_w = kTileWFlat; p.tile_h = kTileH;
    } else if (p.rays == 64) {               // v2: 16x8 tiles, two 8x8 waves
        p.tile_w = kTileWKd; p.tile_h = kTileH;
    } else {                                 // v3, two stacked 8 x (rays/8) waves
        p.tile_w = 8; p.tile_h = kd3_waves(p.rays) * (p.rays / 8);
    }
    p.tiles_x = (g.w + p.tile_w - 1) / p.tile_w;
    p.block_rows = ((nbands + p.nranks - 1) / p.nranks) * (kTileH / p.tile_h);
    p.plain_xf = 1;
    for (int k = 0; k < 12; k++) p.plain_xf &= (p.xf[k] == kIdentXf[k]) ? 1 : 0;
    p.fast = kernel == 3 && !(g.debug & 2048) && fast_proof(g, p) ? 1 : 0;  // debug bit 2048: never
    p.sh_axis = 0;
    p.sh_neg = 0;
    p.fast_sh = kernel == 3 && !(g.debug & 2048) && fast_proof_shadow(g, p) ? 1 : 0;
    p.tiny_s1 = (g.cam_flags & kCamTinyS1) ? 1 : 0;
    // Far groups go to the fine kernel's extra blocks when every coarse group
    // can be far (identity transform, interior root, no diagnostics);
    // otherwise to k_coarse_kd3.
    // A box behind the eye makes every group background under any transform.
    const bool can_fuse = kernel == 3 && !g.root_leaf && !(g.debug & (1 | 4 | 8));
    return set_fine_region(g, p, kernel == 3 ? g.coarse : 0, can_fuse && p.plain_xf, can_fuse);
}

void frame_rect_geom(const FrameGeom& g, bool kd_tree, const float* xform, uint32_t mode, int32_t nranks,
                     int32_t rect[4]) {
    const int32_t nbands = (g.h + kTileH - 1) / kTileH;
    rect[0] = 0; rect[1] = g.w; rect[2] = 0; rect[3] = nbands;  // no proof: the whole frame
    if (mode != RT_MODE_KD || !kd_tree) return;
    int32_t x0 = INT32_MAX, x1 = INT32_MIN, b0 = INT32_MAX, b1 = INT32_MIN;
    for (int32_t r = 0; r < nranks; r++) {
        TraceParams p{};
        const rt_tile t{nranks, r};
        if (!frame_geometry(g, xform, &t, mode, p)) return;  // a rank renders unfused
        if (p.cs1 <= p.cs0 || p.cg_x1 <= p.cg_x0) continue;     // nothing fine on this rank
        x0 = std::min(x0, p.cg_x0 * 8);
        x1 = std::max(x1, std::min(p.cg_x1 * 8, g.w));
        b0 = std::min(b0, r + p.cs0 * nranks);
        b1 = std::max(b1, r + (p.cs1 - 1) * nranks + 1);
    }
    if (x0 >= x1 || b0 >= b1) {
        rect[0] = rect[1] = rect[2] = rect[3] = 0;
    } else {
        rect[0] = x0; rect[1] = x1; rect[2] = b0; rect[3] = std::min(b1, nbands);
    }
}

}  // namespace rt
