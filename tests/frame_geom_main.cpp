// frame_geom_main.cpp -- the launch geometry (csrc/frame_geom.cpp) on the CPU,
// built with the address and undefined-behaviour sanitizers by
// tests/test_frame_geom_cpu.py.  Each case arrives as arguments
//     case kind=geom|rect name=... key=value ... exp_<field>=value
// (tests/golden/frame_geom.json; floats as their 32-bit patterns); the program
// checks the invariants of every output and that every field equals the
// recorded one.  --record as the first argument prints the fields instead of
// comparing.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>

#include "../cpp_cuda_raytracer_dev_amd/csrc/frame_geom.h"

using namespace rt;

namespace {

int g_fail = 0;
std::string g_case;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (g_fail++ < 40) {                           \
                fprintf(stderr, "%s: ", g_case.c_str());   \
                fprintf(stderr, __VA_ARGS__);              \
                fprintf(stderr, " [%s]\n", #cond);         \
            }                                              \
        }                                                  \
    } while (0)

typedef std::map<std::string, std::string> Args;
typedef std::vector<std::pair<int32_t, int32_t>> Groups;

const std::string& str(const Args& a, const char* k) {
    auto it = a.find(k);
    if (it == a.end()) {
        fprintf(stderr, "%s: missing %s\n", g_case.c_str(), k);
        exit(2);
    }
    return it->second;
}

int64_t num(const Args& a, const char* k) { return strtoll(str(a, k).c_str(), nullptr, 10); }

// "a,b,c": n integers
std::vector<int64_t> list(const Args& a, const char* k, size_t n) {
    std::vector<int64_t> v;
    const char* s = str(a, k).c_str();
    while (*s) {
        char* end;
        v.push_back(strtoll(s, &end, 10));
        if (end == s) {
            v.clear();
            break;
        }
        s = *end == ',' ? end + 1 : end;
    }
    if (v.size() != n) {
        fprintf(stderr, "%s: %s holds %zu values, not %zu\n", g_case.c_str(), k, v.size(), n);
        exit(2);
    }
    return v;
}

// floats as their bit patterns
void floats(const Args& a, const char* k, float* out, size_t n) {
    const std::vector<int64_t> v = list(a, k, n);
    for (size_t i = 0; i < n; i++) {
        const uint32_t u = (uint32_t)v[i];
        memcpy(out + i, &u, 4);
    }
}

// A case's inputs: rt_frame_geometry's fields, the transform and the ranks.
struct Inputs {
    rt_frame_geometry in;
    float xf[12];
    bool have_xf;
    uint32_t mode;
    int32_t nranks;
};

Inputs inputs_of(const Args& a) {
    Inputs c;
    memset(&c, 0, sizeof c);
    c.in.w = (int32_t)num(a, "w");
    c.in.h = (int32_t)num(a, "h");
    float basis[9];
    floats(a, "basis", basis, 9);
    for (int k = 0; k < 3; k++) {
        c.in.n_mod[k] = basis[k];
        c.in.u_mod[k] = basis[3 + k];
        c.in.v_mod[k] = basis[6 + k];
    }
    floats(a, "box", c.in.root_box, 6);
    c.in.root_is_leaf = (int32_t)num(a, "root_leaf");
    c.in.kernel = (int32_t)num(a, "kernel");
    c.in.rays = (int32_t)num(a, "rays");
    c.in.coarse = (int32_t)num(a, "coarse");
    c.in.debug = (int32_t)num(a, "debug");
    c.have_xf = str(a, "xf") != "none";
    if (c.have_xf) floats(a, "xf", c.xf, 12);
    c.mode = (uint32_t)num(a, "mode");
    c.nranks = (int32_t)num(a, "nranks");
    return c;
}

// Whether pixel (x, y)'s ray X3 (n + u x + v y) from the origin meets the
// root box shifted by the object offset at some t >= 0 (slabs, in double; a
// zero component meets its slab when the slab holds the origin).
bool pixel_hits_box(const Inputs& c, int32_t x, int32_t y) {
    const float* X = c.have_xf ? c.xf : kIdentXf;
    double cam[3], tin = -INFINITY, tout = INFINITY;
    for (int j = 0; j < 3; j++) cam[j] = (double)c.in.n_mod[j] + (double)c.in.u_mod[j] * x + (double)c.in.v_mod[j] * y;
    for (int k = 0; k < 3; k++) {
        const double d = (double)X[4 * k] * cam[0] + (double)X[4 * k + 1] * cam[1] + (double)X[4 * k + 2] * cam[2];
        const double lo = (double)c.in.root_box[2 * k] + (double)X[4 * k + 3];
        const double hi = (double)c.in.root_box[2 * k + 1] + (double)X[4 * k + 3];
        if (d == 0.0) {
            if (!(lo <= 0.0 && 0.0 <= hi)) return false;
            continue;
        }
        const double t0 = lo / d, t1 = hi / d;
        tin = std::max(tin, std::min(t0, t1));
        tout = std::min(tout, std::max(t0, t1));
    }
    return tout >= tin && tout >= 0.0;
}

typedef std::vector<std::pair<std::string, int64_t>> Fields;

Hold g_hold;  // carried from case to case (hold=carry), renewed by hold=new

void run_geom_case(const Args& a, Fields& out) {
    const Inputs c = inputs_of(a);
    Groups tiny;
    FrameGeom g = host_geom(c.in, tiny);
    g.multiframe = num(a, "multiframe") != 0;
    g.cam_flags = (int32_t)num(a, "cam_flags");
    const std::string& hold = str(a, "hold");
    if (hold == "new") g_hold = Hold();
    if (hold != "none") g.hold = &g_hold;
    const rt_tile tile{c.nranks, (int32_t)num(a, "rank")};
    TraceParams p{};
    p.leaf_off = (uint32_t)num(a, "leaf_off");
    const bool fused = frame_geometry(g, c.have_xf ? c.xf : nullptr, &tile, c.mode, p);

    out = {{"tile_w", p.tile_w}, {"tile_h", p.tile_h}, {"rays", p.rays}, {"tiles_x", p.tiles_x},
           {"block_rows", p.block_rows}, {"fine_tx0", p.fine_tx0}, {"fine_s0", p.fine_s0}, {"groups_x", p.groups_x},
           {"nslots", p.nslots}, {"cg_x0", p.cg_x0}, {"cg_x1", p.cg_x1}, {"cs0", p.cs0}, {"cs1", p.cs1},
           {"coarse_per_wave", p.coarse_per_wave}, {"coarse_groups", p.coarse_groups},
           {"coarse_blocks", p.coarse_blocks}, {"fill_blocks", p.fill_blocks}, {"far_rect0", p.far_rect[0]},
           {"far_rect1", p.far_rect[1]}, {"far_rect2", p.far_rect[2]}, {"far_rect3", p.far_rect[3]},
           {"far_all", p.far_all}, {"plain_xf", p.plain_xf}, {"fast", p.fast}, {"fast_sh", p.fast_sh},
           {"sh_axis", p.sh_axis}, {"sh_neg", p.sh_neg}, {"tiny_s1", p.tiny_s1}, {"ret", fused ? 1 : 0},
           {"ntiny", (int64_t)tiny.size()}};

    // the fine region lies inside this rank's grid
    CHECK(p.tile_w > 0 && p.tile_h > 0 && kTileH % p.tile_h == 0, "tile %d x %d", p.tile_w, p.tile_h);
    if (p.tile_w <= 0 || p.tile_h <= 0) return;
    CHECK(p.fine_tx0 >= 0 && p.tiles_x >= 0 && p.fine_tx0 + p.tiles_x <= (c.in.w + p.tile_w - 1) / p.tile_w,
          "fine columns %d + %d", p.fine_tx0, p.tiles_x);
    CHECK(0 <= p.cs0 && p.cs0 <= p.cs1 && p.cs1 <= p.nslots, "slots [%d, %d) of %d", p.cs0, p.cs1, p.nslots);
    CHECK(0 <= p.cg_x0 && p.cg_x0 <= p.cg_x1 && p.cg_x1 <= p.groups_x, "groups [%d, %d) of %d", p.cg_x0, p.cg_x1,
          p.groups_x);
    CHECK(p.block_rows == (p.cs1 - p.cs0) * kTileH / p.tile_h, "block_rows %d", p.block_rows);
    CHECK(p.coarse_groups == (int64_t)p.nslots * p.groups_x - (int64_t)(p.cs1 - p.cs0) * (p.cg_x1 - p.cg_x0) &&
              p.coarse_groups >= 0,
          "coarse_groups %lld", (long long)p.coarse_groups);
    // the launched waves cover the groups
    if (!fused) {
        CHECK(2 * (int64_t)p.coarse_blocks * p.coarse_per_wave >= p.coarse_groups, "%d coarse blocks of %d for %lld groups",
              p.coarse_blocks, p.coarse_per_wave, (long long)p.coarse_groups);
        return;
    }
    CHECK((int64_t)p.fill_blocks * kd3_waves(p.rays) * p.coarse_per_wave >= p.coarse_groups && p.coarse_blocks == 0,
          "%d fill blocks (%d coarse) of %d for %lld groups", p.fill_blocks, p.coarse_blocks, p.coarse_per_wave,
          (long long)p.coarse_groups);
    // every tiny-ray group of this rank lies inside the region (far_all has
    // no region: box_behind's proof holds for rays with zero components too)
    for (const auto& t : tiny) {
        if (p.far_all || t.second < tile.rank || (t.second - tile.rank) % tile.nranks) continue;
        const int32_t slot = (t.second - tile.rank) / tile.nranks;
        CHECK(t.first >= p.cg_x0 && t.first < p.cg_x1 && slot >= p.cs0 && slot < p.cs1,
              "tiny group (%d, %d) outside the fused region", t.first, t.second);
    }
    // no pixel outside the far rectangle (none at all with far_all) meets the box
    for (int32_t y = 0; y < c.in.h; y++)
        for (int32_t x = 0; x < c.in.w; x++) {
            const bool inside = !p.far_all && x >= p.far_rect[0] && x <= p.far_rect[1] && y >= p.far_rect[2] &&
                                y <= p.far_rect[3];
            if (!inside) CHECK(!pixel_hits_box(c, x, y), "far pixel (%d, %d) meets the root box", x, y);
        }
}

void run_rect_case(const Args& a, Fields& out) {
    const Inputs c = inputs_of(a);
    const float* xf = c.have_xf ? c.xf : nullptr;
    Groups tiny;
    const FrameGeom g = host_geom(c.in, tiny);
    int32_t rect[4] = {-1, -1, -1, -1};
    frame_rect_geom(g, true, xf, c.mode, c.nranks, rect);
    out = {{"rect0", rect[0]}, {"rect1", rect[1]}, {"rect2", rect[2]}, {"rect3", rect[3]}};
    const int32_t nbands = (c.in.h + kTileH - 1) / kTileH;
    CHECK(0 <= rect[0] && rect[0] <= rect[1] && rect[1] <= c.in.w && 0 <= rect[2] && rect[2] <= rect[3] &&
              rect[3] <= nbands,
          "rect (%d, %d, %d, %d) outside the frame", rect[0], rect[1], rect[2], rect[3]);
    if (c.nranks != 1) return;
    // one rank: the rectangle contains the fine region
    TraceParams p{};
    (void)frame_geometry(g, xf, nullptr, c.mode, p);
    if (p.cs1 > p.cs0 && p.cg_x1 > p.cg_x0)
        CHECK(rect[0] <= p.cg_x0 * 8 && std::min(p.cg_x1 * 8, c.in.w) <= rect[1] && rect[2] <= p.cs0 && p.cs1 <= rect[3],
              "rect (%d, %d, %d, %d) misses the fine region", rect[0], rect[1], rect[2], rect[3]);
}

}  // namespace

int main(int argc, char** argv) {
    int i = 1;
    const bool record = argc > 1 && !strcmp(argv[1], "--record");
    if (record) i++;
    int ncase = 0;
    while (i < argc) {
        if (strcmp(argv[i], "case")) {
            fprintf(stderr, "expected 'case', got '%s'\n", argv[i]);
            return 2;
        }
        Args a;
        for (i++; i < argc && strcmp(argv[i], "case"); i++) {
            const char* eq = strchr(argv[i], '=');
            if (!eq) {
                fprintf(stderr, "expected key=value, got '%s'\n", argv[i]);
                return 2;
            }
            a[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
        }
        g_case = str(a, "name");
        const std::string kind = str(a, "kind");
        if (kind != "geom" && kind != "rect") {
            fprintf(stderr, "%s: unknown kind '%s'\n", g_case.c_str(), kind.c_str());
            return 2;
        }
        Fields out;
        if (kind == "geom") run_geom_case(a, out);
        else run_rect_case(a, out);
        if (record) printf("%s", g_case.c_str());
        for (const auto& f : out) {
            if (record) printf(" %s=%lld", f.first.c_str(), (long long)f.second);
            else CHECK(num(a, ("exp_" + f.first).c_str()) == f.second, "%s = %lld, recorded %s", f.first.c_str(),
                       (long long)f.second, str(a, ("exp_" + f.first).c_str()).c_str());
        }
        if (record) printf("\n");
        ncase++;
    }
    if (!ncase) {
        fprintf(stderr, "no cases\n");
        return 2;
    }
    if (g_fail) fprintf(stderr, "%d check(s) failed in %d cases\n", g_fail, ncase);
    else if (!record) printf("%d cases ok\n", ncase);
    return g_fail ? 1 : 0;
}
