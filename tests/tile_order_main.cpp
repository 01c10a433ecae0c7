// tile_order_main.cpp -- the tile-order arithmetic (csrc/tile_order_host.h) on
// the CPU, built with the address and undefined-behaviour sanitizers by
// tests/test_tile_order_cpu.py.  Each case arrives as arguments
//     case kind=order|hold name=... key=value ... hash=<hex>
// (tests/golden/tile_order.json); the program checks the invariants of every
// output and that an FNV-1a hash of the outputs equals the recorded one.
// --record as the first argument prints the hashes instead of comparing.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>

#include "../cpp_cuda_raytracer_dev_amd/csrc/tile_order_host.h"

using namespace rt;

namespace {

int g_fail = 0;
std::string g_case;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (g_fail++ < 20) {                           \
                fprintf(stderr, "%s: ", g_case.c_str());   \
                fprintf(stderr, __VA_ARGS__);              \
                fprintf(stderr, " [%s]\n", #cond);         \
            }                                              \
        }                                                  \
    } while (0)

struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void u32(uint32_t v) {
        for (int k = 0; k < 4; k++) {
            h ^= (v >> (8 * k)) & 0xFFu;
            h *= 0x100000001b3ull;
        }
    }
    void i32(int32_t v) { u32((uint32_t)v); }
    void i64(int64_t v) {
        u32((uint32_t)((uint64_t)v & 0xFFFFFFFFull));
        u32((uint32_t)((uint64_t)v >> 32));
    }
    template <class T>
    void vec(const std::vector<T>& v) {
        i64((int64_t)v.size());
        for (T x : v) u32((uint32_t)x);
    }
};

// the same values on every platform (no <random> distribution)
struct Lcg {
    uint64_t s;
    explicit Lcg(uint64_t seed) : s(seed * 2862933555777941757ull + 3037000493ull) {}
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
};

typedef std::map<std::string, std::string> Args;

int64_t num(const Args& a, const char* k) {
    auto it = a.find(k);
    if (it == a.end()) {
        fprintf(stderr, "%s: missing %s\n", g_case.c_str(), k);
        exit(2);
    }
    return strtoll(it->second.c_str(), nullptr, 10);
}

std::string str(const Args& a, const char* k) {
    auto it = a.find(k);
    return it == a.end() ? std::string() : it->second;
}

bool is_permutation(const std::vector<int32_t>& v, int64_t n) {
    if ((int64_t)v.size() != n) return false;
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int32_t t : v) {
        if (t < 0 || t >= n || seen[(size_t)t]) return false;
        seen[(size_t)t] = 1;
    }
    return true;
}

uint32_t tile_max(const std::vector<uint32_t>& c, int64_t t) {
    uint32_t m = 0;
    for (int k = 0; k < kCostSlots; k++) m = std::max(m, c[kCostSlots * (size_t)t + k]);
    return m;
}

// The run (XCD) of every tile as the order's comment defines it, derived
// here independently: mode 2 cuts the row-major tiles into 8 runs of equal
// count, mode 1 the Morton-ordered tiles into 8 runs of equal 1 + cost.
std::vector<int> runs_of(const TileGrid& g, int mode, const std::vector<uint32_t>& cost, int64_t size[8]) {
    const int64_t n = g.tiles();
    std::vector<int> run((size_t)n, 7);
    for (int r = 0; r < 8; r++) size[r] = 0;
    if (mode == 2) {
        for (int64_t t = 0; t < n; t++)
            for (int r = 0; r < 8; r++)
                if (t >= n * r / 8 && t < n * (r + 1) / 8) run[(size_t)t] = r;
    } else {
        std::vector<std::pair<uint64_t, int32_t>> mk;
        for (int64_t t = 0; t < n; t++) {
            const uint64_t x = (uint64_t)(t % g.tiles_x) * g.tile_w, y = (uint64_t)(t / g.tiles_x) * g.tile_h;
            uint64_t key = 0;
            for (int b = 0; b < 32; b++) key |= ((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1);
            mk.push_back({key, (int32_t)t});
        }
        std::sort(mk.begin(), mk.end());
        auto sum = [&](int64_t t) {
            double m = 0;
            for (int k = 0; k < kCostSlots; k++) m += cost[kCostSlots * (size_t)t + k];
            return m;
        };
        double total = 0.0, acc = 0.0;
        for (int64_t t = 0; t < n; t++) total += 1.0 + sum(t);
        int r = 0;  // the run the next tile falls in: the cuts passed so far
        for (int64_t k = 0; k < n; k++) {
            run[(size_t)mk[(size_t)k].second] = r;
            acc += 1.0 + sum(mk[(size_t)k].second);
            while (r < 7 && acc >= total * (r + 1) / 8) r++;
        }
    }
    for (int64_t t = 0; t < n; t++) size[run[(size_t)t]]++;
    return run;
}

uint64_t run_order_case(const Args& a) {
    TileGrid g;
    g.w = (int32_t)num(a, "w"); g.h = (int32_t)num(a, "h");
    g.tile_w = (int32_t)num(a, "tile_w"); g.tile_h = (int32_t)num(a, "tile_h");
    g.tiles_x = (int32_t)num(a, "tiles_x"); g.block_rows = (int32_t)num(a, "block_rows");
    g.nranks = (int32_t)num(a, "nranks"); g.rank = (int32_t)num(a, "rank");
    g.fine_tx0 = (int32_t)num(a, "tx0"); g.fine_s0 = (int32_t)num(a, "s0");
    g.nslots = (int32_t)num(a, "nslots"); g.rays = (int32_t)num(a, "rays");
    const int64_t n = g.tiles();
    const std::string kind = str(a, "cost");
    Lcg rng((uint64_t)num(a, "seed"));
    Fnv f;

    int64_t key[kOrderKey];
    g.key(key);
    for (int64_t k : key) f.i64(k);
    f.i64(all_tiles(g, 0));
    f.i64(all_tiles(g, 64));
    CHECK(all_tiles(g, 0) >= n, "all_tiles %lld below the grid's %lld", (long long)all_tiles(g, 0), (long long)n);

    const std::vector<int32_t> centre = centre_order(g);
    CHECK(is_permutation(centre, n), "centre order is no permutation");
    f.vec(centre);

    // the sample: four waves' costs per tile, the second half's slots zero
    std::vector<uint32_t> eff(kCostSlots * (size_t)n, 0u);
    for (int64_t t = 0; t < n; t++)
        for (int k = 0; k < 4; k++) {
            const uint32_t r = rng.next();
            eff[kCostSlots * (size_t)t + k] = kind == "zero" ? 0u : kind == "equal" ? 40u : r % 200u;
        }
    if (kind == "clamp") {  // above the counting sort's 2^16 clamp, twice (a tie at the clamp)
        eff[kCostSlots * (size_t)(n / 2) + 1] = 70000u;
        eff[kCostSlots * (size_t)(n / 3) + 2] = 66000u;
    }
    // a sample of a frame with split tiles: some with a remembered cost, some without
    std::vector<uint8_t> flags;
    std::vector<uint32_t> mem((size_t)n, 0u);
    if (num(a, "flags")) {
        flags.assign((size_t)n, 0);
        for (int64_t t = 0; t < n; t++) {
            flags[(size_t)t] = (rng.next() >> 7) & 1;
            mem[(size_t)t] = t % 3 == 0 ? 0u : 30u + (uint32_t)(t % 50);
        }
    }
    const std::vector<uint32_t> sample = eff, mem0 = mem;
    effective_costs(eff, flags, mem);
    for (int64_t t = 0; t < n; t++) {
        const bool fl = !flags.empty() && flags[(size_t)t];
        if (fl && mem0[(size_t)t] > 0)
            CHECK(tile_max(eff, t) == mem0[(size_t)t] && mem[(size_t)t] == mem0[(size_t)t], "tile %lld: remembered cost not used", (long long)t);
        else
            CHECK(tile_max(eff, t) == tile_max(sample, t), "tile %lld: sampled cost changed", (long long)t);
        if (!fl) CHECK(mem[(size_t)t] == tile_max(sample, t), "tile %lld: unsplit cost not remembered", (long long)t);
    }
    f.vec(eff);
    f.vec(mem);

    uint32_t mx = 0;
    for (int64_t t = 0; t < n; t++) mx = std::max(mx, tile_max(eff, t));
    mx = std::min<uint32_t>(mx, 1u << 16);
    auto clamped = [&](int64_t t) { return std::min(tile_max(eff, t), mx); };
    std::vector<int64_t> centre_pos((size_t)n);
    for (int64_t k = 0; k < n; k++) centre_pos[(size_t)centre[(size_t)k]] = k;

    std::vector<int32_t> ord0;
    for (int mode = 0; mode < 3; mode++) {
        const std::vector<int32_t> ord = cost_order(g, centre.data(), mode, eff.data());
        CHECK(is_permutation(ord, n), "mode %d: no permutation", mode);
        f.vec(ord);
        if (!is_permutation(ord, n)) continue;
        if (mode == 0) {
            ord0 = ord;
            for (int64_t k = 1; k < n; k++) {
                const int32_t p = ord[(size_t)k - 1], q = ord[(size_t)k];
                CHECK(clamped(p) >= clamped(q), "mode 0: cost rises at %lld", (long long)k);
                if (clamped(p) == clamped(q))
                    CHECK(centre_pos[(size_t)p] < centre_pos[(size_t)q], "mode 0: not stable at %lld", (long long)k);
            }
            continue;
        }
        int64_t size[8], taken[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const std::vector<int> run = runs_of(g, mode, eff, size);
        for (int64_t b = 0; b < n; b++) {
            const int x = (int)(b % 8), r = run[(size_t)ord[(size_t)b]];
            if (taken[x] < size[x]) CHECK(r == x, "mode %d: block %lld from run %d", mode, (long long)b, r);
            taken[r]++;
        }
    }

    if (n > 0 && (int64_t)ord0.size() == n) {
        const uint32_t top = tile_max(eff, ord0[0]);
        const int32_t split = split_count(n, ord0.data(), eff.data(), 3, g.rays, 0);
        CHECK(split >= 0 && split <= n / RT_SPLIT_CAP_DIV, "split %d of %lld tiles", split, (long long)n);
        if (top < 24 || g.rays == 32) CHECK(split == 0, "split %d with top %u, rays %d", split, top, g.rays);
        CHECK(split_count(n, ord0.data(), eff.data(), 3, g.rays, 512) == 0, "split with debug bit 512");
        CHECK(split_count(n, ord0.data(), eff.data(), 4, g.rays, 0) == 0, "split in tile order 4");
        f.i32(split);
    }
    return f.h;
}

uint64_t run_hold_case(const Args& a) {
    const int32_t ntx = (int32_t)num(a, "ntx"), nslots = (int32_t)num(a, "nslots");
    const std::string steps = str(a, "steps");  // "keyvariant,tx0,tx1,s0,s1;..."
    Hold H;
    Fnv f;
    const char* s = steps.c_str();
    int nstep = 0;
    while (*s) {
        int v[5], used = 0;
        if (sscanf(s, "%d,%d,%d,%d,%d%n", &v[0], &v[1], &v[2], &v[3], &v[4], &used) != 5) {
            fprintf(stderr, "%s: bad steps\n", g_case.c_str());
            exit(2);
        }
        s += used;
        if (*s == ';') s++;
        const int32_t key[6] = {8, 8 >> v[0], 1, 0, ntx, nslots};
        int32_t tx0 = v[1], tx1 = v[2], s0 = v[3], s1 = v[4];
        hold_region(H, key, ntx, nslots, tx0, tx1, s0, s1);
        CHECK(tx0 <= v[1] && tx1 >= v[2] && s0 <= v[3] && s1 >= v[4], "step %d: region misses the exact one", nstep);
        CHECK(tx0 >= 0 && tx1 < ntx && s0 >= 0 && s1 < nslots, "step %d: region outside the grid", nstep);
        CHECK(H.valid && H.tx0 == tx0 && H.tx1 == tx1 && H.s0 == s0 && H.s1 == s1 && std::equal(key, key + 6, H.key),
              "step %d: the hold is not the region rendered", nstep);
        for (int32_t x : {tx0, tx1, s0, s1}) f.i32(x);
        nstep++;
    }
    f.i32(nstep);
    return f.h;
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
        if (kind != "order" && kind != "hold") {
            fprintf(stderr, "%s: unknown kind '%s'\n", g_case.c_str(), kind.c_str());
            return 2;
        }
        const uint64_t h = kind == "order" ? run_order_case(a) : run_hold_case(a);
        char hex[32];
        snprintf(hex, sizeof hex, "%016llx", (unsigned long long)h);
        if (record) printf("%s %s\n", g_case.c_str(), hex);
        else CHECK(str(a, "hash") == hex, "hash %s, recorded %s", hex, str(a, "hash").c_str());
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
