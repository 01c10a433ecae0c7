/*
 * oracle/ref_asan_main.cpp -- runs render cases through the reference under a
 * host AddressSanitizer.  TEST INFRASTRUCTURE ONLY.
 *
 * oracle/ref_build.py links this main with the same sources as libref.so,
 * all compiled with -fsanitize=address, into oracle/_ref/ref_asan.  Each
 * argument is a case file written by oracle/_ref.py write_case(): a scene and
 * a transform.  Every case renders two KD frames and two flat frames (KD only
 * with more than one triangle: the reference's per-pixel index queue of a
 * one-triangle mesh has length ceil(log2(1)) = 0).  A clean exit says that
 * on these cases the reference stays inside its own buffers, so that what
 * the tests pin on them is defined behaviour.  Leak checking is left off by
 * the caller: the reference frees little.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct ref_scene;
extern "C" {
ref_scene* ref_scene_create(int32_t w, int32_t h, float f_w, float f_h, float focal, const float pos[3],
                            const float la[3], const float up[3], const float* points9, const float* rad3,
                            uint32_t ntri, const void* leafs, const void* nodes);
void ref_scene_destroy(ref_scene* s);
void ref_scene_set_xform(ref_scene* s, const float x[12]);
void ref_scene_frame(ref_scene* s, int mode, int64_t* hit, float* aov, uint32_t* shown, uint32_t* clean);
}

struct case_header {  // oracle/_ref.py CASE_HEADER
    int32_t w, h;
    float f_w, f_h, focal, pos[3], la[3], up[3];
    uint32_t ntri;
    float xform[12];
};

static bool read_all(FILE* fp, void* dst, size_t bytes) { return fread(dst, 1, bytes, fp) == bytes; }

static int run_case(const char* path) {
    FILE* fp = fopen(path, "rb");
    if (!fp) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    case_header hd;
    if (!read_all(fp, &hd, sizeof hd)) { fclose(fp); return 2; }
    const size_t n = hd.ntri, nnode = 2 * n - 1, npix = (size_t)hd.w * hd.h;
    std::vector<float> pts(9 * n), rad(3 * n);
    std::vector<char> nodes(96 * nnode);
    const bool ok = read_all(fp, pts.data(), 36 * n) && read_all(fp, rad.data(), 12 * n) &&
                    read_all(fp, nodes.data(), nodes.size());
    fclose(fp);
    if (!ok) { fprintf(stderr, "short case file %s\n", path); return 2; }
    std::vector<int64_t> hit(npix);
    std::vector<float> aov(10 * npix);
    std::vector<uint32_t> shown(npix), clean(npix);
    unsigned long long hits = 0;
    for (int mode = n > 1 ? 0 : 1; mode < 2; mode++) {
        ref_scene* s = ref_scene_create(hd.w, hd.h, hd.f_w, hd.f_h, hd.focal, hd.pos, hd.la, hd.up, pts.data(),
                                        rad.data(), hd.ntri, nullptr, nodes.data());
        ref_scene_set_xform(s, hd.xform);
        for (int frame = 0; frame < 2; frame++) {
            ref_scene_frame(s, mode, hit.data(), aov.data(), shown.data(), clean.data());
            for (size_t i = 0; i < npix; i++) hits += hit[i] >= 0;
        }
        ref_scene_destroy(s);
    }
    printf("%s: %u triangles, %dx%d, %llu hit pixels over the frames\n", path, hd.ntri, hd.w, hd.h, hits);
    return 0;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; i++)
        if (int rc = run_case(argv[i])) return rc;
    return 0;
}
