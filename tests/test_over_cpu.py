"""CPU tests of depth-tested renders (rt_render_over): the numpy reference
``composite`` the GPU tests compare with, checked on the committed fixture;
the C ABI's three new functions in the header and the ctypes table; and the
facade's Camera::add_layer.  No GPU calls."""
import os
import re
import subprocess

import numpy as np

from cpp_cuda_raytracer_dev_amd import _lib
from tests.test_aov_cpu import fixture, make_aov

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BG = np.uint32(0x00F08200)
MISS_D = np.float32(400.0)


def composite(layers):
    """The frame of several objects, from their single-object renders.

    layers: (argb u32 [n], hit i64 [n], planes f32 or u32 bits [10, n],
    hit_base) per object in render order.  From the miss state (background,
    hit -1, d = 400, zeros), layer k replaces the running result where
    hit_k >= 0 and d_k < d_running (float compare, strict: a tie keeps what is
    there).  -> (argb u32 [n], hit i64 [n], planes u32 bits [10, n])."""
    n = np.asarray(layers[0][0]).size
    argb = np.full(n, BG, np.uint32)
    hit = np.full(n, -1, np.int64)
    planes = np.zeros((10, n), np.uint32)
    planes[0] = MISS_D.view(np.uint32)
    for a, h, p, base in layers:
        a = np.asarray(a).reshape(n).view(np.uint32)
        h = np.asarray(h).reshape(n)
        p = np.ascontiguousarray(p).reshape(10, n).view(np.uint32)
        with np.errstate(invalid="ignore"):
            win = (h >= 0) & (p[0].view(np.float32) < planes[0].view(np.float32))
        argb[win] = a[win]
        hit[win] = h[win] + base
        planes[:, win] = p[:, win]
    return argb, hit, planes


def hit_classes(hit_a, d_a, hit_b, d_b):
    """Pixel counts (a only, b only, both with b nearer, both with a nearer, ties, neither)."""
    a, b = np.asarray(hit_a).reshape(-1) >= 0, np.asarray(hit_b).reshape(-1) >= 0
    da, db = np.asarray(d_a).reshape(-1).view(np.float32), np.asarray(d_b).reshape(-1).view(np.float32)
    both = a & b
    return (int((a & ~b).sum()), int((b & ~a).sum()), int((both & (db < da)).sum()), int((both & (da < db)).sum()),
            int((both & (da == db)).sum()), int((~a & ~b).sum()))


def fixture_layer(key, hit_base):
    z = fixture()
    return z[key + "_argb"].reshape(-1), z[key + "_hit"].reshape(-1), z[key + "_aov"].reshape(10, -1), hit_base


def test_composite_on_the_fixture():
    G = make_aov()
    kb, kl = G.key_of("dump", 40, 24, 0, False), G.key_of("dump", 40, 24, 0, True)
    base, layer = fixture_layer(kb, 0), fixture_layer(kl, 948)
    assert hit_classes(base[1], base[2][0], layer[1], layer[2][0]) == (3, 6, 34, 5, 0, 912)
    argb, hit, planes = composite([base, layer])
    bp, lp = base[2].view(np.uint32), layer[2].view(np.uint32)
    a, b = base[1] >= 0, layer[1] >= 0
    lwin = b & (~a | (lp[0].view(np.float32) < bp[0].view(np.float32)))
    bwin = a & ~lwin
    assert lwin.sum() == 6 + 34 and bwin.sum() == 3 + 5
    assert (hit[lwin] == layer[1][lwin] + 948).all() and (hit[bwin] == base[1][bwin]).all()
    assert (hit[~a & ~b] == -1).all() and (argb[~a & ~b] == BG).all()
    assert (argb[lwin] == layer[0][lwin]).all() and (argb[bwin] == base[0][bwin]).all()
    assert (planes[:, lwin] == lp[:, lwin]).all() and (planes[:, bwin] == bp[:, bwin]).all()
    assert (planes[0][~a & ~b] == MISS_D.view(np.uint32)).all() and (planes[1:][:, ~a & ~b] == 0).all()
    # no ties: the other order gives the same picture (the hit bases travel with the objects)
    argb2, hit2, planes2 = composite([layer, base])
    assert (argb2 == argb).all() and (planes2 == planes).all() and (hit2 == hit).all()
    # a tie keeps what is there, whichever came first
    t_first, _, _ = composite([base, (layer[0], base[1], base[2], 948)])
    assert (t_first == composite([base])[0]).all()


def test_abi_declares_the_three_functions():
    with open(os.path.join(ROOT, "include", "rt_mi355x.h")) as fp:
        header = fp.read()
    want = {
        "rt_render_over": r"int rt_render_over\(rt_camera\* c, const float\* xform, uint32_t mode, uint32_t flags, "
                          r"const rt_tile\* tile,\s+uint32_t\* d_argb, int64_t\* d_hit, int64_t hit_base, void\* stream\);",
        "rt_render_clear": r"int rt_render_clear\(rt_camera\* c, uint32_t flags, const rt_tile\* tile, uint32_t\* d_argb, "
                           r"int64_t\* d_hit,\s+void\* stream\);",
        "rt_camera_targets": r"int rt_camera_targets\(rt_camera\* c, uint32_t\*\* d_argb, int64_t\*\* d_hit, "
                             r"float\*\* d_aov, int64_t\* plane_stride\);",
    }
    nargs = {"rt_render_over": 9, "rt_render_clear": 6, "rt_camera_targets": 5}
    for name, pat in want.items():
        assert re.search(pat, header), name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == nargs[name], name
    assert _lib.SIGNATURES["rt_render_over"][1][7] is _lib.C.c_int64  # hit_base
    # no new flag and no new ABI version: the entry points are the interface
    assert "#define RT_ABI_VERSION 2" in header and _lib.RT_FLAG_WRITE_AOV == 16
    assert not re.search(r"#define RT_FLAG_\w+ (32|64)u", header)
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.C.CDLL(_lib.LIB_PATH)
        for name in want:
            assert hasattr(L, name), name


FACADE_USER = r"""
#include <cstdio>
#include "rt_facade.hpp"
using namespace rtmi;
int frame(Camera* cam, Object* obj1, Object* obj2) {
    // the reference's loop with its second render restored (TD/WinMain.cpp:212-215)
    int rc = obj1->render(cam);
    if (!rc) rc = obj2->render(cam);
    return rc ? rc : cam->color_pixels(PHONG_COLOR_TAG);
}
int main(int argc, char**) {
    Camera cam(16, 8, film_w(16, 8), .024f, .055f, 0, .1f, -1, 0, .1f, 0, 0, 1, 0);
    Object* obj1 = nullptr;
    Object* obj2 = nullptr;
    if (argc > 100) {  // never: compiled and linked, not run
        cam.add_object(obj1);
        cam.add_layer(obj2);
        std::printf("%d %lld %f\n", frame(&cam, obj1, obj2), (long long)obj2->hit_base, cam.h_mem.d_dist.d[0]);
    }
    return 0;
}
"""


def test_facade_add_layer_compiles(tmp_path):
    """Camera::add_layer, Object::hit_base and a layer's Object::render compile
    warning-free against the header and link against the library."""
    src = tmp_path / "over_user.cpp"
    src.write_text(FACADE_USER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o",
                    str(tmp_path / "over_user"), str(src), _lib.LIB_PATH], check=True)
