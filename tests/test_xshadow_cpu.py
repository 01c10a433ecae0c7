"""CPU tests of the deferred shadow pass (rt_shadow_over): the numpy reference
``cross_shadow`` the GPU tests compare with, built on oracle/np_oracle.py's
trace_kd / trace_shadow and tests/test_over_cpu.py's composite; the pixel
classes of the cases those tests use; the C ABI's new function in the header
and the ctypes table; and the facade's Camera::shadow_layers.  No GPU calls."""
import functools
import os
import re
import subprocess

import numpy as np

from cpp_cuda_raytracer_dev_amd import _lib
from oracle import np_oracle as N
from tests.test_aov_cpu import make_aov
from tests.test_over_cpu import composite

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NTRI_DUMP = 948
F = np.float32


def offset_xform(x, y, z):
    """The identity rotation with offset (X[3], X[7], X[11]) = (x, y, z)."""
    X = N.IDENT.copy()
    X[3], X[7], X[11] = F(x), F(y), F(z)
    return X


def trace_object(S, cam, X, pixels, rad=None):
    """One object's plain render at the pixel indices `pixels`, from
    np_oracle.trace_kd: (argb u32 [m], hit i64 [m], planes f32 [10, m], rays),
    rays[j] = the object-space ray (r, od) of pixel j (a miss has one too)."""
    m = len(pixels)
    argb = np.full(m, N.BG, np.uint32)
    hit = np.full(m, -1, np.int64)
    planes = np.zeros((10, m), F)
    planes[0] = F(400.0)
    rays = []
    w = cam["w"]
    with np.errstate(all="ignore"):
        for j, i in enumerate(pixels):
            iy, ix = divmod(int(i), w)
            rmd = N.primary_ray(cam, ix, iy)
            rmi, d, out, ray = N.trace_kd(S, X, rmd)
            rays.append(ray)
            if rmi >= 0:
                c = N.RAD if rad is None else rad[rmi]
                hit[j] = rmi
                planes[:, j] = [d, *out[0], *out[1], *c]
                argb[j] = N.phong(out[0], out[1], rmd, c)
    return argb, hit, planes, rays


def cross_shadow(S, cam, xforms, pixels=None, order=None, depth=None, traced=None, cnt=None, own_cnt=None):
    """The composite of one object per transform in `xforms` with every
    object's shadows applied, at the pixel indices `pixels` (all by default).

    S: the prepared scene (np_oracle.prepare) of every object, or a list of
    one per object; object k's hit base is the triangle count of the objects
    before it.  From the composite (tests.test_over_cpu.composite of the
    objects' plain renders), object B shadows a hit pixel p iff
    np_oracle.trace_shadow(S_B, rmi, d, (r, od)) finds an occluder, with d the
    float in plane 0 at p, (r, od) B's object-space ray of p as trace_kd's
    first four lines form it, and rmi = hit[p] - base_B when p is B's own
    pixel, else -1 (nothing excluded).  A shadowed pixel is 0x00000000.
    order: the objects' passes in that order (the result does not depend on
    it).  depth: {position in pixels: float} replaces plane 0's value for the
    test.  traced: the objects' trace_object results, when the caller has them.
    cnt: one list of five counters per object; object B's pass adds its shadow
    walks' visits (trace_shadow's cnt) to cnt[B], over every pixel it tests;
    with own_cnt (the same shape) the walks of B's own pixels go to own_cnt[B]
    instead (a skip_own pass walks the others alone).
    -> (argb u32 [m], hit i64 [m], planes u32 bits [10, m], classes) with
    classes = {"owner": i64 [m] (-1: a miss), "by": bool [nobj, m]}."""
    Ss = S if isinstance(S, list) else [S] * len(xforms)
    n = cam["w"] * cam["h"]
    pixels = np.arange(n) if pixels is None else np.asarray(pixels)
    if traced is None:
        traced = [trace_object(Ss[k], cam, xforms[k], pixels) for k in range(len(xforms))]
    bases = np.concatenate([[0], np.cumsum([len(s["e1"]) for s in Ss])]).astype(np.int64)
    argb, hit, planes = composite([(t[0], t[1], t[2], bases[k]) for k, t in enumerate(traced)])
    argb = argb.copy()
    m = len(pixels)
    owner = np.full(m, -1, np.int64)
    for k in range(len(xforms)):
        owner[(hit >= bases[k]) & (hit < bases[k + 1])] = k
    by = np.zeros((len(xforms), m), bool)
    d0 = planes[0].view(F)
    with np.errstate(all="ignore"):
        for B in (range(len(xforms)) if order is None else order):
            for j in np.nonzero(hit >= 0)[0]:
                d = d0[j] if depth is None or int(j) not in depth else F(depth[int(j)])
                rmi = int(hit[j] - bases[B]) if owner[j] == B else -1
                c = cnt if own_cnt is None or owner[j] != B else own_cnt
                by[B, j] = N.trace_shadow(Ss[B], rmi, d, traced[B][3][j], cnt=None if c is None else c[B])
            argb[by[B]] = 0
    return argb, hit, planes, {"owner": owner, "by": by}


def class_counts(classes):
    """(layer pixels shadowed by the base only, by both; base pixels shadowed
    by the layer only, by both) of a two-object frame."""
    o, by = classes["owner"], classes["by"]
    return (int(((o == 1) & by[0] & ~by[1]).sum()), int(((o == 1) & by[0] & by[1]).sum()),
            int(((o == 0) & by[1] & ~by[0]).sum()), int(((o == 0) & by[1] & by[0]).sum()))


# ------------------------------------------- the synthetic scenes' two-object frames
# (tables in tests/synth.py, conditions in tests/test_synth_cpu.py, the kernels in
# tests/test_gpu_xshadow_synth.py)

def _frozen(out):
    for a in out[:3]:
        a.setflags(write=False)
    return out


def two_objects(scs, cam, X, flat_base=False):
    """cross_shadow of scs[0]'s mesh at the identity and scs[1]'s at X from the
    numpy camera cam -> (want, prepared scenes, traced).  flat_base: the base
    layer is the flat list's render (the C oracle's frame and hit index, the
    planes by seq.hit_planes' flat arithmetic): the depths the passes read are
    then the flat walk's."""
    Ps = [N.prepare(sc.pts, N.nodes_from_array(sc.onodes), cam) for sc in scs]
    px = np.arange(cam["w"] * cam["h"])
    traced = [trace_object(Ps[0], cam, N.IDENT, px), trace_object(Ps[1], cam, X, px)]
    if flat_base:
        from tests import seq as Q
        argb, hit, _ = scs[0].oracle(1)
        rays = np.array([N.primary_ray(cam, i % cam["w"], i // cam["w"]) for i in px], F)
        planes = Q.hit_planes(Ps[0], rays, N.IDENT, Q.FLAT, hit, N.RAD).view(F)
        traced[0] = (argb, hit, planes, traced[0][3])
    return _frozen(cross_shadow(Ps, cam, [N.IDENT, X], traced=traced)), Ps, traced


@functools.lru_cache(None)
def pair_want(pose, k, flat_base=False):
    """The two soups of synth.XSHADOW_CLASSES[pose, k]: light_scene(pose) at the
    identity under itself at the offset XSHADOW_OFFSETS[k]."""
    from tests import synth as SY
    with SY.light_scene(pose) as sc:
        return two_objects([sc, sc], sc.np_camera(), offset_xform(*SY.XSHADOW_OFFSETS[k]), flat_base)


@functools.lru_cache(None)
def tiny_want(n, small_is_layer):
    """soup(n) over (small_is_layer) or under soup(65) of synth.XSHADOW_TINY."""
    from tests import synth as SY
    with SY.soup_scene(n) as small, SY.soup_scene(SY.LIGHT_N) as big:
        scs = [big, small] if small_is_layer else [small, big]
        return two_objects(scs, big.np_camera(), offset_xform(*SY.XSHADOW_TINY_OFFSET))


# ------------------------------------------------------------ the dump 40x24 cases

W, H = 40, 24
#: name -> the layer's transform (the base is at the identity)
DUMP_CASES = {"near": offset_xform(-0.1, -0.1, -0.05), "far": offset_xform(0.1, 0.1, 0.05), "moved": None}


@functools.lru_cache(None)
def dump_scene():
    G = make_aov()
    pts, nodes = G._scene("dump")
    cam = G.camera("dump", W, H)
    return N.prepare(pts, nodes, cam), cam, pts, nodes


def dump_xform(name):
    return make_aov().moved_xform("dump", W, H) if name == "moved" else DUMP_CASES[name]


@functools.lru_cache(None)
def dump_traced(name):
    S, cam, _, _ = dump_scene()
    X = N.IDENT if name == "ident" else dump_xform(name)
    return trace_object(S, cam, X, np.arange(W * H))


@functools.lru_cache(None)
def dump_want(name):
    """cross_shadow of the base at the identity and the layer of case `name`."""
    S, cam, _, _ = dump_scene()
    out = cross_shadow(S, cam, [N.IDENT, dump_xform(name)], traced=[dump_traced("ident"), dump_traced(name)])
    for a in out[:3]:
        a.setflags(write=False)
    return out


def test_offset_cases_have_cross_only_pixels():
    """The pixels that change colour only through the new pass."""
    near, far = class_counts(dump_want("near")[3]), class_counts(dump_want("far")[3])
    print("near", near, "far", far)
    assert near[:2] == (20, 30)
    assert far[2:] == (14, 28)


def test_moved_pose_classes():
    c = dump_want("moved")[3]
    o, by = c["owner"], c["by"]
    assert int(((o == 1) & by[0] & by[1]).sum()) == 19 and int(((o == 0) & by[0] & by[1]).sum()) == 1


def test_single_object_is_the_shadow_render():
    S, cam, pts, nodes = dump_scene()
    argb, hit, _, c = cross_shadow(S, cam, [N.IDENT], traced=[dump_traced("ident")])
    oargb, ohit = N.render(pts, nodes, cam, shadow=True)
    assert (hit == ohit).all() and (argb == oargb).all()
    assert c["by"][0].sum() > 0 and ((argb == 0) == c["by"][0]).all()


def subset(traced, idx):
    """trace_object's result at the positions idx."""
    argb, hit, planes, rays = traced
    return argb[idx], hit[idx], planes[:, idx], [rays[int(i)] for i in idx]


def test_pass_order_does_not_matter():
    S, cam, _, _ = dump_scene()
    b = dump_want("near")
    idx = np.nonzero(b[1] >= 0)[0]  # every hit pixel (a miss is never tested)
    tr = [subset(dump_traced("ident"), idx), subset(dump_traced("near"), idx)]
    a = cross_shadow(S, cam, [N.IDENT, dump_xform("near")], pixels=idx, order=(1, 0), traced=tr)
    assert (a[0] == b[0][idx]).all() and (a[3]["by"] == b[3]["by"][:, idx]).all()


def test_nan_depth_is_not_shadowed():
    S, cam, _, _ = dump_scene()
    want = dump_want("near")
    idx = np.nonzero(want[3]["by"].all(0))[0][:3]  # shadowed by both objects
    tr = [subset(dump_traced("ident"), idx), subset(dump_traced("near"), idx)]
    for bad in (np.nan, np.inf, -np.inf):
        got = cross_shadow(S, cam, [N.IDENT, dump_xform("near")], pixels=idx, depth={0: bad}, traced=tr)
        assert not got[3]["by"][:, 0].any() and got[0][0] != 0
        assert (got[0][1:] == 0).all() and got[3]["by"][:, 1:].all()  # the others as they were


# ------------------------------------------------------------------ ABI and facade

def test_abi_declares_rt_shadow_over():
    with open(os.path.join(ROOT, "include", "rt_mi355x.h")) as fp:
        header = fp.read()
    pat = (r"int rt_shadow_over\(rt_camera\* c, const float\* xform, uint32_t flags, const rt_tile\* tile,\s+"
           r"uint32_t\* d_argb, int64_t\* d_hit, int64_t hit_base, int32_t skip_own, void\* stream\);")
    assert re.search(pat, header)
    res, args = _lib.SIGNATURES["rt_shadow_over"]
    P = _lib.C.c_void_p
    assert res is _lib.C.c_int
    assert args == [P, P, _lib.C.c_uint32, _lib.C.POINTER(_lib.RtTile), P, P, _lib.C.c_int64, _lib.C.c_int32, P]
    assert "#define RT_ABI_VERSION 2" in header
    assert not re.search(r"#define RT_FLAG_\w+ (32|64)u", header)
    assert "objects do not shadow one another" not in header
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.C.CDLL(_lib.LIB_PATH), "rt_shadow_over")


FACADE_USER = r"""
#include <cstdio>
#include "rt_facade.hpp"
using namespace rtmi;
int frame(Camera* cam, Object* obj1, Object* obj2) {
    int rc = obj1->render(cam);
    if (!rc) rc = obj2->render(cam);
    if (!rc) rc = cam->shadow_layers();
    return rc ? rc : cam->color_pixels(PHONG_COLOR_TAG);
}
int main(int argc, char**) {
    Camera cam(16, 8, film_w(16, 8), .024f, .055f, 0, .1f, -1, 0, .1f, 0, 0, 1, 0);
    Object* obj1 = nullptr;
    Object* obj2 = nullptr;
    if (argc > 100) {  // never: compiled and linked, not run
        cam.add_object(obj1);
        cam.add_layer(obj2);
        std::printf("%d\n", frame(&cam, obj1, obj2));
    }
    return 0;
}
"""


def test_facade_shadow_layers_compiles(tmp_path):
    """Camera::shadow_layers compiles warning-free against the header and
    links against the library."""
    src = tmp_path / "xshadow_user.cpp"
    src.write_text(FACADE_USER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o",
                    str(tmp_path / "xshadow_user"), str(src), _lib.LIB_PATH], check=True)
