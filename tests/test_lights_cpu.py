"""CPU tests of the light list (rt_camera_set_lights, rt_light_over,
rt_shade_lights): the numpy reference tests/lights_ref.py the GPU tests
compare with, anchored on the cross-shadowed frames of
tests/test_xshadow_cpu.py; the pixel classes of the cases those tests use; the
C ABI's new functions in the header and the ctypes table; the facade's
Camera::set_lights / light_layers; and restated wrong kernels that the
comparison must tell from the reference.  No GPU calls."""
import functools
import os
import re
import subprocess

import numpy as np

from cpp_cuda_raytracer_dev_amd import _lib
from oracle import np_oracle as N
from tests import lights_ref as LR
from tests.test_xshadow_cpu import (dump_scene, dump_traced, dump_want, dump_xform, offset_xform, trace_object)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32

#: the three lights of the dump cases: the literal one, one mirrored in x at
#: half the intensity, one below and behind the eye at twice
L3 = ((2, 2, 2, 1), (-2, 2, 2, 0.5), (0.5, -2, -1, 2))
L2 = L3[:2]
L4 = L3 + ((2, -1, 0.5, 0.25),)
#: hit pixels per mask value 0..7 of the dump cases under L3
DUMP_MASKS = {"near": (0, 14, 11, 57, 2, 5, 1, 2), "far": (2, 8, 9, 52, 1, 5, 2, 3), "moved": (1, 9, 8, 23, 1, 1, 3, 2)}
#: distinct colours among the hit pixels (the background, a miss's colour, is one more over the
#: whole frame: "far" has 44)
DUMP_COLOURS = {"near": 46, "far": 43, "moved": 33}


@functools.lru_cache(None)
def dump_lit(name, lights=L3):
    """lit_composite of the dump base at the identity and the layer of case `name`."""
    S, cam, _, _ = dump_scene()
    out = LR.lit_composite(S, cam, [N.IDENT, dump_xform(name)], lights, traced=[dump_traced("ident"), dump_traced(name)])
    for a in out[:4]:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------ the anchor

def test_default_list_is_the_cross_shadowed_frame():
    for name in ("near", "far", "moved"):
        got, want = dump_lit(name, LR.DEFAULT_LIGHTS), dump_want(name)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[2] == want[2]).all(), name
        assert ((got[3] == 1) == want[3]["by"].any(0)).all() and (got[3] <= 1).all()


def test_single_object_is_the_shadow_render():
    S, cam, pts, nodes = dump_scene()
    argb, hit, _, mask, _ = LR.lit_composite(S, cam, [N.IDENT], LR.DEFAULT_LIGHTS, traced=[dump_traced("ident")])
    oargb, ohit = N.render(pts, nodes, cam, shadow=True)
    assert (hit == ohit).all() and (argb == oargb).all()
    assert mask.sum() > 0 and ((argb == 0) == (mask == 1)).all()


# ------------------------------------------------------------------------ classes

def test_every_subset_of_occluded_lights_occurs():
    for name, table in DUMP_MASKS.items():
        argb, hit, _, mask, _ = dump_lit(name)
        got = tuple(np.bincount(mask[hit >= 0], minlength=8).tolist())
        colours = len(np.unique(argb[hit >= 0]))
        print(name, got, colours)
        assert got == table and colours == DUMP_COLOURS[name]
        assert (mask[hit < 0] == 0).all()
        assert (argb[(hit >= 0) & (mask == 7)] == 0).all()  # every light occluded: the shadow colour
    assert all(DUMP_MASKS["far"]) and DUMP_MASKS["near"][0] == 0


def test_dump_cross_object_occlusion_is_light_0_alone():
    """Only light 0 is occluded across objects in the offset cases (the
    cross-object classes of the other lights come from the two soups)."""
    near = [LR.light_class_counts(dump_lit("near")[4], l) for l in range(3)]
    far = [LR.light_class_counts(dump_lit("far")[4], l) for l in range(3)]
    assert near == [(20, 30, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)] and sum(near[0][:2]) == 50
    assert far == [(0, 0, 14, 28), (0, 0, 0, 0), (0, 0, 0, 0)] and sum(far[0][2:]) == 42


# ---------------------------------------------------------------------- two soups

def soup_lights(pose):
    """Eight lights at the soups' centre relative to the eye of light_pose
    `pose` (2 + o per axis) + 2 * q for q in {-1, +1}^3, intensity 1."""
    from tests import synth as SY
    c = 2.0 + np.array(SY.LIGHT_O[pose], np.float64)
    return tuple(tuple(float(F(x)) for x in c + 2.0 * np.array(q)) + (1.0,) for q in SY.LIGHT_OCTANTS)


@functools.lru_cache(None)
def soups_lit(pose, k, lights=None):
    """soup(65) at the identity under itself at synth.XSHADOW_OFFSETS[k] from
    the eye `pose`, lit by soup_lights(pose) -> (lit_composite's result,
    prepared scenes, traced)."""
    from tests import synth as SY
    with SY.light_scene(pose) as sc:
        cam = sc.np_camera()
        P = N.prepare(sc.pts, N.nodes_from_array(sc.onodes), cam)
        X = offset_xform(*SY.XSHADOW_OFFSETS[k])
        px = np.arange(cam["w"] * cam["h"])
        traced = [trace_object(P, cam, N.IDENT, px), trace_object(P, cam, X, px)]
        out = LR.lit_composite([P, P], cam, [N.IDENT, X], soup_lights(pose) if lights is None else lights, traced=traced)
    for a in out[:4]:
        a.setflags(write=False)
    return out, [P, P], traced


#: (pose, offset index) -> per light the four class_counts (layer pixels whose
#: light the base alone / both occlude, base pixels the layer alone / both)
SOUP_CLASSES = {
    ("ppp", 0): ((9, 0, 4, 0), (23, 24, 48, 66), (54, 5, 12, 2), (18, 6, 23, 15), (18, 20, 41, 11), (14, 24, 73, 76),
                 (49, 5, 14, 24), (19, 15, 42, 60)),
    ("ppp", 1): ((6, 0, 17, 1), (41, 12, 11, 12), (14, 14, 73, 37), (22, 8, 53, 48), (54, 1, 4, 12), (62, 14, 2, 18),
                 (20, 13, 27, 14), (47, 33, 20, 51)),
    ("nnn", 0): ((8, 2, 3, 0), (15, 21, 51, 67), (35, 4, 13, 3), (14, 5, 20, 10), (13, 20, 39, 13), (10, 18, 79, 84),
                 (31, 6, 18, 13), (8, 13, 52, 78)),
    # a straddle eye: the first light's x is exactly 0 relative to the eye (its ray offset -0.0)
    ("zpp", 1): ((19, 6, 23, 3), (41, 15, 16, 22), (11, 13, 70, 48), (29, 12, 70, 40), (74, 2, 5, 8), (48, 17, 5, 19),
                 (20, 24, 22, 15), (63, 21, 25, 35)),
}


def test_two_soups_every_light_is_occluded_across_objects():
    """Every light (none lies within the root box's range on all axes: they
    are 2 away from the centre on each) has at least 2 pixels that only the
    other object occludes it at."""
    for (pose, k), table in SOUP_CLASSES.items():
        out = soups_lit(pose, k)[0]
        got = tuple(LR.light_class_counts(out[4], l) for l in range(8))
        print(pose, k, got)
        assert got == table
        for l, c in enumerate(got):
            assert c[0] + c[2] >= 2, (pose, k, l, c)


# -------------------------------------------------------------------- intensities

def _with_intensity(lights, f):
    return tuple((x, y, z, f(l, i)) for l, (x, y, z, i) in enumerate(lights))


def test_a_power_of_two_on_every_intensity_changes_nothing():
    for name in ("near", "far"):
        want = dump_lit(name)
        for k in (-3, 5):
            got = dump_lit(name, _with_intensity(L3, lambda l, i: i * 2.0 ** k))
            assert (got[0] == want[0]).all() and (got[3] == want[3]).all(), (name, k)


def test_a_light_of_intensity_zero_contributes_nothing():
    """... to the colour: the frame is the one without it wherever the other
    lights reach the pixel.  Its visibility bit is still found."""
    with_zero = dump_lit("far", _with_intensity(L3, lambda l, i: 0.0 if l == 1 else i))
    without = dump_lit("far", (L3[0], L3[2]))
    assert (with_zero[3] == dump_lit("far")[3]).all()
    assert (with_zero[0] == without[0]).all()


def test_swapping_two_lights_moves_mask_bits_alone():
    a, b = dump_lit("far"), dump_lit("far", (L3[1], L3[0], L3[2]))
    swapped = (a[3] & 4) | ((a[3] & 1) << 1) | ((a[3] & 2) >> 1)
    assert (b[3] == swapped).all()
    # the first two terms of the sum trade places, and (0 + a) + b == (0 + b) + a exactly
    assert (b[0] == a[0]).all()


# ------------------------------------------------------------- header and layers

def test_abi_declares_the_light_list():
    with open(os.path.join(ROOT, "include", "rt_mi355x.h")) as fp:
        header = fp.read()
    assert re.search(r"#define RT_LIGHTS_MAX 8\b", header) and _lib.RT_LIGHTS_MAX == 8
    for pat in (r"int rt_camera_set_lights\(rt_camera\* c, const float\* lights4, int32_t n\);",
                r"int rt_camera_get_lights\(rt_camera\* c, float\* lights4, int32_t\* n\);",
                r"int rt_light_over\(rt_camera\* c, const float\* xform, uint32_t flags, const rt_tile\* tile,\s+"
                r"uint32_t\* d_argb, int64_t\* d_hit, int64_t hit_base, void\* stream\);",
                r"int rt_shade_lights\(rt_camera\* c, uint32_t flags, const rt_tile\* tile, uint32_t\* d_argb, "
                r"int64_t\* d_hit,\s+void\* stream\);"):
        assert re.search(pat, header), pat
    Cc, P = _lib.C, _lib.C.c_void_p
    T = Cc.POINTER(_lib.RtTile)
    assert _lib.SIGNATURES["rt_camera_set_lights"] == (Cc.c_int, [P, P, Cc.c_int32])
    assert _lib.SIGNATURES["rt_camera_get_lights"] == (Cc.c_int, [P, P, Cc.POINTER(Cc.c_int32)])
    assert _lib.SIGNATURES["rt_light_over"] == (Cc.c_int, [P, P, Cc.c_uint32, T, P, P, Cc.c_int64, P])
    assert _lib.SIGNATURES["rt_shade_lights"] == (Cc.c_int, [P, Cc.c_uint32, T, P, P, P])
    assert "#define RT_ABI_VERSION 2" in header
    assert not re.search(r"#define RT_FLAG_\w+ (32|64)u", header)
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.C.CDLL(_lib.LIB_PATH)
        for name in ("rt_camera_set_lights", "rt_camera_get_lights", "rt_light_over", "rt_shade_lights"):
            assert hasattr(L, name), name


FACADE_USER = r"""
#include <cstdio>
#include "rt_facade.hpp"
using namespace rtmi;
int frame(Camera* cam, Object* obj1, Object* obj2) {
    const float lights[8] = {2, 2, 2, 1, -2, 2, 2, .5f};
    int rc = cam->set_lights(lights, 2);
    if (!rc) rc = obj1->render(cam);
    if (!rc) rc = obj2->render(cam);
    if (!rc) rc = cam->light_layers();
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


def test_facade_light_layers_compiles(tmp_path):
    """Camera::set_lights / light_layers compile warning-free against the
    header and link against the library."""
    src = tmp_path / "lights_user.cpp"
    src.write_text(FACADE_USER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o",
                    str(tmp_path / "lights_user"), str(src), _lib.LIB_PATH], check=True)


# ------------------------------------------------------------------ wrong kernels
# Each fault is a kernel one could write by mistake, restated in numpy and fed
# to the comparison the GPU tests use (every pixel of frame and mask equal).

def same(got, want):
    return bool((got[0] == want[0]).all() and (got[3] == want[3]).all())


def literal_after_light_0(S, rmi, d, ray, L, cnt=None):
    """H - 2 kept literal: only a light at (2,2,2) gets its own segment."""
    return LR.shadow_from(S, rmi, d, ray, (2, 2, 2), cnt)


def intensity_after_normalisation(pnt, nrm, rmd, rad, lights, occ):
    """c accumulates without I; the normalised channels are scaled by the
    mean intensity of the visible lights instead."""
    lights = LR.as_lights(lights)
    c = [F(0), F(0), F(0)]
    seen = [L[3] for l, L in enumerate(lights) if not (occ >> l) & 1]
    with np.errstate(all="ignore"):
        for l, L in enumerate(lights):
            if not (occ >> l) & 1:
                diff, spec = LR.light_terms(pnt, nrm, rmd, L)
                c = [F(c[k] + F(F(F(rad[k]) * diff) + spec)) for k in range(3)]
        s = F(np.mean(seen)) if seen else F(1)
        return LR.normalise([F(x * s) for x in c]) if seen else LR.normalise(c)


def _dump_fault(name, **kw):
    S, cam, _, _ = dump_scene()
    return LR.lit_composite(S, cam, [N.IDENT, dump_xform(name)], L3, traced=[dump_traced("ident"), dump_traced(name)], **kw)


def test_fault_literal_segment_fails_on_far():
    got = _dump_fault("far", shadow=literal_after_light_0)
    assert not same(got, dump_lit("far"))
    assert ((got[3] & 1) == (dump_lit("far")[3] & 1)).all()  # light 0 is the literal: its bit is right


def test_fault_own_exclusion_on_foreign_pixels_fails_on_the_two_soups():
    """A kernel that excludes the pixel's triangle index (within its owner)
    from every object's walk: with the same mesh twice, the layer's triangle
    t can be shadowed by the base's triangle t, which this drops: 12 pixels'
    masks of the two soups ("ppp", offset 0).  The dump cases do not tell it.
    (Taken literally, hit[p] - hit_base of B at a foreign pixel is never a
    triangle of B while the hit bases are disjoint ranges, so that form of the
    fault cannot show on any frame.)"""
    from tests import synth as SY
    want, Ps, traced = soups_lit("ppp", 0)
    with SY.light_scene("ppp") as sc:
        cam = sc.np_camera()
    got = LR.lit_composite(Ps, cam, [N.IDENT, offset_xform(*SY.XSHADOW_OFFSETS[0])], soup_lights("ppp"), traced=traced,
                           foreign_own=True)
    assert not same(got, want) and int((got[3] != want[3]).sum()) == 12


def test_fault_intensity_after_normalisation_fails_on_far():
    got = _dump_fault("far", shade=intensity_after_normalisation)
    want = dump_lit("far")
    assert (got[3] == want[3]).all() and not same(got, want)


# Accumulation in reverse light order is not among the faults: no frame here
# tells it.  Two terms commute exactly, so only pixels that three or more
# lights reach can differ, and there a different order moves a channel sum by
# an ulp or two of a float, which changes (u8)((c / mx) * 255) only when the
# quotient sits within ~2^-22 of an integer step: none of the ~420 hit pixels
# of the eight-light soups ("ppp", offset 0) nor of the dump cases does.  The
# index order is pinned by the definition and by the kernel's text alone.
