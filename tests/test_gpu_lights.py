"""GPU tests of the light list: rt_light_over ORs, per object, the lights that
object occludes into the top byte of a composite's frame words, and
rt_shade_lights turns planes 1-9, that byte and the camera's lights into the
colour.  Every expected frame and mask is ``lit_composite`` (tests/lights_ref.py,
the numpy oracle's walk and arithmetic), ``cross_shadow`` or a committed
fixture, never the new entry points' own output; tests/test_lights_cpu.py shows
which wrong kernels this comparison (every pixel equal) catches.  Frames are at
most 96 x 54."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from cpp_cuda_raytracer_dev_amd import _lib, raytracer as R, scenes
from oracle import np_oracle as N
from tests import helpers as H, lights_ref as LR, synth as SY
from tests.test_gpu_over import POISON, Targets, assert_same, scene
from tests.test_gpu_xshadow import PASS_CFGS, counters_match, pass_options, shadow
from tests.test_gpu_xshadow_synth import live, set_all
from tests.test_lights_cpu import L2, L3, L4, dump_lit, soup_lights, soups_lit
from tests.test_xshadow_cpu import (NTRI_DUMP, dump_scene, dump_want, dump_xform, offset_xform, trace_object)

pytestmark = pytest.mark.gpu

COUNT, FRAME_OUT = R.RT_FLAG_COUNT, R.RT_FLAG_FRAME_OUT
W, Hh = 40, 24
F = np.float32


def light(t, cam, **kw):
    """The visibility pass of cam's object over the targets t."""
    t.bind(cam)
    cam.light_over(t.argb, t.hit, **kw)
    return t


def shade(t, cam, **kw):
    t.bind(cam)
    cam.shade_lights(t.argb, t.hit, **kw)
    return t


def set_lights(cams, lights):
    for cam in cams:
        cam.set_lights(lights)


def lit(t, cams, xforms, bases, order=None, **kw):
    """Every object's visibility pass (in `order`), the frame between the
    passes and the shading, then the shading pass by the first camera.
    -> (the frame words with the mask in the top byte, the shaded read)."""
    for k in (range(len(cams)) if order is None else order):
        light(t, cams[k], xform=xforms[k], hit_base=bases[k], **kw)
    marked = t.read()[0]
    shade(t, cams[0], **kw)
    return marked, t.read()


def check_lit(marked, got, before, want, what=""):
    """The mask in the top byte and the untouched low bits between the passes;
    then lit_composite's frame, with hit and planes as the composite had them."""
    assert ((marked >> 24) == want[3]).all(), (what, "mask", np.nonzero((marked >> 24) != want[3])[0][:8])
    assert ((marked & 0xFFFFFF) == (before[0] & 0xFFFFFF)).all(), (what, "low bits")
    assert (marked[before[1] < 0] == before[0][before[1] < 0]).all(), (what, "misses")
    assert_same(got, (want[0], before[1], before[2]), what)


# ------------------------------------------------------------------ 1. default list

@pytest.mark.parametrize("case", ["near", "far", "moved"])
def test_default_list_is_the_cross_shadowed_frame(case):
    want = dump_want(case)
    X = dump_xform(case)
    with scene("dump", W, Hh) as base, scene("dump", W, Hh) as layer:
        cams = (base.cam, layer.cam)
        assert (base.cam.lights == np.array([[2, 2, 2, 1]], F)).all()
        t = Targets(W * Hh).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=NTRI_DUMP)
        before = t.read()
        frame0 = t.argb.clone()
        assert_same(before[1:], want[1:3], (case, "the composite"))
        shadow(t, base.cam)
        shadow(t, layer.cam, xform=X, hit_base=NTRI_DUMP)
        assert_same(t.read(), (want[0], before[1], before[2]), (case, "rt_shadow_over"))
        for tile_order in (0, 1):
            set_all(cams, _lib.RT_OPT_TILE_ORDER, tile_order)
            for items, order in PASS_CFGS:
                pass_options(cams, items, order)
                for first in (0, 1):
                    t.argb.copy_(frame0)
                    marked, got = lit(t, cams, (None, X), (0, NTRI_DUMP), order=(first, 1 - first))
                    what = (case, tile_order, items, order, first)
                    assert ((marked >> 24) == want[3]["by"].any(0)).all(), what
                    assert_same(got, (want[0], before[1], before[2]), what)


# -------------------------------------------------------- 2. masks and frames: dump

@pytest.mark.parametrize("lights", [L2, L3, L4], ids=["2", "3", "4"])
@pytest.mark.parametrize("case", ["near", "far", "moved"])
def test_dump_lit_frames(case, lights):
    want = dump_lit(case, lights)
    X = dump_xform(case)
    with scene("dump", W, Hh) as base, scene("dump", W, Hh) as layer:
        cams = (base.cam, layer.cam)
        set_lights(cams, lights)
        assert (layer.cam.lights == np.array(lights, F)).all()
        t = Targets(W * Hh).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=NTRI_DUMP)
        before = t.read()
        marked, got = lit(t, cams, (None, X), (0, NTRI_DUMP))
        check_lit(marked, got, before, want, (case, len(lights)))


# ---------------------------------------------------------- 3. idempotence and order

def test_passes_are_idempotent_commute_and_or_into_preset_bits():
    import torch
    want = dump_lit("far")
    X = dump_xform("far")
    with scene("dump", W, Hh) as base, scene("dump", W, Hh) as layer:
        cams = (base.cam, layer.cam)
        set_lights(cams, L3)
        t = Targets(W * Hh).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=NTRI_DUMP)
        before = t.read()
        frame0 = t.argb.clone()
        args = ((dict(), dict(xform=X, hit_base=NTRI_DUMP)))
        seen = []
        for run in ((0, 1), (1, 0), (0, 0, 1, 1, 0)):
            t.argb.copy_(frame0)
            for k in run:
                light(t, cams[k], **args[k])
            seen.append(t.read())
            assert ((seen[-1][0] >> 24) == want[3]).all(), run
            assert_same(seen[-1][1:], before[1:], run)
        # one pass alone: that object's bits
        for k in (0, 1):
            t.argb.copy_(frame0)
            one = light(t, cams[k], **args[k]).read()[0] >> 24
            by = want[4]["by"][k]
            assert (one == sum(by[l].astype(np.uint32) << l for l in range(3))).all(), k
        # bits set by hand: at hit pixels (kept, ORed with what is found) and at a miss (never touched)
        hits = np.nonzero(before[1] >= 0)[0]
        chosen = hits[::5]
        miss = int(np.nonzero(before[1] < 0)[0][3])
        preset = np.zeros(W * Hh, np.uint32)
        preset[chosen] = (np.arange(len(chosen)) % 255 + 1).astype(np.uint32) << 24
        preset[miss] = 0xA5 << 24
        t.argb.copy_(torch.from_numpy((before[0] | preset).view(np.int32)).cuda())
        for k in (1, 0):
            light(t, cams[k], **args[k])
        got = t.read()
        wantw = before[0] | preset
        wantw[hits] |= want[3][hits].astype(np.uint32) << 24
        assert (got[0] == wantw).all()
        assert_same(got[1:], before[1:])


# --------------------------------------------------------------------- 4. counters

@pytest.mark.parametrize("case", ["near", "far"])
def test_counters_are_the_summed_per_light_walks(case):
    import torch
    want = dump_lit(case)
    X = dump_xform(case)
    with scene("dump", W, Hh) as base, scene("dump", W, Hh) as layer:
        cams = (base.cam, layer.cam)
        set_lights(cams, L3)
        t = Targets(W * Hh).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=NTRI_DUMP)
        before = t.read()
        frame0 = t.argb.clone()
        args = ((dict(), dict(xform=X, hit_base=NTRI_DUMP)))
        full = [LR.summed_counters(want[4], k) for k in (0, 1)]
        preset = np.where(before[1] >= 0, np.uint32(0x05000000), np.uint32(0))  # lights 0 and 2 marked everywhere
        walked = {}  # (pre, run, object) -> the full counted pass's own counters
        for pre in (False, True):
            for debug in (0, 16):
                set_all(cams, _lib.RT_OPT_DEBUG, debug)
                for run in ((0, 1), (1, 0)):
                    t.argb.copy_(frame0 if not pre else torch.from_numpy((before[0] | preset).view(np.int32)).cuda())
                    for cam in cams:
                        cam.counters()
                    for k in run:
                        light(t, cams[k], flags=COUNT, **args[k])
                    got = t.read()
                    assert ((got[0] >> 24) == (want[3] | ((preset >> 24) if pre else 0))).all(), (pre, debug, run)
                    for k in (0, 1):
                        cnt = cams[k].counters()
                        assert int(cnt[3]) == 0
                        if debug:
                            # walks that stop at occluders visit a subset of the full walks' nodes: [0], [1],
                            # [4] no larger than the reference's sums, [2] (kernel 3's valid candidates, which
                            # may exceed the DFS's accepts) no larger than the full counted pass's own
                            for i in (0, 1, 4):
                                assert 0 < int(cnt[i]) <= full[k][i], (pre, run, k, i, cnt, full[k])
                            assert 0 < int(cnt[2]) <= int(walked[pre, run, k][2]), (pre, run, k, cnt)
                        else:  # every light of every tested pixel, whatever the bits on entry and the order
                            counters_match(cnt, full[k][:3] + [0] + full[k][4:])
                            walked[pre, run, k] = cnt
        set_all(cams, _lib.RT_OPT_DEBUG, 0)
        # a timed pass adds nothing to the counters
        light(t, cams[0])
        assert not cams[0].counters().any()


# ------------------------------------------------------------------ 5. the two soups

@pytest.mark.parametrize("pose,k", [("ppp", 0), ("ppp", 1), ("nnn", 0), ("zpp", 1)])
def test_two_soups_eight_lights(pose, k):
    want = soups_lit(pose, k)[0]
    X = offset_xform(*SY.XSHADOW_OFFSETS[k])
    with live(SY.light_scene(pose), SY.light_scene(pose)) as (base, layer):
        cams = (base.cam, layer.cam)
        n, ntri = base.w * base.h, len(base.pts)
        set_lights(cams, soup_lights(pose))
        t = Targets(n).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=ntri)
        before = t.read()
        frame0 = t.argb.clone()
        assert_same(before[1:], want[1:3], (pose, k, "the composite"))
        for items, order in ((2, 1), (1, 2)):
            pass_options(cams, items, order)
            for first in (0, 1):
                t.argb.copy_(frame0)
                marked, got = lit(t, cams, (None, X), (0, ntri), order=(first, 1 - first))
                check_lit(marked, got, before, want, (pose, k, items, order, first))
        # the counted passes: each object's eight walks of every hit pixel
        t.argb.copy_(frame0)
        for j, cam in enumerate(cams):
            cam.counters()
            light(t, cam, xform=(None, X)[j], hit_base=(0, ntri)[j], flags=COUNT)
            full = LR.summed_counters(want[4], j)
            counters_match(cam.counters(), full[:3] + [0] + full[4:])


@functools.lru_cache(None)
def tiny_lit(n, small_is_layer):
    """soup(n) over (small_is_layer) or under soup(65) at synth.XSHADOW_TINY_OFFSET, three lights."""
    with SY.soup_scene(n) as small, SY.soup_scene(SY.LIGHT_N) as big:
        scs = [big, small] if small_is_layer else [small, big]
        cam = big.np_camera()
        Ps = [N.prepare(sc.pts, N.nodes_from_array(sc.onodes), cam) for sc in scs]
        return LR.lit_composite(Ps, cam, [N.IDENT, offset_xform(*SY.XSHADOW_TINY_OFFSET)], L3)


@pytest.mark.parametrize("small_is_layer", [False, True], ids=["under", "over"])
@pytest.mark.parametrize("n", [1, 2, 9, 257])
def test_tiny_soups(n, small_is_layer):
    """A leaf root (n = 1), a root with leaf children (2) and pools of a few
    items as the occluder and as the receiver."""
    want = tiny_lit(n, small_is_layer)
    X = offset_xform(*SY.XSHADOW_TINY_OFFSET)
    with live(SY.soup_scene(n), SY.soup_scene(SY.LIGHT_N)) as (small, big):
        scs = (big, small) if small_is_layer else (small, big)
        cams = (scs[0].cam, scs[1].cam)
        ntri = len(scs[0].pts)
        set_lights(cams, L3)
        t = Targets(big.w * big.h).clear(cams[0]).over(cams[0]).over(cams[1], xform=X, hit_base=ntri)
        before = t.read()
        assert_same(before[1:], want[1:3], (n, "the composite"))
        marked, got = lit(t, cams, (None, X), (0, ntri))
        check_lit(marked, got, before, want, (n, small_is_layer))


# ----------------------------------------- 6. transforms, other owners, materials

@functools.lru_cache(None)
def dump_lit_xf(key):
    S, cam, _, _ = dump_scene()
    X = {"rot": H.rot_y(17.0, (0.05, 0.02, -0.03)), "xlate": H.rot_y(0.0, (0.01, -0.005, 0.02))}[key]
    return LR.lit_composite(S, cam, [N.IDENT, np.asarray(X, F)], L3), np.asarray(X, F)


@pytest.mark.parametrize("key", ["rot", "xlate"])
def test_layer_under_a_rotation_and_a_translation(key):
    want, X = dump_lit_xf(key)
    with scene("dump", W, Hh) as base, scene("dump", W, Hh) as layer:
        cams = (base.cam, layer.cam)
        set_lights(cams, L3)
        t = Targets(W * Hh).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=NTRI_DUMP)
        before = t.read()
        assert_same(before[1:], want[1:3], (key, "the composite"))
        marked, got = lit(t, cams, (None, X), (0, NTRI_DUMP))
        check_lit(marked, got, before, want, key)


@pytest.mark.parametrize("owner", [dict(kernel=2), dict(flat=12)], ids=["kernel2", "flat"])
def test_owner_from_kernel_2_or_the_flat_list(owner):
    """The base layer rendered by kernel 2 or by the flat list (its planes are
    the flat walk's), shaded by that camera's rt_shade_lights; the visibility
    passes run on kernel-3 cameras of the same pose."""
    case = "far"
    X = dump_xform(case)
    flat = "flat" in owner
    with scene("dump", W, Hh, **owner) as first, scene("dump", W, Hh) as base, scene("dump", W, Hh) as layer:
        set_lights((first.cam, base.cam, layer.cam), L3)
        t = Targets(W * Hh).clear(first.cam).over(first.cam, mode=1 if flat else 0)
        t.over(layer.cam, xform=X, hit_base=NTRI_DUMP)
        before = t.read()
        S, cam, _, _ = dump_scene()
        px = np.arange(W * Hh)
        traced = [trace_object(S, cam, N.IDENT, px), trace_object(S, cam, X, px)]
        if flat:  # the depths and points the passes read are the flat walk's
            base_planes = Targets(W * Hh).clear(first.cam).over(first.cam, mode=1).read()
            traced[0] = (base_planes[0], base_planes[1], base_planes[2].view(F), traced[0][3])
        want = LR.lit_composite(S, cam, [N.IDENT, X], L3, traced=traced)
        assert_same(before[1:], want[1:3], (owner, "the composite"))
        light(t, base.cam)
        light(t, layer.cam, xform=X, hit_base=NTRI_DUMP)
        marked = t.read()[0]
        shade(t, first.cam)
        check_lit(marked, t.read(), before, want, owner)


@functools.lru_cache(None)
def materials_lit():
    (n0, tab0, _), (n1, tab1, X) = SY.OVER_LAYERS
    with SY.material_scene(tab0, n0) as a, SY.material_scene(tab1, n1) as b:
        cam = a.np_camera()
        Ps = [N.prepare(sc.pts, N.nodes_from_array(sc.onodes), cam) for sc in (a, b)]
        px = np.arange(cam["w"] * cam["h"])
        Xn = np.asarray(X, F)
        traced = [trace_object(Ps[0], cam, N.IDENT, px, rad=a.rad), trace_object(Ps[1], cam, Xn, px, rad=b.rad)]
        return LR.lit_composite(Ps, cam, [N.IDENT, Xn], L3, traced=traced), Xn


def test_material_tables_on_the_two_layers():
    """Per-triangle radiances, the edge table's zeros, negatives and huge
    values among them, through plane 7-9 into the sum."""
    want, X = materials_lit()
    (n0, tab0, _), (n1, tab1, _) = SY.OVER_LAYERS
    with live(SY.material_scene(tab0, n0), SY.material_scene(tab1, n1)) as (a, b):
        cams = (a.cam, b.cam)
        ntri = len(a.pts)
        set_lights(cams, L3)
        t = Targets(a.w * a.h).clear(a.cam).over(a.cam).over(b.cam, xform=X, hit_base=ntri)
        before = t.read()
        assert_same(before[1:], want[1:3], "the composite")
        marked, got = lit(t, cams, (None, X), (0, ntri))
        check_lit(marked, got, before, want, "materials")


# ------------------------------------------------------------- 7. sizes and tiles

@functools.lru_cache(None)
def dump_np_lit(w, h):
    G = dump_scene()
    cam = N.camera(w, h)  # the default view, as Camera.default
    S = N.prepare(G[2], G[3], cam)
    out = LR.lit_composite(S, cam, [N.IDENT, dump_xform("near")], L3)
    for a in out[:4]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("w,h", [(1, 1), (7, 130), (33, 9)])
@pytest.mark.parametrize("tile_order", [0, 1])
def test_partial_units_and_bands(w, h, tile_order):
    want = dump_np_lit(w, h)
    X = dump_xform("near")
    with scene("dump", w, h, tile_order=tile_order) as base, scene("dump", w, h, tile_order=tile_order) as layer:
        cams = (base.cam, layer.cam)
        set_lights(cams, L3)
        t = Targets(w * h).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=NTRI_DUMP)
        before = t.read()
        marked, got = lit(t, cams, (None, X), (0, NTRI_DUMP))
        check_lit(marked, got, before, want, (w, h, tile_order))


@pytest.mark.parametrize("nranks", [2, 3])
def test_tiles(nranks):
    w, h = 33, 19
    want = dump_np_lit(w, h)
    assert (want[3] > 0).sum() >= 10
    X = dump_xform("near")
    npk = R.packed_pixels(w, h, nranks)
    rows = np.arange(h)
    full = np.full((h, w), 0xEE, np.uint32)
    fullm = np.full((h, w), 0xEE, np.uint32)
    with scene("dump", w, h) as base, scene("dump", w, h) as layer:
        cams = (base.cam, layer.cam)
        set_lights(cams, L3)
        for r in range(nranks):
            tile = (nranks, r)
            mine = rows[(rows // 8) % nranks == r]
            other = np.setdiff1d(rows, mine)
            # packed: slot j of rank r is band r + j * nranks, 8 rows each; the planes'
            # slots beyond the rank's pixels keep their poison
            t = Targets(npk).clear(base.cam, tile=tile).over(base.cam, tile=tile)
            t.over(layer.cam, xform=X, hit_base=NTRI_DUMP, tile=tile)
            before = t.read()
            marked, pk = lit(t, cams, (None, X), (0, NTRI_DUMP), tile=tile)
            assert_same(pk[1:], before[1:], "packed hit and planes")
            sel = (mine // 8 // nranks) * 8 + mine % 8
            full[mine] = pk[0].reshape(npk // w, w)[sel]
            fullm[mine] = marked.reshape(npk // w, w)[sel] >> 24
            # at the frame rows of a w*h buffer; the other ranks' rows hold poison
            t = Targets(w * h).plain(base.cam, flags=FRAME_OUT, tile=tile)
            t.over(layer.cam, xform=X, hit_base=NTRI_DUMP, flags=FRAME_OUT, tile=tile)
            before = t.read()
            marked, fo = lit(t, cams, (None, X), (0, NTRI_DUMP), order=(1, 0), flags=FRAME_OUT, tile=tile)
            assert_same(fo[1:], before[1:], "frame-out hit and planes")
            assert (fo[0].reshape(h, w)[mine] == want[0].reshape(h, w)[mine]).all()
            assert ((marked >> 24).reshape(h, w)[mine] == want[3].reshape(h, w)[mine]).all()
            assert (fo[0].reshape(h, w)[other] == POISON).all() and (fo[1].reshape(h, w)[other] == -9).all()
            assert (marked.reshape(h, w)[other] == POISON).all()
    assert (full.reshape(-1) == want[0]).all() and (fullm.reshape(-1) == want[3]).all()


def test_pool_cap_89():
    want = dump_lit("far")
    X = dump_xform("far")
    with scene("dump", W, Hh) as base, scene("dump", W, Hh) as layer:
        cams = (base.cam, layer.cam)
        set_lights(cams, L3)
        set_all(cams, _lib.RT_OPT_POOL_CAP, 89)
        t = Targets(W * Hh).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=NTRI_DUMP)
        before = t.read()
        marked, got = lit(t, cams, (None, X), (0, NTRI_DUMP))
        check_lit(marked, got, before, want, "pool cap 89")


def test_split_field_tree_as_the_occluder():
    (v, f), trees = SY.tree_variants()
    X = H.rot_y(0.0, (0.01, -0.005, 0.02))
    w, h = SY.W, SY.H_
    with live(SY.SynthScene(v, f, w, h), SY.SynthScene(v, f, w, h, nodes=trees["inflated_split"])) as (base, occ):
        cam = base.np_camera()
        Ss = [N.prepare(sc.pts, N.nodes_from_array(sc.onodes), cam) for sc in (base, occ)]
        want = LR.lit_composite(Ss, cam, [N.IDENT, np.asarray(X, F)], L3)
        assert want[4]["by"][1].any()
        cams = (base.cam, occ.cam)
        ntri = len(base.pts)
        set_lights(cams, L3)
        t = Targets(w * h).clear(base.cam).over(base.cam).over(occ.cam, xform=X, hit_base=ntri)
        before = t.read()
        assert_same(before[1:], want[1:3])
        marked, got = lit(t, cams, (None, X), (0, ntri), order=(1, 0))
        check_lit(marked, got, before, want, "split fields")


# ------------------------------------------------- 8. the old paths ignore the list

def test_old_paths_ignore_the_list():
    want = dump_want("near")
    X = dump_xform("near")
    oargb, ohit, _ = H.oracle_render("dump", W, Hh, 0, shadow=True)
    with scene("dump", W, Hh) as base, scene("dump", W, Hh) as layer:
        set_lights((base.cam, layer.cam), L4)
        argb, hit, _ = base.render(0, shadow=True)
        assert (argb == oargb).all() and (hit == ohit).all()
        t = Targets(W * Hh).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=NTRI_DUMP)
        shadow(t, base.cam)
        shadow(t, layer.cam, xform=X, hit_base=NTRI_DUMP)
        assert_same(t.read(), want[:3], "rt_shadow_over after set_lights")


# ------------------------------------------------------------ 9. caller-owned planes

def test_nan_depth_occludes_nothing():
    want = dump_lit("near")
    X = dump_xform("near")
    j = int(np.nonzero(want[3] == 7)[0][0])  # every light occluded
    with scene("dump", W, Hh) as base, scene("dump", W, Hh) as layer:
        cams = (base.cam, layer.cam)
        set_lights(cams, L3)
        S, cam, _, _ = dump_scene()
        for bits in (POISON, 0x7F800000, 0xFF800000, 0xFFFFFFFF):  # NaNs and the infinities
            t = Targets(W * Hh).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=NTRI_DUMP)
            t.planes[j] = bits - (1 << 32) if bits >= 1 << 31 else bits
            before = t.read()
            marked, got = lit(t, cams, (None, X), (0, NTRI_DUMP))
            assert base.cam.device_error() == 0 and layer.cam.device_error() == 0
            assert_same(got[1:], before[1:])
            keep = np.arange(W * Hh) != j
            assert (marked[j] >> 24) == 0 and ((marked >> 24)[keep] == want[3][keep]).all(), hex(bits)
            pl = before[2].view(F)
            unlit = LR.phong_lights(pl[1:4, j], pl[4:7, j], N.primary_ray(cam, j % W, j // W), pl[7:10, j], L3, 0)
            assert got[0][j] == unlit != 0 and (got[0][keep] == want[0][keep]).all()


def test_any_plane_bits_terminate():
    """The planes are the caller's data: random bit patterns in all ten end
    with device error 0, store nothing outside hit pixels, and leave a zero
    top byte at every hit pixel after the shading."""
    import torch
    X = dump_xform("near")
    n = W * Hh
    with scene("dump", W, Hh) as base, scene("dump", W, Hh) as layer:
        cams = (base.cam, layer.cam)
        set_lights(cams, L4)
        t = Targets(n).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=NTRI_DUMP)
        g = torch.Generator(device="cpu").manual_seed(11)
        t.planes[:] = torch.randint(-2**31, 2**31 - 1, (10 * n,), generator=g, dtype=torch.int64).to(torch.int32).cuda()
        before = t.read()
        marked, got = lit(t, cams, (None, X), (0, NTRI_DUMP))
        assert base.cam.device_error() == 0 and layer.cam.device_error() == 0
    assert_same(got[1:], before[1:])
    miss = before[1] < 0
    assert (marked[miss] == before[0][miss]).all() and (got[0][miss] == before[0][miss]).all()
    assert ((marked & 0xFFFFFF) == (before[0] & 0xFFFFFF)).all() and ((marked >> 24) < 16).all()
    assert ((got[0][~miss] >> 24) == 0).all()


# ------------------------------------------------------------------- 10. contract

def test_error_contract():
    import torch
    n = W * Hh
    L = _lib.lib()
    INVALID, STATE = -1, -5
    xf = R.Quaternion().xform()
    with scene("dump", W, Hh) as s:
        cam = s.cam
        t = Targets(n)
        a, hp = _lib.ptr(t.argb), _lib.ptr(t.hit)
        lo = lambda flags=0, base=0, tile=None, argb=a, hit=hp, c=cam._h: L.rt_light_over(  # noqa: E731
            c, _lib.ptr(xf), flags, tile, argb, hit, base, None)
        sl = lambda flags=0, tile=None, argb=a, hit=hp, c=cam._h: L.rt_shade_lights(  # noqa: E731
            c, flags, tile, argb, hit, None)
        # the list: 1..8 finite lights, else unchanged
        good = np.array(L3, F)
        cam.set_lights(good)
        bad = good.copy()
        bad[1, 2] = np.inf
        nan = good.copy()
        nan[2, 3] = np.nan
        nine = np.tile(good[:1], (9, 1))
        for arr, cnt in ((good, 0), (good, 9), (good, -1), (bad, 3), (nan, 3), (nine, 9)):
            assert L.rt_camera_set_lights(cam._h, _lib.ptr(arr), cnt) == INVALID
        assert L.rt_camera_set_lights(cam._h, None, 1) == INVALID and L.rt_camera_set_lights(None, _lib.ptr(good), 1) == INVALID
        assert (cam.lights == good).all()
        cam.set_lights(np.tile(good[:1], (8, 1)))
        assert cam.lights.shape == (8, 4)
        cam.set_lights(good)
        # own planes, never filled
        for f in (lo, sl):
            assert f() == STATE and f(argb=None, hit=None) == STATE
        cam.targets()                                                # allocating them fills nothing
        assert lo() == STATE and sl() == STATE
        t.bind(cam)
        for flags in (1, 4, 16, 32, 64, 1 << 31, 2 | 4):
            assert lo(flags) == INVALID, flags
        for flags in (1, 2, 4, 16, 32, 1 << 31):
            assert sl(flags) == INVALID, flags
        assert lo(base=-1) == INVALID
        for f in (lo, sl):
            assert f(tile=C.byref(_lib.RtTile(2, 2))) == INVALID
            assert f(hit=None) == INVALID                            # the owner is needed
            assert f(c=None) == INVALID
        cam.set_option(_lib.RT_OPT_KERNEL, 2)
        assert lo() == INVALID
        cam.set_aov(t.planes.view(torch.float32), n - 1)
        assert sl() == INVALID and b"stride" in L.rt_last_error_string()
        cam.set_option(_lib.RT_OPT_KERNEL, 3)
        assert lo() == INVALID and b"stride" in L.rt_last_error_string()
        t.bind(cam)
        pts = H.mesh("dump")[0]
        bare = R.Trixel(len(pts), pts)                               # a scene without a tree
        cam2 = R.Camera.default(W, Hh)
        obj2 = R.Object(bare)
        try:
            cam2.add_object(obj2)
            t.bind(cam2)
            assert lo(c=cam2._h) == STATE
        finally:
            for x in (cam2, obj2.motion, bare):
                x.close()
        argb, hit, planes = t.read()
        assert (argb == POISON).all() and (hit == -9).all() and (planes == POISON).all()  # nothing was launched
        # the accepted flags pass, and a frame of misses gets no store
        t.bind(cam)
        t.clear(cam)
        before = t.read()
        assert lo(COUNT) == 0 and lo(FRAME_OUT) == 0 and sl() == 0 and sl(FRAME_OUT) == 0
        assert_same(t.read(), before)
        # rt_shade_lights needs no tree and no kernel 3
        cam.set_option(_lib.RT_OPT_KERNEL, 2)
        assert sl() == 0
        cam.set_option(_lib.RT_OPT_KERNEL, 3)


# ------------------------------------------------------------------ 11. end to end

LIGHTS_ARG = "2,2,2,1;-2,2,2,0.5;0.5,-2,-1,2"


def moved_light_layers_frame():
    """obj1.render; obj2.render; light_layers; color_pixels with the fixture's
    moved pose, through the Python classes (the list set before the layer is
    added and again after)."""
    with scene("dump", W, Hh) as s:
        obj2 = R.Object(s.trixel)
        try:
            s.cam.set_lights(L2)
            s.cam.add_layer(obj2)
            for layer in s.cam._layers.values():
                assert (layer.lights == np.array(L2, F)).all()
            s.cam.set_lights(L3)
            obj2.quat.rot_m = dump_xform("moved").reshape(3, 4)
            for _ in range(2):
                s.obj.render(s.cam)
                obj2.render(s.cam)
                s.cam.light_layers()
                s.cam.color_pixels()
            for layer in s.cam._layers.values():
                assert layer.device_error() == 0 and (layer.lights == np.array(L3, F)).all()
            return s.cam.h_color.copy(), s.cam.h_rmi.copy()
        finally:
            if obj2.motion is not None:
                obj2.motion.close()


def test_light_layers_end_to_end():
    want = dump_lit("moved")
    argb, hit = moved_light_layers_frame()
    assert (hit == want[1]).all() and (argb == want[0]).all()
    assert len(np.unique(argb[hit >= 0])) > 20


def test_headless_lights(tmp_path):
    """tools/rt_headless --over KEYS --lights ...: Camera::set_lights and
    light_layers in the facade, with the fixture's moved pose as key ticks."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tools", "rt_headless")
    assert os.path.exists(exe), "tools/rt_headless is not built (python -m cpp_cuda_raytracer_dev_amd.build --driver)"
    ppm = tmp_path / "frame.ppm"
    r = subprocess.run([exe, os.path.join(root, "tests", "golden", "ply", "dump.ply"), str(scenes.FIXTURE_MODES["dump"]),
                        str(W), str(Hh), "2", str(ppm), "--over", "RW+QR", "--lights", LIGHTS_ARG],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rgb = np.frombuffer(ppm.read_bytes()[-3 * W * Hh:], np.uint8).reshape(Hh, W, 3)[::-1].astype(np.uint32)
    got = (rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2]).reshape(-1)
    assert (got == dump_lit("moved")[0]).all()
    assert (got == moved_light_layers_frame()[0]).all()
