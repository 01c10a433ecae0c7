"""GPU tests of the deferred shadow pass: rt_shadow_over blackens every hit
pixel of a composite that its camera's object shadows, seeded from the depth
in plane 0, and stores nothing else.  Every expected frame is ``cross_shadow``
(tests/test_xshadow_cpu.py: the numpy oracle's trace_kd / trace_shadow over
``composite``), a committed hash or the C oracle's shadow render, never the
new entry point's own output."""
import ctypes as C
import functools
import hashlib
import os
import subprocess

import numpy as np
import pytest

from cpp_cuda_raytracer_dev_amd import _lib, raytracer as R, scenes
from oracle import np_oracle as N
from tests import helpers as H, synth as SY
from tests.test_gpu_over import KD_CONFIGS, POISON, Targets, assert_same, cfg_id, scene
from tests.test_xshadow_cpu import (NTRI_DUMP, class_counts, cross_shadow, dump_scene, dump_want, dump_xform,
                                    offset_xform, trace_object)

pytestmark = pytest.mark.gpu

AOV = R.RT_FLAG_WRITE_AOV
W, Hh = 40, 24
PASS_CFGS = [(items, order) for items in (1, 2) for order in (0, 1, 2, 3)]


def shadow(t, cam, **kw):
    """The pass of cam's object over the targets t."""
    t.bind(cam)
    cam.shadow_over(t.argb, t.hit, **kw)
    return t


def pass_options(cams, items=None, order=None):
    for cam in cams:
        cam.set_option(_lib.RT_OPT_KERNEL, 3)
        if items is not None:
            cam.set_option(_lib.RT_OPT_ITEMS, items)
        if order is not None:
            cam.set_option(_lib.RT_OPT_SHADOW_ORDER, order)


# ------------------------------- 1. cross-shadowed frames against the numpy reference

@pytest.mark.parametrize("cfg", KD_CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("case", ["near", "far", "moved"])
def test_cross_shadowed_frames(case, cfg):
    want = dump_want(case)
    X = dump_xform(case)
    with scene("dump", W, Hh, **cfg) as base, scene("dump", W, Hh, **cfg) as layer:
        t = Targets(W * Hh).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=NTRI_DUMP)
        before = t.read()
        frame0 = t.argb.clone()
        assert_same(before[1:], want[1:3], (case, cfg, "the composite"))
        cams = (base.cam, layer.cam)
        for items, order in PASS_CFGS:
            pass_options(cams, items, order)
            for first in (0, 1):
                t.argb.copy_(frame0)
                for k in (first, 1 - first):
                    shadow(t, cams[k], xform=(None, X)[k], hit_base=(0, NTRI_DUMP)[k])
                got = t.read()
                assert_same(got, (want[0], before[1], before[2]), (case, cfg, items, order, first))
        assert layer.cam.device_error() == 0


# ------------------------------------------------------------------------ 2. skip_own

@pytest.mark.parametrize("case", ["near", "far", "moved"])
def test_skip_own(case):
    want = dump_want(case)
    X = dump_xform(case)
    SH = R.RT_FLAG_SHADOW
    with scene("dump", W, Hh) as base, scene("dump", W, Hh) as layer:
        t = Targets(W * Hh).clear(base.cam).over(base.cam, flags=SH).over(layer.cam, xform=X, hit_base=NTRI_DUMP, flags=SH)
        own = t.read()
        assert ((own[0] == 0) & (own[1] >= 0)).any()  # the objects' own shadows are in already
        # and the cross-only shadows are not (the moved pose has none: every
        # shadowed pixel there is shadowed by both objects)
        assert (own[0] != want[0]).any() == (case != "moved")
        shadow(t, base.cam, skip_own=True)
        shadow(t, layer.cam, xform=X, hit_base=NTRI_DUMP, skip_own=True)
        assert_same(t.read(), want[:3], case)
        assert layer.cam.device_error() == 0


# ------------------------------- 3. one object at real tiling, against the C oracle

def counters_match(got, want):
    """[0], [1], [4] equal the oracle's; [2] is kernel 3's valid-candidate
    count (>= the DFS's accept events); [3] the render's hit pixels."""
    got, want = [int(x) for x in got], [int(x) for x in want[:5]]
    assert got[2] >= want[2], (got, want)
    got[2] = want[2]
    assert got == want


def self_shadowed(s, count=True):
    """A plain WRITE_HIT | WRITE_AOV render of s's object into its camera's
    own buffers, then the pass of itself."""
    cnt = R.RT_FLAG_COUNT if count else 0
    s.cam.counters()
    s.obj.render(s.cam, flags=R.RT_FLAG_WRITE_HIT | AOV | cnt)
    s.cam.shadow_over(flags=cnt)
    s.cam.color_pixels()
    return s.cam.h_color.copy(), s.cam.h_rmi.copy(), s.cam.counters()


def test_rabbit_960x540_is_the_committed_shadow_frame():
    g = H.golden()
    with scene("rabbit_70k", 960, 540) as s:
        argb, _, cnt = self_shadowed(s)
    assert hashlib.sha256(argb.tobytes()).hexdigest() == str(g["rabbit_70k_960x540_shadow_argb_sha"])
    counters_match(cnt, g["rabbit_70k_960x540_shadow_counters"])


@pytest.mark.parametrize("w,h", [(33, 9), (7, 130), (1, 1)])
@pytest.mark.parametrize("order", [0, 1])
def test_partial_units_and_bands(w, h, order):
    oargb, ohit, ocnt = H.oracle_render("rabbit_70k", w, h, 0, shadow=True)
    with scene("rabbit_70k", w, h, tile_order=order) as s:
        argb, hit, cnt = self_shadowed(s)
        assert (argb == oargb).all() and (hit == ohit).all()
        counters_match(cnt, ocnt)
        s.cam.set_option(_lib.RT_OPT_DEBUG, 16)  # counted walks stop at occluders: the same frame
        argb2, _, cnt2 = self_shadowed(s)
        assert (argb2 == oargb).all() and int(cnt2[0]) <= int(cnt[0])


# --------------------------------------------------------- 4. two rabbits at 320x180

W4, H4, STEP4 = 320, 180, 7


@functools.lru_cache(None)
def rabbit_np():
    """The numpy reference's scene of the rabbit from the oracle's tree, and
    the base object's plain render on every 7th pixel index."""
    pts = H.mesh("rabbit_70k")[0]
    cam = N.camera(W4, H4)
    S = N.prepare(pts, N.nodes_from_array(H.oracle_tree("rabbit_70k")), cam)
    pixels = np.arange(0, W4 * H4, STEP4)
    return S, cam, pixels, trace_object(S, cam, N.IDENT, pixels)


@pytest.mark.parametrize("off,cross", [((-0.1, -0.1, -0.05), 0), ((0.1, 0.1, 0.05), 2)], ids=["near", "far"])
def test_two_rabbits(off, cross):
    S, cam, pixels, base_tr = rabbit_np()
    X = offset_xform(*off)
    want = cross_shadow(S, cam, [N.IDENT, X], pixels=pixels, traced=[base_tr, trace_object(S, cam, X, pixels)])
    counts = class_counts(want[3])
    print("layer pixels shadowed by the base only / both, base pixels by the layer only / both:", counts)
    assert counts[cross] >= 50, counts
    ntri = len(H.mesh("rabbit_70k")[0])
    with scene("rabbit_70k", W4, H4) as base, scene("rabbit_70k", W4, H4) as layer:
        t = Targets(W4 * H4).plain(base.cam).over(layer.cam, xform=X, hit_base=ntri)
        before = t.read()
        shadow(t, layer.cam, xform=X, hit_base=ntri)
        shadow(t, base.cam)
        got = t.read()
        assert layer.cam.device_error() == 0
    assert_same((got[1], got[2]), (before[1], before[2]), "hit and planes")
    assert_same([x[..., pixels] for x in got], want[:3], off)
    black = got[0] == 0
    assert ((before[0][black] == 0) | (got[1][black] >= 0)).all()
    assert (got[0][~black] == before[0][~black]).all()


# ------------------------------------------------------------------------- 5. tiles

@functools.lru_cache(None)
def dump_np(w, h):
    G = dump_scene()
    cam = N.camera(w, h)  # the default view, as Camera.default
    S = N.prepare(G[2], G[3], cam)
    X = dump_xform("near")
    out = cross_shadow(S, cam, [N.IDENT, X])
    for a in out[:3]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("w,h", [(48, 27), (33, 9)])
def test_tiles(w, h, nranks):
    want = dump_np(w, h)
    if (w, h) == (48, 27):
        assert want[3]["by"].any(0).sum() >= 10 and class_counts(want[3])[0] > 0
    X = dump_xform("near")
    npk = R.packed_pixels(w, h, nranks)
    rows = np.arange(h)
    full = np.full((h, w), 0xEE, np.uint32)
    with scene("dump", w, h) as base, scene("dump", w, h) as layer:
        for r in range(nranks):
            tile = (nranks, r)
            mine = rows[(rows // 8) % nranks == r]
            other = np.setdiff1d(rows, mine)
            # packed: slot j of rank r is band r + j * nranks, 8 rows each
            t = Targets(npk).clear(base.cam, tile=tile).over(base.cam, tile=tile)
            t.over(layer.cam, xform=X, hit_base=NTRI_DUMP, tile=tile)
            before = t.read()
            shadow(t, base.cam, tile=tile)
            pk = shadow(t, layer.cam, xform=X, hit_base=NTRI_DUMP, tile=tile).read()
            assert_same(pk[1:], before[1:], "packed hit and planes")
            full[mine] = pk[0].reshape(npk // w, w)[(mine // 8 // nranks) * 8 + mine % 8]
            # at the frame rows of a w*h buffer; the other ranks' rows hold poison
            t = Targets(w * h).plain(base.cam, flags=R.RT_FLAG_FRAME_OUT, tile=tile)
            t.over(layer.cam, xform=X, hit_base=NTRI_DUMP, flags=R.RT_FLAG_FRAME_OUT, tile=tile)
            before = t.read()
            shadow(t, layer.cam, xform=X, hit_base=NTRI_DUMP, flags=R.RT_FLAG_FRAME_OUT, tile=tile)
            fo = shadow(t, base.cam, flags=R.RT_FLAG_FRAME_OUT, tile=tile).read()
            assert_same(fo[1:], before[1:], "frame-out hit and planes")
            assert (fo[0].reshape(h, w)[mine] == want[0].reshape(h, w)[mine]).all()
            assert (fo[0].reshape(h, w)[other] == POISON).all() and (fo[1].reshape(h, w)[other] == -9).all()
        assert layer.cam.device_error() == 0
    assert (full.reshape(-1) == want[0]).all()


# --------------------------------------- 6. a hand-made tree with differing split fields

def test_split_field_tree_as_the_occluder():
    (v, f), trees = SY.tree_variants()
    X = H.rot_y(0.0, (0.01, -0.005, 0.02))
    w, h = SY.W, SY.H_
    with SY.SynthScene(v, f, w, h) as base, SY.SynthScene(v, f, w, h, nodes=trees["inflated_split"]) as occ:
        cam = base.np_camera()
        Ss = [N.prepare(sc.pts, N.nodes_from_array(sc.onodes), cam) for sc in (base, occ)]
        want = cross_shadow(Ss, cam, [N.IDENT, X])
        assert want[3]["by"][1].any() and class_counts(want[3])[2] > 0  # the occluder shadows base pixels
        base._gpu()
        occ._gpu()
        ntri = len(base.pts)
        t = Targets(w * h).clear(base.cam).over(base.cam).over(occ.cam, xform=X, hit_base=ntri)
        before = t.read()
        shadow(t, occ.cam, xform=X, hit_base=ntri)
        shadow(t, base.cam)
        got = t.read()
        assert base.cam.device_error() == 0 and occ.cam.device_error() == 0
    assert_same(got, (want[0], before[1], before[2]))
    assert_same(before[1:], want[1:3])


# ------------------------------------------------------------------------ 7. contract

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
        sh = lambda flags=0, base=0, tile=None, argb=a, hit=hp, c=cam._h: L.rt_shadow_over(  # noqa: E731
            c, _lib.ptr(xf), flags, tile, argb, hit, base, 0, None)
        assert sh() == STATE and sh(argb=None, hit=None) == STATE  # own planes, never filled
        cam.targets()                                                # allocating them fills nothing
        assert sh() == STATE
        t.bind(cam)
        for flags in (1, 4, 16, 32, 64, 1 << 31, 2 | 4):
            assert sh(flags) == INVALID, flags
        assert sh(base=-1) == INVALID
        assert sh(tile=C.byref(_lib.RtTile(2, 2))) == INVALID
        assert sh(hit=None) == INVALID                               # the owner is needed
        assert sh(c=None) == INVALID
        cam.set_option(_lib.RT_OPT_KERNEL, 2)
        assert sh() == INVALID
        cam.set_option(_lib.RT_OPT_KERNEL, 3)
        cam.set_aov(t.planes.view(torch.float32), n - 1)
        assert sh() == INVALID and b"stride" in L.rt_last_error_string()
        t.bind(cam)
        pts = H.mesh("dump")[0]
        bare = R.Trixel(len(pts), pts)                               # a scene without a tree
        cam2 = R.Camera.default(W, Hh)
        obj2 = R.Object(bare)
        try:
            cam2.add_object(obj2)
            t.bind(cam2)
            assert sh(c=cam2._h) == STATE
        finally:
            for x in (cam2, obj2.motion, bare):
                x.close()
        argb, hit, planes = t.read()
        assert (argb == POISON).all() and (hit == -9).all() and (planes == POISON).all()  # nothing was launched
        # the accepted flags pass, and a frame of misses gets no store
        t.bind(cam)
        t.clear(cam)
        before = t.read()
        assert sh(R.RT_FLAG_COUNT) == 0 and sh(R.RT_FLAG_FRAME_OUT) == 0
        assert_same(t.read(), before)


def test_nan_depth_pixel_is_left_alone():
    want = dump_want("near")
    X = dump_xform("near")
    j = int(np.nonzero(want[3]["by"].all(0))[0][0])  # shadowed by both objects
    with scene("dump", W, Hh) as base, scene("dump", W, Hh) as layer:
        for bits in (POISON, 0x7F800000, 0xFF800000, 0xFFFFFFFF):  # NaNs and the infinities
            t = Targets(W * Hh).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=NTRI_DUMP)
            t.planes[j] = bits - (1 << 32) if bits >= 1 << 31 else bits
            before = t.read()
            shadow(t, base.cam)
            shadow(t, layer.cam, xform=X, hit_base=NTRI_DUMP)
            got = t.read()
            assert base.cam.device_error() == 0 and layer.cam.device_error() == 0
            assert_same(got[1:], before[1:])
            keep = np.arange(W * Hh) != j
            assert got[0][j] == before[0][j] != 0
            assert (got[0][keep] == want[0][keep]).all()


def test_any_depth_bits_terminate():
    """The depth is the caller's data: random bit patterns in plane 0 end with
    device error 0 and store nothing but zeros at hit pixels."""
    import torch
    X = dump_xform("near")
    with scene("dump", W, Hh) as base, scene("dump", W, Hh) as layer:
        t = Targets(W * Hh).clear(base.cam).over(base.cam).over(layer.cam, xform=X, hit_base=NTRI_DUMP)
        g = torch.Generator(device="cpu").manual_seed(9)
        t.planes[:W * Hh] = torch.randint(-2**31, 2**31 - 1, (W * Hh,), generator=g, dtype=torch.int64).to(torch.int32).cuda()
        before = t.read()
        shadow(t, base.cam)
        shadow(t, layer.cam, xform=X, hit_base=NTRI_DUMP)
        got = t.read()
        assert base.cam.device_error() == 0 and layer.cam.device_error() == 0
    assert_same(got[1:], before[1:])
    changed = got[0] != before[0]
    assert (got[0][changed] == 0).all() and (before[1][changed] >= 0).all()


def moved_layers_frame():
    """obj1.render; obj2.render; shadow_layers; color_pixels with the
    fixture's moved pose, through the Python classes."""
    with scene("dump", W, Hh) as s:
        obj2 = R.Object(s.trixel)
        try:
            s.cam.add_layer(obj2)
            obj2.quat.rot_m = dump_xform("moved").reshape(3, 4)
            for _ in range(2):
                s.obj.render(s.cam)
                obj2.render(s.cam)
                s.cam.shadow_layers()
                s.cam.color_pixels()
            for layer in s.cam._layers.values():
                assert layer.device_error() == 0
            return s.cam.h_color.copy(), s.cam.h_rmi.copy()
        finally:
            if obj2.motion is not None:
                obj2.motion.close()


def test_shadow_layers_end_to_end():
    want = dump_want("moved")
    argb, hit = moved_layers_frame()
    assert (hit == want[1]).all() and (argb == want[0]).all()
    assert ((argb == 0) & (hit >= 0)).sum() == want[3]["by"].any(0).sum() > 0


def test_headless_cross_shadow(tmp_path):
    """tools/rt_headless --over KEYS --cross-shadow: Camera::shadow_layers in
    the facade, with the fixture's moved pose as key ticks."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tools", "rt_headless")
    assert os.path.exists(exe), "tools/rt_headless is not built (python -m cpp_cuda_raytracer_dev_amd.build --driver)"
    ppm = tmp_path / "frame.ppm"
    r = subprocess.run([exe, os.path.join(root, "tests", "golden", "ply", "dump.ply"), str(scenes.FIXTURE_MODES["dump"]),
                        str(W), str(Hh), "2", str(ppm), "--over", "RW+QR", "--cross-shadow"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rgb = np.frombuffer(ppm.read_bytes()[-3 * W * Hh:], np.uint8).reshape(Hh, W, 3)[::-1].astype(np.uint32)
    got = (rgb[..., 0] << 16 | rgb[..., 1] << 8 | rgb[..., 2]).reshape(-1)
    assert (got == dump_want("moved")[0]).all()
    assert (got == moved_layers_frame()[0]).all()
