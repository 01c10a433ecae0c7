"""Regenerate tests/golden/aov_small.npz: the per-pixel hit planes
(RT_FLAG_WRITE_AOV: d, pnt, norm, rad of the nearest hit, the reference's
Camera::pixel_memory, TD/Camera.h:50-59) of five small frames, from the
independent numpy restatement (oracle/np_oracle.py) alone.

Per key K the file holds K_aov [10, h, w] float32 (planes d, pnt.xyz,
norm.xyz, rad.rgb; a miss is d = 400 -- init_cam_mem_cuda, TD/Camera.cu:109 --
and zeros), K_hit [h, w] int64, K_argb [h, w] uint32, K_xform [12] and
K_view [2, 3] (camera position and look-at point).
tests/test_aov_cpu.py ties the planes to the C oracle (orc_phong of them is
its frame); tests/test_gpu_aov.py compares the library's with them bit for bit.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from cpp_cuda_raytracer_dev_amd import scenes  # noqa: E402
from oracle import motion as M, np_oracle as N  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "aov_small.npz")
MISS_D = np.float32(400.0)
# The default view (scenes.view) has the 16 x 16 `tester` sheet cover every
# pixel, and scenes has no other view of it: its frames look at it from
# further back and off its axis, so that they hold hits and misses (and few
# enough hits to keep the file small: float planes do not compress).
VIEWS = {"dump": scenes.view("dump"), "tester": {"pos": (4.0, 3.0, -70.0), "look_at": (0.0, 0.1, 0.0)}}
# (scene, w, h, mode, moved pose); tester 33x9: a partial band and a partial 8-pixel group
CASES = [("dump", 40, 24, 0, False), ("dump", 40, 24, 0, True), ("tester", 48, 27, 0, False),
         ("tester", 48, 27, 1, False), ("tester", 33, 9, 0, False)]
MOVED_TICKS = (M.KEY_R, M.KEY_W | M.KEY_Q, M.KEY_R)


def key_of(scene, w, h, mode, moved):
    return f"{scene}_{w}x{h}_m{mode}_{'moved' if moved else 'ident'}"


def camera(scene, w, h):
    v = VIEWS[scene]
    return N.camera(w, h, pos=v["pos"], la=v["look_at"])


def moved_xform(scene, w, h):
    """The object transform after the key ticks R, W|Q, R (oracle/motion.py):
    a rotation and an offset, both non-trivial."""
    cam = camera(scene, w, h)
    m = M.Motion(cam["pos"], cam["n"], cam["u"])
    for keys in MOVED_TICKS:
        m.tick(keys)
    return m.xform()


_scene_cache = {}


def _scene(scene):
    if scene not in _scene_cache:
        v, a, ix = scenes.fixture_mesh(scene)
        pts, boxes = N.assemble(v, a, ix)
        _scene_cache[scene] = (pts, N.build_kd(boxes))
    return _scene_cache[scene]


def planes(scene, w, h, mode, moved, step=1):
    """-> (aov [10, h, w] f32, hit [h, w] i64, argb [h, w] u32, xform [12]);
    step > 1 traces every step-th pixel only (the others stay zero)."""
    pts, nodes = _scene(scene)
    cam = camera(scene, w, h)
    S = N.prepare(pts, nodes if mode == 0 else None, cam)
    X = moved_xform(scene, w, h) if moved else N.IDENT.copy()
    aov = np.zeros((10, h, w), np.float32)
    hit = np.zeros((h, w), np.int64)
    argb = np.zeros((h, w), np.uint32)
    with np.errstate(all="ignore"):
        for i in range(0, w * h, step):
            iy, ix = divmod(i, w)
            rmd = N.primary_ray(cam, ix, iy)
            if mode == 0:
                rmi, d, out, _ = N.trace_kd(S, X, rmd)
            else:
                rmi, d, out = N.trace_flat(S, rmd)
            hit[iy, ix] = rmi
            if rmi >= 0:
                aov[:, iy, ix] = [d, *out[0], *out[1], *N.RAD]
                argb[iy, ix] = N.phong(out[0], out[1], rmd, N.RAD)
            else:
                aov[0, iy, ix] = MISS_D
                argb[iy, ix] = N.BG
    return aov, hit, argb, X


def main():
    out = {}
    for case in CASES:
        k = key_of(*case)
        aov, hit, argb, X = planes(*case)
        nhit = int((hit >= 0).sum())
        print(k, "hit", nhit, "miss", hit.size - nhit, flush=True)
        # a frame without both kinds of pixel checks half of nothing:
        # choose another view from scenes.view then
        assert nhit >= 20 and hit.size - nhit >= 20, k
        out[k + "_aov"], out[k + "_hit"], out[k + "_argb"], out[k + "_xform"] = aov, hit, argb, X
        out[k + "_view"] = np.array([VIEWS[case[0]]["pos"], VIEWS[case[0]]["look_at"]], np.float32)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
