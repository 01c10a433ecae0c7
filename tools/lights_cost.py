#!/usr/bin/env python3
"""Cost of the light list's passes (rt_light_over, rt_shade_lights) beside the
deferred shadow pass (rt_shadow_over), with the method of tools/xshadow_cost.py:
bursts of `--frames` frames timed on the host around a synchronise, `--rounds`
rounds alternating over the configurations, medians.

    python tools/lights_cost.py [--scene knot] [--width 1920 --height 1080] [--out FILE]

Two frames: one object (a plain WRITE_HIT | WRITE_AOV render) and two objects
(that render plus rt_render_over of the same mesh at an offset).  On each: the
render alone; with rt_shadow_over per object; with one-light rt_light_over per
object (the same walks plus a 4-byte load and a conditional store per hit
pixel); with rt_shade_lights alone; and the whole lit frame -- the passes of 1,
2, 4 and 8 lights, then the shading.  A pass's cost is the difference of two
medians.  The frame is restored before every visibility pass by the render
itself, so no pass starts from bits an earlier burst left."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

#: the literal light first, then seven more around the default view's scene
LIGHTS = [(2, 2, 2, 1), (-2, 2, 2, 0.5), (0.5, -2, -1, 2), (2, -1, 0.5, 0.25), (-2, -2, 2, 1), (2, 2, -2, 1),
          (-1, 3, -2, 0.5), (0, 2.5, 0, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="knot")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "lights_cost.json"))
    a = ap.parse_args()
    import torch
    from cpp_cuda_raytracer_dev_amd import _lib, raytracer as R
    from tests import helpers as H
    w, h = a.width, a.height
    n = w * h
    base, layer = H.GpuScene(a.scene, w, h), H.GpuScene(a.scene, w, h)
    ntri = base.trixel.num_trixels
    X = np.array([1, 0, 0, -0.1, 0, 1, 0, -0.1, 0, 0, 1, -0.05], np.float32)
    dev = torch.device("cuda:0")
    argb = torch.zeros(n, dtype=torch.int32, device=dev)
    hit = torch.zeros(n, dtype=torch.int64, device=dev)
    planes = torch.zeros(10 * n, dtype=torch.float32, device=dev)
    for s in (base, layer):
        s.cam.set_aov(planes, n)
    PLAIN = R.RT_FLAG_WRITE_HIT | R.RT_FLAG_WRITE_AOV

    def frame(two):
        base.cam.render_into(argb, hit, flags=PLAIN)
        if two:
            layer.cam.render_over(argb, hit, xform=X, hit_base=ntri)

    def shadowed(two):
        frame(two)
        base.cam.shadow_over(argb, hit)
        if two:
            layer.cam.shadow_over(argb, hit, xform=X, hit_base=ntri)

    def marked(two):
        frame(two)
        base.cam.light_over(argb, hit)
        if two:
            layer.cam.light_over(argb, hit, xform=X, hit_base=ntri)

    def shaded(two):
        frame(two)
        base.cam.shade_lights(argb, hit)

    def lit(two):
        marked(two)
        base.cam.shade_lights(argb, hit)

    res = {}
    for two in (False, True):
        key = "two_objects" if two else "one_object"
        configs = {"render": (frame, 1), "shadow_over": (shadowed, 1), "light_over_1": (marked, 1),
                   "shade_lights_1": (shaded, 1)}
        configs.update({f"lit_{k}": (lit, k) for k in (1, 2, 4, 8)})
        for name, (fn, k) in configs.items():  # warm up
            for s in (base, layer):
                s.cam.set_lights(LIGHTS[:k])
            for _ in range(40):
                fn(two)
        torch.cuda.synchronize()
        hits = int((hit >= 0).sum().item())
        times = {k: [] for k in configs}
        for _ in range(a.rounds):
            for name, (fn, k) in configs.items():
                for s in (base, layer):
                    s.cam.set_lights(LIGHTS[:k])  # synchronises
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.frames):
                    fn(two)
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0) / a.frames)
        r = {k: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}
             for k, v in times.items()}
        med = {k: v["median_ms"] for k, v in r.items()}
        shade = med["shade_lights_1"] - med["render"]
        one = med["light_over_1"] - med["render"]
        r.update({
            "shadow_over_by_difference_ms": round(med["shadow_over"] - med["render"], 5),
            "shadow_over_spread_above_median_ms": round(r["shadow_over"]["max_ms"] - med["shadow_over"], 5),
            "light_over_1_by_difference_ms": round(one, 5),
            "light_over_1_minus_shadow_over_ms": round(med["light_over_1"] - med["shadow_over"], 5),
            "shade_lights_by_difference_ms": round(shade, 5),
            "hit_pixels": hits,
        })
        for k in (1, 2, 4, 8):
            passes = med[f"lit_{k}"] - med["render"] - shade
            r[f"light_over_{k}_passes_by_difference_ms"] = round(passes, 5)
            r[f"light_over_{k}_over_{k}_times_one_light"] = round(passes / (k * one), 4) if one > 0 else None
        res[key] = r
    res.update({
        "frames_per_burst": a.frames, "rounds": a.rounds, "scene": a.scene, "resolution": [w, h],
        "layer_offset": [-0.1, -0.1, -0.05], "lights": LIGHTS,
        "device_err": [base.cam.device_error(), layer.cam.device_error()],
        "shadow_order_in_use": base.cam.get_option(_lib.RT_OPT_SHADOW_ORDER), "build_id": _lib.build_id(),
    })
    for s in (base, layer):
        s.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        json.dump(res, fp, indent=1)
        fp.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
