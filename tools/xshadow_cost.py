#!/usr/bin/env python3
"""Cost of the deferred shadow pass (rt_shadow_over) beside the fused shadow
walk (RT_FLAG_SHADOW), with the method of profiles/r08/over_cost.json: bursts
of `--frames` frames timed on the host around a synchronise, `--rounds`
rounds alternating over the configurations, medians.

    python tools/xshadow_cost.py [--scene knot] [--width 1920 --height 1080] [--out FILE]

Configurations: the plain WRITE_HIT | WRITE_AOV render; the same with
RT_FLAG_SHADOW; the plain render followed by rt_shadow_over of itself; two
objects (plain + over) without and with the two passes."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="knot")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "xshadow_cost.json"))
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

    def plain():
        base.cam.render_into(argb, hit, flags=PLAIN)

    def fused():
        base.cam.render_into(argb, hit, flags=PLAIN | R.RT_FLAG_SHADOW)

    def deferred():
        plain()
        base.cam.shadow_over(argb, hit)

    def two():
        plain()
        layer.cam.render_over(argb, hit, xform=X, hit_base=ntri)

    def two_shadowed():
        two()
        base.cam.shadow_over(argb, hit)
        layer.cam.shadow_over(argb, hit, xform=X, hit_base=ntri)

    configs = {"plain_write_hit_aov": plain, "fused_shadow": fused, "plain_then_shadow_over": deferred,
               "two_objects": two, "two_objects_cross_shadowed": two_shadowed}
    sha, fast_used = {}, {}
    for name, fn in configs.items():  # warm up (the fused walk's order trials included), and the frames
        for _ in range(60):
            fn()
        torch.cuda.synchronize()
        sha[name] = hashlib.sha256(argb.cpu().numpy().tobytes()).hexdigest()
        fast_used[name] = base.cam.get_option(_lib.RT_OPT_FAST_USED)
    hits = int((hit >= 0).sum().item())
    times = {k: [] for k in configs}
    for _ in range(a.rounds):
        for name, fn in configs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.frames):
                fn()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / a.frames)
    res = {k: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}
           for k, v in times.items()}
    med = {k: v["median_ms"] for k, v in res.items()}
    res.update({
        "shadow_over_alone_by_difference_ms": round(med["plain_then_shadow_over"] - med["plain_write_hit_aov"], 5),
        "fused_shadow_walk_by_difference_ms": round(med["fused_shadow"] - med["plain_write_hit_aov"], 5),
        "deferred_excess_over_fused_ms": round(med["plain_then_shadow_over"] - med["fused_shadow"], 5),
        "two_passes_by_difference_ms": round(med["two_objects_cross_shadowed"] - med["two_objects"], 5),
        "deferred_frame_equals_fused_frame": sha["plain_then_shadow_over"] == sha["fused_shadow"],
        "frames_per_burst": a.frames, "rounds": a.rounds, "scene": a.scene, "resolution": [w, h],
        "hit_pixels_two_objects": hits, "layer_offset": [-0.1, -0.1, -0.05],
        "device_err": [base.cam.device_error(), layer.cam.device_error()],
        "shadow_order_in_use": base.cam.get_option(_lib.RT_OPT_SHADOW_ORDER),
        "fast_used_fused": fast_used["fused_shadow"],
        "rays_used": base.cam.get_option(_lib.RT_OPT_RAYS_USED), "build_id": _lib.build_id(),
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
