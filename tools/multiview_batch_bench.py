#!/usr/bin/env python3
"""What the `batch` sensor is for: N views of the bench scene (instanced1m, textured, `prb`) rendered and differentiated per optimisation step, in two ways --
  loop : N consecutive single-sensor render + render_backward pairs (what a multi-view loop does without the batch sensor),
  batch: ONE render + render_backward of a batch sensor holding the same N cameras on a film N times as wide.
Both do the same work: N x res^2 x spp paths forward and backward.  Timed with HIP events on the current stream: warm-up steps first, then `--repeats` timed steps
each; the median and the spread are printed, and one JSON line at the end.

`--loop-only` times the loop alone: on a commit without the `batch` plugin that is the baseline line (`--root DIR`: the checkout whose package is measured).

Usage: python tools/multiview_batch_bench.py [--views 16] [--res 128] [--spp 64] [--warmup 3] [--repeats 10] [--loop-only] [--root DIR]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--loop-only", action="store_true", help="time the single-sensor loop alone (works on a commit without the batch sensor)")
    ap.add_argument("--root", default=ROOT, help="checkout whose mitsuba3_amd package is measured (default: this one)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    import mitsuba3_amd as mi
    mi.set_variant("hip_ad_rgb")
    T = mi.ScalarTransform4f
    n, res, spp = args.views, args.res, args.spp

    def camera(i):
        a = 2.0 * math.pi * i / n
        origin = [0.8 * math.cos(a), 0.4 * math.sin(a), 3.9]
        return {"type": "perspective", "fov_axis": "smaller", "near_clip": 0.001, "far_clip": 100.0, "fov": 39.3077,
                "to_world": T().look_at(origin=origin, target=[0, 0, 0], up=[0, 1, 0])}

    def scene_dict():
        d = mi.instanced_spheres_scene(width=res, height=res, spp=spp, grid=10, n_u=100, n_v=50, max_depth=args.max_depth, textured=True)
        d["integrator"] = {"type": "prb", "max_depth": args.max_depth, "rr_depth": 5, "emitter_gradients": True}
        return d

    film = lambda w: {"type": "hdrfilm", "width": w, "height": res, "rfilter": {"type": "gaussian"}, "pixel_format": "rgb"}
    d = scene_dict(); d.pop("sensor")
    for i in range(n):
        d["view%02d" % i] = dict(camera(i), film=film(res), sampler={"type": "independent", "sample_count": spp})
    loop_scene = mi.load_dict(d)
    batch_scene = None
    d = scene_dict()
    d["sensor"] = {"type": "batch", "film": film(res * n), "sampler": {"type": "independent", "sample_count": spp}}
    for i in range(n):
        d["sensor"]["view%02d" % i] = camera(i)
    if not args.loop_only:
        batch_scene = mi.load_dict(d)
        assert len(batch_scene.sensors()) == 1
    assert len(loop_scene.sensors()) == n

    g_one = torch.ones((res, res, 3), dtype=torch.float32, device="cuda")
    g_all = torch.ones((res, res * n, 3), dtype=torch.float32, device="cuda")

    def loop_step():
        it = loop_scene.integrator()
        for i in range(n):
            it.render(loop_scene, sensor=i, seed=i, spp=spp, evaluate=False)
            it.render_backward(loop_scene, None, g_one, sensor=i, seed=i + 1000, spp=spp)

    def batch_step():
        it = batch_scene.integrator()
        it.render(batch_scene, seed=0, spp=spp, evaluate=False)
        it.render_backward(batch_scene, None, g_all, seed=1000, spp=spp)

    def timed(step):
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
            a.record(); step(); b.record(); b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    out = {"views": n, "res": res, "spp": spp, "max_depth": args.max_depth, "warmup": args.warmup, "repeats": args.repeats,
           "paths_per_step": n * res * res * spp, "device": torch.cuda.get_device_name(0)}
    # interleaved twice, so that a drift of the clocks shows up as a difference between the two rounds instead of between the two methods
    rounds = {"loop": []} if args.loop_only else {"loop": [], "batch": []}
    for _ in range(2):
        rounds["loop"] += timed(loop_step)
        if not args.loop_only:
            rounds["batch"] += timed(batch_step)
    for name, ms in rounds.items():
        out[name + "_ms"] = {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "all": [round(float(x), 3) for x in ms]}
        print("%-5s median %.3f ms  (min %.3f, max %.3f, %d steps)" % (name, np.median(ms), np.min(ms), np.max(ms), len(ms)))
    if not args.loop_only:
        out["ratio_loop_over_batch"] = out["loop_ms"]["median"] / out["batch_ms"]["median"]
        print("loop / batch = %.3f" % out["ratio_loop_over_batch"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
