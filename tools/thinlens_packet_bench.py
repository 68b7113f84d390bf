#!/usr/bin/env python3
"""Does the wave-shared packet descent of the camera rays still pay through a thin lens?  The bench frame (instanced1m, `path`) through a `thinlens` sensor with a small
and a large aperture -- and through the pinhole camera for scale -- with packet tracing forced on and forced off.  At >= 64 spp a wave holds the 64 rays of one pixel;
through a lens their origins are spread over the aperture, so the packet's bounds are wider than a pinhole's.  Timed with HIP events on the current stream: warm-up
frames, then `--repeats` timed frames per setting, the settings interleaved twice; medians and one JSON line are printed.

Usage: python tools/thinlens_packet_bench.py [--res 512] [--spp 256] [--warmup 2] [--repeats 5] [--small 0.005] [--large 0.2] [--focus 3.9]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", type=float, default=0.005)
    ap.add_argument("--large", type=float, default=0.2)
    ap.add_argument("--focus", type=float, default=3.9)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import mitsuba3_amd as mi
    mi.set_variant("hip_ad_rgb")
    res, spp = args.res, args.spp
    scenes = {}
    for name, radius in (("pinhole", None), ("small", args.small), ("large", args.large)):
        d = mi.instanced_spheres_scene(width=res, height=res, spp=spp, grid=10, n_u=100, n_v=50, max_depth=args.max_depth)
        if radius is not None:
            s = d["sensor"]
            s["type"] = "thinlens"; s["aperture_radius"] = radius; s["focus_distance"] = args.focus
            for k in ("principal_point_offset_x", "principal_point_offset_y"):
                s.pop(k, None)
        scenes[name] = mi.load_dict(d)
    integ = {mode: mi.load_dict({"type": "path", "max_depth": args.max_depth, "packet_tracing": mode == "on"}) for mode in ("on", "off")}

    def timed(scene, it):
        for _ in range(args.warmup):
            it.render(scene, seed=0, spp=spp, evaluate=False)
        torch.cuda.synchronize()
        ms = []
        for k in range(args.repeats):
            a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
            a.record(); it.render(scene, seed=k, spp=spp, evaluate=False); b.record(); b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    out = {"res": res, "spp": spp, "max_depth": args.max_depth, "small": args.small, "large": args.large, "focus": args.focus, "device": torch.cuda.get_device_name(0)}
    rounds = {(n, m): [] for n in scenes for m in integ}
    for _ in range(2):
        for (n, m) in rounds:
            rounds[(n, m)] += timed(scenes[n], integ[m])
    paths = res * res * spp
    for (n, m), ms in rounds.items():
        med = float(np.median(ms))
        out["%s_packets_%s" % (n, m)] = {"median_ms": med, "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "mpaths_per_s": paths / med / 1e3}
        print("%-8s packets %-3s median %8.3f ms  (min %.3f, max %.3f)  %7.1f Mpaths/s" % (n, m, med, np.min(ms), np.max(ms), paths / med / 1e3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
