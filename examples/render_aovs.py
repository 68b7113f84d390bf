#!/usr/bin/env python3
"""Radiance next to what a denoiser or a reconstruction loop wants with it: the `aov` integrator (src/integrators/aov.cpp) on the Cornell box.
One render() returns the path tracer's image followed by depth, shading normal and albedo per pixel; each is written with the existing image writers.
Usage: python examples/render_aovs.py [output directory] [exr|pfm]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mitsuba3_amd as mi                                     # noqa: E402


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "out"
    ext = sys.argv[2] if len(sys.argv) > 2 else "exr"
    os.makedirs(out_dir, exist_ok=True)
    mi.set_variant("hip_ad_rgb")
    d = mi.cornell_box()
    d["integrator"] = {"type": "aov", "aovs": "depth:depth,normal:sh_normal,albedo:albedo", "image": {"type": "path", "max_depth": 8}}
    scene = mi.load_dict(d)
    img = mi.render(scene, spp=64, seed=0)                     # H x W x (3 + 1 + 3 + 3)
    names = scene.integrator().aov_names()                     # image.R .G .B .A, depth.T, normal.X .Y .Z, albedo.R .G .B
    print("channels:", [n for n in names if not n.endswith(".A")])
    for name, channels in (("image", slice(0, 3)), ("depth", slice(3, 4)), ("normal", slice(4, 7)), ("albedo", slice(7, 10))):
        path = os.path.join(out_dir, "cornell_%s.%s" % (name, ext))
        mi.write_bitmap(path, img[:, :, channels].contiguous())
        print("wrote %s  mean %.4f" % (path, float(img[:, :, channels].mean())))


if __name__ == "__main__":
    main()
