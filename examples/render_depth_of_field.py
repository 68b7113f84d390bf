"""Depth of field with the `thinlens` sensor: the Cornell box at two focus distances -- on the front face of the tall block, and on the back wall -- written as EXR.

Usage: python examples/render_depth_of_field.py [--res 256] [--spp 256] [--aperture 0.12] [--out .]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--aperture", type=float, default=0.12)
    ap.add_argument("--out", default=".")
    args = ap.parse_args()
    import mitsuba3_amd as mi
    mi.set_variant("hip_ad_rgb")
    d = mi.cornell_box()
    cam = d["sensor"]
    cam["type"] = "thinlens"                      # the box's own camera: same pose, same field of view
    cam["aperture_radius"] = args.aperture
    cam["film"]["width"] = args.res; cam["film"]["height"] = args.res
    for name, focus in (("near", 3.6), ("far", 4.9)):          # the camera stands 3.9 in front of the box's centre; the back wall is at z = -1
        cam["focus_distance"] = focus
        scene = mi.load_dict(d)
        sensor = scene.sensors()[0]
        assert sensor.needs_aperture_sample() and sensor.focus_distance() == focus
        img = mi.render(scene, spp=args.spp, seed=0)
        path = os.path.join(args.out, "cornell_focus_%s.exr" % name)
        mi.write_bitmap(path, img)
        print("focus distance %.2f -> %s" % (focus, path))
    # the focus can also be pulled on a loaded scene
    params = mi.traverse(scene)
    import torch
    params["sensor.focus_distance"] = torch.tensor([4.2]); params.update()
    mi.write_bitmap(os.path.join(args.out, "cornell_focus_pulled.exr"), mi.render(scene, spp=args.spp, seed=0))


if __name__ == "__main__":
    main()
