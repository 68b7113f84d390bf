#!/usr/bin/env python3
"""A leaf card: one rectangle carries `mask(twosided(diffuse(bitmap)))` (src/bsdfs/mask.cpp) -- a one-channel opacity bitmap cuts the leaf's outline and a few holes
out of it, a colour bitmap paints both of its sides -- in front of a Cornell box whose back wall is taken away, rendered with `path` onto an `rgba` film.

    python examples/render_cutout.py [output.exr] [spp]

The alpha channel is the share of valid camera samples: 1 on the walls, the boxes and the leaf, 0 where a ray leaves through the missing back wall -- also when it
went through the card's cut-outs first, because a null interaction does not make a sample valid (path.cpp:307-308).  The script prints the range and the mean of
the alpha channel."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mitsuba3_amd as mi                                   # noqa: E402


def leaf_maps(n=64):
    """(opacity n x n x 1 of zeros and ones, colour n x n x 3): a pointed leaf with a midrib and three holes"""
    v, u = (np.mgrid[0:n, 0:n] + 0.5) / n
    x, y = 2 * u - 1, 2 * v - 1
    half_width = 0.62 * np.sqrt(np.clip(1 - y * y, 0, 1)) * (1 - 0.35 * y)
    inside = np.abs(x) < half_width
    for cx, cy, r in ((-0.25, -0.3, 0.12), (0.22, 0.05, 0.1), (-0.1, 0.45, 0.08)):
        inside &= (x - cx) ** 2 + (y - cy) ** 2 > r * r
    rib = np.exp(-(x / 0.04) ** 2) + 0.6 * np.exp(-((np.abs(x) - 0.5 * (y + 1)) / 0.05) ** 2)
    green = np.stack([0.12 + 0.25 * rib, 0.45 + 0.25 * rib, 0.08 + 0.1 * rib], 2)
    return inside.astype(np.float32)[:, :, None], np.clip(green, 0, 1).astype(np.float32)


def scene_dict(res, spp):
    T = mi.ScalarTransform4f
    opacity, colour = leaf_maps()
    d = mi.cornell_box()
    d["sensor"]["film"].update({"width": res, "height": res, "pixel_format": "rgba"})
    d["sensor"]["sampler"] = {"type": "independent", "sample_count": spp}
    d.pop("back")
    d["leaf"] = {"type": "mask", "opacity": {"type": "bitmap", "data": opacity, "raw": True, "filter_type": "nearest"},
                 "material": {"type": "twosided", "paint": {"type": "diffuse", "reflectance": {"type": "bitmap", "data": colour, "raw": True}}}}
    d["card"] = {"type": "rectangle", "to_world": T().translate([0.0, 0.15, 0.75]).rotate([0, 1, 0], 20).scale([0.45, 0.55, 1.0]), "bsdf": {"type": "ref", "id": "leaf"}}
    return d, opacity


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "cutout.exr"
    spp = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    mi.set_variant("hip_ad_rgb")
    d, opacity = scene_dict(256, spp)
    img = mi.render(mi.load_dict(d), spp=spp, seed=0).cpu().numpy()
    assert img.shape[2] == 4
    mi.Bitmap(np.ascontiguousarray(img, np.float32)).write(out)
    alpha = img[..., 3]
    print("wrote %s: %d x %d RGBA, alpha in [%.3f, %.3f], mean alpha %.3f (mean opacity of the leaf bitmap %.3f)" % (out, img.shape[1], img.shape[0], alpha.min(), alpha.max(), alpha.mean(), opacity.mean()))


if __name__ == "__main__":
    main()
