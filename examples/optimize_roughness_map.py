#!/usr/bin/env python3
"""Recover a spatially varying roughness: a lit plate carries a `roughconductor` whose `alpha` is a 16 x 16 bitmap (roughconductor.cpp:195-198: alpha is a texture).
The target is rendered from a map of smooth and rough patches; the map is then recovered from a constant one, from ONE view, with mi.render + Adam -- the gradient with
respect to the texels comes out of the `prb` adjoint: the hand-derived d value / d alpha_u, d alpha_v of the microfacet model at every vertex on the plate, scattered
through the transpose of the bitmap lookup (mi.render switches `bsdf_parameter_gradients` on for a key that requires a gradient).

    python examples/optimize_roughness_map.py [iterations]

The loss at the start and at the end is printed, with the RMS error of the recovered texels."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mitsuba3_amd as mi                                   # noqa: E402


def patches(n=16, cells=4, lo=0.08, hi=0.45):
    """n x n x 1 roughness: a checkerboard of cells x cells smooth and rough patches, softened at the borders"""
    v, u = (np.mgrid[0:n, 0:n] + 0.5) / n
    s = 0.5 + 0.5 * np.sin(np.pi * cells * u) * np.sin(np.pi * cells * v)
    return (lo + (hi - lo) * s).astype(np.float32)[:, :, None]


def scene_dict(texels, res, spp):
    T = mi.ScalarTransform4f
    return {"type": "scene",
            "integrator": {"type": "prb", "max_depth": 3},
            "sensor": {"type": "perspective", "fov": 35, "to_world": T().look_at([0, -2.0, 1.8], [0, 0, 0], [0, 0, 1]),
                       "film": {"type": "hdrfilm", "width": res, "height": res}, "sampler": {"type": "independent", "sample_count": spp}},
            "metal": {"type": "roughconductor", "distribution": "ggx", "eta": {"type": "rgb", "value": [0.2, 0.9, 1.1]}, "k": {"type": "rgb", "value": [3.9, 2.4, 2.2]},
                      "alpha": {"type": "bitmap", "data": texels, "raw": True, "filter_type": "bilinear", "wrap_mode": "clamp"}},
            "plate": {"type": "rectangle", "bsdf": {"type": "ref", "id": "metal"}},
            # a large panel above and behind the plate: every patch mirrors some part of it into the camera, so every texel shapes a highlight
            "panel": {"type": "rectangle", "to_world": T().translate([0, 1.6, 1.6]).rotate([1, 0, 0], 135).scale([2.0, 1.2, 1.0]),
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [6, 6.5, 7]}}},
            "lamp": {"type": "rectangle", "to_world": T().translate([-1.2, -0.4, 1.5]).rotate([0, 1, 0], 140).scale([0.3, 0.3, 1.0]),
                     "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [20, 18, 15]}}}}


def main():
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    mi.set_variant("hip_ad_rgb")
    res, spp, n = 128, 32, 16
    truth = patches(n)
    target = mi.render(mi.load_dict(scene_dict(truth, res, 256)), spp=256, seed=1000)
    scene = mi.load_dict(scene_dict(np.full((n, n, 1), 0.25, np.float32), res, spp))
    params = mi.traverse(scene)
    key = "metal.alpha.data"
    params[key].requires_grad_(True)
    opt = torch.optim.Adam([params[key]], lr=0.01)
    true_a = torch.from_numpy(truth)
    first = None
    for it in range(iterations):
        opt.zero_grad()
        img = mi.render(scene, params, spp=spp, seed=it)
        loss = ((img - target) ** 2).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            params[key].clamp_(0.02, 1.0)          # (a texel at or below 1e-4 is clamped by the microfacet model and receives no gradient)
        params.update()
        value = float(loss.detach()); first = value if first is None else first
        if it % 10 == 0 or it == iterations - 1:
            rms = float(((params[key].detach().cpu() - true_a) ** 2).mean().sqrt())
            print("iter %3d  loss %.6f  RMS alpha error %.4f (the map spans %.2f .. %.2f)" % (it, value, rms, float(truth.min()), float(truth.max())))
    print("loss: %.6f -> %.6f" % (first, value))


if __name__ == "__main__":
    main()
