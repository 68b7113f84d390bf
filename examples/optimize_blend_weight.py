#!/usr/bin/env python3
"""Recover a material mask: a plane blends `diffuse` paint and a `roughconductor` metal by a 32 x 32 weight bitmap (`blendbsdf`, src/bsdfs/blendbsdf.cpp), and the
mask is recovered from a target image with mi.render + Adam -- the gradient of the weight comes out of the `prb` adjoint like the gradient of any bitmap.

    python examples/optimize_blend_weight.py [iterations]

The loss, the mean texel error of the mask and the milliseconds per step (render + backward + update) are printed every step."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mitsuba3_amd as mi                                   # noqa: E402


def scene_dict(mask, res, spp):
    T = mi.ScalarTransform4f
    return {"type": "scene",
            "integrator": {"type": "prb", "max_depth": 3},
            "sensor": {"type": "perspective", "fov": 40, "to_world": T().look_at([0, -1.6, 2.4], [0, 0, 0], [0, 0, 1]),
                       "film": {"type": "hdrfilm", "width": res, "height": res}, "sampler": {"type": "independent", "sample_count": spp}},
            "mat": {"type": "blendbsdf", "weight": {"type": "bitmap", "data": mask, "raw": True},
                    "paint": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.15, 0.35, 0.7]}},
                    "metal": {"type": "roughconductor", "alpha": 0.25, "distribution": "ggx", "specular_reflectance": {"type": "rgb", "value": [0.95, 0.8, 0.5]}}},
            "plane": {"type": "rectangle", "bsdf": {"type": "ref", "id": "mat"}},
            "light": {"type": "rectangle", "to_world": T().translate([0.4, 0.8, 1.8]).rotate([1, 0, 0], 150).scale([0.7, 0.7, 1.0]),
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [14, 14, 14]}}}}


def main():
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    mi.set_variant("hip_ad_rgb")
    res, spp, n = 128, 32, 32
    y, x = np.mgrid[0:n, 0:n]
    truth = (((x - 15.5) ** 2 + (y - 15.5) ** 2 < 100) ^ ((x // 4 + y // 4) % 2 == 0)).astype(np.float32)[:, :, None] * 0.8 + 0.1      # metal where the mask is high
    target = mi.render(mi.load_dict(scene_dict(truth, res, 256)), spp=256, seed=1000)
    scene = mi.load_dict(scene_dict(np.full((n, n, 1), 0.5, np.float32), res, spp))
    params = mi.traverse(scene)
    key = "mat.weight.data"
    params[key].requires_grad_(True)
    opt = torch.optim.Adam([params[key]], lr=0.05)
    first = None
    for it in range(iterations):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        opt.zero_grad()
        img = mi.render(scene, params, spp=spp, seed=it)
        loss = ((img - target) ** 2).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            params[key].clamp_(0.02, 0.98)          # (the weight is clipped to [0, 1] by the BSDF, and has no gradient outside)
        params.update()
        torch.cuda.synchronize(); ms = 1e3 * (time.perf_counter() - t0)
        value = float(loss.detach()); first = value if first is None else first
        err = float((params[key].detach().cpu() - torch.from_numpy(truth)).abs().mean())
        print("iter %3d  loss %.6f  mean |mask error| %.4f  %.1f ms" % (it, value, err, ms))
    print("loss: %.6f -> %.6f" % (first, value))


if __name__ == "__main__":
    main()
