#!/usr/bin/env python3
"""Recovering a projected pattern: the 16 x 12 texels of a `projector`'s irradiance and its `scale` from ONE camera view of the diffuse wall it lights.

    python examples/optimize_projector.py [iterations]

'<emitter>.irradiance.data' and '<emitter>.scale' of a `projector` are differentiable (projector.cpp:136-141): requires_grad on them switches the `prb` integrator's
`light_texel_gradients` on for the backward pass of that mi.render() call.  The render is linear in both, so the problem is a linear least-squares fit seen through
the camera's pixels; texels and scale are only determined up to their product, and the error printed is that of scale * data."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mitsuba3_amd as mi                                   # noqa: E402


def target_pattern(w=16, h=12):
    """a checkerboard with a coloured gradient over it"""
    y, x = np.mgrid[0:h, 0:w]
    check = ((x // 2 + y // 2) % 2).astype(np.float32)
    img = np.stack([0.2 + 0.8 * check * x / (w - 1), 0.2 + 0.8 * check * y / (h - 1), 0.3 + 0.6 * (1 - check)], axis=2)
    return img.astype(np.float32)


def scene_dict(pattern, scale, res=(96, 72), spp=16):
    T = mi.ScalarTransform4f
    return {"type": "scene", "integrator": {"type": "prb", "max_depth": 3},
            "sensor": {"type": "perspective", "fov": 45, "to_world": T().look_at(origin=[1.2, 0.4, 3.0], target=[0, 0, 0], up=[0, 1, 0]),
                       "film": {"type": "hdrfilm", "width": res[0], "height": res[1], "rfilter": {"type": "gaussian"}},
                       "sampler": {"type": "independent", "sample_count": spp}},
            "wall": {"type": "rectangle", "to_world": T().scale([1.6, 1.2, 1.0]), "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.8, 0.8, 0.8]}}},
            "floor": {"type": "rectangle", "to_world": T().translate([0, -1.2, 1.0]).rotate([1, 0, 0], -90).scale([1.6, 1.0, 1.0]), "bsdf": {"type": "diffuse"}},
            "projector": {"type": "projector", "irradiance": {"type": "bitmap", "data": np.asarray(pattern, np.float32), "raw": True, "wrap_mode": "clamp"},
                          "scale": float(scale), "fov": 50.0, "to_world": T().look_at(origin=[-0.6, 0.2, 2.5], target=[0, 0, 0], up=[0, 1, 0])}}


def main():
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    mi.set_variant("hip_ad_rgb")
    truth, true_scale = target_pattern(), 3.0
    reference = mi.render(mi.load_dict(scene_dict(truth, true_scale)), spp=64, seed=1000).detach()

    scene = mi.load_dict(scene_dict(np.full_like(truth, 0.5), 1.0))
    params = mi.traverse(scene)
    keys = ["projector.irradiance.data", "projector.scale"]
    for k in keys:
        params[k].requires_grad_()
    opt = torch.optim.Adam([params[k] for k in keys], lr=0.05)
    want = torch.as_tensor(truth * true_scale)
    for it in range(iterations):
        opt.zero_grad()
        image = mi.render(scene, params, spp=16, seed=it)
        loss = ((image - reference) ** 2).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            params[keys[0]].clamp_(min=0.0)
        params.update()
        if it % 5 == 0 or it == iterations - 1:
            have = (params[keys[0]] * params[keys[1]]).detach().cpu()
            err = float(((have - want) ** 2).mean().sqrt() / (want ** 2).mean().sqrt())
            print("iteration %3d  loss %.6f  scale %.3f  relative error of scale * data %.3f" % (it, float(loss.detach()), float(params[keys[1]].detach()), err))


if __name__ == "__main__":
    main()
