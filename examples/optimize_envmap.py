#!/usr/bin/env python3
"""Recovering the lighting: a 16 x 8 environment map and its `scale` from ONE rendered view of a diffuse and a rough metal box on a floor.

    python examples/optimize_envmap.py [iterations]

'<emitter>.data' and '<emitter>.scale' of an `envmap` are differentiable (envmap.cpp:203-208): requires_grad on them switches the `prb` integrator's
`envmap_gradients` on for the backward pass of that mi.render() call.  The gradient of `data` comes in the parameter's own layout, H x (W + 2) x 3 -- one halo column
on each side that the emitter refreshes from the opposite edge on every params.update(); the halo columns' gradient is zero, what reaches them is folded onto the real
columns.  Texels and scale are only determined up to their product, and the rows below the horizon barely light this scene (the floor hides them), so the error
printed is that of scale * data over the sky rows."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mitsuba3_amd as mi                                   # noqa: E402


def sky(w=16, h=8):
    """the target: a warm sun low in the sky, a blue gradient above the horizon, a dim brown ground"""
    v = (np.arange(h) + 0.5) / h; u = (np.arange(w) + 0.5) / w
    img = np.zeros((h, w, 3), np.float32)
    img[:] = np.where(v[:, None, None] < 0.5, np.float32([0.25, 0.45, 0.9]) * (0.4 + 1.2 * v[:, None, None]), np.float32([0.2, 0.15, 0.1]))
    img += np.float32([2.0, 1.5, 0.9]) * np.exp(-(((u[None, :] - 0.3) / 0.08) ** 2 + ((v[:, None] - 0.3) / 0.12) ** 2))[:, :, None]
    return img


def scene_dict(image, scale, res=96, spp=32):
    T = mi.ScalarTransform4f
    d = {"type": "scene", "integrator": {"type": "prb", "max_depth": 4},
         "sensor": mi.cornell_box()["sensor"],
         "white": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.7, 0.7]}},
         "metal": {"type": "roughconductor", "alpha": 0.2},
         "floor": {"type": "rectangle", "to_world": T().translate([0.0, -1.0, 0.0]).rotate([1, 0, 0], -90).scale(3.0), "bsdf": {"type": "ref", "id": "white"}},
         "box": {"type": "cube", "to_world": T().translate([-0.5, -0.6, 0.1]).rotate([0, 1, 0], 25).scale(0.4), "bsdf": {"type": "ref", "id": "white"}},
         "rough": {"type": "cube", "to_world": T().translate([0.5, -0.6, -0.1]).rotate([0, 1, 0], -30).scale(0.4), "bsdf": {"type": "ref", "id": "metal"}},
         "env": {"type": "envmap", "bitmap": mi.Bitmap(np.asarray(image, np.float32)), "scale": float(scale)}}
    d["sensor"]["film"]["width"] = res; d["sensor"]["film"]["height"] = res
    d["sensor"]["sampler"]["sample_count"] = spp
    return d


def main():
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 80
    mi.set_variant("hip_ad_rgb")
    spp = 32
    truth, truth_scale = sky(), 1.5
    target = mi.render(mi.load_dict(scene_dict(truth, truth_scale)), spp=256, seed=1000)
    scene = mi.load_dict(scene_dict(np.full_like(truth, 0.5), 1.0))          # start: a uniform grey sky
    params = mi.traverse(scene)
    data = params["env.data"].detach().clone().requires_grad_(True); scale = params["env.scale"].detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [data], "lr": 0.05}, {"params": [scale], "lr": 0.02}])
    want = torch.as_tensor(truth * truth_scale, device=data.device)
    sky_rows = truth.shape[0] // 2
    for it in range(iterations):
        params["env.data"] = data; params["env.scale"] = scale
        params.update()                                                        # refreshes the halo and rebuilds the map's sampling distribution
        opt.zero_grad()
        loss = ((mi.render(scene, params, spp=spp, seed=it) - target) ** 2).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            data.clamp_(min=1e-3); scale.clamp_(min=1e-3)
        err = float(((data[:sky_rows, 1:-1] * scale).detach() - want[:sky_rows]).abs().mean() / want[:sky_rows].abs().mean())
        print("iter %3d  loss %.6f  scale %.3f  relative error of scale * data (sky) %.4f" % (it, float(loss.detach()), float(scale.detach()), err))


if __name__ == "__main__":
    main()
