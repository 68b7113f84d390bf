#!/usr/bin/env python3
"""Multi-view inverse rendering with the `batch` sensor: recover the 32 x 32 albedo texture of the Cornell box's white walls from FOUR views, with ONE mi.render and
one backward pass per step -- the four cameras share a film four times as wide as each view (src/sensors/batch.cpp), so all of them are one wavefront.

    python examples/optimize_multiview.py [iterations]

The loss and the mean texel error are printed every step.  The loss falls to the floor the Monte Carlo noise of a 64 spp render sets (about three quarters of its
starting value here); the texel error falls from 0.27 to about 0.05."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mitsuba3_amd as mi                                   # noqa: E402


def main():
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    mi.set_variant("hip_ad_rgb")
    T = mi.ScalarTransform4f
    res, tex_res, spp = 96, 32, 64          # 64 spp: the Monte Carlo noise of the image stays below the part of the loss the texture explains
    d = mi.textured_cornell_box(res=res, tex_res=tex_res, spp=spp)
    key = "white.reflectance.data"
    i = np.arange(tex_res) * 8 // tex_res
    checker = 0.5 + 0.3 * (2 * ((i[:, None] + i[None, :]) & 1) - 1)
    d["white"]["reflectance"]["data"] = np.repeat(checker[:, :, None], 3, axis=2).astype(np.float32)
    origins = [[0.0, 0.0, 3.9], [0.9, 0.3, 3.4], [-0.9, 0.3, 3.4], [0.0, -0.5, 3.0]]
    d["sensor"] = {"type": "batch", "sampler": {"type": "independent", "sample_count": spp},
                   "film": {"type": "hdrfilm", "width": res * len(origins), "height": res, "rfilter": {"type": "gaussian"}, "pixel_format": "rgb"}}
    for k, o in enumerate(origins):
        d["sensor"]["view%d" % k] = {"type": "perspective", "fov": 45.0, "near_clip": 0.001, "far_clip": 100.0,
                                     "to_world": T().look_at(origin=o, target=[0, 0, 0], up=[0, 1, 0])}
    scene = mi.load_dict(d)
    target = mi.render(scene, spp=256, seed=1000)              # res x (4 res) x 3: the four views side by side
    params = mi.traverse(scene)
    params[key] = torch.full_like(params[key], 0.5).requires_grad_(True)
    params.update()
    opt = torch.optim.Adam([params[key]], lr=0.03)
    first = None
    for it in range(iterations):
        opt.zero_grad()
        img = mi.render(scene, params, spp=spp, seed=it)        # all views, differentiable w.r.t. params[key]
        loss = ((img - target) ** 2).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            params[key].clamp_(0.0, 1.0)
        params.update()
        value = float(loss.detach())
        first = value if first is None else first
        err = float((params[key].detach().cpu() - torch.from_numpy(d["white"]["reflectance"]["data"])).abs().mean())
        print("iter %3d  loss %.6f  mean |texel error| %.4f" % (it, value, err))
    print("loss: %.6f -> %.6f" % (first, value))


if __name__ == "__main__":
    main()
