#!/usr/bin/env python3
"""Recover vertex colours: a small grid mesh without a UV atlas carries a `diffuse` BSDF over a `mesh_attribute` texture (src/textures/mesh_attribute.cpp) that reads the
mesh's 'vertex_color' attribute, and random colours are recovered from one target image with mi.render + Adam -- the gradient of the attribute comes out of the `prb`
adjoint under the shape's own name, '<shape>.vertex_color', in the parameter's (vertices, 3) shape.

    python examples/optimize_vertex_colors.py [iterations]

The loss, the mean colour error and the milliseconds per step (render + backward + update, all on the device) are printed every step."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mitsuba3_amd as mi                                   # noqa: E402


def grid(n):
    """an indexed n x n grid in the plane z = 0: (n + 1)^2 shared vertices, 2 n^2 triangles, no normals, no texcoords"""
    s = np.linspace(-1.0, 1.0, n + 1)
    P = np.stack([np.tile(s, n + 1), np.repeat(s, n + 1), np.zeros((n + 1) ** 2)], 1).astype(np.float32)
    F = []
    for j in range(n):
        for i in range(n):
            v = j * (n + 1) + i
            F += [[v, v + 1, v + n + 2], [v, v + n + 2, v + n + 1]]
    return P, np.asarray(F, np.uint32)


def scene_dict(P, F, colors, res, spp):
    T = mi.ScalarTransform4f
    return {"type": "scene",
            "integrator": {"type": "prb", "max_depth": 3},
            "sensor": {"type": "perspective", "fov": 40, "to_world": T().look_at([0, -1.6, 2.4], [0, 0, 0], [0, 0, 1]),
                       "film": {"type": "hdrfilm", "width": res, "height": res}, "sampler": {"type": "independent", "sample_count": spp}},
            "panel": {"type": "mesh", "faces": F, "positions": P, "attributes": {"vertex_color": colors},
                      "bsdf": {"type": "diffuse", "reflectance": {"type": "mesh_attribute", "name": "vertex_color"}}},
            "light": {"type": "rectangle", "to_world": T().translate([0.4, 0.8, 1.8]).rotate([1, 0, 0], 150).scale([0.7, 0.7, 1.0]),
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [14, 14, 14]}}}}


def main():
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    mi.set_variant("hip_ad_rgb")
    res, spp, n = 128, 32, 12
    P, F = grid(n)
    truth = np.random.default_rng(1).uniform(0.05, 0.95, (len(P), 3)).astype(np.float32)
    target = mi.render(mi.load_dict(scene_dict(P, F, truth, res, 256)), spp=256, seed=1000)
    scene = mi.load_dict(scene_dict(P, F, np.full((len(P), 3), 0.5, np.float32), res, spp))
    params = mi.traverse(scene)
    key = "panel.vertex_color"
    params[key].requires_grad_(True)
    opt = torch.optim.Adam([params[key]], lr=0.03)
    first = None
    for it in range(iterations):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        opt.zero_grad()
        img = mi.render(scene, params, spp=spp, seed=it)
        loss = ((img - target) ** 2).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            params[key].clamp_(0.0, 1.0)
        params.update()
        torch.cuda.synchronize(); ms = 1e3 * (time.perf_counter() - t0)
        value = float(loss.detach()); first = value if first is None else first
        err = float((params[key].detach().cpu() - torch.from_numpy(truth)).abs().mean())
        print("iter %3d  loss %.6f  mean |colour error| %.4f  %.1f ms" % (it, value, err, ms))
    print("loss: %.6f -> %.6f" % (first, value))


if __name__ == "__main__":
    main()
