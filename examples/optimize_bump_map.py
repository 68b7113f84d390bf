#!/usr/bin/env python3
"""Recover a height map: a smooth-shaded mesh WITH vertex normals and texture coordinates -- the case a `normalmap` refuses, because its frame would need per-vertex
tangents -- carries `bumpmap(roughplastic)` (src/bsdfs/bumpmap.cpp) under a point light and an area light.  The target is rendered from a 32 x 32 height map of cosine
bumps; the map is then recovered from the flat one (all zeros) with mi.render + Adam -- the gradient with respect to the texels comes out of the `prb` adjoint: the reverse
sweep through the bump frame, the nested model's directional derivatives and the shadow term, deposited through the transpose of the bitmap's eval_1_grad.

    python examples/optimize_bump_map.py [iterations]

A constant added to the height changes no picture, so the mean is removed after every step.  The loss at the start and at the end is printed, with the RMS error of the
recovered heights."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mitsuba3_amd as mi                                   # noqa: E402


def bumps(n=32, cells=3, depth=0.02):
    """n x n x 1 heights of cells x cells cosine bumps"""
    v, u = (np.mgrid[0:n, 0:n] + 0.5) / n
    return (depth * np.cos(2 * np.pi * cells * u) * np.cos(2 * np.pi * cells * v)).astype(np.float32)[:, :, None]


def dome(k=24, half=1.0, bulge=0.3):
    """a (k + 1)^2 grid bulging upwards, with the bulge's normals and the unit square as texture coordinates"""
    xs = np.linspace(-half, half, k + 1)
    X, Y = np.meshgrid(xs, xs)
    Z = bulge * (1 - (X / half) ** 2) * (1 - (Y / half) ** 2)
    dzx = bulge * (-2 * X / half ** 2) * (1 - (Y / half) ** 2); dzy = bulge * (1 - (X / half) ** 2) * (-2 * Y / half ** 2)
    nrm = np.stack([-dzx, -dzy, np.ones_like(X)], -1).reshape(-1, 3); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    faces = []
    for j in range(k):
        for i in range(k):
            a = j * (k + 1) + i
            faces += [[a, a + 1, a + k + 2], [a, a + k + 2, a + k + 1]]
    return {"type": "mesh", "positions": np.stack([X, Y, Z], -1).reshape(-1, 3).astype(np.float32), "faces": np.array(faces, np.uint32), "normals": nrm.astype(np.float32),
            "texcoords": np.stack([(X + half) / (2 * half), (Y + half) / (2 * half)], -1).reshape(-1, 2).astype(np.float32)}


def scene_dict(texels, res, spp):
    T = mi.ScalarTransform4f
    return {"type": "scene",
            "integrator": {"type": "prb", "max_depth": 3},
            "sensor": {"type": "perspective", "fov": 40, "to_world": T().look_at([0, -1.6, 2.6], [0, 0, 0.1], [0, 0, 1]),
                       "film": {"type": "hdrfilm", "width": res, "height": res}, "sampler": {"type": "independent", "sample_count": spp}},
            "mat": {"type": "bumpmap", "height": {"type": "bitmap", "data": texels, "raw": True},
                    "coating": {"type": "roughplastic", "diffuse_reflectance": {"type": "rgb", "value": [0.25, 0.4, 0.7]}, "alpha": 0.2}},
            "dome": dict(dome(), bsdf={"type": "ref", "id": "mat"}),
            "lamp": {"type": "point", "position": [0.9, 0.6, 1.6], "intensity": {"type": "rgb", "value": [5.0, 4.5, 4.0]}},
            "panel": {"type": "rectangle", "to_world": T().translate([-0.9, 0.5, 1.7]).rotate([0, 1, 0], 145).scale([0.6, 0.6, 1.0]),
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [9, 10, 12]}}}}


def main():
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 80
    mi.set_variant("hip_ad_rgb")
    res, spp, n = 128, 32, 32
    truth = bumps(n)
    target = mi.render(mi.load_dict(scene_dict(truth, res, 256)), spp=256, seed=1000)
    scene = mi.load_dict(scene_dict(np.zeros((n, n, 1), np.float32), res, spp))
    params = mi.traverse(scene)
    key = "mat.nested_texture.data"
    params[key].requires_grad_(True)
    opt = torch.optim.Adam([params[key]], lr=0.002)
    true_h = torch.from_numpy(truth - truth.mean())
    first = None
    for it in range(iterations):
        opt.zero_grad()
        img = mi.render(scene, params, spp=spp, seed=it)
        loss = ((img - target) ** 2).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            params[key] -= params[key].mean()
        params.update()
        value = float(loss.detach()); first = value if first is None else first
        if it % 10 == 0 or it == iterations - 1:
            rms = float(((params[key].detach().cpu() - true_h) ** 2).mean().sqrt())
            print("iter %3d  loss %.6f  RMS height error %.5f (the bumps' amplitude: %.3f)" % (it, value, rms, float(np.abs(truth).max())))
    print("loss: %.6f -> %.6f" % (first, value))


if __name__ == "__main__":
    main()
