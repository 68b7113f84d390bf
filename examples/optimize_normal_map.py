#!/usr/bin/env python3
"""Recover a normal map: a rectangle carries `normalmap(roughplastic)` (src/bsdfs/normalmap.cpp) under a point light and an area light.  The target is rendered from a
bumpy 32 x 32 normal map; the map is then recovered from the flat one, (0.5, 0.5, 1) everywhere, with mi.render + Adam -- the gradient with respect to the texels comes
out of the `prb` adjoint: the chain through 2c - 1, the flip, normalize, the perturbed frame, the nested model's directional derivatives and the shadow term.

    python examples/optimize_normal_map.py [iterations]

After each step the texels are re-projected: the normal n = 2c - 1 is made unit length again and kept within 60 degrees of the surface normal, so that it stays away
from the zero vector (where normalize has no derivative) and from the horizon.  The loss at the start and at the end is printed, with the mean angle between the
recovered and the true normals."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mitsuba3_amd as mi                                   # noqa: E402


def bumps(n=32, cells=3, depth=0.5):
    """n x n x 3 normal-map texels of a height field of cells x cells cosine bumps: n = normalize(-dh/du, -dh/dv, 1), stored as n * 0.5 + 0.5"""
    v, u = (np.mgrid[0:n, 0:n] + 0.5) / n
    pu, pv = 2 * np.pi * cells * u, 2 * np.pi * cells * v
    nrm = np.stack([depth * np.sin(pu) * (1 + np.cos(pv)) * 0.5, depth * np.sin(pv) * (1 + np.cos(pu)) * 0.5, np.ones_like(u)], 2)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    return (nrm * 0.5 + 0.5).astype(np.float32)


def scene_dict(texels, res, spp):
    T = mi.ScalarTransform4f
    return {"type": "scene",
            "integrator": {"type": "prb", "max_depth": 3},
            "sensor": {"type": "perspective", "fov": 40, "to_world": T().look_at([0, -1.6, 2.4], [0, 0, 0], [0, 0, 1]),
                       "film": {"type": "hdrfilm", "width": res, "height": res}, "sampler": {"type": "independent", "sample_count": spp}},
            "mat": {"type": "normalmap", "normalmap": {"type": "bitmap", "data": texels, "raw": True},
                    "coating": {"type": "roughplastic", "diffuse_reflectance": {"type": "rgb", "value": [0.25, 0.4, 0.7]}, "alpha": 0.2}},
            "plane": {"type": "rectangle", "bsdf": {"type": "ref", "id": "mat"}},
            "lamp": {"type": "point", "position": [0.9, 0.6, 1.5], "intensity": {"type": "rgb", "value": [5.0, 4.5, 4.0]}},
            "panel": {"type": "rectangle", "to_world": T().translate([-0.9, 0.5, 1.6]).rotate([0, 1, 0], 145).scale([0.6, 0.6, 1.0]),
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [9, 10, 12]}}}}


def reproject(c, max_tilt_deg=60.0):
    """texels -> texels of unit normals within max_tilt_deg of +z (in place)"""
    n = 2.0 * c - 1.0
    n[..., 2].clamp_(min=1e-3)
    n /= n.norm(dim=-1, keepdim=True)
    zmin = float(np.cos(np.radians(max_tilt_deg)))
    low = n[..., 2] < zmin
    if bool(low.any()):
        xy = n[..., :2][low]
        n[..., :2][low] = xy / xy.norm(dim=-1, keepdim=True) * float(np.sqrt(1 - zmin * zmin))
        n[..., 2][low] = zmin
    c.copy_(n * 0.5 + 0.5)


def main():
    iterations = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    mi.set_variant("hip_ad_rgb")
    res, spp, n = 128, 32, 32
    truth = bumps(n)
    target = mi.render(mi.load_dict(scene_dict(truth, res, 256)), spp=256, seed=1000)
    flat = np.tile(np.array([0.5, 0.5, 1.0], np.float32), (n, n, 1))
    scene = mi.load_dict(scene_dict(flat, res, spp))
    params = mi.traverse(scene)
    key = "mat.normalmap.data"
    params[key].requires_grad_(True)
    opt = torch.optim.Adam([params[key]], lr=0.02)
    true_n = torch.from_numpy(2.0 * truth - 1.0)
    first = None
    for it in range(iterations):
        opt.zero_grad()
        img = mi.render(scene, params, spp=spp, seed=it)
        loss = ((img - target) ** 2).mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            reproject(params[key])
        params.update()
        value = float(loss.detach()); first = value if first is None else first
        if it % 10 == 0 or it == iterations - 1:
            rec_n = 2.0 * params[key].detach().cpu() - 1.0
            ang = torch.rad2deg(torch.acos(((rec_n / rec_n.norm(dim=-1, keepdim=True)) * true_n).sum(-1).clamp(-1, 1))).mean()
            print("iter %3d  loss %.6f  mean angle to the true normals %.2f degrees" % (it, value, float(ang)))
    print("loss: %.6f -> %.6f" % (first, value))


if __name__ == "__main__":
    main()
