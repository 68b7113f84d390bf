#!/usr/bin/env python3
"""A window: the Cornell box behind a tinted pane of thin glass (`thindielectric`, src/bsdfs/thindielectric.cpp), rendered with `path` onto an `rgba` film, and one
`prb` step on the texture of the back wall seen THROUGH the pane.

    python examples/render_window.py [output.exr] [spp]

The pane is one rectangle across the open front of the box.  A thin dielectric reflects with r' = r * 2 / (1 + r) (the Fresnel reflectance with the internal
reflections summed) and otherwise lets the ray pass straight through -- a null lobe, so nothing refracts and a camera sample that only ever passed through panes is
not a valid one (path.cpp:307-308).  Shadow rays are stopped by the pane, as in the reference (Scene::ray_test): the box is lit by its own lamp, and light reaches
the camera side only along BSDF-sampled paths.  The pane's own parameters have no `prb` gradient (its eval() is zero for every direction); the wall texture behind
it does, and the script prints the loss before and after one gradient step on it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mitsuba3_amd as mi                                   # noqa: E402


def scene_dict(res, spp, integrator="path"):
    T = mi.ScalarTransform4f
    d = mi.cornell_box()
    d["integrator"] = {"type": integrator, "max_depth": 6}
    d["sensor"]["film"].update({"width": res, "height": res, "pixel_format": "rgba" if integrator == "path" else "rgb"})
    d["sensor"]["sampler"] = {"type": "independent", "sample_count": spp}
    d["glass"] = {"type": "thindielectric", "int_ior": "bk7", "ext_ior": "air", "specular_transmittance": {"type": "rgb", "value": [0.75, 0.9, 0.8]}}
    d["window"] = {"type": "rectangle", "to_world": T().translate([0.0, 0.0, 1.0]), "bsdf": {"type": "ref", "id": "glass"}}
    v, u = (np.mgrid[0:16, 0:16] + 0.5) / 16
    checker = 0.25 + 0.5 * (((u * 4).astype(int) + (v * 4).astype(int)) % 2)
    d["paper"] = {"type": "diffuse", "reflectance": {"type": "bitmap", "data": np.stack([checker, checker, 0.8 * checker], 2).astype(np.float32), "raw": True}}
    d["back"]["bsdf"] = {"type": "ref", "id": "paper"}
    return d


def main():
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else "window.exr"
    spp = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    mi.set_variant("hip_ad_rgb")
    img = mi.render(mi.load_dict(scene_dict(256, spp)), spp=spp, seed=0).cpu().numpy()
    assert img.shape[2] == 4
    mi.Bitmap(np.ascontiguousarray(img, np.float32)).write(out)
    print("wrote %s: %d x %d RGBA, alpha in [%.3f, %.3f], mean alpha %.3f" % (out, img.shape[1], img.shape[0], img[..., 3].min(), img[..., 3].max(), img[..., 3].mean()))
    # one prb step on the wall texture behind the pane: make the wall brighter where the image is darker than a flat grey target
    scene = mi.load_dict(scene_dict(96, 16, "prb"))
    params = mi.traverse(scene); key = "paper.reflectance.data"
    params[key].requires_grad_()
    loss_of = lambda im: ((im - 0.4) ** 2).mean()
    loss = loss_of(mi.render(scene, params, spp=16, seed=1)); loss.backward()
    g = params[key].grad
    with torch.no_grad():
        params[key] = (params[key] - 0.5 * g / g.abs().max()).clamp(0.02, 0.98); params.update()
    after = loss_of(mi.render(scene, spp=16, seed=1))
    print("prb through the pane: loss %.5f -> %.5f after one step on %s (|grad| max %.3g); '%s' has no gradient of its own" % (float(loss.detach()), float(after), key, float(g.abs().max()), "glass.eta"))


if __name__ == "__main__":
    main()
