"""Randomised parity: small scenes drawn from the whole plugin inventory of the variant (shapes, instances, every BSDF model incl. zero and bitmap colours, every emitter kind,
both sensors, filters, crop windows, integrator depths) rendered by the HIP path and by the oracle with the same seed -- forward image (1e-4) with equal vertex counts, `prb`
primal image, and EVERY gradient of one `render_backward` call (colours, texels, emitter radiances; 1e-3) -- plus vertex-position gradients of the eligible meshes on a second call.
The hand-made scenes of the other files test what their author thought of; this file tests combinations nobody wrote down (round 6: the gradient at a black albedo was found by
comparing every gradient of a two-light scene).  Seeds are fixed: a failure is reproducible by its parameter."""
import numpy as np
import pytest

from tests.test_gpu_boundary import rel_l2

pytestmark = pytest.mark.gpu


def _seeds(var, default):
    """the seeds of one test: `default` of them in the suite; <var>=n runs n, HAR_FUZZ_SEED0=k starts at k (sweeps beyond the committed range)"""
    import os
    k = int(os.environ.get("HAR_FUZZ_SEED0", "0"))
    return list(range(k, k + int(os.environ.get(var, str(default)))))


def _colour(rng, allow_zero=True):
    c = rng.uniform(0.05, 0.9, 3)
    if allow_zero and rng.random() < 0.25:
        c[rng.integers(0, 3)] = 0.0                      # a channel that is exactly zero
    if allow_zero and rng.random() < 0.1:
        c[:] = 0.0                                       # a black surface
    return [float(x) for x in c]


def _bitmap(rng, lo=0.05, hi=0.9, allow_zero=True):
    h, w = int(rng.integers(2, 9)), int(rng.integers(2, 9))
    t = rng.uniform(lo, hi, (h, w, 3)).astype(np.float32)
    if allow_zero and rng.random() < 0.4:
        t[: max(1, h // 2), : max(1, w // 2)] = 0.0
    d = {"type": "bitmap", "data": t, "raw": True}
    if rng.random() < 0.4:
        d["filter_type"] = "nearest"
    if rng.random() < 0.5:
        d["wrap_mode"] = ["repeat", "mirror", "clamp"][int(rng.integers(0, 3))]
    return d


def _slot(rng, allow_zero=True):
    """a colour slot.  allow_zero = False for the diffuse base of `plastic` / `roughplastic`: with a channel at zero the value of that channel is the specular lobe alone, tiny away from
    the highlight, and prb's  L * (df / d rho) / f  multiplies the rounding noise of L (a difference of O(10) terms in fp32) by 1e15 -- in the reference as well; the product and the
    oracle then both return noise, not the same noise (seeds 5, 14, 18, 23 of the first version of this file)"""
    return _bitmap(rng, allow_zero=allow_zero) if rng.random() < 0.35 else {"type": "rgb", "value": _colour(rng, allow_zero)}


def _bsdf(rng, smooth_only=False):
    kinds = ["diffuse", "diffuse", "roughconductor", "roughplastic", "plastic", "twosided"] + ([] if smooth_only else ["dielectric", "conductor"])
    k = kinds[int(rng.integers(0, len(kinds)))]
    if k == "diffuse":
        return {"type": "diffuse", "reflectance": _slot(rng)}
    if k == "roughconductor":
        d = {"type": "roughconductor", "distribution": ["ggx", "beckmann"][int(rng.integers(0, 2))], "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14]}
        if rng.random() < 0.5:
            d["alpha"] = float(rng.uniform(0.1, 0.5))
        else:
            d["alpha_u"] = float(rng.uniform(0.1, 0.5)); d["alpha_v"] = float(rng.uniform(0.1, 0.5))
        if rng.random() < 0.3:
            d["specular_reflectance"] = {"type": "rgb", "value": _colour(rng, False)}
        return d
    if k == "roughplastic":
        return {"type": "roughplastic", "alpha": float(rng.uniform(0.1, 0.4)), "diffuse_reflectance": _slot(rng, False), "nonlinear": bool(rng.random() < 0.3)}
    if k == "plastic":
        return {"type": "plastic", "diffuse_reflectance": _slot(rng, False), "int_ior": float(rng.uniform(1.3, 1.9))}
    if k == "dielectric":
        return {"type": "dielectric", "int_ior": float(rng.uniform(1.2, 1.8))}
    if k == "conductor":
        return {"type": "conductor", "eta": [0.143, 0.375, 1.442], "k": [3.983, 2.386, 1.603]}
    inner = _bsdf(rng, smooth_only=True)
    while inner["type"] == "twosided":
        inner = _bsdf(rng, smooth_only=True)
    if rng.random() < 0.5:
        return {"type": "twosided", "m": inner}
    back = _bsdf(rng, smooth_only=True)
    while back["type"] == "twosided":
        back = _bsdf(rng, smooth_only=True)
    return {"type": "twosided", "front": inner, "back": back}


def random_scene(mi, seed):
    rng = np.random.default_rng(1000 + seed)
    T = mi.ScalarTransform4f
    W, H = int(rng.integers(20, 41)), int(rng.integers(20, 41))
    film = {"type": "hdrfilm", "width": W, "height": H, "pixel_format": "rgb",
            "rfilter": {"type": ["gaussian", "box", "tent"][int(rng.integers(0, 3))]}}
    if rng.random() < 0.3:
        cw, ch = int(rng.integers(8, W)), int(rng.integers(8, H))
        film.update({"crop_width": cw, "crop_height": ch, "crop_offset_x": int(rng.integers(0, W - cw + 1)), "crop_offset_y": int(rng.integers(0, H - ch + 1))})
    spp = int([4, 8, 16, 12][int(rng.integers(0, 4))])
    cam = T().look_at(origin=[float(rng.uniform(-0.4, 0.4)), float(rng.uniform(0.6, 1.4)), 3.2], target=[0, 0.3, 0], up=[0, 1, 0])
    if rng.random() < 0.2:
        sensor = {"type": "orthographic", "to_world": cam @ T().scale([1.6, 1.6, 1.0])}
    else:
        sensor = {"type": "perspective", "fov": float(rng.uniform(35, 60)), "to_world": cam}
    sensor.update({"film": film, "sampler": {"type": "independent", "sample_count": spp}})
    d = {"type": "scene", "sensor": sensor,
         "floor": {"type": "rectangle", "to_world": T().rotate([1, 0, 0], -90).scale([2.0, 2.0, 1.0]), "bsdf": _bsdf(rng, smooth_only=True)},
         "back": {"type": "rectangle", "to_world": T().translate([0, 1.0, -1.6]).scale([2.0, 1.4, 1.0]), "bsdf": _bsdf(rng, smooth_only=True)}}
    n_obj = int(rng.integers(1, 4))
    for i in range(n_obj):
        pos = [float(rng.uniform(-1.0, 1.0)), float(rng.uniform(0.25, 0.9)), float(rng.uniform(-0.9, 0.9))]
        xf = T().translate(pos).rotate([0, 1, 0], float(rng.uniform(0, 90))).scale([float(rng.uniform(0.15, 0.35))] * 3)
        kind = ["cube", "rectangle", "sphere"][int(rng.integers(0, 3))]
        if kind == "sphere":
            P, N, UV, F = mi.scenes.bumpy_sphere(10, 6, 1.0)
            M = np.asarray(xf.matrix, np.float64)
            Pw = (P.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
            d["obj%d" % i] = {"type": "mesh", "positions": Pw, "faces": F, "texcoords": UV, "bsdf": _bsdf(rng)}        # flat-shaded
        else:
            d["obj%d" % i] = {"type": kind, "to_world": xf, "bsdf": _bsdf(rng)}
    if rng.random() < 0.4:                     # a shape group with two or three instances
        d["grp"] = {"type": "shapegroup", "c": {"type": "cube", "bsdf": _bsdf(rng, smooth_only=True)}}
        for j in range(int(rng.integers(2, 4))):
            pos = [float(rng.uniform(-1.2, 1.2)), float(rng.uniform(0.2, 0.8)), float(rng.uniform(-1.0, 0.6))]
            d["inst%d" % j] = {"type": "instance", "shapegroup": {"type": "ref", "id": "grp"},
                               "to_world": T().translate(pos).rotate([0.3, 1, 0.2], float(rng.uniform(0, 180))).scale([float(rng.uniform(0.08, 0.2))] * 3)}
    # emitters
    kinds = ["area", "area_bitmap", "area_mesh", "point", "spot", "directional", "env"]
    n_em = int(rng.integers(1, 4)); chosen = []
    for e in range(n_em):
        k = kinds[int(rng.integers(0, len(kinds)))]
        if k == "env" and "env" in chosen:
            k = "area"
        if k == "area_bitmap" and "area_bitmap" in chosen:
            k = "area"
        chosen.append(k)
        sw = {"sampling_weight": float(rng.uniform(0.3, 3.0))} if rng.random() < 0.4 else {}
        pos = [float(rng.uniform(-0.8, 0.8)), float(rng.uniform(1.5, 2.0)), float(rng.uniform(-0.6, 0.8))]
        rad = [float(x) for x in rng.uniform(4.0, 12.0, 3)]
        if rng.random() < 0.15:
            rad = [0.0, 0.0, 0.0]                                  # a light that is switched off
        if k == "area":
            d["em%d" % e] = {"type": "rectangle", "to_world": T().translate(pos).rotate([1, 0, 0], 90).scale([0.25, 0.25, 1.0]),
                             "emitter": dict({"type": "area", "radiance": {"type": "rgb", "value": rad}}, **sw)}
        elif k == "area_bitmap":
            bm = _bitmap(rng, 2.0, 14.0, allow_zero=True); bm.pop("raw")
            if not bm["data"].any():
                bm["data"][:] = 3.0
            bm["data"][-1, -1] = 9.0                                # (some luminance to sample)
            d["em%d" % e] = {"type": "rectangle", "to_world": T().translate(pos).rotate([1, 0, 0], 90).scale([0.3, 0.3, 1.0]),
                             "emitter": dict({"type": "area", "radiance": bm}, **sw)}
        elif k == "area_mesh":
            d["em%d" % e] = {"type": "cube", "to_world": T().translate(pos).scale([0.12, 0.05, 0.12]), "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": _colour(rng)}},
                             "emitter": dict({"type": "area", "radiance": {"type": "rgb", "value": rad}}, **sw)}
        elif k == "point":
            d["em%d" % e] = dict({"type": "point", "position": pos, "intensity": {"type": "rgb", "value": rad}}, **sw)
        elif k == "spot":
            d["em%d" % e] = dict({"type": "spot", "to_world": T().look_at(origin=pos, target=[float(rng.uniform(-0.5, 0.5)), 0.0, float(rng.uniform(-0.5, 0.5))], up=[0, 0, 1]),
                                  "intensity": {"type": "rgb", "value": [3.0 * r for r in rad]}, "cutoff_angle": float(rng.uniform(30, 60)), "beam_width": float(rng.uniform(8, 25))}, **sw)
        elif k == "directional":
            d["em%d" % e] = dict({"type": "directional", "direction": [float(rng.uniform(-0.5, 0.5)), -1.0, float(rng.uniform(-0.5, 0.5))],
                                  "irradiance": {"type": "rgb", "value": [0.3 * r for r in rad]}}, **sw)
        else:
            if rng.random() < 0.5:
                d["em%d" % e] = dict({"type": "constant", "radiance": {"type": "rgb", "value": [0.08 * r for r in rad]}}, **sw)
            else:
                eh = int(rng.integers(4, 9))
                d["em%d" % e] = dict({"type": "envmap", "bitmap": mi.Bitmap(rng.uniform(0.1, 1.2, (eh, 2 * eh, 3)).astype(np.float32)), "scale": float(rng.uniform(0.5, 1.5))}, **sw)
    md = int(rng.integers(2, 8)); rr = int(rng.integers(2, 6))
    return d, dict(max_depth=md, rr_depth=rr, spp=spp, hide=bool(rng.random() < 0.15))


def _compare(name, got, ref, tol):
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    scale = np.sqrt((ref ** 2).sum())
    err = np.sqrt(((got - ref) ** 2).sum())
    assert np.isfinite(got).all(), name
    # absolute floor: prb's adjoint pass forms the radiance still to come as  L - sum(terms so far)  (prb.py:288-313), which for a path that ends at the vertex is the rounding
    # residue of an O(1) sum (a few 2^-24) where the oracle's dual numbers hold an exact zero -- a parameter no lit path reaches comes back as 1e-7, not 0 (seed 84 of the update test)
    # (err is an L2 norm: the floor grows with the square root of the number of colours compared -- seed 9158 of the update test: a texture no lit path reaches, 1e-8 per texel)
    # (the residue is relative to the radiance the path carries -- lights of radiance 4 ... 14 here: seed 20606 of the extended test, 5.7e-7 on the black BSDF of a light)
    assert err <= tol * scale + 2e-6 * max(1.0, np.abs(ref).max()) * max(1.0, np.sqrt(ref.size / 3.0)), (name, err / max(scale, 1e-30), got.reshape(-1)[:6], ref.reshape(-1)[:6])


def extend_scene(mi, d, seed):
    """what random_scene() does not draw, applied on top of its scenes with a stream of its own (the scenes of the other tests keep their seeds): all six reconstruction
    filters, `sample_border`, a smooth-shaded mesh (vertex normals) under a rotation, `to_uv` on the BSDFs' bitmaps, a rotated environment map, a shape group with a second
    child placed by its own transform"""
    rng = np.random.default_rng(31337 + seed)
    T = mi.ScalarTransform4f
    film = d["sensor"]["film"]
    film["rfilter"] = {"type": ["gaussian", "box", "tent", "mitchell", "catmullrom", "lanczos"][int(rng.integers(0, 6))]}
    if rng.random() < 0.25:
        film["sample_border"] = True
    if rng.random() < 0.7:
        P, N, UV, F = mi.scenes.bumpy_sphere(12, 8, 1.0)
        xf = T().translate([float(rng.uniform(-0.9, 0.9)), float(rng.uniform(0.3, 0.8)), float(rng.uniform(-0.6, 0.8))]).rotate([0.2, 1, 0.4], float(rng.uniform(0, 180))).scale(float(rng.uniform(0.15, 0.3)))
        M = np.asarray(xf.matrix, np.float64); R = M[:3, :3] / np.cbrt(np.linalg.det(M[:3, :3]))
        d["smooth"] = {"type": "mesh", "positions": (P.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32), "normals": (lambda n: (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32))(N.astype(np.float64) @ R.T),
                       "faces": F, "texcoords": UV, "bsdf": _bsdf(rng, smooth_only=True)}

    def walk(x, under_emitter=False):
        for k, v in list(x.items()):
            if not isinstance(v, dict):
                continue
            if v.get("type") == "bitmap" and not under_emitter and rng.random() < 0.4:
                v["to_uv"] = mi.ScalarTransform3f().translate([float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-0.5, 0.5))]).rotate(float(rng.uniform(0, 90))).scale([float(rng.uniform(0.5, 2.5)), float(rng.uniform(0.5, 2.5))])
            if v.get("type") == "envmap" and rng.random() < 0.7:
                v["to_world"] = T().rotate([0, 1, 0], float(rng.uniform(0, 360))).rotate([1, 0, 0], float(rng.uniform(-40, 40)))
            walk(v, under_emitter or k == "emitter")
    walk(d)
    if "grp" in d and rng.random() < 0.6:
        d["grp"]["r"] = {"type": "rectangle", "to_world": T().translate([0.0, 1.6, 0.0]).rotate([1, 0, 0], float(rng.uniform(20, 160))).scale([1.4, 0.8, 1.0]), "bsdf": _bsdf(rng, smooth_only=True)}
    return d


def _check_scene(mi, O, d, cfg, seed):
    spp, md, rr = cfg["spp"], cfg["max_depth"], cfg["rr_depth"]
    # ---- forward
    d["integrator"] = {"type": "path", "max_depth": md, "rr_depth": rr, "hide_emitters": cfg["hide"]}
    scene = mi.load_dict(d)
    osc, sensor = O.scene_from_product(scene); osc.set_hide_emitters(cfg["hide"])
    img = mi.render(scene, spp=spp, seed=seed).cpu().numpy()
    ref, ost = osc.render_path(sensor, seed=seed, spp=spp, max_depth=md, rr_depth=rr)
    _compare("path image", img, ref, 1e-4)
    st = scene.integrator().stats()
    assert st["vertices"] == ost.vertices and st["paths"] == ost.paths, (st, ost.vertices, ost.paths)
    # ---- prb: primal image and every gradient of one backward call
    d["integrator"] = {"type": "prb", "max_depth": md, "rr_depth": rr, "hide_emitters": cfg["hide"], "light_texel_gradients": True}
    scene = mi.load_dict(d)
    osc, sensor = O.scene_from_product(scene); osc.set_hide_emitters(cfg["hide"])
    img = mi.render(scene, spp=spp, seed=seed + 1).cpu().numpy()
    ref, _ = osc.render_prb(sensor, seed=seed + 1, spp=spp, max_depth=md, rr_depth=rr)
    _compare("prb image", img, ref, 1e-4)
    grad_in = np.random.default_rng(seed).uniform(0.5, 1.5, ref.shape).astype(np.float32)
    grads = scene.integrator().render_backward(scene, None, grad_in, seed=seed + 2, spp=spp)
    w_refl, w_tex, w_emit, _ = osc.render_prb_backward_emitters(sensor, grad_in, seed=seed + 2, spp=spp, max_depth=md, rr_depth=rr)
    for k, (kind, b) in scene._param_keys().items():
        want = w_emit[b] if kind == "emit" else (w_tex[b.tex_index] if kind == "tex" else w_refl[b.index])
        _compare(k, grads[k].cpu().numpy(), want, 1e-3)
    for k, (kind, i) in scene._pose_keys().items():
        if kind == "emitter_tex":
            _compare(k, grads[k].cpu().numpy(), w_tex[scene.emitters[i]["light"].tex_index], 1e-3)
    # ---- vertex-position gradients of every eligible top-level mesh (second call: item path instead of the tapes)
    if cfg["hide"]:
        return
    integ = scene.integrator(); integ.light_texel_gradients = False; integ.shape_gradients = True
    keys = scene._differentiable_position_keys()
    if not keys:
        return
    grads = integ.render_backward(scene, None, grad_in, seed=seed + 2, spp=spp)
    ids = sorted(keys.values())
    want, _, _, _ = osc.render_prb_backward_shape(sensor, grad_in, ids, seed=seed + 2, spp=spp, max_depth=md, rr_depth=rr)
    total = max(np.abs(want[m]).max() for m in ids)
    for k, m in keys.items():
        got = grads[k].cpu().numpy().reshape(-1, 3)
        assert np.isfinite(got).all(), k
        assert np.abs(got - want[m]).max() <= 2e-3 * max(np.abs(want[m]).max(), 1e-3 * total) + 1e-7, (k, np.abs(got - want[m]).max(), np.abs(want[m]).max())


@pytest.mark.parametrize("seed", _seeds("HAR_FUZZ_SEEDS", 32))
def test_random_scene_parity(mi, O, seed):
    d, cfg = random_scene(mi, seed)
    _check_scene(mi, O, d, cfg, seed)


@pytest.mark.parametrize("seed", _seeds("HAR_FUZZ_SEEDS6", 24))
def test_random_scene_extended(mi, O, seed):
    """the same checks (forward, prb, every gradient, vertex positions) on scenes with the features extend_scene() adds"""
    d, cfg = random_scene(mi, seed + 4000)
    _check_scene(mi, O, extend_scene(mi, d, seed), cfg, seed)


@pytest.mark.parametrize("seed", _seeds("HAR_FUZZ_SEEDS2", 24))
def test_random_scene_options(mi, O, seed):
    """the same scenes under the integrator's OTHER code paths: chunked wavefronts, multi-pass renders, the lane-indexed replay cache / no cache at all, per-material queues, the
    forward-mode derivative (RBIntegrator.render_forward: random tangents on every colour / texel / radiance), gradients of alpha / eta / k / specular colours, and instance
    transforms -- each against the oracle"""
    d, cfg = random_scene(mi, seed + 500)
    rng = np.random.default_rng(7000 + seed)
    spp, md, rr = cfg["spp"], cfg["max_depth"], cfg["rr_depth"]
    if spp == 12:
        spp = 8
    opts = {}
    if rng.random() < 0.5:
        opts["chunk_lanes"] = int(rng.integers(1, 5)) * 2048          # several chunks per frame
    if rng.random() < 0.3:
        opts["material_queues"] = True
    # ---- forward, possibly in passes
    popts = dict(opts)
    if rng.random() < 0.4 and spp >= 4:
        popts["samples_per_pass"] = spp // 2
    d["integrator"] = dict({"type": "path", "max_depth": md, "rr_depth": rr}, **popts)
    scene = mi.load_dict(d)
    osc, sensor = O.scene_from_product(scene)
    img = mi.render(scene, spp=spp, seed=seed).cpu().numpy()
    if "samples_per_pass" in popts:
        ref, _ = osc.render_path_passes(sensor, seed=seed, spp=spp, spp_per_pass=spp // 2, max_depth=md, rr_depth=rr)
    else:
        ref, _ = osc.render_path(sensor, seed=seed, spp=spp, max_depth=md, rr_depth=rr)
    _compare("path image", img, ref, 1e-4)
    # ---- prb backward through the replay cache / without any cache
    if rng.random() < 0.5:
        opts["replay_cache"] = False
    d["integrator"] = dict({"type": "prb", "max_depth": md, "rr_depth": rr, "bsdf_parameter_gradients": bool(rng.random() < 0.5)}, **opts)
    if d["integrator"]["bsdf_parameter_gradients"]:
        d["integrator"].pop("replay_cache", None)                      # (those gradients need the cache)
    scene = mi.load_dict(d)
    osc, sensor = O.scene_from_product(scene)
    grad_in = np.random.default_rng(seed).uniform(0.5, 1.5, ref.shape).astype(np.float32)
    integ = scene.integrator()
    grads = integ.render_backward(scene, None, grad_in, seed=seed + 2, spp=spp)
    w_refl, w_tex, w_emit, _ = osc.render_prb_backward_emitters(sensor, grad_in, seed=seed + 2, spp=spp, max_depth=md, rr_depth=rr)
    for k, (kind, b) in scene._param_keys().items():
        want = w_emit[b] if kind == "emit" else (w_tex[b.tex_index] if kind == "tex" else w_refl[b.index])
        _compare(k, grads[k].cpu().numpy(), want, 1e-3)
    if integ.bsdf_parameter_gradients and scene._bsdf_param_keys():
        gx = osc.render_prb_backward_bsdf_params(sensor, grad_in, seed=seed + 2, spp=spp, max_depth=md, rr_depth=rr)
        gx = gx[0] if isinstance(gx, tuple) else gx
        for k, (what, b) in scene._bsdf_param_keys().items():
            if what == "ior":
                continue                                                  # (the scalar index of refraction: updatable, no gradient)
            rec = np.asarray(gx[b.index], np.float64).reshape(5, 3)
            want = {"alpha": rec[0:2].sum(), "alpha_u": rec[0].sum(), "alpha_v": rec[1].sum(), "eta": rec[2], "k": rec[3], "slot1": rec[4]}[what]
            got = grads[k].cpu().numpy().astype(np.float64)
            scale = max(np.abs(np.atleast_1d(want)).max(), 1e-3 * float(np.abs(gx).max()), 1e-12)        # (a record only a handful of paths reach: L * (df / d theta) / f is noise at the 1e-6 level)
            assert np.isfinite(got).all() and np.abs(got.reshape(-1) - np.atleast_1d(want).reshape(-1)).max() <= 2e-3 * scale + 5e-7, (k, got, want)      # (+ the residue floor of _compare: seeds 2091, 2094, 5258)
    # ---- forward mode: random tangents on every key of the gradient tables
    keys = scene._param_keys()
    if keys:
        trng = np.random.default_rng(seed + 11)
        tangents, t_refl, t_emit = {}, np.zeros((len(scene.bsdfs), 3), np.float32), np.zeros((max(1, len(scene.emitters)), 3), np.float32)
        t_tex = [np.zeros_like(np.asarray(t, np.float32)) for t in scene.textures]
        for k, (kind, b) in keys.items():
            if kind == "tex":
                t_tex[b.tex_index] = trng.uniform(-1, 1, t_tex[b.tex_index].shape).astype(np.float32); tangents[k] = t_tex[b.tex_index]
            elif kind == "emit":
                t_emit[b] = trng.uniform(-1, 1, 3); tangents[k] = t_emit[b]
            else:
                t_refl[b.index] = trng.uniform(-1, 1, 3); tangents[k] = t_refl[b.index]
        fimg = integ.render_forward(scene, None, seed=seed + 3, spp=spp, tangents=tangents).cpu().numpy()
        fref = osc.render_prb_forward(sensor, t_refl, t_tex, t_emit, seed=seed + 3, spp=spp, max_depth=md, rr_depth=rr)
        _compare("forward-mode image", fimg, fref, 1e-3)
    # ---- instance transforms
    ikeys = scene._instance_keys()
    smooth = all(scene._bsdf_has_smooth_lobe(m["bsdf"]) for m in scene.meshes[scene.top_mesh_count:])
    if ikeys and smooth:
        integ.bsdf_parameter_gradients = False
        integ.shape_gradients = sorted(ikeys)
        grads = integ.render_backward(scene, None, grad_in, seed=seed + 2, spp=spp)
        want, _, _, _ = osc.render_prb_backward_instances(sensor, grad_in, None, seed=seed + 2, spp=spp, max_depth=md, rr_depth=rr)
        total = max(np.abs(want[i]).max() for i in ikeys.values())
        for k, i in ikeys.items():
            got = grads[k].cpu().numpy()
            # floor 1e-5 of the largest instance gradient: an instance that paths only END on has an exact zero in the oracle and the rounding residue of  L - sum(terms)  (see
            # _compare) times the geometric terms' 1 / r in the product (seed 2098: 1.4e-5 against 3.1 for the neighbouring instance)
            assert np.isfinite(got).all() and np.abs(got[:3] - want[i]).max() <= 2e-3 * max(np.abs(want[i]).max(), 1e-3 * total) + 1e-5 * max(total, 1.0), (k, np.abs(got[:3] - want[i]).max(), np.abs(want[i]).max())      # (total = 0: no instance is reached by a lit path -- seeds 3215, 3219)


def _perturb(mi, scene, params, rng, torch):
    """new values for a random subset of the keys of mi.traverse(scene), of every kind an update path exists for; returns {key written: a host copy of its value}"""
    from tests.update_reference import final_values
    written = []
    pose = scene._pose_keys(); bsdfp = scene._bsdf_param_keys(); pos = scene._position_keys(); inst = scene._instance_keys(); colour = scene._param_keys(); rect = scene._rect_keys()
    for k in list(params.keys()):
        if rng.random() > 0.5:
            continue
        v = params[k]
        if k in colour:
            new = v * torch.as_tensor(rng.uniform(0.5, 1.5, tuple(v.shape)), dtype=v.dtype, device=v.device)
            if rng.random() < 0.5:
                with torch.no_grad():
                    v.copy_(new)                                  # in place, as an optimiser step would (version counter)
            else:
                params[k] = new
        elif k in pos:
            m = pos[k]
            if scene.meshes[m]["emitter"] >= 0 and scene.meshes[m].get("rect") is not None:
                continue                                          # (a rectangle light moves through its '<rect>.to_world' here)
            noise = torch.as_tensor(rng.normal(0.0, 0.004, tuple(v.shape)), dtype=v.dtype, device=v.device)
            params[k] = (v + noise) if rng.random() < 0.5 else (v + noise).cpu()          # device-resident and host update paths
        elif k in inst:
            m = v.clone(); m[:3, 3] += torch.as_tensor(rng.uniform(-0.05, 0.05, 3), dtype=v.dtype, device=v.device)
            params[k] = m if rng.random() < 0.5 else m.cpu()
        elif k in rect:                                           # Rectangle's own parameter: the shape (and its area light's sampling record) is re-baked from it
            if k[:-len(".to_world")] + ".positions" in written:
                continue                                          # (one way of moving a shape per round)
            m = v.clone(); m[:3, 3] += torch.as_tensor(rng.uniform(-0.04, 0.04, 3), dtype=v.dtype, device=v.device)
            if rng.random() < 0.3:
                m[:3, 0] *= float(rng.uniform(0.8, 1.2))          # stretched along its first axis
            params[k] = m
        elif k in bsdfp:
            what = bsdfp[k][0]
            if what in ("alpha", "alpha_u", "alpha_v"):
                params[k] = (v * float(rng.uniform(0.7, 1.3))).clamp(0.05, 0.9)
            elif what in ("eta", "k"):
                params[k] = v * torch.as_tensor(rng.uniform(0.9, 1.1, tuple(v.shape)), dtype=v.dtype, device=v.device)
            elif what == "ior":
                params[k] = (v * float(rng.uniform(0.95, 1.08))).clamp(1.05, 2.5)
            else:
                params[k] = (v * float(rng.uniform(0.6, 1.2))).clamp(0.0, 1.0)
        elif k in pose:
            kind = pose[k][0]
            if kind == "position":
                params[k] = v + torch.as_tensor(rng.uniform(-0.1, 0.1, 3), dtype=v.dtype, device=v.device)
            elif kind in ("emitter_to_world", "sensor"):
                m = v.clone(); m[:3, 3] += torch.as_tensor(rng.uniform(-0.05, 0.05, 3), dtype=v.dtype, device=v.device)
                if kind == "emitter_to_world" and scene.emitters[pose[k][1]].get("type") == 2:      # an environment map: turned about the y axis
                    a = float(rng.uniform(0.2, 1.0)); c, sn = np.cos(a), np.sin(a)
                    m = torch.as_tensor(np.array([[c, 0, sn, 0], [0, 1, 0, 0], [-sn, 0, c, 0], [0, 0, 0, 1]], np.float32), device=v.device) @ v
                params[k] = m
            elif kind == "cutoff_angle":
                continue                                          # (cutoff and beam width move together below)
            elif kind == "beam_width":
                ck = k.replace("beam_width", "cutoff_angle"); f = float(rng.uniform(0.8, 1.1))
                params[k] = v * f; params[ck] = params[ck] * f; written.append(ck)
            elif kind == "sampling_weight":
                params[k] = v * float(rng.uniform(0.5, 2.0))
            elif kind == "env_scale":
                params[k] = v * float(rng.uniform(0.5, 1.5))
            elif kind == "x_fov":
                params[k] = v * float(rng.uniform(0.8, 1.2))
            elif kind in ("emitter_tex", "env_data"):
                params[k] = v * torch.as_tensor(rng.uniform(0.5, 1.5, tuple(v.shape)), dtype=v.dtype, device=v.device)
            else:
                continue                                          # to_uv: constrained (a light's must keep the unit square), covered by its own tests
        else:
            continue
        written.append(k)
    return final_values(params, written)


@pytest.mark.parametrize("seed", _seeds("HAR_FUZZ_SEEDS3", 24))
def test_random_parameter_updates(mi, O, seed):
    """params.update() after writing a random subset of mi.traverse(scene) -- colours and texels (device-to-device, in place or as new tensors), emitter radiances, vertex positions
    (device-resident refit and the host path; emitter meshes included), instance transforms, alpha / eta / k, light placements and cones, sampling weights, the sensor's pose --
    then a second round on top.  After each round: the render equals the oracle's render of the scene's host mirrors (device state == host state), every key written so far
    reads back its last written value through a new mi.traverse (host state == what was written: update_reference.assert_values_kept), and the render equals the render of a
    FRESH load with those values written before its first render, and the oracle's render of that fresh scene (update_reference.fresh_reference: a reference that is not
    made from the scene under test); one backward call at the end"""
    import torch
    from tests.update_reference import assert_values_kept, fresh_reference
    d, cfg = random_scene(mi, seed + 900)
    spp, md, rr = cfg["spp"], cfg["max_depth"], cfg["rr_depth"]
    d["integrator"] = {"type": "prb", "max_depth": md, "rr_depth": rr}
    scene = mi.load_dict(d)
    params = mi.traverse(scene)
    first = mi.render(scene, spp=spp, seed=seed).cpu().numpy()
    rng = np.random.default_rng(4000 + seed)
    values = {}                                                     # every key written so far -> its last written value
    for rnd in range(2):
        written = _perturb(mi, scene, params, rng, torch)
        params.update()
        rect = scene._rect_keys()
        for k in written:                                           # a rectangle moved through its positions and through its to_world: the later write is its state
            base = k.rsplit(".", 1)[0]
            if k in rect:
                values.pop(base + ".positions", None)
            elif k.endswith(".positions") and base + ".to_world" in rect:
                values.pop(base + ".to_world", None)
        values.update(written)
        img = mi.render(scene, spp=spp, seed=seed).cpu().numpy()
        osc, sensor = O.scene_from_product(scene)
        ref, ost = osc.render_prb(sensor, seed=seed, spp=spp, max_depth=md, rr_depth=rr)
        _compare("image after update round %d (%d keys)" % (rnd, len(written)), img, ref, 1e-4)
        assert scene.integrator().stats()["vertices"] == ost.vertices, (rnd, written)
        if rnd == 0 and len(written) >= 3 and np.abs(first).max() > 0:                # (a sensor that sees nothing stays black)
            assert rel_l2(img, first) > 1e-4, written              # the update did change the picture
        assert_values_kept(scene, values)
        fresh = fresh_reference(d, values)
        # (1e-5, not 1e-6: normals regenerated on the device differ from the host's by a few ulps, test_gpu_accel_update.py)
        _compare("image after update round %d vs a fresh load" % rnd, img, mi.render(fresh, spp=spp, seed=seed).cpu().numpy(), 1e-5)
        fosc, fsensor = O.scene_from_product(fresh)
        fref, _ = fosc.render_prb(fsensor, seed=seed, spp=spp, max_depth=md, rr_depth=rr)
        _compare("image after update round %d vs the oracle of a fresh load" % rnd, img, fref, 1e-4)
    grad_in = np.random.default_rng(seed).uniform(0.5, 1.5, ref.shape).astype(np.float32)
    grads = scene.integrator().render_backward(scene, None, grad_in, seed=seed + 2, spp=spp)
    w_refl, w_tex, w_emit, _ = osc.render_prb_backward_emitters(sensor, grad_in, seed=seed + 2, spp=spp, max_depth=md, rr_depth=rr)
    for k, (kind, b) in scene._param_keys().items():
        want = w_emit[b] if kind == "emit" else (w_tex[b.tex_index] if kind == "tex" else w_refl[b.index])
        _compare(k, grads[k].cpu().numpy(), want, 1e-3)


@pytest.mark.parametrize("seed", _seeds("HAR_FUZZ_SEEDS4", 16))
def test_random_scene_bands(mi, O, seed):
    """the multi-GPU partition on random scenes (contiguous row bands of the reference's lane order, global lane indices, additive films and gradients): the frame cut
    into two to four random row bands, each rendered on its own (lanes = [begin, end), as a rank does) -- the band films add up to the single render's raw film with equal
    path / vertex / ray counters, the bands' weight films to the weight film, and the bands' `prb` gradients (every colour, texel and radiance key, each band against the
    SUMMED weight film: render_distributed's two-phase adjoint) to the single call's; the sum is then held to the oracle once"""
    import torch
    d, cfg = random_scene(mi, seed + 1700)
    rng = np.random.default_rng(9000 + seed)
    spp, md, rr = cfg["spp"], cfg["max_depth"], cfg["rr_depth"]
    d["integrator"] = {"type": "prb", "max_depth": md, "rr_depth": rr}
    scene = mi.load_dict(d)
    integ = scene.integrator(); sensor = scene.sensors()[0]
    w, h = sensor.film().crop_size()
    per_row = w * spp
    cuts = sorted(set(int(x) for x in rng.integers(1, h, int(rng.integers(1, 4)))))
    rows = [0] + cuts + [h]
    bands = [(rows[i] * per_row, rows[i + 1] * per_row) for i in range(len(rows) - 1)]
    full = integ.render_film(scene, seed=seed, spp=spp); st_full = integ.stats()
    acc = torch.zeros_like(full); st_sum = dict.fromkeys(st_full, 0)
    for b in bands:
        acc += integ.render_film(scene, seed=seed, spp=spp, lanes=b)
        for k, v in integ.stats().items():
            st_sum[k] += v
    assert st_sum == st_full, (bands, st_sum, st_full)
    _compare("sum of the band films", acc.cpu().numpy(), full.cpu().numpy(), 2e-6)
    wf = integ.render_weights(scene, seed=seed + 2, spp=spp)
    wsum = sum(integ.render_weights(scene, seed=seed + 2, spp=spp, lanes=b) for b in bands)
    _compare("sum of the band weight films", wsum.cpu().numpy(), wf.cpu().numpy(), 2e-6)
    grad_in = np.random.default_rng(seed).uniform(0.5, 1.5, (h, w, 3)).astype(np.float32)
    g_full = integ.render_backward(scene, None, grad_in, seed=seed + 2, spp=spp)
    g_sum = None
    for b in bands:
        g = integ.render_backward(scene, None, grad_in, seed=seed + 2, spp=spp, lanes=b, weight_film=wsum)
        g_sum = {k: v.clone() for k, v in g.items()} if g_sum is None else {k: g_sum[k] + g[k] for k in g_sum}
    assert set(g_sum) == set(g_full)
    for k in g_full:
        _compare("band gradients " + k, g_sum[k].cpu().numpy(), g_full[k].cpu().numpy(), 1e-4)
    osc, osensor = O.scene_from_product(scene)
    w_refl, w_tex, w_emit, _ = osc.render_prb_backward_emitters(osensor, grad_in, seed=seed + 2, spp=spp, max_depth=md, rr_depth=rr)
    for k, (kind, b) in scene._param_keys().items():
        want = w_emit[b] if kind == "emit" else (w_tex[b.tex_index] if kind == "tex" else w_refl[b.index])
        _compare(k, g_sum[k].cpu().numpy(), want, 1e-3)


@pytest.mark.parametrize("seed", _seeds("HAR_FUZZ_SEEDS5", 12))
def test_random_scene_boundary_calls(mi, O, seed):
    """the array-valued entry points of the boundary on random scenes (the hand-made tests use three): Scene::ray_intersect_preliminary / ray_test (accelerated and brute force,
    bit for bit against the oracle's brute force), PreliminaryIntersection::compute_surface_interaction, SamplingIntegrator::sample of `path` and `prb` with a random `active`
    mask (masked lanes: zero radiance, invalid, sampler untouched)"""
    from tests.test_gpu_parity import random_rays
    d, cfg = random_scene(mi, seed + 2600)
    md, rr = cfg["max_depth"], cfg["rr_depth"]
    n = 20000
    o, dd = random_rays(n, seed=seed); o = (1.5 * o).astype(np.float32); o[1] += 0.6
    rng = np.random.default_rng(seed)
    maxt = np.where(rng.random(n) < 0.3, rng.uniform(0.05, 3.0, n), 3.402823466e+38).astype(np.float32)
    for kind in ("path", "prb"):
        d["integrator"] = {"type": kind, "max_depth": md, "rr_depth": rr}
        scene = mi.load_dict(d)
        osc, _ = O.scene_from_product(scene)
        ray = mi.Ray3f(o, dd, maxt)
        if kind == "path":
            ref = osc.ray_intersect(o, dd, maxt, naive=True); hit = np.isfinite(ref[0])
            for naive in (False, True):
                pi = scene._intersect(ray, naive)
                assert np.array_equal(pi.t.cpu().numpy(), ref[0])
                for got, want in ((pi.prim_uv[0], ref[1]), (pi.prim_uv[1], ref[2]), (pi.prim_index, ref[3]), (pi.shape_index, ref[4]), (pi.instance, ref[5])):
                    g = got.cpu().numpy(); g = g.astype(np.uint32) if want.dtype == np.uint32 else g
                    assert np.array_equal(g[hit], want[hit])
                assert np.array_equal(scene.ray_test(ray, naive=naive).cpu().numpy(), osc.ray_test(o, dd, maxt))
            pi = scene.ray_intersect_preliminary(ray); si = pi.compute_surface_interaction(ray)
            t = pi.t.cpu().numpy(); u = pi.prim_uv[0].cpu().numpy(); v = pi.prim_uv[1].cpu().numpy()
            prim = pi.prim_index.cpu().numpy().astype(np.uint32); shape = pi.shape_index.cpu().numpy().astype(np.uint32); inst = pi.instance.cpu().numpy().astype(np.uint32)
            got = {k: getattr(si, k).cpu().numpy() for k in ("p", "n", "wi", "uv")}
            got["sn"] = si.sh_frame.n.cpu().numpy(); got["ss"] = si.sh_frame.s.cpu().numpy(); got["st"] = si.sh_frame.t.cpu().numpy()
            out = np.empty(24, np.float32)
            for i in np.flatnonzero(hit)[:600]:
                O.lib().orc_surface_interaction(osc.handle, O.fp(np.ascontiguousarray(o[:, i])), O.fp(np.ascontiguousarray(dd[:, i])), float(t[i]), float(u[i]), float(v[i]),
                                                int(prim[i]), int(shape[i]), int(inst[i]), O.fp(out))
                for key, sl in (("p", slice(0, 3)), ("n", slice(3, 6)), ("sn", slice(6, 9)), ("ss", slice(9, 12)), ("st", slice(12, 15)), ("wi", slice(15, 18)), ("uv", slice(18, 20))):
                    assert np.allclose(got[key][:, i], out[sl], rtol=4e-6, atol=4e-7), (key, int(i), got[key][:, i], out[sl])
        # SamplingIntegrator::sample with a mask
        active = rng.random(n) < 0.8
        sampler = mi.Sampler({"sample_count": 4, "seed": 5}); sampler.seed(3, n)
        before = sampler.state.cpu().numpy().view(np.uint64).copy()
        full = np.full(n, 3.402823466e+38, np.float32)
        spec, valid = scene.integrator().sample(scene, sampler, mi.Ray3f(o, dd, full), active=active)
        ref, rvalid, rstate = osc.integrator_sample(o, dd, full, seed=5 + 3, max_depth=md, rr_depth=rr, prb=(kind == "prb"))
        spec = spec.cpu().numpy(); valid = valid.cpu().numpy().astype(np.uint8)
        assert np.array_equal(valid[active], rvalid[active]) and not valid[~active].any() and not spec[:, ~active].any()
        _compare(kind + " sample()", spec[:, active], ref[:, active], 1e-4)
        after = sampler.state.cpu().numpy().view(np.uint64).reshape(-1)
        assert np.array_equal(after[~active], before.reshape(-1)[~active])                     # a masked lane's stream is where it was
        if kind == "path":
            assert np.array_equal(after[active], np.asarray(rstate).reshape(-1)[active])       # the others advanced exactly as the oracle's
