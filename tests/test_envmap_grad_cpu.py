"""`prb` gradients of an environment map's `data` and `scale`, the parts that need no GPU: the transpose of the map's bilinear lookup on the host (envmap_taps through
har_envmap_taps_host) against the oracle's lookup and a float64 scatter, the Python surface (`envmap_gradients`, mi.render's refusals, the gradient's layout) and the property
the device test leans on -- the oracle's same-seed render is affine along luminance-free texel directions."""
import ctypes as C

import numpy as np
import pytest

from tests import envmap_grad_cases as K


def _taps(mi, scene, uv, g=None):
    n = len(uv); fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    h, w, _ = scene.textures[[e for e in scene.emitters if e["type"] == 2][0]["mesh"]].shape
    uvt = np.ascontiguousarray(np.asarray(uv, np.float32).T)
    idx = np.zeros((4, n), np.uint32); wgt = np.zeros((4, n), np.float32); value = np.zeros((3, n), np.float32); ev = np.zeros((3, n), np.float32)
    gg = np.ascontiguousarray(np.asarray(g, np.float32).T) if g is not None else None
    grad = np.zeros((h, w, 3), np.float32) if g is not None else None
    d = scene.desc()
    rc = mi.lib().har_envmap_taps_host(C.byref(d), n, fp(uvt), idx.ctypes.data_as(C.c_void_p), fp(wgt), fp(value), fp(ev), fp(gg) if g is not None else None,
                                       fp(grad) if g is not None else None)
    assert rc == 0, mi.lib().har_last_error()
    return idx.T, wgt.T, value.T, ev.T, grad


def _uv_pairs(w, rng, n=20000):
    """n lookups: random ones, u within one float of 0 and 1, u outside [0, 1], v = 0, v = 1 and both seam columns (the first and last half texel in u)"""
    uv = rng.random((n, 2)).astype(np.float32)
    one = np.float32(1.0)
    edge = np.float32([0.0, np.nextafter(np.float32(0), one), np.nextafter(one, np.float32(0)), 1.0, -np.nextafter(np.float32(0), one), np.nextafter(one, np.float32(2))])
    uv[:600, 0] = np.tile(edge, 100)
    uv[600:1200, 0] = rng.uniform(-2.5, 3.5, 600).astype(np.float32)            # outside [0, 1]: the lookup wraps
    uv[1200:1500, 1] = 0.0; uv[1500:1800, 1] = 1.0                               # the poles: rows clamp
    uv[1800:1900, 1] = rng.uniform(-0.5, 0.0, 100).astype(np.float32); uv[1900:2000, 1] = rng.uniform(1.0, 1.5, 100).astype(np.float32)
    uv[2000:3000, 0] = (rng.random(1000) * 0.5 / w).astype(np.float32)           # storage column 0 = the halo that copies real column W - 1
    uv[3000:4000, 0] = (1.0 - rng.random(1000) * 0.5 / w).astype(np.float32)     # storage column W + 1 = the halo that copies real column 0
    return uv


@pytest.mark.parametrize("name", ["8x4", "6x5", "zeros"])
def test_envmap_taps_on_the_host(mi, O, name):
    """envmap_taps, the function the in-place commit deposits through, on 20 000 lookups.  (1) sum_k w_k data[tap_k] scale equals the host's envmap_eval_uv and -- at the
    direction of (u, v), for the lookups a direction can express -- the oracle's lookup, rtol 2e-6 (the leaf bar; the absolute part covers the float32 round trip uv ->
    direction -> uv of the oracle, worked out at the assertion).  (2) the deposit of random adjoints equals a float64 scatter whose halo
    folding is written independently (tests/envmap_grad_cases.taps_f64), 1e-5.  (3) no tap leaves [0, W) x [0, H)"""
    scale = 0.7
    scene = mi.load_dict(K.env_scene_dict(mi, name, scale=scale))
    img = K.env_image(name); h, w, _ = img.shape
    rng = np.random.default_rng(2)
    uv = _uv_pairs(w, rng); n = len(uv)
    g = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    idx, wgt, value, ev, dep = _taps(mi, scene, uv, g)
    assert idx.max() < w * h and np.all(idx // w < h) and np.all(wgt >= 0) and np.all(wgt <= 1) and np.allclose(wgt.sum(1), 1, atol=1e-6)
    assert np.allclose(value, ev, rtol=2e-6, atol=1e-7)
    # the float64 lookup through the independent taps: value and deposit
    want_v = np.zeros((n, 3)); want_d = np.zeros((h, w, 3))
    for i in range(n):
        for y, x, wk in K.taps_f64(uv[i, 0], uv[i, 1], w, h):
            want_v[i] += wk * img[y, x]
            want_d[y, x] += wk * g[i].astype(np.float64)
    assert np.allclose(value, want_v * scale, rtol=2e-6, atol=3e-6)       # (float32 texel coordinates against float64 ones: W + 2 ulps of a texel difference)
    e = K.rel_l2(dep, want_d); print("host deposit against the float64 scatter, %s: %.3g" % (name, e))
    assert np.abs(want_d).max() > 0 and e <= 1e-5
    # the oracle's lookup at the direction of (u, v): u in [0, 1), v in [0.1, 0.9] -- towards the poles acos() of a float32 cosine loses v (d v = d cos / (pi sin theta)) and
    # the comparison would measure the round trip; the pole rows are covered by the two comparisons above
    ok = (uv[:, 0] >= 0) & (uv[:, 0] < 1) & (uv[:, 1] >= 0.1) & (uv[:, 1] <= 0.9)
    dirs = K.uv_to_direction(uv[ok, 0], uv[ok, 1]).astype(np.float32)
    ref = O.EnvMap(img, scale=scale).eval(dirs)
    err = np.abs(value[ok] - ref) / np.maximum(np.abs(ref), 1e-3)
    print("taps against orc_envmap_eval, %s: max rel %.3g" % (name, err.max()))
    # the round trip's share: |du| <= 2^-23 at W texels per unit of u, |dv| <= 2^-24 / (pi sin(0.1 pi)) at H - 1 texels per unit, texel differences <= 1.2 * scale: 1.2e-6
    assert ok.sum() > 10000 and np.allclose(value[ok], ref, rtol=2e-6, atol=2e-6)


def test_surface_property_and_refusals(mi):
    """`envmap_gradients` is a property of `prb` alone; mi.render no longer calls the map's `data` / `scale` non-differentiable (the other placement keys keep their
    refusal); what the library refuses for the texel terms is said by name before anything touches a device"""
    import torch
    d = K.env_scene_dict(mi, "8x4", props={"envmap_gradients": True})
    scene = mi.load_dict(d)
    assert scene.integrator().envmap_gradients is True
    assert mi.load_dict(K.env_scene_dict(mi, "8x4")).integrator().envmap_gradients is False
    with pytest.raises(RuntimeError, match="envmap_gradients"):
        mi.load_dict(K.env_scene_dict(mi, "8x4", integrator="path", props={"envmap_gradients": True}))
    # the key set of the differentiable-parameter table stays what it was: the map's keys live with the placement keys
    assert not any(k.startswith("env.") for k in scene._param_keys())
    assert scene._pose_keys()["env.data"][0] == "env_data" and scene._pose_keys()["env.scale"][0] == "env_scale"
    # mi.render: requires_grad on the map's keys passes the "not differentiable" refusal (and then needs a device); a point light's position still meets it
    d2 = K.env_scene_dict(mi, "8x4"); d2["pt"] = {"type": "point", "position": [0.0, 0.5, 0.5], "intensity": {"type": "rgb", "value": 1.0}}
    sc2 = mi.load_dict(d2); params = mi.traverse(sc2)
    for key in ("env.data", "env.scale"):
        p = mi.traverse(sc2); p[key] = p[key].detach().clone().requires_grad_(True)
        try:
            mi.render(sc2, p, spp=1)
            reached = True
        except Exception as e:           # without a device the render itself fails -- with any message but the refusal
            reached = "not differentiable" not in str(e)
        assert reached, key
    params["pt.position"] = params["pt.position"].detach().clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="not differentiable parameters in hip_ad_rgb"):
        mi.render(sc2, params, spp=1)
    # refusals by name, raised before a device is needed
    grad_in = np.ones((K.FILM[1], K.FILM[0], 3), np.float32)
    for props, what in (({"max_depth": 13}, "envmap gradients: max_depth must not exceed 12"), ({"max_depth": -1}, "envmap gradients: max_depth must not exceed 12"),
                        ({"replay_cache": False}, "envmap gradients need the replay cache"), ({"shape_gradients": True}, "envmap gradients cannot be combined with vertex-position")):
        sc = mi.load_dict(K.env_scene_dict(mi, "8x4", props=dict({"envmap_gradients": True}, **props)))
        with pytest.raises(RuntimeError, match=what):
            sc.integrator().render_backward(sc, None, grad_in, seed=0, spp=1)
    tiny = mi.load_dict(K.env_scene_dict(mi, "8x4", image=np.full((2, 2, 3), 0.5, np.float32), props={"envmap_gradients": True}))
    with pytest.raises(RuntimeError, match="envmap gradients: an environment map smaller than 2 x 3"):
        tiny.integrator().render_backward(tiny, None, grad_in, seed=0, spp=1)
    # forward-mode tangents stay refused with the words they had
    with pytest.raises(Exception, match="not differentiable parameters of the `prb` forward mode|requires a HIP device"):
        scene.integrator().render_forward(scene, tangents={"env.data": np.zeros((4, 10, 3), np.float32)}, spp=1)


def test_gradient_layout_from_the_deposit(mi):
    """what render_backward returns for the map, from the library's deposit D (H x W x 3, real texels, without `scale`): `data` in the parameter's shape H x (W + 2) x 3 with
    ZERO halo columns and scale * D inside, `scale` = <D, data> in the shape mi.traverse shows -- also at scale = 0"""
    import torch
    for scale in (0.7, 0.0):
        scene = mi.load_dict(K.env_scene_dict(mi, "6x5", scale=scale))
        img = K.env_image("6x5"); h, w, _ = img.shape
        keys = {kind: (k, i) for k, (kind, i) in scene._pose_keys().items() if kind in ("env_data", "env_scale")}
        D = torch.as_tensor(np.random.default_rng(1).uniform(-1, 1, (h, w, 3)).astype(np.float32))
        out = scene._envmap_gradients(D, keys)
        params = mi.traverse(scene)
        gd = out["env.data"].numpy(); gs = out["env.scale"].numpy()
        assert gd.shape == tuple(params["env.data"].shape) == (h, w + 2, 3) and gs.shape == tuple(params["env.scale"].shape)
        assert not gd[:, 0].any() and not gd[:, -1].any() and np.allclose(gd[:, 1:-1], np.float32(scale) * D.numpy(), rtol=1e-7, atol=0)
        assert np.isclose(gs[0], (D.numpy().astype(np.float64) * img).sum(), rtol=1e-6) and gs[0] != 0


@pytest.mark.parametrize("name", ["8x4", "rotated"])
def test_oracle_is_affine_along_luminance_free_directions(mi, O, name):
    """the device test's reference: the oracle's same-seed `prb` render of data + eps delta, for delta with zero luminance at every texel (the map's sampling distribution
    does not move), is affine in eps -- I(+) + I(-) - 2 I(0) within 1e-5 of |I(0)| for every direction that test uses"""
    img = K.env_image(name); h, w, _ = img.shape

    def render(image):
        sc = mi.load_dict(K.env_scene_dict(mi, name, image=image))
        osc, sensor = O.scene_from_product(sc)
        return osc.render_prb(sensor, seed=5, spp=16, max_depth=4, rr_depth=3)[0].astype(np.float64)
    base = render(img)
    for label, delta in directions(img, name):
        up = render((img + delta).astype(np.float32)); down = render((img - delta).astype(np.float32))
        e = np.linalg.norm(up + down - 2 * base) / np.linalg.norm(base)
        print("affine along %s (%s): %.3g, |I+ - I-| / |I| = %.3g" % (label, name, e, np.linalg.norm(up - down) / np.linalg.norm(base)))
        assert e < 1e-5, label


def directions(img, name):
    """the luminance-free directions of the oracle comparison (eps = 1 folded in: |delta| <= 0.9 data keeps the texels positive): eight random ones on disjoint blocks, a single
    texel of row 0, column 0, column W - 1, all texels; the rotated map: one over all texels"""
    h, w, _ = img.shape; rng = np.random.default_rng(3)
    if name == "rotated":
        return [("all", K.luminance_free(img, np.ones((h, w), bool), rng))]
    out = [("block%d" % i, K.luminance_free(img, m, rng)) for i, m in enumerate(K.block_masks(h, w))]
    pole = np.zeros((h, w), bool); pole[0, 3] = True
    c0 = np.zeros((h, w), bool); c0[:, 0] = True
    cl = np.zeros((h, w), bool); cl[:, -1] = True
    return out + [("pole", K.luminance_free(img, pole, rng)), ("column0", K.luminance_free(img, c0, rng)), ("columnW-1", K.luminance_free(img, cl, rng)),
                  ("all", K.luminance_free(img, np.ones((h, w), bool), rng))]
