"""The `projector` emitter on the GPU: the device per-call entry against the host entry, the directional twin against the oracle (`path`, the `prb` primal, chunked,
two passes, next to an area light with sampling weights, inside a batch sensor) with its `scale` / irradiance gradients on both backward routes, a textured projector
on a tilted plane against the lane-by-lane composition from oracle entries (film, `Integrator.sample` lanes, per-texel gradient), a projector-lit box
against the host twin's film, the gradient identities of a render that is linear in texels and `scale`, and the shapes that can break a kernel."""
import ctypes as C

import numpy as np
import pytest

from tests import blend_cases as B
from tests import projector_cases as P

pytestmark = pytest.mark.gpu

RES, SPP = (32, 24), 16


def _ulp(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64); b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a); b = np.where(b < 0, -(b & 0x7fffffff), b)
    return int(np.abs(a - b).max())


def test_device_entry_equals_host_entry(mi):
    """the same HAR_HD function in a kernel and on the host over the 20 000 points of the CPU test: bit for bit (division and square root are correctly rounded on both
    sides and the build keeps contraction off); NaN / inf uv of lanes at z = 0 compare by bits too.  Every third lane off in a second call writes zeros."""
    worst = {}
    for name, cfg in P.configs(mi).items():
        pts = P.points(name, cfg, mi, 2500)
        scene = P.config_scene(mi, cfg)
        host = P.host_sample_direction(mi, scene, 0, pts); dev = P.device_sample_direction(mi, scene, 0, pts)
        for k in host:
            fin = np.isfinite(host[k]) & np.isfinite(dev[k])
            worst[k] = max(worst.get(k, 0), _ulp(np.where(fin, host[k], 0), np.where(fin, dev[k], 0)))
        print(name, {k: _ulp(np.where(np.isfinite(host[k]), host[k], 0), np.where(np.isfinite(dev[k]), dev[k], 0)) for k in host})
        for k in host:
            assert np.array_equal(host[k].view(np.uint32), dev[k].view(np.uint32)), (name, k, worst)
        mask = (np.arange(pts.shape[1]) % 3 != 0).astype(np.uint8)
        part = P.device_sample_direction(mi, scene, 0, pts, mask)
        for k in host:
            assert np.array_equal(part[k][..., mask == 1].view(np.uint32), host[k][..., mask == 1].view(np.uint32)) and np.all(part[k][..., mask == 0] == 0), (name, k)
    print("max ulp distance device / host:", worst)


# ---- the directional twin

S0, C0 = 1.7, (0.9, 0.5, 0.3)


def _twin_pair(mi, O, **kw):
    pj, dr = P.twin_lights(mi, kw.pop("s", S0), kw.pop("c", C0))
    scene = mi.load_dict(P.twin_scene(mi, pj, res=RES, spp=SPP, **kw))
    oracle, sensor = O.scene_from_product(mi.load_dict(P.twin_scene(mi, dr, res=RES, spp=SPP, **kw)))
    return scene, oracle, sensor


@pytest.mark.parametrize("max_depth", [2, 4, 8])
@pytest.mark.parametrize("integrator", ["path", "prb"])
def test_twin_render_equals_oracle(mi, O, integrator, max_depth):
    """the projector as the ONLY emitter (its record travels with the kernel arguments)"""
    scene, oracle, sensor = _twin_pair(mi, O, integrator=integrator, max_depth=max_depth)
    assert scene.emitters[0]["type"] == 8 and len(scene.emitters) == 1
    img = mi.render(scene, spp=SPP, seed=3).cpu().numpy()
    ref, ost = (oracle.render_path if integrator == "path" else oracle.render_prb)(sensor, seed=3, spp=SPP, max_depth=max_depth, rr_depth=5)
    err = P.rel_l2(img, ref); st = scene.integrator().stats()
    print("twin %s max_depth %d: rel L2 %.3g" % (integrator, max_depth, err))
    assert img.max() > 0 and err <= 1e-4
    assert (st["paths"], st["vertices"]) == (ost.paths, ost.vertices)


@pytest.mark.parametrize("variant", ["chunked", "two_passes", "area_weights", "area_uniform"])
def test_twin_variants_equal_oracle(mi, O, variant):
    kw = dict(integrator="path", max_depth=4)
    if variant == "chunked":
        kw["chunk_lanes"] = 4096
    if variant == "two_passes":
        kw["samples_per_pass"] = SPP // 2
    if variant.startswith("area"):
        kw["area"] = True
        if variant == "area_weights":
            kw["weights"] = (0.7, 1.8)
    scene, oracle, sensor = _twin_pair(mi, O, **kw)
    img = mi.render(scene, spp=SPP, seed=5).cpu().numpy()
    if variant == "two_passes":
        ref, ost = oracle.render_path_passes(sensor, seed=5, spp=SPP, spp_per_pass=SPP // 2, max_depth=4, rr_depth=5)
    else:
        ref, ost = oracle.render_path(sensor, seed=5, spp=SPP, max_depth=4, rr_depth=5)
    err = P.rel_l2(img, ref)
    print("twin %s: rel L2 %.3g" % (variant, err))
    assert err <= 1e-4
    if variant != "two_passes":
        st = scene.integrator().stats()
        assert (st["paths"], st["vertices"]) == (ost.paths, ost.vertices)


def test_twin_inside_a_batch_sensor(mi, O):
    """two views in one wavefront against the oracle's directional twin, composed lane by lane as tests/batch_cases.py composes a batch render (batch_select +
    orc_sensor_sample_ray per child, integrator_sample, orc_film_put on the wide film): 1e-4, weights 2e-6"""
    from tests import batch_cases as BC
    pj, dr = P.twin_lights(mi, S0, C0)
    scene = mi.load_dict(P.twin_scene(mi, pj, res=RES, spp=SPP, batch=True, max_depth=4))
    osc, _ = O.scene_from_product(mi.load_dict(P.twin_scene(mi, dr, res=RES, spp=SPP, batch=True, max_depth=4)))
    want, lanes = BC.oracle_batch_film(O, osc, scene.sensors()[0], "gaussian", 2, SPP, 4, rr_depth=5)
    film = scene.integrator().render_film(scene, seed=2, spp=SPP).cpu().numpy()
    e_rgb = P.rel_l2(film[:, :, :3], want[:, :, :3]); e_w = P.rel_l2(film[:, :, 3], want[:, :, 3])
    print("twin batch film / oracle composition: rgb %.3g, weights %.3g" % (e_rgb, e_w))
    assert film.shape == (RES[1], 2 * RES[0], 4) and want[:, :RES[0], :3].max() > 0 and want[:, RES[0]:, :3].max() > 0
    assert e_rgb <= 1e-4 and e_w <= 2e-6


# ---- the textured render, lane by lane, against the composition from oracle entries

@pytest.mark.parametrize("which", list(P.PLANE_MAPS))
@pytest.mark.parametrize("integrator", ["path", "prb"])
def test_textured_plane_equals_oracle_composition(mi, O, integrator, which):
    """the 32 x 24 x 16 film and the `Integrator.sample` lanes of the tilted plane under the textured projector against the composition (unit point light at the apex
    times pi s T(uv) d^2 / (z^2 cos) in float64): 1e-4, weights 2e-6"""
    import torch
    prb = integrator == "prb"
    comp = P.composed_plane(mi, O, which, 6, SPP, res=RES, prb=prb)
    pj, _, _ = P.plane_lights(mi, which)
    scene = mi.load_dict(P.plane_scene(mi, pj, res=RES, spp=SPP, integrator=integrator))
    film = scene.integrator().render_film(scene, seed=6, spp=SPP).cpu().numpy()
    e_rgb = P.rel_l2(film[:, :, :3], comp["film"][:, :, :3]); e_w = P.rel_l2(film[:, :, 3], comp["film"][:, :, 3])
    sampler = mi.Sampler({"sample_count": SPP, "seed": 0}); sampler.seed(6, comp["n"])
    sampler.state = torch.as_tensor(comp["state"].view(np.int64), device="cuda")
    spec, _ = scene.integrator().sample(scene, sampler, mi.Ray3f(comp["o"], comp["d"], comp["maxt"]))
    e_lane = P.rel_l2(spec.cpu().numpy(), comp["rgb"])
    print("plane %s %s: film rgb %.3g, weights %.3g, lanes %.3g (lit %d of %d hits)" % (which, integrator, e_rgb, e_w, e_lane, comp["lit"].sum(), comp["hit"].sum()))
    assert comp["lit"].sum() > 1000 and (comp["hit"] & ~comp["lit"]).sum() > 1000
    assert e_rgb <= 1e-4 and e_w <= 2e-6 and e_lane <= 1e-4


def test_nearest_map_texel_gradient_equals_restricted_composition(mi, O):
    """with the nearest map the composition restricted to the lanes that look texel t up gives d / d T_t: the product's per-texel gradient at 1e-3"""
    import torch
    which = "nearest44"
    comp = P.composed_plane(mi, O, which, 6, SPP, res=RES, prb=True)
    grad_in = np.random.default_rng(13).uniform(0.2, 1.0, (RES[1], RES[0], 3)).astype(np.float32)
    want = P.composed_texel_gradient(O, comp, grad_in, P.PLANE_MAPS[which][1][0].shape)
    pj, _, _ = P.plane_lights(mi, which)
    scene = mi.load_dict(P.plane_scene(mi, pj, res=RES, spp=SPP, integrator="prb"))
    it = scene.integrator(); it.light_texel_gradients = True
    g = it.render_backward(scene, mi.traverse(scene), torch.as_tensor(grad_in), seed=6, spp=SPP)
    got = g["light.irradiance.data"].cpu().numpy().astype(np.float64)
    err = np.abs(got - want).max() / np.abs(want).max()
    print("per-texel gradient / restricted composition: max err %.3g of max %.3g; texels lit %d of %d" % (err, np.abs(want).max(), (np.abs(want).sum(axis=2) > 0).sum(), want.shape[0] * want.shape[1]))
    assert (np.abs(want).sum(axis=2) > 0).sum() >= 8
    assert np.allclose(got, want, rtol=1e-3, atol=1e-3 * np.abs(want).max() * 1e-2)
    # ... and `scale`: the whole composition per unit of scale
    want_s = float((want * P.PLANE_MAPS[which][1][0].astype(np.float64)).sum()) / P.PLANE_SCALE
    assert np.isclose(float(g["light.scale"].cpu()[0]), want_s, rtol=1e-3)


@pytest.mark.parametrize("route", ["state_tape", "replay_cache"])
@pytest.mark.parametrize("case", ["plain", "scale_zero", "colour_zero"])
def test_twin_gradients_equal_oracle(mi, O, route, case):
    """grad_scale = grad_E . (pi c / h^2), grad_c = grad_E * (pi s / h^2) against render_prb_backward_emitters of the directional twin, at 1e-3 -- also where `scale`
    or the colour is exactly zero (the zero-contribution samples are traced)"""
    import torch
    s = 0.0 if case == "scale_zero" else S0
    c = (0.0, 0.0, 0.0) if case == "colour_zero" else C0
    kw = dict(integrator="prb", max_depth=4, s=s, c=c)
    if route == "replay_cache":
        kw["hide_emitters"] = True
    scene, oracle, sensor = _twin_pair(mi, O, **kw)
    if route == "replay_cache":
        oracle.set_hide_emitters(True)
    rng = np.random.default_rng(8); grad_in = rng.uniform(0.2, 1.0, (RES[1], RES[0], 3)).astype(np.float32)
    _, _, g_emit, _ = oracle.render_prb_backward_emitters(sensor, grad_in, seed=4, spp=SPP, max_depth=4, rr_depth=5)
    gE = g_emit[0].astype(np.float64)
    params = mi.traverse(scene)
    integ = scene.integrator(); integ.emitter_gradients = True
    g = integ.render_backward(scene, params, torch.as_tensor(grad_in), seed=4, spp=SPP)
    k = np.pi / P.TWIN_H ** 2
    want_s = float((gE * k * np.asarray(c, np.float64)).sum()); want_c = gE * k * s
    got_s = float(g["light.scale"].cpu().numpy()[0]); got_c = g["light.irradiance.value"].cpu().numpy().astype(np.float64)
    print("twin gradients %s %s: scale %.6g / %.6g, colour %s / %s" % (route, case, got_s, want_s, got_c, want_c))
    assert np.abs(gE).min() > 0
    assert abs(got_s - want_s) <= 1e-3 * max(abs(want_s), np.abs(gE * k).max() * 1e-3) and np.allclose(got_c, want_c, rtol=1e-3, atol=1e-3 * np.abs(gE * k).max() * 1e-3)
    assert np.isfinite(got_s) and np.isfinite(got_c).all()


# ---- a box lit by a textured projector

@pytest.fixture(scope="module")
def box(mi):
    import torch
    data = P.pattern()
    scene = mi.load_dict(P.projector_box(mi, data, scale=2.0, res=RES, spp=SPP, integrator="prb", max_depth=6))
    params = mi.traverse(scene)
    rng = np.random.default_rng(21); grad_in = torch.as_tensor(rng.uniform(0.1, 1.0, (RES[1], RES[0], 3)).astype(np.float32))
    integ = scene.integrator(); integ.light_texel_gradients = True
    img = integ.render(scene, seed=7, spp=SPP)
    g = integ.render_backward(scene, params, grad_in, seed=7, spp=SPP)
    return dict(scene=scene, params=params, data=data, grad_in=grad_in, img=img, g=g)


def test_box_film_equals_host_twin(mi):
    scene = mi.load_dict(P.projector_box(mi, P.pattern(), res=RES, spp=SPP, integrator="path", max_depth=6))
    film = scene.integrator().render(scene, seed=1, spp=SPP, develop=False).cpu().numpy()
    host, hst = B.host_render_stats(mi, scene, 1, SPP, 6, 5)
    st = scene.integrator().stats()
    err = P.rel_l2(film[:, :, :3], host[:, :, :3])
    print("box film device / host: rel L2 %.3g" % err)
    assert host[:, :, :3].max() > 0 and err <= 1e-4 and np.allclose(film[:, :, 3], host[:, :, 3], rtol=2e-6)
    assert (st["paths"], st["vertices"]) == (hst.paths, hst.vertices)


def test_linearity_identities(box):
    """the render is linear in the texels and in `scale` and no density depends on them: sum grad_data * data == scale * grad_scale == sum grad_in * image (same seed),
    at 2e-4 (the envmap bar)"""
    g = box["g"]
    a = float((g["projector.irradiance.data"].double().cpu() * np.asarray(box["data"], np.float64)).sum())
    b = 2.0 * float(g["projector.scale"].double().cpu()[0])
    c = float((box["grad_in"].double() * box["img"].double().cpu()).sum())
    print("identities: <g_data, data> %.8g, scale * g_scale %.8g, <grad_in, image> %.8g" % (a, b, c))
    assert c > 0 and abs(a - c) <= 2e-4 * c and abs(b - c) <= 2e-4 * c


def test_zero_texel_block_and_zero_scale(mi, box):
    """a block of exactly-zero texels keeps the identity, and its texels have the gradient of the same texels when lit (d / d texel does not depend on the texel);
    at scale = 0 the texel gradients vanish and grad_scale stays what it was per unit of scale"""
    import torch
    data = P.pattern(zero_block=True)
    scene = mi.load_dict(P.projector_box(mi, data, scale=2.0, res=RES, spp=SPP, integrator="prb", max_depth=6))
    integ = scene.integrator(); integ.light_texel_gradients = True
    img = integ.render(scene, seed=7, spp=SPP)
    g = integ.render_backward(scene, mi.traverse(scene), box["grad_in"], seed=7, spp=SPP)
    a = float((g["projector.irradiance.data"].double().cpu() * np.asarray(data, np.float64)).sum()); b = 2.0 * float(g["projector.scale"].cpu()[0])
    c = float((box["grad_in"].double() * img.double().cpu()).sum())
    assert abs(a - c) <= 2e-4 * c and abs(b - c) <= 2e-4 * c
    gz = g["projector.irradiance.data"].cpu().numpy(); gl = box["g"]["projector.irradiance.data"].cpu().numpy()
    assert np.abs(gz[2:6, 3:9]).max() > 0 and np.allclose(gz[2:6, 3:9], gl[2:6, 3:9], rtol=1e-3, atol=1e-3 * np.abs(gl).max())
    scene0 = mi.load_dict(P.projector_box(mi, P.pattern(), scale=0.0, res=RES, spp=SPP, integrator="prb", max_depth=6))
    i0 = scene0.integrator(); i0.light_texel_gradients = True
    g0 = i0.render_backward(scene0, mi.traverse(scene0), box["grad_in"], seed=7, spp=SPP)
    assert float(g0["projector.irradiance.data"].abs().max()) == 0.0
    assert np.isclose(float(g0["projector.scale"].cpu()[0]), float(box["g"]["projector.scale"].cpu()[0]), rtol=1e-3)


def test_central_differences_along_a_texel_direction(mi, box):
    """the same-seed `path` render is affine in the texels, so a central difference along a random direction is exact up to rounding: held at the 3 % bar"""
    rng = np.random.default_rng(2); direction = rng.uniform(-1, 1, box["data"].shape).astype(np.float32)
    eps = 0.05
    imgs = []
    for sign in (+1, -1):
        sc = mi.load_dict(P.projector_box(mi, box["data"] + sign * eps * direction, res=RES, spp=SPP, integrator="prb", max_depth=6))
        imgs.append(sc.integrator().render(sc, seed=7, spp=SPP).double().cpu())
    fd = float((box["grad_in"].double() * (imgs[0] - imgs[1]) / (2 * eps)).sum())
    ad = float((box["g"]["projector.irradiance.data"].double().cpu() * direction.astype(np.float64)).sum())
    print("central difference %.8g against adjoint %.8g: relative %.3g" % (fd, ad, abs(fd - ad) / abs(fd)))
    assert abs(fd - ad) <= 0.03 * abs(fd)


def test_one_channel_map_against_three_channel_gradients(mi, box):
    """a one-channel map is the three-channel map with equal channels: its gradient is the channel sum of the other's"""
    import torch
    mono = P.pattern()[:, :, :1].copy()
    out = []
    for data in (mono, np.repeat(mono, 3, axis=2)):
        sc = mi.load_dict(P.projector_box(mi, data, res=RES, spp=SPP, integrator="prb", max_depth=5))
        it = sc.integrator(); it.light_texel_gradients = True
        out.append(it.render_backward(sc, mi.traverse(sc), box["grad_in"], seed=9, spp=SPP)["projector.irradiance.data"].cpu().numpy())
    assert out[0].shape == mono.shape and out[1].shape == (mono.shape[0], mono.shape[1], 3)
    assert np.allclose(out[0][:, :, 0], out[1].sum(axis=2), rtol=1e-4, atol=1e-4 * np.abs(out[0]).max())


def test_state_tape_against_replay_cache(mi, box):
    sc = mi.load_dict(P.projector_box(mi, box["data"], res=RES, spp=SPP, integrator="prb", max_depth=6, replay_cache=True, hide_emitters=True))
    it = sc.integrator(); it.light_texel_gradients = True
    g = it.render_backward(sc, mi.traverse(sc), box["grad_in"], seed=7, spp=SPP)
    for k in ("projector.irradiance.data", "projector.scale"):
        a = g[k].cpu().numpy(); b = box["g"][k].cpu().numpy()
        assert np.allclose(a, b, rtol=1e-3, atol=1e-3 * np.abs(b).max()), k


@pytest.mark.parametrize("res,spp,tol", [((8, 8), 1, 0.0), (RES, SPP, 1e-4)])
def test_autograd_against_render_backward(mi, res, spp, tol):
    """mi.render + loss.backward() switches the texel terms on for the projector's keys: bit for bit on one wave, 1e-4 at the full size"""
    import torch
    data = P.pattern()
    sc = mi.load_dict(P.projector_box(mi, data, res=res, spp=spp, integrator="prb", max_depth=5))
    params = mi.traverse(sc)
    params["projector.irradiance.data"].requires_grad_(); params["projector.scale"].requires_grad_()
    img = mi.render(sc, params, spp=spp, seed=3, seed_grad=11)
    w = torch.as_tensor(np.random.default_rng(5).uniform(0.1, 1.0, tuple(img.shape)).astype(np.float32), device=img.device)
    (img * w).sum().backward()
    sc2 = mi.load_dict(P.projector_box(mi, data, res=res, spp=spp, integrator="prb", max_depth=5))
    it = sc2.integrator(); it.light_texel_gradients = True
    g = it.render_backward(sc2, mi.traverse(sc2), w, seed=11, spp=spp)
    for k in ("projector.irradiance.data", "projector.scale"):
        a = params[k].grad.cpu().numpy().reshape(-1); b = g[k].cpu().numpy().reshape(-1)
        assert np.abs(b).max() > 0
        if tol == 0.0:
            assert np.array_equal(a, b), k
        else:
            assert np.allclose(a, b, rtol=tol, atol=tol * np.abs(b).max()), k


def test_three_adam_steps_lower_the_loss(mi):
    import torch
    target_scene = mi.load_dict(P.projector_box(mi, P.pattern(seed=9), scale=1.5, res=RES, spp=SPP, integrator="prb", max_depth=4))
    target = mi.render(target_scene, spp=SPP, seed=1).detach()
    sc = mi.load_dict(P.projector_box(mi, np.full((12, 16, 3), 0.8, np.float32), scale=1.0, res=RES, spp=SPP, integrator="prb", max_depth=4))
    params = mi.traverse(sc)
    keys = ["projector.irradiance.data", "projector.scale"]
    for k in keys:
        params[k].requires_grad_()
    opt = torch.optim.Adam([params[k] for k in keys], lr=0.05)
    losses = []
    for step in range(4):
        opt.zero_grad()
        loss = ((mi.render(sc, params, spp=SPP, seed=step) - target) ** 2).mean()
        losses.append(float(loss))
        if step < 3:
            loss.backward(); opt.step(); params.update()
    print("losses:", losses)
    assert losses[3] < losses[0] and all(np.isfinite(losses))


# ---- shapes that can break a kernel

@pytest.mark.parametrize("res,spp", [((1, 1), 1), ((7, 5), 3)])
def test_odd_lane_counts(mi, res, spp):
    sc = mi.load_dict(P.projector_box(mi, P.pattern(), res=res, spp=spp, integrator="path", max_depth=5))
    film = sc.integrator().render(sc, seed=2, spp=spp, develop=False).cpu().numpy()
    host, _ = B.host_render_stats(mi, sc, 2, spp, 5, 5)
    assert np.isfinite(film).all() and np.allclose(film, host, rtol=1e-4, atol=1e-6)


def test_projector_that_lights_nothing(mi):
    """all geometry behind the projector (it looks up through the ceiling): a zero image, zero and finite gradients"""
    import torch
    d = P.projector_box(mi, P.pattern(), res=RES, spp=4, integrator="prb", max_depth=4)
    d["projector"]["to_world"] = mi.ScalarTransform4f().look_at(origin=[0.0, 1.5, 0.0], target=[0.0, 3.0, 0.1], up=[0, 0, 1])
    sc = mi.load_dict(d)
    it = sc.integrator(); it.light_texel_gradients = True
    img = it.render(sc, seed=0, spp=4)
    g = it.render_backward(sc, mi.traverse(sc), torch.ones((RES[1], RES[0], 3)), seed=0, spp=4)
    assert float(img.abs().max()) == 0.0
    for k in ("projector.irradiance.data", "projector.scale"):
        assert torch.isfinite(g[k]).all() and float(g[k].abs().max()) == 0.0


def test_camera_hits_on_the_apex_plane(mi):
    """a floor IN the projector's z = 0 plane: every camera hit has it_local.z == 0 (or a rounding of it) -- nothing is lit, nothing is NaN"""
    T = mi.ScalarTransform4f
    d = P.twin_scene(mi, {"type": "projector", "fov": 40.0, "to_world": T().look_at(origin=[0, 0, 0], target=[0, 0, -1], up=[0, 1, 0])}, res=RES, spp=4, max_depth=3)
    img = mi.render(mi.load_dict(d), spp=4, seed=0).cpu().numpy()
    assert np.isfinite(img).all()
    assert np.all(img[RES[1] // 2 + 4:, RES[0] // 2 - 2:RES[0] // 2 + 2] == 0)          # the floor's pixels in front of the camera


def test_updates_between_renders_equal_fresh_loads(mi):
    import torch
    data0, data1 = P.pattern(seed=3), P.pattern(seed=4)
    T = mi.ScalarTransform4f
    tw1 = T().look_at(origin=[0.2, 0.8, -0.1], target=[0.0, -1.0, 0.2], up=[0, 0, 1])
    sc = mi.load_dict(P.projector_box(mi, data0, scale=2.0, res=RES, spp=SPP, integrator="path", max_depth=4))
    mi.render(sc, spp=SPP, seed=1)
    params = mi.traverse(sc)
    params["projector.irradiance.data"] = torch.as_tensor(data1, device="cuda"); params["projector.scale"] = torch.tensor([0.75], device="cuda")
    params["projector.to_world"] = torch.as_tensor(np.asarray(tw1.matrix, np.float32).reshape(4, 4))
    params.update()
    a = mi.render(sc, spp=SPP, seed=1).cpu().numpy()
    d = P.projector_box(mi, data1, scale=0.75, res=RES, spp=SPP, integrator="path", max_depth=4); d["projector"]["to_world"] = tw1
    b = mi.render(mi.load_dict(d), spp=SPP, seed=1).cpu().numpy()
    assert b.max() > 0 and P.rel_l2(a, b) <= 1e-5
    # ... and a constant irradiance with its `scale`
    pj, _ = P.twin_lights(mi, 1.0, (1.0, 1.0, 1.0))
    sc = mi.load_dict(P.twin_scene(mi, pj, res=RES, spp=SPP, max_depth=3)); mi.render(sc, spp=SPP, seed=1)
    params = mi.traverse(sc)
    params["light.irradiance.value"] = torch.tensor([0.9, 0.5, 0.3], device="cuda"); params["light.scale"] = torch.tensor([1.7]); params.update()
    a = mi.render(sc, spp=SPP, seed=1).cpu().numpy()
    b = mi.render(mi.load_dict(P.twin_scene(mi, P.twin_lights(mi, 1.7, (0.9, 0.5, 0.3))[0], res=RES, spp=SPP, max_depth=3)), spp=SPP, seed=1).cpu().numpy()
    assert b.max() > 0 and P.rel_l2(a, b) <= 1e-6


def test_gpu_refusals_by_name(mi):
    import torch
    sc = mi.load_dict(P.projector_box(mi, P.pattern(), res=(8, 8), spp=1, integrator="prb", max_depth=3))
    params = mi.traverse(sc)
    it = sc.integrator()
    it.shape_gradients = ["floor.positions"]
    with pytest.raises(RuntimeError, match="projector: vertex-position gradients are not produced"):
        it.render_backward(sc, params, torch.ones((8, 8, 3)), seed=0, spp=1)
    it.shape_gradients = False
    with pytest.raises(RuntimeError, match="projector: render_forward is not implemented"):
        it.render_forward(sc, params, seed=0, spp=1, tangents={"white.reflectance.value": torch.ones(3)})
    with pytest.raises(RuntimeError, match="projector: render_forward\\(\\): forward-mode tangents of"):
        it.render_forward(sc, params, seed=0, spp=1, tangents={"projector.scale": torch.ones(1)})
    with pytest.raises(RuntimeError, match="projector: a DeviceGroup"):
        mi.DeviceGroup(sc, [0])
    # the C ABI's colour setters refuse a projector by name (its lowered colour is irradiance * scale): the record is replaced as a whole
    const = mi.load_dict(P.twin_scene(mi, P.twin_lights(mi, 1.7, (0.9, 0.5, 0.3))[0], res=(8, 8), spp=1))
    rgb = np.ones(3, np.float32); dev_rgb = torch.ones(3, device="cuda")
    for h, what in ((const, "the record's colour is irradiance \\* scale"), (sc, "irradiance is a bitmap")):
        assert mi.lib().har_scene_set_emitter_radiance(h._handle(), 0, P._fp(rgb)) != 0
        assert __import__("re").search("projector: .*" + what, (mi.lib().har_last_error() or b"").decode())
        assert mi.lib().har_scene_set_emitter_radiance_device(h._handle(), 0, dev_rgb.data_ptr(), None) != 0
        assert __import__("re").search("projector: .*" + what, (mi.lib().har_last_error() or b"").decode())
