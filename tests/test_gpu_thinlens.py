"""The `thinlens` sensor on the GPU: device rays against the host twin bit for bit, the forward film of `path` and `prb` against a film composed from oracle calls only
(tests/thinlens_cases.py), multi-pass and chunked renders, the wave-shared packet descent against the per-lane kernel, a batch of {thinlens, perspective}, the `aov`
integrator, a closed-form depth-of-field check without the oracle, `prb` gradients (linearity, central differences, record tape against the re-shading replay,
mi.render + autograd) and a device group of one."""
import numpy as np
import pytest

from tests import aov_cases as A
from tests import batch_cases as B
from tests import thinlens_cases as T

pytestmark = pytest.mark.gpu

W, H, SPP = 24, 16, 4
CROP = (3, 2, 17, 11)


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x).view(np.uint32)


def test_device_rays_equal_host_twin(mi):
    import torch
    pos, ap = T.sample_pairs(20000)
    tpos = torch.tensor(pos, device="cuda"); tap = torch.tensor(ap, device="cuda")
    lens = mi.load_dict(T.thinlens_dict(mi, 0.25, 2.5, film=T.film_dict(96, 64, crop=(10, 7, 50, 33))))
    batch = mi.load_dict(T.lens_batch_dict(mi, "tpt", 96, 32))
    for cam in (lens, batch):
        ray, _ = cam.sample_ray(0.0, 0.0, tpos, tap)
        o, d, mt = cam.sample_ray_host(pos, ap)
        assert np.array_equal(_bits(ray.o), o.view(np.uint32)) and np.array_equal(_bits(ray.d), d.view(np.uint32)) and np.array_equal(_bits(ray.maxt), mt.view(np.uint32)), cam.kind
        ray, _ = cam.sample_ray(0.0, 0.0, tpos)                     # no aperture sample: the centre of the lens
        o, d, mt = cam.sample_ray_host(pos)
        assert np.array_equal(_bits(ray.o), o.view(np.uint32)) and np.array_equal(_bits(ray.d), d.view(np.uint32)) and np.array_equal(_bits(ray.maxt), mt.view(np.uint32)), cam.kind
    o_ap = lens.sample_ray_host(pos, ap)[0]
    assert np.abs(o_ap - o_ap[:, :1]).max() > 0.1                   # the aperture sample does move the origins


@pytest.mark.parametrize("crop", [False, True])
@pytest.mark.parametrize("rfilter", ["box", "gaussian"])
def test_forward_film_against_oracle_composition(mi, O, rfilter, crop):
    seed, md = 5, 4
    film = T.film_dict(W, H, rfilter, crop=CROP if crop else None, sample_border=crop)
    counters = {}
    for itype in ("path", "prb"):
        scene = mi.load_dict(T.lens_scene(mi, T.thinlens_dict(mi, 0.12, 3.4, film=dict(film), spp=SPP), {"type": itype, "max_depth": md}))
        sensor = scene.sensors()[0]
        osc, _ = O.scene_from_product(scene)
        want, lanes = T.composed_film(mi, O, osc, sensor, rfilter, seed, SPP, md, prb=(itype == "prb"))
        sw, sh = sensor.film().sample_grid()
        assert lanes["n"] == sw * sh * SPP and lanes["hit"].mean() >= 0.5
        it = scene.integrator()
        got = it.render_film(scene, seed=seed, spp=SPP).cpu().numpy()
        assert got.shape == want.shape == ((CROP[3], CROP[2], 4) if crop else (H, W, 4))
        wref = O.render_weights(lanes["wide"], seed, SPP)[:, :, 3]
        e_w0, e_w1 = T.rel_l2(want[:, :, 3], wref), T.rel_l2(got[:, :, 3], wref)
        e_rgb = T.rel_l2(got[:, :, :3], want[:, :, :3])
        st = it.stats(); counters[itype] = (st["paths"], st["vertices"])
        print(itype, rfilter, "crop" if crop else "full", "weights: composition", e_w0, "device", e_w1, "rgb", e_rgb, st)
        assert e_w0 <= 2e-6 and e_w1 <= 2e-6
        assert np.linalg.norm(want[:, :, :3]) > 0 and e_rgb <= 1e-4
        assert st["paths"] == lanes["n"]
    assert counters["path"] == counters["prb"]


def test_multi_pass_and_chunks(mi, O):
    seed, md, spp, per_pass = 2, 5, 4, 2
    mk = lambda extra: mi.load_dict(dict({"type": "path", "max_depth": md}, **extra))
    scene = mi.load_dict(T.lens_scene(mi, T.thinlens_dict(mi, 0.12, 3.4, film=T.film_dict(W, H), spp=spp), {"type": "path", "max_depth": md}))
    sensor = scene.sensors()[0]
    osc, _ = O.scene_from_product(scene)
    # pass p of a lane continues the sampler where pass p - 1 left it (integrator.cpp:349-356): jitter AND aperture are drawn again
    want = np.zeros((H, W, 4), np.float32)
    lanes = T.lanes_of(mi, O, sensor, seed, per_pass)
    n = lanes["n"]
    for p in range(spp // per_pass):
        rgb, _, state = osc.integrator_sample(lanes["o"], lanes["d"], lanes["maxt"], seed=seed, lane_offset=0, state=lanes["state"], max_depth=md, rr_depth=5)
        want += B.film_put(O, lanes["wide"], "gaussian", lanes, rgb)
        lanes = T.lanes_of(mi, O, sensor, seed, per_pass, draws=T.next_draws(O, seed, n, 4, state=state))
    multi = mk({"samples_per_pass": per_pass}).render_film(scene, seed=seed, spp=spp).cpu().numpy()
    print("multi-pass vs oracle composition", T.rel_l2(multi[..., :3], want[..., :3]), T.rel_l2(multi[..., 3], want[..., 3]))
    assert T.rel_l2(multi[..., 3], want[..., 3]) <= 2e-6 and T.rel_l2(multi[..., :3], want[..., :3]) <= 1e-4
    single = mk({}).render_film(scene, seed=seed, spp=spp).cpu().numpy()
    assert T.rel_l2(multi[..., :3], single[..., :3]) > 1e-3           # (another stream than the one-pass render: the test above is not vacuous)
    ref_it = mk({}); chunk_it = mk({"chunk_lanes": 512})
    chunked = chunk_it.render_film(scene, seed=seed, spp=spp).cpu().numpy()
    whole = ref_it.render_film(scene, seed=seed, spp=spp).cpu().numpy()
    print("chunked vs unchunked", T.rel_l2(chunked, whole))
    assert T.rel_l2(chunked, whole) <= 1e-6 and chunk_it.stats()["vertices"] == ref_it.stats()["vertices"]


def test_packet_descent_against_per_lane_kernel(mi, O):
    """64 samples per pixel: a wave is one pixel, and its 64 origins lie all over a lens as wide as the box's blocks -- the packet's bounds must hold them all"""
    seed, md, spp = 4, 4, 64
    cam = T.thinlens_dict(mi, 0.6, 3.4, film=T.film_dict(8, 8), spp=spp)
    scene = mi.load_dict(T.lens_scene(mi, cam, {"type": "path", "max_depth": md}))
    sensor = scene.sensors()[0]
    out = {}
    for on in (True, False):
        it = mi.load_dict({"type": "path", "max_depth": md, "packet_tracing": on})
        out[on] = (it.render_film(scene, seed=seed, spp=spp).cpu().numpy(), it.stats())
    print("packets on / off", T.rel_l2(out[True][0], out[False][0]), out[True][1], out[False][1])
    assert T.rel_l2(out[True][0], out[False][0]) <= 1e-6
    assert out[True][1]["paths"] == out[False][1]["paths"] == 8 * 8 * spp and out[True][1]["vertices"] == out[False][1]["vertices"]
    osc, _ = O.scene_from_product(scene)
    want, lanes = T.composed_film(mi, O, osc, sensor, "gaussian", seed, spp, md)
    o = lanes["o"].reshape(3, 64, spp)
    spread = (o.max(axis=2) - o.min(axis=2)).max(axis=0)
    assert spread.min() > 0.6                                          # every pixel's origins span more than half the lens's diameter
    e = T.rel_l2(out[True][0][..., :3], want[..., :3])
    print("packets on vs composition", e, "hit", lanes["hit"].mean())
    assert lanes["hit"].mean() > 0.5 and e <= 1e-4


def test_batch_with_a_thin_lens_child(mi, O):
    seed, md = 7, 4
    for itype in ("path", "prb"):
        d = B.batch_scene(mi, "pp", 48, 16, "gaussian", SPP, integrator={"type": itype, "max_depth": md})
        d["sensor"] = T.lens_batch_dict(mi, "tp", 48, 16, "gaussian", SPP)
        scene = mi.load_dict(d)
        batch = scene.sensors()[0]
        osc, _ = O.scene_from_product(scene)
        want, lanes = T.composed_film(mi, O, osc, batch, "gaussian", seed, SPP, md, prb=(itype == "prb"))
        n = lanes["n"]
        assert np.array_equal(lanes["state"], T.lane_streams4(O, seed, n)[2])          # every lane, the perspective child's too, stands behind four draws
        right = lanes["px"] >= 0.5
        o0, d0, _ = batch.sample_ray_host(np.stack([lanes["px"], lanes["py"]]))
        assert np.array_equal(o0[:, right].view(np.uint32), lanes["o"][:, right].view(np.uint32)) and np.array_equal(d0[:, right].view(np.uint32), lanes["d"][:, right].view(np.uint32))
        assert np.abs(o0[:, ~right] - lanes["o"][:, ~right]).max() > 0.05                # the perspective child ignores the aperture sample, the lens does not
        got = scene.integrator().render_film(scene, seed=seed, spp=SPP).cpu().numpy()
        e_rgb = T.rel_l2(got[..., :3], want[..., :3]); e_w = T.rel_l2(got[..., 3], want[..., 3])
        print(itype, "batch {thinlens, perspective}: rgb", e_rgb, "weights", e_w, "hit", lanes["hit"].mean())
        assert lanes["hit"].mean() > 0.3 and e_w <= 2e-6 and e_rgb <= 1e-4


@pytest.mark.parametrize("rfilter", ["box", "gaussian"])
def test_aov_depth_and_shape_index(mi, O, rfilter):
    seed = 6
    types = ["depth", "shape_index"]
    scene = mi.load_dict(T.lens_scene(mi, T.thinlens_dict(mi, 0.2, 3.0, film=T.film_dict(W, H, rfilter), spp=SPP)))
    sensor = scene.sensors()[0]
    osc, _ = O.scene_from_product(scene)
    lanes = T.lanes_of(mi, O, sensor, seed, SPP)
    vals, hit, _ = A.oracle_aovs(O, scene, osc, types, lanes["o"], lanes["d"], lanes["maxt"])
    rgb = np.zeros((3, lanes["n"]), np.float32); rgb[:2] = vals.astype(np.float32)
    want = B.film_put(O, lanes["wide"], rfilter, lanes, rgb)
    aov = mi.load_dict({"type": "aov", "aovs": "dd:depth,si:shape_index"})
    got = aov.render(scene, seed=seed, spp=SPP, develop=False).cpu().numpy()
    assert got.shape == (H, W, 3) and hit.mean() > 0.5
    for c, name in enumerate(types):
        e = T.rel_l2(got[:, :, c], want[:, :, c]); print(rfilter, name, e)
        assert e <= 1e-4
    assert T.rel_l2(got[:, :, 2], want[:, :, 3]) <= 2e-6


def test_closed_form_plane_in_and_out_of_focus(mi):
    """No oracle: a textured emitter perpendicular to the optical axis.  At the focus distance every aperture ray of a film position meets the plane where the pinhole
    ray does, and the jitter is the first two draws of both streams: the thin-lens image IS the perspective image of the same seed.  At half the distance it is not."""
    seed, spp, focus, fov = 11, 16, 4.0, 40.0
    tex = np.random.default_rng(2).uniform(0.2, 3.0, (16, 16, 3)).astype(np.float32)
    Tr = mi.ScalarTransform4f

    def image(kind, depth):
        cam = {"type": kind, "fov": fov, "near_clip": 0.01, "far_clip": 100.0, "to_world": Tr().look_at(origin=[0, 0, 0], target=[0, 0, 1], up=[0, 1, 0]),
               "film": T.film_dict(32, 32, "box"), "sampler": {"type": "independent", "sample_count": spp}}
        if kind == "thinlens":
            cam.update(aperture_radius=0.3, focus_distance=focus)
        scene = mi.load_dict({"type": "scene", "integrator": {"type": "path", "max_depth": 1}, "sensor": cam,
                              "light": {"type": "rectangle", "to_world": Tr().translate([0, 0, depth]).rotate([0, 1, 0], 180.0).scale([3.0, 3.0, 1.0]),
                                        "emitter": {"type": "area", "radiance": {"type": "bitmap", "data": tex, "raw": True, "filter_type": "bilinear"}}}})
        return scene.integrator().render(scene, seed=seed, spp=spp).cpu().numpy()

    lens_in, pin_in = image("thinlens", focus), image("perspective", focus)
    assert pin_in.min() > 0.1                                          # the rectangle covers the whole view
    e_in = T.rel_l2(lens_in, pin_in)
    lens_out, pin_out = image("thinlens", 0.5 * focus), image("perspective", 0.5 * focus)
    assert lens_out.min() > 0.1 and pin_out.min() > 0.1
    e_out = T.rel_l2(lens_out, pin_out)
    print("in focus", e_in, "out of focus", e_out)
    assert e_in <= 1e-4
    assert e_out >= 10.0 * e_in and e_out > 1e-3


def _grad_scene(mi, integ, spp):
    return mi.load_dict(T.lens_scene(mi, T.thinlens_dict(mi, 0.15, 3.4, film=T.film_dict(W, H), spp=spp), integ, textured=True, spp=spp))


def test_gradients_identity_and_central_differences(mi):
    """with rr_depth > max_depth the same-seed render is a polynomial in the albedos (linear in the radiance) and PRB's gradient is its exact derivative"""
    import torch
    seed, spp = 9, 16
    integ = {"type": "prb", "max_depth": 4, "rr_depth": 10, "emitter_gradients": True}
    scene = _grad_scene(mi, integ, spp)
    it = scene.integrator()
    grad_in = np.random.default_rng(8).uniform(0.5, 1.5, (H, W, 3)).astype(np.float32)
    loss = lambda: float((it.render(scene, seed=seed, spp=spp).cpu().numpy().astype(np.float64) * grad_in).sum())
    grads = it.render_backward(scene, None, grad_in, seed=seed, spp=spp)
    params = mi.traverse(scene)
    k_rad = "light.emitter.radiance.value"
    lhs = float((grads[k_rad].cpu().numpy().astype(np.float64).ravel() * params[k_rad].cpu().numpy().astype(np.float64).ravel()).sum())
    rhs = loss()
    print("radiance identity", lhs, rhs, abs(lhs - rhs) / abs(rhs))
    assert abs(lhs - rhs) <= 2e-4 * abs(rhs)
    rng = np.random.default_rng(12)
    for key, eps in (("green.reflectance.value", 0.02), ("white.reflectance.data", 0.02)):
        x0 = params[key].detach().clone()
        v = torch.tensor(rng.uniform(-1, 1, tuple(x0.shape)).astype(np.float32), device=x0.device)
        vals = []
        for s in (+1.0, -1.0):
            params[key] = x0 + s * eps * v; params.update(); vals.append(loss())
        params[key] = x0; params.update()
        fd = (vals[0] - vals[1]) / (2 * eps)
        an = float((grads[key].cpu().numpy().astype(np.float64).reshape(-1) * v.cpu().numpy().astype(np.float64).reshape(-1)).sum())
        print(key, "central difference", fd, "prb", an, "relative error", abs(fd - an) / abs(fd))
        assert abs(fd) > 0 and abs(fd - an) <= 0.03 * abs(fd)


def test_record_tape_against_replay_and_autograd(mi):
    import torch
    grad_in = np.random.default_rng(4).uniform(0.5, 1.5, (H, W, 3)).astype(np.float32)
    got = []
    for cache in (True, False):          # the record tape (default) against the re-shading replay, which regenerates every lane from its index
        sc = _grad_scene(mi, {"type": "prb", "max_depth": 6, "rr_depth": 5, "replay_cache": cache}, SPP)
        grads = sc.integrator().render_backward(sc, None, grad_in, seed=2, spp=SPP)
        got.append(np.concatenate([grads[k].cpu().numpy().ravel() for k in sorted(grads)]))
    print("record tape / replay", T.rel_l2(got[0], got[1]))
    assert np.abs(got[1]).max() > 0 and T.rel_l2(got[0], got[1]) <= 1e-3
    scene = _grad_scene(mi, {"type": "prb", "max_depth": 5}, 8)
    params = mi.traverse(scene)
    key = "white.reflectance.data"
    params[key].requires_grad_()
    img = mi.render(scene, params, spp=8, seed=1)
    assert tuple(img.shape) == (H, W, 3)
    target = torch.full_like(img, 0.3)
    ((img - target) ** 2).mean().backward()
    g = params[key].grad
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    x = img.detach().clone().requires_grad_()
    ((x - target) ** 2).mean().backward()
    seed_grad = mi.sample_tea_32(1, 1)[0]
    direct = scene.integrator().render_backward(scene, params, x.grad, seed=seed_grad, spp=8)[key]
    assert T.rel_l2(g.cpu().numpy(), direct.reshape(g.shape).cpu().numpy()) <= 1e-6


def test_device_group_of_one(mi):
    scene = mi.load_dict(T.lens_scene(mi, T.thinlens_dict(mi, 0.12, 3.4, film=T.film_dict(W, H), spp=SPP), {"type": "path", "max_depth": 4}))
    group = mi.DeviceGroup(scene, devices=[0], integrator=mi.load_dict({"type": "path", "max_depth": 4}))
    a = group.render(seed=3, spp=SPP, develop=False)
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    b = scene.integrator().render_film(scene, seed=3, spp=SPP).cpu().numpy()
    print("device group of one vs har_render", T.rel_l2(a, b))
    assert a.shape == b.shape and np.linalg.norm(b[..., :3]) > 0 and T.rel_l2(a, b) <= 1e-6
