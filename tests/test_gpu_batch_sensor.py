"""The `batch` sensor on the GPU: device rays against the host twin, the forward film of `path` and `prb` against a film composed from oracle calls only
(tests/batch_cases.py), a batch of one child against the plain sensor, invariances (packet tracing, chunks, passes, replay cache), gradients (linearity in the
emitter's radiance, central differences of the product's own pinned forward render), the `aov` integrator, mi.render + autograd, refusals on the device path."""
import ctypes as C

import numpy as np
import pytest

from tests import aov_cases as A
from tests import batch_cases as B

pytestmark = pytest.mark.gpu

W, H, SPP = 96, 32, 4


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x).view(np.uint32)


@pytest.mark.parametrize("kinds", ["pp", "pop"])
def test_device_rays_equal_host_twin(mi, kinds):
    import torch
    b = mi.load_dict(B.batch_dict(mi, kinds, W, H))
    rng = np.random.default_rng(3)
    n = 20000
    n_children = len(kinds)
    pos = rng.uniform(0, 1, (2, n)).astype(np.float32)
    pos[0, :n_children + 1] = np.arange(n_children + 1, dtype=np.float32) / np.float32(n_children)      # the seams, 0 and 1
    pos[0, n_children + 1] = np.nextafter(np.float32(1), np.float32(0))
    pos[0, 4096:8192] = np.sort(pos[0, 4096:8192])          # waves whose lanes agree on the child (the scalar-load branch) next to waves that do not
    ray, _ = b.sample_ray(0.0, 0.0, torch.tensor(pos, device="cuda"))
    o, d, mt = b.sample_ray_host(pos)
    assert np.array_equal(_bits(ray.o), o.view(np.uint32)) and np.array_equal(_bits(ray.d), d.view(np.uint32)) and np.array_equal(_bits(ray.maxt), mt.view(np.uint32))


@pytest.mark.parametrize("kinds", ["pp", "pop"])
@pytest.mark.parametrize("rfilter", ["box", "gaussian"])
@pytest.mark.parametrize("itype", ["path", "prb"])
def test_forward_film_against_oracle_composition(mi, O, itype, rfilter, kinds):
    seed, md = 5, 4
    scene = mi.load_dict(B.batch_scene(mi, kinds, W, H, rfilter, SPP, integrator={"type": itype, "max_depth": md}))
    batch = scene.sensors()[0]
    osc, wide = O.scene_from_product(scene)
    want, lanes = B.oracle_batch_film(O, osc, batch, rfilter, seed, SPP, md, prb=(itype == "prb"))
    # conditions on the input, on the oracle side: no lane left out, every child gets its share of lanes, and its lanes see geometry
    assert lanes["n"] == W * H * SPP == lanes["index"].size
    for k in range(len(kinds)):
        mine = lanes["index"] == k
        assert mine.mean() >= 0.2 and lanes["hit"][mine].mean() >= 0.3, (k, mine.mean(), lanes["hit"][mine].mean())
    got = scene.integrator().render_film(scene, seed=seed, spp=SPP).cpu().numpy()
    assert got.shape == want.shape == (H, W, 4)
    wref = O.render_weights(wide, seed, SPP)[:, :, 3]
    e_w0, e_w1 = B.rel_l2(want[:, :, 3], wref), B.rel_l2(got[:, :, 3], wref)
    e_rgb = B.rel_l2(got[:, :, :3], want[:, :, :3])
    print(itype, rfilter, kinds, "weights: composition", e_w0, "device", e_w1, "rgb", e_rgb)
    assert e_w0 <= 2e-6 and e_w1 <= 2e-6          # first: the proof that the film positions were composed right
    assert np.linalg.norm(want[:, :, :3]) > 0 and e_rgb <= 1e-4


def _single_and_batch_of_one(mi, integrator, rfilter="gaussian", textured=True):
    d1 = mi.textured_cornell_box(res=32, tex_res=16, spp=SPP) if textured else mi.cornell_box()
    d1["integrator"] = dict(integrator)
    child = B.child_dicts(mi, "p")[0]
    film = {"type": "hdrfilm", "width": 40, "height": 32, "rfilter": {"type": rfilter}, "pixel_format": "rgb"}
    d1["sensor"] = dict(child, film=dict(film), sampler={"type": "independent", "sample_count": SPP})
    dB = dict(d1)
    dB["sensor"] = {"type": "batch", "film": dict(film), "sampler": {"type": "independent", "sample_count": SPP}, "only": dict(child)}
    return mi.load_dict(d1), mi.load_dict(dB)


def test_batch_of_one_equals_plain_sensor(mi):
    """Raw film and every gradient array, bit for bit.  Sums over more than one wave are accumulated with float atomics whose order is not fixed from run to run (two runs of
    the SAME plain render differ in the last bit of the filter-weight channel, which no camera ray enters), so the comparison is made wave by wave: every 64-lane range of
    the render is rendered and differentiated on its own, through the plain sensor and through the batch of one, and each pair must be equal in every bit.  Together the
    ranges cover every lane of the film.  The whole-film results are compared at the invariance bar (1e-6) as well."""
    integ = {"type": "prb", "max_depth": 5, "rr_depth": 5, "emitter_gradients": True}
    plain, batch = _single_and_batch_of_one(mi, integ)
    ip, ib = plain.integrator(), batch.integrator()
    total = 40 * 32 * SPP
    grad_in = np.random.default_rng(4).uniform(0.5, 1.5, (32, 40, 3)).astype(np.float32)
    nonzero_film = nonzero_grad = 0
    for lo in range(0, total, 64):
        fa = ip.render_film(plain, seed=3, spp=SPP, lanes=(lo, lo + 64)); fb = ib.render_film(batch, seed=3, spp=SPP, lanes=(lo, lo + 64))
        assert np.array_equal(_bits(fa), _bits(fb)), lo
        nonzero_film += int(float(fa[..., :3].abs().sum()) > 0)
        ga = ip.render_backward(plain, None, grad_in, seed=7, spp=SPP, lanes=(lo, lo + 64)); gb = ib.render_backward(batch, None, grad_in, seed=7, spp=SPP, lanes=(lo, lo + 64))
        assert sorted(ga) == sorted(gb) and len(ga) >= 3
        for k in ga:
            assert np.array_equal(_bits(ga[k]), _bits(gb[k])), (lo, k)
        nonzero_grad += int(any(float(g.abs().max()) > 0 for g in ga.values()))
    assert nonzero_film > total // 64 // 2 and nonzero_grad > total // 64 // 2
    fa = ip.render_film(plain, seed=3, spp=SPP).cpu().numpy(); fb = ib.render_film(batch, seed=3, spp=SPP).cpu().numpy()
    ga = ip.render_backward(plain, None, grad_in, seed=7, spp=SPP); gb = ib.render_backward(batch, None, grad_in, seed=7, spp=SPP)
    ea = np.concatenate([ga[k].cpu().numpy().ravel() for k in sorted(ga)]); eb = np.concatenate([gb[k].cpu().numpy().ravel() for k in sorted(gb)])
    print("whole film", B.rel_l2(fb, fa), "whole gradients", B.rel_l2(eb, ea), "film bits equal", np.array_equal(fa.view(np.uint32), fb.view(np.uint32)))
    assert B.rel_l2(fb, fa) <= 1e-6 and B.rel_l2(eb, ea) <= 1e-6
    # integrator reuse: a batch render, then a plain sensor, then the batch again on ONE integrator -- the child table is bound and cleared as needed
    it = mi.load_dict({"type": "path", "max_depth": 4})
    two = mi.load_dict(B.batch_scene(mi, "pp", 80, 32, "gaussian", SPP))
    r0 = it.render_film(two, seed=1, spp=SPP).cpu().numpy()
    p0 = it.render_film(plain, seed=1, spp=SPP).cpu().numpy()
    p1 = mi.load_dict({"type": "path", "max_depth": 4}).render_film(plain, seed=1, spp=SPP).cpu().numpy()
    r1 = it.render_film(two, seed=1, spp=SPP).cpu().numpy()
    assert B.rel_l2(p0, p1) <= 1e-6 and B.rel_l2(r1, r0) <= 1e-6 and B.rel_l2(r0[:, :40], p0) > 1e-2


def test_invariances(mi, O):
    import torch
    seed, md = 2, 5
    mk = lambda extra: mi.load_dict(dict({"type": "path", "max_depth": md}, **extra))
    Wi = 108          # sub-films of 36 pixels at 8 spp: every fifth 64-lane packet of a row holds the rays of two cameras
    scene = mi.load_dict(B.batch_scene(mi, "pop", Wi, H, "gaussian", 8))
    ref_integ = mk({"packet_tracing": True})
    ref = ref_integ.render_film(scene, seed=seed, spp=8).cpu().numpy(); st_ref = ref_integ.stats()
    for extra in ({"packet_tracing": False}, {"chunk_lanes": 4096}):
        it = mk(extra)
        out = it.render_film(scene, seed=seed, spp=8).cpu().numpy(); st = it.stats()
        print(extra, B.rel_l2(out, ref))
        assert B.rel_l2(out, ref) <= 1e-6
        assert st["paths"] == st_ref["paths"] and st["vertices"] == st_ref["vertices"]
    # samples_per_pass: pass p of a lane continues the sampler where pass p - 1 left it (integrator.cpp:349-356) -- composed from oracle calls pass by pass
    spp, per_pass = 8, 4
    batch = scene.sensors()[0]
    osc, wide = O.scene_from_product(scene)
    L = O.lib()
    want = np.zeros((H, Wi, 4), np.float32)
    lanes = B.oracle_batch_lanes(O, batch, seed, per_pass)
    n = lanes["n"]
    inc = np.zeros(n, np.uint64); v = (C.c_uint32 * 2)(); si = (C.c_uint64 * 2)()
    for i in range(n):
        L.orc_sample_tea_32(seed, i, 4, v); L.orc_pcg32_seed(v[0], v[1], si); inc[i] = si[1]
    for p in range(spp // per_pass):
        rgb, _, state = osc.integrator_sample(lanes["o"], lanes["d"], lanes["maxt"], seed=seed, lane_offset=0, state=lanes["state"], max_depth=md, rr_depth=5)
        want += B.film_put(O, wide, "gaussian", lanes, rgb)
        jit = np.zeros((2, n), np.float32); after = np.zeros(n, np.uint64)
        for i in range(n):
            si[0] = int(state[i]); si[1] = int(inc[i])
            jit[0, i] = L.orc_pcg32_next_float32(si); jit[1, i] = L.orc_pcg32_next_float32(si); after[i] = si[0]
        lanes = B.oracle_batch_lanes(O, batch, seed, per_pass, jitter=jit); lanes["state"] = after
    multi = mk({"samples_per_pass": per_pass}).render_film(scene, seed=seed, spp=spp).cpu().numpy()
    print("multi-pass vs oracle composition", B.rel_l2(multi[..., :3], want[..., :3]), B.rel_l2(multi[..., 3], want[..., 3]))
    assert B.rel_l2(multi[..., 3], want[..., 3]) <= 2e-6 and B.rel_l2(multi[..., :3], want[..., :3]) <= 1e-4
    # replay cache on / off for the adjoint
    got = []
    for cache in (True, False):
        sc = mi.load_dict(B.batch_scene(mi, "pop", W, H, "gaussian", SPP, integrator={"type": "prb", "max_depth": 6, "rr_depth": 5, "replay_cache": cache}, textured=True))
        grad_in = np.random.default_rng(4).uniform(0.5, 1.5, (H, W, 3)).astype(np.float32)
        grads = sc.integrator().render_backward(sc, None, grad_in, seed=2, spp=SPP)
        got.append(np.concatenate([grads[k].cpu().numpy().ravel() for k in sorted(grads)]))
    print("replay cache on / off", B.rel_l2(got[0], got[1]))
    assert np.abs(got[1]).max() > 0 and B.rel_l2(got[0], got[1]) <= 1e-5          # the bar of test_prb_replay_cache_is_transparent


def test_gradients_identity_and_central_differences(mi):
    """with rr_depth > max_depth the same-seed render is a polynomial in the albedos (linear in the radiance) and PRB's gradient is its exact derivative"""
    import torch
    seed, spp = 9, 16
    integ = {"type": "prb", "max_depth": 4, "rr_depth": 10, "emitter_gradients": True}
    scene = mi.load_dict(B.batch_scene(mi, "pop", W, H, "gaussian", spp, integrator=integ, textured=True))
    it = scene.integrator()
    grad_in = np.random.default_rng(8).uniform(0.5, 1.5, (H, W, 3)).astype(np.float32)
    loss = lambda: float((it.render(scene, seed=seed, spp=spp).cpu().numpy().astype(np.float64) * grad_in).sum())
    grads = it.render_backward(scene, None, grad_in, seed=seed, spp=spp)
    params = mi.traverse(scene)
    # (a) linear in the emitter's radiance: sum(grad * radiance) == sum(grad_in * image)
    k_rad = "light.emitter.radiance.value"
    lhs = float((grads[k_rad].cpu().numpy().astype(np.float64).ravel() * params[k_rad].cpu().numpy().astype(np.float64).ravel()).sum())
    rhs = loss()
    print("radiance identity", lhs, rhs, abs(lhs - rhs) / abs(rhs))
    assert abs(lhs - rhs) <= 2e-4 * abs(rhs)
    # (b) a constant albedo and the bitmap's texels along a fixed random direction, against central differences of the pinned forward render
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


@pytest.mark.parametrize("rfilter", ["box", "gaussian"])
def test_aov_depth_and_shape_index(mi, O, rfilter):
    seed = 6
    types = ["depth", "shape_index"]
    scene = mi.load_dict(B.batch_scene(mi, "pop", W, H, rfilter, SPP))
    batch = scene.sensors()[0]
    osc, wide = O.scene_from_product(scene)
    lanes = B.oracle_batch_lanes(O, batch, seed, SPP)
    vals, hit, _ = A.oracle_aovs(O, scene, osc, types, lanes["o"], lanes["d"], lanes["maxt"])
    rgb = np.zeros((3, lanes["n"]), np.float32); rgb[:2] = vals.astype(np.float32)
    want = B.film_put(O, wide, rfilter, lanes, rgb)
    aov = mi.load_dict({"type": "aov", "aovs": "dd:depth,si:shape_index"})
    got = aov.render(scene, seed=seed, spp=SPP, develop=False).cpu().numpy()
    assert got.shape == (H, W, 3) and hit.mean() > 0.3
    for c, name in enumerate(types):
        e = B.rel_l2(got[:, :, c], want[:, :, c]); print(rfilter, name, e)
        assert e <= 1e-4
    assert B.rel_l2(got[:, :, 2], want[:, :, 3]) <= 2e-6


def test_mi_render_autograd(mi):
    import torch
    scene = mi.load_dict(B.batch_scene(mi, "pp", 64, 32, "gaussian", 8, integrator={"type": "prb", "max_depth": 5}, textured=True))
    params = mi.traverse(scene)
    key = "white.reflectance.data"
    params[key].requires_grad_()
    img = mi.render(scene, params, spp=8, seed=1)
    assert tuple(img.shape) == (32, 64, 3)
    target = torch.full_like(img, 0.3)
    loss = ((img[:, :32] - target[:, :32]) ** 2).mean() + 2.0 * ((img[:, 32:] - target[:, 32:]) ** 2).mean()        # one term per view
    loss.backward()
    g = params[key].grad
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    x = img.detach().clone().requires_grad_()
    l2 = ((x[:, :32] - target[:, :32]) ** 2).mean() + 2.0 * ((x[:, 32:] - target[:, 32:]) ** 2).mean()
    l2.backward()
    seed_grad = mi.sample_tea_32(1, 1)[0]
    direct = scene.integrator().render_backward(scene, params, x.grad, seed=seed_grad, spp=8)[key]
    assert B.rel_l2(g.cpu().numpy(), direct.reshape(g.shape).cpu().numpy()) <= 1e-6


def test_device_path_refusals(mi):
    scene = mi.load_dict(B.batch_scene(mi, "pp", 64, 32, "gaussian", SPP))
    group = mi.DeviceGroup(scene, devices=[0], integrator=mi.load_dict({"type": "path", "max_depth": 3}))
    with pytest.raises(RuntimeError, match="batch sensor is not implemented by DeviceGroup"):
        group.render(spp=1)
    prb_group = mi.DeviceGroup(scene, devices=[0], integrator=mi.load_dict({"type": "prb", "max_depth": 3}))
    with pytest.raises(RuntimeError, match="batch sensor is not implemented by DeviceGroup"):
        prb_group.render_backward(np.ones((32, 64, 3), np.float32), spp=1)
    # the C entry: a crop window next to a bound child table, and a wide film whose width the child count does not divide
    it = mi.load_dict({"type": "path", "max_depth": 3})
    batch = scene.sensors()[0]
    it.render_film(scene, seed=0, spp=1)
    import copy
    import torch
    bad = copy.copy(batch); bad.har = type(batch.har).from_buffer_copy(bytes(batch.har)); bad.har.crop_width = 32
    film = torch.zeros((32, 64, 4), device="cuda")
    rc = mi.lib().har_render(scene._handle(), it._handle(), C.byref(bad.har), 0, 1, 0, 0, C.c_void_p(film.data_ptr()), None)
    assert rc != 0 and b"crop window or sample_border on the batch film" in mi.lib().har_last_error()
    three = mi.load_dict(B.batch_dict(mi, "ppp", 96, 32)).children_har()
    it3 = mi.load_dict({"type": "path", "max_depth": 3})
    mi.core.check(mi.lib().har_integrator_set_batch_sensors(it3._handle(), three, 3, None))
    rc = mi.lib().har_render(scene._handle(), it3._handle(), C.byref(batch.har), 0, 1, 0, 0, C.c_void_p(film.data_ptr()), None)
    msg = mi.lib().har_last_error()
    assert rc != 0 and b"BatchSensor: the horizontal resolution (currently 64) must be divisible by the number of child sensors (3)!" in msg, msg
