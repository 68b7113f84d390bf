"""`prb` gradients of an environment map's `data` and `scale` on the device (`envmap_gradients`, har_integrator_set_grad_envmap): homogeneity of degree one in the texels,
luminance-free texel directions against the oracle's same-seed renders, general directions against central differences of the product's own `path` render, the two replay
routes, mi.render's autograd path, and the switch left off.  Scenes: tests/envmap_grad_cases.py, 32 x 24 at 16 spp and one wave (8 x 8 at 1 spp)."""
import os

import numpy as np
import pytest

from tests import envmap_grad_cases as K
from tests.test_envmap_grad_cpu import directions

pytestmark = pytest.mark.gpu
SEED, SPP, MD, RR = 5, 16, 4, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "envmap_grad_switch_off.npz")


def _grad_in(film=K.FILM, seed=4):
    return np.random.default_rng(seed).uniform(0.5, 1.5, (film[1], film[0], 3)).astype(np.float32)


def _backward(scene, grad_in, seed=SEED, spp=SPP):
    return {k: v.detach().cpu().numpy() for k, v in scene.integrator().render_backward(scene, None, grad_in, seed=seed, spp=spp).items()}


def _close(a, b, tol):
    return abs(a - b) <= tol * max(abs(a), abs(b))


@pytest.mark.parametrize("hide", [False, True], ids=["tape", "cache"])
@pytest.mark.parametrize("name", K.MAPS)
def test_homogeneity_in_the_texels(mi, name, hide):
    """a scene lit by the map alone is homogeneous of degree one in the texels and in `scale`, and scaling either leaves the sampling distribution alone: with the backward
    pass on the primal's seed, sum grad_data . data == scale * grad_scale == sum grad_in . image (2e-4, the bar of this identity for a light's texels).  State tape, and the
    lane-indexed cache (hide_emitters: no depth-0 escape term, the identity holds against the hidden-emitter image)"""
    scale = 0.7
    scene = mi.load_dict(K.env_scene_dict(mi, name, scale=scale, hide=hide, props={"envmap_gradients": True}))
    grad_in = _grad_in()
    image = mi.render(scene, spp=SPP, seed=SEED).cpu().numpy().astype(np.float64)
    g = _backward(scene, grad_in)
    data = K.halo(K.env_image(name)).astype(np.float64)
    assert g["env.data"].shape == data.shape and not g["env.data"][:, 0].any() and not g["env.data"][:, -1].any()
    a = float((g["env.data"].astype(np.float64)[:, 1:-1] * data[:, 1:-1]).sum()); b = scale * float(g["env.scale"][0]); c = float((grad_in * image).sum())
    print("homogeneity %s %s: data %.9g scale %.9g image %.9g" % (name, "cache" if hide else "tape", a, b, c))
    assert c > 0 and _close(a, c, 2e-4) and _close(b, c, 2e-4) and _close(a, b, 2e-4)
    if name == "zeros":          # texels that are exactly 0 contribute nothing and still have a derivative
        assert np.abs(g["env.data"][:, 1:-1][K.ZERO_BLOCK]).min() > 0


@pytest.mark.parametrize("hide", [False, True], ids=["tape", "cache"])
def test_homogeneity_with_an_area_light(mi, hide):
    """... with an area light next to the map and `emitter_gradients`: sum grad_data . data + sum_c radiance_c grad_radiance_c == sum grad_in . image"""
    scene = mi.load_dict(K.env_scene_dict(mi, "8x4", area=True, hide=hide, props={"envmap_gradients": True, "emitter_gradients": True}))
    grad_in = _grad_in()
    image = mi.render(scene, spp=SPP, seed=SEED).cpu().numpy().astype(np.float64)
    g = _backward(scene, grad_in)
    data = K.halo(K.env_image("8x4")).astype(np.float64)
    key = [k for k, v in scene._param_keys().items() if v[0] == "emit"]
    assert len(key) == 1
    rad = np.float64([e for e in scene.emitters if e["type"] != 2][0]["radiance"])
    a = float((g["env.data"].astype(np.float64) * data).sum()); e = float((g[key[0]].astype(np.float64).reshape(3) * rad).sum()); c = float((grad_in * image).sum())
    print("homogeneity with an area light (%s): data %.9g radiance %.9g image %.9g" % ("cache" if hide else "tape", a, e, c))
    assert a > 0 and e > 0 and _close(a + e, c, 2e-4)
    assert _close(0.7 * float(g["env.scale"][0]), a, 2e-4)


@pytest.mark.parametrize("name", ["8x4", "rotated"])
def test_luminance_free_directions_against_the_oracle(mi, O, name):
    """the map's sampling distribution is built from the texels' luminance alone (envmap.cpp:468-528): along a direction delta whose luminance vanishes at every texel the
    same-seed render is affine, so <grad_data, delta> == sum grad_in . (I(data + delta) - I(data - delta)) / 2 with I the ORACLE's `prb` primal of the two perturbed scenes
    (tests/test_envmap_grad_cpu.py checks that it is affine), held to 1e-3.  delta = 0.9 data at most per channel, the largest step that keeps the texels positive;
    |I+ - I-| / |I| is printed: it reaches 0.3 for the directions over many bright texels and cannot for a block of four texels or a single pole texel of a map whose
    texels lie in [0.2, 1.2] (docs/parity.md).  Eight disjoint blocks, a texel of row 0 (the pole clamp), column 0 and column W - 1 (the seam: half of their deposit arrives
    through the halo), all texels; the rotated map"""
    img = K.env_image(name)
    scene = mi.load_dict(K.env_scene_dict(mi, name, props={"envmap_gradients": True}))
    grad_in = _grad_in()
    g = _backward(scene, grad_in)["env.data"].astype(np.float64)[:, 1:-1]

    def oracle(image):
        osc, sensor = O.scene_from_product(mi.load_dict(K.env_scene_dict(mi, name, image=image)))
        return osc.render_prb(sensor, seed=SEED, spp=SPP, max_depth=MD, rr_depth=RR)[0].astype(np.float64)
    base = oracle(img)
    parity = K.rel_l2(mi.render(scene, spp=SPP, seed=SEED).cpu().numpy(), base)
    print("primal against the oracle (%s): %.3g" % (name, parity))
    assert parity < 1e-4
    for label, delta in directions(img, name):
        up = oracle((img + delta).astype(np.float32)); down = oracle((img - delta).astype(np.float32))
        d32 = ((img + delta).astype(np.float32).astype(np.float64) - (img - delta).astype(np.float32)) / 2          # the step the two float32 maps really take
        want = float((grad_in * (up - down)).sum()) / 2; got = float((g * d32).sum())
        print("luminance-free %s (%s): gradient %.9g oracle %.9g rel %.3g, |I+ - I-| / |I| = %.3g" % (label, name, got, want, abs(got - want) / abs(want), np.linalg.norm(up - down) / np.linalg.norm(base)))
        assert want != 0 and abs(got - want) <= 1e-3 * abs(want), label


def test_channels_of_a_grey_scene(mi):
    """colourless materials and a grad_in that treats the channels alike: the three channel gradients of every texel are equal (1e-5 of the largest) -- with the directions
    above, which fix two components per texel, this pins the third"""
    scene = mi.load_dict(K.env_scene_dict(mi, "8x4", grey=True, props={"envmap_gradients": True}))
    gi = np.repeat(_grad_in()[:, :, :1], 3, axis=2)
    g = _backward(scene, gi)["env.data"][:, 1:-1].astype(np.float64)
    print("grey scene, channel spread / largest: %.3g" % (np.abs(g - g[:, :, :1]).max() / np.abs(g).max()))
    assert g.max() > 0 and np.abs(g - g[:, :, :1]).max() <= 1e-5 * np.abs(g).max()


@pytest.mark.parametrize("case", ["random", "zero_block"])
def test_general_directions_against_central_differences(mi, case):
    """directions that move the sampling distribution: same-seed central differences of the product's own `path` render, rr_depth > max_depth (no roulette), 3 % -- the bar
    of this kind of check (a light's texels, `thinlens`, `batch`).  The per-seed derivative equals the detached gradient in expectation only; the spp and the measured
    figures are in docs/parity.md.  `zero_block`: a non-negative direction on the 2 x 2 block of texels that are exactly 0, whose gradient must not vanish"""
    spp = 256
    name = "zeros" if case == "zero_block" else "8x4"
    img = K.env_image(name); rng = np.random.default_rng(8)
    if case == "zero_block":
        delta = np.zeros_like(img, dtype=np.float64); delta[K.ZERO_BLOCK] = rng.uniform(0.5, 1.0, (2, 2, 3)); eps = 0.25
    else:
        delta = rng.uniform(-1.0, 1.0, img.shape) * img; eps = 0.1
    scene = mi.load_dict(K.env_scene_dict(mi, name, max_depth=MD, rr_depth=10, spp=spp, props={"envmap_gradients": True}))
    grad_in = _grad_in()
    g = _backward(scene, grad_in, seed=1, spp=spp)["env.data"].astype(np.float64)[:, 1:-1]

    def path(image):
        sc = mi.load_dict(K.env_scene_dict(mi, name, image=image.astype(np.float32), integrator="path", max_depth=MD, rr_depth=10, spp=spp))
        return mi.render(sc, spp=spp, seed=2).cpu().numpy().astype(np.float64)
    want = float((grad_in * (path(img + eps * delta) - path(img - eps * delta))).sum()) / (2 * eps); got = float((g * delta).sum())
    print("general direction %s at %d spp: gradient %.9g central difference %.9g rel %.3g" % (case, spp, got, want, abs(got - want) / abs(want)))
    if case == "zero_block":
        assert np.abs(g[K.ZERO_BLOCK]).min() > 0
    assert abs(got - want) <= 0.03 * abs(want)


def test_state_tape_against_the_lane_indexed_cache(mi):
    """no camera ray escapes (a back wall): hide_emitters changes nothing but the route -- the lane-indexed cache instead of the state tape.  1e-3"""
    grad_in = _grad_in(); out = []
    for hide in (False, True):
        scene = mi.load_dict(K.env_scene_dict(mi, "6x5", closed=True, hide=hide, props={"envmap_gradients": True}))
        out.append(_backward(scene, grad_in))
    assert np.abs(out[0]["env.data"]).max() > 0
    print("state tape against lane-indexed cache: data %.3g scale %.3g" % (K.rel_l2(out[1]["env.data"], out[0]["env.data"]), K.rel_l2(out[1]["env.scale"], out[0]["env.scale"])))
    assert K.rel_l2(out[1]["env.data"], out[0]["env.data"]) < 1e-3 and K.rel_l2(out[1]["env.scale"], out[0]["env.scale"]) < 1e-3


@pytest.mark.parametrize("film,spp", [((8, 8), 1), (K.FILM, SPP)], ids=["one_wave", "32x24x16"])
def test_autograd_against_render_backward(mi, film, spp):
    """mi.render + loss.backward() with requires_grad on the map's keys switches the term on for that call only and returns what render_backward returns on the differential
    seed: bit for bit on one wave, 1e-4 at 32 x 24 x 16 (the order of the atomic adds: `blendbsdf` in docs/parity.md)"""
    import torch
    scene = mi.load_dict(K.env_scene_dict(mi, "6x5", film=film, spp=spp))
    params = mi.traverse(scene)
    assert params.flags("env.data") == mi.ParamFlags.Differentiable and params.flags("env.scale") == mi.ParamFlags.Differentiable
    gi = torch.as_tensor(_grad_in(film), device="cuda")
    for k in ("env.data", "env.scale"):
        params[k] = params[k].detach().clone().requires_grad_(True)
    img = mi.render(scene, params, spp=spp, seed=SEED)
    (img * gi).sum().backward()
    assert not scene.integrator().envmap_gradients
    scene.integrator().envmap_gradients = True
    ref = _backward(scene, gi.cpu().numpy(), seed=mi.sample_tea_32(SEED, 1)[0], spp=spp)
    for k in ("env.data", "env.scale"):
        got = params[k].grad.cpu().numpy()
        assert got.shape == tuple(params[k].shape) and np.abs(got).max() > 0
        if spp == 1:
            assert np.array_equal(got, ref[k].reshape(got.shape)), k
        else:
            print("autograd against render_backward, %s: %.3g" % (k, K.rel_l2(got, ref[k].reshape(got.shape))))
            assert K.rel_l2(got, ref[k].reshape(got.shape)) < 1e-4, k
    # the other placement keys keep their refusal
    params["sensor.to_world"] = params["sensor.to_world"].detach().clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="not differentiable parameters in hip_ad_rgb"):
        mi.render(scene, params, spp=spp, seed=SEED)


def test_three_steps_lower_the_loss(mi):
    """Adam on the texels and `scale`, params.update() between the steps: an L2 loss against a render of other texels goes down"""
    import torch
    scene = mi.load_dict(K.env_scene_dict(mi, "8x4", scale=0.5))
    params = mi.traverse(scene)
    params["env.data"] = torch.as_tensor(K.halo(K.env_image("8x4", seed=12)), device="cuda"); params["env.scale"] = torch.tensor([0.9], device="cuda"); params.update()
    target = mi.render(scene, spp=64, seed=1).detach()
    data = torch.as_tensor(K.halo(K.env_image("8x4")), device="cuda").requires_grad_(True); scale = torch.tensor([0.5], device="cuda", requires_grad=True)
    opt = torch.optim.Adam([data, scale], lr=0.03)
    losses = []
    for step in range(3):
        params["env.data"] = data; params["env.scale"] = scale; params.update()
        loss = ((mi.render(scene, params, spp=64, seed=1 + step) - target) ** 2).mean()
        opt.zero_grad(); loss.backward(); opt.step()
        with torch.no_grad():
            data.clamp_(min=1e-3)
        losses.append(float(loss.detach()))
    print("three Adam steps:", losses)
    assert data.grad is not None and float(data.grad.abs().max()) > 0 and float(scale.grad.abs().max()) > 0
    assert losses[2] < losses[0]


def test_switch_off_is_the_parent(mi):
    """without `envmap_gradients` render_backward of an environment-lit scene returns the keys it returned before the feature existed and, on one wave, the same bits
    (tests/golden/envmap_grad_switch_off.npz: recorded from the commit before it); and a bitmap on a wall of the same scene gets the same texel gradients with the switch on"""
    gold = np.load(GOLDEN)
    wall = np.random.default_rng(6).uniform(0.2, 0.8, (6, 6, 3)).astype(np.float32)
    scene = mi.load_dict(K.env_scene_dict(mi, "6x5", film=(8, 8), spp=1, wall=wall))
    off = _backward(scene, _grad_in((8, 8)), spp=1)
    assert sorted(off) == sorted(gold.files)
    for k in off:
        # the flat colours: bit for bit.  The wall's texels are accumulated with float atomics whose order is not fixed even within one wave: two backward passes of the
        # commit before the feature, in one process, differ in one channel of one texel by one ulp (and so do two of this one) -- held to 1e-6 instead
        if k.endswith(".data"):
            assert np.abs(gold[k]).max() > 0 and K.rel_l2(off[k], gold[k]) < 1e-6, k
        else:
            assert np.array_equal(off[k], gold[k]), k
    grad_in = _grad_in(); pair = []
    for on in (False, True):
        sc = mi.load_dict(K.env_scene_dict(mi, "6x5", wall=wall, props={"envmap_gradients": on}))
        pair.append(_backward(sc, grad_in))
    assert sorted(set(pair[1]) - set(pair[0])) == ["env.data", "env.scale"] and sorted(off) == sorted(pair[0])
    key = [k for k in pair[0] if k.endswith("reflectance.data")][0]
    print("wall texels, switch on against off: %.3g" % K.rel_l2(pair[1][key], pair[0][key]))
    assert np.abs(pair[0][key]).max() > 0 and K.rel_l2(pair[1][key], pair[0][key]) < 1e-6


def test_library_refusals_name_the_feature(mi, monkeypatch):
    """what the library itself refuses for the texel terms (har_integrator_set_grad_envmap, har_render_backward); the Python surface says the same before it gets there
    (Integrator._check_envmap_routes, switched off here so that the library answers)"""
    from mitsuba3_amd.core import lib, Integrator
    path = mi.load_dict(K.env_scene_dict(mi, "8x4", film=(8, 8), spp=1, integrator="path"))
    mi.render(path, spp=1)
    assert lib().har_integrator_set_grad_envmap(path.integrator()._handle(), 1) != 0 and b"envmap gradients are computed by the `prb` integrator" in lib().har_last_error()
    monkeypatch.setattr(Integrator, "_check_envmap_routes", lambda self, scene, keys: None)
    for props, what in (({"max_depth": 13}, "envmap gradients: max_depth must not exceed 12"), ({"replay_cache": False}, "envmap gradients need the replay cache"),
                        ({"shape_gradients": True}, "envmap gradients need the replay cache and cannot be combined with vertex-position gradients")):
        scene = mi.load_dict(K.env_scene_dict(mi, "8x4", film=(8, 8), spp=1, props=dict({"envmap_gradients": True}, **props)))
        with pytest.raises(RuntimeError, match=what):
            _backward(scene, _grad_in((8, 8)), spp=1)
    tiny = mi.load_dict(K.env_scene_dict(mi, "8x4", film=(8, 8), spp=1, image=np.full((2, 2, 3), 0.5, np.float32), props={"envmap_gradients": True}))
    with pytest.raises(RuntimeError, match="envmap gradients: an environment map smaller than 2 x 3"):
        _backward(tiny, _grad_in((8, 8)), spp=1)
