"""`mask` on the GPU: the kernels against the host entries and the oracle -- per-call parity, same-stream renders through identical geometry, partial opacity
statistically, valid_ray per lane and on an `rgba` film, prb gradients of the opacity and of the nested colours, the aov channels.  Shapes are small: every test takes
a few seconds."""
import numpy as np
import pytest

from tests import blend_cases as B
from tests import mask_cases as M
from tests.test_gpu_boundary import rel_l2

pytestmark = pytest.mark.gpu
ALL = M.ALL
LEAF = dict(rtol=2e-6, atol=1e-9)


# ------------------------------------------------------------------------------------------------ 1. device against host

@pytest.mark.parametrize("opacity", M.OPACITY_NAMES)
@pytest.mark.parametrize("nested", M.NESTED_NAMES)
def test_device_against_host(mi, nested, opacity):
    """har_bsdf_eval_pdf / _eval / _pdf / _sample on the tuples of the CPU composition test against the host entries (which that test pins to the oracle), every context,
    with an `active` mask; sampled_type and sampled_component equal on every lane"""
    bsdf = mi.load_dict(M.mask_dict(mi, nested, opacity)); scene, ib = B.bound(mi, bsdf)
    wi, uv, wo, s1, s2, o = B.tuples(opacity)
    active = np.arange(wi.shape[1]) % 5 != 0
    si = type("SI", (), dict(wi=wi, uv=uv))()
    for ctx in M.contexts(nested):
        c = mi.BSDFContext(*ctx)
        val, pdf = bsdf.eval_pdf(c, si, wo, active)
        hv, hp = B.host_eval_pdf(mi, scene, ib, ctx, wi, uv, wo, active)
        val = val.cpu().numpy(); pdf = pdf.cpu().numpy()
        assert np.allclose(val, hv, **LEAF) and np.allclose(pdf, hp, **LEAF), (nested, opacity, ctx, float(np.abs(val - hv).max()), float(np.abs(pdf - hp).max()))
        assert np.array_equal(bsdf.eval(c, si, wo, active).cpu().numpy(), val) and np.array_equal(bsdf.pdf(c, si, wo, active).cpu().numpy(), pdf)
        bs, wgt = bsdf.sample(c, si, s1, s2, active)
        h = B.host_sample(mi, scene, ib, ctx, wi, uv, s1, s2, active)
        assert np.array_equal(bs.sampled_type.cpu().numpy().astype(np.uint32), h["sampled_type"]) and np.array_equal(bs.sampled_component.cpu().numpy().astype(np.uint32), h["sampled_component"])
        assert np.array_equal(bs.eta.cpu().numpy(), h["eta"])
        assert np.allclose(bs.wo.cpu().numpy(), h["wo"], rtol=2e-6, atol=1e-7) and np.allclose(bs.pdf.cpu().numpy(), h["pdf"], **LEAF)
        assert np.allclose(wgt.cpu().numpy(), h["weight"], rtol=5e-6, atol=1e-9), (nested, opacity, ctx)
        m = ~active
        assert (val[:, m] == 0).all() and (pdf[m] == 0).all() and (wgt.cpu().numpy()[:, m] == 0).all() and (bs.wo.cpu().numpy()[:, m] == 0).all()
    assert (bs.sampled_type.cpu().numpy() == M.NULL).any()


# ------------------------------------------------------------------------------------------------ 2. device renders against the oracle through identical geometry

RES, SPP = (32, 24), 16


def _render_vs_oracle(mi, O, product, twin, integrator, seed=3, passes=None, hide=False):
    scene = mi.load_dict(product); rscene = mi.load_dict(twin)
    osc, osensor = O.scene_from_product(rscene); osc.set_hide_emitters(hide)
    it = scene.integrator()
    img = mi.render(scene, spp=SPP, seed=seed).cpu().numpy()
    if passes:
        want, ost = osc.render_path_passes(osensor, seed=seed, spp=SPP, spp_per_pass=passes, max_depth=it.max_depth, rr_depth=it.rr_depth)
    else:
        want, ost = (osc.render_path if integrator == "path" else osc.render_prb)(osensor, seed=seed, spp=SPP, max_depth=it.max_depth, rr_depth=it.rr_depth)
    st = it.stats()
    assert np.isfinite(img).all() and img.max() > 0
    return rel_l2(img, want), (st["paths"], st["vertices"]), (ost.paths, ost.vertices)


@pytest.mark.parametrize("integrator,variant", [(i, v) for i in ("path", "prb") for v in ("plain", "chunked", "passes", "twosided", "instanced", "two_layers")
                                                if not (i == "prb" and v == "passes")])          # (`prb` renders one wavefront and refuses `samples_per_pass`)
def test_device_render_binary_tiles(mi, O, integrator, variant):
    """opacity texels of 0 and 1: the mask card against the oracle's card of nested / index-matched dielectric quads, `path` and the `prb` primal, 32 x 24 at 16 spp:
    relative L2 1e-4 with equal path and vertex counts (ray counts are not compared: the mask files zero-contribution emitter samples that the dielectric does not).
    A `sample1` of exactly 0 would make the index-matched dielectric reflect: seed 3 meets none (the counters would differ)."""
    tex = M.binary_texels()
    nested = M.TWOSIDED if variant == "twosided" else M.DIFFUSE
    kw = dict(integrator=integrator, layers=(0.55, 0.2) if variant == "two_layers" else (0.55, ), instanced=variant == "instanced")
    product = M.card_scene(mi, RES, SPP, tex, nested, True, **kw); twin = M.card_scene(mi, RES, SPP, tex, nested, False, **kw)
    if variant == "chunked":
        product["integrator"]["chunk_lanes"] = 4096
    if variant == "passes":
        product["integrator"]["samples_per_pass"] = SPP // 2
    err, got, want = _render_vs_oracle(mi, O, product, twin, integrator, passes=SPP // 2 if variant == "passes" else None)
    print("mask card %s / %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (integrator, variant, err, got, want))
    assert err <= 1e-4 and got == want


@pytest.mark.parametrize("kind", ["one_constant", "one_bitmap", "zero"])
def test_device_render_end_points(mi, O, kind):
    """o == 1 (a constant, a bitmap) against the pure nested card with equal counters, o == 0 against the all-dielectric card"""
    full = np.ones((M.K, M.K, 1), np.float32) if kind != "zero" else np.zeros((M.K, M.K, 1), np.float32)
    product = M.card_scene(mi, RES, SPP, full, M.DIFFUSE, True, opacity=1.0 if kind == "one_constant" else None)
    err, got, want = _render_vs_oracle(mi, O, product, M.card_scene(mi, RES, SPP, full, M.DIFFUSE, False), "path")
    print("mask card, %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (kind, err, got, want))
    assert err <= 1e-4 and got == want


# ------------------------------------------------------------------------------------------------ 3. partial opacity, statistically

def test_partial_opacity_statistics(mi, O):
    """constant o = 0.4, max_depth 3, rr_depth 8: E[I] = o I(nested) + (1 - o) I(absent), Z-test of tests/ztest.py against oracle batches of the two pure scenes; the same
    statistic must reject the composition at o = 0.55 (tests/test_mask_cpu.py runs it through the host render path)"""
    pure = M.oracle_pure_batches(mi, O)
    spp = 4096
    scene = mi.load_dict(M.lit_card(mi, {"type": "mask", "opacity": M.OPACITY, "n": dict(M.DIFFUSE)}, spp))
    img = mi.render(scene, spp=spp, seed=77).cpu().numpy().astype(np.float64)
    ok, pmin, alpha, bad, pmin_bad = M.statistics_verdicts(img, spp, pure)
    print("mask z-test: accepted %s (min p %.3g, alpha %.3g); against o = 0.55: accepted %s (min p %.3g)" % (ok, pmin, alpha, bad, pmin_bad))
    assert not bad, "the test has no power: the composition at o = 0.55 is accepted"
    assert ok


# ------------------------------------------------------------------------------------------------ 4. valid_ray, per lane and on the film

O1, O2 = 0.45, 0.7


def _through_both(n, seed=2):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n), np.full(n, 2.0)]).astype(np.float32)
    d = np.stack([rng.uniform(-0.15, 0.15, n), rng.uniform(-0.15, 0.15, n), np.full(n, -1.0)]); d = (d / np.linalg.norm(d, axis=0)).astype(np.float32)
    return o, d, np.full(n, np.inf, np.float32)


def _sample(mi, scene, o, d, maxt, seed=3):
    n = o.shape[1]
    sampler = mi.Sampler({"sample_count": 4, "seed": 5}); sampler.seed(seed, n)
    before = sampler.state.cpu().numpy().view(np.uint64).copy()          # (torch has no unsigned 64-bit type: the states travel as int64 bit patterns)
    spec, valid = scene.integrator().sample(scene, sampler, mi.Ray3f(o, d, maxt))
    return spec.cpu().numpy(), valid.cpu().numpy(), before, sampler.state.cpu().numpy().view(np.uint64)


def _lane_incs(mi, O, sampler_seed, n, before):
    """the increments of the lanes' pcg32 streams: Sampler::seed from the oracle's entries, checked against the states the product's sampler started from"""
    state, inc = M.lane_seeds(O, sampler_seed, n)
    assert np.array_equal(state, before.astype(np.uint64))
    return inc


@pytest.mark.parametrize("max_depth", [8, 1])
def test_valid_ray_per_lane(mi, O, max_depth):
    """rays through both masks: valid == (d3 < o1) or (d9 < o2), d_k the k-th float of the lane's stream -- six draws per vertex in JIT order (emitter 2, sample1, sample2
    2, roulette 1), asserted against the returned sampler state; radiance zero where `valid` is not set.  max_depth = 1: the last-vertex draw, valid == d3 < o1."""
    n = 1024
    scene = mi.load_dict(M.two_layers(mi, O1, O2, max_depth=max_depth))
    o, d, maxt = _through_both(n)
    spec, valid, before, after = _sample(mi, scene, o, d, maxt)
    sampler = mi.Sampler({"sample_count": 4, "seed": 5}); sampler.seed(3, n)
    inc = _lane_incs(mi, O, sampler.m_seed_value, n, before)
    want = np.zeros(n, bool); checked = 0
    for i in range(n):
        dr, _ = M.stream_draws(O, before[i], inc[i], 12)
        want[i] = dr[2] < O1 if max_depth == 1 else (dr[2] < O1 or dr[8] < O2)
        if max_depth == 1:                       # one iteration: six draws
            assert M.stream_draws(O, before[i], inc[i], 6)[1] == int(after[i]); checked += 1
        elif not want[i]:                        # null, null, miss: three iterations of six draws
            assert M.stream_draws(O, before[i], inc[i], 18)[1] == int(after[i]); checked += 1
    assert np.array_equal(valid, want), int((valid != want).sum())
    assert want.any() and (~want).any() and checked > 50
    assert (spec[:, ~valid] == 0).all() and (spec[:, valid] > 0).any() if max_depth > 1 else (spec == 0).all()


def test_valid_ray_prb_counts_null_interactions(mi):
    """prb keeps depth != 0 (prb.py:332): every ray that meets a mask is valid, whatever lobe it samples there"""
    scene = mi.load_dict(M.two_layers(mi, O1, O2, integrator="prb"))
    o, d, maxt = _through_both(512)
    o[2, ::7] = -3.0                              # below both: a miss
    spec, valid, _, _ = _sample(mi, scene, o, d, maxt)
    assert np.array_equal(valid, o[2] > 0)


def _film_flags(mi, O, scene, seed, spp, flags_of):
    """developed orc_film_put of per-lane flags over the wavefront of render(): (alpha plane H x W, the flags).  flags_of(draws, lanes, i): the flag of lane i from the 12
    numbers of its stream that follow the pixel jitter"""
    from tests import batch_cases as BC
    from tests import thinlens_cases as TL
    sensor = scene.sensors()[0]
    sv = (sensor.sampler().m_base_seed + seed) & 0xffffffff
    lanes = TL.lanes_of(mi, O, sensor, sv, spp)
    _, inc = M.lane_seeds(O, sv, lanes["n"])
    flags = np.array([flags_of(M.stream_draws(O, lanes["state"][i], inc[i], 12)[0], lanes, i) for i in range(lanes["n"])], np.float32)
    film = BC.film_put(O, lanes["wide"], "gaussian", lanes, np.stack([flags, flags, flags]))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(film[..., 3] > 0, film[..., 0] / film[..., 3], 0.0), flags, lanes


def test_rgba_film_of_a_mask_scene(mi, O):
    """the `rgba` film of the two-mask scene (both rectangles cover the view): its alpha channel is orc_film_put of the per-lane flags (d3 < o1) or (d9 < o2), the draws
    counted from the lane's state after the pixel jitter; weight-channel bar 2e-6.  Radiance where a sample is invalid is dropped: alpha 0 means a black pixel."""
    seed, spp = 4, 4
    scene = mi.load_dict(M.two_layers(mi, O1, O2, film={}, spp=spp))
    img = mi.render(scene, spp=spp, seed=seed).cpu().numpy()
    assert img.shape == (12, 16, 4)
    alpha, flags, _ = _film_flags(mi, O, scene, seed, spp, lambda dr, lanes, i: float(dr[2] < O1 or dr[8] < O2))
    assert 0.2 < flags.mean() < 0.95
    assert np.allclose(img[..., 3], alpha, rtol=2e-6, atol=2e-6), float(np.abs(img[..., 3] - alpha).max())
    dark = alpha == 0
    assert (img[..., :3][dark] == 0).all()


def test_rgba_film_without_a_mask_is_what_it_was(mi, O):
    """a scene WITHOUT a mask record keeps k_alpha_flags: its alpha channel is orc_film_put of `the camera ray met geometry`, at the 1e-6 bar of atomics-ordered sums"""
    seed, spp = 4, 4
    d = M.two_layers(mi, O1, O2, film={}, spp=spp)
    T = mi.ScalarTransform4f
    d["m1"] = dict(M.DIFFUSE); d["m2"] = dict(M.DIFFUSE)
    d["r1"]["to_world"] = T().translate([0.4, 0.2, 0]).scale([0.7, 0.5, 1.0]); d["r2"]["to_world"] = T().translate([-0.5, -0.3, -1.0]).scale([0.6, 0.6, 1.0])
    scene = mi.load_dict(d)
    img = mi.render(scene, spp=spp, seed=seed).cpu().numpy()
    osc, _ = O.scene_from_product(scene)
    hits = {}

    def met(dr, lanes, i):
        if not hits:
            hits["t"] = np.isfinite(osc.ray_intersect(lanes["o"], lanes["d"], lanes["maxt"])[0])
        return float(hits["t"][i])

    alpha, flags, _ = _film_flags(mi, O, scene, seed, spp, met)
    assert 0.05 < flags.mean() < 0.9
    assert np.allclose(img[..., 3], alpha, rtol=1e-6, atol=1e-6), float(np.abs(img[..., 3] - alpha).max())


# ------------------------------------------------------------------------------------------------ 5. gradients

def _grad_in(res=RES, seed=9):
    return np.random.default_rng(seed).uniform(-1, 1, (res[1], res[0], 3)).astype(np.float32)


def _np(g):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in g.items()}


@pytest.mark.parametrize("route", ["state_tape", "lane_cache"])
@pytest.mark.parametrize("child", ["constant", "bitmap"])
def test_nested_colour_gradients_binary_tiles(mi, O, child, route):
    """(a) the binary-tile card: the gradient of the nested BSDF's colour (a constant, a bitmap) equals the oracle's render_prb_backward for the nested record of the twin
    scene at 1e-3.  `state_tape`: the default route of a backward pass; `lane_cache`: hide_emitters keeps the tape away (backward_range) and the adjoint replays from
    the lane-indexed cache."""
    tex = M.binary_texels(); seed = 5
    nested = dict(M.DIFFUSE)
    if child == "bitmap":
        nested = {"type": "diffuse", "reflectance": {"type": "bitmap", "data": np.random.default_rng(12).uniform(0.2, 0.8, (6, 5, 3)).astype(np.float32), "raw": True}}
    kw = dict(integrator="prb", hide_emitters=route == "lane_cache")
    scene = mi.load_dict(M.card_scene(mi, RES, SPP, tex, nested, True, **kw)); twin = mi.load_dict(M.card_scene(mi, RES, SPP, tex, nested, False, **kw))
    osc, osensor = O.scene_from_product(twin); osc.set_hide_emitters(route == "lane_cache")
    g = _np(scene.integrator().render_backward(scene, None, _grad_in(), seed=seed, spp=SPP))
    g_refl, g_tex, _ = osc.render_prb_backward(osensor, _grad_in(), seed=seed, spp=SPP, max_depth=6, rr_depth=7)
    solid = [b for b in twin.bsdf_objs if b.id == "solid"][0]
    if child == "bitmap":
        got, want = g["cut.nested_bsdf.reflectance.data"], g_tex[solid.tex_index].astype(np.float64)
    else:
        got, want = g["cut.nested_bsdf.reflectance.value"].reshape(3), g_refl[solid.index].astype(np.float64)
    e = rel_l2(got.reshape(want.shape), want)
    white = rel_l2(g["white.reflectance.value"].reshape(3), g_refl[[b for b in twin.bsdf_objs if b.id == "white"][0].index])
    print("nested colour gradient, %s child, %s: %.3g (the walls' albedo: %.3g)" % (child, route, e, white))
    assert np.abs(want).max() > 0 and e <= 1e-3 and white <= 1e-3
    assert np.abs(g["cut.opacity.data"]).max() == 0.0          # texels AT 0 and 1: the clip's derivative is taken as 0 there (unpinned, docs/parity.md)


def test_opacity_times_its_gradient_equals_albedo_times_its(mi):
    """(b) constant o = 0.6 over a constant albedo rho: o and rho enter every differentiated term only as their product, so o grad_o == sum_c rho_c grad_rho_c, both
    from one backward pass; 1e-4"""
    scene = mi.load_dict(M.card_scene(mi, RES, SPP, M.binary_texels(), M.DIFFUSE, True, integrator="prb", opacity=0.6))
    g = _np(scene.integrator().render_backward(scene, None, _grad_in(), seed=5, spp=SPP))
    rho = np.array(M.DIFFUSE["reflectance"]["value"], np.float64)
    lhs = 0.6 * float(g["cut.opacity.value"].reshape(-1)[0]); rhs = float((rho * g["cut.nested_bsdf.reflectance.value"].reshape(3)).sum())
    print("o grad_o = %.7g, sum rho grad_rho = %.7g, relative difference %.3g" % (lhs, rhs, abs(lhs - rhs) / abs(rhs)))
    assert abs(rhs) > 0 and abs(lhs - rhs) <= 1e-4 * abs(rhs)


def test_nested_colour_gradient_against_central_differences(mi):
    """(c) grad_rho at o = 0.6 against central differences of the product's own same-seed forward render, rr_depth > max_depth: the null lobe does not depend on rho, the
    render is a polynomial in it, so this is a true derivative; within 3 %"""
    import torch
    seed = 9
    scene = mi.load_dict(M.card_scene(mi, RES, SPP, M.binary_texels(), M.DIFFUSE, True, integrator="prb", opacity=0.6, max_depth=4, rr_depth=10))
    it = scene.integrator(); grad_in = np.random.default_rng(8).uniform(0.5, 1.5, (RES[1], RES[0], 3)).astype(np.float32)
    loss = lambda: float((it.render(scene, seed=seed, spp=SPP).cpu().numpy().astype(np.float64) * grad_in).sum())
    grads = it.render_backward(scene, None, grad_in, seed=seed, spp=SPP)
    params = mi.traverse(scene); key = "cut.nested_bsdf.reflectance.value"
    x0 = params[key].detach().clone()
    v = torch.tensor(np.random.default_rng(12).uniform(-1, 1, tuple(x0.shape)).astype(np.float32), device=x0.device)
    vals = []
    for s in (+1.0, -1.0):
        params[key] = x0 + s * 0.02 * v; params.update(); vals.append(loss())
    params[key] = x0; params.update()
    fd = (vals[0] - vals[1]) / 0.04
    an = float((grads[key].cpu().numpy().astype(np.float64).reshape(-1) * v.cpu().numpy().astype(np.float64).reshape(-1)).sum())
    print(key, "central difference", fd, "prb", an, "relative error", abs(fd - an) / abs(fd))
    assert abs(fd) > 0 and abs(fd - an) <= 0.03 * abs(fd)


def _interior_texels(seed=3):
    return np.random.default_rng(seed).uniform(0.15, 0.85, (M.K, M.K, 1)).astype(np.float32)


def test_opacity_gradient_per_texel(mi):
    """(d) a one-channel nearest opacity bitmap with interior values: each texel's gradient equals the gradient of the constant opacity of the mask record that sits on
    that texel's quad alone (the same surface, one scalar parameter per quad; same seed, same paths).  1e-3, the gradient bar."""
    tex = _interior_texels(); seed = 5
    a = mi.load_dict(M.card_scene(mi, RES, SPP, tex, M.DIFFUSE, True, integrator="prb"))
    b = mi.load_dict(M.card_scene(mi, RES, SPP, tex, M.DIFFUSE, True, integrator="prb", separate=True))
    ga = _np(a.integrator().render_backward(a, None, _grad_in(), seed=seed, spp=SPP)); gb = _np(b.integrator().render_backward(b, None, _grad_in(), seed=seed, spp=SPP))
    got = ga["cut.opacity.data"]; assert got.shape == (M.K, M.K, 1)
    want = np.array([[gb["cut_%d_%d.opacity.value" % (j, i)].reshape(-1)[0] for i in range(M.K)] for j in range(M.K)])[:, :, None]
    e = rel_l2(got, want)
    print("opacity gradient per texel against per-quad constants: %.3g" % e)
    assert (np.abs(want) > 0).all() and e <= 1e-3


def test_three_channel_opacity_gradient_and_forward_mode(mi):
    """(e) a three-channel opacity bitmap: the opacity is the luminance of the texel, so grad[t, k] = lum_k * (the gradient of the one-channel map of luminances);
    (f) forward mode: the tangent of the opacity against <gradient, tangent>"""
    import torch
    lum = np.array(B.LUM, np.float64); seed = 5
    w3 = np.random.default_rng(21).uniform(0.15, 0.85, (M.K, M.K, 3)).astype(np.float32)
    wl = (w3.astype(np.float64) @ lum).astype(np.float32)[:, :, None]
    prop = {"type": "bitmap", "data": w3, "raw": True, "filter_type": "nearest"}
    a = mi.load_dict(M.card_scene(mi, RES, SPP, wl, M.DIFFUSE, True, integrator="prb", opacity=prop))
    b = mi.load_dict(M.card_scene(mi, RES, SPP, wl, M.DIFFUSE, True, integrator="prb"))
    grad_in = _grad_in()
    ga = _np(a.integrator().render_backward(a, None, grad_in, seed=seed, spp=SPP)); gb = _np(b.integrator().render_backward(b, None, grad_in, seed=seed, spp=SPP))
    got = ga["cut.opacity.data"]; assert got.shape == (M.K, M.K, 3)
    e = rel_l2(got, gb["cut.opacity.data"].reshape(M.K, M.K, 1) * lum.reshape(1, 1, 3))
    print("three-channel opacity: gradient against lum_k * grad of the luminance map %.3g" % e)
    assert np.abs(got).max() > 0 and e <= 1e-3
    for scene, g, shape in ((a, got, (M.K, M.K, 3)), (b, gb["cut.opacity.data"].reshape(M.K, M.K, 1), (M.K, M.K, 1))):
        tan = np.random.default_rng(22).uniform(-1, 1, shape).astype(np.float32)
        fwd = scene.integrator().render_forward(scene, None, seed=seed, spp=SPP, tangents={"cut.opacity.data": torch.tensor(tan)}).cpu().numpy().astype(np.float64)
        lhs = float((fwd * grad_in).sum()); rhs = float((g * tan).sum())
        print("forward mode against <grad, tangent>, %d channel(s):" % shape[2], lhs, rhs)
        assert abs(lhs - rhs) <= 1e-3 * abs(rhs)


GRAD_KEYS = ["cut.opacity.data", "cut.nested_bsdf.brdf_0.reflectance.value"]


@pytest.mark.parametrize("size,bar", [(((8, 8), 1), 1e-6), ((RES, SPP), 1e-4)])
def test_autograd_equals_render_backward(mi, size, bar):
    """(g) `mi.render` + autograd against `render_backward`: 1e-6 on a one-wave render (8 x 8, 1 spp), where an accumulator takes a few dozen atomic adds; 1e-4 at
    32 x 24 x 16 spp, where the float atomics' order alone moves two runs of the same pass by about 1e-6 (docs/parity.md, "blendbsdf")"""
    import torch
    res, spp = size
    scene = mi.load_dict(M.card_scene(mi, res, spp, _interior_texels(), M.TWOSIDED, True, integrator="prb"))
    params = mi.traverse(scene)
    for k in GRAD_KEYS:
        params[k].requires_grad_()
    img = mi.render(scene, params, spp=spp, seed=4)
    x = torch.tensor(np.random.default_rng(3).uniform(-1, 1, tuple(img.shape)).astype(np.float32), device=img.device)
    (img * x).sum().backward()
    direct = scene.integrator().render_backward(scene, params, x, seed=mi.sample_tea_32(4, 1)[0], spp=spp)
    err = {k: rel_l2(params[k].grad.cpu().numpy(), direct[k].reshape(params[k].shape).cpu().numpy()) for k in GRAD_KEYS}
    print("autograd against render_backward, %s x %d spp:" % (res, spp), err)
    for k in GRAD_KEYS:
        assert float(params[k].grad.abs().max()) > 0 and tuple(params[k].grad.shape) == tuple(params[k].shape)
        assert err[k] <= bar, (k, err)


def test_refusals_are_named_and_the_process_keeps_rendering(mi):
    """(h) what a scene with a mask record refuses, scene-wide, with the parameter or feature in the message"""
    import torch
    rc = {"type": "twosided", "a": {"type": "diffuse"}, "b": {"type": "roughconductor", "alpha": 0.3}}
    d = M.card_scene(mi, RES, 4, _interior_texels(), rc, True, integrator="prb")
    scene = mi.load_dict(d); params = mi.traverse(scene)
    ones = np.ones((RES[1], RES[0], 3), np.float32)
    params["cut.nested_bsdf.brdf_1.alpha.value"].requires_grad_()
    with pytest.raises(RuntimeError, match="cut.nested_bsdf.brdf_1.alpha.value"):
        mi.render(scene, params, spp=4, seed=0)
    scene.integrator().bsdf_parameter_gradients = True
    with pytest.raises(RuntimeError, match="cut.nested_bsdf.brdf_1.alpha.value"):
        scene.integrator().render_backward(scene, None, ones, seed=0, spp=4)
    scene.integrator().bsdf_parameter_gradients = False
    with pytest.raises(RuntimeError, match="nested_bsdf.brdf_0.reflectance.value"):
        scene.integrator().render_forward(scene, None, seed=1, spp=4, tangents={"cut.nested_bsdf.brdf_0.reflectance.value": torch.ones(3)})
    scene.integrator().shape_gradients = True
    with pytest.raises(RuntimeError, match="mask"):
        scene.integrator().render_backward(scene, None, ones, seed=0, spp=4)
    scene.integrator().shape_gradients = False
    deep = mi.load_dict(M.card_scene(mi, RES, 4, _interior_texels(), M.DIFFUSE, True, integrator="prb", max_depth=14))
    with pytest.raises(RuntimeError, match="mask.*max_depth must not exceed"):
        deep.integrator().render_backward(deep, None, ones, seed=0, spp=4)
    nocache = M.card_scene(mi, RES, 4, _interior_texels(), M.DIFFUSE, True, integrator="prb"); nocache["integrator"]["replay_cache"] = False
    nocache = mi.load_dict(nocache)
    with pytest.raises(RuntimeError, match="mask.*replay cache"):
        nocache.integrator().render_backward(nocache, None, ones, seed=0, spp=4)
    g = scene.integrator().render_backward(scene, None, ones, seed=0, spp=4)          # ... and the process keeps rendering
    assert float(g["cut.opacity.data"].abs().max()) > 0 and float(mi.render(scene, spp=4, seed=0).max()) > 0


# ------------------------------------------------------------------------------------------------ 6. aov

def test_aov_device_equals_host(mi):
    """k_aov_fill of a mask scene against the host entry (which tests/test_mask_cpu.py holds to the unmasked scene): albedo, depth, shape_index bit for bit"""
    import torch
    tex = np.random.default_rng(4).uniform(0.1, 0.9, (6, 4, 3)).astype(np.float32)
    inner = {"type": "twosided", "x": {"type": "diffuse", "reflectance": {"type": "bitmap", "data": tex, "raw": True}}}
    masked = mi.load_dict(M.lit_card(mi, {"type": "mask", "opacity": 0.25, "n": inner}, 4))
    n = 4096; rng = np.random.default_rng(6)
    o = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-1.2, 1.2, n), np.where(np.arange(n) % 2 == 0, 2.0, 0.25)]).astype(np.float32)
    d = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), np.where(np.arange(n) % 2 == 0, -1.0, 1.0)]); d = (d / np.linalg.norm(d, axis=0)).astype(np.float32)
    maxt = np.full(n, np.inf, np.float32)
    aov = mi.load_dict({"type": "aov", "aovs": "ab:albedo,dd:depth,si:shape_index"})
    dev = aov.sample(masked, mi.Ray3f(torch.tensor(o), torch.tensor(d), torch.tensor(maxt))).cpu().numpy()
    host = aov.sample_host(masked, o, d, maxt)
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32)) and (dev[0:3] > 0).any()
