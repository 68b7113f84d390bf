"""`blendbsdf` on the GPU: the kernels against the host entries and the oracle (forward renders, prb gradients of the weight and of the nested BSDFs' colours, the aov
albedo), and two statistical tests with different nested models.  Shapes are small: every test takes a few seconds."""
import numpy as np
import pytest

from tests import blend_cases as B
from tests.test_gpu_boundary import rel_l2

pytestmark = pytest.mark.gpu
ALL = B.ALL
LEAF = dict(rtol=2e-6, atol=1e-9)          # device against oracle for the leaf models (tests/test_gpu_boundary_masks.py)


# ------------------------------------------------------------------------------------------------ 5. device against host

@pytest.mark.parametrize("weight", B.WEIGHT_NAMES)
@pytest.mark.parametrize("pair", B.PAIR_NAMES)
def test_device_against_host(mi, pair, weight):
    """har_bsdf_eval_pdf / _eval / _pdf / _sample on the tuples of the CPU composition test against the host entries (which that test pins to the oracle), every context,
    with an `active` mask"""
    bsdf = mi.load_dict(B.blend_dict(mi, pair, weight)); scene, ib = B.bound(mi, bsdf)
    wi, uv, wo, s1, s2, w = B.tuples(weight)
    active = np.arange(wi.shape[1]) % 5 != 0
    si = type("SI", (), dict(wi=wi, uv=uv))()
    for ctx in B.contexts(pair):
        c = mi.BSDFContext(*ctx)
        val, pdf = bsdf.eval_pdf(c, si, wo, active)
        hv, hp = B.host_eval_pdf(mi, scene, ib, ctx, wi, uv, wo, active)
        val = val.cpu().numpy(); pdf = pdf.cpu().numpy()
        assert np.allclose(val, hv, **LEAF) and np.allclose(pdf, hp, **LEAF), (pair, weight, ctx, float(np.abs(val - hv).max()), float(np.abs(pdf - hp).max()))
        assert np.array_equal(bsdf.eval(c, si, wo, active).cpu().numpy(), val) and np.array_equal(bsdf.pdf(c, si, wo, active).cpu().numpy(), pdf)
        bs, wgt = bsdf.sample(c, si, s1, s2, active)
        h = B.host_sample(mi, scene, ib, ctx, wi, uv, s1, s2, active)
        assert np.array_equal(bs.sampled_type.cpu().numpy().astype(np.uint32), h["sampled_type"]) and np.array_equal(bs.sampled_component.cpu().numpy().astype(np.uint32), h["sampled_component"])
        assert np.array_equal(bs.eta.cpu().numpy(), h["eta"])
        fin = np.isfinite(h["pdf"]) & np.isfinite(h["weight"]).all(0)
        assert np.allclose(bs.wo.cpu().numpy(), h["wo"], rtol=2e-6, atol=1e-7) and np.allclose(bs.pdf.cpu().numpy()[fin], h["pdf"][fin], **LEAF)
        assert np.allclose(wgt.cpu().numpy()[:, fin], h["weight"][:, fin], rtol=5e-6, atol=1e-9), (pair, weight, ctx)
        m = ~active
        assert (val[:, m] == 0).all() and (pdf[m] == 0).all() and (wgt.cpu().numpy()[:, m] == 0).all() and (bs.wo.cpu().numpy()[:, m] == 0).all()
    v0, p0 = bsdf.eval_pdf(None, si, wo); v1, p1 = bsdf.eval_pdf(mi.BSDFContext(), si, wo)
    assert np.array_equal(v0.cpu().numpy(), v1.cpu().numpy()) and np.array_equal(p0.cpu().numpy(), p1.cpu().numpy()) and float(v0.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 6. device renders against the oracle

RES, SPP = (32, 24), 16


def _render_vs_oracle(mi, O, blend, ref, integrator, seed=3, passes=None):
    scene = mi.load_dict(blend); rscene = mi.load_dict(ref)
    osc, osensor = O.scene_from_product(rscene)
    it = scene.integrator()
    img = mi.render(scene, spp=SPP, seed=seed).cpu().numpy()
    if passes:
        want, ost = osc.render_path_passes(osensor, seed=seed, spp=SPP, spp_per_pass=passes, max_depth=it.max_depth, rr_depth=it.rr_depth)
    else:
        want, ost = (osc.render_path if integrator == "path" else osc.render_prb)(osensor, seed=seed, spp=SPP, max_depth=it.max_depth, rr_depth=it.rr_depth)
    st = it.stats()
    assert np.isfinite(img).all() and img.max() > 0
    return rel_l2(img, want), (st["paths"], st["vertices"]), (ost.paths, ost.vertices)


@pytest.mark.parametrize("integrator,variant", [(i, v) for i in ("path", "prb") for v in ("plain", "chunked", "passes", "twosided", "instanced")
                                                if not (i == "prb" and v == "passes")])          # (`prb` renders one wavefront and refuses `samples_per_pass`, as the reference's AD integrators do: see test_prb_renders_one_wavefront)
def test_device_render_against_oracle(mi, O, integrator, variant):
    """the diffuse + diffuse box of the CPU test on the device, `path` and the `prb` primal, 32 x 24 at 16 spp: equal to the oracle's render of the equivalent albedo
    bitmap, with equal path and vertex counters"""
    w = B.weight_map8()
    kw = dict(integrator=integrator, max_depth=6, rr_depth=7)
    blend = B.blended_box(mi, RES, SPP, B.DIFFUSE_PAIR, w, twosided=variant == "twosided", instanced=variant == "instanced", **kw)
    ref = B.equivalent_box(mi, RES, SPP, B.albedo_map(w), instanced=variant == "instanced", twosided=variant == "twosided", **kw)
    if variant == "chunked":
        blend["integrator"]["chunk_lanes"] = 4096
    if variant == "passes":
        blend["integrator"]["samples_per_pass"] = SPP // 2
    err, got, want = _render_vs_oracle(mi, O, blend, ref, integrator, passes=SPP // 2 if variant == "passes" else None)
    print("blend box %s / %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (integrator, variant, err, got, want))
    assert err <= 1e-4 and got == want


def test_prb_renders_one_wavefront(mi):
    """why the list above has no (prb, passes): the property belongs to SamplingIntegrator, `prb` refuses it (common.py:358-363 renders one wavefront)"""
    w = B.weight_map8()
    d = B.blended_box(mi, RES, SPP, B.DIFFUSE_PAIR, w, integrator="prb", max_depth=6, rr_depth=7)
    d["integrator"]["samples_per_pass"] = SPP // 2
    with pytest.raises(RuntimeError, match="samples_per_pass"):
        mi.load_dict(d)


@pytest.mark.parametrize("end", [0.0, 1.0])
def test_device_render_end_points(mi, O, end):
    rc = {"type": "roughconductor", "alpha": 0.3, "distribution": "ggx", "specular_reflectance": {"type": "rgb", "value": [0.9, 0.7, 0.5]}}
    df = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.4, 0.6, 0.7]}}
    blend = B.blended_box(mi, RES, SPP, (rc, df), end)
    pure = B.blended_box(mi, RES, SPP, (rc, df), end); pure["white"] = dict(rc if end == 0.0 else df)
    err, got, want = _render_vs_oracle(mi, O, blend, pure, "path")
    print("blend box, w = %g against the pure nested scene: rel L2 %.3g" % (end, err))
    assert err <= 1e-4 and got == want


# ------------------------------------------------------------------------------------------------ 7. gradients, exact pins

def _grad_pins(mi, O, w, a_bitmap=None, nearest=False, seed=5, w_blend=None):
    """render_backward of the blended box and the oracle's texel gradient G_T of the equivalent albedo bitmap (`w_blend`: the weight bitmap the blend is given, where it
    is not the one-channel `w` itself)"""
    integ = dict(integrator="prb", max_depth=6, rr_depth=7)
    blend = B.blended_box(mi, RES, SPP, B.DIFFUSE_PAIR, w if w_blend is None else w_blend, nearest=nearest, a_bitmap=a_bitmap, **integ)
    a = B.A_RGB if a_bitmap is None else a_bitmap
    ref = B.equivalent_box(mi, RES, SPP, B.albedo_map(w, a), nearest=nearest, **integ)
    scene = mi.load_dict(blend); osc, osensor = O.scene_from_product(mi.load_dict(ref))
    grad_in = np.random.default_rng(9).uniform(-1, 1, (RES[1], RES[0], 3)).astype(np.float32)
    grads = scene.integrator().render_backward(scene, None, grad_in, seed=seed, spp=SPP)
    _, g_tex, _ = osc.render_prb_backward(osensor, grad_in, seed=seed, spp=SPP, max_depth=6, rr_depth=7)
    return scene, {k: v.cpu().numpy().astype(np.float64) for k, v in grads.items()}, g_tex[0].astype(np.float64), grad_in


def test_gradients_of_weight_and_nested_colours(mi, O):
    """diffuse + diffuse: with G_T the oracle's texel gradient of the albedo bitmap (1 - w) A + w B,
    grad_w[t] = sum_c (B_c - A_c) G_T[t, c], grad_A[c] = sum_t (1 - w_t) G_T[t, c], grad_B[c] = sum_t w_t G_T[t, c]"""
    w = B.weight_map8()
    scene, g, GT, _ = _grad_pins(mi, O, w)
    A, Bc = B.A_RGB.astype(np.float64), B.B_RGB.astype(np.float64); w64 = w.astype(np.float64)
    want_w = (GT * (Bc - A)).sum(2, keepdims=True); want_a = ((1 - w64) * GT).sum((0, 1)); want_b = (w64 * GT).sum((0, 1))
    e = {k: rel_l2(g[k].reshape(v.shape), v) for k, v in (("white.weight.data", want_w), ("white.bsdf_0.reflectance.value", want_a), ("white.bsdf_1.reflectance.value", want_b))}
    print("blend gradients against the oracle's albedo-bitmap gradient:", e)
    assert np.abs(want_w).max() > 0 and all(v <= 1e-3 for v in e.values()), e


def test_gradient_of_a_three_channel_weight(mi, O):
    """a three-channel weight bitmap: the weight is the luminance of the interpolated texel, which is the interpolated luminance map (both are affine in the texels), so
    with grad_w the gradient of the one-channel map of luminances (pinned to the oracle's G_T as above), grad_w3[t, k] = lum_k grad_w[t]; forward mode: the tangent of
    the bitmap against <gradient, tangent>"""
    import torch
    lum = np.array(B.LUM, np.float64)
    w3 = np.random.default_rng(21).uniform(0.1, 0.9, (8, 8, 3)).astype(np.float32)
    wl = (w3.astype(np.float64) @ lum).astype(np.float32)[:, :, None]
    scene, g, GT, grad_in = _grad_pins(mi, O, wl, w_blend=w3)
    A, Bc = B.A_RGB.astype(np.float64), B.B_RGB.astype(np.float64)
    want_w = (GT * (Bc - A)).sum(2, keepdims=True)
    got = g["white.weight.data"]
    assert got.shape == (8, 8, 3)
    e = rel_l2(got, want_w * lum.reshape(1, 1, 3))
    ea = rel_l2(g["white.bsdf_0.reflectance.value"].reshape(3), ((1 - wl.astype(np.float64)) * GT).sum((0, 1)))
    print("three-channel weight: gradient against lum_k * grad_w %.3g, nested colour %.3g" % (e, ea))
    assert np.abs(want_w).max() > 0 and e <= 1e-3 and ea <= 1e-3
    tan = np.random.default_rng(22).uniform(-1, 1, (8, 8, 3)).astype(np.float32)
    fwd = scene.integrator().render_forward(scene, None, seed=5, spp=SPP, tangents={"white.weight.data": torch.tensor(tan)}).cpu().numpy().astype(np.float64)
    lhs = float((fwd * grad_in).sum()); rhs = float((got * tan).sum())
    print("three-channel weight, forward mode against <grad, tangent>:", lhs, rhs)
    assert abs(lhs - rhs) <= 1e-3 * abs(rhs)


def test_gradients_nearest_with_a_bitmap_child(mi, O):
    """A a bitmap of the weight's size, everything with the nearest filter, so that the per-texel product is exact: grad_A[t, c] = (1 - w_t) G_T[t, c]; texels of the weight
    outside [0, 1] have a gradient of exactly zero"""
    w = B.weight_map8(); w[0, 0, 0] = -0.3; w[5, 2, 0] = 1.4
    a = np.random.default_rng(12).uniform(0.2, 0.8, (8, 8, 3)).astype(np.float32)
    wc = np.clip(w, 0, 1)
    scene, g, GT, _ = _grad_pins(mi, O, wc, a_bitmap=a, nearest=True)            # the oracle's equivalent scene: the clipped weights
    scene2, g2, _, _ = _grad_pins(mi, O, w, a_bitmap=a, nearest=True)            # the product with the texels at -0.3 / 1.4
    w64 = wc.astype(np.float64); Bc = B.B_RGB.astype(np.float64)
    want_a = (1 - w64) * GT; want_w = (GT * (Bc - a.astype(np.float64))).sum(2, keepdims=True); want_b = (w64 * GT).sum((0, 1))
    inside = np.ones((8, 8), bool); inside[0, 0] = inside[5, 2] = False          # (the two texels sit AT 0 and 1 in the first scene: the derivative there is unpinned, docs/parity.md)
    e = {"A": rel_l2(g["white.bsdf_0.reflectance.data"], want_a), "w": rel_l2(g["white.weight.data"][inside], want_w[inside]), "B": rel_l2(g["white.bsdf_1.reflectance.value"].reshape(3), want_b)}
    print("nearest filter, bitmap child:", e)
    assert all(v <= 1e-3 for v in e.values()), e
    gw = g2["white.weight.data"]
    assert gw[0, 0, 0] == 0.0 and gw[5, 2, 0] == 0.0 and np.abs(gw).max() > 0
    assert rel_l2(gw[inside], want_w[inside]) <= 1e-3 and rel_l2(g2["white.bsdf_0.reflectance.data"], want_a) <= 1e-3


GRAD_KEYS = ["white.weight.data", "white.bsdf_0.reflectance.value", "white.bsdf_1.reflectance.value"]
ONE_WAVE = ((8, 8), 1)            # film and spp of a render of 64 paths: one wave of one block


def test_autograd_equals_render_backward(mi):
    """`mi.render` + autograd against `render_backward` at 1e-6, on a render of ONE WAVE (8 x 8 film, 1 spp).  Both sides are two runs of the same kernels with the same
    arguments if the glue is right (gradient seed sample_tea_32(seed, 1), spp, the adjoint image, the parameters' shapes, the channel sums of the weight), so what the
    bar can hold depends on the float32 atomics alone, which arrive in an order that differs from run to run.  An accumulator that takes N atomic adds of like size
    rounds each partial sum by at most ulp / 2 (rms ulp / sqrt(12) <= 3.4e-8 of the partial sum); the partial sums grow linearly, so one run carries a relative rms
    error of 3.4e-8 sqrt(N / 3) and two runs differ by sqrt(2) times that.  At the 32 x 24 film with 16 spp the 12288 paths are 192 waves of up to 6 vertices: a nested
    colour's row takes up to 1152 wave-reduced atomics and a weight texel as many, which gives 9.5e-7 between two runs -- the size of the bar itself, so a test
    at that size passes or fails by the order of the day whatever the code does (random signs in the adjoint image do not change the scaling: sums and partial sums
    shrink alike).  Measured there, six identical `render_backward` calls against each other: nested colours up to 1.8e-6 (median 5 - 7e-7), weight texels 1 - 2e-7;
    autograd against them: the same figures.  With 64 paths one wave issues every atomic add of the pass and the per-block LDS accumulators are flushed once onto
    zeros: an accumulator takes at most a few dozen adds (in any order: 3.4e-8 sqrt(36 / 3) sqrt(2) = 1.7e-7), and 1e-6 measures the glue.  Measured: the nested
    colours bit for bit, the weight texels <= 3e-8.  Sums over many waves and blocks are pinned to the oracle at the gradient bar (1e-3) by the three tests above."""
    import torch
    res, spp = ONE_WAVE
    scene = mi.load_dict(B.blended_box(mi, res, spp, B.DIFFUSE_PAIR, B.weight_map8(), integrator="prb", max_depth=6, rr_depth=7))
    params = mi.traverse(scene)
    for k in GRAD_KEYS:
        params[k].requires_grad_()
    img = mi.render(scene, params, spp=spp, seed=4)
    x = torch.tensor(np.random.default_rng(3).uniform(-1, 1, tuple(img.shape)).astype(np.float32), device=img.device)
    (img * x).sum().backward()
    direct = scene.integrator().render_backward(scene, params, x, seed=mi.sample_tea_32(4, 1)[0], spp=spp)
    err = {k: rel_l2(params[k].grad.cpu().numpy(), direct[k].reshape(params[k].shape).cpu().numpy()) for k in GRAD_KEYS}
    print("autograd against render_backward, one wave:", err)
    for k in GRAD_KEYS:
        assert float(params[k].grad.abs().max()) > 0 and tuple(params[k].grad.shape) == tuple(params[k].shape)
        assert err[k] <= 1e-6, (k, err)


def test_gradient_routes_autograd_and_forward_mode(mi, O):
    """at the size of the exact pins (32 x 24, 16 spp): `mi.render` + autograd returns every requested gradient in its parameter's shape (its VALUE against
    `render_backward` is pinned on one wave above; here it is printed), forward mode against <gradient, tangent>, and the refused tangents"""
    import torch
    w = B.weight_map8()
    integ = dict(integrator="prb", max_depth=6, rr_depth=7)
    scene = mi.load_dict(B.blended_box(mi, RES, SPP, B.DIFFUSE_PAIR, w, **integ))
    params = mi.traverse(scene)
    keys = GRAD_KEYS
    for k in keys:
        params[k].requires_grad_()
    img = mi.render(scene, params, spp=SPP, seed=4)
    x = torch.tensor(np.random.default_rng(3).uniform(-1, 1, tuple(img.shape)).astype(np.float32), device=img.device)
    (img * x).sum().backward()
    direct = scene.integrator().render_backward(scene, params, x, seed=mi.sample_tea_32(4, 1)[0], spp=SPP)
    err = {k: rel_l2(params[k].grad.cpu().numpy(), direct[k].reshape(params[k].shape).cpu().numpy()) for k in keys}
    print("autograd against render_backward, 192 waves (two runs of the same pass, atomics in another order):", err)
    for k in keys:
        assert float(params[k].grad.abs().max()) > 0 and tuple(params[k].grad.shape) == tuple(params[k].shape)
        assert err[k] <= 1e-4, (k, err)          # ten times under the gradient bar and a hundred times over the atomics' spread (see above): a wrong seed, adjoint or route, not noise
    # forward mode: the weight's tangent against <gradient, tangent> (adjoint image x, same seed)
    tan = torch.tensor(np.random.default_rng(8).uniform(-1, 1, (8, 8, 1)).astype(np.float32), device=img.device)
    fwd = scene.integrator().render_forward(scene, params, seed=mi.sample_tea_32(4, 1)[0], spp=SPP, tangents={"white.weight.data": tan})
    lhs = float((fwd * x).sum()); rhs = float((direct["white.weight.data"].reshape(8, 8, 1) * tan).sum())
    print("forward mode against <grad, tangent>:", lhs, rhs)
    assert abs(lhs - rhs) <= 1e-3 * abs(rhs)
    with pytest.raises(RuntimeError, match="bsdf_0.reflectance.value"):
        scene.integrator().render_forward(scene, params, seed=1, spp=SPP, tangents={"white.bsdf_0.reflectance.value": torch.ones(3)})
    # a BSDF object that was bound before it was nested is named by itself, not as '<blend>.bsdf_0': its record is nested all the same, and its tangent is refused
    df = mi.load_dict(dict(B.DIFFUSE_PAIR[0])); B.bound(mi, df)
    d = B.blended_box(mi, RES, SPP, B.DIFFUSE_PAIR, w, **integ); d["white"]["bsdf_a"] = df
    shared = mi.load_dict(d)
    own = [k for k, (kind, b) in shared._param_keys().items() if b is df]
    assert len(own) == 1 and ".bsdf_0." not in own[0]
    with pytest.raises(RuntimeError, match="nested in a `blendbsdf`"):
        shared.integrator().render_forward(shared, None, seed=1, spp=SPP, tangents={own[0]: torch.ones(3)})


def test_refused_gradients_are_named(mi):
    import torch
    rc = {"type": "roughconductor", "alpha": 0.3}
    d = B.blended_box(mi, RES, SPP, (B.DIFFUSE_PAIR[0], rc), 0.4, integrator="prb")
    scene = mi.load_dict(d); params = mi.traverse(scene)
    params["white.bsdf_1.alpha.value"].requires_grad_()
    with pytest.raises(RuntimeError, match="white.bsdf_1.alpha.value"):
        mi.render(scene, params, spp=4, seed=0)
    scene.integrator().bsdf_parameter_gradients = True
    with pytest.raises(RuntimeError, match="white.bsdf_1.alpha.value"):
        scene.integrator().render_backward(scene, None, np.ones((RES[1], RES[0], 3), np.float32), seed=0, spp=4)
    scene.integrator().bsdf_parameter_gradients = False
    scene.integrator().shape_gradients = True
    with pytest.raises(RuntimeError, match="blendbsdf"):
        scene.integrator().render_backward(scene, None, np.ones((RES[1], RES[0], 3), np.float32), seed=0, spp=4)
    scene.integrator().shape_gradients = False
    deep = mi.load_dict(B.blended_box(mi, RES, 4, B.DIFFUSE_PAIR, 0.4, integrator="prb", max_depth=14))
    with pytest.raises(RuntimeError, match="max_depth must not exceed"):
        deep.integrator().render_backward(deep, None, np.ones((RES[1], RES[0], 3), np.float32), seed=0, spp=4)


# ------------------------------------------------------------------------------------------------ 8. different models, statistically

def _lit_rectangle(mi, bsdf, spp, integrator="path"):
    T = mi.ScalarTransform4f
    return {"type": "scene",
            "integrator": {"type": integrator, "max_depth": 2},
            "sensor": {"type": "perspective", "fov": 35, "to_world": T().look_at([0, -2.2, 1.6], [0, 0, 0], [0, 0, 1]),
                       "film": {"type": "hdrfilm", "width": 16, "height": 16, "rfilter": {"type": "box"}}, "sampler": {"type": "independent", "sample_count": spp}},
            "mat": bsdf,
            "plane": {"type": "rectangle", "to_world": T().scale([1.5, 1.5, 1.0]), "bsdf": {"type": "ref", "id": "mat"}},
            "light": {"type": "rectangle", "to_world": T().translate([0.3, 0.9, 1.2]).rotate([1, 0, 0], 140).scale([0.5, 0.5, 1.0]),
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [12, 10, 8]}}}}


DF = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.5, 0.3]}}
RC = {"type": "roughconductor", "alpha": 0.3, "distribution": "ggx"}
W8 = 0.35


@pytest.fixture(scope="module")
def pure_batches(mi, O):
    """oracle batches of the two pure scenes: per-batch images (for means, variances and sums); computed once"""
    spp_b, batches = 64, 24
    out = []
    for k, b in enumerate((DF, RC)):
        osc, sensor = O.scene_from_product(mi.load_dict(_lit_rectangle(mi, dict(b), spp_b)))
        out.append(np.stack([osc.render_path(sensor, seed=1000 + 50 * k + s, spp=spp_b, max_depth=2)[0].astype(np.float64) for s in range(batches)]))
    return out, spp_b, batches


def test_forward_statistics(mi, O, pure_batches):
    """max_depth 2: the image is linear in the BSDF, E[I] = 0.65 I0 + 0.35 I1.  Two-sample Z-test of tests/ztest.py at its own bars, reference mean and per-sample variance
    combined from oracle batches of the two pure scenes, other seeds on the product's side.  The per-sample variance of the blended estimator is bounded by that of the
    estimator that picks one of the two pure estimators with probabilities (1 - w, w): (1 - w) v0 + w v1 + w (1 - w) (m0 - m1)^2 -- the blend samples its direction that way
    and shares the emitter sample, which only lowers it.  Power is a condition: 0.55 I0 + 0.45 I1 must be rejected."""
    from tests import ztest
    (b0, b1), spp_b, batches = pure_batches
    m0, m1 = b0.mean(0), b1.mean(0); v0, v1 = b0.var(0, ddof=1) * spp_b, b1.var(0, ddof=1) * spp_b
    spp = 4096
    scene = mi.load_dict(_lit_rectangle(mi, {"type": "blendbsdf", "weight": W8, "a": dict(DF), "b": dict(RC)}, spp))
    img = mi.render(scene, spp=spp, seed=77).cpu().numpy().astype(np.float64)
    n_ref = spp_b * batches

    def verdict(w):
        mean = (1 - w) * m0 + w * m1; var = (1 - w) * v0 + w * v1 + w * (1 - w) * (m0 - m1) ** 2
        return ztest.accept(img, spp, mean, var, n_ref)

    ok, pmin, alpha = verdict(W8); bad, pmin_bad, _ = verdict(0.45)
    print("blend z-test: accepted %s (min p %.3g, alpha %.3g); against w = 0.45: accepted %s (min p %.3g)" % (ok, pmin, alpha, bad, pmin_bad))
    assert not bad, "the test has no power: 0.55 I0 + 0.45 I1 is accepted"
    assert ok


def test_weight_gradient_statistics(mi, O, pure_batches):
    """d (sum of the image) / d w = sum(I1 - I0): mean and standard error over 16 seeds of render_backward with a unit adjoint against the oracle's batches, within
    4 combined standard errors; the band must separate the value from its negative and from the value scaled by (1 - w)"""
    (b0, b1), spp_b, batches = pure_batches
    per_batch = (b1 - b0).sum((1, 2, 3))
    want = per_batch.mean(); se_ref = np.sqrt(b0.sum((1, 2, 3)).var(ddof=1) / batches + b1.sum((1, 2, 3)).var(ddof=1) / batches)
    spp = 256
    scene = mi.load_dict(_lit_rectangle(mi, {"type": "blendbsdf", "weight": W8, "a": dict(DF), "b": dict(RC)}, spp, integrator="prb"))
    ones = np.ones((16, 16, 3), np.float32)
    vals = np.array([float(scene.integrator().render_backward(scene, None, ones, seed=200 + s, spp=spp)["mat.weight.value"].cpu().numpy().reshape(-1)[0]) for s in range(16)])
    got = vals.mean(); se = np.sqrt(vals.var(ddof=1) / 16 + se_ref ** 2)
    print("d sum(I) / d w: product %.5g +- %.3g, oracle %.5g +- %.3g, combined se %.3g" % (got, np.sqrt(vals.var(ddof=1) / 16), want, se_ref, se))
    assert se <= 0.02 * abs(want), "the band is too wide to mean anything"
    assert abs(-want - want) > 4 * se and abs((1 - W8) * want - want) > 4 * se
    assert abs(got - want) <= 4 * se


# ------------------------------------------------------------------------------------------------ 9. aov albedo

def test_aov_albedo(mi, O):
    """albedo of a blend = rho_0 (1 - w) + rho_1 w (blendbsdf.cpp:228-233), rho_k from the oracle-side AOV lookups of the scenes that carry the nested BSDFs alone"""
    import torch
    from tests import aov_cases as A
    tex = np.random.default_rng(4).uniform(0.1, 0.9, (6, 4, 3)).astype(np.float32)
    c0 = {"type": "diffuse", "reflectance": {"type": "bitmap", "data": tex, "raw": True}}
    c1 = {"type": "roughconductor", "alpha": 0.2, "specular_reflectance": {"type": "rgb", "value": [0.9, 0.6, 0.3]}}
    mk = lambda bsdf: mi.load_dict(_lit_rectangle(mi, bsdf, 4))
    scene = mk(B.blend_dict(mi, "plastic+diffuse", "bitmap3_bilinear_to_uv") | {"first": c0, "second": c1})
    pure = [mk(dict(c0)), mk(dict(c1))]
    n = 4096; rng = np.random.default_rng(6)
    o = np.stack([rng.uniform(-1.4, 1.4, n), rng.uniform(-1.4, 1.4, n), np.full(n, 2.0)]).astype(np.float32)
    d = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), np.full(n, -1.0)]); d = (d / np.linalg.norm(d, axis=0)).astype(np.float32)
    maxt = np.full(n, np.inf, np.float32)
    aov = mi.load_dict({"type": "aov", "aovs": "ab:albedo,uv:uv"})
    dev = aov.sample(scene, mi.Ray3f(torch.tensor(o), torch.tensor(d), torch.tensor(maxt))).cpu().numpy()
    host = aov.sample_host(scene, o, d, maxt)
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))
    rho = []
    for sc in pure:
        osc, _ = O.scene_from_product(sc)
        vals, hit, _ = A.oracle_aovs(O, sc, osc, ["albedo", "uv"], o, d, maxt)
        rho.append(vals)
    plane = (rho[0][3:5] != 0).any(0) & hit
    w = B.lookup_weight("bitmap3_bilinear_to_uv", rho[0][3:5].astype(np.float32)).astype(np.float64)
    want = rho[0][0:3] * (1 - w) + rho[1][0:3] * w
    assert plane.sum() > 1000 and np.allclose(dev[0:3, plane], want[:, plane], rtol=2e-5, atol=1e-7), float(np.abs(dev[0:3, plane] - want[:, plane]).max())
