"""`bumpmap` on the GPU: the kernels against the host entries (which tests/test_bumpmap_cpu.py pins to bumpmap.cpp restated over the oracle), the aov shading normal, renders
against the host render path, the plane-height identity, the gradients of the height map -- central differences in the pathwise-exact case, exact identities at full depth --
and the refusals.  Shapes are small: every test takes a few seconds."""
import numpy as np
import pytest

from tests import blend_cases as B
from tests import bumpmap_cases as U
from tests import normalmap_cases as N
from tests.test_gpu_boundary import rel_l2

pytestmark = pytest.mark.gpu
ALL = N.ALL
F32 = np.float32
RES, SPP = (32, 24), 16


@pytest.fixture(scope="module")
def tuples20k():
    return N.tuples()


# ------------------------------------------------------------------------------------------------ 1. per call: device against host, bit for bit

@pytest.mark.parametrize("flip,shadow", U.SWITCHES)
@pytest.mark.parametrize("nested", U.NESTED_NAMES)
def test_device_si_entries_equal_the_host_twins(mi, tuples20k, nested, flip, shadow):
    """har_bsdf_eval_pdf_si / har_bsdf_sample_si (through BSDF.eval_pdf / eval / pdf / sample, which read the interaction when the BSDF is a bumpmap) on the 20 000 tuples of
    the CPU test over the smooth-mesh interactions, every context, with an `active` mask: the same HAR_HD code on both sides, compiled without contraction -- equal bits"""
    import torch
    wi, uv, wo, s1, s2 = tuples20k
    n = wi.shape[1]
    geom = U.geometry("smooth_mesh", n)
    tex, m, scale = U.height_case(mi, "smooth_mesh", uv)
    active = np.arange(n) % 5 != 0
    si = U.SI(wi, uv, geom)
    bsdf = mi.load_dict(U.bumpmap_dict(mi, nested, U.bitmap_prop(mi, tex, m), scale, flip, shadow)); scene, ib = B.bound(mi, bsdf)
    for ctx in N.contexts(nested):
        c = mi.BSDFContext(*ctx)
        val, pdf = bsdf.eval_pdf(c, si, wo, active)
        hv, hp = U.host_eval_pdf_si(mi, scene, ib, ctx, wi, uv, wo, geom, active)
        val = val.cpu().numpy(); pdf = pdf.cpu().numpy()
        assert np.array_equal(val, hv) and np.array_equal(pdf, hp), (ctx, float(np.abs(val - hv).max()), float(np.abs(pdf - hp).max()))
        assert np.array_equal(bsdf.eval(c, si, wo, active).cpu().numpy(), val) and np.array_equal(bsdf.pdf(c, si, wo, active).cpu().numpy(), pdf)
        bs, wgt = bsdf.sample(c, si, s1, s2, active)
        h = U.host_sample_si(mi, scene, ib, ctx, wi, uv, s1, s2, geom, active)
        assert np.array_equal(bs.sampled_type.cpu().numpy().astype(np.uint32), h["sampled_type"]) and np.array_equal(bs.sampled_component.cpu().numpy().astype(np.uint32), h["sampled_component"])
        assert np.array_equal(bs.eta.cpu().numpy(), h["eta"]) and np.array_equal(bs.wo.cpu().numpy(), h["wo"]) and np.array_equal(bs.pdf.cpu().numpy(), h["pdf"])
        assert np.array_equal(wgt.cpu().numpy(), h["weight"]), ctx
        assert (val[:, ~active] == 0).all() and (wgt.cpu().numpy()[:, ~active] == 0).all()
    assert (h["weight"] != 0).any()
    # the entries without the interaction refuse the record by name
    with pytest.raises(RuntimeError, match="bumpmap"):
        mi.core.check(mi.lib().har_bsdf_eval_pdf(scene._handle(), ib, None, 1, mi.core._ptr(torch.zeros(3, 1, device="cuda")), mi.core._ptr(torch.zeros(2, 1, device="cuda")),
                                                 mi.core._ptr(torch.zeros(3, 1, device="cuda")), None, mi.core._ptr(torch.zeros(3, 1, device="cuda")), mi.core._ptr(torch.zeros(1, device="cuda")), None))


# ------------------------------------------------------------------------------------------------ 2. aov

@pytest.mark.parametrize("shape", ["rectangle", "smooth_mesh"])
def test_aov_sh_normal_and_albedo_device(mi, shape):
    """sh_normal and albedo on 20 480 rays over a rectangle and the smooth mesh under a bilinear height map: the device equals the host twin bit for bit; the normal is
    perturbed and the albedo is the nested BSDF's"""
    import torch
    from tests.test_normalmap_cpu import aov_rays
    scene = mi.load_dict(U.lit_scene(mi, U.bump_bsdf(mi), shape, area_light=False))
    o, d, maxt = aov_rays()
    aov = mi.load_dict({"type": "aov", "aovs": "nn:sh_normal,aa:albedo"})
    dev = aov.sample(scene, mi.Ray3f(torch.tensor(o), torch.tensor(d), torch.tensor(maxt))).cpu().numpy()
    host = aov.sample_host(scene, o, d, maxt)
    assert np.array_equal(dev, host)
    plain = aov.sample_host(mi.load_dict(U.lit_scene(mi, N.nested_dict("roughplastic"), shape, area_light=False)), o, d, maxt)
    hit = (plain[0:3] != 0).any(0)
    assert hit.sum() > 5000 and (np.abs(dev[0:3] - plain[0:3]).max(0)[hit] > 1e-3).mean() > 0.9 and np.allclose(np.linalg.norm(dev[0:3][:, hit], axis=0), 1, atol=1e-5)
    assert np.array_equal(dev[3:6], plain[3:6])


# ------------------------------------------------------------------------------------------------ 3. renders

def _render(mi, d, seed=3):
    scene = mi.load_dict(d)
    img = mi.render(scene, spp=SPP, seed=seed).cpu().numpy()
    st = scene.integrator().stats()
    assert np.isfinite(img).all() and img.max() > 0
    return img, (st["paths"], st["vertices"])


def _variant_scene(mi, variant, integrator):
    kw = dict(res=RES, spp=SPP, integrator=integrator, max_depth=6, rr_depth=7)
    if variant == "twosided":
        d = U.lit_scene(mi, U.bump_bsdf(mi), "rectangle", wrap=lambda x: {"type": "twosided", "x": x}, **kw)
    elif variant == "instanced":
        d = U.lit_scene(mi, U.bump_bsdf(mi), "smooth_mesh", instanced=True, **kw)
    elif variant == "smooth_mesh":
        d = U.lit_scene(mi, U.bump_bsdf(mi, channels=3), "smooth_mesh", **kw)
    elif variant == "mixed":          # next to a normalmap rectangle and a mask card in one scene
        d = U.lit_scene(mi, U.bump_bsdf(mi), "smooth_mesh", **kw)
        T = mi.ScalarTransform4f
        d["nm"] = {"type": "rectangle", "to_world": T().translate([0.9, 0.6, 0.3]).rotate([0, 1, 0], -40.0).scale([0.4, 0.4, 1.0]),
                   "bsdf": {"type": "normalmap", "normalmap": {"type": "bitmap", "data": N.bumpy_texels(), "raw": True}, "x": N.nested_dict("diffuse")}}
        d["cut"] = {"type": "rectangle", "to_world": T().translate([-0.6, -0.5, 0.5]).scale([0.4, 0.4, 1.0]),
                    "bsdf": {"type": "mask", "opacity": {"type": "bitmap", "data": (np.random.default_rng(3).random((4, 4, 1)) > 0.5).astype(F32), "raw": True, "filter_type": "nearest"},
                             "x": N.nested_dict("diffuse")}}
    else:
        d = U.lit_scene(mi, U.bump_bsdf(mi), "rectangle", **kw)
        if variant == "chunked":
            d["integrator"]["chunk_lanes"] = 4096
    return d


@pytest.mark.parametrize("integrator,variant", [("path", v) for v in ("plain", "chunked", "passes", "twosided", "instanced", "smooth_mesh", "mixed")] +
                         [("prb", v) for v in ("plain", "chunked", "twosided", "instanced", "smooth_mesh", "mixed")])
def test_device_against_host_render_path(mi, O, integrator, variant):
    """`path` and the `prb` primal at full depth with an area light against the host render path (har_render_lanes_stats_host): relative L2 1e-6, equal path and vertex counters"""
    if variant == "passes":
        # the host render path renders one pass; a render in two passes (persistent sampler streams) draws other samples.  Held instead by the plane-height identity, both
        # scenes in two passes: equal counters, 1e-6 (the identity holds at 9e-8 in one pass)
        h, m = U.plane_height(0.3, -0.2)
        da = U.unit_rectangle_scene(mi, U.bumpmap_dict(mi, "roughplastic", U.bitmap_prop(mi, h, m, "clamp")), RES, SPP, max_depth=6, rr_depth=7)
        db = U.unit_rectangle_scene(mi, {"type": "normalmap", "normalmap": {"type": "rgb", "value": U.plane_normal_colour(0.3, -0.2)}, "inner": N.nested_dict("roughplastic")}, RES, SPP, max_depth=6, rr_depth=7)
        for d in (da, db):
            d["integrator"]["samples_per_pass"] = SPP // 2
        (a, sa), (b, sb) = _render(mi, da), _render(mi, db)
        one, _ = _render(mi, U.unit_rectangle_scene(mi, U.bumpmap_dict(mi, "roughplastic", U.bitmap_prop(mi, h, m, "clamp")), RES, SPP, max_depth=6, rr_depth=7))
        print("two passes, plane height against the constant normal map: rel L2 %.3g, %s vs %s; %.3g away from the one-pass render" % (rel_l2(a, b), sa, sb, rel_l2(a, one)))
        assert rel_l2(a, b) <= 1e-6 and sa == sb and rel_l2(a, one) > 1e-2
        return
    d = _variant_scene(mi, variant, integrator)
    img, counters = _render(mi, d)
    film, st = B.host_render_stats(mi, mi.load_dict(d), 3, SPP, 6, 7)
    err = rel_l2(img, O.develop(film))
    print("device / host render path %s / %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (integrator, variant, err, counters, (st.paths, st.vertices)))
    assert err <= 1e-6 and counters == (st.paths, st.vertices)


@pytest.mark.parametrize("nested", ["diffuse", "roughplastic"])
def test_plane_height_is_a_constant_normal_map(mi, nested):
    """a plane height a u + b v on an untransformed +z rectangle equals the `normalmap` scene with the colour 0.5 + 0.5 normalize(-2a, -2b, 4) at 1e-4"""
    a_, b_ = 0.3, -0.2
    h, m = U.plane_height(a_, b_)
    bump, sa = _render(mi, U.unit_rectangle_scene(mi, U.bumpmap_dict(mi, nested, U.bitmap_prop(mi, h, m, "clamp")), RES, SPP))
    nmap, sb = _render(mi, U.unit_rectangle_scene(mi, {"type": "normalmap", "normalmap": {"type": "rgb", "value": U.plane_normal_colour(a_, b_)}, "inner": N.nested_dict(nested)}, RES, SPP))
    flat, _ = _render(mi, U.unit_rectangle_scene(mi, N.nested_dict(nested), RES, SPP))
    err = rel_l2(bump, nmap)
    print("plane height over %s against the constant normal map: rel L2 %.3g, %s vs %s; %.3g away from the flat scene" % (nested, err, sa, sb, rel_l2(bump, flat)))
    assert err <= 1e-4 and sa == sb and rel_l2(bump, flat) > 1e-3


# ------------------------------------------------------------------------------------------------ 4. gradients

GRES, GSPP = (32, 24), 16
KEY = "mat.nested_texture.data"


def grad_scene(mi, nested, channels=1, max_depth=2, rr_depth=8, area_light=False, seed=31, scale=1.0, texels=None, shape="smooth_mesh", res=GRES, spp=GSPP, instanced=False, **integrator_props):
    """the point-light scene under `prb` on the smooth mesh (normals AND texcoords), the height a bilinear bitmap with to_uv whose tilts stay under 50 degrees, seen from
    within 35 degrees of the normal so that no texel sits at a flip seam"""
    m = np.eye(3); m[:2, :] = N.TO_UV
    tex = U.bumpy_height(6, 8, channels, seed, 0.1) if texels is None else texels
    bs = U.bumpmap_dict(mi, nested, U.bitmap_prop(mi, tex, m), scale)
    d = U.lit_scene(mi, bs, shape, res, spp, integrator="prb", max_depth=max_depth, rr_depth=rr_depth, area_light=area_light, top_camera=True, instanced=instanced)
    d["integrator"].update(integrator_props)
    return mi.load_dict(d)


def _directional(mi, scene, key, grad_in, seed, h, rng_seed=12):
    """(prb's <gradient, v>, the central difference of the same-seed forward render along v, the gradient) for a random direction v in the parameter's space"""
    import torch
    it = scene.integrator()
    loss = lambda: float((it.render(scene, seed=seed, spp=GSPP).cpu().numpy().astype(np.float64) * grad_in).sum())
    grads = it.render_backward(scene, None, grad_in, seed=seed, spp=GSPP)
    params = mi.traverse(scene)
    x0 = torch.as_tensor(params[key]).detach().clone()
    v = torch.tensor(np.random.default_rng(rng_seed).uniform(-1, 1, tuple(x0.shape)).astype(F32), device=x0.device)
    vals = []
    for sgn in (+1.0, -1.0):
        params[key] = x0 + sgn * h * v; params.update(); vals.append(loss())
    params[key] = x0; params.update()
    g = grads[key].cpu().numpy().astype(np.float64)
    assert g.shape == tuple(x0.shape)                                        # the gradient comes back in the parameter's shape
    return float((g.reshape(-1) * v.cpu().numpy().astype(np.float64).reshape(-1)).sum()), (vals[0] - vals[1]) / (2 * h), g


def _grad_in(seed=8, res=GRES):
    return np.random.default_rng(seed).uniform(0.5, 1.5, (res[1], res[0], 3)).astype(F32)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("nested", ["diffuse", "roughplastic", "roughconductor_beckmann", "twosided(diffuse)"])
def test_height_map_gradient_against_central_differences(mi, nested, channels):
    """The pathwise-exact case: one point light, max_depth 2, rr_depth > max_depth -- neither the path nor the light sample depends on the frame, so the prb gradient of the
    height map is the derivative of the same-seed forward render.  Central differences along a random direction in texel space (h = 1e-3), within 3 %."""
    scene = grad_scene(mi, nested, channels)
    an, fd, g = _directional(mi, scene, KEY, _grad_in(), 7, 1e-3)
    print("height map gradient %s / %d channel(s): prb %.6g, central difference %.6g, relative error %.3g" % (nested, channels, an, fd, abs(fd - an) / abs(fd)))
    assert np.isfinite(g).all() and abs(fd) > 0 and abs(fd - an) <= 0.03 * abs(fd)


def test_nested_colour_gradient_against_central_differences(mi):
    """the nested BSDF's colour under the same scene (the `blend_child_commit` route): the render is linear in it at max_depth 2, central differences within 3 %"""
    scene = grad_scene(mi, "roughplastic")
    an, fd, g = _directional(mi, scene, "mat.nested_bsdf.diffuse_reflectance.value", _grad_in(), 7, 0.02)
    print("nested colour gradient: prb %.6g, central difference %.6g, relative error %.3g" % (an, fd, abs(fd - an) / abs(fd)))
    assert abs(fd) > 0 and abs(fd - an) <= 0.03 * abs(fd)


def test_exact_identities_of_the_texel_gradient(mi):
    """at full depth with an area light (every term of prb):
      * sum_j grad_j = 0 -- a constant added to the height changes nothing --, at 1e-4 of sum_j |grad_j| (a wrong sign or weight gives order one, the atomics' spread 1e-6);
      * the gradient at (scale 2, texels h) equals twice the gradient at (scale 1, texels 2h) at 1e-5, and the two images agree at 1e-6;
      * for three channels grad_k = lum_k x the luminance map's gradient"""
    tex = U.bumpy_height(6, 8, 1, 31, 0.05)
    a = grad_scene(mi, "roughplastic", texels=tex, scale=2.0, max_depth=6, rr_depth=7, area_light=True)
    b = grad_scene(mi, "roughplastic", texels=(2.0 * tex).astype(F32), scale=1.0, max_depth=6, rr_depth=7, area_light=True)
    gi = _grad_in()
    ga = a.integrator().render_backward(a, None, gi, seed=4, spp=GSPP)[KEY].cpu().numpy().astype(np.float64)
    gb = b.integrator().render_backward(b, None, gi, seed=4, spp=GSPP)[KEY].cpu().numpy().astype(np.float64)
    ia = mi.render(a, spp=GSPP, seed=4).cpu().numpy(); ib = mi.render(b, spp=GSPP, seed=4).cpu().numpy()
    zero = abs(ga.sum()) / np.abs(ga).sum()
    twice = rel_l2(ga, 2.0 * gb)
    print("texel gradient identities: |sum grad| / sum |grad| = %.3g; grad(scale 2, h) against 2 grad(scale 1, 2h): %.3g; the two images: %.3g" % (zero, twice, rel_l2(ia, ib)))
    assert np.abs(ga).sum() > 0 and zero <= 1e-4 and twice <= 1e-5 and rel_l2(ia, ib) <= 1e-6
    tex3 = U.bumpy_height(6, 8, 3, 31, 0.05)
    c3 = grad_scene(mi, "roughplastic", channels=3, texels=tex3, max_depth=6, rr_depth=7, area_light=True)
    lum = (tex3.astype(np.float64) * U.LUM).sum(2, keepdims=True).astype(F32)
    c1 = grad_scene(mi, "roughplastic", channels=1, texels=lum, max_depth=6, rr_depth=7, area_light=True)
    g3 = c3.integrator().render_backward(c3, None, gi, seed=4, spp=GSPP)[KEY].cpu().numpy().astype(np.float64)
    g1 = c1.integrator().render_backward(c1, None, gi, seed=4, spp=GSPP)[KEY].cpu().numpy().astype(np.float64)
    e = rel_l2(g3, g1 * U.LUM)
    print("three channels: grad_k against lum_k x the luminance map's gradient: %.3g" % e)
    assert g3.shape == (6, 8, 3) and g1.shape == (6, 8, 1) and e <= 1e-4          # (the luminance is rounded to float32 once more in the one-channel scene)


def test_delta_models_give_a_zero_height_gradient(mi):
    scene = grad_scene(mi, "dielectric", max_depth=4, rr_depth=7, area_light=True)
    g = scene.integrator().render_backward(scene, None, _grad_in(), seed=4, spp=GSPP)[KEY].cpu().numpy()
    assert (g == 0).all()


@pytest.mark.parametrize("size", ["one_wave", "film"])
def test_autograd_equals_render_backward(mi, size):
    """mi.render + autograd returns the height map's gradient in the parameter's shape: the numbers of render_backward with the loss's own gradient image -- bit for bit on
    one wave (8 x 8 x 1 spp: one block commits, no race between atomics), 1e-4 at 32 x 24 x 16"""
    import torch
    res, spp = ((8, 8), 1) if size == "one_wave" else (GRES, GSPP)
    scene = grad_scene(mi, "diffuse", max_depth=4, rr_depth=7, area_light=True, res=res, spp=spp)
    w = torch.tensor(_grad_in(res=res), device="cuda")
    params = mi.traverse(scene)
    params[KEY].requires_grad_()
    img = mi.render(scene, params, spp=spp, seed=6)
    (img * w).sum().backward()
    ref = scene.integrator().render_backward(scene, params, w, seed=mi.sample_tea_32(6, 1)[0], spp=spp)[KEY].cpu().numpy()          # (the gradient pass draws its own seed)
    got = params[KEY].grad.cpu().numpy()
    e = rel_l2(got, ref)
    print("autograd against render_backward, %s: %.3g" % (size, e))
    assert got.shape == ref.shape == (6, 8, 1) and np.abs(ref).max() > 0
    assert np.array_equal(got, ref) if size == "one_wave" else e <= 1e-4


# ------------------------------------------------------------------------------------------------ 5. refusals

def test_refusals_by_name_and_rendering_goes_on(mi):
    """refused scene-wide, each with `bumpmap` in the message, and the process keeps rendering: forward-mode tangents, vertex-position gradients, instance to_world gradients, gradients of `scale` and of
    nested non-colour parameters, a backward pass with max_depth > 12 or with the replay cache off"""
    import torch
    scene = grad_scene(mi, "roughplastic")
    before = mi.render(scene, spp=4, seed=1).cpu().numpy()
    it = scene.integrator()
    with pytest.raises(RuntimeError, match="bumpmap"):
        it.render_forward(scene, mi.traverse(scene), spp=4, seed=1, tangents={"mat.nested_bsdf.diffuse_reflectance.value": torch.ones(3, device="cuda")})
    p = mi.traverse(scene)
    p["mat.scale"].requires_grad_()
    with pytest.raises(RuntimeError, match="mat.scale.*bumpmap"):
        mi.render(scene, p, spp=4, seed=1)
    rough = grad_scene(mi, "roughconductor_beckmann")
    p = mi.traverse(rough)
    p["mat.nested_bsdf.alpha.value"].requires_grad_()
    with pytest.raises(RuntimeError, match="mat.nested_bsdf.alpha.value.*bumpmap"):          # gradients of nested non-colour parameters
        mi.render(rough, p, spp=4, seed=1)
    rough.integrator().bsdf_parameter_gradients = True
    with pytest.raises(RuntimeError, match="bumpmap"):
        rough.integrator().render_backward(rough, None, _grad_in(), seed=1, spp=4)
    rough.integrator().bsdf_parameter_gradients = False
    # vertex-position gradients, on a rectangle (the smooth mesh carries normals of its own, which `shape_gradients=True` leaves out: nothing would be asked for)
    flat = grad_scene(mi, "roughplastic", shape="rectangle")
    flat.integrator().shape_gradients = True
    with pytest.raises(RuntimeError, match="bumpmap"):
        flat.integrator().render_backward(flat, None, _grad_in(), seed=1, spp=4)
    flat.integrator().shape_gradients = False
    # instance to_world gradients, on the bump-mapped mesh inside an instanced group
    placed = grad_scene(mi, "roughplastic", instanced=True)
    first = mi.render(placed, spp=4, seed=1).cpu().numpy()
    assert "placed.to_world" in placed._instance_keys()
    placed.integrator().shape_gradients = ["placed.to_world"]
    with pytest.raises(RuntimeError, match="instance to_world gradients.*bumpmap"):
        placed.integrator().render_backward(placed, None, _grad_in(), seed=1, spp=4)
    placed.integrator().shape_gradients = False
    assert np.array_equal(mi.render(placed, spp=4, seed=1).cpu().numpy(), first) and first.max() > 0
    nocache = grad_scene(mi, "diffuse", replay_cache=False)
    with pytest.raises(RuntimeError, match="bumpmap.*replay cache"):
        nocache.integrator().render_backward(nocache, None, _grad_in(), seed=1, spp=4)
    deep = grad_scene(mi, "diffuse", max_depth=13, rr_depth=20)
    with pytest.raises(RuntimeError, match="bumpmap.*max_depth"):
        deep.integrator().render_backward(deep, None, _grad_in(), seed=1, spp=4)
    after = mi.render(scene, spp=4, seed=1).cpu().numpy()
    assert np.array_equal(before, after) and before.max() > 0
