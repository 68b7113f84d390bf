"""`normalmap` on the GPU: the kernels against the host entries (which tests/test_normalmap_cpu.py pins to normalmap.cpp restated over the oracle), the shading frames of
rectangles, the aov shading normal, renders -- the identity map against the nested BSDF alone, films composed on the CPU from oracle calls, the device against the host
render path -- and the refusals.  Shapes are small: every test takes a few seconds."""
import numpy as np
import pytest

from tests import blend_cases as B
from tests import normalmap_cases as N
from tests import test_normalmap_cpu as T
from tests.test_gpu_boundary import rel_l2

pytestmark = pytest.mark.gpu
ALL = N.ALL
LEAF = dict(rtol=2e-6, atol=1e-9)


@pytest.fixture(scope="module")
def tuples20k():
    return N.tuples()


# ------------------------------------------------------------------------------------------------ 1. per call: device against host

@pytest.mark.parametrize("flip,shadow", N.SWITCHES)
@pytest.mark.parametrize("nmap", N.MAP_NAMES)
@pytest.mark.parametrize("nested", N.NESTED_NAMES)
def test_device_against_host(mi, tuples20k, nested, nmap, flip, shadow):
    """har_bsdf_eval_pdf / _eval / _pdf / _sample on the 20 000 tuples of the CPU composition test against the host entries, every combination of the two switches (one
    case each: a host call lowers the scene anew), every context, with an `active` mask: the same HAR_HD code on both sides -- the project's leaf bars, and sampled_type,
    sampled_component, eta and the zero lanes equal on EVERY lane"""
    wi, uv, wo, s1, s2 = tuples20k
    active = np.arange(wi.shape[1]) % 5 != 0
    si = type("SI", (), dict(wi=wi, uv=uv))()
    worst = 0.0
    bsdf = mi.load_dict(N.normalmap_dict(mi, nested, nmap, flip, shadow)); scene, ib = B.bound(mi, bsdf)
    for ctx in N.contexts(nested):
        c = mi.BSDFContext(*ctx)
        val, pdf = bsdf.eval_pdf(c, si, wo, active)
        hv, hp = B.host_eval_pdf(mi, scene, ib, ctx, wi, uv, wo, active)
        val = val.cpu().numpy(); pdf = pdf.cpu().numpy()
        assert np.array_equal(val != 0, hv != 0) and np.array_equal(pdf != 0, hp != 0), (ctx, "zero lanes")
        assert np.allclose(val, hv, **LEAF) and np.allclose(pdf, hp, **LEAF), (ctx, float(np.abs(val - hv).max()), float(np.abs(pdf - hp).max()))
        assert np.array_equal(bsdf.eval(c, si, wo, active).cpu().numpy(), val) and np.array_equal(bsdf.pdf(c, si, wo, active).cpu().numpy(), pdf)
        bs, wgt = bsdf.sample(c, si, s1, s2, active)
        h = B.host_sample(mi, scene, ib, ctx, wi, uv, s1, s2, active)
        wgt = wgt.cpu().numpy()
        assert np.array_equal(bs.sampled_type.cpu().numpy().astype(np.uint32), h["sampled_type"]) and np.array_equal(bs.sampled_component.cpu().numpy().astype(np.uint32), h["sampled_component"])
        assert np.array_equal(bs.eta.cpu().numpy(), h["eta"]) and np.array_equal(wgt != 0, h["weight"] != 0) and np.array_equal(bs.pdf.cpu().numpy() != 0, h["pdf"] != 0)
        assert np.allclose(bs.wo.cpu().numpy(), h["wo"], rtol=2e-6, atol=1e-7) and np.allclose(bs.pdf.cpu().numpy(), h["pdf"], **LEAF)
        assert np.allclose(wgt, h["weight"], rtol=5e-6, atol=1e-9), ctx
        m = ~active
        assert (val[:, m] == 0).all() and (pdf[m] == 0).all() and (wgt[:, m] == 0).all() and (bs.wo.cpu().numpy()[:, m] == 0).all()
        worst = max(worst, float(np.abs(val - hv).max()), float(np.abs(wgt - h["weight"]).max()))
    print("normalmap device / host %s / %s / flip %s / shadow %s: largest absolute difference of values and weights %.2e" % (nested, nmap, flip, shadow, worst))


# ------------------------------------------------------------------------------------------------ 2. frames

def _device_rows(mi, scene, hits):
    import torch
    d, t, u, v, prim, shape, inst = hits
    n = t.size
    tt = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    ray = mi.Ray3f(torch.zeros((3, n), device="cuda"), tt(d, torch.float32), torch.full((n, ), float("inf"), device="cuda"))
    pi = mi.PreliminaryIntersection3f(scene, tt(t, torch.float32), tt(u, torch.float32), tt(v, torch.float32), tt(prim.astype(np.int32), torch.int32),
                                      tt(shape.astype(np.int32), torch.int32), tt(inst.view(np.int32), torch.int32))
    si = pi.compute_surface_interaction(ray)
    return np.concatenate([si.p.cpu().numpy(), si.n.cpu().numpy(), si.sh_frame.n.cpu().numpy(), si.sh_frame.s.cpu().numpy(), si.sh_frame.t.cpu().numpy(), si.wi.cpu().numpy(),
                           si.uv.cpu().numpy(), si.t.cpu().numpy()[None, :], si.dp_du.cpu().numpy(), si.dp_dv.cpu().numpy(), si.dn_du.cpu().numpy(), si.dn_dv.cpu().numpy()])


@pytest.mark.parametrize("xf,flip_normals,inst", T.FRAME_CASES)
def test_rectangle_frames_device(mi, xf, flip_normals, inst):
    """the sh_frame rows of the array-valued compute_surface_interaction for a rectangle under a normalmap: the reference's rule in float64 at rtol 3e-6 / atol 3e-7, the
    sign of t . cross(n, s), and the host twin's rows bit for bit"""
    rows, prow, hits = T.check_rectangle_frame(mi, lambda scene, h: _device_rows(mi, scene, h), xf, flip_normals, inst)
    tw = N.rectangle_transforms(mi)[xf]; itw = None if inst is None else N.instance_transform(mi, inst)
    scene = mi.load_dict(N.frame_scene(mi, tw, flip_normals, N.normalmap_dict(mi, "diffuse", "tilt30"), itw))
    assert np.array_equal(rows, N.host_si(mi, scene, *hits))


def test_frames_without_a_normalmap_are_todays_rows(mi):
    """a rectangle WITHOUT a normalmap, and a mesh without vertex normals WITH one, in a scene that holds a normalmap record (the kernel with the tangent code) report the
    rows of the same shapes in a scene without any (the kernel that has no such code), bit for bit"""
    T4 = mi.ScalarTransform4f
    tw = N.rectangle_transforms(mi)["scale"]
    nm = N.normalmap_dict(mi, "diffuse", "tilt30")
    with_nm = mi.load_dict({"type": "scene", "plain": {"type": "rectangle", "to_world": tw, "bsdf": N.nested_dict("diffuse")},
                            "flat": dict(N.flat_mesh(), bsdf=dict(nm), to_world=T4().translate([0, 0, -2.0]).rotate([0.6, 0.0, 0.8], 40.0)),
                            "bumpy": {"type": "rectangle", "to_world": T4().translate([0, 0, 3.0]), "bsdf": dict(nm)}})
    without = mi.load_dict({"type": "scene", "plain": {"type": "rectangle", "to_world": tw, "bsdf": N.nested_dict("diffuse")},
                            "flat": dict(N.flat_mesh(), bsdf=N.nested_dict("diffuse"), to_world=T4().translate([0, 0, -2.0]).rotate([0.6, 0.0, 0.8], 40.0)),
                            "bumpy": {"type": "rectangle", "to_world": T4().translate([0, 0, 3.0]), "bsdf": N.nested_dict("diffuse")}})
    keys = [m["key"] for m in with_nm.meshes]
    for name in ("plain", "flat"):
        hits = T._hits_on(mi, with_nm, keys.index(name), 0xffffffff)
        a = _device_rows(mi, with_nm, hits); b = _device_rows(mi, without, hits)
        assert np.array_equal(a, b), name


# ------------------------------------------------------------------------------------------------ 3. aov

@pytest.mark.parametrize("shape", ["rectangle", "mesh"])
def test_aov_sh_normal_device(mi, O, shape):
    """sh_normal and albedo on 20 480 rays over a rectangle / a flat mesh with a bitmap normal map: the device equals the host twin bit for bit, and the float64
    restatement at rtol 3e-6 / atol 3e-7"""
    import torch
    scene, tex = T.aov_scene(mi, shape)
    o, d, maxt = T.aov_rays()
    aov = mi.load_dict({"type": "aov", "aovs": "nn:sh_normal,aa:albedo"})
    dev = aov.sample(scene, mi.Ray3f(torch.tensor(o), torch.tensor(d), torch.tensor(maxt))).cpu().numpy()
    host = aov.sample_host(scene, o, d, maxt)
    assert np.array_equal(dev, host)
    want, card, seam = T.expected_sh_normal(mi, O, scene, tex, shape, o, d, maxt)
    assert card.sum() > 5000 and np.allclose(dev[0:3][:, ~seam], want[:, ~seam], **T.FRAME)


# ------------------------------------------------------------------------------------------------ 4. renders

RES, SPP = (32, 24), 16


def _render(mi, d, seed=3):
    scene = mi.load_dict(d)
    img = mi.render(scene, spp=SPP, seed=seed).cpu().numpy()
    st = scene.integrator().stats()
    assert np.isfinite(img).all() and img.max() > 0
    return img, (st["paths"], st["vertices"])


@pytest.mark.parametrize("nested", N.NESTED_NAMES)
def test_device_render_identity_map(mi, nested):
    """an identity normal map over the nested model on the Cornell walls (N.WALLS) is the scene with the nested BSDF alone, `path`: relative L2 1e-6, equal counters"""
    a, sa = _render(mi, N.walls_box(mi, RES, SPP, N.normalmap_dict(mi, nested, "identity"), N.nested_dict(nested)))
    b, sb = _render(mi, N.walls_box(mi, RES, SPP, N.nested_dict(nested), N.nested_dict(nested)))
    err = rel_l2(a, b)
    print("identity map over %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (nested, err, sa, sb))
    assert err <= 1e-6 and sa == sb


@pytest.mark.parametrize("nested", N.HALF_TURN_INVARIANT)
def test_device_render_identity_map_all_five_walls(mi, nested):
    """... with the map on the red and the green wall too, for the nested models whose sampling commutes with the half turn between those walls' two frames (see N.WALLS)"""
    a, sa = _render(mi, N.walls_box(mi, RES, SPP, N.normalmap_dict(mi, nested, "identity"), N.nested_dict(nested), walls=N.ALL_WALLS))
    b, sb = _render(mi, N.walls_box(mi, RES, SPP, N.nested_dict(nested), N.nested_dict(nested), walls=N.ALL_WALLS))
    err = rel_l2(a, b)
    print("identity map on all five walls over %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (nested, err, sa, sb))
    assert err <= 1e-6 and sa == sb


@pytest.mark.parametrize("variant", ["chunked", "passes", "twosided", "instanced", "prb"])
def test_device_render_identity_map_variants(mi, variant):
    """... chunked, in two passes, under an outer `twosided`, inside an instanced group, and the `prb` primal"""
    nd = N.nested_dict("roughplastic")
    kw = dict(integrator="prb" if variant == "prb" else "path", instanced=variant == "instanced")
    wrap = (lambda x: {"type": "twosided", "x": x}) if variant == "twosided" else (lambda x: x)
    da = N.walls_box(mi, RES, SPP, wrap(N.normalmap_dict(mi, "roughplastic", "identity")), wrap(dict(nd)), **kw)
    db = N.walls_box(mi, RES, SPP, wrap(dict(nd)), wrap(dict(nd)), **kw)
    for d in (da, db):
        if variant == "chunked":
            d["integrator"]["chunk_lanes"] = 4096
        if variant == "passes":
            d["integrator"]["samples_per_pass"] = SPP // 2
    a, sa = _render(mi, da); b, sb = _render(mi, db)
    err = rel_l2(a, b)
    print("identity map, %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (variant, err, sa, sb))
    assert err <= 1e-6 and sa == sb


@pytest.mark.parametrize("integrator", ["path", "prb"])
@pytest.mark.parametrize("nested", ["diffuse", "roughplastic"])
@pytest.mark.parametrize("shape", ["rectangle", "mesh"])
def test_device_render_composition(mi, O, shape, nested, integrator):
    """a rectangle (case 2) and a flat mesh (case 1) under a bilinear bitmap normal map with to_uv, one point light, max_depth 2: the device film (`path`, and the `prb`
    primal) equals the film composed on the CPU from oracle calls and the restated eval at relative L2 1e-4, the weights at 2e-6"""
    scene, tex = T.composition_scene(mi, nested, shape, spp=SPP, res=RES, integrator=integrator)
    img = mi.render(scene, spp=SPP, seed=5).cpu().numpy()
    want, near = composed(mi, O, scene, tex, nested, shape, True, True)
    err = rel_l2(img, O.develop(want))
    print("composition %s / %s / %s: rel L2 %.3g" % (integrator, shape, nested, err))
    assert np.linalg.norm(want[..., :3]) > 0 and err <= 1e-4


def composed(mi, O, scene, tex, nested, shape, flip, shadow, low=False):
    saved = T.RES
    T.RES = RES
    try:
        return T.composed_film(mi, O, scene, tex, nested, shape, flip, shadow, 5, SPP, low)
    finally:
        T.RES = saved


@pytest.mark.parametrize("switch", ["flip_invalid_normals", "use_shadowing_function"])
def test_device_render_switches(mi, O, switch):
    flip, shadow = switch != "flip_invalid_normals", switch != "use_shadowing_function"
    low = switch == "flip_invalid_normals"
    scene, tex = T.composition_scene(mi, "roughplastic", "rectangle", flip, shadow, spp=SPP, res=RES, low_camera=low)
    img = mi.render(scene, spp=SPP, seed=5).cpu().numpy()
    want, _ = composed(mi, O, scene, tex, "roughplastic", "rectangle", flip, shadow, low)
    default, _ = composed(mi, O, scene, tex, "roughplastic", "rectangle", True, True, low)
    err = rel_l2(img, O.develop(want)); apart = rel_l2(img, O.develop(default))
    print("%s = false: rel L2 %.3g against the restatement, %.3g away from the default" % (switch, err, apart))
    assert err <= 1e-4 and apart > 1e-3


@pytest.mark.parametrize("nested", ["diffuse", "roughplastic"])
@pytest.mark.parametrize("shape,hide", [("rectangle", False), ("mesh", False), ("rectangle", True)])
def test_device_against_host_render_path(mi, O, shape, nested, hide):
    """the same scenes at full depth (max_depth 6, an area light added, hide_emitters once): the device film equals the host render path's at relative L2 1e-4 with equal
    path and vertex counters (har_render_lanes_stats_host)"""
    tex = N.bumpy_texels()
    m = np.eye(3); m[:2, :] = N.TO_UV
    nm = {"type": "normalmap", "normalmap": {"type": "bitmap", "data": tex, "raw": True, "to_uv": mi.ScalarTransform3f(m)}, "x": N.nested_dict(nested)}
    d = N.lit_scene(mi, nm, shape, RES, SPP, max_depth=6, rr_depth=7, area_light=True, hide_emitters=hide)
    img, counters = _render(mi, d)
    scene = mi.load_dict(d)
    film, st = B.host_render_stats(mi, scene, 3, SPP, 6, 7)          # (no environment: hide_emitters hides nothing here -- the device film under it is the same film)
    err = rel_l2(img, O.develop(film))
    print("device / host render path %s / %s%s: rel L2 %.3g, (paths, vertices) %s vs %s" % (shape, nested, " / hide_emitters" if hide else "", err, counters, (st.paths, st.vertices)))
    assert err <= 1e-4 and counters == (st.paths, st.vertices)


# ------------------------------------------------------------------------------------------------ 5. gradients

GRES, GSPP = (32, 24), 16
NESTED_GRAD = ("diffuse", "roughplastic", "roughconductor_beckmann", "twosided(diffuse)")


def grad_scene(mi, nested, kind, shape="rectangle", max_depth=2, rr_depth=8, area_light=False, seed=31, **integrator_props):
    """the point-light scene of the composition tests under `prb`, its normal map a bilinear bitmap with to_uv, a nearest bitmap or a constant, tilts between 5 and 50
    degrees, seen from within 35 degrees of the surface normal so that no texel sits at a flip seam: (scene, the parameter's key)"""
    tex = N.bumpy_texels(6, 8, seed=seed)
    if kind == "constant":
        nm = {"type": "rgb", "value": [float(x) for x in N.tilted_texels(1, 1, 25.0, 25.0, 3)[0, 0]]}
    else:
        m = np.eye(3); m[:2, :] = N.TO_UV
        nm = {"type": "bitmap", "data": tex, "raw": True}
        if kind == "bilinear":
            nm["to_uv"] = mi.ScalarTransform3f(m)
        else:
            nm["filter_type"] = "nearest"
    d = N.lit_scene(mi, {"type": "normalmap", "normalmap": nm, "x": N.nested_dict(nested)}, shape, GRES, GSPP, integrator="prb", max_depth=max_depth, rr_depth=rr_depth, area_light=area_light, top_camera=True)
    d["integrator"].update(integrator_props)
    return mi.load_dict(d), "mat.normalmap.value" if kind == "constant" else "mat.normalmap.data"


def _directional(mi, scene, key, grad_in, seed, h, rng_seed=12):
    """(prb's <gradient, v>, the central difference of the same-seed forward render along v, the gradient) for a random direction v in the parameter's space"""
    import torch
    it = scene.integrator()
    loss = lambda: float((it.render(scene, seed=seed, spp=GSPP).cpu().numpy().astype(np.float64) * grad_in).sum())
    grads = it.render_backward(scene, None, grad_in, seed=seed, spp=GSPP)
    params = mi.traverse(scene)
    x0 = torch.as_tensor(params[key]).detach().clone()
    v = torch.tensor(np.random.default_rng(rng_seed).uniform(-1, 1, tuple(x0.shape)).astype(np.float32), device=x0.device)
    vals = []
    for sgn in (+1.0, -1.0):
        params[key] = x0 + sgn * h * v; params.update(); vals.append(loss())
    params[key] = x0; params.update()
    g = grads[key].cpu().numpy().astype(np.float64)
    assert g.shape == tuple(x0.shape)                                        # the gradient comes back in the parameter's shape
    return float((g.reshape(-1) * v.cpu().numpy().astype(np.float64).reshape(-1)).sum()), (vals[0] - vals[1]) / (2 * h), g


def _grad_in(seed=8):
    return np.random.default_rng(seed).uniform(0.5, 1.5, (GRES[1], GRES[0], 3)).astype(np.float32)


@pytest.mark.parametrize("kind", ["bilinear", "nearest", "constant"])
@pytest.mark.parametrize("nested", NESTED_GRAD)
def test_normal_map_gradient_against_central_differences(mi, nested, kind):
    """The pathwise-exact case: one point light, max_depth 2, rr_depth > max_depth -- neither the path nor the light sample depends on the frame, so the prb gradient of the
    normal map is the derivative of the same-seed forward render.  Central differences along a random direction in texel space (h = 2e-3), within 3 %."""
    scene, key = grad_scene(mi, nested, kind)
    an, fd, g = _directional(mi, scene, key, _grad_in(), 7, 2e-3)
    print("normal map gradient %s / %s: prb %.6g, central difference %.6g, relative error %.3g" % (nested, kind, an, fd, abs(fd - an) / abs(fd)))
    assert np.isfinite(g).all() and abs(fd) > 0 and abs(fd - an) <= 0.03 * abs(fd)


@pytest.mark.parametrize("shape", ["rectangle", "mesh"])
def test_nested_colour_gradient_against_central_differences(mi, shape):
    """the nested BSDF's colour under the same scenes (the `blend_child_commit` route: the leaf receives shadow * d_slot0 at the perturbed directions): the render is linear
    in it at max_depth 2, central differences within 3 %"""
    scene, _ = grad_scene(mi, "roughplastic", "bilinear", shape)
    an, fd, g = _directional(mi, scene, "mat.nested_bsdf.diffuse_reflectance.value", _grad_in(), 7, 0.02)
    print("nested colour gradient %s: prb %.6g, central difference %.6g, relative error %.3g" % (shape, an, fd, abs(fd - an) / abs(fd)))
    assert abs(fd) > 0 and abs(fd - an) <= 0.03 * abs(fd)


def test_exact_identity_of_the_texel_gradient(mi):
    """value depends on a texel c only through normalize(2c - 1): for a NEAREST map every lookup reads one texel, so sum_k grad_k (c_k - 0.5) = 0 per texel, at full depth
    with an area light (every term of prb); held at 1e-3 of sum |.| (sums of float32 atomics over thousands of vertices)"""
    scene, key = grad_scene(mi, "roughplastic", "nearest", max_depth=6, rr_depth=7, area_light=True)
    g = scene.integrator().render_backward(scene, None, _grad_in(), seed=4, spp=GSPP)[key].cpu().numpy().astype(np.float64)
    c = np.asarray(mi.traverse(scene)[key].cpu() if hasattr(mi.traverse(scene)[key], "cpu") else mi.traverse(scene)[key], np.float64)
    num = np.abs((g * (c - 0.5)).sum(2)); den = np.abs(g * (c - 0.5)).sum(2)
    hit = den > 0
    print("texel gradient identity: worst texel %.3g of sum |.| over %d texels with a gradient" % (float((num[hit] / den[hit]).max()), int(hit.sum())))
    assert hit.sum() > 10 and (num[hit] <= 1e-3 * den[hit]).all()


def test_delta_models_give_a_zero_normal_map_gradient(mi):
    scene, key = grad_scene(mi, "dielectric", "bilinear", max_depth=4, rr_depth=7, area_light=True)
    g = scene.integrator().render_backward(scene, None, _grad_in(), seed=4, spp=GSPP)[key].cpu().numpy()
    assert (g == 0).all()


def test_autograd_equals_render_backward(mi):
    """mi.render + autograd returns the normal map's gradient in the parameter's shape: the same numbers as render_backward with the loss's own gradient image"""
    import torch
    scene, key = grad_scene(mi, "diffuse", "bilinear", max_depth=4, rr_depth=7, area_light=True)
    w = torch.tensor(_grad_in(), device="cuda")
    params = mi.traverse(scene)
    params[key].requires_grad_()
    img = mi.render(scene, params, spp=GSPP, seed=6)
    (img * w).sum().backward()
    ref = scene.integrator().render_backward(scene, params, w, seed=mi.sample_tea_32(6, 1)[0], spp=GSPP)[key].cpu().numpy()          # (the gradient pass draws its own seed)
    got = params[key].grad.cpu().numpy()
    e = rel_l2(got, ref)
    print("autograd against render_backward: %.3g" % e)
    assert got.shape == ref.shape and np.abs(ref).max() > 0 and e <= 1e-4


# ------------------------------------------------------------------------------------------------ 6. refusals

def test_refusals_by_name_and_rendering_goes_on(mi):
    """refused scene-wide, each with `normalmap` in the message, and the process keeps rendering: forward-mode tangents, vertex-position gradients, gradients of nested
    non-colour parameters, a backward pass with max_depth > 12 or with the replay cache off"""
    import torch
    scene, key = grad_scene(mi, "roughplastic", "bilinear")
    before = mi.render(scene, spp=4, seed=1).cpu().numpy()
    it = scene.integrator()
    with pytest.raises(RuntimeError, match="normalmap"):
        it.render_forward(scene, mi.traverse(scene), spp=4, seed=1, tangents={"mat.nested_bsdf.diffuse_reflectance.value": torch.ones(3, device="cuda")})
    rough, _ = grad_scene(mi, "roughconductor_beckmann", "bilinear")
    p = mi.traverse(rough)
    p["mat.nested_bsdf.alpha.value"].requires_grad_()
    with pytest.raises(RuntimeError, match="mat.nested_bsdf.alpha.value.*normalmap"):          # gradients of nested non-colour parameters
        mi.render(rough, p, spp=4, seed=1)
    rough.integrator().bsdf_parameter_gradients = True
    with pytest.raises(RuntimeError, match="normalmap"):
        rough.integrator().render_backward(rough, None, _grad_in(), seed=1, spp=4)
    rough.integrator().bsdf_parameter_gradients = False
    scene.integrator().shape_gradients = True
    with pytest.raises(RuntimeError, match="normalmap"):                                          # vertex-position gradients
        scene.integrator().render_backward(scene, None, _grad_in(), seed=1, spp=4)
    scene.integrator().shape_gradients = False
    nocache, _ = grad_scene(mi, "diffuse", "bilinear", replay_cache=False)
    with pytest.raises(RuntimeError, match="normalmap.*replay cache"):
        nocache.integrator().render_backward(nocache, None, _grad_in(), seed=1, spp=4)
    deep, _ = grad_scene(mi, "diffuse", "bilinear", max_depth=13, rr_depth=20)
    with pytest.raises(RuntimeError, match="normalmap.*max_depth"):
        deep.integrator().render_backward(deep, None, _grad_in(), seed=1, spp=4)
    after = mi.render(scene, spp=4, seed=1).cpu().numpy()
    assert np.array_equal(before, after) and before.max() > 0
