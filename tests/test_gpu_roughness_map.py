"""Roughness maps on the GPU: the kernels of a scene whose `roughconductor` reads `alpha` from a bitmap against the host entries and the oracle's twin
(tests/roughness_map_cases.py) -- the device entries, `path` / `prb` renders, the texel gradients of `prb` with `bsdf_parameter_gradients`, mi.render + autograd,
updates in place and the refusals.  32 x 24 films at 16 spp: every test takes a few seconds."""
import numpy as np
import pytest

from tests import blend_cases as B
from tests import roughness_map_cases as R
from tests.test_roughness_map_cpu import build_pair, _tuples, CONTEXTS

pytestmark = pytest.mark.gpu
RES, SPP = (32, 24), 16
LEAF = dict(rtol=2e-6, atol=1e-9)
PRB_BAR = 1e-3          # the project's PRB bar


# ------------------------------------------------------------------------------------------------ 1. the entries

def test_device_entries_against_host(mi):
    """har_bsdf_alpha on the device == the host entry bit for bit; BSDF.eval_pdf / eval / pdf / sample of a twosided record with two anisotropic maps against the host entries
    on the same tuples, at the bars the mask and blend device tests use"""
    import ctypes as C
    import torch
    wi, uv, wo, s1, s2, uvp = _tuples(n_uv=64, n_dir=100)
    mu = R.bitmap(mi, R.texels(21), "bilinear", "mirror", R.to_uv(mi)); mv = R.bitmap(mi, R.texels(22, 3, 5, 3), "nearest", "clamp")
    bsdf = mi.load_dict({"type": "twosided", "inner": R.conductor(alpha_u=mu, alpha_v=mv, sample_visible=False)}); scene, ib = B.bound(mi, bsdf)
    n = uv.shape[1]
    duv = torch.as_tensor(uv, device="cuda").contiguous(); au = torch.empty(n, device="cuda"); av = torch.empty(n, device="cuda")
    mi.core.check(mi.lib().har_bsdf_alpha(scene._handle(), ib, n, C.c_void_p(duv.data_ptr()), C.c_void_p(au.data_ptr()), C.c_void_p(av.data_ptr()), None))
    torch.cuda.synchronize()
    hu, hv = R.host_alpha(mi, scene, ib, uv)
    assert np.array_equal(au.cpu().numpy(), hu) and np.array_equal(av.cpu().numpy(), hv) and hu.std() > 0 and hv.std() > 0
    active = np.arange(n) % 5 != 0
    si = type("SI", (), dict(wi=wi, uv=uv))()
    for ctx in CONTEXTS:
        c = mi.BSDFContext(*ctx)
        val, pdf = bsdf.eval_pdf(c, si, wo, active)
        hv_, hp = B.host_eval_pdf(mi, scene, ib, ctx, wi, uv, wo, active)
        val = val.cpu().numpy(); pdf = pdf.cpu().numpy()
        assert np.allclose(val, hv_, **LEAF) and np.allclose(pdf, hp, **LEAF), (ctx, float(np.abs(val - hv_).max()), float(np.abs(pdf - hp).max()))
        assert np.array_equal(bsdf.eval(c, si, wo, active).cpu().numpy(), val) and np.array_equal(bsdf.pdf(c, si, wo, active).cpu().numpy(), pdf)
        bs, wgt = bsdf.sample(c, si, s1, s2, active)
        h = B.host_sample(mi, scene, ib, ctx, wi, uv, s1, s2, active)
        assert np.array_equal(bs.sampled_type.cpu().numpy().astype(np.uint32), h["sampled_type"]) and np.array_equal(bs.sampled_component.cpu().numpy().astype(np.uint32), h["sampled_component"])
        assert np.allclose(bs.wo.cpu().numpy(), h["wo"], rtol=2e-6, atol=1e-7) and np.allclose(bs.pdf.cpu().numpy(), h["pdf"], **LEAF)
        assert np.allclose(wgt.cpu().numpy(), h["weight"], rtol=5e-6, atol=1e-9), ctx


# ------------------------------------------------------------------------------------------------ 2. renders against the oracle's twin

RENDER_CASES = ["nearest", "bilinear_to_uv_mirror", "three_channel", "anisotropic", "twosided", "instanced", "chunked", "passes"]


@pytest.mark.parametrize("integrator,case", [(i, c) for i in ("path", "prb") for c in RENDER_CASES if not (i == "prb" and c == "passes")])
def test_device_render_against_oracle_twin(mi, O, integrator, case):
    """`path` and the `prb` primal against the oracle's render of the twin: relative L2 <= 1e-4 with equal path and vertex counters"""
    extra = {"chunk_lanes": 4096} if case == "chunked" else {"samples_per_pass": 4} if case == "passes" else None
    base = "nearest" if case in ("instanced", "passes") else "bilinear_to_uv_mirror" if case == "chunked" else case
    sc, tw = build_pair(mi, base, RES, SPP, integrator=integrator, instanced=case == "instanced", extra=extra)
    osc, sensor = O.scene_from_product(tw)
    it = sc.integrator()
    img = mi.render(sc, spp=SPP, seed=3).cpu().numpy()
    if case == "passes":
        want, ost = osc.render_path_passes(sensor, seed=3, spp=SPP, spp_per_pass=4, max_depth=it.max_depth, rr_depth=it.rr_depth)
    else:
        want, ost = (osc.render_path if integrator == "path" else osc.render_prb)(sensor, seed=3, spp=SPP, max_depth=it.max_depth, rr_depth=it.rr_depth)
    st = it.stats()
    err = R.rel_l2(img, want)
    print("device render %s %s: rel L2 %.3g" % (integrator, case, err))
    assert np.isfinite(img).all() and (st["paths"], st["vertices"]) == (ost.paths, ost.vertices) and err <= 1e-4, (integrator, case, err)


def test_device_render_blend_nested_against_host(mi):
    """a textured roughconductor nested in a blendbsdf (bitmap weight): the device render against the host render"""
    inner = R.conductor(alpha=R.bitmap(mi, R.texels(3), "bilinear", "mirror", R.to_uv(mi)))
    w = R.bitmap(mi, np.random.default_rng(2).random((4, 4, 1)).astype(np.float32), "bilinear")
    sc = mi.load_dict(R.product_scene(mi, RES, SPP, {"type": "blendbsdf", "weight": w, "a": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.2, 0.5, 0.8]}}, "b": inner}))
    raw = mi.render(sc, spp=SPP, seed=3).cpu().numpy()
    film, st = B.host_render_stats(mi, sc, 3, SPP, 6, 7)
    from oracle import oracle as O_
    err = R.rel_l2(raw, O_.develop(film))
    gst = sc.integrator().stats()
    print("blend-nested device vs host: rel L2 %.3g" % err)
    assert (gst["paths"], gst["vertices"]) == (st.paths, st.vertices) and err <= 1e-4


# ------------------------------------------------------------------------------------------------ 3. texel gradients against the oracle

def _grad_in(seed=6):
    r = np.random.default_rng(seed)
    return (r.uniform(0.5, 1.5, (RES[1], RES[0], 3)) * np.where(r.random((RES[1], RES[0], 3)) < 0.5, -1.0, 1.0)).astype(np.float32) / (RES[0] * RES[1] * 3)


def _oracle_grads(O, tw, grad_in, seed=11):
    osc, sensor = O.scene_from_product(tw)
    it = tw.integrator()
    gx, g_refl = osc.render_prb_backward_bsdf_params(sensor, grad_in, seed=seed, spp=SPP, max_depth=it.max_depth, rr_depth=it.rr_depth)
    idx = np.array([[next(b.index for b in tw.bsdf_objs if b.id == "rough_%d_%d" % (j, i)) for i in range(R.K)] for j in range(R.K)])
    return gx[idx], g_refl[idx]          # K x K x 5 x 3, K x K x 3


PG = {"bsdf_parameter_gradients": True}


@pytest.mark.parametrize("case", ["nearest", "anisotropic_nearest", "bilinear_to_uv_mirror"])
def test_texel_gradients_against_oracle(mi, O, case):
    """render_backward with a random-sign adjoint image: the map's texel gradient against the alpha gradients of the twin's 16 records (nearest: texel (j, i) = groups 0 + 1 of
    record (j, i); anisotropic: the alpha_u map against group 0, the alpha_v map against group 1; bilinear: sum_q w_qk g_q with the float64 tap weights at uv_q, taps that
    mirror onto one texel included) at relative L2 <= 1e-3; eta, k and specular_reflectance of the textured record equal the sums over the twin's records"""
    grad_in = _grad_in()
    if case == "anisotropic_nearest":
        tu, tv = R.texels(3), R.texels(8)
        sc = mi.load_dict(R.product_scene(mi, RES, SPP, R.conductor(alpha_u=R.bitmap(mi, tu, "nearest"), alpha_v=R.bitmap(mi, tv, "nearest")), integrator="prb", extra=PG))
        tw = mi.load_dict(R.twin_scene(mi, RES, SPP, tu[:, :, 0], tv[:, :, 0], integrator="prb", extra=PG))
    else:
        sc, tw = build_pair(mi, case, RES, SPP, integrator="prb", extra=PG)
    grads = sc.integrator().render_backward(sc, None, grad_in, seed=11, spp=SPP)
    gx, g_refl = _oracle_grads(O, tw, grad_in)
    gq = gx[:, :, :2, :].sum(axis=3)          # K x K x 2: d / d alpha_u, d / d alpha_v per record
    if case == "nearest":
        pairs = [("rough.alpha.data", gq.sum(axis=2))]
    elif case == "anisotropic_nearest":
        pairs = [("rough.alpha_u.data", gq[:, :, 0]), ("rough.alpha_v.data", gq[:, :, 1])]
    else:
        pts = R.uv_points(5); am = R.rough_record(sc)[0].alpha_maps["alpha"]
        want = np.zeros((R.K, R.K))
        for j in range(R.K):
            for i in range(R.K):
                want += R.tap_weights64(R.K, R.K, "bilinear", "mirror", sc.texture_to_uv[am.tex_index], pts[j, i]) * gq[j, i].sum()
        pairs = [("rough.alpha.data", want)]
    for key, want in pairs:
        got = grads[key].cpu().numpy()
        err = R.rel_l2(got.reshape(-1), want.reshape(-1))
        print("texel gradient %s %s: rel L2 %.3g (|g| max %.3g)" % (case, key, err, np.abs(want).max()))
        assert tuple(got.shape) == (R.K, R.K, 1) and np.abs(want).max() > 0 and err <= PRB_BAR, (case, key, err)
    for key, want in (("rough.eta.value", gx[:, :, 2].sum(axis=(0, 1))), ("rough.k.value", gx[:, :, 3].sum(axis=(0, 1))), ("rough.specular_reflectance.value", g_refl.sum(axis=(0, 1)))):
        err = R.rel_l2(grads[key].cpu().numpy().reshape(-1), want)
        assert err <= PRB_BAR, (case, key, err)


def test_product_only_gradient_checks(mi):
    """(a) the map's per-texel gradient against a product scene with 16 separate constant-alpha records at 1e-4; (b) a 3-channel map's gradient == lum_k * the 1-channel
    map's at 1e-6; (c) a bilinear map with all texels equal to c: image and counters equal the {'alpha': c} scene, and the sum over its texels of the gradient equals that
    scene's scalar alpha gradient at 1e-4"""
    grad_in = _grad_in(9)
    t1 = R.texels(3)
    sc = mi.load_dict(R.product_scene(mi, RES, SPP, R.conductor(alpha=R.bitmap(mi, t1, "nearest")), integrator="prb", extra=PG))
    g1 = sc.integrator().render_backward(sc, None, grad_in, seed=11, spp=SPP)["rough.alpha.data"].cpu().numpy()
    sep = mi.load_dict(R.twin_scene(mi, RES, SPP, t1[:, :, 0], t1[:, :, 0], integrator="prb", extra=PG))
    gs = sep.integrator().render_backward(sep, None, grad_in, seed=11, spp=SPP)
    want = np.array([[float(gs["rough_%d_%d.alpha_u.value" % (j, i)].sum() + gs["rough_%d_%d.alpha_v.value" % (j, i)].sum()) for i in range(R.K)] for j in range(R.K)])
    err = R.rel_l2(g1.reshape(-1), want.reshape(-1))
    print("map against 16 separate records: rel L2 %.3g" % err)
    assert err <= 1e-4
    t3 = np.repeat(t1, 3, axis=2)          # the luminance of (a, a, a) is a up to the rounding of the coefficients' sum: the same surface
    sc3 = mi.load_dict(R.product_scene(mi, RES, SPP, R.conductor(alpha=R.bitmap(mi, t3, "nearest")), integrator="prb", extra=PG))
    g3 = sc3.integrator().render_backward(sc3, None, grad_in, seed=11, spp=SPP)["rough.alpha.data"].cpu().numpy()
    err3 = R.rel_l2(g3.reshape(-1), (g1 * R.LUM.reshape(1, 1, 3)).reshape(-1))
    print("3-channel against lum_k x 1-channel: rel L2 %.3g" % err3)
    assert tuple(g3.shape) == (R.K, R.K, 3) and err3 <= 1e-6
    c = 0.3
    flat = mi.load_dict(R.product_scene(mi, RES, SPP, R.conductor(alpha=R.bitmap(mi, np.full((4, 4, 1), c, np.float32), "bilinear", "mirror", R.to_uv(mi))), integrator="prb", extra=PG))
    const = mi.load_dict(R.product_scene(mi, RES, SPP, R.conductor(alpha=c), integrator="prb", extra=PG))
    ia = mi.render(flat, spp=SPP, seed=3).cpu().numpy(); sa = flat.integrator().stats()
    ib = mi.render(const, spp=SPP, seed=3).cpu().numpy(); sb = const.integrator().stats()
    assert R.rel_l2(ia, ib) <= 1e-6 and (sa["paths"], sa["vertices"]) == (sb["paths"], sb["vertices"])
    gf = flat.integrator().render_backward(flat, None, grad_in, seed=11, spp=SPP)["rough.alpha.data"].cpu().numpy().astype(np.float64).sum()
    gc = float(const.integrator().render_backward(const, None, grad_in, seed=11, spp=SPP)["rough.alpha.value"].sum())
    print("sum of the flat map's gradient %.6g against the scalar alpha gradient %.6g" % (gf, gc))
    assert abs(gf - gc) <= 1e-4 * abs(gc)


# ------------------------------------------------------------------------------------------------ 4. autograd, updates, refusals

@pytest.mark.parametrize("res,spp,bar", [((8, 8), 1, 1e-6), (RES, SPP, 1e-4)])
def test_mi_render_autograd(mi, res, spp, bar):
    """mi.render + autograd on '...alpha.data' equals render_backward: <= 1e-6 on a one-wave render (8 x 8, 1 spp), <= 1e-4 at 32 x 24 x 16 (the order of the float atomics
    of two runs, docs/parity.md "blendbsdf")"""
    import torch
    sc = mi.load_dict(R.product_scene(mi, res, spp, {"type": "twosided", "inner": R.conductor(alpha=R.bitmap(mi, R.texels(4, channels=3), "bilinear"))}, integrator="prb"))
    params = mi.traverse(sc); key = "rough.brdf_0.alpha.data"
    params[key].requires_grad_()
    img = mi.render(sc, params, spp=spp, seed=1)
    (img ** 2).mean().backward()
    g = params[key].grad
    assert tuple(g.shape) == (4, 4, 3) and torch.isfinite(g).all() and float(g.abs().max()) > 0
    x = img.detach().clone().requires_grad_(); (x ** 2).mean().backward()
    it = sc.integrator(); it.bsdf_parameter_gradients = True
    direct = it.render_backward(sc, params, x.grad, seed=mi.sample_tea_32(1, 1)[0], spp=spp)[key]
    it.bsdf_parameter_gradients = False
    err = R.rel_l2(g.cpu().numpy(), direct.reshape(g.shape).cpu().numpy())
    print("autograd against render_backward %s x %d: rel L2 %.3g" % (res, spp, err))
    assert err <= bar


def test_updates_in_place_and_adam(mi):
    """new texels through a host array and through a device tensor, then render: equals a freshly loaded scene at 1e-6 with equal counters; a three-step Adam loop on
    the map runs without rebuilding the scene (the handle is unchanged)"""
    import torch
    t0, t1, t2 = R.texels(3), R.texels(13), R.texels(14)
    mk = lambda t: mi.load_dict(R.product_scene(mi, RES, SPP, R.conductor(alpha=R.bitmap(mi, t, "bilinear")), integrator="prb"))
    sc = mk(t0); params = mi.traverse(sc); key = "rough.alpha.data"
    mi.render(sc, spp=SPP, seed=3); handle = sc._handle()
    for t, dev in ((t1, "cpu"), (t2, "cuda")):
        params[key] = torch.as_tensor(t, device=dev); params.update()
        img = mi.render(sc, spp=SPP, seed=3).cpu().numpy(); sa = sc.integrator().stats()
        fresh = mk(t); want = mi.render(fresh, spp=SPP, seed=3).cpu().numpy(); sb = fresh.integrator().stats()
        assert R.rel_l2(img, want) <= 1e-6 and (sa["paths"], sa["vertices"]) == (sb["paths"], sb["vertices"]) and sc._handle() == handle
    target = mi.render(mk(t0), spp=SPP, seed=5).detach()
    x = params[key].detach().clone().requires_grad_(); opt = torch.optim.Adam([x], lr=0.02)
    for step in range(3):
        opt.zero_grad()
        params[key] = x
        loss = ((mi.render(sc, params, spp=SPP, seed=5 + step) - target) ** 2).mean()
        loss.backward(); opt.step()
        with torch.no_grad():
            x.clamp_(0.02, 0.9)
        assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0 and sc._handle() == handle


def test_refusals_then_render(mi):
    """every refusal raises with its name, and the process renders correctly afterwards"""
    import torch
    inner = R.conductor(alpha=R.bitmap(mi, R.texels(3), "nearest"))
    ref = mi.load_dict(R.product_scene(mi, RES, SPP, inner, integrator="prb"))
    want = mi.render(ref, spp=SPP, seed=3).cpu().numpy()
    grad_in = _grad_in()
    for wrapper in ({"type": "blendbsdf", "weight": 0.5, "a": {"type": "diffuse"}, "b": inner}, {"type": "mask", "opacity": 0.5, "n": inner},
                    {"type": "normalmap", "normalmap": {"type": "rgb", "value": [0.5, 0.5, 1.0]}, "n": inner},
                    {"type": "bumpmap", "arbitrary": {"type": "bitmap", "data": np.full((4, 4, 1), 0.3, np.float32), "raw": True}, "n": inner}):
        sc = mi.load_dict(R.product_scene(mi, RES, SPP, wrapper, integrator="prb", extra=PG))
        with pytest.raises(RuntimeError, match="alpha texel gradients"):
            sc.integrator().render_backward(sc, None, grad_in, seed=11, spp=SPP)
        p = mi.traverse(sc); key = next(k for k in p.keys() if k.endswith("alpha.data")); p[key].requires_grad_()
        with pytest.raises(RuntimeError, match="alpha texels of a roughness map"):
            mi.render(sc, p, spp=SPP, seed=1)
    sc = mi.load_dict(R.product_scene(mi, RES, SPP, inner, integrator="prb", extra=dict(PG, shape_gradients=True)))
    with pytest.raises(RuntimeError, match="roughness map: vertex-position gradients"):
        sc.integrator().render_backward(sc, None, grad_in, seed=11, spp=SPP)
    sc = mi.load_dict(R.product_scene(mi, RES, SPP, inner, integrator="prb"))
    with pytest.raises(RuntimeError, match="roughness map: render_forward"):
        sc.integrator().render_forward(sc, None, seed=1, spp=SPP, tangents={"rough.specular_reflectance.value": torch.ones(3)})
    # DeviceGroup backward: har_multi_render_backward routes no BSDF-parameter gradients; the group names the keys it cannot produce (a one-device group, as the other
    # DeviceGroup tests of the suite build)
    group = mi.DeviceGroup(sc, devices=[0], integrator=mi.load_dict({"type": "prb", "max_depth": 6, "rr_depth": 7, "bsdf_parameter_gradients": True}))
    with pytest.raises(RuntimeError, match=r"roughness map: the alpha texel gradients \['rough\.alpha\.data'\] are not produced by DeviceGroup\.render_backward"):
        group.render_backward(grad_in, spp=SPP)
    plain = mi.DeviceGroup(sc, devices=[0], integrator=mi.load_dict({"type": "prb", "max_depth": 6, "rr_depth": 7}))
    g = plain.render_backward(grad_in, spp=SPP)          # without `bsdf_parameter_gradients` the group differentiates what it always did, and shows no gradient for the map
    assert "rough.alpha.data" not in g and "rough.specular_reflectance.value" in g
    del group, plain
    got = mi.render(ref, spp=SPP, seed=3).cpu().numpy()
    assert R.rel_l2(got, want) <= 1e-6
