"""`mesh_attribute` on the device: forward renders and `prb` gradients of an indexed mesh whose BSDF reads a vertex / face attribute against the oracle's render of the
twin scene (tests/attribute_cases.py: a triangle soup with a bitmap that reproduces the barycentric blend sample for sample), the per-ray lookup against a float64
restatement of Mesh::barycentric_coordinates + interpolate_attribute, and the checks that need no oracle (linearity, central differences, autograd, the optimiser loop).

The record tape is not a route of such a scene (docs/widening.md): the gradients are pinned over the two routes a backward pass can take -- the state tape (default) and
the lane-indexed replay cache (hide_emitters)."""
import numpy as np
import pytest

from tests import attribute_cases as A
from tests import mask_cases as M
from tests.test_cpu_host import rel_l2

pytestmark = pytest.mark.gpu

RES, SPP = (32, 24), 16
MIXED = dict(rtol=2e-5, atol=1e-7)          # the project's bar for mixed values (tests/test_mask_cpu.py)


def _case(name):
    """[(key, P, F, attribute, values, options)], first"""
    if name == "quad":                      # 2 triangles, 4 vertices: every lane of a wave hits the same rows; declared FIRST (vertex / face offsets 0)
        P, F = A.grid_mesh(1, 1); return [("M", P, F, "vertex_color", A.vertex_colors(4), {})], True
    if name == "grid16":                    # 512 triangles: many distinct rows per wave; declared behind the cubes (offsets non-zero)
        P, F = A.grid_mesh(16, 16, jitter=0.3); return [("M", P, F, "vertex_color", A.vertex_colors(P.shape[0]), {})], False
    if name == "two_meshes":                # different row counts, a record each
        P, F = A.grid_mesh(3, 2, center=(-0.45, -0.2, 0.4), ex=(0.3, 0.0, 0.05), ey=(0.0, 0.4, -0.1))
        Q, G = A.grid_mesh(5, 4, center=(0.45, 0.1, 0.3), ex=(0.3, 0.0, -0.08), ey=(0.0, 0.35, -0.12), seed=2)
        return [("M", P, F, "vertex_color", A.vertex_colors(P.shape[0]), {}), ("N", Q, G, "vertex_tint", A.vertex_colors(Q.shape[0], seed=8), {})], False
    if name == "twosided":
        P, F = A.grid_mesh(4, 3); return [("M", P, F, "vertex_color", A.vertex_colors(P.shape[0]), {"twosided": True})], False
    if name == "scaled":
        P, F = A.grid_mesh(4, 3); return [("M", P, F, "vertex_color", A.vertex_colors(P.shape[0]), {"scale": 0.5})], False
    if name == "mono":                      # one channel as a colour: broadcast
        P, F = A.grid_mesh(4, 3); return [("M", P, F, "vertex_gray", A.vertex_colors(P.shape[0], dim=1), {})], False
    if name == "face":
        P, F = A.grid_mesh(6, 5); return [("M", P, F, "face_color", A.vertex_colors(F.shape[0], seed=6), {})], False
    if name == "face_mono":
        P, F = A.grid_mesh(3, 3); return [("M", P, F, "face_gray", A.vertex_colors(F.shape[0], dim=1, seed=6), {})], True
    raise KeyError(name)


CASES = ["quad", "grid16", "two_meshes", "twosided", "scaled", "mono", "face", "face_mono"]


def _grad_in(res=RES, seed=9):
    return np.random.default_rng(seed).uniform(-1, 1, (res[1], res[0], 3)).astype(np.float32)


def _np(g):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in g.items()}


def _same_image(a, b):
    """two renders of the same radiance per lane: equal up to the order of the film's float atomics (1e-6, as tests/test_gpu_boundary.py takes it)"""
    a = a.cpu().numpy(); b = b.cpu().numpy()
    return np.array_equal(a, b) or rel_l2(a, b) < 1e-6


# ------------------------------------------------------------------------------------------------ 1. forward renders against the oracle's twin

@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("integrator", ["path", "prb"])
def test_forward_against_oracle_twin(mi, O, integrator, case):
    """both sides draw the same numbers along the same rays: relative L2 1e-4 (the project's forward bar), path and vertex counters equal"""
    meshes, first = _case(case)
    product, twin = A.pair(mi, RES, SPP, meshes, first=first, integrator=integrator)
    scene = mi.load_dict(product); osc, osensor = O.scene_from_product(mi.load_dict(twin))
    it = scene.integrator()
    img = mi.render(scene, spp=SPP, seed=3).cpu().numpy()
    want, ost = (osc.render_path if integrator == "path" else osc.render_prb)(osensor, seed=3, spp=SPP, max_depth=it.max_depth, rr_depth=it.rr_depth)
    st = it.stats(); e = rel_l2(img, want)
    print("mesh_attribute %s / %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (integrator, case, e, (st["paths"], st["vertices"]), (ost.paths, ost.vertices)))
    assert np.isfinite(img).all() and img.max() > 0 and e <= 1e-4 and (st["paths"], st["vertices"]) == (ost.paths, ost.vertices)


# ------------------------------------------------------------------------------------------------ 2. gradients against the oracle's texel gradients

@pytest.mark.parametrize("route", ["state_tape", "lane_cache"])
@pytest.mark.parametrize("case", CASES)
def test_gradients_against_oracle_twin(mi, O, case, route):
    """grad['<shape>.<name>'] against the oracle's render_prb_backward of the twin: a vertex row is the sum over its faces of alpha_k Sg + beta_k Sxg + gamma_k Syg of the
    face's 2 x 2 cell, a face row is its texel; relative L2 1e-3 (the project's gradient bar).  `lane_cache`: hide_emitters keeps the tape away."""
    meshes, first = _case(case); seed = 5
    product, twin = A.pair(mi, RES, SPP, meshes, first=first, integrator="prb")
    if route == "lane_cache":
        product["integrator"]["hide_emitters"] = True; twin["integrator"]["hide_emitters"] = True
    scene = mi.load_dict(product); tscene = mi.load_dict(twin)
    osc, osensor = O.scene_from_product(tscene); osc.set_hide_emitters(route == "lane_cache")
    g = _np(scene.integrator().render_backward(scene, None, _grad_in(), seed=seed, spp=SPP))
    g_refl, g_tex, _ = osc.render_prb_backward(osensor, _grad_in(), seed=seed, spp=SPP, max_depth=6, rr_depth=7)
    for key, P, F, name, values, opt in meshes:
        tb = tscene.bsdf_objs[tscene.meshes[[m["key"] for m in tscene.meshes].index(key)]["bsdf"]]
        G = g_tex[tb.tex_index].astype(np.float64)
        want = A.vertex_gradient_from_texels(F, P.shape[0], G) if name.startswith("vertex_") else A.face_gradient_from_texels(F.shape[0], G)
        want = want * float(opt.get("scale") or 1.0)          # the twin's texels are colour * scale
        got = g[key + "." + name]
        assert got.shape == np.asarray(values).shape
        if got.shape[1] == 1:
            want = want.sum(1, keepdims=True)                 # a one-channel attribute is broadcast: its gradient is the channel sum
        e = rel_l2(got, want)
        print("mesh_attribute gradient %s / %s / %s: %.3g (|want| max %.3g)" % (case, key, route, e, np.abs(want).max()))
        assert np.abs(want).max() > 0 and e <= 1e-3
    white = rel_l2(g["white.reflectance.value"].reshape(3), g_refl[[b for b in tscene.bsdf_objs if b.id == "white"][0].index])
    assert white <= 1e-3


def test_wall_texels_next_to_an_attribute(mi):
    """an attribute mesh next to a bitmap-textured wall, both gradients from one pass: the wall's texel gradients equal those of the same scene with the attribute
    replaced by its bitmap twin (same paths, same values), to 1e-6"""
    meshes, first = _case("grid16")
    product, twin = A.pair(mi, RES, SPP, meshes, integrator="prb")
    wall = np.random.default_rng(31).uniform(0.2, 0.8, (8, 8, 3)).astype(np.float32)
    for d in (product, twin):
        d["white"] = {"type": "diffuse", "reflectance": {"type": "bitmap", "data": wall, "raw": True}}
    a = mi.load_dict(product); b = mi.load_dict(twin)
    ga = _np(a.integrator().render_backward(a, None, _grad_in(), seed=5, spp=SPP)); gb = _np(b.integrator().render_backward(b, None, _grad_in(), seed=5, spp=SPP))
    e = rel_l2(ga["white.reflectance.data"], gb["white.reflectance.data"])
    print("wall texel gradients with / without the attribute: %.3g" % e)
    assert np.abs(gb["white.reflectance.data"]).max() > 0 and np.abs(ga["M.vertex_color"]).max() > 0 and e <= 1e-6


def test_scale_halves_gradient_and_image(mi):
    """scale = 0.5: the image is that of halved colours, the gradient half of theirs"""
    P, F = A.grid_mesh(4, 3); col = A.vertex_colors(P.shape[0])
    mk = lambda values, scale: mi.load_dict(dict(A.base_scene(mi, RES, SPP, integrator="prb"), M=A.product_shape(P, F, "vertex_color", values, scale)))
    a = mk(col, 0.5); b = mk((col * np.float32(0.5)).astype(np.float32), None)
    ia = mi.render(a, spp=SPP, seed=2).cpu().numpy(); ib = mi.render(b, spp=SPP, seed=2).cpu().numpy()
    ga = _np(a.integrator().render_backward(a, None, _grad_in(), seed=5, spp=SPP)); gb = _np(b.integrator().render_backward(b, None, _grad_in(), seed=5, spp=SPP))
    e = rel_l2(ga["M.vertex_color"], 0.5 * gb["M.vertex_color"])
    print("scale 0.5: image %.3g, gradient %.3g" % (rel_l2(ia, ib), e))
    assert rel_l2(ia, ib) <= 1e-6 and np.abs(gb["M.vertex_color"]).max() > 0 and e <= 1e-3
    params = mi.traverse(a)
    assert params.flags("M.bsdf.reflectance.scale") & mi.ParamFlags.NonDifferentiable
    params["M.bsdf.reflectance.scale"] = params["M.bsdf.reflectance.scale"] * 0 + 1.0; params.update()       # `scale` is updatable: back to the full colours
    full = mi.load_dict(dict(A.base_scene(mi, RES, SPP, integrator="prb"), M=A.product_shape(P, F, "vertex_color", col)))
    assert _same_image(mi.render(a, spp=SPP, seed=2), mi.render(full, spp=SPP, seed=2))


# ------------------------------------------------------------------------------------------------ 3. eval_1: opacity and weight; the dimensions that evaluate to 0

def _card(mi, kind, values, as_attribute, integrator="prb", k=M.K):
    """ONE mesh of k x k quads in front of the boxes whose `mask` opacity / `blendbsdf` weight is a one-channel FACE attribute (both triangles of quad (j, i) carry
    values[j, i]) -- or, the nearest-bitmap version: the same triangles with texcoords inside texel (j, i) of the k x k bitmap `values`"""
    d = A.base_scene(mi, RES, SPP, integrator=integrator)
    Ps, Fs, UV, rows = [], [], [], []
    for P, F, uv, (j, i) in M.card_quads(0.55, k=k):
        Fs.append(F + 4 * len(Ps)); Ps.append(P); UV.append(uv); rows += [values[j, i], values[j, i]]
    P = np.concatenate(Ps); F = np.concatenate(Fs).astype(np.uint32); uv = np.concatenate(UV)
    tex = ({"type": "mesh_attribute", "name": "face_cut"} if as_attribute else
           {"type": "bitmap", "data": np.asarray(values, np.float32).reshape(k, k, 1), "raw": True, "filter_type": "nearest"})
    if kind == "mask":
        bsdf = {"type": "mask", "opacity": tex, "material": dict(M.DIFFUSE)}
    else:
        bsdf = {"type": "blendbsdf", "weight": tex, "a": dict(M.DIFFUSE), "b": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.1, 0.6, 0.3]}}}
    d["card"] = {"type": "mesh", "faces": F, "positions": P, "texcoords": uv, "bsdf": bsdf}
    if as_attribute:
        d["card"]["attributes"] = {"face_cut": np.asarray(rows, np.float32).reshape(-1, 1)}
    return d


@pytest.mark.parametrize("values", ["binary", "interior"])
@pytest.mark.parametrize("kind", ["mask", "blendbsdf"])
def test_one_channel_attribute_as_opacity_and_weight(mi, kind, values):
    """the binary-tile card of tests/mask_cases.py with a face attribute of zeros and ones against its nearest-bitmap version: image 1e-4, gradients 1e-3.  At 0 and 1 the
    clip's derivative is taken as 0 (both versions: zero gradients), so the gradient is also compared on interior values, where it is not"""
    v = M.binary_texels()[:, :, 0] if values == "binary" else np.random.default_rng(3).uniform(0.15, 0.85, (M.K, M.K)).astype(np.float32)
    a = mi.load_dict(_card(mi, kind, v, True)); b = mi.load_dict(_card(mi, kind, v, False))
    ia = mi.render(a, spp=SPP, seed=3).cpu().numpy(); ib = mi.render(b, spp=SPP, seed=3).cpu().numpy()
    ga = _np(a.integrator().render_backward(a, None, _grad_in(), seed=5, spp=SPP)); gb = _np(b.integrator().render_backward(b, None, _grad_in(), seed=5, spp=SPP))
    key = "card.bsdf." + ("opacity" if kind == "mask" else "weight") + ".data"
    got = ga["card.face_cut"]; assert got.shape == (2 * M.K * M.K, 1)
    got = got.reshape(M.K, M.K, 2).sum(2); want = gb[key].reshape(M.K, M.K)
    print("%s over a face attribute, %s: image %.3g, gradient %.3g" % (kind, values, rel_l2(ia, ib), rel_l2(got, want) if np.abs(want).max() > 0 else 0.0))
    assert rel_l2(ia, ib) <= 1e-4
    if values == "interior":
        assert np.abs(want).max() > 0 and rel_l2(got, want) <= 1e-3
    else:
        assert np.abs(want).max() == 0 and np.abs(got).max() == 0


def test_dimensions_that_evaluate_to_zero(mi):
    """a three-channel attribute as a weight gives the image of weight 0 (eval_1 of dim 3 is 0); a two-channel attribute as a colour gives black"""
    k = M.K; rng = np.random.default_rng(4)
    d3 = _card(mi, "blendbsdf", np.zeros((k, k), np.float32), True); d3["card"]["attributes"] = {"face_cut": rng.uniform(0.2, 0.8, (2 * k * k, 3)).astype(np.float32)}
    d0 = _card(mi, "blendbsdf", np.zeros((k, k), np.float32), True)
    a = mi.load_dict(d3); b = mi.load_dict(d0)
    assert _same_image(mi.render(a, spp=SPP, seed=3), mi.render(b, spp=SPP, seed=3))
    g = _np(a.integrator().render_backward(a, None, _grad_in(), seed=5, spp=SPP))
    assert g["card.face_cut"].shape == (2 * k * k, 3) and np.abs(g["card.face_cut"]).max() == 0
    P, F = A.grid_mesh(4, 3)
    two = mi.load_dict(dict(A.base_scene(mi, RES, SPP), M=A.product_shape(P, F, "vertex_pair", rng.uniform(0.2, 0.8, (P.shape[0], 2)).astype(np.float32))))
    black = mi.load_dict(dict(A.base_scene(mi, RES, SPP), M={"type": "mesh", "faces": F, "positions": P, "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0, 0, 0]}}}))
    assert _same_image(mi.render(two, spp=SPP, seed=3), mi.render(black, spp=SPP, seed=3))


# ------------------------------------------------------------------------------------------------ 4. per ray

def test_per_ray_lookup_device_host_float64(mi):
    """the `aov` albedo of a diffuse over a vertex attribute on 20 480 rays: device and host twin bit for bit; both against a float64 restatement of
    Mesh::barycentric_coordinates + interpolate_attribute from the hit's p, at the project's 2e-5 for mixed values (triangles of aspect ratio <= 4)"""
    import torch
    P, F = A.grid_mesh(16, 16, jitter=0.3); col = A.vertex_colors(P.shape[0], lo=0.05, hi=0.95)
    scene = mi.load_dict(dict(A.base_scene(mi, RES, SPP), M=A.product_shape(P, F, "vertex_color", col)))
    n = 20480; rng = np.random.default_rng(6)
    target = np.asarray([0.0, -0.15, 0.35])[:, None] + np.asarray([0.6, 0.0, 0.12])[:, None] * rng.uniform(-1, 1, n) + np.asarray([0.0, 0.53, -0.2])[:, None] * rng.uniform(-1, 1, n)
    o = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), np.full(n, 3.5)]); d = target - o; d = d / np.linalg.norm(d, axis=0)
    o = o.astype(np.float32); d = d.astype(np.float32); maxt = np.full(n, np.inf, np.float32)
    aov = mi.load_dict({"type": "aov", "aovs": "ab:albedo,pp:position,pi:prim_index,si:shape_index"})
    dev = aov.sample(scene, mi.Ray3f(torch.tensor(o), torch.tensor(d), torch.tensor(maxt))).cpu().numpy()
    host = aov.sample_host(scene, o, d, maxt)
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))
    on = dev[7] == float(len(scene.meshes))                  # M is the last shape of the scene
    assert on.sum() > 15000
    prim = dev[6, on].astype(np.int64); p = dev[3:6, on].T.astype(np.float64)
    b = A.barycentric_reference(P, F, prim, p)
    c = col.astype(np.float64)
    want = c[F[prim, 0]] * b[:, 0:1] + c[F[prim, 1]] * b[:, 1:2] + c[F[prim, 2]] * b[:, 2:3]
    got = dev[0:3, on].T.astype(np.float64)
    worst = float(np.abs(got - want).max()); rel = float((np.abs(got - want) / np.abs(want)).max())
    print("per-ray lookup against float64: largest absolute difference %.3g, relative %.3g on %d hits" % (worst, rel, int(on.sum())))
    assert np.allclose(got, want, **MIXED)


# ------------------------------------------------------------------------------------------------ 5. without an oracle

def _panel(mi, res=RES, spp=SPP, max_depth=6, rr_depth=7, n=(4, 3)):
    P, F = A.grid_mesh(*n); col = A.vertex_colors(P.shape[0])
    return mi.load_dict(dict(A.base_scene(mi, res, spp, integrator="prb", max_depth=max_depth, rr_depth=rr_depth), M=A.product_shape(P, F, "vertex_color", col))), col


def test_linearity_at_depth_two(mi):
    """max_depth 2: a path meets the attribute at most once, the image is affine in it, so <grad, attr> == sum w * (image - the image at attr = 0); 2e-4"""
    scene, col = _panel(mi, max_depth=2, rr_depth=9)
    it = scene.integrator(); w = _grad_in(seed=11)
    g = it.render_backward(scene, None, w, seed=7, spp=SPP)["M.vertex_color"].cpu().numpy().astype(np.float64)
    img = it.render(scene, seed=7, spp=SPP).cpu().numpy().astype(np.float64)
    params = mi.traverse(scene); params["M.vertex_color"] = params["M.vertex_color"] * 0; params.update()
    img0 = it.render(scene, seed=7, spp=SPP).cpu().numpy().astype(np.float64)
    lhs = float((g * col).sum()); rhs = float((w * (img - img0)).sum())
    print("linearity: <grad, attr> %.7g, sum w (I - I0) %.7g, relative %.3g" % (lhs, rhs, abs(lhs - rhs) / abs(rhs)))
    assert abs(rhs) > 0 and abs(lhs - rhs) <= 2e-4 * abs(rhs)


def test_gradient_against_central_differences(mi):
    """central differences of the product's own same-seed forward render along a random direction in attribute space, rr_depth > max_depth; within 3 %"""
    import torch
    scene, col = _panel(mi, max_depth=4, rr_depth=10); seed = 9
    it = scene.integrator(); grad_in = np.random.default_rng(8).uniform(0.5, 1.5, (RES[1], RES[0], 3)).astype(np.float32)
    loss = lambda: float((it.render(scene, seed=seed, spp=SPP).cpu().numpy().astype(np.float64) * grad_in).sum())
    grads = it.render_backward(scene, None, grad_in, seed=seed, spp=SPP)
    params = mi.traverse(scene); key = "M.vertex_color"
    x0 = params[key].detach().clone()
    v = torch.tensor(np.random.default_rng(12).uniform(-1, 1, tuple(x0.shape)).astype(np.float32), device=x0.device)
    vals = []
    for s in (+1.0, -1.0):
        params[key] = x0 + s * 0.02 * v; params.update(); vals.append(loss())
    params[key] = x0; params.update()
    fd = (vals[0] - vals[1]) / 0.04
    an = float((grads[key].cpu().numpy().astype(np.float64) * v.cpu().numpy().astype(np.float64)).sum())
    print(key, "central difference", fd, "prb", an, "relative error", abs(fd - an) / abs(fd))
    assert abs(fd) > 0 and abs(fd - an) <= 0.03 * abs(fd)


@pytest.mark.parametrize("size,bitwise", [(((8, 8), 1), True), ((RES, SPP), False)])
def test_autograd_equals_render_backward(mi, size, bitwise):
    """`mi.render` + autograd against `render_backward`: bit for bit on one wave (8 x 8, 1 spp); 1e-4 at 32 x 24 x 16 spp, where the float atomics' order alone moves
    two runs of the same pass (docs/parity.md, "blendbsdf")"""
    import torch
    res, spp = size
    scene, _ = _panel(mi, res=res, spp=spp)
    params = mi.traverse(scene); key = "M.vertex_color"
    params[key].requires_grad_()
    img = mi.render(scene, params, spp=spp, seed=4)
    x = torch.tensor(np.random.default_rng(3).uniform(-1, 1, tuple(img.shape)).astype(np.float32), device=img.device)
    (img * x).sum().backward()
    direct = scene.integrator().render_backward(scene, params, x, seed=mi.sample_tea_32(4, 1)[0], spp=spp)[key]
    a = params[key].grad.cpu().numpy(); b = direct.cpu().numpy()
    assert a.shape == tuple(params[key].shape) == b.shape and np.abs(a).max() > 0
    e = rel_l2(a, b)
    print("autograd against render_backward, %s x %d spp: %.3g" % (res, spp, e))
    assert np.array_equal(a, b) if bitwise else e <= 1e-4


def test_three_step_loop_device_equals_host_updates(mi):
    """render -> loss -> backward -> step -> update(), three steps: parameters that live on the GPU (device-to-device updates) against the same loop with host arrays; 1e-3"""
    import torch
    outs = []
    for on_device in (True, False):
        scene, col = _panel(mi)
        target = torch.full((RES[1], RES[0], 3), 0.25, device="cuda")
        params = mi.traverse(scene); key = "M.vertex_color"
        x = params[key].detach().clone()
        for step in range(3):
            params[key] = x if on_device else x.cpu().numpy()
            params.update()
            img = scene.integrator().render(scene, seed=step, spp=SPP)
            g = scene.integrator().render_backward(scene, None, 2 * (img - target) / img.numel(), seed=100 + step, spp=SPP)[key]
            x = (x - 2000.0 * g).clamp(0.01, 0.99)
        outs.append(x.cpu().numpy())
        fresh = mi.load_dict(dict(A.base_scene(mi, RES, SPP, integrator="prb"), M=A.product_shape(*A.grid_mesh(4, 3), "vertex_color", scene.meshes[-1]["attributes"]["vertex_color"] if not on_device else mi.traverse(scene)[key].cpu().numpy())))
        assert _same_image(scene.integrator().render(scene, seed=1, spp=SPP), fresh.integrator().render(fresh, seed=1, spp=SPP))
    e = rel_l2(outs[0], outs[1])
    print("three-step loop, device against host updates: %.3g; moved by %.3g" % (e, float(np.abs(outs[0] - A.vertex_colors(outs[0].shape[0])).max())))
    assert np.abs(outs[0] - A.vertex_colors(outs[0].shape[0])).max() > 1e-3 and e <= 1e-3


@pytest.mark.parametrize("case", ["grid16", "mono", "face", "scaled", "opacity"])
def test_forward_mode_equals_gradient_times_tangent(mi, case):
    """`render_forward` reads the tangents of an attribute through the lookup's taps: sum(grad_in * forward image) == <grad, tangent>, 1e-3 (the bar of the other forward-mode
    checks, tests/test_gpu_mask.py); a vertex colour, a one-channel colour, a face colour, with `scale`, and a one-channel face attribute as a mask opacity"""
    import torch
    if case == "opacity":
        v = np.random.default_rng(3).uniform(0.15, 0.85, (M.K, M.K)).astype(np.float32)
        scene = mi.load_dict(_card(mi, "mask", v, True)); key = "card.face_cut"
    else:
        meshes, first = _case(case)
        scene = mi.load_dict(A.pair(mi, RES, SPP, meshes, first=first, integrator="prb")[0]); key = "M." + meshes[0][3]
    grad_in = _grad_in(); seed = 5
    g = scene.integrator().render_backward(scene, None, grad_in, seed=seed, spp=SPP)[key].cpu().numpy().astype(np.float64)
    tan = np.random.default_rng(22).uniform(-1, 1, g.shape).astype(np.float32)
    fwd = scene.integrator().render_forward(scene, None, seed=seed, spp=SPP, tangents={key: torch.tensor(tan)}).cpu().numpy().astype(np.float64)
    lhs = float((fwd * grad_in).sum()); rhs = float((g * tan).sum())
    print("forward mode against <grad, tangent>, %s: %.7g %.7g relative %.3g" % (case, lhs, rhs, abs(lhs - rhs) / abs(rhs)))
    assert abs(rhs) > 0 and abs(lhs - rhs) <= 1e-3 * abs(rhs)


def test_refusals_are_named_and_the_process_keeps_rendering(mi):
    import torch
    scene, _ = _panel(mi, spp=4)
    ones = np.ones((RES[1], RES[0], 3), np.float32)
    with pytest.raises(RuntimeError, match="M.vertex_color"):
        scene.integrator().render_forward(scene, None, seed=1, spp=4, tangents={"M.vertex_color": torch.ones(7, 3)})
    scene.integrator().bsdf_parameter_gradients = True
    with pytest.raises(RuntimeError, match="mesh_attribute"):
        scene.integrator().render_backward(scene, None, ones, seed=0, spp=4)
    scene.integrator().bsdf_parameter_gradients = False
    # instance `to_world` gradients of a scene whose TOP-LEVEL mesh reads an attribute
    P, F = A.grid_mesh(4, 3); d = dict(A.base_scene(mi, RES, 4, integrator="prb"), M=A.product_shape(P, F, "vertex_color", A.vertex_colors(P.shape[0])))
    d["g"] = {"type": "shapegroup", "c": {"type": "cube", "bsdf": {"type": "diffuse"}}}
    d["inst"] = {"type": "instance", "to_world": mi.ScalarTransform4f().translate([0.5, 0.5, 0.0]).scale(0.1), "g": {"type": "ref", "id": "g"}}
    instanced = mi.load_dict(d); instanced.integrator().shape_gradients = ["inst.to_world"]
    with pytest.raises(RuntimeError, match="instance to_world gradients.*mesh_attribute"):
        instanced.integrator().render_backward(instanced, None, ones, seed=0, spp=4)
    instanced.integrator().shape_gradients = False
    assert float(instanced.integrator().render_backward(instanced, None, ones, seed=0, spp=4)["M.vertex_color"].abs().max()) > 0
    deepf, _ = _panel(mi, spp=4, max_depth=14, rr_depth=5)
    with pytest.raises(RuntimeError, match="mesh_attribute.*render_forward"):
        deepf.integrator().render_forward(deepf, None, seed=1, spp=4, tangents={"M.vertex_color": torch.ones(20, 3)})
    scene.integrator().shape_gradients = ["M.positions"]
    with pytest.raises(RuntimeError, match="mesh_attribute"):
        scene.integrator().render_backward(scene, None, ones, seed=0, spp=4)
    scene.integrator().shape_gradients = False
    deep, _ = _panel(mi, spp=4, max_depth=14, rr_depth=5)
    with pytest.raises(RuntimeError, match="mesh_attribute.*max_depth must not exceed"):
        deep.integrator().render_backward(deep, None, ones, seed=0, spp=4)
    with pytest.raises(RuntimeError, match="mesh_attribute"):
        scene.bsdf_objs[scene.meshes[-1]["bsdf"]].eval(mi.BSDFContext(), type("si", (), dict(wi=torch.tensor([0.0, 0.0, 1.0]), uv=None))(), torch.tensor([[0.0], [0.0], [1.0]]))
    params = mi.traverse(scene)
    with pytest.raises(RuntimeError, match="M.vertex_color"):
        params["M.vertex_color"] = torch.zeros(7, 3); params.update()
    params = mi.traverse(scene)
    g = scene.integrator().render_backward(scene, None, ones, seed=0, spp=4)          # ... and the process keeps rendering
    assert float(g["M.vertex_color"].abs().max()) > 0 and float(mi.render(scene, spp=4, seed=0).max()) > 0
