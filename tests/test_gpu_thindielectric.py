"""`thindielectric` on the GPU: the kernels against the host entries, valid_ray and radiance per lane against the restatement over the lanes' pcg32 streams, exact-twin
renders against the oracle's index-matched dielectric and the product's own mask of opacity 0 (with the alpha plane of an `rgba` film), prb gradients through the pane
against the oracle's twin, its own homogeneity and central differences, the refusals, and the aov channels.  Shapes are small: every test takes a few seconds."""
import numpy as np
import pytest

from tests import blend_cases as B
from tests import mask_cases as M
from tests import thindielectric_cases as TD
from tests.test_gpu_boundary import rel_l2

pytestmark = pytest.mark.gpu
ALL = TD.ALL
LEAF = dict(rtol=2e-6, atol=1e-9)


# ------------------------------------------------------------------------------------------------ 4. device entries against the host entries

@pytest.mark.parametrize("colour", TD.COLOURS)
@pytest.mark.parametrize("eta", list(TD.ETAS))
def test_device_against_host(mi, O, eta, colour):
    """har_bsdf_eval_pdf / _sample on the tuples of the CPU per-call test against the host entries (which that test holds to the restatement), every context, with an
    `active` mask; wo, eta, sampled_type and sampled_component equal on every lane, pdf and weight at the leaf bar"""
    bsdf = mi.load_dict(TD.thin_dict(mi, eta, colour)); scene, ib = B.bound(mi, bsdf)
    wi, uv, wo, s1, s2, rp = TD.tuples(O, eta)
    active = np.arange(wi.shape[1]) % 5 != 0
    si = type("SI", (), dict(wi=wi, uv=uv))()
    for ctx in TD.CONTEXTS:
        c = mi.BSDFContext(*ctx)
        val, pdf = bsdf.eval_pdf(c, si, wo, active)
        assert float(val.abs().max()) == 0 and float(pdf.abs().max()) == 0
        bs, wgt = bsdf.sample(c, si, s1, s2, active)
        h = B.host_sample(mi, scene, ib, ctx, wi, uv, s1, s2, active)
        assert np.array_equal(bs.sampled_type.cpu().numpy().astype(np.uint32), h["sampled_type"]) and np.array_equal(bs.sampled_component.cpu().numpy().astype(np.uint32), h["sampled_component"])
        assert np.array_equal(bs.eta.cpu().numpy(), h["eta"]) and np.array_equal(bs.wo.cpu().numpy(), h["wo"])
        assert np.allclose(bs.pdf.cpu().numpy(), h["pdf"], **LEAF) and np.allclose(wgt.cpu().numpy(), h["weight"], **LEAF), (eta, colour, ctx)
        m = ~active
        assert (wgt.cpu().numpy()[:, m] == 0).all() and (bs.wo.cpu().numpy()[:, m] == 0).all()
    assert (h["sampled_type"] == TD.NULL).any()


# ------------------------------------------------------------------------------------------------ 5. per lane, no geometry behind

ETA1, ETA2 = "bk7/air", "diamond"
SEED = 3


def _through_both(n, seed=2, spread=0.9):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), np.full(n, 2.0)]).astype(np.float32)
    d = np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), np.full(n, -1.0)]); d = (d / np.linalg.norm(d, axis=0)).astype(np.float32)
    return o, d, np.full(n, np.inf, np.float32)


def _sample(mi, scene, o, d, maxt, seed=SEED):
    n = o.shape[1]
    sampler = mi.Sampler({"sample_count": 4, "seed": 5}); sampler.seed(seed, n)
    before = sampler.state.cpu().numpy().view(np.uint64).copy()
    spec, valid = scene.integrator().sample(scene, sampler, mi.Ray3f(o, d, maxt))
    return spec.cpu().numpy(), valid.cpu().numpy(), before, sampler.state.cpu().numpy().view(np.uint64)


def _draws(mi, O, n, before, count):
    sampler = mi.Sampler({"sample_count": 4, "seed": 5}); sampler.seed(SEED, n)
    state, inc = M.lane_seeds(O, sampler.m_seed_value, n)
    assert np.array_equal(state, before.astype(np.uint64))
    return np.stack([M.stream_draws(O, before[i], inc[i], count)[0] for i in range(n)]), inc


@pytest.mark.parametrize("max_depth", [8, 1])
def test_valid_ray_per_lane(mi, O, max_depth):
    """(a) two parallel panes, nothing else: valid == (d3 <= r'1) or (d9 <= r'2), d_k the k-th float of the lane's stream (six draws per vertex in JIT order), r' the
    restatement at the lane's |cos theta| = |d.z| (both panes face +z).  Lanes with |d - r'| <= 1e-6 are set aside (the product forms cos theta through the shading
    frame), at most 0.5 % of them -- the cap holds on the NumPy side alone.  Lanes that pass both panes and miss return the state after 18 draws; radiance is zero
    where `valid` is not set.  max_depth = 1: the last-vertex draw, valid == d3 <= r'1."""
    n = 1024
    scene = mi.load_dict(TD.two_panes(mi, TD.thin_dict(mi, ETA1), TD.thin_dict(mi, ETA2), max_depth=max_depth))
    o, d, maxt = _through_both(n)
    spec, valid, before, after = _sample(mi, scene, o, d, maxt)
    dr, inc = _draws(mi, O, n, before, 18)
    r1 = TD.r_prime(O, d[2], TD.ETAS[ETA1]); r2 = TD.r_prime(O, d[2], TD.ETAS[ETA2])
    aside = (np.abs(dr[:, 2] - r1) <= 1e-6) | (np.abs(dr[:, 8] - r2) <= 1e-6)
    assert aside.mean() <= 0.005
    refl1 = dr[:, 2] <= r1
    want = refl1 if max_depth == 1 else (refl1 | (dr[:, 8] <= r2))
    keep = ~aside
    assert np.array_equal(valid[keep], want[keep]), int((valid[keep] != want[keep]).sum())
    assert want.any() and (~want).any()
    checked = 0
    for i in np.nonzero(keep & ~want)[0][:200]:
        assert M.stream_draws(O, before[i], inc[i], 6 if max_depth == 1 else 18)[1] == int(after[i]); checked += 1
    assert checked > 50
    assert (spec[:, ~valid] == 0).all()
    print("valid_ray per lane, max_depth %d: %d of %d lanes valid, %d set aside" % (max_depth, int(want.sum()), n, int(aside.sum())))


def test_radiance_per_lane_under_a_constant_emitter(mi, O):
    """(b) one pane with colours R and T under a `constant` emitter of radiance E: spec == (d3 <= r' ? R : T) * E per lane at 1e-6 -- both lobes are delta, so the
    escaping ray meets the environment with MIS weight 1"""
    n = 1024; E = np.array([0.7, 1.1, 1.9], np.float32)
    d = TD.two_panes(mi, TD.thin_dict(mi, ETA1, "constants"), {"type": "diffuse"}, max_depth=4, emitter={"type": "constant", "radiance": {"type": "rgb", "value": [float(x) for x in E]}})
    d.pop("r2"); d.pop("m2")
    scene = mi.load_dict(d)
    o, dd, maxt = _through_both(n)
    spec, valid, before, _ = _sample(mi, scene, o, dd, maxt)
    dr, _ = _draws(mi, O, n, before, 6)
    rp = TD.r_prime(O, dd[2], TD.ETAS[ETA1])
    keep = np.abs(dr[:, 2] - rp) > 1e-6
    assert (~keep).mean() <= 0.005 and valid.all()
    refl = dr[:, 2] <= rp
    want = np.where(refl[None, :], (TD.R_RGB * E)[:, None], (TD.T_RGB * E)[:, None]).astype(np.float32)
    assert refl.any() and (~refl).any()
    assert np.allclose(spec[:, keep], want[:, keep], rtol=1e-6, atol=1e-7), float(np.abs(spec[:, keep] - want[:, keep]).max())


def test_valid_ray_prb_counts_null_interactions(mi):
    """(c) prb keeps depth != 0 (prb.py:332): every ray that meets a pane is valid, whatever lobe it samples there"""
    scene = mi.load_dict(TD.two_panes(mi, TD.thin_dict(mi, ETA1), TD.thin_dict(mi, ETA2), integrator="prb"))
    o, d, maxt = _through_both(512, spread=0.15)
    o[2, ::7] = -3.0                              # below both: a miss
    spec, valid, _, _ = _sample(mi, scene, o, d, maxt)
    assert np.array_equal(valid, o[2] > 0)


# ------------------------------------------------------------------------------------------------ 6. per lane, full transport, r' strictly inside (0, 1)

BLACK_WALL = {"type": "twosided", "w": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0, 0, 0]}}}
_EXPECTED = {}


def _chamber_pair(mi, integrator, rfilter):
    a = TD.chambers(mi, TD.thin_dict(mi, "bk7/air", "constants"), integrator=integrator); b = TD.chambers(mi, BLACK_WALL, integrator=integrator)
    for d in (a, b):
        d["sensor"]["fov"] = 40                         # every camera ray meets the pane first
        d["sensor"]["film"]["rfilter"] = {"type": rfilter}
    return a, b


def _compose(mi, O, osc, sv, lanes, inc, prb):
    """one pass over `lanes`: (rgb 3 x n, set aside n, reflected n, valid n, the lanes' sampler states after the path)"""
    f = np.float32; n = lanes["n"]
    t, u, v, prim, shape, inst = osc.ray_intersect(lanes["o"], lanes["d"], lanes["maxt"])
    si = osc.surface_interaction_flags(lanes["o"], lanes["d"], t, u, v, prim, shape, inst)
    p, ng, sn, ss, st, wi = si[0:3], si[3:6], si[6:9], si[9:12], si[12:15], si[15:18]
    assert np.isfinite(t).all() and (np.abs(p[2]) < 1e-5).all(), "a camera ray misses the pane"
    d3 = np.empty(n, f); adv = np.empty(n, np.uint64)
    for i in range(n):
        dr, s6 = M.stream_draws(O, lanes["state"][i], inc[i], 6); d3[i] = dr[2]; adv[i] = s6
    rp = TD.r_prime(O, wi[2], TD.ETAS["bk7/air"])
    assert ((rp > 0) & (rp < 1)).all()
    aside = np.abs(d3 - rp) <= 1e-6
    refl = d3 <= rp
    wo = np.where(refl[None, :], np.stack([-wi[0], -wi[1], wi[2]]), -wi).astype(f)
    wo_w = ((ss * wo[0]).astype(f) + (st * wo[1]).astype(f) + (sn * wo[2]).astype(f)).astype(f)
    mag = ((f(1) + np.abs(p).max(axis=0)).astype(f) * f(5.9604644775390625e-8 * 1500.0)).astype(f)
    mag = np.where((ng * wo_w).sum(axis=0) < 0, -mag, mag).astype(f)
    o2 = (p + ng * mag[None, :]).astype(f)
    rad, valid2, after = osc.integrator_sample(o2, wo_w, np.full(n, np.inf, f), seed=sv, lane_offset=0, state=adv, max_depth=2, rr_depth=8, prb=prb)
    colour = np.where(refl[None, :], TD.R_RGB[:, None], TD.T_RGB[:, None]).astype(f)
    # path.cpp:307-308: the sample is valid if a non-null lobe was sampled at the pane, or along the continuation; prb counts every surface it meets (prb.py:332)
    valid = np.ones(n, bool) if prb else (refl | valid2.astype(bool))
    return (colour * rad).astype(f), aside, refl, valid, after


def _expected_lanes(mi, O, integrator, seed, spp, rfilter="box"):
    """per lane of render(): the oracle's hit on the pane, the lobe from d3 against r' at the lane's |cos theta|, the continuation ray spawn_ray(+-) restated in float32,
    and the oracle's SamplingIntegrator::sample along it (max_depth 2, the lane's state advanced by the six draws of the first vertex) in the scene whose pane is a
    black two-sided wall: it occludes the same shadow rays and returns zero where a product path would meet the pane at its last vertex.
    (rgb 3 x n, lanes, set aside, reflected, valid)"""
    from tests import thinlens_cases as TL
    key = (integrator, seed, spp, rfilter)          # (the film record of the lanes carries the filter)
    if key in _EXPECTED:
        return _EXPECTED[key]
    a, b = _chamber_pair(mi, integrator, rfilter)
    scene = mi.load_dict(a); twin = mi.load_dict(b)
    osc, _ = O.scene_from_product(twin)
    sensor = scene.sensors()[0]
    sv = (sensor.sampler().m_base_seed + seed) & 0xffffffff
    lanes = TL.lanes_of(mi, O, sensor, sv, spp)
    _, inc = M.lane_seeds(O, sv, lanes["n"])
    rgb, aside, refl, valid, _ = _compose(mi, O, osc, sv, lanes, inc, integrator == "prb")
    _EXPECTED[key] = (rgb, lanes, aside, refl, valid)
    return _EXPECTED[key]


@pytest.mark.parametrize("integrator", ["path", "prb"])
def test_full_transport_per_lane(mi, O, integrator):
    """Integrator.sample over the camera rays of the 32 x 24 x 16 spp frame, started from the lanes' sampler states: relative L2 over all lanes 1e-4 against the
    composition of _expected_lanes; every lane is valid (the box is closed)"""
    import torch
    seed, spp = 4, SPP
    want, lanes, aside, refl, want_valid = _expected_lanes(mi, O, integrator, seed, spp)
    assert aside.mean() <= 0.005 and refl.any() and (~refl).any()
    scene = mi.load_dict(_chamber_pair(mi, integrator, "box")[0])
    n = lanes["n"]
    sampler = mi.Sampler({"sample_count": spp, "seed": 0}); sampler.seed((scene.sensors()[0].sampler().m_base_seed + seed) & 0xffffffff, n)
    sampler.state = torch.tensor(lanes["state"].view(np.int64), device=sampler.state.device)
    spec, valid = scene.integrator().sample(scene, sampler, mi.Ray3f(lanes["o"], lanes["d"], lanes["maxt"]))
    spec = spec.cpu().numpy(); keep = ~aside
    err = rel_l2(spec[:, keep], want[:, keep])
    print("full transport per lane, %s: rel L2 %.3g over %d lanes (%d set aside, %d reflected)" % (integrator, err, int(keep.sum()), int(aside.sum()), int(refl.sum())))
    assert np.abs(want).max() > 0 and err <= 1e-4
    assert np.array_equal(valid.cpu().numpy()[keep], want_valid[keep]) and want_valid.all()          # (the box is closed: every continuation meets a wall)
    # the lobe choice, lane by lane: R and T differ in every channel and the two continuations see different chambers, so a lane that took the other lobe misses this
    # bound by far (a lane-wise 1e-3: float32 transport of three vertices; lanes darker than 1e-3 of the brightest carry no information)
    bright = keep & (np.abs(want).max(axis=0) > 1e-3 * np.abs(want).max())
    assert bright.sum() > 1000 and (bright & refl).any() and (bright & ~refl).any() and np.allclose(spec[:, bright], want[:, bright], rtol=1e-3, atol=1e-6), int((~np.isclose(spec[:, bright], want[:, bright], rtol=1e-3, atol=1e-6)).any(axis=0).sum())


@pytest.mark.parametrize("integrator,rfilter", [(i, f) for i in ("path", "prb") for f in ("box", "gaussian")])
def test_full_transport_on_the_film(mi, O, integrator, rfilter):
    """mi.render equals orc_film_put of those lane radiances (box and gaussian filters, `path` and the `prb` primal) at 1e-4; a chunked render equals the unchunked one
    at 1e-6.  No lane of this seed lies within 1e-6 of its threshold (asserted)."""
    from tests import batch_cases as BC
    seed, spp = 4, SPP
    want, lanes, aside, _, _ = _expected_lanes(mi, O, integrator, seed, spp, rfilter)
    assert not aside.any()
    a, _ = _chamber_pair(mi, integrator, rfilter)
    img = mi.render(mi.load_dict(a), spp=spp, seed=seed).cpu().numpy()
    film = BC.film_put(O, lanes["wide"], rfilter, lanes, want)
    err = rel_l2(img, O.develop(film))
    a["integrator"]["chunk_lanes"] = 4096
    chunked = mi.render(mi.load_dict(a), spp=spp, seed=seed).cpu().numpy()
    ec = rel_l2(chunked, img)
    print("full transport on the film, %s / %s: rel L2 %.3g; chunked against unchunked %.3g" % (integrator, rfilter, err, ec))
    assert img.max() > 0 and err <= 1e-4 and ec <= 1e-6


def test_full_transport_two_passes(mi, O):
    """`path` with samples_per_pass = spp / 2: pass p of a lane continues the sampler where pass p - 1 left it (integrator.cpp:349-356), composed pass by pass as above;
    the raw film equals the composition at 1e-4, its weight channel at 2e-6"""
    from tests import batch_cases as BC
    from tests import thinlens_cases as TL
    seed, spp, per_pass = 4, SPP, SPP // 2
    a, b = _chamber_pair(mi, "path", "gaussian")
    scene = mi.load_dict(a); osc, _ = O.scene_from_product(mi.load_dict(b))
    sensor = scene.sensors()[0]
    # (render_film takes the seed as it is: the sampler's base seed is added by render())
    lanes = TL.lanes_of(mi, O, sensor, seed, per_pass); n = lanes["n"]
    _, inc = M.lane_seeds(O, seed, n)
    want = np.zeros((24, 32, 4), np.float32); near = 0
    for p in range(spp // per_pass):
        rgb, aside, _, _, state = _compose(mi, O, osc, seed, lanes, inc, False); near += int(aside.sum())
        want += BC.film_put(O, lanes["wide"], "gaussian", lanes, rgb)
        lanes = TL.lanes_of(mi, O, sensor, seed, per_pass, draws=TL.next_draws(O, seed, n, 2, state=state))
    assert near == 0
    it = mi.load_dict({"type": "path", "max_depth": 3, "rr_depth": 8, "samples_per_pass": per_pass})
    multi = it.render_film(scene, seed=seed, spp=spp).cpu().numpy()
    e_rgb, e_w = rel_l2(multi[..., :3], want[..., :3]), rel_l2(multi[..., 3], want[..., 3])
    print("full transport, two passes of %d spp: rgb %.3g, weights %.3g" % (per_pass, e_rgb, e_w))
    assert np.linalg.norm(want[..., :3]) > 0 and e_rgb <= 1e-4 and e_w <= 2e-6


# ------------------------------------------------------------------------------------------------ 7. exact-twin renders on the device

RES, SPP = (32, 24), 16
FRAME = M.binary_texels()


def _variant_kw(variant):
    return dict(instanced=variant == "instanced", frame=FRAME if variant == "framed" else None)


@pytest.mark.parametrize("integrator,variant", [(i, v) for i in ("path", "prb") for v in ("plain", "chunked", "instanced", "framed")])
def test_device_render_index_matched_against_oracle(mi, O, integrator, variant):
    """an index-matched pane (plain, chunked, inside an instanced shape group, nested in a `mask` with a 4 x 4 binary opacity bitmap) against the oracle's render of the same
    card as an index-matched `dielectric`: relative L2 1e-4, path and vertex counters equal.  (Under the frame, opacity 1 hands sample1 / 1 to the pane and opacity 0
    takes the mask's own null lobe: every quad passes the ray on with weight 1.)"""
    kw = _variant_kw(variant)
    product = TD.card_scene(mi, RES, SPP, TD.INDEX_MATCHED, integrator=integrator, **kw)
    if variant == "chunked":
        product["integrator"]["chunk_lanes"] = 4096
    scene = mi.load_dict(product)
    osc, osensor = O.scene_from_product(mi.load_dict(TD.card_scene(mi, RES, SPP, M.ABSENT, integrator=integrator, instanced=kw["instanced"])))
    it = scene.integrator()
    img = mi.render(scene, spp=SPP, seed=3).cpu().numpy()
    want, ost = (osc.render_path if integrator == "path" else osc.render_prb)(osensor, seed=3, spp=SPP, max_depth=it.max_depth, rr_depth=it.rr_depth)
    st = it.stats()
    err = rel_l2(img, want)
    print("index-matched pane %s / %s against the oracle: rel L2 %.3g, (paths, vertices) %s vs %s" % (integrator, variant, err, (st["paths"], st["vertices"]), (ost.paths, ost.vertices)))
    assert np.isfinite(img).all() and img.max() > 0 and err <= 1e-4 and (st["paths"], st["vertices"]) == (ost.paths, ost.vertices)


@pytest.mark.parametrize("integrator,variant", [(i, v) for i in ("path", "prb") for v in ("plain", "chunked", "instanced", "framed")])
def test_device_render_twin_of_mask_opacity_zero(mi, integrator, variant):
    """the same pane against the product's own `mask` of opacity 0 over a diffuse on an `rgba` film: 1e-6, alpha included.  `framed`: the pane under a `mask` with the
    4 x 4 binary opacity bitmap -- a null lobe of weight 1 on every quad, the frame's own or the pane's -- against the same twin (a mask cannot nest a mask)"""
    kw = _variant_kw(variant); film = {"pixel_format": "rgba"}
    a = TD.card_scene(mi, RES, SPP, TD.INDEX_MATCHED, integrator=integrator, film=film, **kw); b = TD.card_scene(mi, RES, SPP, TD.MASK_ZERO, integrator=integrator, film=film, instanced=kw["instanced"])
    if variant == "chunked":
        a["integrator"]["chunk_lanes"] = 4096; b["integrator"]["chunk_lanes"] = 4096
    ia = mi.render(mi.load_dict(a), spp=SPP, seed=3).cpu().numpy(); ib = mi.render(mi.load_dict(b), spp=SPP, seed=3).cpu().numpy()
    err = rel_l2(ia[..., :3], ib[..., :3]); ea = float(np.abs(ia[..., 3] - ib[..., 3]).max())
    print("pane against mask opacity 0, %s / %s: rel L2 %.3g, largest alpha difference %.3g" % (integrator, variant, err, ea))
    assert ia.shape[2] == 4 and ib[..., :3].max() > 0 and err <= 1e-6 and ea <= 1e-6 and ib[..., 3].min() >= 0


def test_rgba_film_of_two_panes(mi, O):
    """the `rgba` film of the two-pane scene: its alpha channel is orc_film_put of the per-lane flags (d3 <= r'1) or (d9 <= r'2), at 2e-6; lanes within 1e-6 of a
    threshold would move a pixel's alpha by a filter weight -- the chosen seed meets none (asserted on the NumPy side)"""
    from tests.test_gpu_mask import _film_flags
    seed, spp = 4, 4
    scene = mi.load_dict(TD.two_panes(mi, TD.thin_dict(mi, ETA1), TD.thin_dict(mi, ETA2), film={}, spp=spp))
    img = mi.render(scene, spp=spp, seed=seed).cpu().numpy()
    near = []

    def flag(dr, lanes, i):
        c = lanes["d"][2, i]
        r1 = float(TD.r_prime(O, [c], TD.ETAS[ETA1])[0]); r2 = float(TD.r_prime(O, [c], TD.ETAS[ETA2])[0])
        near.append(min(abs(float(dr[2]) - r1), abs(float(dr[8]) - r2)))
        return float(dr[2] <= r1 or dr[8] <= r2)

    alpha, flags, _ = _film_flags(mi, O, scene, seed, spp, flag)
    assert min(near) > 1e-6 and 0.02 < flags.mean() < 0.95
    assert np.allclose(img[..., 3], alpha, rtol=2e-6, atol=2e-6), float(np.abs(img[..., 3] - alpha).max())
    assert (img[..., :3][alpha == 0] == 0).all()


# ------------------------------------------------------------------------------------------------ 8. gradients through the pane

def _grad_in(res=RES, seed=9):
    return np.random.default_rng(seed).uniform(-1, 1, (res[1], res[0], 3)).astype(np.float32)


def _np(g):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in g.items()}


def _chambers(mi, pane, **kw):
    d = TD.chambers(mi, pane, **kw)
    d["integrator"]["emitter_gradients"] = True
    return d


@pytest.mark.parametrize("route", ["state_tape", "lane_cache"])
def test_gradients_through_an_index_matched_pane_against_oracle(mi, O, route):
    """(a) int_ior == ext_ior: the texel gradients of the wall behind the pane, of the other textures and of both emitters' radiances equal the oracle's
    render_prb_backward of the index-matched-dielectric twin at 1e-3.  `state_tape`: the default route of a backward pass; `lane_cache`: hide_emitters keeps the tape
    away and the adjoint replays from the lane-indexed cache (the record tape is not taken by such a scene)."""
    seed = 5; hide = route == "lane_cache"
    a = _chambers(mi, TD.INDEX_MATCHED, max_depth=4); b = _chambers(mi, M.ABSENT, max_depth=4)
    if hide:
        a["integrator"]["hide_emitters"] = True; b["integrator"]["hide_emitters"] = True
    scene = mi.load_dict(a); twin = mi.load_dict(b)
    osc, osensor = O.scene_from_product(twin); osc.set_hide_emitters(hide)
    g = _np(scene.integrator().render_backward(scene, None, _grad_in(), seed=seed, spp=SPP))
    g_refl, g_tex, g_emit, _ = osc.render_prb_backward_emitters(osensor, _grad_in(), seed=seed, spp=SPP, max_depth=4, rr_depth=8)
    errs = {}
    for name in ("wall_a", "wall_b", "side"):
        tb = [x for x in twin.bsdf_objs if x.id == name][0]
        errs[name] = rel_l2(g[name + ".reflectance.data"], g_tex[tb.tex_index].astype(np.float64))
        assert np.abs(g_tex[tb.tex_index]).max() > 0
    for k, key in enumerate(twin._emitter_order):
        gk = [v for kk, v in g.items() if kk.endswith("emitter.radiance.value") and kk.startswith(str(key).split(".")[0])]
        assert len(gk) == 1
        errs["emitter %d" % k] = rel_l2(gk[0].reshape(3), g_emit[k].astype(np.float64))
    print("gradients through an index-matched pane, %s:" % route, {k: "%.3g" % v for k, v in errs.items()})
    assert all(v <= 1e-3 for v in errs.values()), errs
    assert np.abs(g["glass.eta"]).max() == 0


def test_radiance_gradient_homogeneity(mi):
    """(b) bk7 / air: the render is homogeneous of degree one in the emitters' radiances and sampling does not depend on them, so sum grad_radiance * radiance ==
    sum w * image for the same seed, at 2e-4"""
    seed = 7
    scene = mi.load_dict(_chambers(mi, TD.thin_dict(mi, "bk7/air", "constants")))
    it = scene.integrator(); w = _grad_in(seed=10)
    img = it.render(scene, seed=seed, spp=SPP).cpu().numpy().astype(np.float64)
    g = _np(it.render_backward(scene, None, w, seed=seed, spp=SPP))
    p = mi.traverse(scene)
    lhs = sum(float((g[k].reshape(-1) * p[k].cpu().numpy().astype(np.float64).reshape(-1)).sum()) for k in g if k.endswith("emitter.radiance.value"))
    rhs = float((img * w).sum())
    print("homogeneity: sum grad_radiance * radiance = %.7g, sum w * image = %.7g, relative difference %.3g" % (lhs, rhs, abs(lhs - rhs) / abs(rhs)))
    assert abs(rhs) > 0 and abs(lhs - rhs) <= 2e-4 * abs(rhs)


def test_wall_texel_gradient_against_central_differences(mi):
    """(c) bk7 / air: the gradient of the texels of the wall BEHIND the pane along a random direction against central differences of the same-seed forward render.  Neither
    the pane's nor a diffuse wall's sampling depends on the texels and rr_depth > max_depth: the render is a polynomial in them; within 3 %"""
    import torch
    seed = 9
    scene = mi.load_dict(_chambers(mi, TD.thin_dict(mi, "bk7/air", "constants"), max_depth=4))
    it = scene.integrator(); grad_in = np.random.default_rng(8).uniform(0.5, 1.5, (RES[1], RES[0], 3)).astype(np.float32)
    loss = lambda: float((it.render(scene, seed=seed, spp=SPP).cpu().numpy().astype(np.float64) * grad_in).sum())
    grads = it.render_backward(scene, None, grad_in, seed=seed, spp=SPP)
    params = mi.traverse(scene); key = "wall_a.reflectance.data"
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


def test_forward_mode_against_gradient(mi):
    """(d) render_forward(tangent) against <grad, tangent> at 1e-3, for the texels of the wall behind the pane and for an emitter's radiance"""
    import torch
    seed = 6
    scene = mi.load_dict(_chambers(mi, TD.thin_dict(mi, "bk7/air", "constants"), max_depth=4))
    it = scene.integrator(); w = _grad_in(seed=13)
    g = _np(it.render_backward(scene, None, w, seed=seed, spp=SPP))
    p = mi.traverse(scene)
    for key in ("wall_a.reflectance.data", "light_a.emitter.radiance.value"):
        tan = np.random.default_rng(22).uniform(-1, 1, tuple(p[key].shape)).astype(np.float32)
        fwd = it.render_forward(scene, None, seed=seed, spp=SPP, tangents={key: torch.tensor(tan)}).cpu().numpy().astype(np.float64)
        lhs = float((fwd * w).sum()); rhs = float((g[key].reshape(tan.shape) * tan).sum())
        print("forward mode against <grad, tangent>, %s: %.7g %.7g" % (key, lhs, rhs))
        assert abs(rhs) > 0 and abs(lhs - rhs) <= 1e-3 * abs(rhs)


def test_rough_parameter_gradients_on_other_surfaces(mi, O):
    """alpha / eta / k of the roughconductor block behind an index-matched pane (`bsdf_parameter_gradients`) against the oracle's render_prb_backward_bsdf_params of the
    index-matched-dielectric twin at 1e-3"""
    seed = 5
    a = _chambers(mi, TD.INDEX_MATCHED, max_depth=4); b = _chambers(mi, M.ABSENT, max_depth=4)
    a["integrator"]["bsdf_parameter_gradients"] = True
    scene = mi.load_dict(a); twin = mi.load_dict(b)
    osc, osensor = O.scene_from_product(twin)
    g = _np(scene.integrator().render_backward(scene, None, _grad_in(), seed=seed, spp=SPP))
    g_x, _ = osc.render_prb_backward_bsdf_params(osensor, _grad_in(), seed=seed, spp=SPP, max_depth=4, rr_depth=8)
    rec = g_x[[x for x in twin.bsdf_objs if x.id == "metal"][0].index].astype(np.float64)
    errs = {"alpha": abs(float(g["metal.alpha.value"].reshape(-1)[0]) - rec[0:2].sum()) / abs(rec[0:2].sum()),
            "eta": rel_l2(g["metal.eta.value"].reshape(3), rec[2]), "k": rel_l2(g["metal.k.value"].reshape(3), rec[3])}
    print("rough parameters behind an index-matched pane:", {k: "%.3g" % v for k, v in errs.items()})
    assert np.abs(rec[0:4]).max() > 0 and all(v <= 1e-3 for v in errs.values()), errs


GRAD_KEYS = ["wall_a.reflectance.data", "glass.specular_transmittance.value", "glass.specular_reflectance.value", "glass.eta"]


@pytest.mark.parametrize("size,bar", [(((8, 8), 1), 0.0), ((RES, SPP), 1e-4)])
def test_autograd_equals_render_backward_and_own_keys_are_zero(mi, size, bar):
    """(e) `mi.render` + autograd against `render_backward`: bit for bit on one wave (8 x 8, 1 spp), 1e-4 at 32 x 24 x 16 spp (the float atomics' order, docs/parity.md,
    "blendbsdf"); (f) the pane's own keys come back as zeros of the parameters' shapes from both"""
    import torch
    res, spp = size
    scene = mi.load_dict(_chambers(mi, TD.thin_dict(mi, "bk7/air", "constants"), res=res, spp=spp))
    params = mi.traverse(scene)
    for k in GRAD_KEYS:
        params[k].requires_grad_()
    img = mi.render(scene, params, spp=spp, seed=4)
    x = torch.tensor(np.random.default_rng(3).uniform(-1, 1, tuple(img.shape)).astype(np.float32), device=img.device)
    (img * x).sum().backward()
    direct = scene.integrator().render_backward(scene, params, x, seed=mi.sample_tea_32(4, 1)[0], spp=spp)
    k = GRAD_KEYS[0]
    a = params[k].grad.cpu().numpy(); b = direct[k].reshape(params[k].shape).cpu().numpy()
    err = rel_l2(a, b)
    print("autograd against render_backward, %s x %d spp: %s %.3g" % (res, spp, k, err))
    assert np.abs(b).max() > 0 and (np.array_equal(a, b) if bar == 0.0 else err <= bar)
    for k in GRAD_KEYS[1:]:
        assert tuple(params[k].grad.shape) == tuple(params[k].shape) and float(params[k].grad.abs().max()) == 0 and float(direct[k].abs().max()) == 0


def test_bitmap_transmittance_renders_and_its_texels_have_zero_gradient(mi):
    tex = TD.nearest_texels()
    scene = mi.load_dict(_chambers(mi, {"type": "thindielectric", "specular_transmittance": {"type": "bitmap", "data": tex, "raw": True}}))
    g = scene.integrator().render_backward(scene, None, _grad_in(), seed=2, spp=SPP)
    assert tuple(g["glass.specular_transmittance.data"].shape) == tex.shape and float(g["glass.specular_transmittance.data"].abs().max()) == 0
    assert float(g["wall_a.reflectance.data"].abs().max()) > 0


def test_refusals_are_named_and_the_process_keeps_rendering(mi):
    """(g) what a scene with a pane refuses, scene-wide, with the feature in the message"""
    import torch
    scene = mi.load_dict(_chambers(mi, TD.thin_dict(mi, "bk7/air", "constants"), spp=4))
    it = scene.integrator(); ones = np.ones((RES[1], RES[0], 3), np.float32)
    it.shape_gradients = True
    with pytest.raises(RuntimeError, match="thindielectric"):
        it.render_backward(scene, None, ones, seed=0, spp=4)
    it.shape_gradients = False
    # a pane next to a composite record runs the widest set, which has neither the alpha / eta / k terms nor the item-writing adjoint of forward mode
    wide = _chambers(mi, TD.thin_dict(mi, "bk7/air"), spp=4); wide["side"] = {"type": "mask", "opacity": 0.9, "m": dict(wide["side"])}
    wide = mi.load_dict(wide)
    with pytest.raises(RuntimeError, match="thindielectric.*render_forward"):
        wide.integrator().render_forward(wide, None, seed=1, spp=4, tangents={"wall_a.reflectance.data": torch.ones(6, 5, 3)})
    mq = _chambers(mi, TD.thin_dict(mi, "bk7/air"), spp=4, integrator="path"); mq["integrator"].pop("emitter_gradients"); mq["integrator"]["material_queues"] = True
    mq = mi.load_dict(mq)
    with pytest.raises(RuntimeError, match="thindielectric.*material_queues"):
        mi.render(mq, spp=4, seed=0)
    deep = mi.load_dict(_chambers(mi, TD.thin_dict(mi, "bk7/air"), spp=4, max_depth=14))
    with pytest.raises(RuntimeError, match="thindielectric.*max_depth must not exceed"):
        deep.integrator().render_backward(deep, None, ones, seed=0, spp=4)
    nocache = _chambers(mi, TD.thin_dict(mi, "bk7/air"), spp=4); nocache["integrator"]["replay_cache"] = False
    nocache = mi.load_dict(nocache)
    with pytest.raises(RuntimeError, match="thindielectric.*replay cache"):
        nocache.integrator().render_backward(nocache, None, ones, seed=0, spp=4)
    with pytest.raises(RuntimeError, match="Only materials without a transmission component can be nested"):
        mi.load_dict({"type": "twosided", "x": {"type": "thindielectric"}})
    g = it.render_backward(scene, None, ones, seed=0, spp=4)          # ... and the process keeps rendering
    assert float(g["wall_a.reflectance.data"].abs().max()) > 0 and float(mi.render(scene, spp=4, seed=0).max()) > 0


# ------------------------------------------------------------------------------------------------ 9. aov

def test_aov_device_equals_host_and_albedo_is_zero(mi):
    """depth / normal / position / shape_index / albedo with the pane as first hit: the device equals the host twin bit for bit, the geometric channels are the pane's
    (depth = the distance to the plane z = 0), the albedo is the base-class value eval(wo = (0, 0, 1)) * pi = 0"""
    import torch
    scene = mi.load_dict(TD.chambers(mi, TD.thin_dict(mi, "bk7/air", "constants")))
    n = 4096; rng = np.random.default_rng(6)
    o = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.6, 0.6, n), np.full(n, 1.5)]).astype(np.float32)
    d = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), np.full(n, -1.0)]); d = (d / np.linalg.norm(d, axis=0)).astype(np.float32)
    maxt = np.full(n, np.inf, np.float32)
    aov = mi.load_dict({"type": "aov", "aovs": "ab:albedo,dd:depth,nn:sh_normal,pp:position,si:shape_index"})
    dev = aov.sample(scene, mi.Ray3f(torch.tensor(o), torch.tensor(d), torch.tensor(maxt))).cpu().numpy()
    host = aov.sample_host(scene, o, d, maxt)
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))
    si = scene.ray_intersect(mi.Ray3f(torch.tensor(o), torch.tensor(d), torch.tensor(maxt)))          # har_ray_intersect: the geometric channels are the first hit's
    assert np.array_equal(dev[3], si.t.cpu().numpy()) and np.array_equal(dev[7:10], si.p.cpu().numpy()) and np.array_equal(dev[4:7], si.sh_frame.n.cpu().numpy())
    assert (dev[0:3] == 0).all() and np.allclose(dev[3], 1.5 / -d[2], rtol=1e-5) and np.allclose(dev[9], 0.0, atol=1e-6) and np.allclose(np.abs(dev[6]), 1.0, atol=1e-6)
    assert len(np.unique(dev[10])) == 1 and dev[10][0] > 0
