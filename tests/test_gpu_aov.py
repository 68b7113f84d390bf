"""The `aov` integrator on the GPU: har_aov_sample against its host twin and against har_ray_intersect, the AOV film of har_render_aovs against a film composed
from oracle calls only, consistency with the children's radiance, lane partitions / chunks, autograd through a `prb` child, refusals."""
import numpy as np
import pytest

from tests import aov_cases as A

pytestmark = pytest.mark.gpu

FILM_TYPES = ["depth", "sh_normal", "albedo", "position", "uv", "prim_index", "shape_index"]
FILM_SPEC = ",".join("f%d:%s" % (i, t) for i, t in enumerate(FILM_TYPES))


def cornell(mi, res=64, spp=4, rfilter="gaussian", film_extra=None):
    d = mi.cornell_box()
    d["sensor"]["film"].update({"width": res, "height": res, "rfilter": {"type": rfilter}})
    d["sensor"]["film"].update(film_extra or {})
    d["sensor"]["sampler"]["sample_count"] = spp
    return d


def test_device_equals_host_bit_for_bit(mi):
    import torch
    scene = mi.load_dict(A.feature_scene(mi))
    aov = mi.load_dict({"type": "aov", "aovs": A.ALL_SPEC})
    o, d, maxt, active = A.feature_rays()
    ray = mi.Ray3f(torch.tensor(o, device="cuda"), torch.tensor(d, device="cuda"), torch.tensor(maxt, device="cuda"))
    act = torch.tensor(active, device="cuda")
    dev = aov.sample(scene, ray, active=act).cpu().numpy()
    host = aov.sample_host(scene, o, d, maxt, active)
    assert dev.shape == host.shape == (23, o.shape[1])
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))
    assert (dev[:, ~active] == 0).all()
    # geometric channels == the rows of har_ray_intersect of the same build, bit for bit
    si = scene.ray_intersect(ray, active=act)
    hit = np.isfinite(si.t.cpu().numpy()) & active
    sl, _ = A.channel_slices(A.ALL_TYPES)
    for name, field in (("position", si.p), ("geo_normal", si.n), ("sh_normal", si.sh_frame.n), ("uv", si.uv), ("depth", si.t.reshape(1, -1)),
                        ("dp_du", si.dp_du), ("dp_dv", si.dp_dv)):
        rows = np.ascontiguousarray(field.cpu().numpy())
        assert np.array_equal(np.ascontiguousarray(dev[sl[name]][:, hit]).view(np.uint32), np.ascontiguousarray(rows[:, hit]).view(np.uint32)), name
    assert np.array_equal(dev[sl["prim_index"]][0][hit], si.prim_index.cpu().numpy()[hit].astype(np.float32))
    assert (dev[:, ~hit] == 0).all() and 0.2 < hit.mean() < 0.9


FILM_CASES = [(rf, extra) for rf in ("box", "gaussian", "catmullrom") for extra in (None, "border_crop")]


@pytest.mark.parametrize("which", ["cornell", "feature"])
@pytest.mark.parametrize("rfilter,extra", FILM_CASES)
def test_aov_film_against_oracle_composition(mi, O, which, rfilter, extra):
    """the expected film comes from oracle calls only (tests/aov_cases.py: sampler stream -> film position -> sensor ray -> intersection -> interaction -> film put)"""
    res, spp, seed = (64, 4, 3) if which == "cornell" else (48, 8, 5)
    fe = None
    if extra:
        fe = {"sample_border": True, "crop_offset_x": 5, "crop_offset_y": 9, "crop_width": res - 14, "crop_height": res - 20}
    d = cornell(mi, res, spp, rfilter, fe) if which == "cornell" else A.feature_scene(mi, res, spp, rfilter, fe)
    scene = mi.load_dict(d)
    osc, sensor = O.scene_from_product(scene)
    aov = mi.load_dict({"type": "aov", "aovs": FILM_SPEC})
    want, lanes = A.oracle_aov_film(O, scene, osc, sensor, rfilter, FILM_TYPES, seed, spp)
    got = aov.render(scene, seed=seed, spp=spp, develop=False).cpu().numpy()
    sl, count = A.channel_slices(FILM_TYPES)
    assert got.shape == want.shape == (sensor.crop_height, sensor.crop_width, count + 1)
    # (a) the weight channel: O.render_weights, at the bound tests/test_gpu_headline.py::test_splat_gather_at_high_sample_counts uses for it -- which also pins that
    # the oracle-side film positions were composed correctly, before any AOV is compared
    wref = O.render_weights(sensor, seed, spp)[:, :, 3]
    print(which, rfilter, extra, "weights: composition", A.rel_l2(want[:, :, count], wref), "device", A.rel_l2(got[:, :, count], wref))
    assert A.rel_l2(want[:, :, count], wref) < 2e-6
    assert A.rel_l2(got[:, :, count], wref) < 2e-6
    # (b) every AOV type on its own at the forward image bar
    for name in FILM_TYPES:
        e = A.rel_l2(got[:, :, sl[name]], want[:, :, sl[name]])
        print("   ", name, e)
        assert e <= 1e-4, (name, e)
    # (c) integer AOVs on pixels all of whose contributing lanes hit the same primitive (box filter: the lanes of the pixel)
    if rfilter == "box" and not extra:
        prim = lanes["vals"][sl["prim_index"]][0].reshape(-1, spp); hit = lanes["hit"].reshape(-1, spp)
        shp = lanes["vals"][sl["shape_index"]][0].reshape(-1, spp)
        pure = hit.all(1) & (prim == prim[:, :1]).all(1) & (shp == shp[:, :1]).all(1)
        if which == "cornell":
            assert pure.mean() >= 0.5, pure.mean()                 # a condition on the input, checked on the oracle side
        dev = aov.render(scene, seed=seed, spp=spp).cpu().numpy().reshape(-1, count)
        for name, ref in (("prim_index", prim[:, 0]), ("shape_index", shp[:, 0])):
            g = dev[:, sl[name]][:, 0][pure]; r = ref[pure]
            assert np.all(np.abs(g - r) <= 1e-4 * np.maximum(np.abs(r), 1.0)), name
            assert (r > 0).any() or name == "prim_index"


def test_radiance_consistency_with_children(mi):
    import torch
    spp, seed = 16, 7
    scene = mi.load_dict(cornell(mi, 64, spp))
    path = mi.load_dict({"type": "path", "max_depth": 6})
    ref = path.render(scene, seed=seed, spp=spp)
    aov = mi.load_dict({"type": "aov", "aovs": "dd:depth,nn:sh_normal", "img": {"type": "path", "max_depth": 6}})
    out = aov.render(scene, seed=seed, spp=spp)
    assert out.shape == (64, 64, 3 + 4)
    assert A.rel_l2(out[..., :3].cpu().numpy(), ref.cpu().numpy()) <= 1e-6
    two = mi.load_dict({"type": "aov", "aovs": "dd:depth", "a": {"type": "path", "max_depth": 6}, "b": {"type": "path", "max_depth": 6}})
    o2 = two.render(scene, seed=seed, spp=spp).cpu().numpy()
    assert o2.shape == (64, 64, 7) and A.rel_l2(o2[..., 0:3], o2[..., 3:6]) <= 1e-6 and A.rel_l2(o2[..., 6], out[..., 3].cpu().numpy()) <= 1e-6
    assert float(out[16:48, 16:48, 3].min()) > 2.0                  # the camera stands 3.9 in front of a box of depth 2: the central rays all hit something
    # rgba film: 4 + 4 channels
    sa = mi.load_dict(cornell(mi, 64, spp, film_extra={"pixel_format": "rgba"}))
    o4 = two.render(sa, seed=seed, spp=spp).cpu().numpy()
    r4 = path.render(sa, seed=seed, spp=spp).cpu().numpy()
    assert o4.shape == (64, 64, 9) and r4.shape == (64, 64, 4)
    assert A.rel_l2(o4[..., 0:4], r4) <= 1e-6 and A.rel_l2(o4[..., 4:8], r4) <= 1e-6
    # hide_emitters on the child: the radiance hides the lamp, the depth still sees it
    hid = mi.load_dict({"type": "aov", "aovs": "dd:depth", "img": {"type": "path", "max_depth": 6, "hide_emitters": True}})
    oh = hid.render(scene, seed=seed, spp=spp).cpu().numpy()
    rh = mi.load_dict({"type": "path", "max_depth": 6, "hide_emitters": True}).render(scene, seed=seed, spp=spp).cpu().numpy()
    assert A.rel_l2(oh[..., :3], rh) <= 1e-6 and A.rel_l2(rh, ref.cpu().numpy()) > 1e-3
    assert A.rel_l2(oh[..., 3], out[..., 3].cpu().numpy()) <= 1e-6
    # the scene's own integrator
    sc = mi.load_dict(dict(cornell(mi, 64, spp), integrator={"type": "aov", "aovs": "dd:depth,nn:sh_normal", "img": {"type": "path", "max_depth": 6}}))
    assert A.rel_l2(mi.render(sc, seed=seed, spp=spp).cpu().numpy(), out.cpu().numpy()) <= 1e-6


def test_partitions_chunks_and_the_per_lane_splat(mi, O):
    spp, seed = 8, 2
    scene = mi.load_dict(A.feature_scene(mi, 48, spp))
    aov = mi.load_dict({"type": "aov", "aovs": FILM_SPEC})
    full = aov.render_aov_film(scene, seed=seed, spp=spp)
    n = 48 * 48 * spp; k = 5000
    part = aov.render_aov_film(scene, seed=seed, spp=spp, lanes=(0, k))
    part = aov.render_aov_film(scene, seed=seed, spp=spp, lanes=(k, n), film=part)
    assert A.rel_l2(part.cpu().numpy(), full.cpu().numpy()) <= 1e-6
    small = mi.load_dict({"type": "aov", "aovs": FILM_SPEC, "chunk_lanes": 6144})          # 18432 lanes: three chunks
    assert A.rel_l2(small.render_aov_film(scene, seed=seed, spp=spp).cpu().numpy(), full.cpu().numpy()) <= 1e-6
    # film window: the rows a band of lanes can reach
    lo, hi = 10, 30
    band = aov.render_aov_film(scene, seed=seed, spp=spp, lanes=(16 * 48 * spp, 24 * 48 * spp), film_window=(lo, hi - lo))
    whole = aov.render_aov_film(scene, seed=seed, spp=spp, lanes=(16 * 48 * spp, 24 * 48 * spp))
    assert A.rel_l2(band.cpu().numpy(), whole[lo:hi].cpu().numpy()) <= 1e-6 and float(whole[:lo].abs().sum() + whole[hi:].abs().sum()) == 0.0
    with pytest.raises(RuntimeError, match="film_window"):
        aov.render_aov_film(scene, seed=seed, spp=spp, film_window=(lo, hi - lo))
    # spp not a power of two, width * spp not a multiple of 256: the per-lane splat path, held to 5 (b)
    res, spp = 37, 3
    for rfilter in ("box", "gaussian"):
        sc = mi.load_dict(A.feature_scene(mi, res, spp, rfilter))
        osc, sensor = O.scene_from_product(sc)
        want, _ = A.oracle_aov_film(O, sc, osc, sensor, rfilter, FILM_TYPES, seed, spp)
        got = aov.render(sc, seed=seed, spp=spp, develop=False).cpu().numpy()
        sl, count = A.channel_slices(FILM_TYPES)
        assert A.rel_l2(got[:, :, count], O.render_weights(sensor, seed, spp)[:, :, 3]) < 2e-6
        for name in FILM_TYPES:
            assert A.rel_l2(got[:, :, sl[name]], want[:, :, sl[name]]) <= 1e-4, (rfilter, name)


def test_autograd_through_a_prb_child(mi):
    """test06_backward: the gradient of a loss on the radiance channels is the bare prb integrator's; a loss that touches an AOV channel is refused"""
    import torch
    spp = 16
    d = cornell(mi, 48, spp); d["integrator"] = {"type": "prb", "max_depth": 4}
    key = "red.reflectance.value"

    def grad(make_integrator, loss):
        scene = mi.load_dict(d)
        params = mi.traverse(scene); params[key].requires_grad_()
        img = mi.render(scene, params, integrator=make_integrator(), seed=4, seed_grad=9, spp=spp)
        loss(img).backward()
        return params[key].grad.cpu().numpy().copy()

    bare = grad(lambda: mi.load_dict({"type": "prb", "max_depth": 4}), lambda im: (im ** 2).mean())
    wrapped = grad(lambda: mi.load_dict({"type": "aov", "aovs": "dd:depth,ab:albedo", "img": {"type": "prb", "max_depth": 4}}), lambda im: (im[..., :3] ** 2).mean())
    assert np.abs(bare).max() > 0 and A.rel_l2(wrapped, bare) <= 1e-6, (wrapped, bare)
    with pytest.raises(RuntimeError, match="gradients through the AOV channels"):
        grad(lambda: mi.load_dict({"type": "aov", "aovs": "dd:depth,ab:albedo", "img": {"type": "prb", "max_depth": 4}}), lambda im: (im ** 2).mean())


def test_refusals_on_the_gpu(mi):
    scene = mi.load_dict(cornell(mi, 32, 4))
    aov = mi.load_dict({"type": "aov", "aovs": "dd:depth", "img": {"type": "prb"}})
    with pytest.raises(RuntimeError, match="`aov` integrator is not implemented"):
        mi.DeviceGroup(scene, devices=(0,), integrator=aov)
    with pytest.raises(RuntimeError, match="`aov` integrator is not implemented"):
        aov.render_forward(scene)
    mi.set_variant("scalar_rgb")
    try:
        with pytest.raises(RuntimeError, match="scalar_rgb"):
            mi.render(scene, integrator=aov, spp=1)
    finally:
        mi.set_variant("hip_ad_rgb")
