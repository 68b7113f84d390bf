"""The `thinlens` sensor (src/sensors/thinlens.cpp; HarSensor::projection = 2) without a GPU: the host twin of the per-lane ray code against a float64 restatement, the
expectations of src/sensors/tests/test_thinlens.py:42-111, the focal-plane property, loader / traverse / refusals, and the sampler stream of the host render path
(four draws before the first vertex) with its film against the film composed from oracle calls (tests/thinlens_cases.py)."""
import warnings

import numpy as np
import pytest

from tests import batch_cases as B
from tests import thinlens_cases as T


ORIGINS = [[1.0, 0.0, 1.5], [1.0, 4.0, 1.5]]
DIRECTIONS = [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]


def _reference_camera(mi, o, d, aperture=0.1, focus=15.0, near_clip=1.0, **extra):
    """create_camera of src/sensors/tests/test_thinlens.py:8-29"""
    c = {"type": "thinlens", "near_clip": near_clip, "far_clip": 35.0, "focus_distance": focus, "aperture_radius": aperture, "fov": 34, "fov_axis": "x",
         "shutter_open": 1.5, "shutter_close": 5,
         "to_world": mi.ScalarTransform4f().look_at(origin=o, target=[o[i] + d[i] for i in range(3)], up=[0, 1, 0]),
         "film": {"type": "hdrfilm", "width": 512, "height": 256}}
    c.update(extra)
    return mi.load_dict(c)


@pytest.fixture(scope="module")
def pairs():
    return T.sample_pairs(20000)


@pytest.mark.parametrize("fov_axis", ["x", "y", "diagonal"])
def test_host_twin_against_float64_restatement(mi, O, pairs, fov_axis):
    pos, ap = pairs
    film = {"type": "hdrfilm", "width": 96, "height": 64, "crop_offset_x": 10, "crop_offset_y": 7, "crop_width": 50, "crop_height": 33}
    for aperture in (0.01, 0.1, 0.25):
        for focus in (15.0, 25.0):
            cam = _reference_camera(mi, ORIGINS[1], [1.0, -0.3, 0.2], aperture, focus, fov_axis=fov_axis, film=dict(film))
            o, d, mt = cam.sample_ray_host(pos, ap)
            o64, d64, mt64, _ = T.thinlens_rays64(O, cam.har, pos[0], pos[1], ap[0], ap[1])
            for name, got, want in (("o", o, o64), ("d", d, d64), ("maxt", mt, mt64)):
                err = np.abs(got - want) - 3e-6 * np.abs(want)
                assert np.isfinite(got).all() and err.max() <= 3e-7, (fov_axis, aperture, focus, name, err.max())
            assert np.abs(np.linalg.norm(d.astype(np.float64), axis=0) - 1).max() <= 1e-6
    # a null aperture sample is the centre of the lens, and a pinhole camera ignores the sample
    o0, d0, m0 = cam.sample_ray_host(pos)
    o1, d1, m1 = cam.sample_ray_host(pos, np.full_like(pos, 0.5))
    assert np.array_equal(o0.view(np.uint32), o1.view(np.uint32)) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32)) and np.array_equal(m0.view(np.uint32), m1.view(np.uint32))
    pin = mi.load_dict(B.child_dicts(mi, "p")[0])
    for x, y in zip(pin.sample_ray_host(pos, ap), pin.sample_ray_host(pos)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("origin", ORIGINS)
@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("aperture", [0.01, 0.1, 0.25])
@pytest.mark.parametrize("focus", [15.0, 25.0])
def test_reference_expectations(mi, O, origin, direction, aperture, focus):
    """src/sensors/tests/test_thinlens.py:42-55 (test01_create) and :58-111 (test02_sample_ray)"""
    near_clip = 1.0
    cam = _reference_camera(mi, origin, direction, aperture, focus, near_clip)
    assert cam.needs_aperture_sample() and cam.near_clip == 1.0 and cam.far_clip == 35.0 and cam.focus_distance() == focus
    if focus == 15.0:
        assert _reference_camera(mi, origin, direction).focus_distance() == 15
    m = np.asarray(cam.to_world.matrix, np.float64).reshape(4, 4); inv = np.linalg.inv(m)
    pos = np.array([[0.2, 0.1, 0.2], [0.6, 0.9, 0.2]], np.float32)
    o, d, _ = cam.sample_ray_host(pos, np.full((2, 3), 0.5, np.float32))
    for k in range(3):
        local = inv[:3, :3] @ d[:, k].astype(np.float64)
        assert np.abs(o[:, k] - (np.asarray(origin) + near_clip / local[2] * d[:, k].astype(np.float64))).max() <= 1e-4          # ray.o lies on the near plane
    o, d, _ = cam.sample_ray_host(np.full((2, 1), 0.5, np.float32), np.full((2, 1), 0.5, np.float32))
    assert np.abs(d[:, 0] - np.asarray(direction)).max() <= 1e-7
    # aperture sampling (:93-111)
    ap = np.array([[0.9, 0.4, 0.2], [0.6, 0.9, 0.7]], np.float32)
    centre = np.full((2, 3), 0.5, np.float32)
    o, d, _ = cam.sample_ray_host(centre, ap)
    oc, dc, _ = cam.sample_ray_host(centre, centre)
    lens = aperture * T.disk(O, ap[0], ap[1]).astype(np.float64)
    aperture_v = m[:3, :3] @ np.stack([lens[0], lens[1], np.zeros(3)])
    for k in range(3):
        izc = 1.0 / (inv[:3, :3] @ dc[:, k].astype(np.float64))[2]; iz = 1.0 / (inv[:3, :3] @ d[:, k].astype(np.float64))[2]
        o_centred = oc[:, k] - near_clip * izc * dc[:, k].astype(np.float64)
        assert np.abs(o[:, k] - (o_centred + aperture_v[:, k] + near_clip * iz * d[:, k].astype(np.float64))).max() <= 1e-4
        want = dc[:, k].astype(np.float64) * focus - aperture_v[:, k]
        assert np.abs(d[:, k] - want / np.linalg.norm(want)).max() <= 1e-4


@pytest.mark.parametrize("aperture,focus", [(0.25, 15.0), (0.1, 25.0), (0.3, 3.9)])
def test_rays_of_one_film_position_meet_on_the_focal_plane(mi, O, aperture, focus):
    cam = _reference_camera(mi, ORIGINS[0], [0.3, -0.2, 1.0], aperture, focus, near_clip=0.05, far_clip=100.0)
    ap = np.random.default_rng(5).uniform(0, 1, (2, 256)).astype(np.float32)
    worst = 0.0
    for fx, fy in ((0.5, 0.5), (0.03, 0.97), (0.8, 0.15)):
        pos = np.tile(np.array([[fx], [fy]], np.float32), (1, 256))
        o, d, _ = cam.sample_ray_host(pos, ap)
        _, _, _, focus_w = T.thinlens_rays64(O, cam.har, pos[0], pos[1], ap[0], ap[1])          # to_world * focus_p
        v = focus_w - o.astype(np.float64)
        dist = np.linalg.norm(np.cross(v.T, d.astype(np.float64).T), axis=1)
        along = (v * d.astype(np.float64)).sum(axis=0)
        assert (along > 0).all()                      # the point lies ahead of every origin
        worst = max(worst, float(dist.max()))
    print("largest distance of a ray from the focus point", worst, "bar", 1e-5 * focus)
    assert worst <= 1e-5 * focus
    assert np.linalg.norm(o - o[:, :1], axis=0).max() > 0.5 * aperture          # and the origins do spread over the lens


def test_loader_parameters_and_refusals(mi):
    import torch
    Tr = mi.ScalarTransform4f
    xml = """<sensor version="3.0.0" type="thinlens">
        <float name="fov" value="40"/><float name="aperture_radius" value="0.2"/><float name="focus_distance" value="3.5"/>
        <float name="near_clip" value="0.1"/><float name="far_clip" value="50"/>
        <transform name="to_world"><lookat origin="0, 0, 3.9" target="0, 0, 0" up="0, 1, 0"/></transform>
        <film type="hdrfilm"><integer name="width" value="64"/><integer name="height" value="16"/><rfilter type="box"/></film>
    </sensor>"""
    d = {"type": "thinlens", "fov": 40.0, "aperture_radius": 0.2, "focus_distance": 3.5, "near_clip": 0.1, "far_clip": 50.0,
         "to_world": Tr().look_at(origin=[0, 0, 3.9], target=[0, 0, 0], up=[0, 1, 0]), "film": {"type": "hdrfilm", "width": 64, "height": 16, "rfilter": {"type": "box"}}}
    a = mi.load_string(xml); b = mi.load_dict(d)
    assert a.kind == b.kind == "thinlens" and bytes(a.har) == bytes(b.har) and a.har.projection == 2
    assert abs(a.har.aperture_radius - 0.2) < 1e-7 and a.har.focus_distance == 3.5
    # the perspective record of the same camera differs in `projection` and in the two words a thin lens keeps its parameters in (a pinhole: the principal point offsets)
    p = mi.load_dict(dict({k: v for k, v in d.items() if k != "aperture_radius"}, type="perspective"))
    assert list(p.har.sample_to_camera) == list(a.har.sample_to_camera) and p.har.projection == 0 and p.har.principal_point_offset_x == 0 and p.har.principal_point_offset_y == 0
    assert len(bytes(p.har)) == len(bytes(a.har)) and sum(x != y for x, y in zip(bytes(p.har), bytes(a.har))) <= 9
    assert not p.needs_aperture_sample()
    no_focus = mi.load_dict({k: v for k, v in d.items() if k != "focus_distance"})
    assert no_focus.focus_distance() == 50.0 and no_focus.har.focus_distance == 50.0          # sensor.cpp:127: far_clip
    with pytest.raises(RuntimeError, match='Property "aperture_radius" has not been specified!'):
        mi.load_dict({k: v for k, v in d.items() if k != "aperture_radius"})
    with pytest.raises(RuntimeError, match="Unreferenced property"):
        mi.load_dict(dict(d, principal_point_offset_x=0.1))
    with pytest.raises(RuntimeError, match="Unreferenced property"):
        mi.load_dict(dict(d, lens_shape="round"))
    with pytest.raises(RuntimeError, match="Scale factors in the camera-to-world transformation are not allowed!"):
        mi.load_dict(dict(d, to_world=Tr().look_at(origin=[0, 0, 3.9], target=[0, 0, 0], up=[0, 1, 0]).scale([2.0, 2.0, 2.0])))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        z = mi.load_dict(dict(d, aperture_radius=0.0))
    assert z.har.aperture_radius == np.float32(2.0 ** -24) and any("zero aperture radius" in str(x.message) for x in w)
    # the C entry refuses a record the Python layer cannot produce
    import ctypes as C
    bad = type(a.har).from_buffer_copy(bytes(a.har)); bad.aperture_radius = 0.0
    px = np.zeros(1, np.float32); o3 = np.zeros((3, 1), np.float32); fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    assert mi.lib().har_sensor_sample_ray_aperture_host(C.byref(bad), 1, fp(px), fp(px), None, None, fp(o3), fp(o3), fp(px)) != 0 and b"aperture_radius" in mi.lib().har_last_error()
    bad = type(a.har).from_buffer_copy(bytes(a.har)); bad.projection = 3
    assert mi.lib().har_sensor_sample_ray_aperture_host(C.byref(bad), 1, fp(px), fp(px), None, None, fp(o3), fp(o3), fp(px)) != 0 and b"unsupported sensor projection" in mi.lib().har_last_error()

    # traverse: the reference's four names (thinlens.cpp:171-177), all non-differentiable; three scalar ones and to_world are updatable
    sd = T.lens_scene(mi, dict(d, sampler={"type": "independent", "sample_count": 4}))
    scene = mi.load_dict(sd)
    params = mi.traverse(scene)
    for k in ("sensor.aperture_radius", "sensor.focus_distance", "sensor.x_fov", "sensor.to_world"):
        assert k in params and params.flags(k) & mi.ParamFlags.NonDifferentiable, k
    assert "sensor.principal_point_offset_x" not in params
    assert abs(float(params["sensor.aperture_radius"][0]) - 0.2) < 1e-7 and float(params["sensor.focus_distance"][0]) == 3.5 and abs(float(params["sensor.x_fov"][0]) - 40.0) < 1e-5
    new_pose = Tr().look_at(origin=[0.3, 0.1, 3.0], target=[0.0, -0.1, 0.0], up=[0, 1, 0])
    for key, value, fresh_key, fresh_value in (("sensor.aperture_radius", torch.tensor([0.05]), "aperture_radius", float(np.float32(0.05))),
                                               ("sensor.focus_distance", torch.tensor([2.75]), "focus_distance", 2.75),
                                               ("sensor.x_fov", torch.tensor([33.0]), "fov", 33.0),
                                               ("sensor.to_world", torch.tensor(np.asarray(new_pose.matrix, np.float32).reshape(4, 4)), "to_world", new_pose)):
        params[key] = value
        params.update()
        sd["sensor"][fresh_key] = fresh_value
        want = mi.load_dict(sd).sensors()[0]
        assert bytes(scene.sensors()[0].har) == bytes(want.har), key
    with pytest.raises(RuntimeError, match="focus_distance must be positive"):
        params["sensor.focus_distance"] = torch.tensor([0.0]); params.update()
    params["sensor.aperture_radius"].requires_grad_()
    with pytest.raises(RuntimeError, match="not differentiable"):
        mi.render(scene, params, spp=1)

    mi.set_variant("scalar_rgb")
    try:
        with pytest.raises(RuntimeError, match="`thinlens` sensor is not implemented by the scalar_rgb variant"):
            mi.render(scene, spp=1)
    finally:
        mi.set_variant("hip_ad_rgb")
    # ... and so does the scalar driver's C entry
    film = np.zeros((16, 64, 4), np.float32); desc = scene.desc(); used = C.c_uint32(0)
    rc = mi.lib().har_render_scalar(C.byref(desc), C.byref(scene.sensors()[0].har), 0, 1, 4, 5, 0, 1, film.ctypes.data_as(C.c_void_p), C.byref(used))
    assert rc != 0 and b"`thinlens` sensor is not implemented by the scalar_rgb variant" in mi.lib().har_last_error()

    # a batch sensor takes thin-lens children; one is enough for the whole batch to need the aperture sample
    batch = mi.load_dict(T.lens_batch_dict(mi, "tp", 48, 16))
    assert [c.kind for c in batch.sensors()] == ["thinlens", "perspective"] and batch.needs_aperture_sample()
    assert not mi.load_dict(B.batch_dict(mi, "pp", 48, 16)).needs_aperture_sample()


def test_stream_and_host_render(mi, O):
    """the host render path -- raygen_lane, shade_lane and the splat compiled for the CPU (har_raygen_lanes_host, har_render_lanes_host) -- draws four numbers before the
    first vertex through a thin lens and two through a pinhole; its film is the film composed from oracle calls"""
    seed, spp, md = 3, 4, 4
    W, H = 16, 12
    n = W * H * spp
    jit2, state2 = B.lane_streams(O, seed, n)
    jit4, ap4, state4 = T.lane_streams4(O, seed, n)
    assert np.array_equal(jit2, jit4) and not np.array_equal(state2, state4)
    lens = mi.load_dict(T.lens_scene(mi, T.thinlens_dict(mi, 0.1, 3.9, film=T.film_dict(W, H), spp=spp), {"type": "path", "max_depth": md}))
    pin_d = B.child_dicts(mi, "p")[0]; pin_d["film"] = T.film_dict(W, H); pin_d["sampler"] = {"type": "independent", "sample_count": spp}
    pin = mi.load_dict(T.lens_scene(mi, pin_d, {"type": "path", "max_depth": md}))
    o, d, mt, pos, st = T.host_raygen(mi, lens.sensors()[0], seed, spp, n)
    assert np.array_equal(st, state4)
    p = np.arange(n) // spp
    assert np.array_equal(pos, (np.stack([p % W, p // W]).astype(np.float32) + jit4).astype(np.float32))
    lanes = T.lanes_of(mi, O, lens.sensors()[0], seed, spp)
    assert np.array_equal(lanes["ap"], ap4) and np.array_equal(o.view(np.uint32), lanes["o"].view(np.uint32)) and np.array_equal(d.view(np.uint32), lanes["d"].view(np.uint32))
    assert np.array_equal(T.host_raygen(mi, pin.sensors()[0], seed, spp, n)[4], state2)
    # a batch: four draws on every lane as soon as one child is a thin lens, two otherwise
    tp = mi.load_dict(T.lens_batch_dict(mi, "tp", 2 * W, H, spp=spp)); pp = mi.load_dict(B.batch_dict(mi, "pp", 2 * W, H, spp=spp))
    assert np.array_equal(T.host_raygen(mi, tp, seed, spp, 2 * n)[4], T.lane_streams4(O, seed, 2 * n)[2])
    assert np.array_equal(T.host_raygen(mi, pp, seed, spp, 2 * n)[4], B.lane_streams(O, seed, 2 * n)[1])
    # pass > 0 of a multi-pass render: jitter and aperture again, from the resumed state
    u, after = T.next_draws(O, seed, n, 4, state=state4)
    o2, d2, _, pos2, st2 = T.host_raygen(mi, lens.sensors()[0], seed, spp, n, resume=state4)
    assert np.array_equal(st2, after) and np.array_equal(pos2, (np.stack([p % W, p // W]).astype(np.float32) + u[:2]).astype(np.float32))
    l2 = T.lanes_of(mi, O, lens.sensors()[0], seed, spp, draws=(u, after))
    assert np.array_equal(o2.view(np.uint32), l2["o"].view(np.uint32)) and np.array_equal(d2.view(np.uint32), l2["d"].view(np.uint32))

    for scene in (lens, pin):
        sensor = scene.sensors()[0]
        osc, _ = O.scene_from_product(scene)
        want, lanes = T.composed_film(mi, O, osc, sensor, "gaussian", seed, spp, md)
        got = T.host_render(mi, scene, sensor, seed, spp, md)
        e_rgb = T.rel_l2(got[..., :3], want[..., :3]); e_w = T.rel_l2(got[..., 3], want[..., 3])
        print(sensor.kind, "host render against the composition: rgb", e_rgb, "weights", e_w, "hit", lanes["hit"].mean())
        assert lanes["hit"].mean() > 0.5 and np.linalg.norm(want[..., :3]) > 0 and e_rgb <= 1e-4 and e_w <= 2e-6
    # the lens reaches the picture: with the pinhole's rays in the thin lens's stream the film is another one
    assert T.rel_l2(T.host_render(mi, lens, lens.sensors()[0], seed, spp, md)[..., :3], T.host_render(mi, pin, pin.sensors()[0], seed, spp, md)[..., :3]) > 1e-2
