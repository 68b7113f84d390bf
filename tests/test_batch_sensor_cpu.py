"""The `batch` sensor (src/sensors/batch.cpp) without a GPU: construction and refusals, the expectations of src/sensors/tests/test_batch.py:68-106 through the
host twin har_batch_sample_ray_host, the twin against the oracle bit for bit, mi.traverse, XML == dict."""
import ctypes as C

import numpy as np
import pytest

from tests import batch_cases as B


def _perspective(mi, o, d, near_clip=1.0, film=None):
    return {"type": "perspective", "near_clip": near_clip, "far_clip": 35.0, "focus_distance": 15.0, "fov": 34, "fov_axis": "x", "shutter_open": 1.5, "shutter_close": 5,
            "to_world": mi.ScalarTransform4f().look_at(origin=o, target=[o[i] + d[i] for i in range(3)], up=[0, 1, 0]),
            "film": film or {"type": "hdrfilm", "width": 256, "height": 256}}


ORIGINS = [[1.0, 0.0, 1.5], [1.0, 4.0, 1.5]]
DIRECTIONS = [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]


def _reference_batch(mi, width=512, height=256):
    d = {"type": "batch", "shutter_open": 1.5, "shutter_close": 5, "film": {"type": "hdrfilm", "width": width, "height": height}}
    for i in range(2):
        d["sensor_%d" % i] = _perspective(mi, ORIGINS[i], DIRECTIONS[i])
    return mi.load_dict(d)


def test_constructor_and_refusals(mi):
    b = _reference_batch(mi)
    assert b.kind == "batch" and len(b.sensors()) == 2 and b.child_names == ["sensor_0", "sensor_1"]
    for c in b.sensors():                                    # batch.cpp:122-124: every child's film is the sub-film, full crop
        assert c.film().size() == (256, 256) and c.film().crop_size() == (256, 256) and (c.har.film_width, c.har.film_height) == (256, 256)
    three = mi.load_dict(B.batch_dict(mi, "pop", 96, 32))
    assert [c.kind for c in three.sensors()] == ["perspective", "orthographic", "perspective"]
    assert all(c.film().size() == (32, 32) for c in three.sensors())
    film = {"type": "hdrfilm", "width": 64, "height": 32}
    with pytest.raises(RuntimeError, match="BatchSensor: at least one child sensor must be specified!"):
        mi.load_dict({"type": "batch", "film": film})
    with pytest.raises(RuntimeError, match=r"BatchSensor: the horizontal resolution \(currently 64\) must be divisible by the number of child sensors \(3\)!"):
        mi.load_dict(B.batch_dict(mi, "ppp", 64, 32))
    with pytest.raises(RuntimeError, match="crop window on the batch sensor's film"):
        mi.load_dict(dict(B.batch_dict(mi, "pp", 64, 32), film=dict(film, crop_width=32, crop_offset_x=8)))
    with pytest.raises(RuntimeError, match="`sample_border` on the batch sensor's film"):
        mi.load_dict(dict(B.batch_dict(mi, "pp", 64, 32), film=dict(film, sample_border=True)))
    with pytest.raises(RuntimeError, match='crop window on the film of child sensor "b"'):
        mi.load_dict({"type": "batch", "film": film, "a": _perspective(mi, ORIGINS[0], DIRECTIONS[0]),
                      "b": _perspective(mi, ORIGINS[1], DIRECTIONS[1], film={"type": "hdrfilm", "width": 64, "height": 64, "crop_width": 32})})
    with pytest.raises(RuntimeError, match="nested `batch`"):
        mi.load_dict({"type": "batch", "film": film, "inner": B.batch_dict(mi, "pp", 64, 32)})
    with pytest.raises(RuntimeError, match="BatchSensor: shapes can only be specified as children if a sensor is associated with them!"):
        mi.load_dict({"type": "batch", "film": film, "a": _perspective(mi, ORIGINS[0], DIRECTIONS[0]), "shape": {"type": "rectangle"}})
    with pytest.raises(RuntimeError, match="Unreferenced property"):
        mi.load_dict(dict(B.batch_dict(mi, "pp", 64, 32), fov=40.0))
    with pytest.raises(RuntimeError, match="Unreferenced property"):
        mi.load_dict(dict(B.batch_dict(mi, "pp", 64, 32), bsdf={"type": "diffuse"}))
    # the C entry points refuse what the Python layer cannot reach
    ch = b.children_har()
    o = np.zeros((3, 1), np.float32); px = np.zeros(1, np.float32); mt = np.zeros(1, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert mi.lib().har_batch_sample_ray_host(ch, 0, 1, fp(px), fp(px), fp(o), fp(o), fp(mt)) != 0 and b"at least one child sensor" in mi.lib().har_last_error()
    ch[1].crop_width = 100
    assert mi.lib().har_batch_sample_ray_host(ch, 2, 1, fp(px), fp(px), fp(o), fp(o), fp(mt)) != 0 and b"crop window on a child's film" in mi.lib().har_last_error()


def test_scene_sensors_and_driver_refusals(mi):
    scene = mi.load_dict(B.batch_scene(mi, "pp", 64, 32))
    assert len(scene.sensors()) == 1 and scene.sensors()[0].kind == "batch"
    mi.set_variant("scalar_rgb")
    try:
        with pytest.raises(RuntimeError, match="batch sensor is not implemented by scalar_rgb"):
            mi.render(scene, spp=1)
    finally:
        mi.set_variant("hip_ad_rgb")
    with pytest.raises(RuntimeError, match="batch sensor is not implemented by render_distributed"):
        mi.render_distributed(scene, spp=1)
    with pytest.raises(RuntimeError, match="batch sensor is not implemented by render_distributed"):
        mi.render_backward_distributed(scene, np.zeros((32, 64, 3), np.float32), spp=1)


def test_reference_expectations_through_host_twin(mi):
    """src/sensors/tests/test_batch.py:68-106 (test02_sample_ray)"""
    b = _reference_batch(mi)
    o, d, _ = b.sample_ray_host(np.array([[0.25, 0.25, 0.75], [0.5, 0.5, 0.5]], np.float32))
    want = np.array([DIRECTIONS[0], DIRECTIONS[0], DIRECTIONS[1]], np.float64).T
    assert np.abs(d - want).max() <= 1e-7
    pos = np.array([[0.2, 0.1, 0.6], [0.6, 0.9, 0.2]], np.float32)
    o, d, _ = b.sample_ray_host(pos)
    near_clip = 1.0
    for lane, cam in ((0, 0), (1, 0), (2, 1)):
        m = np.asarray(b.sensors()[cam].to_world.matrix, np.float64).reshape(4, 4)
        local = np.linalg.inv(m)[:3, :3] @ d[:, lane].astype(np.float64)
        expect = np.asarray(ORIGINS[cam]) + near_clip / local[2] * d[:, lane].astype(np.float64)
        assert np.abs(o[:, lane] - expect).max() <= 1e-4


@pytest.mark.parametrize("kinds", ["po", "pop"])
def test_host_twin_against_oracle_bit_for_bit(mi, O, kinds):
    n_children = len(kinds)
    b = mi.load_dict(B.batch_dict(mi, kinds, 96, 32))
    children = [B.oracle_sensor(O, c.har) for c in b.sensors()]
    rng = np.random.default_rng(11)
    n = 20000
    px = rng.uniform(0, 1, n).astype(np.float32); py = rng.uniform(0, 1, n).astype(np.float32)
    edge = np.array([k / n_children for k in range(n_children + 1)] + [np.nextafter(np.float32(1), np.float32(0)), 0.0]
                    + [np.nextafter(np.float32(k / n_children), np.float32(0)) for k in range(1, n_children)], np.float32)
    px = np.concatenate([px, edge]); py = np.concatenate([py, np.full(edge.size, 0.37, np.float32)])
    o, d, mt = b.sample_ray_host(np.stack([px, py]))
    wo, wd, wmt, index = B.oracle_batch_rays(O, children, px, py)
    assert all((index == k).sum() > 0.2 * n for k in range(n_children))
    assert index[n + n_children] == n_children - 1 and index[n] == 0          # px = 1 lands on the last child (batch.cpp:141), px = 0 on the first
    for got, want in ((o, wo), (d, wd), (mt, wmt)):
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def test_traverse_names_and_updates(mi):
    import torch
    d = B.batch_scene(mi, "ppo", 96, 32)
    d["sensor"] = B.batch_dict(mi, "ppo", 96, 32, names=["left", "_arg_0", "ortho"])        # `_arg_<n>`: an anonymous XML child -> sensor<i> (batch.cpp:277-279)
    scene = mi.load_dict(d)
    params = mi.traverse(scene)
    for k in ("sensor.left.to_world", "sensor.left.x_fov", "sensor.sensor1.to_world", "sensor.sensor1.principal_point_offset_x", "sensor.ortho.to_world"):
        assert k in params and params.flags(k) & mi.ParamFlags.NonDifferentiable, k
    assert "sensor.ortho.x_fov" not in params and "sensor.to_world" not in params and "sensor.x_fov" not in params
    T = mi.ScalarTransform4f
    new_pose = T().look_at(origin=[0.3, 0.1, 3.0], target=[0.0, -0.1, 0.0], up=[0, 1, 0])
    params["sensor.left.to_world"] = torch.tensor(np.asarray(new_pose.matrix, np.float32).reshape(4, 4))
    params["sensor.sensor1.x_fov"] = torch.tensor([33.0])
    params.update()
    fresh = B.batch_dict(mi, "ppo", 96, 32, names=["left", "_arg_0", "ortho"])
    fresh["left"]["to_world"] = new_pose
    fresh["_arg_0"]["fov"] = 33.0
    want = mi.load_dict(fresh)
    got = scene.sensors()[0]
    for a, b in zip(got.sensors(), want.sensors()):          # the records of a freshly loaded scene, byte for byte (the untouched third child included)
        assert bytes(a.har) == bytes(b.har)
    # the rays follow the update
    pos = np.array([[0.1, 0.5, 0.9], [0.3, 0.6, 0.2]], np.float32)
    for x, y in zip(got.sample_ray_host(pos), want.sample_ray_host(pos)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    params["sensor.left.to_world"].requires_grad_()
    with pytest.raises(RuntimeError, match="not differentiable"):          # mi.render refuses the key before it touches the device
        mi.render(scene, params, spp=1)


def test_xml_equals_dict(mi):
    xml = """<sensor version="3.0.0" type="batch">
        <film type="hdrfilm"><integer name="width" value="64"/><integer name="height" value="16"/><rfilter type="box"/></film>
        <sensor type="perspective" id="first"><float name="fov" value="40"/>
            <transform name="to_world"><lookat origin="0, 0, 3.9" target="0, 0, 0" up="0, 1, 0"/></transform></sensor>
        <sensor type="orthographic"><transform name="to_world"><lookat origin="1, 0.5, 3" target="0, 0, 0" up="0, 1, 0"/></transform></sensor>
    </sensor>"""
    a = mi.load_string(xml)
    T = mi.ScalarTransform4f
    b = mi.load_dict({"type": "batch", "film": {"type": "hdrfilm", "width": 64, "height": 16, "rfilter": {"type": "box"}},
                      "first": {"type": "perspective", "fov": 40.0, "to_world": T().look_at(origin=[0, 0, 3.9], target=[0, 0, 0], up=[0, 1, 0])},
                      "second": {"type": "orthographic", "to_world": T().look_at(origin=[1, 0.5, 3], target=[0, 0, 0], up=[0, 1, 0])}})
    assert a.kind == "batch" and a.child_names == ["first", "sensor1"] and b.child_names == ["first", "second"]
    assert bytes(a.har) == bytes(b.har)
    assert [bytes(c.har) for c in a.sensors()] == [bytes(c.har) for c in b.sensors()]
