"""State that outlives a call, held to references that are not made from the object under test (tests/update_reference.py): params.update() of emitter meshes and
rectangle lights on a scene that already has a handle, device-resident updates that are followed by a failing one, DeviceGroup replicas against mi.render, and a `prb`
forward render after adjoint calls against the same render before them.  Small films and sample counts: each case takes a second or two."""
import copy

import numpy as np
import pytest

from tests.test_emitters_cpu import mesh_light_scene
from tests.test_gpu_boundary import rel_l2
from tests.test_rect_light_positions_cpu import assert_same_light, moved, rect_light_box, render_tolerance
from tests.update_reference import assert_values_kept, final_values, fresh_reference

pytestmark = pytest.mark.gpu


def _render(mi, scene, spp=16, seed=3):
    img = mi.render(scene, spp=spp, seed=seed).cpu().numpy()
    return img, scene.integrator().stats()


def _oracle(O, scene, spp=16, seed=3):
    it = scene.integrator()
    osc, sensor = O.scene_from_product(scene)
    return (osc.render_prb if it.type == "prb" else osc.render_path)(sensor, seed=seed, spp=spp, max_depth=it.max_depth, rr_depth=it.rr_depth)


def _assert_equals_fresh(mi, O, scene, d, values, tol=1e-6, oracle=True):
    """the render of `scene` == the render of a fresh load with `values` (same samples; the film's float atomics have no fixed order) == its oracle render"""
    img, st = _render(mi, scene)
    fresh = fresh_reference(d, values)
    fimg, fst = _render(mi, fresh)
    assert np.abs(fimg).max() > 0 and rel_l2(img, fimg) <= tol and st == fst, (rel_l2(img, fimg), st, fst)
    if oracle:
        ref, ost = _oracle(O, fresh)
        assert rel_l2(img, ref) <= 1e-4 and st["vertices"] == ost.vertices, rel_l2(img, ref)
    return img


# ---------------------------------------------------------------- emitter meshes (type 3)

_INTEGRATORS = {"path": {"type": "path", "max_depth": 2}, "prb": {"type": "prb", "max_depth": 5}}


@pytest.mark.parametrize("integrator", sorted(_INTEGRATORS))
@pytest.mark.parametrize("where,schedule", [("cuda", "one"), ("cpu", "one"), ("cuda", "two"), ("cuda", "two-render"), ("cpu", "two-render")])
def test_emitter_mesh_updates_equal_a_fresh_load(mi, O, integrator, where, schedule):
    """a cube light moved and scaled, a patch light deformed, on a scene that has a handle: in one update(), or over two with or without a render in between"""
    import torch
    d = mesh_light_scene(mi, 32); d["integrator"] = dict(_INTEGRATORS[integrator])
    scene = mi.load_dict(d)
    before, _ = _render(mi, scene)                          # the handle exists: the update paths of a live scene are the ones under test
    params = mi.traverse(scene)
    cube = params["cube_light.positions"].cpu().numpy().astype(np.float64); patch = params["patch_light.positions"].cpu().numpy().astype(np.float64)
    moved_cube = cube + [0.06, -0.05, 0.04]
    c = moved_cube.mean(axis=0)
    final = {"cube_light.positions": c + 1.3 * (moved_cube - c), "patch_light.positions": patch + 0.03 * np.sin(9.0 * patch[:, ::-1])}
    rounds = [final] if schedule == "one" else [{"cube_light.positions": moved_cube, "patch_light.positions": final["patch_light.positions"]},
                                                {"cube_light.positions": final["cube_light.positions"]}]
    for r, vals in enumerate(rounds):
        for k, v in vals.items():
            params[k] = torch.tensor(np.ascontiguousarray(v, np.float32), device=where)
        params.update()
        if schedule == "two-render" and r == 0:
            _render(mi, scene)
    values = final_values(params, final)
    assert_values_kept(scene, values)
    img = _assert_equals_fresh(mi, O, scene, d, values)
    assert rel_l2(img, before) > 1e-2                       # the lights did move


# ---------------------------------------------------------------- rectangle lights (types 0 and 7)

@pytest.mark.parametrize("where", ["cuda", "cpu"])
@pytest.mark.parametrize("textured", [False, True], ids=["rgb", "bitmap"])
def test_rect_light_positions_move_its_frame(mi, O, textured, where):
    """'light.positions' = T * P on a live scene == the scene loaded with to_world = T * to_world (records, render, oracle); positions that are not a parallelogram are
    refused and leave the scene as it was"""
    import torch
    d = rect_light_box(mi, textured, 32); d["integrator"] = {"type": "path", "max_depth": 2}
    scene = mi.load_dict(d)
    _render(mi, scene)
    params = mi.traverse(scene)
    P, d2 = moved(mi, d, params["light.positions"].cpu().numpy())
    params["light.positions"] = torch.tensor(P, device=where); params.update()
    fresh = mi.load_dict(d2)
    assert_same_light(scene, fresh)
    assert_values_kept(scene, {"light.positions": torch.tensor(P)})
    assert np.abs(mi.traverse(scene)["light.to_world"].cpu().numpy() - mi.traverse(fresh)["light.to_world"].cpu().numpy()).max() <= 1e-6
    img, st = _render(mi, scene); fimg, fst = _render(mi, fresh)
    assert rel_l2(img, fimg) <= render_tolerance(textured) and st == fst, rel_l2(img, fimg)
    ref, ost = _oracle(O, fresh)
    assert rel_l2(img, ref) <= 1e-4 and st["vertices"] == ost.vertices
    # not a parallelogram: refused, naming the parameter that moves a rectangle freely; the scene keeps its light
    V0 = [np.array(m["V"]) for m in scene.meshes]; E0 = copy.deepcopy(scene.emitters)
    bad = P.copy(); bad[3] += np.float32(0.05)
    params["light.positions"] = torch.tensor(bad, device=where)
    with pytest.raises(RuntimeError, match=r"'light\.to_world'"):
        params.update()
    assert all(np.array_equal(a, m["V"]) for a, m in zip(V0, scene.meshes))
    for a, b in zip(E0, scene.emitters):
        assert all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("to_world", "normal", "inv_area", "radiance"))
    assert rel_l2(_render(mi, scene)[0], img) <= 1e-6


# ---------------------------------------------------------------- a failing device-resident update after good ones

def _failure_scene(mi):
    """the Cornell box's cubes (top-level meshes A, B) and three instances of a cube group: every update here takes the device-resident path"""
    T = mi.ScalarTransform4f
    d = mi.cornell_box(); d["sensor"]["film"]["width"] = 32; d["sensor"]["film"]["height"] = 32
    d["integrator"] = {"type": "path", "max_depth": 4}
    d["grp"] = {"type": "shapegroup", "c": {"type": "cube", "bsdf": {"type": "ref", "id": "white"}}}
    for j, (x, z) in enumerate(((-0.5, 0.4), (0.0, 0.5), (0.5, 0.3))):
        d["inst%d" % j] = {"type": "instance", "shapegroup": {"type": "ref", "id": "grp"}, "to_world": T().translate([x, 0.3, z]).scale(0.1)}
    return d


@pytest.mark.parametrize("case", ["mesh-then-nonfinite-mesh", "instance-then-singular-instance", "mesh-then-singular-instance"])
def test_a_failed_update_keeps_the_good_updates_before_it(mi, O, case):
    """good CUDA update of A (a mesh) or i (an instance), then a bad value for B / j, reported one call late: the error is raised, the good update survives in the mirrors
    (one more update() later: every written key reads back, the render equals a fresh load), the failing object keeps its last valid value, and its key is looked at
    again.  Nothing renders between the bad write and the update that reports it."""
    import torch
    d = _failure_scene(mi)
    scene = mi.load_dict(d)
    _render(mi, scene, spp=4)
    params = mi.traverse(scene)
    good_key, bad_key = {"mesh-then-nonfinite-mesh": ("small-box.positions", "large-box.positions"),
                         "instance-then-singular-instance": ("inst0.to_world", "inst2.to_world"),
                         "mesh-then-singular-instance": ("small-box.positions", "inst2.to_world")}[case]
    if good_key.endswith("positions"):
        params[good_key] = params[good_key] * 1.2 + torch.tensor([0.05, 0.0, -0.04], device="cuda")
    else:
        m = params[good_key].clone(); m[:3, 3] += torch.tensor([0.1, 0.2, -0.1], device="cuda"); params[good_key] = m
    params.update()
    assert scene._h is not None
    last_valid = params[bad_key].cpu().numpy().copy()
    bad = params[bad_key].clone()
    if bad_key.endswith("positions"):
        bad[5, 1] = float("nan")
        good = params[bad_key] + torch.tensor([-0.05, 0.02, 0.03], device="cuda")
    else:
        bad[:3, :3] = 0.0
        good = params[bad_key].clone(); good[:3, 3] += torch.tensor([-0.1, 0.1, 0.05], device="cuda")
    params[bad_key] = bad; params.update()                  # enqueued: nothing has looked at the values yet
    assert scene._h is not None
    params[bad_key] = good
    with pytest.raises(RuntimeError, match="not finite" if bad_key.endswith("positions") else "singular"):
        params.update()
    assert scene._h is None
    if bad_key.endswith("positions"):                        # the failing object: its last valid value in the mirror
        assert np.array_equal(scene.meshes[scene._position_keys()[bad_key]]["V"][:, :3], last_valid)
    else:
        assert np.array_equal(scene._instance_matrix(scene._instance_keys()[bad_key]), last_valid)
    params.update()                                         # the rejected key is looked at again
    values = final_values(params, [good_key, bad_key])
    assert_values_kept(scene, values)
    # (1e-5: the good mesh's normals were regenerated on the device, a few ulps from the host's -- test_gpu_accel_update.py)
    _assert_equals_fresh(mi, O, scene, d, values, tol=1e-5, oracle=False)


# ---------------------------------------------------------------- DeviceGroup against mi.render

_GROUP_SETTINGS = {
    "hide_emitters": ({"hide_emitters": True}, {}),
    "samples_per_pass": ({"samples_per_pass": 4}, {}),
    "material_queues": ({"material_queues": True}, {}),
    "packet_tracing_off": ({"packet_tracing": False}, {}),
    "packet_tracing_on": ({"packet_tracing": True}, {}),
    "crop_window": ({}, {"crop_width": 20, "crop_height": 14, "crop_offset_x": 5, "crop_offset_y": 9}),
    "box_filter": ({}, {"rfilter": {"type": "box"}}),
    "luminance": ({}, {"pixel_format": "luminance"}),
    "prb": ({"type": "prb", "max_depth": 5}, {}),
}


def _group_scene(mi, integ=None, film=None):
    d = mi.cornell_box(); d["sensor"]["film"]["width"] = 32; d["sensor"]["film"]["height"] = 32
    d["sensor"]["film"].update(film or {})
    d["integrator"] = dict({"type": "path", "max_depth": 5}, **(integ or {}))
    return mi.load_dict(d)


@pytest.mark.parametrize("devices", [[0], [0, 0, 0]], ids=["one", "three-on-one"])
@pytest.mark.parametrize("setting", sorted(_GROUP_SETTINGS))
def test_device_group_honours_the_integrator_and_film_settings(mi, setting, devices):
    scene = _group_scene(mi, *_GROUP_SETTINGS[setting])
    want, st = _render(mi, scene, spp=16, seed=4)
    g = mi.DeviceGroup(scene, devices=devices)
    got = g.render(spp=16, seed=4).cpu().numpy()
    assert got.shape == want.shape and rel_l2(got, want) <= 1e-6 and g.stats() == st, (rel_l2(got, want) if got.shape == want.shape else got.shape, g.stats(), st)


@pytest.mark.parametrize("devices", [[0], [0, 0, 0]], ids=["one", "three-on-one"])
def test_device_group_adjoint_without_replay_cache(mi, devices):
    """replay_cache = False on the replicas too: the group's adjoint == the single device's (the tolerance of test_gpu_multi's adjoint test); a forward render after it
    == mi.render"""
    import torch
    d = mi.textured_cornell_box(res=32, tex_res=16, spp=16)
    d["integrator"]["replay_cache"] = False; d["integrator"]["emitter_gradients"] = True
    scene = mi.load_dict(d)
    torch.manual_seed(3)
    grad_in = torch.rand((32, 32, 3), device="cuda") / (32 * 32 * 3)
    want = scene.integrator().render_backward(scene, None, grad_in, seed=11, spp=16)
    g = mi.DeviceGroup(scene, devices=devices)
    got = g.render_backward(grad_in, seed=11, spp=16)
    assert set(got) == set(want)
    for k in want:
        a, b = got[k].cpu().numpy(), want[k].cpu().numpy()
        assert np.isfinite(a).all() and np.abs(b).max() > 0 and rel_l2(a, b) < 1e-4, (k, rel_l2(a, b))
    img, st = _render(mi, scene, spp=16, seed=2)
    assert rel_l2(g.render(spp=16, seed=2).cpu().numpy(), img) < 1e-6 and g.stats() == st


def test_device_group_refuses_an_rgba_film(mi):
    scene = _group_scene(mi, film={"pixel_format": "rgba"})
    g = mi.DeviceGroup(scene, devices=[0])
    with pytest.raises(RuntimeError, match="rgba"):         # (the group's film has no alpha channel: refused, not rendered without it)
        g.render(spp=4, seed=1)


# ---------------------------------------------------------------- a `prb` forward render does not depend on call history

def test_prb_forward_render_is_the_same_after_adjoint_calls(mi):
    """area light with a bitmap radiance, bitmap albedo, rough BSDF: mi.render before and after render_backward (emitter, BSDF-parameter and light-texel gradients on) and
    render_forward -- every counter equal, the image equal"""
    import torch
    from tests.test_textured_area_light_cpu import _bitmap, lit_box
    d = lit_box(mi, _bitmap(2), 32)
    d["integrator"] = {"type": "prb", "max_depth": 5, "emitter_gradients": True, "bsdf_parameter_gradients": True, "light_texel_gradients": True}
    d["small-box"]["bsdf"] = {"type": "roughconductor", "alpha": 0.3}
    d["floor"]["bsdf"] = {"type": "diffuse", "reflectance": {"type": "bitmap", "data": _bitmap(5, 8, 8) / 40.0, "raw": True}}
    scene = mi.load_dict(d)
    integ = scene.integrator()
    i1, s1 = _render(mi, scene, spp=16, seed=2)
    grads = integ.render_backward(scene, None, np.ones((32, 32, 3), np.float32), seed=5, spp=8)
    assert any(float(g.abs().max()) > 0 for k, g in grads.items() if "emitter" in k)
    integ.render_forward(scene, None, seed=6, spp=8, tangents={"red.reflectance.value": torch.ones(3, device="cuda")})
    i2, s2 = _render(mi, scene, spp=16, seed=2)
    assert s2 == s1 and rel_l2(i2, i1) <= 1e-6, (s1, s2, rel_l2(i2, i1))
