"""The `projector` emitter (src/emitters/projector.cpp) without a GPU: Projector::sample_direction through the host per-call entry against an independent float64
restatement, the geometric facts of the source's comments, the host twin's render against the oracle's render of the directional twin, and the Python interface
(dict == XML, traverse names and flags, update == fresh load, every refusal by name, the C ABI's record checks)."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

from tests import blend_cases as B
from tests import projector_cases as P


N_PER_CONFIG = 2500          # 8 configurations: 20 000 points


@pytest.fixture(scope="module")
def per_call(mi):
    """(configuration, points, host entry's result, float64 expectation) of every configuration -- computed once"""
    out = {}
    for name, cfg in P.configs(mi).items():
        pts = P.points(name, cfg, mi, N_PER_CONFIG)
        out[name] = (cfg, pts, P.host_sample_direction(mi, P.config_scene(mi, cfg), 0, pts), P.expected(cfg, mi, pts))
    return out


def test_sample_direction_against_float64(per_call):
    """d, dist, p, n, uv at rtol 3e-6 / atol 3e-7 (the sensor bar), spec at 2e-5 (the mixed-value bar); active / pdf equal on every lane but the `unsure` ones (uv within
    4 ulp of the unit square's border, |z| within 4 ulp of 0, a nearest lookup on a texel boundary), which are at most 0.5 % of the 20 000"""
    total = 0; left_out = 0; lit = 0
    for name, (cfg, pts, got, exp) in per_call.items():
        n = pts.shape[1]; total += n
        keep = ~exp["unsure"]; left_out += int((~keep).sum())
        assert np.array_equal(got["pdf"][keep], exp["pdf"][keep].astype(np.float32)), name
        act = keep & exp["active"]; lit += int(act.sum())
        assert act.sum() > 0.3 * n, name
        # the geometric part does not depend on the frustum: every lane with a finite distance
        geo = keep & (exp["dist"] > 0)
        for k in ("d", "dist", "p", "n"):
            assert np.allclose(got[k][..., geo], exp[k][..., geo], rtol=3e-6, atol=3e-7), (name, k)
        assert np.allclose(got["uv"][:, act], exp["uv"][:, act], rtol=3e-6, atol=3e-7), name
        err = np.abs(got["spec"][:, act] - exp["spec"][:, act]) / np.maximum(np.abs(exp["spec"][:, act]), 1e-30)
        print("%s: %d lanes lit, %d left out, spec max rel err %.3g" % (name, act.sum(), (~keep).sum(), err.max()))
        assert err.max() <= 2e-5, (name, err.max())
        assert np.all(got["spec"][:, keep & ~exp["active"]] == 0), name
        assert np.isfinite(got["spec"]).all(), name
    assert total == 20000 and left_out <= 0.005 * total, (total, left_out)
    print("lanes lit %d of %d, left out %d" % (lit, total, left_out))


def test_special_lanes_are_covered(per_call):
    """the inputs hold what the issue lists: lanes behind the projector and at z = 0 (inactive), lanes on the axis (uv = 1/2), lanes at every border"""
    cfg, pts, got, exp = per_call["bilinear53_mirror_larger"]          # the identity transform: local == world
    assert (pts[2] < 0).sum() >= 10 and (pts[2] == 0).sum() >= 1
    assert np.all(got["pdf"][pts[2] <= 0] == 0) and np.all(got["spec"][:, pts[2] <= 0] == 0)
    axis = (pts[0] == 0) & (pts[1] == 0) & (pts[2] > 0)
    assert axis.sum() >= 4 and np.all(got["uv"][:, axis] == 0.5) and np.all(got["pdf"][axis] == 1)
    assert sum(int(e[3]["unsure"].sum()) for e in per_call.values()) >= 60          # the lanes at the borders and at z = 0 exist


def test_geometric_facts(mi):
    """projector.cpp:234-239: a point on the axis at z = 1 receives spec * cos = pi * scale * irradiance, and dist^2 cos^3 == z^2 cos"""
    cfg = P.configs(mi)["constant_x"]
    s = float(np.float32(cfg[0]["scale"])); c = np.asarray(cfg[0]["irradiance"]["value"], np.float32)
    M = P.matrix64(P.transforms(mi)["rotated"])
    p = (M @ np.array([0, 0, 1, 1.0]))[:3].astype(np.float32).reshape(3, 1)
    got = P.host_sample_direction(mi, P.config_scene(mi, cfg), 0, p)
    cos = -float((got["n"][:, 0] * got["d"][:, 0]).sum())
    assert np.allclose(got["spec"][:, 0] * cos, np.pi * s * c, rtol=2e-5)
    pts = P.points("constant_x", cfg, mi, 2000); got = P.host_sample_direction(mi, P.config_scene(mi, cfg), 0, pts); exp = P.expected(cfg, mi, pts)
    a = exp["active"] & ~exp["unsure"]
    cos = -(got["n"].astype(np.float64) * got["d"]).sum(axis=0)[a]
    z = (np.linalg.inv(M) @ np.concatenate([pts.astype(np.float64), np.ones((1, pts.shape[1]))]))[2][a]
    assert np.allclose(got["dist"][a].astype(np.float64) ** 2 * cos ** 3, z ** 2 * cos, rtol=2e-5)


def test_placed_projector_at_small_distances(mi):
    """The translated projector at z in [1e-3, 1], which the 20 000 points leave to z >= 1.  The local point is R^-1 p + t' accumulated in float32 over four terms: its
    components carry the forward error bound of that sum, delta_k = 4 * 2^-24 * (sum_j |R^-1_kj| |p_j| + |t'_k|) -- an ABSOLUTE error of the size of the world
    coordinates' ulp.  uv = m * x / z + 1/2 and spec ~ 1 / z^2 inherit it as |m| (delta_x + |x / z| delta_z) / z and 2 delta_z / z on top of their bars (3e-6 / 3e-7
    and 2e-5); lanes whose uv lies within that of a border are left out of the active comparison (at most 0.5 %)."""
    cfg0 = P.configs(mi)["constant_focal"]
    cfg = (cfg0[0], cfg0[1], cfg0[2], (1e-3, 1.0))
    pts = P.points("small", cfg, mi, 4000, seed=9)[:, 80:]          # (the random lanes: the special ones are the other test's)
    got = P.host_sample_direction(mi, P.config_scene(mi, cfg), 0, pts); exp = P.expected(cfg, mi, pts)
    T = P.transforms(mi)["placed"]; Minv = P.matrix64(T.inverse())
    p = pts.astype(np.float64)
    delta = 4 * 2.0 ** -24 * (np.abs(Minv[:3, :3]) @ np.abs(p) + np.abs(Minv[:3, 3:4]))
    local = (Minv @ np.concatenate([p, np.ones((1, p.shape[1]))]))[:3]
    aspect = 1.0; cot = 1.0 / np.tan(0.5 * np.radians(float(np.float32(P.x_fov_of(cfg[0], aspect)))))
    m = np.array([0.5 * cot, 0.5 * aspect * cot])[:, None]
    z = local[2]
    tol_uv = 3e-7 + 3e-6 * np.abs(exp["uv"]) + 1.01 * m * (delta[:2] + np.abs(local[:2] / z) * delta[2]) / z
    near = (np.minimum(np.abs(exp["uv"]), np.abs(exp["uv"] - 1)) <= tol_uv).any(axis=0)
    keep = ~near
    print("small z: %d of %d lanes left out, uv tolerance up to %.3g" % (near.sum(), near.size, tol_uv.max()))
    assert near.sum() <= 0.005 * near.size and z.min() < 2e-3
    assert np.array_equal(got["pdf"][keep], exp["pdf"][keep].astype(np.float32))
    act = keep & exp["active"]
    assert act.sum() > 1000
    assert np.all(np.abs(got["uv"][:, act] - exp["uv"][:, act]) <= tol_uv[:, act])
    rel = np.abs(got["spec"][:, act] - exp["spec"][:, act]) / np.abs(exp["spec"][:, act])
    bound = 2e-5 + 2.02 * delta[2, act] / z[act]
    print("small z: spec rel err up to %.3g, bound up to %.3g" % (rel.max(), bound.max()))
    assert np.all(rel <= bound[None, :])
    for k in ("p", "n"):
        assert np.allclose(got[k], exp[k], rtol=3e-6, atol=3e-7), k


def test_active_mask(mi):
    cfg = P.configs(mi)["bilinear53_to_uv_y"]
    pts = P.points("m", cfg, mi, 300)
    mask = (np.arange(300) % 3 != 0).astype(np.uint8)
    full = P.host_sample_direction(mi, P.config_scene(mi, cfg), 0, pts); part = P.host_sample_direction(mi, P.config_scene(mi, cfg), 0, pts, mask)
    for k in full:
        assert np.array_equal(part[k][..., mask == 1], full[k][..., mask == 1]) and np.all(part[k][..., mask == 0] == 0), k


# ---- the directional twin on the host

@pytest.fixture(scope="module")
def twin(mi, O):
    s, c = 1.7, (0.9, 0.5, 0.3)
    pj, dr = P.twin_lights(mi, s, c)
    oracle, sensor = O.scene_from_product(mi.load_dict(P.twin_scene(mi, dr)))
    return dict(s=s, c=c, projector=mi.load_dict(P.twin_scene(mi, pj)), oracle=oracle, sensor=sensor)


def test_twin_walls_are_dark_in_the_oracle(twin):
    """at max_depth 2 only the directly lit floor shows: every pixel the floor's footprint does not reach is exactly zero (the walls get nothing from the directional
    light: cos = 0 exactly), and the floor is lit"""
    film, _ = twin["oracle"].render_path(twin["sensor"], seed=0, spp=4, max_depth=2, rr_depth=5, raw=True)
    assert (film[:, :, :3].sum(axis=2) == 0).sum() > 20 and film[:, :, :3].max() > 0
    # a wall pixel: the leftmost and rightmost columns of the top rows see only walls
    assert np.all(film[:3, :2, :3] == 0) and np.all(film[:3, -2:, :3] == 0)


@pytest.mark.parametrize("max_depth", [2, 4, 8])
def test_twin_host_render_equals_oracle(mi, twin, max_depth):
    film, st = B.host_render_stats(mi, twin["projector"], 0, 4, max_depth, 5)
    ref, rst = twin["oracle"].render_path(twin["sensor"], seed=0, spp=4, max_depth=max_depth, rr_depth=5, raw=True)
    err = P.rel_l2(film, ref)
    print("twin host render, max_depth %d: rel L2 %.3g" % (max_depth, err))
    assert err <= 1e-4
    assert (st.paths, st.vertices) == (rst.paths, rst.vertices)


# ---- the textured render, lane by lane, against the composition from oracle entries

@pytest.mark.parametrize("which", list(P.PLANE_MAPS))
def test_textured_plane_host_film_equals_oracle_composition(mi, O, which):
    """the host twin's 16 x 12 x 4 film of the tilted plane under the textured projector against orc_sensor_sample_ray + integrator_sample under a unit point light
    at the apex, times pi s T(uv) d^2 / (z^2 cos) in float64, + orc_film_put: 1e-4, weights 2e-6"""
    comp = P.composed_plane(mi, O, which, 3, 4, res=(16, 12))
    pj, _, _ = P.plane_lights(mi, which)
    film, _ = B.host_render_stats(mi, mi.load_dict(P.plane_scene(mi, pj, res=(16, 12), spp=4)), 3, 4, 2, 5)
    assert comp["lit"].sum() > 100 and (comp["hit"] & ~comp["lit"]).sum() > 100 and comp["unsure"].sum() == 0          # part of the plane is outside the frustum
    e_rgb = P.rel_l2(film[:, :, :3], comp["film"][:, :, :3]); e_w = P.rel_l2(film[:, :, 3], comp["film"][:, :, 3])
    print("plane %s host film / composition: rgb %.3g, weights %.3g" % (which, e_rgb, e_w))
    assert comp["film"][:, :, :3].max() > 0 and e_rgb <= 1e-4 and e_w <= 2e-6


# ---- the Python interface

def _xml(body):
    return '<scene version="3.0.0"><shape type="rectangle"/>' + body + '</scene>'


def test_dict_equals_xml(mi):
    d = {"type": "scene", "r": {"type": "rectangle"},
         "light": {"type": "projector", "irradiance": {"type": "rgb", "value": [0.2, 0.4, 0.6]}, "scale": 2.5, "fov": 35.0, "fov_axis": "y", "sampling_weight": 0.5,
                   "to_world": mi.ScalarTransform4f().look_at(origin=[1, 1, 1], target=[1, 2, 1], up=[0, 0, 1])}}
    a = mi.load_dict(d)
    b = mi.load_string(_xml('<emitter type="projector"><rgb name="irradiance" value="0.2, 0.4, 0.6"/><float name="scale" value="2.5"/><float name="fov" value="35"/>'
                            '<string name="fov_axis" value="y"/><float name="sampling_weight" value="0.5"/>'
                            '<transform name="to_world"><lookat origin="1, 1, 1" target="1, 2, 1" up="0, 0, 1"/></transform></emitter>'))
    ea, eb = a.emitters[0], b.emitters[0]
    assert ea["type"] == eb["type"] == 8
    for k in ("radiance", "to_world", "to_local", "normal", "sampling_weight"):
        assert np.allclose(np.asarray(ea[k], np.float32), np.asarray(eb[k], np.float32), rtol=0, atol=0), k


def test_bitmap_from_file_in_xml(mi):
    data = P.map53()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "pattern.exr")
        mi.Bitmap(data).write(path)
        b = mi.load_string(_xml('<emitter type="projector"><texture type="bitmap" name="irradiance"><string name="filename" value="%s"/><boolean name="raw" value="true"/>'
                                '</texture><float name="fov" value="50"/></emitter>' % path))
    a = mi.load_dict({"type": "scene", "r": {"type": "rectangle"}, "light": {"type": "projector", "irradiance": {"type": "bitmap", "data": data, "raw": True}, "fov": 50.0}})
    assert np.array_equal(a.textures[a.emitters[0]["radiance_texture"]], b.textures[b.emitters[0]["radiance_texture"]])
    assert a.emitters[0]["normal"] == b.emitters[0]["normal"]


def test_traverse_names_and_flags(mi):
    F = mi.ParamFlags
    for irr, names in (({"type": "rgb", "value": 1.0}, ["light.irradiance.value"]), ({"type": "bitmap", "data": P.map53(), "raw": True}, ["light.irradiance.data", "light.irradiance.to_uv"])):
        sc = mi.load_dict({"type": "scene", "r": {"type": "rectangle"}, "light": {"type": "projector", "irradiance": irr}})
        p = mi.traverse(sc)
        mine = sorted(k for k in p.keys() if k.startswith("light."))
        assert mine == sorted(names + ["light.scale", "light.to_world", "light.sampling_weight"])
        assert p.flags("light.scale") == F.Differentiable and p.flags(names[0]) == F.Differentiable
        assert p.flags("light.to_world") == F.NonDifferentiable
        assert tuple(p["light.to_world"].shape) == (4, 4) and tuple(p["light.scale"].shape) == (1,)
    sc = mi.load_dict({"type": "scene", "r": {"type": "rectangle"}, "light": {"type": "projector", "irradiance": {"type": "bitmap", "data": P.map44(1), "raw": True}}})
    assert tuple(mi.traverse(sc)["light.irradiance.data"].shape) == (4, 4, 1)


def _records(scene):
    return [{k: (np.asarray(v, np.float32).tolist() if k in ("radiance", "to_world", "to_local", "normal") else v) for k, v in e.items() if k != "light"} for e in scene.emitters]


def test_update_equals_fresh_load(mi):
    import torch
    T = mi.ScalarTransform4f
    mk = lambda data, scale, tw: {"type": "scene", "r": {"type": "rectangle"},
                                  "light": {"type": "projector", "irradiance": {"type": "bitmap", "data": data, "raw": True}, "scale": scale, "fov": 50.0, "to_world": tw}}
    tw2 = T().translate([0.1, 0.2, 0.3]).rotate([0, 1, 0], 25.0)
    sc = mi.load_dict(mk(P.map53(), 1.0, T()))
    p = mi.traverse(sc)
    new = (P.map53() * 0.5 + 0.1).astype(np.float32)
    p["light.irradiance.data"] = torch.as_tensor(new); p["light.scale"] = torch.tensor([3.25]); p["light.to_world"] = torch.as_tensor(np.asarray(tw2.matrix, np.float32).reshape(4, 4))
    p.update()
    fresh = mi.load_dict(mk(new, 3.25, tw2))
    assert np.array_equal(sc.textures[0], fresh.textures[0])
    a, b = _records(sc)[0], _records(fresh)[0]
    assert a["normal"] == b["normal"] and np.allclose(a["to_world"], b["to_world"], atol=1e-7) and np.allclose(a["to_local"], b["to_local"], atol=1e-6)
    pts = P.points("u", P.configs(mi)["bilinear53_mirror_larger"], mi, 500)
    ga, gb = P.host_sample_direction(mi, sc, 0, pts), P.host_sample_direction(mi, fresh, 0, pts)
    for k in ga:
        assert np.allclose(ga[k], gb[k], rtol=1e-5, atol=1e-6), k
    with pytest.raises(RuntimeError, match="projector: the irradiance bitmap must keep its shape"):
        p["light.irradiance.data"] = torch.zeros((4, 4, 3)); p.update()


def test_refusals_by_name(mi):
    base = lambda light: {"type": "scene", "r": {"type": "rectangle"}, "light": dict({"type": "projector"}, **light)}
    with pytest.raises(RuntimeError, match="Unreferenced property \"intensity\" in plugin of type \"projector\""):
        mi.load_dict(base({"intensity": 2.0}))
    with pytest.raises(RuntimeError, match="Unreferenced property \"child\" in plugin of type \"projector\""):
        mi.load_dict(base({"child": {"type": "diffuse"}}))
    with pytest.raises(RuntimeError, match="not found"):
        mi.load_dict(base({"irradiance": {"type": "no_such_texture"}}))
    with pytest.raises(RuntimeError, match="projector: a `mesh_attribute` as property \"irradiance\" is not implemented"):
        mi.load_dict(base({"irradiance": {"type": "mesh_attribute", "name": "vertex_color"}}))
    with pytest.raises(RuntimeError, match="Please specify either a focal length"):
        mi.load_dict(base({"fov": 30.0, "focal_length": "50mm"}))
    with pytest.raises(RuntimeError, match="fov_axis"):
        mi.load_dict(base({"fov": 30.0, "fov_axis": "sideways"}))
    with pytest.raises(RuntimeError, match="projector: to_world is singular"):
        mi.load_dict(base({"to_world": mi.ScalarTransform4f().scale([1.0, 0.0, 1.0])}))
    with pytest.raises(RuntimeError, match="is not a surface emitter"):
        mi.load_dict({"type": "scene", "r": {"type": "rectangle", "emitter": {"type": "projector"}}})
    assert mi.core._plugin_kind("projector") == "emitter"


def test_c_abi_record_checks(mi):
    """har_scene_create's checks behind the host entries: a texture index out of range, a `mesh_attribute` record as irradiance, a singular to_world"""
    from mitsuba3_amd import _capi
    sc = mi.load_dict({"type": "scene", "r": {"type": "rectangle", "bsdf": {"type": "diffuse"}},
                       "light": {"type": "projector", "irradiance": {"type": "bitmap", "data": P.map53(), "raw": True}}})
    out = [np.zeros((3, 1), np.float32) for _ in range(7)]
    call = lambda d: mi.lib().har_emitter_sample_direction_host(C.byref(d), 0, 1, P._fp(np.ones((3, 1), np.float32)), None, None, *[P._fp(o) for o in out])
    err = lambda: (mi.lib().har_last_error() or b"").decode()
    d = sc.desc(); assert call(d) == 0
    d = sc.desc(); d.emitters[0].radiance_texture = 7
    assert call(d) != 0 and "projector: `irradiance` references a bitmap that does not exist" in err()
    d = sc.desc(); d.textures[0].mode = 8; d.textures[0].width = 1; d.textures[0].height = 4; d.textures[0].reserved = 0          # HAR_TEX_MESH_ATTRIBUTE over mesh 0's four vertices
    assert call(d) != 0 and "mesh_attribute" in err()
    d = sc.desc()
    for k in (0, 1, 2):
        d.emitters[0].to_world[k] = 0.0
    assert call(d) != 0 and "projector: to_world is singular" in err()
    d = sc.desc(); d.emitters[0].type = 4
    assert call(d) != 0 and "implemented for a `projector`" in err()


def test_device_group_is_refused_by_name(mi):
    """har_multi_create names the projector before it looks for devices"""
    sc = mi.load_dict(P.twin_scene(mi, P.twin_lights(mi, 1.0, (1, 1, 1))[0]))
    d = sc.desc(); dev = (C.c_int * 1)(0); h = C.c_void_p()
    fn = mi.lib().har_multi_create
    rc = fn(C.byref(d), 0, 4, 5, 0, dev, 1, C.byref(h))
    assert rc != 0 and "projector: a DeviceGroup" in (mi.lib().har_last_error() or b"").decode()
