"""The `aov` integrator (src/integrators/aov.cpp) without a GPU: construction (re-hosting src/integrators/tests/test_aov.py::test01 in this project's words), the
host twin har_aov_sample_host against the oracle, and the closed-form rectangle of test04."""
import numpy as np
import pytest

from tests import aov_cases as A


def test_construction_and_names(mi):
    one = mi.load_dict({"type": "aov", "aovs": "dd.y:depth"})
    assert one.aov_names() == ["dd.y.T"]
    many = mi.load_dict({"type": "aov", "aovs": "dd.y:depth,nn:sh_normal,ab:albedo", "img": {"type": "path"}, "second": {"type": "prb", "max_depth": 3}})
    assert many.aov_names() == ["img.R", "img.G", "img.B", "img.A", "second.R", "second.G", "second.B", "second.A",
                                "dd.y.T", "nn.X", "nn.Y", "nn.Z", "ab.R", "ab.G", "ab.B"]
    assert [c.type for c in many.children] == ["path", "prb"] and many.children[1].max_depth == 3
    everything = mi.load_dict({"type": "aov", "aovs": A.ALL_SPEC})
    assert len(everything.aov_names()) == 23 and everything.channels == 23      # 3 + 1 + 3 + 2 + 3 + 3 + 3 + 3 + 1 + 1
    C = mi.core.C; n = C.c_uint32()
    mi.core.check(mi.lib().har_aov_channel_count(10, (C.c_uint32 * 10)(*range(10)), C.byref(n)))
    assert n.value == 23
    assert mi.lib().har_aov_channel_count(1, (C.c_uint32 * 1)(10), C.byref(n)) != 0
    with pytest.raises(RuntimeError, match="aovs"):
        mi.load_dict({"type": "aov"})
    with pytest.raises(RuntimeError, match='Invalid AOV type "bogus"'):
        mi.load_dict({"type": "aov", "aovs": "x:bogus"})
    for t in ("duv_dx", "duv_dy"):
        with pytest.raises(RuntimeError, match="not implemented by hip_ad_rgb"):
            mi.load_dict({"type": "aov", "aovs": "x:" + t})
    with pytest.raises(RuntimeError, match="SamplingIntegrator"):
        mi.load_dict({"type": "aov", "aovs": "x:depth", "child": {"type": "diffuse"}})
    with pytest.raises(RuntimeError, match="nested `aov`"):
        mi.load_dict({"type": "aov", "aovs": "x:depth", "child": {"type": "aov", "aovs": "y:depth"}})
    with pytest.raises(RuntimeError, match="Unreferenced property"):
        mi.load_dict({"type": "aov", "aovs": "x:depth", "max_depth": 3})
    with pytest.raises(RuntimeError, match="not implemented by hip_ad_rgb"):
        mi.load_dict({"type": "aov", "aovs": "x:depth", "samples_per_pass": 2})


def test_xml_equals_dict(mi):
    xml = """<integrator version="3.0.0" type="aov"><string name="aovs" value="dd.y:depth,nn:sh_normal,ab:albedo"/>
               <integrator type="path" name="img"><integer name="max_depth" value="5"/></integrator><integrator type="prb" name="second"/></integrator>"""
    a = mi.load_string(xml)
    b = mi.load_dict({"type": "aov", "aovs": "dd.y:depth,nn:sh_normal,ab:albedo", "img": {"type": "path", "max_depth": 5}, "second": {"type": "prb"}})
    assert a.type == "aov" and a.aov_names() == b.aov_names() and a.aov_types == b.aov_types
    assert [(c.type, c.max_depth, c.rr_depth) for c in a.children] == [(c.type, c.max_depth, c.rr_depth) for c in b.children] == [("path", 5, 5), ("prb", 6, 5)]
    d = A.feature_scene(mi, integrator={"type": "aov", "aovs": "d:depth", "img": {"type": "path"}})
    assert mi.load_dict(d).integrator().aov_names() == ["img.R", "img.G", "img.B", "img.A", "d.T"]


def test_refusals_without_a_gpu(mi):
    aov = mi.load_dict({"type": "aov", "aovs": "d:depth", "img": {"type": "prb"}})
    scene = mi.load_dict(A.feature_scene(mi))
    with pytest.raises(RuntimeError, match="`aov` integrator is not implemented"):
        aov.render_forward(scene)
    with pytest.raises(RuntimeError, match="`aov` integrator is not implemented"):
        mi.DeviceGroup(scene, devices=(0,), integrator=aov)
    with pytest.raises(RuntimeError, match="`aov` integrator is not implemented"):
        mi.render_distributed(scene, integrator=aov)
    mi.set_variant("scalar_rgb")
    try:
        with pytest.raises(RuntimeError, match="`aov` integrator is not implemented by the scalar_rgb variant"):
            mi.render(scene, integrator=aov, spp=1)
    finally:
        mi.set_variant("hip_ad_rgb")


def check_against_oracle(got, want, hit, kind, types):
    """the comparison of har_aov_sample(_host) with the oracle composition; returns the largest deviations for the log"""
    sl, _ = A.channel_slices(types)
    assert (got[:, ~hit] == 0).all()                                                  # missed and masked lanes: exactly 0 in every channel (aov.cpp:186)
    for name in ("prim_index", "shape_index"):
        assert np.array_equal(got[sl[name]], want[sl[name]].astype(np.float32)), name
    worst = {}
    # rtol / atol: what tests/test_gpu_boundary_masks.py holds Scene.ray_intersect's interaction to the same oracle rows at
    for name in ("depth", "position", "uv", "geo_normal", "sh_normal", "dp_du", "dp_dv"):
        g = got[sl[name]].astype(np.float64); w = want[sl[name]]
        worst[name] = float(np.max(np.abs(g - w) - 3e-6 * np.abs(w)))
        assert np.allclose(g, w, rtol=3e-6, atol=3e-7), (name, worst[name])
    # albedo.  Textured / constant colours: bilinear interpolation of float32 texels against a float64 lookup, the bound tests/test_bsdfs_cpu.py uses for that
    # comparison (rtol 2e-5, atol 2e-6).  Base-class eval * pi: oracle and product evaluate the same float32 formulas -- microfacet terms differ by a few ulp, 2e-5.
    g = got[sl["albedo"]].astype(np.float64); w = want[sl["albedo"]]
    for k in (1, 2):
        m = kind == k
        assert m.any(), k
        assert np.allclose(g[:, m], w[:, m], rtol=2e-5, atol=2e-6), (k, float(np.abs(g[:, m] - w[:, m]).max()))
    assert (g[:, kind == 0] == 0).all()
    return worst


def test_host_twin_against_oracle(mi, O):
    scene = mi.load_dict(A.feature_scene(mi))
    osc, _ = O.scene_from_product(scene)
    aov = mi.load_dict({"type": "aov", "aovs": A.ALL_SPEC})
    o, d, maxt, active = A.feature_rays()
    assert o.shape[1] >= 20000
    got = aov.sample_host(scene, o, d, maxt, active)
    want, hit, kind = A.oracle_aovs(O, scene, osc, A.ALL_TYPES, o, d, maxt, active)
    assert 0.2 < hit.mean() < 0.9 and (~active).sum() > 1000                          # a share of the rays miss, a share is masked
    # the scene exercises what it claims: every BSDF model is hit, the `twosided` pair from both sides, instances, the textured floor, the smooth mesh
    shapes = got[A.channel_slices(A.ALL_TYPES)[0]["shape_index"]][0][hit].astype(int)
    keys = [m["key"] for m in scene.meshes[:scene.top_mesh_count]]
    for name in ("floor", "pair", "single", "glass", "metal", "rough", "cap", "lamp"):
        assert (shapes == keys.index(name) + 1).sum() > 20, name
    for k in range(2):
        assert (shapes == scene.top_mesh_count + k + 1).sum() > 20
    pair = shapes == keys.index("pair") + 1
    alb = got[0:3][:, hit][:, pair]
    assert (np.abs(alb[0] - 0.7) < 1e-6).sum() > 10 and (np.abs(alb[2] - 0.8) < 1e-6).sum() > 10      # front: diffuse red, back: plastic blue
    print(check_against_oracle(got, want, hit, kind, A.ALL_TYPES))
    # the unmasked call agrees on the lanes both trace
    got2 = aov.sample_host(scene, o, d, maxt)
    assert np.array_equal(got2[:, active], got[:, active])


def test_closed_form_rectangle(mi, O):
    """test04: a rectangle scaled (10, 10, 1) at z = -1 with albedo 0.4, rays along -z"""
    scene = mi.load_dict({"type": "scene", "r": {"type": "rectangle", "to_world": mi.ScalarTransform4f().translate([0, 0, -1]).scale([10, 10, 1]),
                                                 "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": 0.4}}}})
    aov = mi.load_dict({"type": "aov", "aovs": "nn:sh_normal,gn:geo_normal,ab:albedo,pp:position,dd:depth"})
    n = 64
    rng = np.random.default_rng(1)
    o = np.zeros((3, n), np.float32); o[0:2] = rng.uniform(-9, 9, (2, n)); o[2] = rng.uniform(0.5, 7.0, n)
    d = np.zeros((3, n), np.float32); d[2] = -1.0
    out = aov.sample_host(scene, o, d, np.full(n, np.inf, np.float32)).astype(np.float64)
    assert np.abs(out[0:3] - np.array([[0], [0], [1.0]])).max() <= 1e-6 and np.abs(out[3:6] - np.array([[0], [0], [1.0]])).max() <= 1e-6
    assert np.abs(out[6:9] - 0.4).max() <= 1e-6
    assert np.abs(out[11] + 1.0).max() <= 1e-6
    # x, y of the hit point are not in test04's list.  They are interpolated from vertex coordinates of +-10 (three products, two sums, each rounded to half an ulp of a
    # value below 16, 2^-20): 5 * 2^-21 = 2.4e-6 is what float32 allows; 1e-6 is below the spacing of the numbers compared
    assert np.abs(out[9:11] - o[0:2]).max() <= 5 * 2.0 ** -21
    assert np.abs(out[12] - (o[2].astype(np.float64) + 1.0)).max() <= 1e-6
