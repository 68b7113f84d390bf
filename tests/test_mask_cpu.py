"""`mask` on the CPU, through the library's host entries (har_bsdf_eval_pdf_host / har_bsdf_sample_host / har_render_lanes_stats_host / har_aov_sample_host run the HAR_HD
code the kernels run): the composition against the oracle's answers for the nested BSDF, host renders against the oracle through identical geometry, partial opacity
statistically, the aov channels, and the loader."""
import numpy as np
import pytest

from tests import blend_cases as B
from tests import mask_cases as M

ALL = M.ALL
LEAF = dict(rtol=2e-6, atol=1e-9)          # the bars of tests/test_blendbsdf_cpu.py for the same situation: the leaf models against the oracle, pdfs and un-mixed values
MIXED = dict(rtol=2e-5, atol=1e-7)         # ... and composed values: value * o


# ------------------------------------------------------------------------------------------------ 1. the record

def test_components_and_flags(mi):
    F = mi.BSDFFlags
    null = F.Null | F.FrontSide | F.BackSide
    m = mi.load_dict({"type": "mask", "opacity": 0.3, "child": {"type": "diffuse"}})
    assert m.component_count() == 2 and m.flags(0) == F.DiffuseReflection | F.FrontSide and m.flags(1) == null
    assert m.flags() == m.flags(0) | null and (m.flags() & F.Smooth)
    m = mi.load_dict({"type": "mask", "child": {"type": "twosided", "a": {"type": "diffuse"}, "b": {"type": "roughplastic"}}})
    assert m.component_count() == 4 and m.flags(3) == null and m.flags(1) == F.GlossyReflection | F.BackSide
    assert abs(float(m.value[0]) - 0.5) < 1e-7                     # the default opacity (mask.cpp:95)
    m = mi.load_dict({"type": "mask", "child": {"type": "conductor"}})
    assert m.component_count() == 2 and not (m.flags() & F.Smooth)


# ------------------------------------------------------------------------------------------------ 2. composition against the oracle

@pytest.mark.parametrize("opacity", M.OPACITY_NAMES)
@pytest.mark.parametrize("nested", M.NESTED_NAMES)
def test_composition_against_oracle(mi, O, nested, opacity):
    """eval / pdf / sample of the mask on 20 000 tuples (both sides, grazing directions, sample1 at 0, at o, one float below and above o, one float below 1), five
    contexts, against mask.cpp restated in float32 over the oracle's nested answers; the opacity from an independent float64 lookup.  Every lane is compared;
    sampled_type and sampled_component must be equal.  Measured maxima: docs/parity.md, "mask"."""
    bsdf = mi.load_dict(M.mask_dict(mi, nested, opacity)); scene, ib = B.bound(mi, bsdf)
    ch = M.Nested(mi, O, nested)
    wi, uv, wo, s1, s2, o = B.tuples(opacity)
    worst = {}
    nulls = 0
    for ctx in M.contexts(nested):
        val, pdf = B.host_eval_pdf(mi, scene, ib, ctx, wi, uv, wo)
        ev, ep, raw = M.expected_eval_pdf(ch, ctx, o, wi, uv, wo)
        assert np.isfinite(val).all() and np.isfinite(pdf).all()
        assert np.allclose(pdf, ep, **LEAF), (nested, opacity, ctx, "pdf", float(np.abs(pdf - ep).max()))
        assert np.allclose(val, ev, **MIXED), (nested, opacity, ctx, "value", float(np.abs(val - ev).max()))
        got = B.host_sample(mi, scene, ib, ctx, wi, uv, s1, s2)
        want = M.expected_sample(ch, ctx, o, wi, uv, s1, s2)
        for key in ("sampled_type", "sampled_component", "eta"):
            assert np.array_equal(got[key], want[key]), (nested, opacity, ctx, key, int((got[key] != want[key]).sum()))
        nl = want["null"] & (want["sampled_type"] == M.NULL)
        nulls += int(nl.sum())
        assert np.array_equal(got["wo"][:, nl], -wi[:, nl]) and (got["weight"][:, nl] == 1).all()      # the null lobe: wo = -wi and weight = 1 exactly (its pdf 1 - o: the leaf bar, below)
        assert np.allclose(got["wo"], want["wo"], rtol=2e-6, atol=1e-7), (nested, opacity, ctx, "wo")
        assert np.allclose(got["pdf"], want["pdf"], **LEAF), (nested, opacity, ctx, "sample pdf", float(np.abs(got["pdf"] - want["pdf"]).max()))
        assert np.allclose(got["weight"], want["weight"], **LEAF), (nested, opacity, ctx, "weight", float(np.abs(got["weight"] - want["weight"]).max()))
        for name, a, b in (("value", val, ev), ("pdf", pdf, ep), ("sample weight", got["weight"], want["weight"]), ("sample pdf", got["pdf"], want["pdf"])):
            big = np.abs(b) > 1e-6
            if big.any():
                worst[name] = max(worst.get(name, 0.0), float((np.abs(a[big].astype(np.float64) - b[big]) / np.abs(b[big])).max()))
    assert nulls > 1000
    if nested != "dielectric":
        assert worst.get("value", 0.0) >= 0.0 and (B.host_eval_pdf(mi, scene, ib, (0, 0x1ff, ALL), wi, uv, wo)[0] > 0).any()
    print("mask composition %s / %s: largest relative differences %s" % (nested, opacity, {k: "%.2e" % v for k, v in worst.items()}))


def test_masked_lanes_and_null_context(mi):
    bsdf = mi.load_dict(M.mask_dict(mi, "plastic", "constant")); scene, ib = B.bound(mi, bsdf)
    wi, uv, wo, s1, s2, o = B.tuples("constant", n=512)
    active = (np.arange(512) % 3 != 0)
    val, pdf = B.host_eval_pdf(mi, scene, ib, (0, 0x1ff, ALL), wi, uv, wo, active)
    v0, p0 = B.host_eval_pdf(mi, scene, ib, None, wi, uv, wo)
    assert (val[:, ~active] == 0).all() and (pdf[~active] == 0).all() and np.array_equal(val[:, active], v0[:, active]) and np.array_equal(pdf[active], p0[active])
    bs = B.host_sample(mi, scene, ib, (0, 0x1ff, ALL), wi, uv, s1, s2, active)
    assert (bs["weight"][:, ~active] == 0).all() and (bs["wo"][:, ~active] == 0).all() and (bs["sampled_type"][~active] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. host renders against the oracle through identical geometry

RES, SPP = (16, 12), 4


def _host_vs_oracle(mi, O, product, twin, seed=3, spp=SPP, md=6, rr=7):
    from tests.test_cpu_host import rel_l2
    scene = mi.load_dict(product); ref = mi.load_dict(twin)
    osc, osensor = O.scene_from_product(ref)
    got, gst = B.host_render_stats(mi, scene, seed, spp, md, rr)
    want, st = osc.render_path(osensor, seed=seed, spp=spp, max_depth=md, rr_depth=rr, raw=True, threads=2)
    assert np.isfinite(got).all() and np.linalg.norm(want[..., :3]) > 0
    return rel_l2(O.develop(got), O.develop(want)), (gst.paths, gst.vertices), (st.paths, st.vertices)


@pytest.mark.parametrize("variant", ["plain", "twosided", "instanced", "two_layers"])
def test_host_render_binary_tiles(mi, O, variant):
    """opacity texels of 0 and 1: the product's mask card against the oracle's card of nested / index-matched dielectric quads.  With o in {0, 1} the remap sample1 / o is
    the identity, so both sides draw the same numbers along the same rays: relative L2 1e-4 and equal path and vertex counts (ray counts are not compared: the mask files
    zero-contribution emitter samples that the dielectric does not).  A `sample1` of exactly 0 would make the index-matched dielectric reflect; seed 3 meets none."""
    tex = M.binary_texels()
    nested = M.TWOSIDED if variant == "twosided" else M.DIFFUSE
    kw = dict(layers=(0.55, 0.2) if variant == "two_layers" else (0.55, ), instanced=variant == "instanced")
    err, got, want = _host_vs_oracle(mi, O, M.card_scene(mi, RES, SPP, tex, nested, True, **kw), M.card_scene(mi, RES, SPP, tex, nested, False, **kw))
    print("host render, binary tiles %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (variant, err, got, want))
    assert err <= 1e-4 and got == want and got[1] > got[0]


@pytest.mark.parametrize("kind", ["one_constant", "one_bitmap", "zero"])
def test_host_render_end_points(mi, O, kind):
    """o == 1 (a constant, a bitmap) against the pure nested card with equal counters, o == 0 against the all-dielectric card"""
    full = np.ones((M.K, M.K, 1), np.float32) if kind != "zero" else np.zeros((M.K, M.K, 1), np.float32)
    product = M.card_scene(mi, RES, SPP, full, M.DIFFUSE, True, opacity=1.0 if kind == "one_constant" else None)
    err, got, want = _host_vs_oracle(mi, O, product, M.card_scene(mi, RES, SPP, full, M.DIFFUSE, False))
    print("host render, %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (kind, err, got, want))
    assert err <= 1e-4 and got == want


# ------------------------------------------------------------------------------------------------ 4. partial opacity, statistically

OPACITY = M.OPACITY


@pytest.fixture(scope="module")
def pure_batches(mi, O):
    return M.oracle_pure_batches(mi, O)


def test_partial_opacity_statistics_host(mi, O, pure_batches):
    spp = 512
    scene = mi.load_dict(M.lit_card(mi, {"type": "mask", "opacity": OPACITY, "n": dict(M.DIFFUSE)}, spp))
    film, _ = B.host_render_stats(mi, scene, 77, spp, 3, 8)
    img = O.develop(film).astype(np.float64)
    ok, pmin, alpha, bad, pmin_bad = M.statistics_verdicts(img, spp, pure_batches)
    print("mask z-test (host): accepted %s (min p %.3g, alpha %.3g); against o = 0.55: accepted %s (min p %.3g)" % (ok, pmin, alpha, bad, pmin_bad))
    assert not bad, "the test has no power: the composition at o = 0.55 is accepted"
    assert ok


# ------------------------------------------------------------------------------------------------ 5. aov

def test_aov_channels(mi, O):
    """albedo of a mask pixel = the nested BSDF's (mask.cpp:229-232; the integrator reports the FIRST intersection and does not look through masks); depth and
    shape_index equal those of the scene without the mask bit for bit"""
    tex = np.random.default_rng(4).uniform(0.1, 0.9, (6, 4, 3)).astype(np.float32)
    inner = {"type": "twosided", "x": {"type": "diffuse", "reflectance": {"type": "bitmap", "data": tex, "raw": True}}}
    masked = mi.load_dict(M.lit_card(mi, {"type": "mask", "opacity": 0.25, "n": inner}, 4))
    plain = mi.load_dict(M.lit_card(mi, dict(inner), 4))
    n = 2048; rng = np.random.default_rng(6)
    o = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-1.2, 1.2, n), np.where(np.arange(n) % 2 == 0, 2.0, 0.25)]).astype(np.float32)       # from above and from below the card
    d = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), np.where(np.arange(n) % 2 == 0, -1.0, 1.0)]); d = (d / np.linalg.norm(d, axis=0)).astype(np.float32)
    maxt = np.full(n, np.inf, np.float32)
    aov = mi.load_dict({"type": "aov", "aovs": "ab:albedo,dd:depth,si:shape_index"})
    a = aov.sample_host(masked, o, d, maxt); b = aov.sample_host(plain, o, d, maxt)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and (a[0:3] > 0).any() and (a[3] > 0).any()


# ------------------------------------------------------------------------------------------------ 6. the loader

def test_loader_errors(mi):
    df = {"type": "diffuse"}
    with pytest.raises(RuntimeError, match="Cannot specify more than one child BSDF"):
        mi.load_dict({"type": "mask", "opacity": 0.5, "a": df, "b": df})
    with pytest.raises(RuntimeError, match="Child BSDF not specified"):
        mi.load_dict({"type": "mask", "opacity": 0.5})
    with pytest.raises(RuntimeError, match="Unreferenced property \"alpha\""):
        mi.load_dict({"type": "mask", "opacity": 0.5, "a": df, "alpha": 0.3})
    with pytest.raises(RuntimeError, match="Unreferenced property \"light\""):
        mi.load_dict({"type": "mask", "opacity": 0.5, "a": df, "light": {"type": "point"}})
    with pytest.raises(RuntimeError, match="nested `blendbsdf`"):
        mi.load_dict({"type": "mask", "a": {"type": "blendbsdf", "weight": 0.1, "x": df, "y": df}})
    with pytest.raises(RuntimeError, match="nested `mask`"):
        mi.load_dict({"type": "mask", "a": {"type": "mask", "x": df}})
    with pytest.raises(RuntimeError, match="nested `mask`"):
        mi.load_dict({"type": "blendbsdf", "weight": 0.5, "a": df, "b": {"type": "mask", "x": df}})
    with pytest.raises(RuntimeError, match="Only materials without a transmission component can be nested"):
        mi.load_dict({"type": "twosided", "n": {"type": "mask", "x": df}})
    with pytest.raises(RuntimeError, match="1 or 3"):
        mi.load_dict({"type": "mask", "opacity": {"type": "bitmap", "data": np.zeros((2, 2, 4), np.float32)}, "a": df})
    for ok in ({"type": "twosided", "x": df}, {"type": "twosided", "x": df, "y": {"type": "roughplastic"}}, {"type": "dielectric"}):
        assert mi.load_dict({"type": "mask", "a": ok}).kind == "mask"


def test_record_validation(mi):
    """the C ABI (lower_scene) refuses what the loader refuses, by name"""
    import ctypes as C
    from mitsuba3_amd import _capi
    L = mi.lib()

    def create(recs):
        arr = (_capi.HarBSDF * len(recs))()
        for i, r in enumerate(recs):
            arr[i].type = r.get("type", 0); arr[i].texture = -1; arr[i].flags = r.get("flags", 0); arr[i].back = r.get("back", -1); arr[i].eta = 1.5
            arr[i].nested = (C.c_int32 * 2)(*r.get("nested", (0, 0)))
        d = _capi.HarSceneDesc(); d.bsdfs = arr; d.bsdf_count = len(recs)
        v = np.zeros((3, 1), np.float32); uv = np.zeros((2, 1), np.float32); out = np.zeros((3, 1), np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        rc = L.har_bsdf_eval_pdf_host(C.byref(d), 0, None, 1, fp(v), fp(uv), fp(v), None, fp(out), None)
        return rc, (L.har_last_error() or b"").decode()

    assert create([dict(type=7, nested=(1, -1)), dict()])[0] == 0
    assert create([dict(type=7, nested=(1, -1)), dict(flags=1)])[0] == 0                       # twosided, one BSDF
    assert create([dict(type=7, nested=(1, -1)), dict(flags=1, back=2), dict(type=3)])[0] == 0  # twosided, two BSDFs
    rc, msg = create([dict(type=7, nested=(3, -1)), dict()]); assert rc != 0 and "out of range" in msg
    rc, msg = create([dict(type=7, nested=(-1, -1)), dict()]); assert rc != 0 and "out of range" in msg
    rc, msg = create([dict(type=7, nested=(1, -1)), dict(type=7, nested=(2, -1)), dict()]); assert rc != 0 and "nested `mask`" in msg
    rc, msg = create([dict(type=7, nested=(1, -1)), dict(type=6, nested=(2, 2)), dict()]); assert rc != 0 and "nested `blendbsdf`" in msg
    rc, msg = create([dict(type=6, nested=(1, 2)), dict(type=7, nested=(2, -1)), dict()]); assert rc != 0 and "nested `mask`" in msg
    rc, msg = create([dict(type=7, flags=1, nested=(1, -1)), dict()]); assert rc != 0 and "twosided over `mask`" in msg and "transmission" in msg
    rc, msg = create([dict(flags=1, back=1), dict(type=7, nested=(2, -1)), dict()]); assert rc != 0 and "twosided over `mask`" in msg
    rc, msg = create([dict(type=8)]); assert rc != 0 and "unsupported BSDF type" in msg


def _plane_scene(mi, opacity, nested=None):
    return {"type": "scene",
            "integrator": {"type": "path", "max_depth": 3},
            "sensor": {"type": "perspective", "fov": 40, "to_world": mi.ScalarTransform4f().look_at([0, 0, 3], [0, 0, 0], [0, 1, 0]),
                       "film": {"type": "hdrfilm", "width": 12, "height": 8}, "sampler": {"type": "independent", "sample_count": 4}},
            "mat": {"type": "mask", "opacity": opacity, "material": nested or {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.8, 0.3, 0.2]}}},
            "plane": {"type": "rectangle", "bsdf": {"type": "ref", "id": "mat"}},
            "behind": {"type": "rectangle", "to_world": mi.ScalarTransform4f().translate([0, 0, -0.5]).scale([2.0, 2.0, 1.0]),
                       "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.2, 0.6, 0.7]}}},
            "light": {"type": "rectangle", "to_world": mi.ScalarTransform4f().translate([0, 0, 4]).rotate([1, 0, 0], 180), "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [9, 9, 9]}}}}


def _host_film(mi, scene, seed=1):
    from tests.thinlens_cases import host_render
    return host_render(mi, scene, scene.sensors()[0], seed, 4, 3)


def test_traverse_names_and_update(mi):
    import torch
    scene = mi.load_dict(_plane_scene(mi, 0.3))
    p = mi.traverse(scene)
    assert {"mat.opacity.value", "mat.nested_bsdf.reflectance.value"} <= set(p.keys())
    assert tuple(p["mat.opacity.value"].shape) == (1,) and abs(float(p["mat.opacity.value"][0]) - 0.3) < 1e-7
    two = mi.traverse(mi.load_dict(_plane_scene(mi, 0.3, {"type": "twosided", "a": {"type": "diffuse"}, "b": {"type": "roughconductor"}})))
    assert {"mat.opacity.value", "mat.nested_bsdf.brdf_0.reflectance.value", "mat.nested_bsdf.brdf_1.specular_reflectance.value", "mat.nested_bsdf.brdf_1.alpha.value"} <= set(two.keys())
    one = mi.traverse(mi.load_dict(_plane_scene(mi, 0.3, {"type": "twosided", "a": {"type": "diffuse"}})))
    assert "mat.nested_bsdf.brdf_0.reflectance.value" in one and not any(".brdf_1." in k for k in one.keys())
    tex = np.random.default_rng(2).uniform(0.1, 0.9, (4, 6, 1)).astype(np.float32)
    prop = lambda t: {"type": "bitmap", "data": t, "raw": True, "to_uv": mi.ScalarTransform3f().scale([2.0, 1.0])}
    scene1 = mi.load_dict(_plane_scene(mi, prop(tex)))
    p1 = mi.traverse(scene1)
    assert tuple(p1["mat.opacity.data"].shape) == (4, 6, 1) and "mat.opacity.to_uv" in p1 and np.array_equal(p1["mat.opacity.data"].cpu().numpy(), tex)
    tex3 = np.random.default_rng(3).uniform(0.1, 0.9, (4, 6, 3)).astype(np.float32)
    assert tuple(mi.traverse(mi.load_dict(_plane_scene(mi, {"type": "bitmap", "data": tex3, "raw": True})))["mat.opacity.data"].shape) == (4, 6, 3)
    # update() of the opacity, of opacity texels and of a nested colour gives the scene a fresh load gives: the same host render, bit for bit
    p["mat.opacity.value"] = torch.tensor([0.65]); p["mat.nested_bsdf.reflectance.value"] = torch.tensor([0.1, 0.7, 0.4]); p.update()
    fresh = mi.load_dict(_plane_scene(mi, 0.65, {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.1, 0.7, 0.4]}}))
    a, b = _host_film(mi, scene), _host_film(mi, fresh)
    assert np.array_equal(a, b) and np.abs(a[..., :3]).sum() > 0
    assert not np.array_equal(a, _host_film(mi, mi.load_dict(_plane_scene(mi, 0.3))))
    tex_new = (1.0 - tex).astype(np.float32)
    p1["mat.opacity.data"] = torch.tensor(tex_new); p1.update()
    assert np.array_equal(_host_film(mi, scene1), _host_film(mi, mi.load_dict(_plane_scene(mi, prop(tex_new)))))
    with pytest.raises(RuntimeError, match="expected"):
        p["mat.opacity.value"] = torch.tensor([0.1, 0.2, 0.3]); p.update()


def test_load_string_equals_load_dict(mi, tmp_path):
    xml = """<scene version="3.0.0">
  <integrator type="path"><integer name="max_depth" value="3"/></integrator>
  <sensor type="perspective"><float name="fov" value="40"/>
    <transform name="to_world"><lookat origin="0, 0, 3" target="0, 0, 0" up="0, 1, 0"/></transform>
    <film type="hdrfilm"><integer name="width" value="12"/><integer name="height" value="8"/></film>
    <sampler type="independent"><integer name="sample_count" value="4"/></sampler></sensor>
  <bsdf type="mask" id="mat"><float name="opacity" value="0.3"/>
    <bsdf type="diffuse" name="material"><rgb name="reflectance" value="0.8, 0.3, 0.2"/></bsdf></bsdf>
  <shape type="rectangle" id="plane"><ref id="mat"/></shape>
  <shape type="rectangle" id="behind"><transform name="to_world"><scale x="2" y="2" z="1"/><translate x="0" y="0" z="-0.5"/></transform>
    <bsdf type="diffuse"><rgb name="reflectance" value="0.2, 0.6, 0.7"/></bsdf></shape>
  <shape type="rectangle" id="light"><transform name="to_world"><rotate x="1" angle="180"/><translate x="0" y="0" z="4"/></transform>
    <emitter type="area"><rgb name="radiance" value="9, 9, 9"/></emitter></shape>
</scene>"""
    a = mi.load_string(xml); b = mi.load_dict(_plane_scene(mi, 0.3))
    assert [o.kind for o in a.bsdf_objs][:2] == ["mask", "diffuse"]
    fa, fb = _host_film(mi, a), _host_film(mi, b)
    assert np.abs(fb[..., :3]).sum() > 0 and np.allclose(fa, fb, rtol=1e-6, atol=1e-7)
    # <texture name="opacity" .../>: a three-channel bitmap read from a file
    tex = np.random.default_rng(5).uniform(0.1, 0.9, (4, 6, 3)).astype(np.float32)
    f = tmp_path / "opacity.exr"; mi.Bitmap(tex).write(str(f))
    c = mi.load_string(xml.replace('<float name="opacity" value="0.3"/>', '<texture type="bitmap" name="opacity"><string name="filename" value="%s"/><boolean name="raw" value="true"/></texture>' % f))
    e = mi.load_dict(_plane_scene(mi, {"type": "bitmap", "filename": str(f), "raw": True}))
    fc, fe = _host_film(mi, c), _host_film(mi, e)
    assert np.allclose(fc, fe, rtol=1e-6, atol=1e-7) and not np.allclose(fc, fb, rtol=1e-3, atol=1e-6)
