"""`bumpmap` on the CPU, through the library's host entries (har_texture_eval_1_grad_host / har_bsdf_eval_pdf_si_host / har_bsdf_sample_si_host / har_bumpmap_grad_host /
har_render_lanes_stats_host / har_aov_sample_host run the HAR_HD code the kernels run): eval_1_grad of a bitmap and its transpose against NumPy float64, bumpmap.cpp restated
in NumPy over the oracle's answers for the nested BSDF alone, the per-call derivative against central differences of the float64 restatement, host renders, the loader and
the parameters."""
import ctypes as C

import numpy as np
import pytest

from tests import blend_cases as B
from tests import bumpmap_cases as U
from tests import normalmap_cases as N

ALL = N.ALL
F32 = np.float32
LEAF = dict(rtol=2e-6, atol=1e-9)          # the project's bars: the leaf models against the oracle, pdfs and un-mixed values
MIXED = dict(rtol=2e-5, atol=1e-7)         # ... values with the shadow term and sample weights
RES, SPP = (16, 12), 4


# ------------------------------------------------------------------------------------------------ 1. eval_1_grad of a bitmap

# |grad - float64 restatement| / (resolution * max |texel|), largest over all cases: measured 2.2e-7 (docs/parity.md, "bumpmap"); the bar is four times that
EVAL_1_GRAD_BAR = 8.8e-7
assert EVAL_1_GRAD_BAR <= 1e-4


def _grad_uv(n=20000, seed=3):
    return np.random.default_rng(seed).uniform(-2.0, 3.0, (2, n)).astype(F32)


def _tex_scene(mi, prop):
    bsdf = mi.load_dict({"type": "bumpmap", "h": prop, "x": {"type": "diffuse"}})
    scene, ib = B.bound(mi, bsdf)
    return scene, bsdf.tex_index


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", [(8, 8), (3, 5)])          # (h, w): the 8 x 8 and the 5 x 3 (w x h) bitmaps
def test_eval_1_grad_against_float64(mi, size, channels):
    """har_texture_eval_1_grad_host against BitmapTexture::eval_1_grad restated in NumPy float64 at 20 000 uv in [-2, 3]^2: bilinear x repeat / mirror / clamp, to_uv none /
    scale + offset / two rotations; the bar is absolute, relative to resolution * max |texel| (the quantity is a difference of texels)"""
    uv = _grad_uv()
    tex = U.noise(size[0], size[1], channels, 7 + channels)
    worst = 0.0
    for wrap in ("repeat", "mirror", "clamp"):
        for name, m in U.to_uv_cases(mi).items():
            scene, t = _tex_scene(mi, U.bitmap_prop(mi, tex, m, wrap))
            got = U.host_eval_1_grad(mi, scene, t, uv)
            want = U.eval_1_grad64(tex, uv, m, wrap)
            err = float(np.abs(got - want).max() / (max(size) * float(np.abs(tex).max())))
            worst = max(worst, err)
            assert np.isfinite(got).all() and np.abs(want).max() > 0.1
            assert err <= EVAL_1_GRAD_BAR, (wrap, name, err)
    print("eval_1_grad %dx%dx%d: largest |difference| / (resolution * max |texel|) %.3g (bar %.3g)" % (size[1], size[0], channels, worst, EVAL_1_GRAD_BAR))


def test_eval_1_grad_of_a_nearest_map_is_exactly_zero(mi):
    tex = U.noise(8, 8, 3, 4)
    scene, t = _tex_scene(mi, U.bitmap_prop(mi, tex, nearest=True))
    got = U.host_eval_1_grad(mi, scene, t, _grad_uv(2000))
    assert (got == 0).all()
    dep = np.zeros((8, 8, 3), F32)
    U.host_eval_1_grad(mi, scene, t, _grad_uv(2000), g=np.ones((2, 2000), F32), deposit=dep)
    assert (dep == 0).all()


@pytest.mark.parametrize("size", [(8, 8), (3, 5)])
@pytest.mark.parametrize("channels", [1, 3])
def test_eval_1_grad_finite_differences(mi, channels, size):
    """the recipe of the reference's own test (src/textures/tests/test_bitmap.py: eval_1 at uv +- delta against eval_1_grad) in float64 with delta = 1e-4, away from texel-cell
    borders -- the interpolant is bilinear inside a cell, so the central difference is exact up to rounding.  The reference's stated atol = 1e04 is vacuous; the bar here is
    4e-6 of resolution * max |texel|: the product forms the texel coordinate p in float32 (|p| <= 50 for these uv: half an ulp is 1.9e-6, twice -- the to_uv row and the
    resolution), which is the error of a bilinear weight.  eval_1_grad multiplies by the resolution AFTER the transpose of to_uv (bitmap.cpp:593-598): that is the
    derivative of eval_1 for a square bitmap or an axis-aligned to_uv -- with a rotation on a 5 x 3 bitmap it is not (docs/parity.md), and those cases are left to the
    restatement above"""
    h, w = size
    tex = U.noise(h, w, channels, 21)
    uv = _grad_uv(20000, 5)
    for name, m in U.to_uv_cases(mi).items():
        if h != w and name.startswith("rot"):
            continue
        keep = U.cell_margin(tex, uv, m) > 0.02
        mm = np.eye(3) if m is None else np.asarray(m, F32).astype(np.float64)
        f = tex[:, :, 0].astype(np.float64) if channels == 1 else (tex.astype(np.float64) * U.LUM).sum(2)
        big = np.pad(f, ((12 * h, 12 * h), (12 * w, 12 * w)), mode="wrap")

        def eval_1(p):          # bilinear + repeat lookup in float64 at float64 uv
            q = mm[:2, :2] @ p + mm[:2, 2:3]
            px, py = q[0] * w - 0.5, q[1] * h - 0.5
            x0, y0 = np.floor(px).astype(int), np.floor(py).astype(int); fx, fy = px - x0, py - y0
            t = lambda x, y: big[y + 12 * h, x + 12 * w]
            return (1 - fy) * ((1 - fx) * t(x0, y0) + fx * t(x0 + 1, y0)) + fy * ((1 - fx) * t(x0, y0 + 1) + fx * t(x0 + 1, y0 + 1))

        p = uv.astype(np.float64); d = 1e-4
        fd = np.stack([(eval_1(p + [[d], [0]]) - eval_1(p - [[d], [0]])) / (2 * d), (eval_1(p + [[0], [d]]) - eval_1(p - [[0], [d]])) / (2 * d)])
        scene, t = _tex_scene(mi, U.bitmap_prop(mi, tex, m))
        got = U.host_eval_1_grad(mi, scene, t, uv)
        err = float(np.abs(got[:, keep] - fd[:, keep]).max() / (max(size) * float(np.abs(tex).max())))
        print("eval_1_grad against finite differences, %dx%dx%d, to_uv %s: %.3g on %d lookups" % (w, h, channels, name, err, int(keep.sum())))
        assert keep.sum() > 10000 and err <= 4e-6


@pytest.mark.parametrize("channels", [1, 3])
def test_eval_1_grad_adjoint_identity(mi, channels):
    """eval_1_grad is linear in the texels: sum_j deposit_j f_j = sum_i g_i . grad_i(f), at 1e-5 (relative to the sum of |terms|), on the same points, every wrap mode"""
    tex = U.noise(8, 8, channels, 9)
    uv = _grad_uv()
    g = np.random.default_rng(2).uniform(-1, 1, uv.shape).astype(F32)
    for wrap in ("repeat", "mirror", "clamp"):
        for name, m in U.to_uv_cases(mi).items():
            scene, t = _tex_scene(mi, U.bitmap_prop(mi, tex, m, wrap))
            dep = np.zeros((8, 8, 3), F32)
            grad = U.host_eval_1_grad(mi, scene, t, uv, g=g, deposit=dep)
            stored = np.repeat(tex, 3, 2) if channels == 1 else tex
            if channels == 1:
                assert (dep[:, :, 1:] == 0).all()          # a one-channel map is stored three times; channel 0 receives the deposit
                lhs = float((dep[:, :, 0].astype(np.float64) * tex[:, :, 0]).sum())
            else:
                lhs = float((dep.astype(np.float64) * stored).sum())
                # grad_k = lum_k x the luminance map's deposit (the coefficients sum to one); the three channels are accumulated separately in float32
                assert np.allclose(dep, dep.astype(np.float64).sum(2, keepdims=True) * U.LUM, rtol=0, atol=1e-4 * float(np.abs(dep).max()))
            rhs = float((g.astype(np.float64) * grad).sum())
            scale = float(np.abs(g.astype(np.float64) * grad).sum())
            assert abs(lhs - rhs) <= 1e-5 * scale, (wrap, name, lhs, rhs, scale)


def test_texture_eval_1_grad_in_python(mi):
    """Texture.eval_1_grad(si) on a bitmap; any other texture raises NotImplementedError("eval_1_grad") (src/render/texture.cpp:38-39)"""
    tex = U.noise(3, 5, 1, 2)
    t = mi.load_dict(U.bitmap_prop(mi, tex))
    uv = _grad_uv(500)
    si = type("SI", (), dict(uv=uv))()
    got = np.asarray(t.eval_1_grad(si))
    assert np.allclose(got, U.eval_1_grad64(tex, uv), atol=1e-5)
    for other in ({"type": "rgb", "value": [0.1, 0.2, 0.3]}, {"type": "mesh_attribute", "name": "vertex_color"}):
        with pytest.raises(NotImplementedError, match="eval_1_grad"):
            mi.load_dict(other).eval_1_grad(si)


# ------------------------------------------------------------------------------------------------ 2. the record and the loader

def test_components_flags_and_keys(mi):
    F = mi.BSDFFlags
    h1 = U.bitmap_prop(mi, U.noise(4, 6, 1, 1)); h3 = U.bitmap_prop(mi, U.noise(4, 6, 3, 1))
    b = mi.load_dict({"type": "bumpmap", "arbitrary": h1, "nested": {"type": "roughplastic"}})
    assert b.component_count() == 2 and b.flags(0) == F.GlossyReflection | F.FrontSide and b.flags(1) == F.DiffuseReflection | F.FrontSide and (b.flags() & F.Smooth)
    assert int(b.flags) & 64 and int(b.flags) & 128 and int(b.flags) & 16 and b.alpha_u == 1.0          # both switches default to true, scale to 1 (bumpmap.cpp:119-122)
    b = mi.load_dict({"type": "bumpmap", "t": h3, "x": {"type": "conductor"}, "flip_invalid_normals": False, "use_shadowing_function": False, "scale": 2.5})
    assert b.component_count() == 1 and not (b.flags() & F.Smooth) and not (int(b.flags) & (64 | 128 | 16)) and b.alpha_u == 2.5
    sc = mi.load_dict({"type": "scene", "bumpy": {"type": "bumpmap", "t": h1, "inner": {"type": "twosided", "a": {"type": "diffuse"}, "b": {"type": "plastic"}}},
                       "rgbmap": {"type": "twosided", "n": {"type": "bumpmap", "t": h3, "inner": {"type": "diffuse"}, "scale": 0.5}},
                       "r": {"type": "rectangle", "bsdf": {"type": "ref", "id": "bumpy"}}, "q": {"type": "cube", "bsdf": {"type": "ref", "id": "rgbmap"}}})
    p = mi.traverse(sc)
    keys = set(p.keys())
    want = {"bumpy.nested_texture.data", "bumpy.scale", "bumpy.nested_bsdf.brdf_0.reflectance.value", "bumpy.nested_bsdf.brdf_1.diffuse_reflectance.value",
            "rgbmap.brdf_0.nested_texture.data", "rgbmap.brdf_0.scale", "rgbmap.brdf_0.nested_bsdf.reflectance.value"}
    assert want <= keys, sorted(want - keys)
    assert tuple(p["bumpy.nested_texture.data"].shape) == (4, 6, 1) and tuple(p["rgbmap.brdf_0.nested_texture.data"].shape) == (4, 6, 3)
    assert float(p["rgbmap.brdf_0.scale"]) == 0.5
    PF = mi.ParamFlags
    assert p.flags("bumpy.scale") == PF.NonDifferentiable and p.flags("bumpy.nested_texture.data") == PF.Differentiable
    # a bumpmap sets no BSDFFlags::NormalMapped: no mesh gets a tangent frame, a cube (normals AND texcoords) loads
    d = sc.desc()
    assert all((d.meshes[i].flags & 12) == 0 for i in range(d.mesh_count))


def test_loader_messages(mi):
    h = U.bitmap_prop(mi, U.noise(4, 4, 1, 1))
    with pytest.raises(RuntimeError, match="Exactly one BSDF child object must be specified."):
        mi.load_dict({"type": "bumpmap", "t": h})
    with pytest.raises(RuntimeError, match="Only a single BSDF child object can be specified."):
        mi.load_dict({"type": "bumpmap", "t": h, "a": {"type": "diffuse"}, "b": {"type": "diffuse"}})
    with pytest.raises(RuntimeError, match="Exactly one Texture child object must be specified."):
        mi.load_dict({"type": "bumpmap", "a": {"type": "diffuse"}})
    with pytest.raises(RuntimeError, match="Only a single Texture child object can be specified."):
        mi.load_dict({"type": "bumpmap", "t": h, "t2": dict(h), "a": {"type": "diffuse"}})
    with pytest.raises(RuntimeError, match="(?i)unreferenced property \"strength\""):
        mi.load_dict({"type": "bumpmap", "t": h, "a": {"type": "diffuse"}, "strength": True})
    for what, tex in (("rgb", {"type": "rgb", "value": [0.5, 0.5, 1.0]}), ("mesh_attribute", {"type": "mesh_attribute", "name": "vertex_h"}), ("float", 0.5)):
        with pytest.raises(RuntimeError, match="bumpmap.*`%s`.*bitmap" % what):
            mi.load_dict({"type": "bumpmap", "t": tex, "a": {"type": "diffuse"}})
    inner = {"type": "bumpmap", "t": h, "a": {"type": "diffuse"}}
    nm = {"type": "rgb", "value": [0.5, 0.5, 1.0]}
    for kind, child in (("blendbsdf", {"type": "blendbsdf", "weight": 0.5, "a": {"type": "diffuse"}, "b": {"type": "diffuse"}}), ("mask", {"type": "mask", "opacity": 0.5, "a": {"type": "diffuse"}}),
                        ("normalmap", {"type": "normalmap", "normalmap": nm, "a": {"type": "diffuse"}}), ("bumpmap", inner)):
        with pytest.raises(RuntimeError, match="bumpmap: a nested `%s`" % kind):
            mi.load_dict({"type": "bumpmap", "t": h, "x": child})
    with pytest.raises(RuntimeError, match="blendbsdf: a nested `bumpmap`"):
        mi.load_dict({"type": "blendbsdf", "weight": 0.5, "a": dict(inner), "b": {"type": "diffuse"}})
    with pytest.raises(RuntimeError, match="mask: a nested `bumpmap`"):
        mi.load_dict({"type": "mask", "opacity": 0.5, "a": dict(inner)})
    with pytest.raises(RuntimeError, match="normalmap: a nested `bumpmap`"):
        mi.load_dict({"type": "normalmap", "normalmap": nm, "a": dict(inner)})
    with pytest.raises(RuntimeError, match="twosided.*bumpmap"):          # the two-children form with a bumpmap among them
        mi.load_dict({"type": "twosided", "a": dict(inner), "b": {"type": "diffuse"}})
    with pytest.raises(RuntimeError, match="transmission"):               # twosided.cpp:79-83 sees the nested BSDF's lobes
        mi.load_dict({"type": "twosided", "a": {"type": "bumpmap", "t": h, "x": {"type": "dielectric"}}})
    # a scene with a bumpmap and a mesh_attribute texture: refused when the scene is lowered
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)
    sc = mi.load_dict({"type": "scene", "r": {"type": "rectangle", "bsdf": dict(inner)},
                       "tri": {"type": "mesh", "positions": P, "faces": np.array([[0, 1, 2]], np.uint32), "attributes": {"vertex_color": np.ones((3, 3), F32)},
                               "bsdf": {"type": "diffuse", "reflectance": {"type": "mesh_attribute", "name": "vertex_color"}}}})
    d = sc.desc()
    v = np.array([[0.0], [0.0], [1.0]], F32); uv = np.zeros((2, 1), F32); out = np.zeros((3, 1), F32)
    assert mi.lib().har_bsdf_eval_pdf_host(C.byref(d), 0, None, 1, B._fp(v), B._fp(uv), B._fp(v), None, B._fp(out), None) != 0
    err = mi.lib().har_last_error()
    assert b"bumpmap" in err and b"mesh_attribute" in err


def test_old_entries_refuse_a_bumpmap_record_by_name(mi):
    b = mi.load_dict({"type": "bumpmap", "t": U.bitmap_prop(mi, U.noise(4, 4, 1, 1)), "a": {"type": "diffuse"}})
    scene, ib = B.bound(mi, b)
    d = scene.desc()
    v = np.array([[0.0], [0.0], [1.0]], F32); uv = np.zeros((2, 1), F32); out = np.zeros((3, 1), F32)
    assert mi.lib().har_bsdf_eval_pdf_host(C.byref(d), ib, None, 1, B._fp(v), B._fp(uv), B._fp(v), None, B._fp(out), None) != 0
    assert b"bumpmap" in mi.lib().har_last_error()


def test_xml_loader_against_dict(mi, tmp_path):
    """<bsdf type="bumpmap"><texture type="bitmap" name="..."/><bsdf .../></bsdf>: the record of the XML file is the record of the dict"""
    tex = U.noise(4, 3, 1, 6)
    pfm = tmp_path / "height.pfm"
    with open(pfm, "wb") as f:
        f.write(b"Pf\n3 4\n-1.0\n"); f.write(np.ascontiguousarray(tex[::-1, :, 0], "<f4").tobytes())
    xml = tmp_path / "bm.xml"
    xml.write_text('<scene version="3.0.0"><bsdf type="bumpmap" id="bumpy"><texture name="arbitrary" type="bitmap"><string name="filename" value="height.pfm"/>'
                   '<boolean name="raw" value="true"/></texture><float name="scale" value="1.5"/><boolean name="use_shadowing_function" value="false"/><bsdf type="roughplastic"/></bsdf>'
                   '<shape type="cube"><ref id="bumpy"/></shape></scene>')
    sc = mi.load_file(str(xml))
    b = sc.bsdfs[sc.meshes[0]["bsdf"]]
    ref = mi.load_dict({"type": "bumpmap", "arbitrary": U.bitmap_prop(mi, tex), "scale": 1.5, "use_shadowing_function": False, "x": {"type": "roughplastic"}})
    assert b.kind == "bumpmap" and b.nested[0].kind == "roughplastic" and b.alpha_u == 1.5 and int(b.flags) == int(ref.flags) == (16 | 64)
    assert np.array_equal(b.texture, ref.texture) and b.weight_channels == 1


# ------------------------------------------------------------------------------------------------ 3. per call, against bumpmap.cpp restated over the oracle

# The float64 lookup: the product forms grad_uv in float32, the restatement in float64; an ulp of grad_uv is an ulp of the frame, which a rough lobe amplifies by about
# 1 / alpha^2.  The bars are four times the largest differences measured over all nested models, geometries, switches and contexts (docs/parity.md, "bumpmap"), never
# above 1e-4.  Measured: value 5.7e-5, pdf 6.9e-5, sampled wo 7.3e-5, sample pdf 7.1e-5, sample weight 6.2e-5 -- four times each is above the cap, so every bar is the cap.
F64_ATOL = dict(value=1e-4, pdf=1e-4, wo=1e-4, sample_pdf=1e-4, weight=1e-4)
assert max(F64_ATOL.values()) <= 1e-4


@pytest.fixture(scope="module")
def tuples20k():
    return N.tuples()


def check_against_restatement(evaluate, sample, ch, nested, geom, g, flip, shadow, wi, uv, wo, s1, s2, worst, f64):
    """one (nested, geometry, switches) case over all contexts: `evaluate(ctx) -> (value, pdf)` and `sample(ctx) -> dict` are the side under test"""
    for ctx in N.contexts(nested):
        val, pdf = evaluate(ctx)
        ev, ep, act, near = U.expected_eval_pdf(ch, ctx, geom, g, wi, uv, wo, flip, shadow)
        assert np.isfinite(val).all() and np.isfinite(pdf).all()
        assert near.mean() <= 1e-3, ("lanes within 1e-6 of a switch", float(near.mean()))          # the cap, on the restatement alone
        keep = ~near
        assert np.array_equal((val != 0).any(0)[keep], (ev != 0).any(0)[keep]) and np.array_equal((pdf != 0)[keep], (ep != 0)[keep]), (nested, flip, shadow, ctx, "zero lanes")
        vbar = dict(rtol=0, atol=F64_ATOL["value"]) if f64 else (MIXED if shadow else LEAF)
        pbar = dict(rtol=0, atol=F64_ATOL["pdf"]) if f64 else LEAF
        assert np.allclose(val[:, keep], ev[:, keep], **vbar), (nested, flip, shadow, ctx, "value", float(np.abs(val[:, keep] - ev[:, keep]).max()))
        assert np.allclose(pdf[keep], ep[keep], **pbar), (nested, flip, shadow, ctx, "pdf", float(np.abs(pdf[keep] - ep[keep]).max()))
        got = sample(ctx)
        want = U.expected_sample(ch, ctx, geom, g, wi, uv, s1, s2, flip, shadow)
        assert want["near"].mean() <= 1e-3
        keep = ~want["near"]
        for key in ("sampled_type", "sampled_component", "eta"):
            assert np.array_equal(got[key][keep], want[key][keep]), (nested, flip, shadow, ctx, key, int((got[key][keep] != want[key][keep]).sum()))
        zg = ~(got["weight"] != 0).any(0); zw = ~(want["weight"] != 0).any(0)
        assert np.array_equal(zg[keep], zw[keep]) and np.array_equal((got["pdf"] != 0)[keep], (want["pdf"] != 0)[keep]), (nested, flip, shadow, ctx, "zero samples")
        live = keep & ~zw
        bars = {k: dict(rtol=0, atol=F64_ATOL[b]) if f64 else std for k, b, std in (("wo", "wo", dict(rtol=2e-6, atol=1e-7)), ("pdf", "sample_pdf", LEAF), ("weight", "weight", MIXED))}
        for key in ("wo", "pdf", "weight"):
            a, b = got[key][..., live], want[key][..., live]
            assert np.allclose(a, b, **bars[key]), (nested, flip, shadow, ctx, "sample " + key, float(np.abs(a - b).max()))
        # weight * pdf == eval at the sampled direction for valid non-delta samples, at 1e-3
        nd = live & ((got["sampled_type"] & 0x60) == 0) & (got["pdf"] > 0)
        if nd.any() and ctx[2] == ALL and ctx[1] == 0x1ff:
            v2, p2 = evaluate(ctx, wo_override=got["wo"])
            lhs = (got["weight"] * got["pdf"][None, :])[:, nd]; rhs = v2[:, nd]
            back = (rhs != 0).any(0)          # (a direction that came back across the perturbed horizon by an ulp evaluates to zero: counted, not compared)
            rel = np.abs(lhs[:, back] - rhs[:, back]) / np.maximum(np.abs(rhs[:, back]), 1e-3)
            worst["consistency"] = max(worst.get("consistency", 0.0), float(rel.max()) if rel.size else 0.0)
            assert back.mean() > 0.999 and (not rel.size or rel.max() <= 1e-3), (nested, flip, shadow, "weight * pdf == eval", float(rel.max()) if rel.size else 0.0, float(back.mean()))
        for name, a, b, k in (("value", val, ev, ~near), ("pdf", pdf, ep, ~near), ("wo", got["wo"], want["wo"], live), ("sample_pdf", got["pdf"], want["pdf"], live),
                              ("weight", got["weight"], want["weight"], live)):
            d = np.abs(a[..., k].astype(np.float64) - b[..., k])
            if d.size:
                worst[name] = max(worst.get(name, 0.0), float(d.max()))
        worst["near"] = max(worst.get("near", 0.0), float(near.mean()), float(want["near"].mean()))
        worst["dropped"] = worst.get("dropped", 0) + int((~act).sum())


@pytest.mark.parametrize("geom_name", U.GEOMETRIES)
@pytest.mark.parametrize("nested", U.NESTED_NAMES)
def test_composition_against_oracle(mi, O, tuples20k, nested, geom_name):
    """eval / pdf / sample of the bumpmap on 20 000 tuples (both sides, grazing directions, |z| >= 0.002), the interactions of one of three geometries, height gradients
    up to a 60 degree tilt from a bilinear bitmap with to_uv, all four switch combinations, every context of the nested model, against bumpmap.cpp:137-253 restated in
    float32 over the oracle's answers for the nested BSDF; the height gradient from the float64 lookup.  Discrete outputs and zero lanes are equal outside the lanes within
    1e-6 of one of the three switches (at most 0.1 %).  Measured maxima: docs/parity.md, "bumpmap"."""
    wi, uv, wo, s1, s2 = tuples20k
    n = wi.shape[1]
    ch = N.Nested(mi, O, nested)
    geom = U.geometry(geom_name, n)
    # (a one-channel map: the float32 luminance of a three-channel one adds three roundings to every texel, and the amplified difference to the float64 lookup then passes
    # the 1e-4 cap for the sharpest lobes -- measured 1.7e-4 on a sample weight of `plastic`, docs/parity.md; three channels are held to the project's bars below)
    tex, m, scale = U.height_case(mi, geom_name, uv, channels=1)
    g = (U.eval_1_grad64(tex, uv, m) * np.float64(F32(scale))).astype(F32)
    assert 0.9 * U.TAN60 <= float(U.tilt_tan(geom, g.astype(np.float64)).max()) <= 1.001 * U.TAN60
    worst = {}
    for flip, shadow in U.SWITCHES:
        bsdf = mi.load_dict(U.bumpmap_dict(mi, nested, U.bitmap_prop(mi, tex, m), scale, flip, shadow)); scene, ib = B.bound(mi, bsdf)

        def evaluate(ctx, wo_override=None):
            return U.host_eval_pdf_si(mi, scene, ib, ctx, wi, uv, wo if wo_override is None else wo_override, geom)

        check_against_restatement(evaluate, lambda ctx: U.host_sample_si(mi, scene, ib, ctx, wi, uv, s1, s2, geom), ch, nested, geom, g, flip, shadow, wi, uv, wo, s1, s2, worst, True)
    assert worst["dropped"] > 5000          # wo lies on both sides of the perturbed horizon
    print("bumpmap composition %s / %s: largest absolute differences %s" % (nested, geom_name, {k: ("%.2e" % v if isinstance(v, float) else v) for k, v in worst.items()}))


@pytest.mark.parametrize("geom_name", U.GEOMETRIES)
@pytest.mark.parametrize("nested", U.NESTED_NAMES + ["roughplastic_015"])
def test_float32_lookup_holds_the_project_bars(mi, O, tuples20k, nested, geom_name):
    """with the height gradient from a float32 lookup in the product's order (U.eval_1_grad32) the project's bars hold -- 2e-6 for pdfs and un-mixed values, 2e-5 for values
    with the shadow term and sample weights -- on a THREE-channel map (its luminance in float32), every geometry, all four switch combinations, every context"""
    wi, uv, wo, s1, s2 = tuples20k
    ch = N.Nested(mi, O, nested)
    geom = U.geometry(geom_name, wi.shape[1])
    tex, m, scale = U.height_case(mi, geom_name, uv, channels=3)
    g = (U.eval_1_grad32(tex, uv, m) * F32(scale)).astype(F32)
    worst = {}
    for flip, shadow in U.SWITCHES:
        bsdf = mi.load_dict(U.bumpmap_dict(mi, nested, U.bitmap_prop(mi, tex, m), scale, flip, shadow)); scene, ib = B.bound(mi, bsdf)

        def evaluate(ctx, wo_override=None):
            return U.host_eval_pdf_si(mi, scene, ib, ctx, wi, uv, wo if wo_override is None else wo_override, geom)

        check_against_restatement(evaluate, lambda ctx: U.host_sample_si(mi, scene, ib, ctx, wi, uv, s1, s2, geom), ch, nested, geom, g, flip, shadow, wi, uv, wo, s1, s2, worst, False)
    print("bumpmap through the float32 lookup, three channels, %s / %s: largest absolute differences %s" % (nested, geom_name, {k: ("%.2e" % v if isinstance(v, float) else v) for k, v in worst.items()}))


def test_outer_twosided_and_masked_lanes(mi, O, tuples20k):
    """twosided(bumpmap(X)): the fold happens in front of the frame -- the host entry on (wi, wo) equals the plain bumpmap on the folded directions, bit for bit; masked
    lanes return zeros"""
    wi, uv, wo, s1, s2 = tuples20k
    geom = U.geometry("smooth_mesh", wi.shape[1])
    tex, m, scale = U.height_case(mi, "smooth_mesh", uv)
    plain = mi.load_dict(U.bumpmap_dict(mi, "roughplastic", U.bitmap_prop(mi, tex, m), scale)); ps, pi = B.bound(mi, plain)
    two = mi.load_dict({"type": "twosided", "x": U.bumpmap_dict(mi, "roughplastic", U.bitmap_prop(mi, tex, m), scale)}); ts, ti = B.bound(mi, two)
    fwi, fwo, neg = N.fold(wi, wo)
    ctx = (0, 0x1ff, ALL)
    a = U.host_eval_pdf_si(mi, ts, ti, ctx, wi, uv, wo, geom); b = U.host_eval_pdf_si(mi, ps, pi, ctx, fwi, uv, fwo, geom)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[0] != 0).any(0)[neg].sum() > 1000
    active = np.arange(wi.shape[1]) % 3 != 0
    v, p = U.host_eval_pdf_si(mi, ps, pi, ctx, wi, uv, wo, geom, active)
    s = U.host_sample_si(mi, ps, pi, ctx, wi, uv, s1, s2, geom, active)
    assert (v[:, ~active] == 0).all() and (p[~active] == 0).all() and (s["weight"][:, ~active] == 0).all() and (s["wo"][:, ~active] == 0).all()


# ------------------------------------------------------------------------------------------------ 4. the per-call derivative

GRAD_BAR = 1e-2          # relative L2 over the kept lanes
GRAD_H = 2e-3            # the step in grad_uv: h against h / 2 differ by less than a third of the bar for every nested model (printed below; docs/parity.md)


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("nested", U.NON_DELTA)
def test_per_call_derivative_against_central_differences(mi, O, nested, shadow):
    """har_bumpmap_grad_host (the reverse sweep of har_bumpmap_grad.h) against central differences in grad_uv of bumpmap.cpp restated in float64, 5 000 tuples on the
    smooth-mesh interactions.  Lanes within 1e-3 of a switch at the centre or at a displaced point are excluded (at most 2 %).  The step: h against h / 2 under a third of the bar."""
    wi, uv, wo, A, geom, g = U.grad_tuples()
    ch = N.Nested(mi, O, nested)
    bsdf = mi.load_dict(U.bumpmap_dict(mi, nested, U.bitmap_prop(mi, U.noise(3, 5, 1, 1)), 1.0, True, shadow)); scene, ib = B.bound(mi, bsdf)
    val, grad = U.host_bump_grad(mi, scene, ib, wi, uv, wo, geom, A, grad_uv=g)
    F0, masks, prods = U.weighted_value64(ch, geom, g, wi, uv, wo, A, True, shadow)
    # (both sides evaluate the same function: the product's frame is float32, the restatement's float64, and a rough lobe amplifies an ulp of the frame by about 1 / alpha^2)
    assert np.allclose(val, F0, rtol=1e-3, atol=1e-5)

    def central(h):
        out = np.zeros((2, g.shape[1])); near = np.zeros(g.shape[1], bool)
        for k in range(2):
            e = np.zeros((2, 1)); e[k] = h
            fp, _, pp = U.weighted_value64(ch, geom, g.astype(np.float64) + e, wi, uv, wo, A, True, shadow, masks)
            fm, _, pm = U.weighted_value64(ch, geom, g.astype(np.float64) - e, wi, uv, wo, A, True, shadow, masks)
            out[k] = (fp - fm) / (2 * h)
            for pr in pp + pm:
                near |= np.abs(pr) <= 1e-3
        return out, near

    fd, near = central(GRAD_H); fd2, near2 = central(GRAD_H / 2)
    for pr in prods:
        near |= np.abs(pr) <= 1e-3
    near |= near2
    keep = ~near
    assert near.mean() <= 0.02, float(near.mean())
    norm = np.linalg.norm(fd[:, keep])
    step = float(np.linalg.norm(fd[:, keep] - fd2[:, keep]) / norm)
    err = float(np.linalg.norm(grad[:, keep] - fd[:, keep]) / norm)
    print("bumpmap dF/dgrad_uv %s, shadow %s: relative L2 %.3g (bar %.3g); h = %g against h / 2: %.3g; %.2f %% of the lanes excluded, %d lanes with a derivative"
          % (nested, shadow, err, GRAD_BAR, GRAD_H, step, 100 * near.mean(), int((np.abs(fd[:, keep]).sum(0) > 0).sum())))
    assert norm > 0 and step < GRAD_BAR / 3 and err <= GRAD_BAR


def test_per_call_derivative_of_delta_models_is_zero(mi):
    wi, uv, wo, A, geom, g = U.grad_tuples(1000)
    for nested in ("dielectric", {"type": "conductor"}):
        bsdf = mi.load_dict(U.bumpmap_dict(mi, nested, U.bitmap_prop(mi, U.noise(3, 5, 1, 1)))); scene, ib = B.bound(mi, bsdf)
        val, grad = U.host_bump_grad(mi, scene, ib, wi, uv, wo, geom, A, grad_uv=g)
        assert (val == 0).all() and (grad == 0).all()


# ------------------------------------------------------------------------------------------------ 5. renders on the host path

def _pair(mi, O, a, b, seed=3, md=4, rr=8):
    from tests.test_cpu_host import rel_l2
    fa, sa = B.host_render_stats(mi, mi.load_dict(a), seed, SPP, md, rr); fb, sb = B.host_render_stats(mi, mi.load_dict(b), seed, SPP, md, rr)
    assert np.isfinite(fa).all() and np.linalg.norm(fb[..., :3]) > 0
    return rel_l2(O.develop(fa), O.develop(fb)), (sa.paths, sa.vertices), (sb.paths, sb.vertices)


@pytest.mark.parametrize("nested", ["diffuse", "roughplastic", "roughconductor_ggx", "dielectric"])
def test_host_render_zero_height_is_the_nested_bsdf(mi, O, nested):
    """a zero height map on a flat-shaded mesh equals the nested BSDF's scene at 1e-6, with equal path and vertex counters"""
    zero = U.bitmap_prop(mi, np.zeros((4, 4, 1), F32))
    a = N.lit_scene(mi, U.bumpmap_dict(mi, nested, zero), "mesh", RES, SPP, max_depth=4, area_light=True)
    b = N.lit_scene(mi, N.nested_dict(nested), "mesh", RES, SPP, max_depth=4, area_light=True)
    err, got, want = _pair(mi, O, a, b)
    print("host render, zero height over %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (nested, err, got, want))
    assert err <= 1e-6 and got == want and got[1] > got[0]


@pytest.mark.parametrize("nested", ["diffuse", "roughplastic"])
def test_host_render_plane_height_is_a_constant_normal_map(mi, O, nested):
    """a plane height a u + b v on an untransformed +z rectangle equals the `normalmap` scene with the constant colour 0.5 + 0.5 normalize(-2a, -2b, 4), at 1e-4 (to_uv scale
    0.5, offset 0.25, clamp: no lookup reaches the border); measured 9.2e-8 (docs/parity.md)"""
    a_, b_ = 0.3, -0.2
    h, m = U.plane_height(a_, b_)
    bump = U.unit_rectangle_scene(mi, U.bumpmap_dict(mi, nested, U.bitmap_prop(mi, h, m, "clamp")), RES, SPP)
    nmap = U.unit_rectangle_scene(mi, {"type": "normalmap", "normalmap": {"type": "rgb", "value": U.plane_normal_colour(a_, b_)}, "inner": N.nested_dict(nested)}, RES, SPP)
    flat = U.unit_rectangle_scene(mi, N.nested_dict(nested), RES, SPP)
    err, got, want = _pair(mi, O, bump, nmap)
    apart, _, _ = _pair(mi, O, bump, flat)
    print("host render, plane height over %s against the constant normal map: rel L2 %.3g, (paths, vertices) %s vs %s; %.3g away from the flat scene" % (nested, err, got, want, apart))
    assert err <= 1e-4 and got == want and apart > 1e-3


def test_aov_sh_normal_and_albedo_host(mi):
    """aov on the host twin: sh_normal = si.to_world(frame.n) -- the plane height gives the constant normal of the equivalent normal map --, plain si.sh_frame.n under an outer
    twosided; the albedo is the nested BSDF's"""
    from tests.test_normalmap_cpu import aov_rays
    a_, b_ = 0.3, -0.2
    h, m = U.plane_height(a_, b_)
    bs = U.bumpmap_dict(mi, "roughplastic", U.bitmap_prop(mi, h, m, "clamp"))
    o, d, maxt = aov_rays(4096)
    integ = mi.load_dict({"type": "aov", "aovs": "nn:sh_normal,aa:albedo,pp:position"})
    got = integ.sample_host(mi.load_dict(U.unit_rectangle_scene(mi, bs)), o, d, maxt)
    card = (np.abs(got[8]) < 1e-5) & (np.abs(got[6:8]).max(0) < 0.999) & (got[0:3] != 0).any(0) & (d[2] < 0)          # hits on the card's upper side
    n = np.array([-2 * a_, -2 * b_, 4.0]); n /= np.linalg.norm(n)
    assert card.sum() > 500 and np.allclose(got[0:3][:, card], n[:, None], atol=2e-6)
    assert np.allclose(got[3:6][:, card], np.array(N.NESTED["roughplastic"]["diffuse_reflectance"]["value"], F32)[:, None])
    two = integ.sample_host(mi.load_dict(U.unit_rectangle_scene(mi, {"type": "twosided", "x": bs})), o, d, maxt)
    assert np.allclose(two[0:3][:, card], np.array([[0.0], [0.0], [1.0]]), atol=1e-6)


def test_a_mesh_under_a_bumpmap_reports_todays_interaction_rows(mi):
    """a bumpmap changes nothing about the shading frame of a shape: the 33 rows of compute_surface_interaction of a smooth mesh and of a cube under a bumpmap equal the rows
    of the same shapes under the nested BSDF, bit for bit"""
    from tests.test_normalmap_cpu import _hits_on
    bs = U.bump_bsdf(mi)
    for shape in (U.smooth_mesh(), {"type": "cube"}):
        a = mi.load_dict({"type": "scene", "s": dict(shape, bsdf=bs)}); b = mi.load_dict({"type": "scene", "s": dict(shape, bsdf=N.nested_dict("roughplastic"))})
        hits = _hits_on(mi, b, 0, 0xffffffff)
        assert np.array_equal(N.host_si(mi, a, *hits), N.host_si(mi, b, *hits))


# ------------------------------------------------------------------------------------------------ 6. parameters

def test_params_update_gives_the_scene_a_fresh_load_gives(mi, O):
    """in-place params.update() of the height texels, `scale` and a nested colour gives the scene a fresh load gives (host render, equal bits)"""
    import torch
    d = U.lit_scene(mi, U.bump_bsdf(mi, "roughplastic", seed=5), "smooth_mesh", RES, SPP, max_depth=3)
    scene = mi.load_dict(d)
    p = mi.traverse(scene)
    new_tex = U.bumpy_height(6, 8, 1, seed=9)
    p["mat.nested_texture.data"] = torch.tensor(new_tex); p["mat.scale"] = torch.tensor([1.7]); p["mat.nested_bsdf.diffuse_reflectance.value"] = torch.tensor([0.2, 0.6, 0.3])
    p.update()
    m = np.eye(3); m[:2, :] = N.TO_UV
    nested = N.nested_dict("roughplastic"); nested["diffuse_reflectance"] = {"type": "rgb", "value": [0.2, 0.6, 0.3]}
    fresh = mi.load_dict(U.lit_scene(mi, U.bumpmap_dict(mi, nested, U.bitmap_prop(mi, new_tex, m), 1.7), "smooth_mesh", RES, SPP, max_depth=3))
    fa, sa = B.host_render_stats(mi, scene, 3, SPP, 3, 8); fb, sb = B.host_render_stats(mi, fresh, 3, SPP, 3, 8)
    before, _ = B.host_render_stats(mi, mi.load_dict(d), 3, SPP, 3, 8)
    assert np.array_equal(fa, fb) and (sa.paths, sa.vertices) == (sb.paths, sb.vertices) and not np.array_equal(fa, before)
    with pytest.raises(RuntimeError, match="mat.nested_texture.data.*shape"):
        p["mat.nested_texture.data"] = torch.zeros((6, 8, 3)); p.update()
