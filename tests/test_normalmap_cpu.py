"""`normalmap` on the CPU, through the library's host entries (har_bsdf_eval_pdf_host / har_bsdf_sample_host / har_surface_interaction_host / har_aov_sample_host /
har_render_lanes_stats_host run the HAR_HD code the kernels run): the record and the loader, normalmap.cpp restated in NumPy over the oracle's answers for the nested BSDF
alone, the reference's own four tests, the shading frames of rectangles against the reference's rule in float64, the aov shading normal, and host renders -- the identity
map against the nested BSDF alone, and a film composed on the CPU from oracle calls and the restated eval."""
import ctypes as C

import numpy as np
import pytest

from tests import aov_cases as A
from tests import blend_cases as B
from tests import mask_cases as M
from tests import normalmap_cases as N

ALL = N.ALL
F32 = np.float32
LEAF = dict(rtol=2e-6, atol=1e-9)          # the project's bars: the leaf models against the oracle, pdfs and un-mixed values
MIXED = dict(rtol=2e-5, atol=1e-7)         # ... composed values (value * shadow term) and sample weights
FRAME = dict(rtol=3e-6, atol=3e-7)         # the `aov` / `thinlens` bars


# ------------------------------------------------------------------------------------------------ 1. the record and the loader

def test_components_flags_and_keys(mi):
    F = mi.BSDFFlags
    b = mi.load_dict({"type": "normalmap", "normalmap": {"type": "rgb", "value": [0.5, 0.5, 1.0]}, "nested_bsdf": {"type": "roughplastic"}})
    assert b.component_count() == 2 and b.flags(0) == F.GlossyReflection | F.FrontSide and b.flags(1) == F.DiffuseReflection | F.FrontSide and (b.flags() & F.Smooth)
    assert int(b.flags) & 64 and int(b.flags) & 128                    # flip_invalid_normals and use_shadowing_function default to true (normalmap.cpp:114-115)
    b = mi.load_dict({"type": "normalmap", "normalmap": {"type": "rgb", "value": [0.5, 0.5, 1.0]}, "x": {"type": "conductor"}, "flip_invalid_normals": False, "use_shadowing_function": False})
    assert b.component_count() == 1 and not (b.flags() & F.Smooth) and not (int(b.flags) & (64 | 128))
    tex = N.bumpy_texels()
    sc = mi.load_dict({"type": "scene", "bumpy": {"type": "normalmap", "normalmap": {"type": "bitmap", "data": tex, "raw": True}, "inner": {"type": "twosided", "a": {"type": "diffuse"}, "b": {"type": "plastic"}}},
                       "flat": {"type": "twosided", "n": {"type": "normalmap", "normalmap": {"type": "rgb", "value": [0.5, 0.5, 1.0]}, "inner": {"type": "diffuse"}}},
                       "r": {"type": "rectangle", "bsdf": {"type": "ref", "id": "bumpy"}}, "q": {"type": "rectangle", "bsdf": {"type": "ref", "id": "flat"}}})
    keys = set(mi.traverse(sc).keys())
    want = {"bumpy.normalmap.data", "bumpy.nested_bsdf.brdf_0.reflectance.value", "bumpy.nested_bsdf.brdf_1.diffuse_reflectance.value",
            "flat.brdf_0.normalmap.value", "flat.brdf_0.nested_bsdf.reflectance.value"}
    assert want <= keys, sorted(want - keys)
    assert tuple(mi.traverse(sc)["bumpy.normalmap.data"].shape) == tex.shape


def test_loader_messages(mi):
    nm = {"type": "rgb", "value": [0.5, 0.5, 1.0]}
    with pytest.raises(RuntimeError, match="Exactly one BSDF child object must be specified."):
        mi.load_dict({"type": "normalmap", "normalmap": nm})
    with pytest.raises(RuntimeError, match="Only a single BSDF child object can be specified."):
        mi.load_dict({"type": "normalmap", "normalmap": nm, "a": {"type": "diffuse"}, "b": {"type": "diffuse"}})
    with pytest.raises(RuntimeError, match='"normalmap" has not been specified'):
        mi.load_dict({"type": "normalmap", "a": {"type": "diffuse"}})
    with pytest.raises(RuntimeError, match="(?i)unreferenced property \"strength\""):
        mi.load_dict({"type": "normalmap", "normalmap": nm, "a": {"type": "diffuse"}, "strength": 2.0})
    with pytest.raises(RuntimeError, match="normalmap.*1 channel"):
        mi.load_dict({"type": "normalmap", "normalmap": {"type": "bitmap", "data": np.full((4, 4, 1), 0.5, np.float32), "raw": True}, "a": {"type": "diffuse"}})
    inner_nm = {"type": "normalmap", "normalmap": nm, "a": {"type": "diffuse"}}
    for kind, inner in (("blendbsdf", {"type": "blendbsdf", "weight": 0.5, "a": {"type": "diffuse"}, "b": {"type": "diffuse"}}),
                        ("mask", {"type": "mask", "opacity": 0.5, "a": {"type": "diffuse"}}), ("normalmap", inner_nm)):
        with pytest.raises(RuntimeError, match="normalmap: a nested `%s`" % kind):
            mi.load_dict({"type": "normalmap", "normalmap": nm, "x": inner})
    with pytest.raises(RuntimeError, match="blendbsdf: a nested `normalmap`"):
        mi.load_dict({"type": "blendbsdf", "weight": 0.5, "a": dict(inner_nm), "b": {"type": "diffuse"}})
    with pytest.raises(RuntimeError, match="mask: a nested `normalmap`"):
        mi.load_dict({"type": "mask", "opacity": 0.5, "a": dict(inner_nm)})
    with pytest.raises(RuntimeError, match="twosided.*normalmap"):          # the two-BSDF form over a normalmap: refused by name (docs/widening.md)
        mi.load_dict({"type": "twosided", "a": dict(inner_nm), "b": {"type": "diffuse"}})
    with pytest.raises(RuntimeError, match="transmission"):                  # twosided.cpp:79-83 sees the nested BSDF's lobes
        mi.load_dict({"type": "twosided", "a": {"type": "normalmap", "normalmap": nm, "x": {"type": "dielectric"}}})


def test_xml_loader(mi, tmp_path):
    """<bsdf type="normalmap"><texture name="normalmap" .../><bsdf .../></bsdf>, with a bitmap file and with an rgb colour"""
    tex = N.bumpy_texels(4, 3)
    pfm = tmp_path / "bumps.pfm"
    with open(pfm, "wb") as f:
        f.write(b"PF\n3 4\n-1.0\n"); f.write(np.ascontiguousarray(tex[::-1], "<f4").tobytes())
    xml = tmp_path / "nm.xml"
    xml.write_text('<scene version="3.0.0"><bsdf type="normalmap" id="bumpy"><texture name="normalmap" type="bitmap"><string name="filename" value="bumps.pfm"/>'
                   '<boolean name="raw" value="true"/></texture><boolean name="use_shadowing_function" value="false"/><bsdf type="diffuse"/></bsdf>'
                   '<bsdf type="normalmap" id="flat"><rgb name="normalmap" value="0.75, 0.5, 0.933"/><bsdf type="plastic"/></bsdf>'
                   '<shape type="rectangle"><ref id="bumpy"/></shape><shape type="rectangle"><ref id="flat"/></shape></scene>')
    sc = mi.load_file(str(xml))
    b = sc.bsdfs[sc.meshes[0]["bsdf"]]
    assert b.kind == "normalmap" and np.array_equal(b.texture, tex) and (int(b.flags) & 64) and not (int(b.flags) & 128) and b.nested[0].kind == "diffuse"
    b = sc.bsdfs[sc.meshes[1]["bsdf"]]
    assert b.kind == "normalmap" and np.allclose(b.value, [0.75, 0.5, 0.933]) and (int(b.flags) & 192) == 192 and b.nested[0].kind == "plastic"


def test_meshes_with_normals_and_texcoords_are_refused_by_name(mi):
    """case 3: such a mesh packs per-vertex tangents in the reference; a cube has both.  Meshes without normals (case 1) and rectangles (case 2) load."""
    nm = {"type": "normalmap", "normalmap": {"type": "rgb", "value": [0.6, 0.5, 0.9]}, "x": {"type": "diffuse"}}
    with pytest.raises(RuntimeError, match='normalmap: shape "crate".*per-vertex tangents'):
        mi.load_dict({"type": "scene", "crate": {"type": "cube", "bsdf": dict(nm)}})
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    with pytest.raises(RuntimeError, match='normalmap: shape "tri".*per-vertex tangents'):
        mi.load_dict({"type": "scene", "tri": {"type": "mesh", "positions": P, "faces": np.array([[0, 1, 2]], np.uint32), "normals": np.tile([0, 0, 1], (3, 1)).astype(np.float32),
                                               "texcoords": P[:, :2].copy(), "bsdf": dict(nm)}})
    mi.load_dict({"type": "scene", "flat": dict(N.flat_mesh(), bsdf=dict(nm)), "r": {"type": "rectangle", "bsdf": dict(nm)}}).desc()


# ------------------------------------------------------------------------------------------------ 2. per call, against normalmap.cpp restated over the oracle

# The bitmap map: the product interpolates the texel in float32 as the texture unit does, the restatement in float64; an ulp of the colour (6e-8) is an ulp of wi' and
# wo', which a rough lobe amplifies by about 1 / alpha^2 (the reference's own test says so).  That exceeds the project's bars (2e-6 / 2e-5 relative), so the bars
# are four times the largest difference measured over all nested models, switches and contexts (docs/parity.md, "normalmap"), and never above
# the tolerances of the reference's test02 (wo 1e-4, pdf 1e-4, weight 2e-4 absolute).  The constant maps are held to the project's bars (measured: equal bits).
BITMAP_ATOL = dict(value=4.6e-5, pdf=4.6e-5, wo=2.3e-5, sample_pdf=1.0e-4, weight=6.7e-5)
_COLOUR = {}


def _colour(nmap, uv):
    if nmap not in _COLOUR:
        _COLOUR[nmap] = N.map_colour(nmap, uv)
    return _COLOUR[nmap]


def check_against_restatement(evaluate, sample, ch, nested, nmap, flip, shadow, wi, uv, wo, s1, s2, c, worst):
    """one (nested, map, switches) case over all contexts: `evaluate(ctx) -> (value, pdf)` and `sample(ctx) -> dict` are the side under test (host entries or device)"""
    n = wi.shape[1]
    bitmap = nmap == "bitmap_bilinear_to_uv"
    for ctx in N.contexts(nested):
        val, pdf = evaluate(ctx)
        ev, ep, act, near = N.expected_eval_pdf(ch, ctx, c, wi, uv, wo, flip, shadow)
        assert np.isfinite(val).all() and np.isfinite(pdf).all()
        assert near.mean() <= 1e-3, ("lanes within 1e-6 of a switch", float(near.mean()))          # the cap, on the restatement alone
        keep = ~near
        # no lane left out: which lanes are zero is equal
        assert np.array_equal((val != 0).any(0)[keep], (ev != 0).any(0)[keep]) and np.array_equal((pdf != 0)[keep], (ep != 0)[keep]), (nested, nmap, flip, shadow, ctx, "zero lanes")
        vbar = dict(rtol=0, atol=BITMAP_ATOL["value"]) if bitmap else (MIXED if shadow else LEAF)
        pbar = dict(rtol=0, atol=BITMAP_ATOL["pdf"]) if bitmap else LEAF
        assert np.allclose(val[:, keep], ev[:, keep], **vbar), (nested, nmap, flip, shadow, ctx, "value", float(np.abs(val[:, keep] - ev[:, keep]).max()))
        assert np.allclose(pdf[keep], ep[keep], **pbar), (nested, nmap, flip, shadow, ctx, "pdf", float(np.abs(pdf[keep] - ep[keep]).max()))
        got = sample(ctx)
        want = N.expected_sample(ch, ctx, c, wi, uv, s1, s2, flip, shadow)
        assert want["near"].mean() <= 1e-3
        keep = ~want["near"]
        for key in ("sampled_type", "sampled_component", "eta"):
            assert np.array_equal(got[key][keep], want[key][keep]), (nested, nmap, flip, shadow, ctx, key, int((got[key][keep] != want[key][keep]).sum()))
        zg = ~(got["weight"] != 0).any(0); zw = ~(want["weight"] != 0).any(0)
        assert np.array_equal(zg[keep], zw[keep]) and np.array_equal((got["pdf"] != 0)[keep], (want["pdf"] != 0)[keep]), (nested, nmap, flip, shadow, ctx, "zero samples")
        live = keep & ~zw
        bars = {k: dict(rtol=0, atol=BITMAP_ATOL[b]) if bitmap else std for k, b, std in (("wo", "wo", dict(rtol=2e-6, atol=1e-7)), ("pdf", "sample_pdf", LEAF), ("weight", "weight", MIXED if shadow else LEAF))}
        for key in ("wo", "pdf", "weight"):
            a, b = got[key][..., live], want[key][..., live]
            assert np.allclose(a, b, **bars[key]), (nested, nmap, flip, shadow, ctx, "sample " + key, float(np.abs(a - b).max()))
        # consistency: weight * pdf == eval at the sampled direction for valid non-delta samples, the shadow term on both sides
        nd = live & ((got["sampled_type"] & 0x60) == 0) & (got["pdf"] > 0)          # (0x60: the delta lobes)
        if nd.any() and ctx[2] == ALL and ctx[1] == 0x1ff:
            v2, p2 = evaluate(ctx, wo_override=got["wo"])
            lhs = (got["weight"] * got["pdf"][None, :])[:, nd]; rhs = v2[:, nd]
            # the sampled wo went through to_world and comes back through to_local: an ulp of wo' on a lobe of width alpha, as above; directions that came back across the
            # perturbed horizon evaluate to zero and are counted, not compared
            back = (rhs != 0).any(0)
            worst["consistency_lost"] = max(worst.get("consistency_lost", 0.0), float(1.0 - back.mean()))
            rel = np.abs(lhs[:, back] - rhs[:, back]) / np.maximum(np.abs(rhs[:, back]), 1e-3)
            worst["consistency"] = max(worst.get("consistency", 0.0), float(rel.max()) if rel.size else 0.0)
            # bar: four times the largest difference measured (2.55e-4, GGX alpha 0.1 under the 30 degree tilt; docs/parity.md) -- two ulps of wo' times 1 / alpha^2 and the lobe's slope
            assert back.mean() > 0.999 and (not rel.size or rel.max() <= 1e-3), (nested, nmap, flip, shadow, "weight * pdf == eval", float(rel.max()) if rel.size else 0.0, float(back.mean()))
            assert np.allclose(p2[nd][back], got["pdf"][nd][back], rtol=2e-3, atol=1e-5)
        for name, a, b, k in (("value", val, ev, ~near), ("pdf", pdf, ep, ~near), ("sample wo", got["wo"], want["wo"], live), ("sample pdf", got["pdf"], want["pdf"], live),
                              ("sample weight", got["weight"], want["weight"], live)):
            d = np.abs(a[..., k].astype(np.float64) - b[..., k])
            if d.size:
                worst[name] = max(worst.get(name, 0.0), float(d.max()))
        worst["near"] = max(worst.get("near", 0.0), float(near.mean()), float(want["near"].mean()))
        worst["flipped"] = worst.get("flipped", 0) + (int((wi[2] * (wi * (2 * c - 1)).sum(0) <= 0).sum()) if flip else 0)
        worst["dropped"] = worst.get("dropped", 0) + int((~act).sum())


@pytest.fixture(scope="module")
def tuples20k():
    return N.tuples()


@pytest.mark.parametrize("nmap", N.MAP_NAMES)
@pytest.mark.parametrize("nested", N.NESTED_NAMES)
def test_composition_against_oracle(mi, O, tuples20k, nested, nmap):
    """eval / pdf / sample of the normalmap on 20 000 tuples (both sides, grazing directions, wo on either side of the perturbed horizon, wi with and without the flip,
    sample1 edge values), all four combinations of the two switches, every context of the nested model, against normalmap.cpp restated in float32 over the oracle's
    answers for the nested BSDF; the texel from an independent float64 lookup.  Every lane is compared; discrete outputs must be equal outside the lanes within 1e-6 of
    a switch (at most 0.1 %).  Measured maxima: docs/parity.md, "normalmap"."""
    wi, uv, wo, s1, s2 = tuples20k
    ch = N.Nested(mi, O, nested)
    c = _colour(nmap, uv)
    worst = {}
    for flip, shadow in N.SWITCHES:
        bsdf = mi.load_dict(N.normalmap_dict(mi, nested, nmap, flip, shadow)); scene, ib = B.bound(mi, bsdf)

        def evaluate(ctx, wo_override=None):
            return B.host_eval_pdf(mi, scene, ib, ctx, wi, uv, wo if wo_override is None else wo_override)

        check_against_restatement(evaluate, lambda ctx: B.host_sample(mi, scene, ib, ctx, wi, uv, s1, s2), ch, nested, nmap, flip, shadow, wi, uv, wo, s1, s2, c, worst)
    if nmap != "identity":
        assert worst["flipped"] > 500 and worst["dropped"] > 5000          # the flip triggers, and wo lies on both sides of the perturbed horizon
    print("normalmap composition %s / %s: largest absolute differences %s" % (nested, nmap, {k: ("%.2e" % v if isinstance(v, float) else v) for k, v in worst.items()}))


@pytest.mark.parametrize("nested", N.NESTED_NAMES + ["roughplastic_015"])
def test_bitmap_map_with_a_float32_lookup_holds_the_project_bars(mi, O, tuples20k, nested):
    """The bars of the bitmap map above are wide because the restatement's texel is interpolated in float64.  With the texel interpolated in float32 as the product does
    (N.lookup_colour32) that cause is gone: the same comparison on the same tuples, default switches, default context, at the project's bars -- 2e-6 for pdfs, 2e-5 for
    values with the shadow term and sample weights -- for every nested model and for the alpha = 0.15 coating that the float64 lookup could not hold"""
    wi, uv, wo, s1, s2 = tuples20k
    ch = N.Nested(mi, O, nested)
    c = N.lookup_colour32(N._bitmap(), uv, N.TO_UV)
    bsdf = mi.load_dict(N.normalmap_dict(mi, nested, "bitmap_bilinear_to_uv")); scene, ib = B.bound(mi, bsdf)
    ctx = (0, 0x1ff, ALL)
    val, pdf = B.host_eval_pdf(mi, scene, ib, ctx, wi, uv, wo)
    ev, ep, act, near = N.expected_eval_pdf(ch, ctx, c, wi, uv, wo, True, True)
    keep = ~near
    assert near.mean() <= 1e-3 and np.array_equal((val != 0).any(0)[keep], (ev != 0).any(0)[keep])
    assert np.allclose(val[:, keep], ev[:, keep], **MIXED) and np.allclose(pdf[keep], ep[keep], **LEAF), (float(np.abs(val[:, keep] - ev[:, keep]).max()), float(np.abs(pdf[keep] - ep[keep]).max()))
    got = B.host_sample(mi, scene, ib, ctx, wi, uv, s1, s2)
    want = N.expected_sample(ch, ctx, c, wi, uv, s1, s2, True, True)
    keep = ~want["near"]
    for key in ("sampled_type", "sampled_component", "eta"):
        assert np.array_equal(got[key][keep], want[key][keep]), key
    live = keep & (want["weight"] != 0).any(0)
    assert np.array_equal((got["weight"] != 0).any(0)[keep], (want["weight"] != 0).any(0)[keep])
    assert np.allclose(got["wo"][:, live], want["wo"][:, live], rtol=2e-6, atol=1e-7) and np.allclose(got["pdf"][live], want["pdf"][live], **LEAF)
    assert np.allclose(got["weight"][:, live], want["weight"][:, live], **MIXED)
    same = float((N.map_colour("bitmap_bilinear_to_uv", uv) == c).all(0).mean()) if nested == "diffuse" else None
    print("normalmap, bitmap map through the float32 lookup, %s: largest differences value %.2e, pdf %.2e, sample pdf %.2e, sample weight %.2e%s"
          % (nested, np.abs(val[:, keep & ~near] - ev[:, keep & ~near]).max(), np.abs(pdf[~near] - ep[~near]).max(), np.abs(got["pdf"][live] - want["pdf"][live]).max(),
             np.abs(got["weight"][:, live] - want["weight"][:, live]).max(), "" if same is None else "; colours equal to the float64 lookup's on %.1f %% of the tuples" % (100 * same)))


@pytest.mark.parametrize("nested", N.NESTED_NAMES)
def test_identity_map_is_the_nested_bsdf_bit_for_bit(mi, tuples20k, nested):
    """(0.5, 0.5, 1) gives n_raw = (0, 0, 1) exactly: the frame is the identity and the shadow term 1 -- every output equals the nested BSDF's, bit for bit, whatever
    the switches.  (-0 == +0: a perturbed component that is exactly zero may carry the other sign.)"""
    wi, uv, wo, s1, s2 = tuples20k
    plain = mi.load_dict(N.nested_dict(nested)); pscene, pi = B.bound(mi, plain)
    for flip, shadow in N.SWITCHES:
        bsdf = mi.load_dict(N.normalmap_dict(mi, nested, "identity", flip, shadow)); scene, ib = B.bound(mi, bsdf)
        for ctx in N.contexts(nested):
            a = B.host_eval_pdf(mi, scene, ib, ctx, wi, uv, wo); b = B.host_eval_pdf(mi, pscene, pi, ctx, wi, uv, wo)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (nested, flip, shadow, ctx)
            a = B.host_sample(mi, scene, ib, ctx, wi, uv, s1, s2); b = B.host_sample(mi, pscene, pi, ctx, wi, uv, s1, s2)
            ok = (b["weight"] != 0).any(0) & (b["wo"][2] != 0)          # (a sample the nested BSDF itself gives weight 0, or a wo in the plane: the orientation test drops it)
            for key in ("wo", "pdf", "weight"):
                assert np.array_equal(a[key][..., ok], b[key][..., ok]), (nested, flip, shadow, ctx, key)
            for key in ("eta", "sampled_type", "sampled_component"):
                assert np.array_equal(a[key], b[key]), (nested, flip, shadow, ctx, key)
            assert ok.mean() > 0.2 or nested == "dielectric" or ctx != (0, 0x1ff, ALL)


def test_outer_twosided(mi, O, tuples20k):
    """twosided(normalmap(X)), the idiom of scene files: the one-BSDF fold of twosided.cpp (wi.z = |wi.z|, wo.z = mulsign(wo.z, wi.z)) in front of the restatement"""
    wi, uv, wo, s1, s2 = tuples20k
    ch = N.Nested(mi, O, "roughplastic")
    bsdf = mi.load_dict({"type": "twosided", "x": N.normalmap_dict(mi, "roughplastic", "tilt30")}); scene, ib = B.bound(mi, bsdf)
    c = N.map_colour("tilt30", uv)
    wif, wof, neg = N.fold(wi, wo)
    ctx = (0, 0x1ff, ALL)
    val, pdf = B.host_eval_pdf(mi, scene, ib, ctx, wi, uv, wo)
    ev, ep, act, near = N.expected_eval_pdf(ch, ctx, c, wif, uv, wof, True, True)
    assert np.array_equal((val != 0).any(0)[~near], (ev != 0).any(0)[~near]) and (val != 0).any(0)[neg].any()
    assert np.allclose(val[:, ~near], ev[:, ~near], **MIXED) and np.allclose(pdf[~near], ep[~near], **LEAF)
    got = B.host_sample(mi, scene, ib, ctx, wi, uv, s1, s2)
    want = N.expected_sample(ch, ctx, c, wif, uv, s1, s2, True, True)
    want["wo"][2] = np.where(neg, -want["wo"][2], want["wo"][2])
    keep = ~want["near"] & (want["weight"] != 0).any(0)
    assert np.allclose(got["wo"][:, keep], want["wo"][:, keep], rtol=2e-6, atol=1e-7) and np.allclose(got["pdf"][keep], want["pdf"][keep], **LEAF)
    assert np.allclose(got["weight"][:, keep], want["weight"][:, keep], **MIXED)


def test_masked_lanes(mi):
    bsdf = mi.load_dict(N.normalmap_dict(mi, "plastic", "tilt30")); scene, ib = B.bound(mi, bsdf)
    wi, uv, wo, s1, s2 = N.tuples(n=512)
    active = (np.arange(512) % 3 != 0)
    val, pdf = B.host_eval_pdf(mi, scene, ib, (0, 0x1ff, ALL), wi, uv, wo, active)
    v0, p0 = B.host_eval_pdf(mi, scene, ib, None, wi, uv, wo)
    assert (val[:, ~active] == 0).all() and (pdf[~active] == 0).all() and np.array_equal(val[:, active], v0[:, active]) and np.array_equal(pdf[active], p0[active])
    bs = B.host_sample(mi, scene, ib, (0, 0x1ff, ALL), wi, uv, s1, s2, active)
    assert (bs["weight"][:, ~active] == 0).all() and (bs["wo"][:, ~active] == 0).all() and (bs["sampled_type"][~active] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. the reference's own tests (src/bsdfs/tests/test_normalmap.py)

AL = dict(eta=[1.657, 0.880, 0.521], k=[9.224, 6.270, 4.837])          # (`material: Al` needs the spectral data files: an rgb (eta, k) of aluminium instead)


def _sampler_numbers(O, n=1024, seed=0):
    """sample1 (n), sample2 (2 x n) from this project's sampler: the first three floats of lanes 0 .. n - 1 of Sampler::seed(seed, n)"""
    state, inc = M.lane_seeds(O, seed, n)
    d = np.stack([M.stream_draws(O, state[i], inc[i], 3)[0] for i in range(n)], 1)
    return np.ascontiguousarray(d[0]), np.ascontiguousarray(d[1:3])


def test01_empty(mi, O):
    raw = mi.load_dict(dict(type="roughconductor", distribution="ggx", alpha_u=0.4, alpha_v=0.1, **AL)); rs, ri = B.bound(mi, raw)
    nm = mi.load_dict({"type": "normalmap", "normalmap": {"type": "rgb", "value": [0.5, 0.5, 1.0]}, "nested_bsdf": dict(type="roughconductor", distribution="ggx", alpha_u=0.4, alpha_v=0.1, **AL)})
    ns, ni = B.bound(mi, nm)
    s1, s2 = _sampler_numbers(O)
    n = s1.size
    wi = np.repeat(np.array([[0.0], [0.0], [1.0]], F32), n, 1); uv = np.zeros((2, n), F32)
    ref = B.host_sample(mi, rs, ri, None, wi, uv, s1, s2); test = B.host_sample(mi, ns, ni, None, wi, uv, s1, s2)
    mask = (ref["weight"] == 0).all(0)
    for r in (ref, test):
        r["wo"][:, mask] = 0; r["pdf"][mask] = 0
    assert np.allclose(ref["wo"], test["wo"], atol=1e-3) and np.allclose(ref["pdf"], test["pdf"], atol=1e-4) and np.allclose(ref["weight"], test["weight"], atol=1e-2)
    assert (~mask).sum() > 500


def test02_tilted(mi, O):
    sin_t, cos_t = 0.5, 0.5 * np.sqrt(3.0)
    s = np.array([cos_t, 0, -sin_t]); t = np.array([0.0, 1, 0]); nrm = np.array([sin_t, 0, cos_t])
    spec = dict(type="roughconductor", distribution="ggx", alpha_u=0.2, alpha_v=0.05, **AL)
    raw = mi.load_dict(dict(spec)); rs, ri = B.bound(mi, raw)
    nm = mi.load_dict({"type": "normalmap", "normalmap": {"type": "rgb", "value": [float(x) for x in nrm * 0.5 + 0.5]}, "nested_bsdf": dict(spec), "use_shadowing_function": False})
    ns, ni = B.bound(mi, nm)
    s1, s2 = _sampler_numbers(O)
    n = s1.size
    wi = np.repeat(np.array([[0.0], [0.0], [1.0]], F32), n, 1); uv = np.zeros((2, n), F32)
    wi_p = np.repeat(np.array([[s[2]], [t[2]], [nrm[2]]], F32), n, 1)          # normal_frame.to_local((0, 0, 1))
    r = B.host_sample(mi, rs, ri, None, wi_p, uv, s1, s2); test = B.host_sample(mi, ns, ni, None, wi, uv, s1, s2)
    wo_raw = (s[:, None] * r["wo"][0] + t[:, None] * r["wo"][1] + nrm[:, None] * r["wo"][2]).astype(F32)          # normal_frame.to_world
    bad = wo_raw[2] * r["wo"][2] <= 0
    r["pdf"][bad] = 0; r["weight"][:, bad] = 0
    wo_test = test["wo"].copy()
    wo_raw[:, (r["weight"] == 0).all(0)] = 0; wo_test[:, (test["weight"] == 0).all(0)] = 0
    r["pdf"][(r["weight"] == 0).all(0)] = 0; test["pdf"][(test["weight"] == 0).all(0)] = 0
    print("test02: largest differences wo %.2e, pdf %.2e, weight %.2e" % (np.abs(wo_raw - wo_test).max(), np.abs(r["pdf"] - test["pdf"]).max(), np.abs(r["weight"] - test["weight"]).max()))
    assert np.allclose(wo_raw, wo_test, atol=1e-4) and np.allclose(r["pdf"], test["pdf"], atol=1e-4) and np.allclose(r["weight"], test["weight"], atol=2e-4)
    assert (test["weight"] != 0).any(0).sum() > 300 and bad.sum() > 0


def _one(mi, bsdf, wi, wo):
    scene, ib = B.bound(mi, bsdf)
    wi = np.asarray(wi, F32).reshape(3, 1); wo = np.asarray(wo, F32).reshape(3, 1); uv = np.zeros((2, 1), F32)
    smp = B.host_sample(mi, scene, ib, None, wi, uv, np.array([0.5], F32), np.array([[0.5], [0.5]], F32))
    val, pdf = B.host_eval_pdf(mi, scene, ib, None, wi, uv, wo)
    return smp["weight"][:, 0], val[:, 0]


def test03_flip_invalid_normals(mi):
    wo = np.array([0.0, 0, 1]); wi = np.array([-1.0, -1, 0.5]); wi /= np.linalg.norm(wi)
    n = np.ones(3) / np.sqrt(3.0)
    d = {"type": "normalmap", "normalmap": {"type": "rgb", "value": [float(x) for x in n * 0.5 + 0.5]}, "nested_bsdf": {"type": "diffuse"}, "flip_invalid_normals": False}
    w, v = _one(mi, mi.load_dict(dict(d)), wi, wo)
    assert np.allclose(w, 0) and np.allclose(v, 0)
    d["flip_invalid_normals"] = True
    w, v = _one(mi, mi.load_dict(dict(d)), wi, wo)
    assert (w > 0).all() and (v > 0).all()


def test04_use_shadowing_function(mi):
    wo = np.array([1.0, 0.01, 0.01]); wo /= np.linalg.norm(wo); n = wo.copy()
    d = {"type": "normalmap", "normalmap": {"type": "rgb", "value": [float(x) for x in n * 0.5 + 0.5]}, "nested_bsdf": {"type": "diffuse", "reflectance": 1.0}, "use_shadowing_function": False}
    w, v = _one(mi, mi.load_dict(dict(d)), [0, 0, 1], wo)
    assert np.allclose(w, 1.0) and np.allclose(v, 1 / np.pi, atol=1e-2)
    d["use_shadowing_function"] = True
    w, v = _one(mi, mi.load_dict(dict(d)), [0, 0, 1], wo)
    assert (w < 0.05).all() and (v < 0.01).all()


# ------------------------------------------------------------------------------------------------ 3b. the per-call derivative dF / dc

GRAD_H = 1e-3          # texel units.  The issue's starting point, h = 1e-2, does not pass its own h against h / 2 check on the rough lobes: the truncation of a central
                       # difference is about (h S)^2 / 6 of the derivative with S = d ln(value) / d direction, 10 ... 100 for alpha 0.3 ... 0.1 -- not the 1e-4 of a smooth
                       # lobe.  At 1e-3 it is <= 2e-3 and the float32 noise of the oracle's inputs, 6e-8 / (2 h) = 3e-5 of the derivative, stays far below the bar.
GRAD_BAR = 1e-2        # relative L2


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("nested", N.NON_DELTA)
def test_per_call_derivative_against_central_differences(mi, O, nested, shadow):
    """har_normalmap_grad_host on 5 000 tuples against central differences of the float64-frame restatement (N.weighted_value64: the nested values from
    OracleScene.bsdf_evaluate_ctx), every non-delta nested model, with and without the shadow term.  Lanes within 1e-3 of a flip or orientation switch -- at the centre or
    at any of the twelve displaced colours -- are excluded, at most 2 % of them; differences at h and h / 2 agree to a third of the bar; and the exact identity
    sum_k dF/dc_k (c_k - 0.5) = 0 holds per tuple (value depends on c only through normalize(2c - 1))."""
    wi, uv, wo, A, c = N.grad_tuples()
    ch = N.Nested(mi, O, nested)
    d = {"type": "normalmap", "normalmap": N.grad_map(c), "inner": N.nested_dict(nested)}
    if not shadow:
        d["use_shadowing_function"] = False
    bsdf = mi.load_dict(d); scene, ib = B.bound(mi, bsdf)
    F, g = N.host_grad(mi, scene, ib, wi, uv, wo, A)
    F0, fprod, oprod = N.weighted_value64(ch, c, wi, uv, wo, A, True, shadow)
    flip0 = fprod <= 0
    assert np.allclose(F, F0, rtol=2e-5, atol=1e-6)                       # the value the entry returns is the restatement's
    near = (np.abs(fprod) < 1e-3) | (np.abs(oprod) < 1e-3)
    fd = {}
    for h in (GRAD_H, GRAD_H / 2):
        out = np.zeros((3, c.shape[1]))
        for k in range(3):
            e = np.zeros((3, 1)); e[k] = h
            fp, a1, b1 = N.weighted_value64(ch, c.astype(np.float64) + e, wi, uv, wo, A, True, shadow, flip0)
            fm, a2, b2 = N.weighted_value64(ch, c.astype(np.float64) - e, wi, uv, wo, A, True, shadow, flip0)
            out[k] = (fp - fm) / (2 * h)
            if h == GRAD_H:
                near |= (np.abs(a1) < 1e-3) | (np.abs(a2) < 1e-3) | (np.abs(b1) < 1e-3) | (np.abs(b2) < 1e-3) | ((a1 <= 0) != flip0) | ((a2 <= 0) != flip0)
        fd[h] = out
    assert near.mean() <= 0.02, float(near.mean())
    ok = ~near
    rel = lambda a, b: float(np.linalg.norm(a[:, ok] - b[:, ok]) / np.linalg.norm(b[:, ok]))
    step = rel(fd[GRAD_H], fd[GRAD_H / 2]); err = rel(g.astype(np.float64), fd[GRAD_H / 2])
    ident = np.abs((g.astype(np.float64) * (c.astype(np.float64) - 0.5)).sum(0)); scale = np.abs(g.astype(np.float64) * (c.astype(np.float64) - 0.5)).sum(0)
    live = scale > 0
    worst_ident = float((ident[live] / scale[live]).max())
    print("normalmap dF/dc %s / shadow %s: relative L2 %.2e against central differences (h = %g; h against h/2 %.2e), identity %.2e of sum |.|, excluded %.2f %%, live lanes %d"
          % (nested, shadow, err, GRAD_H / 2, step, worst_ident, 100 * near.mean(), int(live.sum())))
    assert live.sum() > 2000 and (F[~live] == 0).all()
    assert step <= GRAD_BAR / 3 and err <= GRAD_BAR
    assert worst_ident <= IDENTITY_BAR


# The identity is exact in exact arithmetic; the sweep ends in the float32 projection (g - n (n . g) / |n|^2) / |n_raw|, whose three products cancel to about an ulp of
# |g| |n| while sum |dF/dc_k (c_k - 0.5)| is as small as the tangential part of g.  Measured worst tuple over the twelve cases: 4.54e-5 of sum |.| (diffuse with the
# shadow term; 1.0e-6 ... 3.1e-5 elsewhere): above 1e-5, so the bar is four times the measured value, as for the other float32 bars (docs/parity.md)
IDENTITY_BAR = 1.9e-4


def test_per_call_derivative_of_delta_models_is_zero(mi):
    wi, uv, wo, A, c = N.grad_tuples(n=500)
    for nested in ("dielectric", ):
        bsdf = mi.load_dict({"type": "normalmap", "normalmap": N.grad_map(c), "inner": N.nested_dict(nested)}); scene, ib = B.bound(mi, bsdf)
        F, g = N.host_grad(mi, scene, ib, wi, uv, wo, A)
        assert (F == 0).all() and (g == 0).all()
    bsdf = mi.load_dict({"type": "normalmap", "normalmap": N.grad_map(c), "inner": {"type": "conductor"}}); scene, ib = B.bound(mi, bsdf)
    F, g = N.host_grad(mi, scene, ib, wi, uv, wo, A)
    assert (F == 0).all() and (g == 0).all()


# ------------------------------------------------------------------------------------------------ 4. frames

def _hits_on(mi, scene, mesh, inst, n=64, seed=3):
    """n preliminary hits on the two faces of mesh `mesh` with random barycentrics and ray directions"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.05, 0.6, n).astype(F32); v = rng.uniform(0.05, 0.35, n).astype(F32)
    d = rng.normal(size=(3, n)); d = (d / np.linalg.norm(d, axis=0)).astype(F32)
    return d, np.ones(n, F32), u, v, (np.arange(n) % 2).astype(np.uint32), np.full(n, mesh, np.uint32), np.full(n, inst, np.uint32)


FRAME_CASES = [(xf, fl, inst) for xf in ("rotation", "scale", "shear", "mirror") for fl in (False, True) for inst in (None, ) + N.INSTANCE_XF]


def check_rectangle_frame(mi, rows_of, xf, flip_normals, inst):
    """the sh_frame rows of a rectangle under a normalmap against the reference's rule in float64; the same rectangle WITHOUT a normalmap keeps coordinate_system(n)"""
    tw = N.rectangle_transforms(mi)[xf]; itw = None if inst is None else N.instance_transform(mi, inst)
    nm = N.normalmap_dict(mi, "diffuse", "tilt30")
    scene = mi.load_dict(N.frame_scene(mi, tw, flip_normals, nm, itw))
    plain = mi.load_dict(N.frame_scene(mi, tw, flip_normals, N.nested_dict("diffuse"), itw))
    hits = _hits_on(mi, scene, 0, 0xffffffff if inst is None else 0)
    rows = rows_of(scene, hits); prow = rows_of(plain, hits)
    n64, s64, t64 = N.rectangle_frame(tw.matrix, flip_normals, None if itw is None else itw.matrix)
    n, s, t = rows[6:9], rows[9:12], rows[12:15]
    assert np.allclose(n, n64[:, None], **FRAME) and np.allclose(s, s64[:, None], **FRAME) and np.allclose(t, t64[:, None], **FRAME), (xf, flip_normals, inst, np.abs(s - s64[:, None]).max(), np.abs(t - t64[:, None]).max())
    tri = (t.astype(np.float64) * np.cross(n.astype(np.float64).T, s.astype(np.float64).T).T).sum(0)
    want_sign = np.sign(np.dot(t64, np.cross(n64, s64)))
    assert (np.sign(tri) == want_sign).all() and np.allclose(np.abs(tri), 1.0, atol=1e-5)
    wi = rows[15:18]; d = hits[0].astype(np.float64)
    assert np.allclose(wi, np.stack([-(d * s64[:, None]).sum(0), -(d * t64[:, None]).sum(0), -(d * n64[:, None]).sum(0)]), rtol=3e-6, atol=1e-6)
    # everything but the frame and wi is what the plain scene reports, bit for bit
    other = [r for r in range(33) if r not in range(9, 18)]
    assert np.array_equal(rows[other], prow[other])
    return rows, prow, hits


@pytest.mark.parametrize("xf,flip_normals,inst", FRAME_CASES)
def test_rectangle_frames_host(mi, xf, flip_normals, inst):
    rows_of = lambda scene, hits: N.host_si(mi, scene, *hits)
    rows, prow, hits = check_rectangle_frame(mi, rows_of, xf, flip_normals, inst)
    # ... and the plain scene's frame is coordinate_system(n): what compute_si builds (the rows of a scene without a normalmap do not go through the tangent code at all)
    n = prow[6:9].astype(np.float64); s = prow[9:12].astype(np.float64); t = prow[12:15].astype(np.float64)
    assert np.allclose((n * s).sum(0), 0, atol=1e-6) and np.allclose(np.cross(n.T, s.T).T, t, atol=1e-6)


def test_mesh_without_normals_keeps_its_frame_bit_for_bit(mi):
    """case 1: a mesh without vertex normals (with and without texcoords) under a normalmap reports today's rows -- those of the same mesh under a plain BSDF"""
    for tc in (True, False):
        nm = N.normalmap_dict(mi, "diffuse", "tilt30")
        a = mi.load_dict({"type": "scene", "m": dict(N.flat_mesh(texcoords=tc), bsdf=nm, to_world=mi.ScalarTransform4f().rotate([0.6, 0.0, 0.8], 40.0))})
        b = mi.load_dict({"type": "scene", "m": dict(N.flat_mesh(texcoords=tc), bsdf=N.nested_dict("diffuse"), to_world=mi.ScalarTransform4f().rotate([0.6, 0.0, 0.8], 40.0))})
        hits = _hits_on(mi, a, 0, 0xffffffff)
        assert np.array_equal(N.host_si(mi, a, *hits), N.host_si(mi, b, *hits))


def test_rectangle_record_survives_to_world_updates(mi):
    """params['<rectangle>.to_world'] = a mirroring transform; update(): the flags are those a fresh load gives"""
    nm = N.normalmap_dict(mi, "diffuse", "tilt30")
    T = N.rectangle_transforms(mi)
    scene = mi.load_dict(N.frame_scene(mi, T["rotation"], False, nm))
    params = mi.traverse(scene)
    params["rect.to_world"] = T["mirror"].matrix.astype(np.float32); params.update()
    fresh = mi.load_dict(N.frame_scene(mi, T["mirror"], False, N.normalmap_dict(mi, "diffuse", "tilt30")))
    hits = _hits_on(mi, scene, 0, 0xffffffff)
    assert scene.desc().meshes[0].flags == fresh.desc().meshes[0].flags == 3 | 4 | 8
    # (the update inverts the 4 x 4 it is given, the loader composes the inverse: the baked normals agree to rounding)
    assert np.allclose(N.host_si(mi, scene, *hits), N.host_si(mi, fresh, *hits), rtol=3e-6, atol=1e-6)
    n64, s64, t64 = N.rectangle_frame(T["mirror"].matrix, False)
    assert np.allclose(N.host_si(mi, scene, *hits)[12:15], t64[:, None], **FRAME)


# ------------------------------------------------------------------------------------------------ 5. aov

def aov_rays(n=20480, seed=9):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-1.3, 1.3, n), rng.uniform(-1.3, 1.3, n), np.where(np.arange(n) % 4 == 0, -1.5, 2.0)]).astype(F32)          # a quarter from below
    d = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), np.where(np.arange(n) % 4 == 0, 1.0, -1.0)]); d = (d / np.linalg.norm(d, axis=0)).astype(F32)
    return o, d, np.full(n, np.inf, F32)


def aov_scene(mi, shape):
    tex = N.bumpy_texels()
    m = np.eye(3); m[:2, :] = N.TO_UV
    nm = {"type": "normalmap", "normalmap": {"type": "bitmap", "data": tex, "raw": True, "to_uv": mi.ScalarTransform3f(m)}, "x": N.nested_dict("roughplastic")}
    return mi.load_dict(N.lit_scene(mi, nm, shape)), tex


def expected_sh_normal(mi, O, scene, tex, shape, o, d, maxt):
    """frame().second.n in float64: the twin scene (the nested BSDF alone) gives hit, n, uv and -- for the flat mesh -- the frame; a rectangle's frame is the float64 rule"""
    twin = mi.load_dict(N.lit_scene(mi, N.nested_dict("roughplastic"), shape))
    osc, _ = O.scene_from_product(twin)
    t, u, v, prim, sh, inst = osc.ray_intersect(o, d, maxt)
    hit = np.isfinite(t)
    rows = osc.surface_interaction_flags(o, d, t, u, v, prim, sh, inst, ray_flags=1, active=hit).astype(np.float64)
    card = hit & (sh == [i for i, m in enumerate(scene.meshes) if m["key"] == "card"][0])
    n, s, tt = rows[6:9].copy(), rows[9:12].copy(), rows[12:15].copy()
    if shape == "rectangle":
        rect = [m for m in scene.meshes if m["key"] == "card"][0]["rect"]
        n64, s64, t64 = N.rectangle_frame(rect["to_world"].matrix, rect["flip"])
        n[:, card] = n64[:, None]; s[:, card] = s64[:, None]; tt[:, card] = t64[:, None]
    dd = d.astype(np.float64)
    wi = np.stack([-(dd * s).sum(0), -(dd * tt).sum(0), -(dd * n).sum(0)])
    c = N.lookup_colour(tex, rows[18:20].astype(F32), N.TO_UV)
    fs, ft, fn = N.frame64(c, wi, True)
    world = s * fn[0] + tt * fn[1] + n * fn[2]
    out = np.where(card[None, :], world, np.where(hit[None, :], n, 0.0))
    seam = card & (np.abs(wi[2] * (wi * (2 * c - 1)).sum(0)) < 1e-6)          # the flip decided the other way round within rounding
    return out, card, seam


@pytest.mark.parametrize("shape", ["rectangle", "mesh"])
def test_aov_sh_normal_host(mi, O, shape):
    scene, tex = aov_scene(mi, shape)
    o, d, maxt = aov_rays()
    integ = mi.load_dict({"type": "aov", "aovs": "nn:sh_normal,aa:albedo"})
    got = integ.sample_host(scene, o, d, maxt)
    want, card, seam = expected_sh_normal(mi, O, scene, tex, shape, o, d, maxt)
    assert card.sum() > 5000 and seam.mean() < 1e-3
    ok = ~seam
    assert np.allclose(got[0:3][:, ok], want[:, ok], **FRAME), float(np.abs(got[0:3][:, ok] - want[:, ok]).max())
    assert (np.abs(got[0:3][:, card] - np.array([[0.0], [0.0], [1.0]])).max(0) > 0.05).mean() > 0.9          # perturbed: not the flat normal
    assert np.allclose(got[3:6][:, card], np.array(N.NESTED["roughplastic"]["diffuse_reflectance"]["value"], F32)[:, None])          # the nested BSDF's albedo


# ------------------------------------------------------------------------------------------------ 6. renders on the host

RES, SPP = (16, 12), 4


def _pair(mi, O, a, b, seed=3, md=6, rr=7):
    from tests.test_cpu_host import rel_l2
    fa, sa = B.host_render_stats(mi, mi.load_dict(a), seed, SPP, md, rr); fb, sb = B.host_render_stats(mi, mi.load_dict(b), seed, SPP, md, rr)
    assert np.isfinite(fa).all() and np.linalg.norm(fb[..., :3]) > 0
    return rel_l2(O.develop(fa), O.develop(fb)), (sa.paths, sa.vertices), (sb.paths, sb.vertices)


@pytest.mark.parametrize("nested", N.NESTED_NAMES)
def test_host_render_identity_map(mi, O, nested):
    """an identity normal map over the nested model on the Cornell walls (N.WALLS) is the scene with the nested BSDF alone: relative L2 1e-6, equal counters"""
    err, got, want = _pair(mi, O, N.walls_box(mi, RES, SPP, N.normalmap_dict(mi, nested, "identity"), N.nested_dict(nested)), N.walls_box(mi, RES, SPP, N.nested_dict(nested), N.nested_dict(nested)))
    print("host render, identity map over %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (nested, err, got, want))
    assert err <= 1e-6 and got == want and got[1] > got[0]


@pytest.mark.parametrize("nested", N.HALF_TURN_INVARIANT)
def test_host_render_identity_map_all_five_walls(mi, O, nested):
    """... with the map on the red and the green wall too, for the nested models whose sampling commutes with the half turn between those walls' two frames (N.WALLS)"""
    err, got, want = _pair(mi, O, N.walls_box(mi, RES, SPP, N.normalmap_dict(mi, nested, "identity"), N.nested_dict(nested), walls=N.ALL_WALLS),
                           N.walls_box(mi, RES, SPP, N.nested_dict(nested), N.nested_dict(nested), walls=N.ALL_WALLS))
    print("host render, identity map on all five walls over %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (nested, err, got, want))
    assert err <= 1e-6 and got == want


@pytest.mark.parametrize("variant", ["twosided", "instanced"])
def test_host_render_identity_map_variants(mi, O, variant):
    nd = N.nested_dict("roughplastic")
    if variant == "twosided":
        a = N.walls_box(mi, RES, SPP, {"type": "twosided", "x": N.normalmap_dict(mi, "roughplastic", "identity")}, {"type": "twosided", "x": dict(nd)})
        b = N.walls_box(mi, RES, SPP, {"type": "twosided", "x": dict(nd)}, {"type": "twosided", "x": dict(nd)})
    else:
        a = N.walls_box(mi, RES, SPP, N.normalmap_dict(mi, "roughplastic", "identity"), dict(nd), instanced=True); b = N.walls_box(mi, RES, SPP, dict(nd), dict(nd), instanced=True)
    err, got, want = _pair(mi, O, a, b)
    print("host render, identity map, %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (variant, err, got, want))
    assert err <= 1e-6 and got == want


def composed_film(mi, O, scene, tex, nested, shape, flip, shadow, seed, spp, low_camera=False):
    """The film of N.lit_scene (one point light, max_depth 2) composed on the CPU, no new oracle entry: the lanes' film positions from orc_sampler_stream, the camera rays
    from orc_sensor_sample_ray, the hits and interactions from the oracle's twin scene (the nested BSDF alone; a rectangle's frame from the float64 rule), the restated
    normalmap.eval over the oracle's nested answers, the point light's intensity / dist^2, an occlusion query, orc_film_put.  With max_depth 2 the only radiance of a lane
    is the emitter sample at the first vertex (the second vertex adds emission only, and nothing emits)."""
    twin = mi.load_dict(N.lit_scene(mi, N.nested_dict(nested), shape, RES, spp, low_camera=low_camera))
    osc, sensor = O.scene_from_product(twin)
    ipos, pos = A.lane_positions(O, sensor, "box", seed, spp)
    n = pos.shape[1]
    sx = F32(1.0) / F32(sensor.crop_width); sy = F32(1.0) / F32(sensor.crop_height)
    px = (pos[0].astype(np.float64) * sx).astype(F32); py = (pos[1].astype(np.float64) * sy).astype(F32)
    o = np.zeros((3, n), F32); d = np.zeros((3, n), F32); mt = np.zeros(n, F32)
    O.lib().orc_sensor_sample_ray(C.byref(sensor), n, O.fp(px), O.fp(py), O.fp(o), O.fp(d), O.fp(mt))
    t, u, v, prim, sh, inst = osc.ray_intersect(o, d, mt)
    hit = np.isfinite(t)
    rows = osc.surface_interaction_flags(o, d, t, u, v, prim, sh, inst, ray_flags=1, active=hit).astype(np.float64)
    nrm, s, tt = rows[6:9].copy(), rows[9:12].copy(), rows[12:15].copy()
    if shape == "rectangle":
        rect = [m for m in scene.meshes if m["key"] == "card"][0]["rect"]
        n64, s64, t64 = N.rectangle_frame(rect["to_world"].matrix, rect["flip"])
        s[:, hit] = s64[:, None]; tt[:, hit] = t64[:, None]
    p = rows[0:3]
    to_local = lambda w: np.stack([(w * s).sum(0), (w * tt).sum(0), (w * nrm).sum(0)])
    wi = to_local(-d.astype(np.float64))
    lamp = np.array([0.6, 0.4, 1.5])[:, None]; intensity = np.array([6.0, 5.0, 4.0])
    L = lamp - p; dist2 = (L * L).sum(0); wl = L / np.sqrt(dist2)
    wo = to_local(wl)
    k = np.nonzero(hit)[0]
    c = N.lookup_colour(tex, rows[18:20][:, k].astype(F32), N.TO_UV).astype(F32)
    ch = N.Nested(mi, O, nested)
    val, _, _, near = N.expected_eval_pdf(ch, (0, 0x1ff, ALL), c, wi[:, k].astype(F32), rows[18:20][:, k].astype(F32), wo[:, k].astype(F32), flip, shadow)
    # occlusion: from the hit point (lifted off the surface) towards the lamp
    so = (p[:, k] + nrm[:, k] * 1e-4 * np.sign((wl[:, k] * nrm[:, k]).sum(0))).astype(F32)
    blocked = osc.ray_test(so, wl[:, k].astype(F32), (np.sqrt(dist2[k]) * (1 - 1e-3)).astype(F32))
    rad = np.zeros((3, n))
    rad[:, k] = np.where(np.asarray(blocked, bool)[None, :], 0.0, val.astype(np.float64) * intensity[:, None] / dist2[k][None, :])
    v4 = np.zeros((n, 4), F32); v4[:, :3] = rad.T.astype(F32); v4[:, 3] = 1.0
    film = np.zeros((sensor.crop_height, sensor.crop_width, 4), F32)
    O.lib().orc_film_put(C.byref(sensor), n, O.fp(np.ascontiguousarray(ipos[0])), O.fp(np.ascontiguousarray(ipos[1])), O.fp(v4), O.fp(film))
    return film, float(near.mean())


def composition_scene(mi, nested, shape, flip=True, shadow=True, spp=SPP, res=RES, integrator="path", low_camera=False):
    tex = N.bumpy_texels()
    m = np.eye(3); m[:2, :] = N.TO_UV
    nm = {"type": "normalmap", "normalmap": {"type": "bitmap", "data": tex, "raw": True, "to_uv": mi.ScalarTransform3f(m)}, "x": N.nested_dict(nested)}
    if not flip:
        nm["flip_invalid_normals"] = False
    if not shadow:
        nm["use_shadowing_function"] = False
    return mi.load_dict(N.lit_scene(mi, nm, shape, res, spp, integrator=integrator, max_depth=2, rr_depth=8, low_camera=low_camera)), tex


@pytest.mark.parametrize("nested", ["diffuse", "roughplastic"])
@pytest.mark.parametrize("shape", ["rectangle", "mesh"])
def test_host_render_composition(mi, O, shape, nested):
    """a rectangle (case 2) and a flat mesh (case 1) under a bilinear bitmap normal map with to_uv, one point light, max_depth 2: the host film equals the film composed
    from oracle calls and the restated eval at relative L2 1e-4, the weights at 2e-6"""
    from tests.test_cpu_host import rel_l2
    scene, tex = composition_scene(mi, nested, shape)
    got, _ = B.host_render_stats(mi, scene, 5, SPP, 2, 8)
    want, near = composed_film(mi, O, scene, tex, nested, shape, True, True, 5, SPP)
    err = rel_l2(O.develop(got), O.develop(want))
    print("host render, composition %s / %s: rel L2 %.3g (lanes near a switch: %.2g)" % (shape, nested, err, near))
    assert np.linalg.norm(want[..., :3]) > 0 and err <= 1e-4 and np.allclose(got[..., 3], want[..., 3], rtol=2e-6, atol=0)


@pytest.mark.parametrize("switch", ["flip_invalid_normals", "use_shadowing_function"])
def test_host_render_switches(mi, O, switch):
    """each switch, turned off, changes the composed film as the restatement predicts (same bars) and differs from the default by more than ten times the bar"""
    from tests.test_cpu_host import rel_l2
    flip, shadow = switch != "flip_invalid_normals", switch != "use_shadowing_function"
    low = switch == "flip_invalid_normals"          # (seen from above no bump of at most 50 degrees turns away from the camera)
    scene, tex = composition_scene(mi, "roughplastic", "rectangle", flip, shadow, low_camera=low)
    got, _ = B.host_render_stats(mi, scene, 5, SPP, 2, 8)
    want, _ = composed_film(mi, O, scene, tex, "roughplastic", "rectangle", flip, shadow, 5, SPP, low)
    default, _ = composed_film(mi, O, scene, tex, "roughplastic", "rectangle", True, True, 5, SPP, low)
    err = rel_l2(O.develop(got), O.develop(want)); apart = rel_l2(O.develop(got), O.develop(default))
    print("host render, %s = false: rel L2 %.3g against the restatement, %.3g away from the default" % (switch, err, apart))
    assert err <= 1e-4 and apart > 1e-3


def test_params_update_gives_the_scene_a_fresh_load_gives(mi, O):
    """in-place params.update() of '<bsdf>.normalmap.data' and of a nested colour: the host film of the updated scene is the film of a scene loaded with those values"""
    scene, tex = composition_scene(mi, "diffuse", "rectangle")
    new_tex = N.bumpy_texels(seed=77); new_rgb = np.array([0.7, 0.2, 0.4], np.float32)
    params = mi.traverse(scene)
    params["mat.normalmap.data"] = new_tex; params["mat.nested_bsdf.reflectance.value"] = new_rgb
    params.update()
    got, _ = B.host_render_stats(mi, scene, 5, SPP, 2, 8)
    m = np.eye(3); m[:2, :] = N.TO_UV
    nm = {"type": "normalmap", "normalmap": {"type": "bitmap", "data": new_tex, "raw": True, "to_uv": mi.ScalarTransform3f(m)},
          "x": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [float(x) for x in new_rgb]}}}
    fresh = mi.load_dict(N.lit_scene(mi, nm, "rectangle", RES, SPP, max_depth=2, rr_depth=8))
    want, _ = B.host_render_stats(mi, fresh, 5, SPP, 2, 8)
    before, _ = B.host_render_stats(mi, composition_scene(mi, "diffuse", "rectangle")[0], 5, SPP, 2, 8)
    assert np.array_equal(got, want) and not np.array_equal(got, before)


def test_parameter_names_of_a_render_scene(mi):
    """mi.traverse names the normal map and the nested colour of a scene's material (gradient requests are refused by name: the device test)"""
    scene, _ = composition_scene(mi, "diffuse", "rectangle", integrator="prb")
    keys = mi.traverse(scene).keys()
    assert "mat.normalmap.data" in keys and "mat.nested_bsdf.reflectance.value" in keys
