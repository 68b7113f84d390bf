"""`blendbsdf` on the CPU, through the library's host entries (har_bsdf_eval_pdf_host / har_bsdf_sample_host / har_render_lanes_host run the HAR_HD code the kernels run):
the reference's own tests (src/bsdfs/tests/test_blendbsdf.py 01-06; 07 / 08 need `roughdielectric`, which this variant does not have, and are left out), the
composition against the oracle's answers for the nested BSDFs, host renders with full oracle parity, and the loader."""
import numpy as np
import pytest

from tests import blend_cases as B

ALL = B.ALL


def _blend(mi, a, b, weight=0.2):
    return mi.load_dict({"type": "blendbsdf", "nested1": a, "nested2": b, "weight": weight})


def _col(v):
    return np.asarray(v, np.float32).reshape(-1, 1)


# ------------------------------------------------------------------------------------------------ 1. the reference's tests

def test01_create(mi):
    F = mi.BSDFFlags
    bsdf = _blend(mi, {"type": "diffuse"}, {"type": "diffuse"})
    assert bsdf.component_count() == 2
    assert bsdf.flags(0) == F.DiffuseReflection | F.FrontSide and bsdf.flags(1) == F.DiffuseReflection | F.FrontSide
    assert bsdf.flags() == bsdf.flags(0) | bsdf.flags(1)
    bsdf = _blend(mi, {"type": "roughconductor"}, {"type": "diffuse"})
    assert bsdf.component_count() == 2
    assert bsdf.flags(0) == F.GlossyReflection | F.FrontSide and bsdf.flags(1) == F.DiffuseReflection | F.FrontSide
    assert bsdf.flags() == bsdf.flags(0) | bsdf.flags(1)
    assert _blend(mi, {"type": "plastic"}, {"type": "roughplastic"}).component_count() == 4


def _three(mi, a, b, weight=0.2):
    """the blend and its two nested BSDFs as objects (the reference's tests hand instantiated plugins to the blend and evaluate them on their own too)"""
    b0, b1 = mi.load_dict(a), mi.load_dict(b)
    blend = _blend(mi, b0, b1, weight)
    scene, index = B.bound(mi, blend)
    return scene, index, b0.index, b1.index


def test02_eval_all(mi):
    w = np.float32(0.2)
    scene, ib, i0, i1 = _three(mi, {"type": "conductor"}, {"type": "diffuse", "reflectance": {"type": "rgb", "value": 1.0}})
    wi = _col([0, 0, 1]); wo = _col([0, 0, 1]); uv = np.zeros((2, 1), np.float32); ctx = (0, 0x1ff, ALL)
    e0 = B.host_eval_pdf(mi, scene, i0, ctx, wi, uv, wo)[0]; e1 = B.host_eval_pdf(mi, scene, i1, ctx, wi, uv, wo)[0]
    value = B.host_eval_pdf(mi, scene, ib, ctx, wi, uv, wo)[0]
    assert np.allclose(value, (1 - w) * e0 + w * e1, rtol=1e-5, atol=1e-8) and (value > 0).all()


def test03_eval_components(mi):
    w = np.float32(0.2)
    scene, ib, i0, i1 = _three(mi, {"type": "conductor"}, {"type": "diffuse", "reflectance": {"type": "rgb", "value": 1.0}})
    wi = _col([0, 0, 1]); wo = _col([0, 0, 1]); uv = np.zeros((2, 1), np.float32); ctx = (0, 0x1ff, ALL)
    e0 = B.host_eval_pdf(mi, scene, i0, ctx, wi, uv, wo)[0]; e1 = B.host_eval_pdf(mi, scene, i1, ctx, wi, uv, wo)[0]
    assert np.allclose(B.host_eval_pdf(mi, scene, ib, (0, 0x1ff, 0), wi, uv, wo)[0], (1 - w) * e0, rtol=1e-5, atol=1e-8)
    v1 = B.host_eval_pdf(mi, scene, ib, (0, 0x1ff, 1), wi, uv, wo)[0]
    assert np.allclose(v1, w * e1, rtol=1e-5, atol=1e-8) and (v1 > 0).all()


def test04_sample_all(mi):
    bsdf = _blend(mi, {"type": "plastic"}, {"type": "diffuse", "reflectance": {"type": "rgb", "value": 1.0}})
    scene, ib = B.bound(mi, bsdf)
    wi = _col([0, 0, 1]); uv = np.zeros((2, 1), np.float32); ctx = (0, 0x1ff, ALL)
    for s1, s2 in ((0.1, [0.2, 0.9]), (0.3, [0.4, 0.6])):          # sample1 below and above the weight: nested BSDF 1, nested BSDF 0
        bs = B.host_sample(mi, scene, ib, ctx, wi, uv, np.float32([s1]), _col(s2))
        val, pdf = B.host_eval_pdf(mi, scene, ib, ctx, wi, uv, bs["wo"])
        assert pdf[0] > 0 and np.allclose(bs["weight"], val / pdf, rtol=1e-5, atol=1e-8)


def test05_sample_components(mi):
    w = np.float32(0.2)
    scene, ib, i0, i1 = _three(mi, {"type": "conductor"}, {"type": "diffuse", "reflectance": {"type": "rgb", "value": 1.0}})
    wi = _col([0, 0, 1]); uv = np.zeros((2, 1), np.float32); ctx = (0, 0x1ff, ALL)
    for comp, child, k in ((0, i0, 1 - w), (1, i1, w)):
        for s1, s2 in ((0.1, [0.5, 0.5]), (0.3, [0.2, 0.7])):
            want = B.host_sample(mi, scene, child, ctx, wi, uv, np.float32([s1]), _col(s2))
            got = B.host_sample(mi, scene, ib, (0, 0x1ff, comp), wi, uv, np.float32([s1]), _col(s2))
            assert np.allclose(got["weight"], k * want["weight"], rtol=1e-5, atol=1e-8) and (want["weight"] > 0).all()
            assert np.allclose(got["wo"], want["wo"], rtol=1e-5, atol=1e-8) and np.allclose(got["pdf"], want["pdf"], rtol=1e-5, atol=1e-8)


CHI2 = {"diffuse+diffuse": ({"type": "diffuse"}, {"type": "diffuse"}),
        "diffuse+roughconductor": ({"type": "diffuse"}, {"type": "roughconductor", "alpha": 0.5}),
        "roughplastic+roughconductor": ({"type": "roughplastic", "alpha": 0.5}, {"type": "roughconductor", "alpha": 0.5})}


@pytest.mark.parametrize("name", list(CHI2))
def test06_chi2(mi, name):
    """the chi^2 test of tests/test_bsdfs_cpu.py::test_sampling_density_chi2 (the reference's ChiSquareTest re-hosted: a (cos theta, phi) histogram of the sampled
    directions against the cell integrals of pdf(), cells below 5 expected samples pooled, significance 0.01, Sidak-corrected over the tests of this file), at its
    sizes, through the host entries"""
    from scipy import stats
    import zlib
    bsdf = _blend(mi, *CHI2[name]); scene, ib = B.bound(mi, bsdf)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n_samples, R, Cc, sub = 40000, 24, 48, 6
    ctx = (0, 0x1ff, ALL)
    for wi3 in ([0.0, 0.0, 1.0], [0.6, -0.3, 0.74]):
        wi3 = np.float32(wi3) / np.linalg.norm(wi3)
        wi = np.repeat(wi3.reshape(3, 1), n_samples, 1).astype(np.float32); uv = np.zeros((2, n_samples), np.float32)
        s = rng.random((3, n_samples)).astype(np.float32)
        bs = B.host_sample(mi, scene, ib, ctx, wi, uv, s[0], s[1:])
        ok = (bs["weight"] > 0).any(0) & ((bs["sampled_type"] & 0x61) == 0)
        z = np.clip(bs["wo"][2, ok].astype(np.float64), -1, 1); phi = np.arctan2(bs["wo"][1, ok].astype(np.float64), bs["wo"][0, ok].astype(np.float64)) % (2 * np.pi)
        hist = np.zeros((R, Cc))
        np.add.at(hist, (np.minimum(((z + 1) / 2 * R).astype(int), R - 1), np.minimum((phi / (2 * np.pi) * Cc).astype(int), Cc - 1)), 1)
        i, j, a, b = np.meshgrid(np.arange(R), np.arange(Cc), np.arange(sub), np.arange(sub), indexing="ij")
        zz = -1 + 2 * (i + (a + 0.5) / sub) / R; pp = 2 * np.pi * (j + (b + 0.5) / sub) / Cc; rr = np.sqrt(np.maximum(0.0, 1 - zz * zz))
        wo = np.stack([rr * np.cos(pp), rr * np.sin(pp), zz]).reshape(3, -1).astype(np.float32)
        m = wo.shape[1]
        pdf = B.host_eval_pdf(mi, scene, ib, ctx, np.repeat(wi3.reshape(3, 1), m, 1), np.zeros((2, m), np.float32), wo)[1]
        cell = (2.0 / R) * (2 * np.pi / Cc)
        expected = pdf.astype(np.float64).reshape(R, Cc, sub * sub).mean(2) * cell * n_samples
        assert abs(expected.sum() / n_samples - hist.sum() / n_samples) < 0.02
        o, e = hist.ravel(), expected.ravel()
        order = np.argsort(e); o, e = o[order], e[order]
        big = e >= 5
        chi2 = float(((o[big] - e[big]) ** 2 / e[big]).sum()); dof = int(big.sum())
        if e[~big].sum() > 0:
            chi2 += (o[~big].sum() - e[~big].sum()) ** 2 / max(e[~big].sum(), 1e-9); dof += 1
        p = stats.chi2.sf(chi2, dof - 1)
        print("chi2 %s wi.z=%.2f: p = %.3f" % (name, wi3[2], p))
        assert p > 1.0 - (1.0 - 0.01) ** (1.0 / 6.0), (name, wi3, chi2, dof, p)


# ------------------------------------------------------------------------------------------------ 2. composition against the oracle

LEAF = dict(rtol=2e-6, atol=1e-9)          # the bars the leaf models hold against the oracle (tests/test_gpu_boundary_masks.py)
MIXED = dict(rtol=2e-5, atol=1e-7)         # composed BSDF values (tests/test_aov_cpu.py): a product sum and a reciprocal on top


@pytest.mark.parametrize("weight", B.WEIGHT_NAMES)
@pytest.mark.parametrize("pair", B.PAIR_NAMES)
def test_composition_against_oracle(mi, O, pair, weight):
    """eval / pdf / sample of the blend on 20 000 tuples, every context, against blendbsdf.cpp restated in float32 over the oracle's nested answers; the weight from an
    independent float64 lookup.  Every lane is compared.  Measured maxima (all pairs, weights and contexts): docs/parity.md, "blendbsdf"."""
    bsdf = mi.load_dict(B.blend_dict(mi, pair, weight)); scene, ib = B.bound(mi, bsdf)
    ch = B.Children(mi, O, pair)
    wi, uv, wo, s1, s2, w = B.tuples(weight)
    worst = {}
    for ctx in B.contexts(pair):
        comp = ctx[2] != ALL
        val, pdf = B.host_eval_pdf(mi, scene, ib, ctx, wi, uv, wo)
        ev, ep = B.expected_eval_pdf(ch, ctx, w, wi, uv, wo)
        assert np.isfinite(val).all() and np.isfinite(pdf).all()
        bar = LEAF if comp else MIXED
        assert np.allclose(pdf, ep, **LEAF), (pair, weight, ctx, "pdf", float(np.abs(pdf - ep).max()))
        assert np.allclose(val, ev, **bar), (pair, weight, ctx, "value", float(np.abs(val - ev).max()))
        got = B.host_sample(mi, scene, ib, ctx, wi, uv, s1, s2)
        want = B.expected_sample(ch, ctx, w, wi, uv, s1, s2)
        for key in ("sampled_type", "sampled_component", "eta"):
            assert np.array_equal(got[key], want[key]), (pair, weight, ctx, key, int((got[key] != want[key]).sum()))
        assert np.allclose(got["wo"], want["wo"], rtol=2e-6, atol=1e-7), (pair, weight, ctx, "wo")
        fin = np.isfinite(want["pdf"]) & np.isfinite(want["weight"]).all(0)          # (a nested delta lobe met at w = 0 / 1 forms 0 * inf in the reference's own arithmetic)
        assert np.array_equal(np.isfinite(got["pdf"]) & np.isfinite(got["weight"]).all(0), fin)
        assert np.allclose(got["pdf"][fin], want["pdf"][fin], **LEAF), (pair, weight, ctx, "sample pdf", float(np.abs(got["pdf"][fin] - want["pdf"][fin]).max()))
        assert np.allclose(got["weight"][:, fin], want["weight"][:, fin], **bar), (pair, weight, ctx, "weight", float(np.abs(got["weight"][:, fin] - want["weight"][:, fin]).max()))
        for name, a, b in (("value", val, ev), ("pdf", pdf, ep), ("sample weight", got["weight"][:, fin], want["weight"][:, fin]), ("sample pdf", got["pdf"][fin], want["pdf"][fin])):
            big = np.abs(b) > 1e-6
            if big.any():
                worst[name] = max(worst.get(name, 0.0), float((np.abs(a[big].astype(np.float64) - b[big]) / np.abs(b[big])).max()))
        if not comp and ctx[1] == 0x1ff:
            assert (val > 0).any() and (got["weight"] > 0).any()
    print("blendbsdf composition %s / %s: largest relative differences %s" % (pair, weight, {k: "%.2e" % v for k, v in worst.items()}))


def test_masks_and_null_context(mi):
    """a masked lane returns zeros; the NULL context is BSDFContext()"""
    bsdf = mi.load_dict(B.blend_dict(mi, "plastic+diffuse", "constant")); scene, ib = B.bound(mi, bsdf)
    wi, uv, wo, s1, s2, w = B.tuples("constant", n=512)
    active = (np.arange(512) % 3 != 0)
    val, pdf = B.host_eval_pdf(mi, scene, ib, (0, 0x1ff, ALL), wi, uv, wo, active)
    v0, p0 = B.host_eval_pdf(mi, scene, ib, None, wi, uv, wo)
    assert (val[:, ~active] == 0).all() and (pdf[~active] == 0).all() and np.array_equal(val[:, active], v0[:, active]) and np.array_equal(pdf[active], p0[active])
    bs = B.host_sample(mi, scene, ib, (0, 0x1ff, ALL), wi, uv, s1, s2, active)
    b0 = B.host_sample(mi, scene, ib, None, wi, uv, s1, s2)
    assert (bs["weight"][:, ~active] == 0).all() and (bs["wo"][:, ~active] == 0).all() and (bs["sampled_type"][~active] == 0).all()
    assert np.array_equal(bs["wo"][:, active], b0["wo"][:, active]) and np.array_equal(bs["weight"][:, active], b0["weight"][:, active])


# ------------------------------------------------------------------------------------------------ 3. host renders with full oracle parity

def _host_vs_oracle(mi, O, blend_scene_dict, ref_scene_dict, seed=3, spp=4, md=6, rr=7):
    """(relative L2 of the developed images, the host render's (paths, vertices), the oracle's)"""
    from tests.test_cpu_host import rel_l2
    scene = mi.load_dict(blend_scene_dict); ref = mi.load_dict(ref_scene_dict)
    osc, osensor = O.scene_from_product(ref)
    got, gst = B.host_render_stats(mi, scene, seed, spp, md, rr)
    want, st = osc.render_path(osensor, seed=seed, spp=spp, max_depth=md, rr_depth=rr, raw=True, threads=2)
    assert np.isfinite(got).all() and np.linalg.norm(want[..., :3]) > 0
    return rel_l2(O.develop(got), O.develop(want)), (gst.paths, gst.vertices), (st.paths, st.vertices)


def test_host_render_diffuse_blend_is_a_diffuse_bsdf(mi, O):
    """a blend of two diffuse BSDFs IS a diffuse BSDF of albedo (1 - w) A + w B with the same sampled directions (diffuse ignores sample1, the two pdfs are equal): the
    host render of a box whose walls all carry such a blend (8 x 8 bilinear weights in (0.1, 0.9)) equals the oracle's render of the box with that albedo bitmap, with
    equal path and vertex counts (har_render_lanes_stats_host)"""
    w = B.weight_map8()
    err, got, want = _host_vs_oracle(mi, O, B.blended_box(mi, (16, 12), 4, B.DIFFUSE_PAIR, w), B.equivalent_box(mi, (16, 12), 4, B.albedo_map(w)))
    print("host render, diffuse + diffuse blend against the oracle's albedo bitmap: rel L2 %.3g, (paths, vertices) %s vs %s" % (err, got, want))
    assert err <= 1e-4 and got == want and got[0] == 16 * 12 * 4 and got[1] > got[0]


@pytest.mark.parametrize("end", [0.0, 1.0])
def test_host_render_end_points(mi, O, end):
    """w == 0 and w == 1 over roughconductor / diffuse: the pure nested scenes (the end points of the sampling branch: sample1 > 0 almost surely, sample1 <= 1 always)"""
    rc = {"type": "roughconductor", "alpha": 0.3, "distribution": "ggx", "specular_reflectance": {"type": "rgb", "value": [0.9, 0.7, 0.5]}}
    df = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.4, 0.6, 0.7]}}
    blend = B.blended_box(mi, (16, 12), 4, (rc, df), end)
    pure = B.blended_box(mi, (16, 12), 4, (rc, df), end)
    pure["white"] = dict(rc if end == 0.0 else df)
    err, got, want = _host_vs_oracle(mi, O, blend, pure)
    print("host render, w = %g against the pure nested scene: rel L2 %.3g, (paths, vertices) %s vs %s" % (end, err, got, want))
    assert err <= 1e-4 and got == want and got[1] > got[0]


# ------------------------------------------------------------------------------------------------ 4. the loader

def test_loader_errors(mi):
    df = {"type": "diffuse"}
    with pytest.raises(RuntimeError, match="Cannot specify more than two child BSDFs"):
        mi.load_dict({"type": "blendbsdf", "weight": 0.5, "a": df, "b": df, "c": df})
    with pytest.raises(RuntimeError, match="Two child BSDFs must be specified"):
        mi.load_dict({"type": "blendbsdf", "weight": 0.5, "a": df})
    with pytest.raises(RuntimeError, match="weight"):
        mi.load_dict({"type": "blendbsdf", "a": df, "b": df})
    with pytest.raises(RuntimeError, match="Unreferenced property \"alpha\""):
        mi.load_dict({"type": "blendbsdf", "weight": 0.5, "a": df, "b": df, "alpha": 0.3})
    with pytest.raises(RuntimeError, match="Unreferenced property \"light\""):
        mi.load_dict({"type": "blendbsdf", "weight": 0.5, "a": df, "b": df, "light": {"type": "point"}})
    with pytest.raises(RuntimeError, match="nested BSDFs must be plain BSDF models in this variant"):
        mi.load_dict({"type": "blendbsdf", "weight": 0.5, "a": df, "b": {"type": "blendbsdf", "weight": 0.1, "x": df, "y": df}})
    with pytest.raises(RuntimeError, match="nested BSDFs must be plain BSDF models in this variant"):
        mi.load_dict({"type": "blendbsdf", "weight": 0.5, "a": df, "b": {"type": "twosided", "x": df}})
    with pytest.raises(RuntimeError, match="Only materials without a transmission component can be nested"):
        mi.load_dict({"type": "twosided", "n": {"type": "blendbsdf", "weight": 0.5, "a": df, "b": {"type": "dielectric"}}})
    with pytest.raises(RuntimeError, match="1 or 3"):
        mi.load_dict({"type": "blendbsdf", "weight": {"type": "bitmap", "data": np.zeros((2, 2, 4), np.float32)}, "a": df, "b": df})
    with pytest.raises(RuntimeError, match="not found"):
        mi.load_dict({"type": "blendbsdf", "weight": 0.5, "a": df, "b": {"type": "roughdielectric"}})


def test_record_validation(mi):
    """the C ABI refuses what the loader refuses: indices out of range, nested blends / twosided records, a transmitting nested BSDF under the twosided flag"""
    import ctypes as C
    from mitsuba3_amd import _capi
    L = mi.lib()

    def create(recs):
        arr = (_capi.HarBSDF * len(recs))()
        for i, r in enumerate(recs):
            arr[i].type = r.get("type", 0); arr[i].texture = -1; arr[i].flags = r.get("flags", 0); arr[i].back = -1; arr[i].eta = 1.5
            arr[i].nested = (C.c_int32 * 2)(*r.get("nested", (0, 0)))
        d = _capi.HarSceneDesc(); d.bsdfs = arr; d.bsdf_count = len(recs)
        v = np.zeros((3, 1), np.float32); uv = np.zeros((2, 1), np.float32); out = np.zeros((3, 1), np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        rc = L.har_bsdf_eval_pdf_host(C.byref(d), 0, None, 1, fp(v), fp(uv), fp(v), None, fp(out), None)
        return rc, (L.har_last_error() or b"").decode()

    assert create([dict(type=6, nested=(1, 2)), dict(), dict(type=2)])[0] == 0
    rc, msg = create([dict(type=6, nested=(1, 3)), dict(), dict()]); assert rc != 0 and "out of range" in msg
    rc, msg = create([dict(type=6, nested=(1, -1)), dict(), dict()]); assert rc != 0 and "out of range" in msg
    rc, msg = create([dict(type=6, nested=(1, 0)), dict()]); assert rc != 0 and "nested BSDFs must be plain BSDF models in this variant" in msg
    rc, msg = create([dict(type=6, nested=(1, 2)), dict(), dict(flags=1)]); assert rc != 0 and "nested BSDFs must be plain BSDF models in this variant" in msg
    rc, msg = create([dict(type=6, flags=1, nested=(1, 2)), dict(), dict(type=1)]); assert rc != 0 and "Only materials without a transmission component can be nested" in msg
    rc, msg = create([dict(type=7)]); assert rc != 0 and "unsupported BSDF type" in msg


def _plane_scene(mi, weight, a=None, wrap=None):
    d = {"type": "scene",
         "integrator": {"type": "path", "max_depth": 3},
         "sensor": {"type": "perspective", "fov": 40, "to_world": mi.ScalarTransform4f().look_at([0, 0, 3], [0, 0, 0], [0, 1, 0]),
                    "film": {"type": "hdrfilm", "width": 12, "height": 8}, "sampler": {"type": "independent", "sample_count": 4}},
         "mat": {"type": "blendbsdf", "weight": weight, "bsdf_a": a or {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.8, 0.3, 0.2]}},
                 "bsdf_b": {"type": "roughconductor", "alpha": 0.2}},
         "plane": {"type": "rectangle", "bsdf": {"type": "ref", "id": "mat"}},
         "light": {"type": "rectangle", "to_world": mi.ScalarTransform4f().translate([0, 0, 4]).rotate([1, 0, 0], 180), "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [9, 9, 9]}}}}
    if wrap:
        d["mat"] = {"type": "twosided", "inner": d["mat"]}
    return d


def _host_film(mi, scene, seed=1):
    from tests.thinlens_cases import host_render
    return host_render(mi, scene, scene.sensors()[0], seed, 4, 3)


def test_traverse_names_and_update(mi):
    import torch
    scene = mi.load_dict(_plane_scene(mi, 0.3))
    p = mi.traverse(scene)
    assert {"mat.weight.value", "mat.bsdf_0.reflectance.value", "mat.bsdf_1.specular_reflectance.value", "mat.bsdf_1.alpha.value", "mat.bsdf_1.eta.value"} <= set(p.keys())
    assert tuple(p["mat.weight.value"].shape) == (1,) and abs(float(p["mat.weight.value"][0]) - 0.3) < 1e-7
    tex = np.random.default_rng(2).uniform(0.1, 0.9, (4, 6, 1)).astype(np.float32)
    scene1 = mi.load_dict(_plane_scene(mi, {"type": "bitmap", "data": tex, "raw": True, "to_uv": mi.ScalarTransform3f().scale([2.0, 1.0])}))
    p1 = mi.traverse(scene1)
    assert tuple(p1["mat.weight.data"].shape) == (4, 6, 1) and "mat.weight.to_uv" in p1 and np.array_equal(p1["mat.weight.data"].cpu().numpy(), tex)
    tex3 = np.random.default_rng(3).uniform(0.1, 0.9, (4, 6, 3)).astype(np.float32)
    p3 = mi.traverse(mi.load_dict(_plane_scene(mi, {"type": "bitmap", "data": tex3, "raw": True})))
    assert tuple(p3["mat.weight.data"].shape) == (4, 6, 3)
    two = mi.load_dict(_plane_scene(mi, 0.3, wrap=True))
    pt = mi.traverse(two)
    assert {"mat.brdf_0.weight.value", "mat.brdf_0.bsdf_0.reflectance.value", "mat.brdf_0.bsdf_1.alpha.value"} <= set(pt.keys())
    assert two.bsdf_objs[0].component_count() == 4
    # update() of the weight, of a weight bitmap and of a nested colour gives the scene a fresh load gives: the same host render, bit for bit
    p["mat.weight.value"] = torch.tensor([0.65]); p["mat.bsdf_0.reflectance.value"] = torch.tensor([0.1, 0.7, 0.4]); p.update()
    fresh = mi.load_dict(_plane_scene(mi, 0.65, a={"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.1, 0.7, 0.4]}}))
    a, b = _host_film(mi, scene), _host_film(mi, fresh)
    assert np.array_equal(a, b) and np.abs(a[..., :3]).sum() > 0
    assert not np.array_equal(a, _host_film(mi, mi.load_dict(_plane_scene(mi, 0.3))))
    tex_new = (1.0 - tex).astype(np.float32)
    p1["mat.weight.data"] = torch.tensor(tex_new); p1.update()
    fresh1 = mi.load_dict(_plane_scene(mi, {"type": "bitmap", "data": tex_new, "raw": True, "to_uv": mi.ScalarTransform3f().scale([2.0, 1.0])}))
    assert np.array_equal(_host_film(mi, scene1), _host_film(mi, fresh1))
    with pytest.raises(RuntimeError, match="expected"):
        p["mat.weight.value"] = torch.tensor([0.1, 0.2, 0.3]); p.update()


def test_xml_equals_dict(mi, tmp_path):
    xml = """<scene version="3.0.0">
  <integrator type="path"><integer name="max_depth" value="3"/></integrator>
  <sensor type="perspective"><float name="fov" value="40"/>
    <transform name="to_world"><lookat origin="0, 0, 3" target="0, 0, 0" up="0, 1, 0"/></transform>
    <film type="hdrfilm"><integer name="width" value="12"/><integer name="height" value="8"/></film>
    <sampler type="independent"><integer name="sample_count" value="4"/></sampler></sensor>
  <bsdf type="blendbsdf" id="mat"><float name="weight" value="0.3"/>
    <bsdf type="diffuse" name="bsdf_a"><rgb name="reflectance" value="0.8, 0.3, 0.2"/></bsdf>
    <bsdf type="roughconductor" name="bsdf_b"><float name="alpha" value="0.2"/></bsdf></bsdf>
  <shape type="rectangle" id="plane"><ref id="mat"/></shape>
  <shape type="rectangle" id="light"><transform name="to_world"><rotate x="1" angle="180"/><translate x="0" y="0" z="4"/></transform>
    <emitter type="area"><rgb name="radiance" value="9, 9, 9"/></emitter></shape>
</scene>"""
    f = tmp_path / "blend.xml"; f.write_text(xml)
    a = mi.load_file(str(f)); b = mi.load_dict(_plane_scene(mi, 0.3))
    assert [o.kind for o in a.bsdf_objs if o.kind in ("blendbsdf", "diffuse", "roughconductor")][:3] == ["blendbsdf", "diffuse", "roughconductor"]
    fa, fb = _host_film(mi, a), _host_film(mi, b)
    assert np.abs(fb[..., :3]).sum() > 0 and np.allclose(fa, fb, rtol=1e-6, atol=1e-7)
