"""Shared cases of the `mask` tests (test_mask_cpu.py, test_gpu_mask.py): the nested models, the opacities, the contexts, src/bsdfs/mask.cpp restated in NumPy float32
over the oracle's answers for the nested BSDF (OracleScene.bsdf_evaluate_ctx / bsdf_sample_ctx of a scene that holds the nested BSDF alone; the opacity from the
independent float64 lookup of tests/blend_cases.py), and the render scenes: a card of K x K quads whose texcoords put each quad strictly inside one texel of a K x K
nearest opacity bitmap, so that a scene with binary opacities has an oracle twin with the same geometry -- the nested BSDF where the texel is 1, a `dielectric` with
int_ior == ext_ior where it is 0 (reflectance 0, the ray goes straight through with weight, pdf and eta 1, a delta lobe: oracle/orc_bsdf.h)."""
import ctypes as C

import numpy as np

from tests import blend_cases as B

ALL = B.ALL
NULL = 0x1
COUNT = B.COUNT

NESTED = {
    "diffuse": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.2, 0.5, 0.8]}},
    "roughconductor": {"type": "roughconductor", "distribution": "ggx", "alpha_u": 0.1, "alpha_v": 0.3, "specular_reflectance": {"type": "rgb", "value": [0.9, 0.8, 0.7]}},
    "plastic": {"type": "plastic", "diffuse_reflectance": {"type": "rgb", "value": [0.1, 0.27, 0.36]}, "int_ior": 1.9},
    "dielectric": {"type": "dielectric", "specular_reflectance": 0.3, "specular_transmittance": 0.6, "int_ior": 1.5, "ext_ior": 1.0},
    "twosided(diffuse)": {"type": "twosided", "inner": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.6, 0.6, 0.2]}}},
    "twosided(diffuse,roughplastic)": {"type": "twosided", "front": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.3, 0.4]}},
                                       "rear": {"type": "roughplastic", "diffuse_reflectance": {"type": "rgb", "value": [0.7, 0.3, 0.1]}, "alpha": 0.15}},
}
NESTED_NAMES = list(NESTED)
OPACITY_NAMES = B.WEIGHT_NAMES            # the constant (0.35), the three-channel bilinear bitmap with to_uv, the one-channel nearest bitmap with texels below 0 and above 1


def nested_dict(name):
    d = NESTED[name]
    return {k: (dict(v) if isinstance(v, dict) else v) for k, v in d.items()}


def null_index(name):
    """component_count of the nested BSDF (twosided.cpp:89-100: the front BSDF's components, then the back's -- twice the same with one nested BSDF)"""
    d = NESTED[name]
    if d["type"] != "twosided":
        return COUNT[d["type"]]
    kids = [v for k, v in d.items() if isinstance(v, dict)]
    return COUNT[kids[0]["type"]] + COUNT[kids[-1]["type"]]


def mask_dict(mi, nested, opacity):
    return {"type": "mask", "opacity": B.weight_prop(mi, opacity) if isinstance(opacity, str) else opacity, "material": nested_dict(nested)}


def contexts(nested):
    """(mode, type_mask, component): default, the null component, component 0, a type mask without Null, a type mask of Null only"""
    return [(0, 0x1ff, ALL), (0, 0x1ff, null_index(nested)), (0, 0x1ff, 0), (0, 0x1ff & ~NULL, ALL), (0, NULL, ALL)]


def is_enabled(ctx, type_, comp):
    """BSDFContext::is_enabled (bsdf.h:177-181)"""
    return (ctx[1] == ALL or (ctx[1] & type_) == type_) and (ctx[2] == ALL or ctx[2] == comp)


class Nested:
    """the nested BSDF alone in an oracle scene (the oracle resolves a `twosided` record itself), with its eval answers cached"""

    def __init__(self, mi, O, name):
        self.name = name; self.null_index = null_index(name)
        obj = mi.load_dict(nested_dict(name))
        self.scene = mi.core.Scene({"c0": obj}); self.index = obj.index
        self.osc, _ = O.scene_from_product(self.scene)
        self._eval = {}

    def eval_pdf(self, ctx, wi, uv, wo):
        key = (ctx, ) + tuple((a.shape, a.tobytes()) for a in (wi, uv, wo))
        if key not in self._eval:
            self._eval[key] = self.osc.bsdf_evaluate_ctx(self.index, ctx, 2, wi, uv, wo)
        return self._eval[key]

    def sample(self, ctx, wi, uv, s1, s2):
        return self.osc.bsdf_sample_ctx(self.index, ctx, wi, uv, s1, s2)


def expected_eval_pdf(ch, ctx, o, wi, uv, wo):
    """MaskBSDF::eval_pdf (mask.cpp:195-217) in float32 over the nested BSDF's oracle answers: (value 3 x n, pdf n, un-mixed nested value)"""
    f = np.float32
    transmission = is_enabled(ctx, NULL, ch.null_index)
    nested = ctx[2] == ALL or ctx[2] < ch.null_index
    val, pdf = ch.eval_pdf(ctx, wi, uv, wo)
    o = o.astype(f)
    value = (val * o[None, :]).astype(f)
    if not nested:
        pdf = np.zeros_like(pdf)
    elif transmission:
        pdf = (pdf * o).astype(f)
    return value, pdf, val


def expected_sample(ch, ctx, o, wi, uv, s1, s2):
    """MaskBSDF::sample (mask.cpp:121-167) in float32 over the nested BSDF's oracle answers: dict as OracleScene.bsdf_sample_ctx returns it, plus `null` (the lanes
    that took the null lobe)"""
    f = np.float32
    n = s1.size
    out = dict(wo=np.zeros((3, n), f), pdf=np.zeros(n, f), weight=np.zeros((3, n), f), eta=np.zeros(n, f), sampled_type=np.zeros(n, np.uint32),
               sampled_component=np.zeros(n, np.uint32), null=np.zeros(n, bool))
    transmission = is_enabled(ctx, NULL, ch.null_index)
    nested = ctx[2] == ALL or ctx[2] < ch.null_index
    if not transmission and not nested:
        return out
    o = o.astype(f).copy()
    if transmission != nested:
        o[:] = f(1) if transmission else f(0)
    take = s1 < o
    out["null"] = ~take
    out["wo"][:, ~take] = -wi[:, ~take]; out["pdf"][~take] = (f(1) - o[~take]).astype(f); out["weight"][:, ~take] = f(1); out["eta"][~take] = f(1)
    out["sampled_type"][~take] = NULL; out["sampled_component"][~take] = ch.null_index
    if take.any():
        r = ch.sample(ctx, wi[:, take], uv[:, take], (s1[take] / o[take]).astype(f), s2[:, take])
        for key in ("wo", "weight"):
            out[key][:, take] = r[key]
        for key in ("eta", "sampled_type", "sampled_component"):
            out[key][take] = r[key]
        out["pdf"][take] = (r["pdf"] * o[take]).astype(f)
    return out


# ---- the render scenes

K = 4
ABSENT = {"type": "dielectric", "int_ior": 1.0, "ext_ior": 1.0}          # the oracle's absent surface: the index-matched branch (oracle/orc_bsdf.h:38)
DIFFUSE = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.8, 0.3, 0.2]}}
TWOSIDED = {"type": "twosided", "inner": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.25, 0.5, 0.75]}}}


def binary_texels(seed=11, k=K):
    """K x K texels of 0 and 1 (both present)"""
    t = (np.random.default_rng(seed).random((k, k)) < 0.5).astype(np.float32)
    t[0, 0] = 0.0; t[k - 1, k - 1] = 1.0
    return t[:, :, None]


def card_quads(z, half=0.62, k=K, tilt=0.0):
    """the K x K quads of a card in the plane z (normal +z, tilted about the y axis by `tilt` radians): [(positions 4 x 3, faces 2 x 3, texcoords 4 x 2, (row, column))];
    the texcoords of quad (row j, column i) lie strictly inside texel (j, i) of a K x K bitmap"""
    out = []
    c, s = np.cos(tilt), np.sin(tilt)
    for j in range(k):
        for i in range(k):
            x0, x1 = -half + 2 * half * i / k, -half + 2 * half * (i + 1) / k
            y0, y1 = -half + 2 * half * j / k, -half + 2 * half * (j + 1) / k
            P = np.array([[x0, y0, 0], [x1, y0, 0], [x1, y1, 0], [x0, y1, 0]], np.float64)
            P = np.stack([P[:, 0] * c, P[:, 1], z - P[:, 0] * s], 1).astype(np.float32)
            u0, u1 = (i + 0.25) / k, (i + 0.75) / k; v0, v1 = (j + 0.25) / k, (j + 0.75) / k
            uv = np.array([[u0, v0], [u1, v0], [u1, v1], [u0, v1]], np.float32)
            out.append((P, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), uv, (j, i)))
    return out


def card_scene(mi, res, spp, texels, nested, product, integrator="path", max_depth=6, rr_depth=7, layers=(0.55, ), instanced=False, separate=False, opacity=None, hide_emitters=False):
    """mi.cornell_box() with cut-out cards (K x K quad meshes each) in front of the boxes.  product: every quad carries ONE `mask` (the nearest opacity bitmap `texels`, or
    `opacity` if given: a float or a bitmap property) over `nested`; otherwise (the oracle's twin) quad (j, i) carries `nested` where texels[j, i] == 1 and the absent
    surface where it is 0.  `separate`: every quad of the product carries a mask record of ITS OWN, 'cut_<j>_<i>', with the constant opacity texels[j, i] -- the same surface as the
    nearest bitmap gives, with one scalar parameter per texel (gradient test (d))."""
    d = mi.cornell_box()
    d["sensor"]["film"]["width"] = res[0]; d["sensor"]["film"]["height"] = res[1]
    d["sensor"]["sampler"] = {"type": "independent", "sample_count": spp}
    d["integrator"] = {"type": integrator, "max_depth": max_depth, "rr_depth": rr_depth}
    if hide_emitters:
        d["integrator"]["hide_emitters"] = True
    tex = np.asarray(texels, np.float32)
    if product and not separate:
        op = opacity if opacity is not None else {"type": "bitmap", "data": tex, "raw": True, "filter_type": "nearest"}
        d["cut"] = {"type": "mask", "opacity": op, "material": dict(nested)}
    if not product:
        d["solid"] = dict(nested)
    if not product:
        d["absent"] = dict(ABSENT)
    shapes = {}
    for li, z in enumerate(layers):
        for P, F, uv, (j, i) in card_quads(z, tilt=0.15 * li):
            if product and separate:
                ref = "cut_%d_%d" % (j, i)
                d[ref] = {"type": "mask", "opacity": float(tex[j, i, 0]), "material": dict(nested)}
            elif product:
                ref = "cut"
            else:
                ref = "solid" if tex[j, i, 0] >= 0.5 else "absent"
            shapes["card%d_%d_%d" % (li, j, i)] = {"type": "mesh", "faces": F, "positions": P, "texcoords": uv, "bsdf": {"type": "ref", "id": ref}}
    if instanced:
        group = {"type": "shapegroup"}; group.update(shapes)
        d["cards"] = group
        d["placed"] = {"type": "instance", "g": {"type": "ref", "id": "cards"}}
    else:
        d.update(shapes)
    return d


def lit_card(mi, bsdf, spp, res=(16, 16), max_depth=3, rr_depth=8, integrator="path"):
    """one planar rectangle carrying `bsdf` over a diffuse floor, lit by an area light: the scene of the statistical test"""
    T = mi.ScalarTransform4f
    return {"type": "scene",
            "integrator": {"type": integrator, "max_depth": max_depth, "rr_depth": rr_depth},
            "sensor": {"type": "perspective", "fov": 35, "to_world": T().look_at([0, -2.2, 1.6], [0, 0, 0.3], [0, 0, 1]),
                       "film": {"type": "hdrfilm", "width": res[0], "height": res[1], "rfilter": {"type": "box"}}, "sampler": {"type": "independent", "sample_count": spp}},
            "mat": bsdf,
            "card": {"type": "rectangle", "to_world": T().translate([0, 0, 0.5]).scale([0.8, 0.8, 1.0]), "bsdf": {"type": "ref", "id": "mat"}},
            # (the floor catches every ray that passes through the card: a null-sampled path that escaped would be an INVALID sample, whose emitter sample at the card is
            # dropped with it -- path.cpp:341-345 -- and the expectation below would not be linear in the opacity)
            "floor": {"type": "rectangle", "to_world": T().scale([8.0, 8.0, 1.0]), "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.3, 0.6, 0.4]}}},
            "light": {"type": "rectangle", "to_world": T().translate([0.3, 0.9, 1.6]).rotate([1, 0, 0], 140).scale([0.5, 0.5, 1.0]),
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [12, 10, 8]}}}}


def two_layers(mi, o1, o2, integrator="path", max_depth=8, film=None, spp=4):
    """two parallel mask rectangles (opacities o1, o2, nested diffuse) facing +z at z = 0 and z = -1, nothing behind them, no environment, a light off to the side"""
    T = mi.ScalarTransform4f
    d = {"type": "scene",
         "integrator": {"type": integrator, "max_depth": max_depth, "rr_depth": 64},
         "m1": {"type": "mask", "opacity": o1, "n": dict(DIFFUSE)}, "m2": {"type": "mask", "opacity": o2, "n": dict(DIFFUSE)},
         "r1": {"type": "rectangle", "to_world": T().scale([4.0, 4.0, 1.0]), "bsdf": {"type": "ref", "id": "m1"}},
         "r2": {"type": "rectangle", "to_world": T().translate([0, 0, -1.0]).scale([4.0, 4.0, 1.0]), "bsdf": {"type": "ref", "id": "m2"}},
         "light": {"type": "rectangle", "to_world": T().translate([6.0, 0, 2.0]).rotate([0, 1, 0], -120).scale([0.5, 0.5, 1.0]),
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [30, 30, 30]}}}}
    if film is not None:
        d["sensor"] = {"type": "perspective", "fov": 40, "to_world": T().look_at([0, 0, 3], [0, 0, 0], [0, 1, 0]),
                       "film": dict({"type": "hdrfilm", "width": 16, "height": 12, "pixel_format": "rgba"}, **film), "sampler": {"type": "independent", "sample_count": spp}}
    return d


def stream_draws(O, state, inc, count):
    """(the first `count` floats of the pcg32 stream (state, inc), the state after them): orc_pcg32_next_float32"""
    L = O.lib()
    si = (C.c_uint64 * 2)(int(state), int(inc))
    vals = np.array([L.orc_pcg32_next_float32(si) for _ in range(count)], np.float32)
    return vals, int(si[0])


def lane_seeds(O, seed, n):
    """(state, inc) of lanes 0..n-1 after Sampler::seed(seed, n) (sampler.cpp:129-148): orc_sample_tea_32 + orc_pcg32_seed"""
    L = O.lib()
    v = (C.c_uint32 * 2)(); si = (C.c_uint64 * 2)()
    state = np.zeros(n, np.uint64); inc = np.zeros(n, np.uint64)
    for i in range(n):
        L.orc_sample_tea_32(seed, i, 4, v); L.orc_pcg32_seed(v[0], v[1], si)
        state[i] = si[0]; inc[i] = si[1]
    return state, inc


# ---- partial opacity, statistically (check 3): shared by the host and the device test

OPACITY = 0.4


def oracle_pure_batches(mi, O, spp_b=64, batches=24):
    """oracle batches of the two pure scenes of lit_card (the nested BSDF on the card, the absent surface on the card): ([batches x H x W x 3] * 2, spp_b, batches)"""
    out = []
    for k, b in enumerate((DIFFUSE, ABSENT)):
        osc, sensor = O.scene_from_product(mi.load_dict(lit_card(mi, dict(b), spp_b)))
        out.append(np.stack([osc.render_path(sensor, seed=1000 + 50 * k + s, spp=spp_b, max_depth=3, rr_depth=8)[0].astype(np.float64) for s in range(batches)]))
    return out, spp_b, batches


def statistics_verdicts(img, spp, pure, wrong=0.55):
    """(accepted at OPACITY, min p, alpha, accepted at the visibly wrong opacity, its min p).  One planar mask rectangle, max_depth 3, no roulette: every path has at most
    one opacity-dependent vertex -- after the card a path needs two more bounces to come back to it (floor, then something above the card: there is only the light,
    which ends it), so E[I] = o I(nested) + (1 - o) I(absent).  The per-sample variance is bounded by that of the estimator that picks one of the two pure estimators
    with probabilities (o, 1 - o): o v0 + (1 - o) v1 + o (1 - o) (m0 - m1)^2."""
    from tests import ztest
    (b0, b1), spp_b, batches = pure
    m0, m1 = b0.mean(0), b1.mean(0); v0, v1 = b0.var(0, ddof=1) * spp_b, b1.var(0, ddof=1) * spp_b
    n_ref = spp_b * batches

    def verdict(o):
        mean = o * m0 + (1 - o) * m1; var = o * v0 + (1 - o) * v1 + o * (1 - o) * (m0 - m1) ** 2
        return ztest.accept(img, spp, mean, var, n_ref)

    ok, pmin, alpha = verdict(OPACITY); bad, pmin_bad, _ = verdict(wrong)
    return ok, pmin, alpha, bad, pmin_bad
