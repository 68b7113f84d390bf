"""Shared cases of the `thindielectric` tests (test_thindielectric_cpu.py, test_gpu_thindielectric.py): src/bsdfs/thindielectric.cpp:142-201 restated in NumPy float32 in
its order of operations over the oracle's fresnel() (orc_fresnel), the (wi, uv, wo, sample1, sample2) tuples, an independent float64 lookup of a bitmap transmittance,
stand-ins for the nested BSDFs of tests/mask_cases.py / tests/blend_cases.py that answer for the thin leaf, and the render scenes: the card of tests/mask_cases.py in the
Cornell box carrying ONE material, and a box cut into two chambers by a pane."""
import ctypes as C

import numpy as np

from tests import blend_cases as B
from tests import mask_cases as M

ALL = B.ALL
NULL, DELTA_REFLECTION = 0x1, 0x20
F32 = np.float32
BK7_AIR = float(F32(1.5046) / F32(1.000277))
ETAS = {"bk7/air": BK7_AIR, "air/bk7": float(F32(1.000277) / F32(1.5046)), "one": 1.0, "diamond": 2.419}
ETA_PROPS = {"bk7/air": {}, "air/bk7": {"int_ior": "air", "ext_ior": "bk7"}, "one": {"int_ior": 1.3, "ext_ior": 1.3}, "diamond": {"int_ior": 2.419, "ext_ior": 1.0}}
T_RGB = np.array([0.2, 0.5, 0.9], F32)
R_RGB = np.array([0.7, 0.6, 0.3], F32)
COLOURS = ["none", "constants", "bitmap_bilinear_to_uv", "bitmap_nearest"]
# (mode, type_mask, component): default, component 0, component 1, DeltaReflection only, Null only, neither, TransportMode::Importance
CONTEXTS = [(0, 0x1ff, ALL), (0, 0x1ff, 0), (0, 0x1ff, 1), (0, DELTA_REFLECTION, ALL), (0, NULL, ALL), (0, 0x2, ALL), (1, 0x1ff, ALL)]


def nearest_texels(k=M.K, seed=17):
    """K x K x 3 texels in [0.1, 0.9]: one texel per quad of the card of tests/mask_cases.py"""
    return np.random.default_rng(seed).uniform(0.1, 0.9, (k, k, 3)).astype(F32)


def colour_props(mi, colour):
    """the two optional colour properties of a case"""
    if colour == "none":
        return {}
    out = {"specular_reflectance": {"type": "rgb", "value": [float(x) for x in R_RGB]}}
    if colour == "constants":
        out["specular_transmittance"] = {"type": "rgb", "value": [float(x) for x in T_RGB]}
    elif colour == "bitmap_bilinear_to_uv":
        m = np.eye(3); m[:2, :] = B.TO_UV
        out["specular_transmittance"] = {"type": "bitmap", "data": B._bitmap3(), "raw": True, "to_uv": mi.ScalarTransform3f(m)}
    else:
        out["specular_transmittance"] = {"type": "bitmap", "data": nearest_texels(), "raw": True, "filter_type": "nearest"}
    return out


def thin_dict(mi, eta="bk7/air", colour="none"):
    d = {"type": "thindielectric"}
    d.update(ETA_PROPS[eta]); d.update(colour_props(mi, colour))
    return d


def lookup_colour(colour, uv):
    """(T 3 x n or None, R 3 x n or None) by an independent lookup: the texel coordinates in float32 as the texture unit forms them, the interpolation in float64 on a
    np.pad'ed image (the lookup of tests/blend_cases.py::lookup_weight, returning the colour instead of its luminance)"""
    n = uv.shape[1]
    if colour == "none":
        return None, None
    R = np.repeat(R_RGB[:, None], n, 1)
    if colour == "constants":
        return np.repeat(T_RGB[:, None], n, 1), R
    bilinear = colour == "bitmap_bilinear_to_uv"
    tex = B._bitmap3() if bilinear else nearest_texels()
    Hh, Ww = tex.shape[:2]; P = 12
    big = np.pad(tex, ((P * Hh, P * Hh), (P * Ww, P * Ww), (0, 0)), mode="wrap").astype(np.float64)
    out = np.zeros((3, n), np.float64)
    t = lambda x, y: big[y + P * Hh, x + P * Ww]
    for i in range(n):
        u, v = F32(uv[0, i]), F32(uv[1, i])
        if bilinear:
            m = B.TO_UV.astype(F32)
            u, v = B._fma32(m[0, 1], v, B._fma32(m[0, 0], u, m[0, 2])), B._fma32(m[1, 1], v, B._fma32(m[1, 0], u, m[1, 2]))
            px, py = B._fma32(u, Ww, -0.5), B._fma32(v, Hh, -0.5)
            x0, y0 = int(np.floor(px)), int(np.floor(py)); fx, fy = float(px - F32(x0)), float(py - F32(y0))
            out[:, i] = (1 - fy) * ((1 - fx) * t(x0, y0) + fx * t(x0 + 1, y0)) + fy * ((1 - fx) * t(x0, y0 + 1) + fx * t(x0 + 1, y0 + 1))
        else:
            out[:, i] = t(int(np.floor(u * F32(Ww))), int(np.floor(v * F32(Hh))))
    return out.astype(F32), R


def fresnel_r(O, cos_abs, eta):
    """fresnel(cos_theta_i, eta)[0] of the oracle, lane by lane"""
    L = O.lib(); L.orc_fresnel.argtypes = [C.c_float, C.c_float, O.c_f32p]
    c = np.asarray(cos_abs, F32).reshape(-1); out = np.empty(c.size, F32); o = np.empty(4, F32)
    for i in range(c.size):
        L.orc_fresnel(C.c_float(c[i]), C.c_float(eta), O.fp(o)); out[i] = o[0]
    return out


def r_prime(O, cos_theta_i, eta):
    """thindielectric.cpp:152-155: r = fresnel(|cos theta_i|, eta)[0]; r *= 2 / (1 + r), float32, IEEE division"""
    r = fresnel_r(O, np.abs(np.asarray(cos_theta_i, F32)), eta)
    return (r * (F32(2) / (F32(1) + r)).astype(F32)).astype(F32)


def is_enabled(ctx, type_, comp):
    return M.is_enabled(ctx, type_, comp)


def expected_sample(ctx, rp, T, R, wi, s1):
    """ThinDielectric::sample (thindielectric.cpp:142-191) in float32: dict as OracleScene.bsdf_sample_ctx returns it, plus `reflect` (the lanes that took lobe 0).
    rp = r' per lane; T / R = the colours per lane (3 x n) or None where the property was not given"""
    n = s1.size
    out = dict(wo=np.zeros((3, n), F32), pdf=np.zeros(n, F32), weight=np.zeros((3, n), F32), eta=np.zeros(n, F32), sampled_type=np.zeros(n, np.uint32),
               sampled_component=np.zeros(n, np.uint32), reflect=np.zeros(n, bool))
    has_r = is_enabled(ctx, DELTA_REFLECTION, 0); has_t = is_enabled(ctx, NULL, 1)
    if not has_r and not has_t:
        return out
    rp = rp.astype(F32); t = (F32(1) - rp).astype(F32)
    if has_r and has_t:
        sel = s1 <= rp; w = np.ones(n, F32); pdf = np.where(sel, rp, t).astype(F32)
    else:
        sel = np.full(n, has_r); w = (rp if has_r else t).copy(); pdf = np.ones(n, F32)
    out["reflect"] = sel; out["pdf"] = pdf
    out["wo"] = np.where(sel[None, :], np.stack([-wi[0], -wi[1], wi[2]]), -wi).astype(F32)
    out["eta"][:] = 1; out["sampled_component"] = np.where(sel, 0, 1).astype(np.uint32); out["sampled_type"] = np.where(sel, DELTA_REFLECTION, NULL).astype(np.uint32)
    weight = np.repeat(w[None, :], 3, 0)
    if R is not None:
        weight = np.where(sel[None, :], (weight * R).astype(F32), weight)
    if T is not None:
        weight = np.where(sel[None, :], weight, (weight * T).astype(F32))
    out["weight"] = weight.astype(F32)
    return out


_TUPLES = {}


def tuples(O, eta_name, n=20000, seed=7):
    """n tuples (wi 3 x n, uv 2 x n, wo 3 x n, sample1 n, sample2 2 x n, r' n): wi over the whole sphere (both sides), an eighth grazing (|z| < 0.02), a sixteenth exactly
    normal (0, 0, +-1), a sixteenth with wi.z == 0 exactly (r' = 1, or 0 at eta == 1); an eighth with sample1 at 0, at r', one float below and above it, one float below 1"""
    key = (eta_name, n, seed)
    if key in _TUPLES:
        return _TUPLES[key]
    rng = np.random.default_rng(seed)
    k = np.arange(n)

    def sphere(grazing):
        z = rng.uniform(-1, 1, n)
        z[grazing] = rng.uniform(-0.02, 0.02, int(grazing.sum()))
        ph = rng.uniform(0, 2 * np.pi, n); r = np.sqrt(1 - z * z)
        return np.stack([r * np.cos(ph), r * np.sin(ph), z]).astype(F32), ph

    wi, ph = sphere(k % 8 == 1); wo, _ = sphere(k % 8 == 2)
    normal = k % 16 == 5; flat = k % 16 == 13
    wi[:, normal] = np.stack([np.zeros(int(normal.sum())), np.zeros(int(normal.sum())), np.where(rng.random(int(normal.sum())) < 0.5, -1.0, 1.0)]).astype(F32)
    wi[:, flat] = np.stack([np.cos(ph[flat]), np.sin(ph[flat]), np.zeros(int(flat.sum()))]).astype(F32)
    uv = rng.uniform(-1.5, 2.5, (2, n)).astype(F32)
    rp = r_prime(O, wi[2], ETAS[eta_name])
    s1 = rng.random(n).astype(F32)
    one_below = np.nextafter(F32(1), F32(0))
    for j, i in enumerate(np.nonzero(k % 8 == 3)[0]):
        s1[i] = (F32(0), rp[i], np.nextafter(rp[i], F32(-1)), np.nextafter(rp[i], F32(2)), one_below)[j % 5]
    s1 = np.clip(s1, F32(0), one_below)
    s2 = rng.random((2, n)).astype(F32)
    _TUPLES[key] = (wi, uv, wo, s1, s2, rp)
    return _TUPLES[key]


class ThinNested:
    """what tests/mask_cases.py::Nested is for an oracle BSDF, for the thin leaf: the restatement above answers (eval and pdf are zero)"""
    null_index = 2

    def __init__(self, O, eta_name, T=None, R=None):
        self.O = O; self.eta = ETAS[eta_name]; self.T = T; self.R = R

    def eval_pdf(self, ctx, wi, uv, wo):
        n = wo.shape[1]
        return np.zeros((3, n), F32), np.zeros(n, F32)

    def sample(self, ctx, wi, uv, s1, s2):
        n = s1.size
        col = lambda c: None if c is None else np.repeat(np.asarray(c, F32)[:, None], n, 1)
        r = expected_sample(ctx, r_prime(self.O, wi[2], self.eta), col(self.T), col(self.R), wi, s1)
        r.pop("reflect")
        return r


class BlendChildren:
    """what tests/blend_cases.py::Children is for two oracle BSDFs, with the thin leaf as child 0 and an oracle BSDF as child 1"""
    two = False; n0 = 2

    def __init__(self, mi, O, eta_name, other, T=None, R=None):
        self.thin = ThinNested(O, eta_name, T, R)
        obj = mi.load_dict(dict(other))
        self.scene = mi.core.Scene({"c1": obj}); self.other = obj.index
        self._osc, _ = O.scene_from_product(self.scene)
        self.osc = self

    def bsdf_evaluate_ctx(self, k, ctx, what, wi, uv, wo):
        return self.thin.eval_pdf(ctx, wi, uv, wo) if k == 0 else self._osc.bsdf_evaluate_ctx(self.other, ctx, what, wi, uv, wo)

    def eval_pdf(self, k, ctx, wi, uv, wo):
        return self.bsdf_evaluate_ctx(k, ctx, 2, wi, uv, wo)

    def sample(self, k, ctx, wi, uv, s1, s2):
        return self.thin.sample(ctx, wi, uv, s1, s2) if k == 0 else self._osc.bsdf_sample_ctx(self.other, ctx, wi, uv, s1, s2)


# ---- the render scenes

INDEX_MATCHED = {"type": "thindielectric", "int_ior": 1.3, "ext_ior": 1.3}
MASK_ZERO = {"type": "mask", "opacity": 0.0, "material": dict(M.DIFFUSE)}
ABSORBING = {"type": "thindielectric", "specular_transmittance": {"type": "rgb", "value": [0, 0, 0]}, "specular_reflectance": {"type": "rgb", "value": [0, 0, 0]}}


def card_scene(mi, res, spp, material, integrator="path", max_depth=6, rr_depth=7, instanced=False, film=None, frame=None):
    """mi.cornell_box() with the card of tests/mask_cases.py (K x K quads, in front of the boxes: every ray that passes the card meets a wall or a box) carrying ONE
    `material`.  frame = K x K binary texels: the card carries a `mask` with that nearest opacity bitmap over `material` (a window with a cut-out frame)"""
    d = mi.cornell_box()
    d["sensor"]["film"]["width"] = res[0]; d["sensor"]["film"]["height"] = res[1]
    if film:
        d["sensor"]["film"].update(film)
    d["sensor"]["sampler"] = {"type": "independent", "sample_count": spp}
    d["integrator"] = {"type": integrator, "max_depth": max_depth, "rr_depth": rr_depth}
    d["pane"] = dict(material) if frame is None else {"type": "mask", "opacity": {"type": "bitmap", "data": np.asarray(frame, F32), "raw": True, "filter_type": "nearest"}, "material": dict(material)}
    shapes = {}
    for P, Fa, uv, (j, i) in M.card_quads(0.55):
        shapes["card_%d_%d" % (j, i)] = {"type": "mesh", "faces": Fa, "positions": P, "texcoords": uv, "bsdf": {"type": "ref", "id": "pane"}}
    if instanced:
        group = {"type": "shapegroup"}; group.update(shapes)
        d["cards"] = group
        d["placed"] = {"type": "instance", "g": {"type": "ref", "id": "cards"}}
    else:
        d.update(shapes)
    return d


def two_panes(mi, pane1, pane2, integrator="path", max_depth=8, film=None, spp=4, emitter=None):
    """two parallel rectangles carrying `pane1` / `pane2` at z = 0 and z = -1, nothing behind them; a light off to the side, or `emitter` (an environment)"""
    T = mi.ScalarTransform4f
    d = {"type": "scene",
         "integrator": {"type": integrator, "max_depth": max_depth, "rr_depth": 64},
         "m1": dict(pane1), "m2": dict(pane2),
         "r1": {"type": "rectangle", "to_world": T().scale([4.0, 4.0, 1.0]), "bsdf": {"type": "ref", "id": "m1"}},
         "r2": {"type": "rectangle", "to_world": T().translate([0, 0, -1.0]).scale([4.0, 4.0, 1.0]), "bsdf": {"type": "ref", "id": "m2"}}}
    if emitter is not None:
        d["env"] = dict(emitter)
    else:
        d["light"] = {"type": "rectangle", "to_world": T().translate([6.0, 0, 2.0]).rotate([0, 1, 0], -120).scale([0.5, 0.5, 1.0]),
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [30, 30, 30]}}}
    if film is not None:
        d["sensor"] = {"type": "perspective", "fov": 40, "to_world": T().look_at([0, 0, 3], [0, 0, 0], [0, 1, 0]),
                       "film": dict({"type": "hdrfilm", "width": 16, "height": 12, "pixel_format": "rgba"}, **film), "sampler": {"type": "independent", "sample_count": spp}}
    return d


def chambers(mi, pane, res=(32, 24), spp=16, integrator="prb", max_depth=3, rr_depth=8, tex_seed=31):
    """a closed box cut into two chambers by ONE pane that spans the whole cross-section (z = 0).  Chamber B (z > 0) holds the camera and a light, chamber A (z < 0) a
    light, a roughconductor block and the bitmap-textured back wall `wall_a`; `pane` = None removes the pane"""
    T = mi.ScalarTransform4f
    rng = np.random.default_rng(tex_seed)
    tex = lambda h, w: {"type": "diffuse", "reflectance": {"type": "bitmap", "data": rng.uniform(0.2, 0.8, (h, w, 3)).astype(F32), "raw": True}}
    d = {"type": "scene",
         "integrator": {"type": integrator, "max_depth": max_depth, "rr_depth": rr_depth},
         "sensor": {"type": "perspective", "fov": 60, "to_world": T().look_at([0.1, 0.05, 1.8], [0, 0, -1], [0, 1, 0]),
                    "film": {"type": "hdrfilm", "width": res[0], "height": res[1], "rfilter": {"type": "gaussian"}}, "sampler": {"type": "independent", "sample_count": spp}},
         "wall_a": tex(6, 5), "wall_b": tex(4, 7), "side": tex(5, 5),
         "metal": {"type": "roughconductor", "alpha": 0.25, "distribution": "ggx", "eta": [0.2, 0.92, 1.1], "k": [3.9, 2.45, 2.14]},
         # the shell: x, y in [-1, 1], z in [-2, 2]; normals point inwards
         "back_a": {"type": "rectangle", "to_world": T().translate([0, 0, -2.0]), "bsdf": {"type": "ref", "id": "wall_a"}},
         "back_b": {"type": "rectangle", "to_world": T().translate([0, 0, 2.0]).rotate([0, 1, 0], 180), "bsdf": {"type": "ref", "id": "wall_b"}},
         "floor": {"type": "rectangle", "to_world": T().translate([0, -1.0, 0]).rotate([1, 0, 0], -90).scale([1.0, 2.0, 1.0]), "bsdf": {"type": "ref", "id": "side"}},
         "ceiling": {"type": "rectangle", "to_world": T().translate([0, 1.0, 0]).rotate([1, 0, 0], 90).scale([1.0, 2.0, 1.0]), "bsdf": {"type": "ref", "id": "side"}},
         "left": {"type": "rectangle", "to_world": T().translate([-1.0, 0, 0]).rotate([0, 1, 0], 90).scale([2.0, 1.0, 1.0]), "bsdf": {"type": "ref", "id": "side"}},
         "right": {"type": "rectangle", "to_world": T().translate([1.0, 0, 0]).rotate([0, 1, 0], -90).scale([2.0, 1.0, 1.0]), "bsdf": {"type": "ref", "id": "side"}},
         "block": {"type": "cube", "to_world": T().translate([-0.45, -0.7, -1.2]).rotate([0, 1, 0], 25).scale([0.25, 0.3, 0.25]), "bsdf": {"type": "ref", "id": "metal"}},
         "light_a": {"type": "rectangle", "to_world": T().translate([0.3, 0.98, -1.0]).rotate([1, 0, 0], 90).scale([0.3, 0.3, 1.0]),
                     "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [14, 12, 9]}}},
         "light_b": {"type": "rectangle", "to_world": T().translate([-0.3, 0.98, 1.0]).rotate([1, 0, 0], 90).scale([0.25, 0.25, 1.0]),
                     "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [6, 8, 11]}}}}
    if pane is not None:
        d["glass"] = dict(pane)
        d["pane"] = {"type": "rectangle", "bsdf": {"type": "ref", "id": "glass"}}
    return d
