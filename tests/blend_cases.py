"""Shared cases of the `blendbsdf` tests (test_blendbsdf_cpu.py, test_gpu_blendbsdf.py): the nested pairs, the weights, the (wi, uv, wo, sample1, sample2)
tuples, an independent float64 lookup of the weight, and src/bsdfs/blendbsdf.cpp restated in NumPy float32 over the oracle's answers for the two nested BSDFs
(OracleScene.bsdf_evaluate_ctx / bsdf_sample_ctx of a scene that holds the nested BSDFs alone)."""
import ctypes as C

import numpy as np

LUM = (np.float32(0.212671), np.float32(0.715160), np.float32(0.072169))        # spectrum.h:439-442: float constants
ALL = 0xffffffff
COUNT = {"diffuse": 1, "dielectric": 2, "roughconductor": 1, "roughplastic": 2, "conductor": 1, "plastic": 2}

PAIRS = {
    "diffuse+roughconductor": ({"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.2, 0.5, 0.8]}},
                               {"type": "roughconductor", "distribution": "ggx", "alpha_u": 0.1, "alpha_v": 0.3, "specular_reflectance": {"type": "rgb", "value": [0.9, 0.8, 0.7]}}),
    "plastic+diffuse": ({"type": "plastic", "diffuse_reflectance": {"type": "rgb", "value": [0.1, 0.27, 0.36]}, "int_ior": 1.9},
                        {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.3, 0.4]}}),
    "conductor+roughplastic": ({"type": "conductor", "eta": [0.143, 0.375, 1.442], "k": [3.983, 2.386, 1.603]},
                               {"type": "roughplastic", "diffuse_reflectance": {"type": "rgb", "value": [0.7, 0.3, 0.1]}, "alpha": 0.15}),
    "dielectric+diffuse": ({"type": "dielectric", "specular_reflectance": 0.3, "specular_transmittance": 0.6, "int_ior": 1.5, "ext_ior": 1.0},
                           {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.6, 0.6, 0.2]}}),
}
PAIR_NAMES = list(PAIRS) + ["twosided(diffuse+roughconductor)"]


def pair_dicts(name):
    """(nested dict 0, nested dict 1, under twosided?)"""
    two = name.startswith("twosided(")
    a, b = PAIRS[name[9:-1] if two else name]
    return dict(a), dict(b), two


def _bitmap3():
    """5 x 3, three channels in [0.15, 0.85], bilinear + repeat, with a to_uv.  The product interpolates in float32 as the reference's texture unit does; against a float64
    lookup the weight then carries up to three roundings of a texel (3 * 2^-24 * 0.85 = 1.5e-7), and a mixed pdf p0 (1 - w) + p1 w inherits that as 1.5e-7 / min(w, 1 - w)
    at worst (one nested pdf much larger than the other): weights at least 0.15 from both ends keep it under the leaf bar of 2e-6 that the pdf is held to.  (Clipped
    weights are the nearest bitmap's part, whose lookup is exact.)  Texels (0, 1) .. (1, 2) are the plateau (0.5, 0.5, 0.5): every bilinear lookup between their
    centres is exactly 0.5 in float32 and so is its luminance, so a `sample1` placed AT the weight is at the weight on both sides of the comparison"""
    rng = np.random.default_rng(41)
    t = rng.uniform(0.15, 0.85, (3, 5, 3)).astype(np.float32)
    t[0:2, 1:3] = (0.5, 0.5, 0.5)
    return t


def _bitmap1():
    """4 x 2, one channel, nearest: texels below 0 and above 1 (clipped weights) next to interior ones"""
    return np.array([[-0.3, 0.25, 1.4, 0.7], [0.6, 1.4, 0.125, -0.3]], np.float32)[:, :, None]


WEIGHT_NAMES = ["constant", "bitmap3_bilinear_to_uv", "bitmap1_nearest"]
TO_UV = np.array([[1.5, 0.25, 0.1], [-0.5, 2.0, 0.3]], np.float64)          # rows of the 2 x 3 affine map


def weight_prop(mi, name):
    if name == "constant":
        return 0.35
    if name == "bitmap3_bilinear_to_uv":
        m = np.eye(3); m[:2, :] = TO_UV
        return {"type": "bitmap", "data": _bitmap3(), "raw": True, "to_uv": mi.ScalarTransform3f(m)}
    return {"type": "bitmap", "data": _bitmap1(), "raw": True, "filter_type": "nearest"}


def blend_dict(mi, pair, weight):
    a, b, two = pair_dicts(pair)
    d = {"type": "blendbsdf", "weight": weight_prop(mi, weight) if isinstance(weight, str) else weight, "first": a, "second": b}
    return {"type": "twosided", "nested": d} if two else d


def _fma32(a, b, c):
    return np.float32(np.float64(np.float32(a)) * np.float64(np.float32(b)) + np.float64(np.float32(c)))


def lookup_weight(name, uv):
    """clip(Texture::eval_1(uv), 0, 1) by an independent lookup: the texel coordinates in float32 as the texture unit forms them (uv through to_uv, times the
    resolution, minus a half), the interpolation and the luminance in float64 on a np.pad'ed image (np.pad 'wrap' = repeat) -- the lookup of
    tests/test_bsdfs_cpu.py::test_bitmap_filter_and_wrap_modes_vs_numpy, extended by to_uv and Texture::eval_1"""
    n = uv.shape[1]
    if name == "constant":
        return np.full(n, np.float32(0.35))
    tex = _bitmap3() if name == "bitmap3_bilinear_to_uv" else _bitmap1()
    Hh, Ww = tex.shape[:2]; R = 12
    big = np.pad(tex, ((R * Hh, R * Hh), (R * Ww, R * Ww), (0, 0)), mode="wrap").astype(np.float64)
    out = np.zeros(n, np.float64)
    for i in range(n):
        u, v = np.float32(uv[0, i]), np.float32(uv[1, i])
        if name == "bitmap3_bilinear_to_uv":
            m = TO_UV.astype(np.float32)
            u, v = _fma32(m[0, 1], v, _fma32(m[0, 0], u, m[0, 2])), _fma32(m[1, 1], v, _fma32(m[1, 0], u, m[1, 2]))
        t = lambda x, y: big[y + R * Hh, x + R * Ww]
        if name == "bitmap1_nearest":
            c = t(int(np.floor(u * np.float32(Ww))), int(np.floor(v * np.float32(Hh))))
            out[i] = c[0]
        else:
            px, py = _fma32(u, Ww, -0.5), _fma32(v, Hh, -0.5)
            x0, y0 = int(np.floor(px)), int(np.floor(py)); fx, fy = float(px - np.float32(x0)), float(py - np.float32(y0))
            c = (1 - fy) * ((1 - fx) * t(x0, y0) + fx * t(x0 + 1, y0)) + fy * ((1 - fx) * t(x0, y0 + 1) + fx * t(x0 + 1, y0 + 1))
            out[i] = c[0] * float(LUM[0]) + c[1] * float(LUM[1]) + c[2] * float(LUM[2])
    return np.clip(out, 0.0, 1.0).astype(np.float32)


def plateau_uv(name, rng, n):
    """uv at which the weight is the same float32 on both sides of the comparison (see _bitmap3): any uv for the constant and the nearest bitmap"""
    if name != "bitmap3_bilinear_to_uv":
        return rng.uniform(-1.5, 2.5, (2, n))
    # texture coordinates between the centres of texels (x 1..2, y 0..1) of the 5 x 3 image, pulled back through to_uv
    tu = rng.uniform(1.6 / 5, 2.4 / 5, n); tv = rng.uniform(0.6 / 3, 1.4 / 3, n)
    A = TO_UV[:, :2]; b = TO_UV[:, 2]
    return np.linalg.solve(A, np.stack([tu, tv]) - b[:, None])


def tuples(weight, n=20000, seed=7):
    """n tuples (wi 3 x n, uv 2 x n, wo 3 x n, sample1 n, sample2 2 x n, w n): wi and wo over the whole sphere (both sides), an eighth of them grazing (|z| < 0.02), and an
    eighth with sample1 at 0, at the weight, at the floats below and above it and at the float below 1 (in turn)"""
    rng = np.random.default_rng(seed)

    def sphere(m, grazing):
        z = rng.uniform(-1, 1, m)
        z[grazing] = rng.uniform(-0.02, 0.02, int(grazing.sum()))
        ph = rng.uniform(0, 2 * np.pi, m); r = np.sqrt(1 - z * z)
        return np.stack([r * np.cos(ph), r * np.sin(ph), z]).astype(np.float32)

    k = np.arange(n)
    wi = sphere(n, k % 8 == 1); wo = sphere(n, k % 8 == 2)
    special = k % 8 == 3
    uv = rng.uniform(-1.5, 2.5, (2, n))
    uv[:, special] = plateau_uv(weight, rng, int(special.sum()))
    uv = uv.astype(np.float32)
    w = lookup_weight(weight, uv)
    s1 = rng.random(n).astype(np.float32)
    one_below = np.nextafter(np.float32(1), np.float32(0))
    idx = np.nonzero(special)[0]
    for j, i in enumerate(idx):
        s1[i] = (np.float32(0), w[i], np.nextafter(w[i], np.float32(-1)), np.nextafter(w[i], np.float32(2)), one_below)[j % 5]
    s1 = np.clip(s1, np.float32(0), one_below)
    s2 = rng.random((2, n)).astype(np.float32)
    return wi, uv, wo, s1, s2, w


def contexts(pair):
    """BSDFContexts (mode, type_mask, component): default, every component of the blend, and a type mask without the diffuse lobe"""
    a, b, _ = pair_dicts(pair)
    n = COUNT[a["type"]] + COUNT[b["type"]]
    return [(0, 0x1ff, ALL)] + [(0, 0x1ff, c) for c in range(n)] + [(0, 0x1ff & ~0x2, ALL)]


class Children:
    """the two nested BSDFs alone in an oracle scene, with their answers cached per (child, context, inputs)"""

    def __init__(self, mi, O, pair):
        a, b, self.two = pair_dicts(pair)
        self.n0 = COUNT[a["type"]]
        self.scene = mi.core.Scene({"c0": mi.load_dict(a), "c1": mi.load_dict(b)})
        self.osc, _ = O.scene_from_product(self.scene)
        self._eval = {}

    def eval_pdf(self, k, ctx, wi, uv, wo):
        key = (k, ctx) + tuple((a.shape, a.tobytes()) for a in (wi, uv, wo))
        if key not in self._eval:
            self._eval[key] = self.osc.bsdf_evaluate_ctx(k, ctx, 2, wi, uv, wo)
        return self._eval[key]

    def sample(self, k, ctx, wi, uv, s1, s2):
        return self.osc.bsdf_sample_ctx(k, ctx, wi, uv, s1, s2)


def _fold(ch, wi, wo=None):
    """TwoSidedBRDF with one nested BSDF (twosided.cpp:124-127, 159-162): wo.z = mulsign(wo.z, wi.z), wi.z = |wi.z|"""
    if not ch.two:
        return wi, wo, None
    neg = np.signbit(wi[2])
    wi2 = wi.copy(); wi2[2] = np.abs(wi2[2])
    wo2 = None
    if wo is not None:
        wo2 = wo.copy(); wo2[2] = np.where(neg, -wo2[2], wo2[2])
    return wi2, wo2, neg


def expected_eval_pdf(ch, ctx, w, wi, uv, wo):
    """BlendBSDF::eval_pdf (blendbsdf.cpp:198-222) in float32 over the nested BSDFs' oracle answers: (value 3 x n, pdf n)"""
    f = np.float32
    wi, wo, _ = _fold(ch, wi, wo)
    w = w.astype(f); one_minus = (f(1) - w).astype(f)
    if ctx[2] != ALL:
        first = ctx[2] < ch.n0
        k = 0 if first else 1
        ctx2 = (ctx[0], ctx[1], ctx[2] if first else (ctx[2] - ch.n0) & ALL)
        val, pdf = ch.eval_pdf(k, ctx2, wi, uv, wo)
        return ((one_minus if first else w)[None, :] * val).astype(f), pdf
    v0, p0 = ch.eval_pdf(0, ctx, wi, uv, wo)
    v1, p1 = ch.eval_pdf(1, ctx, wi, uv, wo)
    val = ((v0 * one_minus[None, :]).astype(f) + (v1 * w[None, :]).astype(f)).astype(f)
    pdf = ((p0 * one_minus).astype(f) + (p1 * w).astype(f)).astype(f)
    return val, pdf


def expected_sample(ch, ctx, w, wi, uv, s1, s2):
    """BlendBSDF::sample (blendbsdf.cpp:108-160) in float32 over the nested BSDFs' oracle answers: dict as OracleScene.bsdf_sample_ctx returns it"""
    f = np.float32
    wi_f, _, neg = _fold(ch, wi)
    n = s1.size
    w = w.astype(f); one_minus = (f(1) - w).astype(f)
    out = dict(wo=np.zeros((3, n), f), pdf=np.zeros(n, f), weight=np.zeros((3, n), f), eta=np.zeros(n, f), sampled_type=np.zeros(n, np.uint32), sampled_component=np.zeros(n, np.uint32))

    def put(mask, r, weight, pdf):
        for key in ("wo", ):
            out[key][:, mask] = r[key]
        out["weight"][:, mask] = weight; out["pdf"][mask] = pdf
        for key in ("eta", "sampled_type", "sampled_component"):
            out[key][mask] = r[key]

    if ctx[2] != ALL:
        first = ctx[2] < ch.n0
        k = 0 if first else 1
        ctx2 = (ctx[0], ctx[1], ctx[2] if first else (ctx[2] - ch.n0) & ALL)
        r = ch.sample(k, ctx2, wi_f, uv, s1, s2)
        put(np.ones(n, bool), r, (r["weight"] * (one_minus if first else w)[None, :]).astype(f), r["pdf"])
    else:
        m0 = s1 > w; m1 = s1 <= w
        with np.errstate(divide="ignore", invalid="ignore"):
            s_first = ((s1 - w).astype(f) / one_minus).astype(f); s_second = (s1 / w).astype(f)
        for mask, ks, ko, ss in ((m0, 0, 1, s_first), (m1, 1, 0, s_second)):
            if not mask.any():
                continue
            a = wi_f[:, mask]; b = uv[:, mask]
            r = ch.sample(ks, ctx, a, b, ss[mask], s2[:, mask])
            ev, ep = ch.osc.bsdf_evaluate_ctx(ko, ctx, 2, a, b, r["wo"])
            ws, wo_ = (one_minus[mask], w[mask]) if ks == 0 else (w[mask], one_minus[mask])           # the sampled BSDF's share, the other's
            pdf_w = ((w[mask] * (ep if ks == 0 else r["pdf"])).astype(f) + (one_minus[mask] * (r["pdf"] if ks == 0 else ep)).astype(f)).astype(f)
            with np.errstate(invalid="ignore"):
                sampled = ((r["weight"] * ws[None, :]).astype(f) * r["pdf"][None, :]).astype(f)
                other = (ev * wo_[None, :]).astype(f)
            total = ((other + sampled) if ks == 0 else (sampled + other)).astype(f)
            with np.errstate(divide="ignore"):
                inv = np.where(pdf_w > 0, (f(1) / pdf_w).astype(f), f(0)).astype(f)
            put(mask, r, (total * inv[None, :]).astype(f), pdf_w)
    if ch.two:
        out["wo"][2] = np.where(neg, -out["wo"][2], out["wo"][2])
    return out


# ---- the product's host entries (har_bsdf_eval_pdf_host / har_bsdf_sample_host) over arrays

def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def host_eval_pdf(mi, scene, index, ctx, wi, uv, wo, active=None):
    from mitsuba3_amd import _capi
    n = wo.shape[1]
    wi = np.ascontiguousarray(wi, np.float32); uv = np.ascontiguousarray(uv, np.float32); wo = np.ascontiguousarray(wo, np.float32)
    val = np.zeros((3, n), np.float32); pdf = np.zeros(n, np.float32)
    d = scene.desc()
    c = _capi.HarBSDFContext(ctx[0], ctx[1] & ALL, ctx[2] & ALL) if ctx is not None else None
    act = np.ascontiguousarray(active, np.uint8) if active is not None else None
    rc = mi.lib().har_bsdf_eval_pdf_host(C.byref(d), index, C.byref(c) if c is not None else None, n, _fp(wi), _fp(uv), _fp(wo), act.ctypes.data_as(C.c_void_p) if act is not None else None,
                                         _fp(val), _fp(pdf))
    assert rc == 0, mi.lib().har_last_error()
    return val, pdf


def host_sample(mi, scene, index, ctx, wi, uv, s1, s2, active=None):
    from mitsuba3_amd import _capi
    n = s2.shape[1]
    wi = np.ascontiguousarray(wi, np.float32); uv = np.ascontiguousarray(uv, np.float32); s1 = np.ascontiguousarray(s1, np.float32); s2 = np.ascontiguousarray(s2, np.float32)
    wo = np.zeros((3, n), np.float32); pdf = np.zeros(n, np.float32); w = np.zeros((3, n), np.float32); eta = np.zeros(n, np.float32)
    st = np.zeros(n, np.uint32); sc = np.zeros(n, np.uint32)
    d = scene.desc()
    c = _capi.HarBSDFContext(ctx[0], ctx[1] & ALL, ctx[2] & ALL) if ctx is not None else None
    act = np.ascontiguousarray(active, np.uint8) if active is not None else None
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    rc = mi.lib().har_bsdf_sample_host(C.byref(d), index, C.byref(c) if c is not None else None, n, _fp(wi), _fp(uv), _fp(s1), _fp(s2),
                                       act.ctypes.data_as(C.c_void_p) if act is not None else None, _fp(wo), _fp(pdf), _fp(w), _fp(eta), u32(st), u32(sc))
    assert rc == 0, mi.lib().har_last_error()
    return dict(wo=wo, pdf=pdf, weight=w, eta=eta, sampled_type=st, sampled_component=sc)


def host_render_stats(mi, scene, seed, spp, max_depth, rr_depth):
    """har_render_lanes_stats_host: (raw film H x W x 4, HarStats) of the forward `path` render on the host, by the functions the kernels run"""
    from mitsuba3_amd import _capi
    sensor = scene.sensors()[0]
    w, h = sensor.film().crop_size()
    film = np.zeros((h, w, 4), np.float32); st = _capi.HarStats()
    desc = scene.desc()
    mi.core.check(mi.lib().har_render_lanes_stats_host(C.byref(desc), C.byref(sensor.har), None, 0, seed, spp, max_depth, rr_depth, _fp(film), C.byref(st)))
    return film, st


def bound(mi, bsdf):
    """(private scene, record index) of a stand-alone BSDF object"""
    if bsdf.scene is None:
        mi.core.Scene({"_bsdf": bsdf})
    return bsdf.scene, bsdf.index


# ---- the render scenes: a Cornell-like box whose walls all carry a blend

def blended_box(mi, res, spp, children, weight, integrator="path", max_depth=6, rr_depth=7, twosided=False, instanced=False, nearest=False, a_bitmap=None):
    """mi.cornell_box() with every wall material replaced by ONE blend of `children` (two dicts) by `weight` (a float, or an 8 x 8 one-channel array)"""
    d = mi.cornell_box()
    d["sensor"]["film"]["width"] = res[0]; d["sensor"]["film"]["height"] = res[1]
    d["sensor"]["sampler"] = {"type": "independent", "sample_count": spp}
    d["integrator"] = {"type": integrator, "max_depth": max_depth, "rr_depth": rr_depth}
    wprop = float(weight) if np.isscalar(weight) else {"type": "bitmap", "data": np.asarray(weight, np.float32), "raw": True, **({"filter_type": "nearest"} if nearest else {})}
    c0 = dict(children[0])
    if a_bitmap is not None:
        c0 = {"type": "diffuse", "reflectance": {"type": "bitmap", "data": np.asarray(a_bitmap, np.float32), "raw": True, **({"filter_type": "nearest"} if nearest else {})}}
    blend = {"type": "blendbsdf", "weight": wprop, "bsdf_a": c0, "bsdf_b": dict(children[1])}
    d["white"] = {"type": "twosided", "nested": blend} if twosided else blend
    for k in ("green", "red"):
        d.pop(k, None)
    for k, v in d.items():
        if isinstance(v, dict) and isinstance(v.get("bsdf"), dict) and v["bsdf"].get("type") == "ref":
            v["bsdf"] = {"type": "ref", "id": "white"}
    if instanced:       # the two boxes move into a shape group that one instance places where they were
        group = {"type": "shapegroup"}
        for k in ("small-box", "large-box"):
            group[k] = d.pop(k)
        d["boxes"] = group
        d["placed"] = {"type": "instance", "g": {"type": "ref", "id": "boxes"}}
    return d


def equivalent_box(mi, res, spp, albedo, integrator="path", max_depth=6, rr_depth=7, instanced=False, nearest=False, twosided=False):
    """the same box with ONE diffuse material of albedo `albedo` (an rgb triple or an H x W x 3 bitmap): what a blend of two diffuse BSDFs is (under `twosided` if the blend is)"""
    d = blended_box(mi, res, spp, ({"type": "diffuse"}, {"type": "diffuse"}), 0.5, integrator, max_depth, rr_depth, False, instanced)
    albedo = np.asarray(albedo, np.float32)
    d["white"] = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [float(x) for x in albedo]} if albedo.ndim == 1 else
                  {"type": "bitmap", "data": albedo, "raw": True, **({"filter_type": "nearest"} if nearest else {})}}
    if twosided:
        d["white"] = {"type": "twosided", "nested": d["white"]}
    return d


A_RGB = np.array([0.8, 0.3, 0.2], np.float32)
B_RGB = np.array([0.25, 0.5, 0.75], np.float32)
DIFFUSE_PAIR = ({"type": "diffuse", "reflectance": {"type": "rgb", "value": [float(x) for x in A_RGB]}},
                {"type": "diffuse", "reflectance": {"type": "rgb", "value": [float(x) for x in B_RGB]}})


def weight_map8(seed=3):
    """8 x 8 weights in (0.1, 0.9)"""
    return np.random.default_rng(seed).uniform(0.1, 0.9, (8, 8, 1)).astype(np.float32)


def albedo_map(w, a=A_RGB, b=B_RGB):
    """(1 - w) A + w B per texel, in float32 as the blend forms it per lookup (for a bilinear bitmap the two commute up to rounding: both are affine in the texels)"""
    w = np.asarray(w, np.float32).reshape(w.shape[0], w.shape[1], 1)
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return ((np.float32(1) - w) * a + w * b).astype(np.float32)
