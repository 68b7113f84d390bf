"""Shared cases of the `normalmap` tests (test_normalmap_cpu.py, test_gpu_normalmap.py): the nested models, the normal maps, the (wi, uv, wo, sample1, sample2) tuples,
an independent float64 lookup of the normal-map colour (the lookup of tests/blend_cases.py, three channels), src/bsdfs/normalmap.cpp restated in NumPy float32 over the
oracle's answers for the nested BSDF alone (OracleScene.bsdf_evaluate_ctx / bsdf_sample_ctx of a scene that holds only the nested BSDF), the reference's rule for the
shading frame of a rectangle restated in float64, and the render scenes."""
import ctypes as C

import numpy as np

from tests import blend_cases as B

ALL = B.ALL
COUNT = B.COUNT
F32 = np.float32

NESTED = {
    "diffuse": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.2, 0.5, 0.8]}},
    "roughconductor_beckmann": {"type": "roughconductor", "distribution": "beckmann", "alpha": 0.2, "eta": [0.2, 0.9, 1.1], "k": [3.9, 2.4, 2.2],
                                "specular_reflectance": {"type": "rgb", "value": [0.9, 0.8, 0.7]}},
    "roughconductor_ggx": {"type": "roughconductor", "distribution": "ggx", "alpha_u": 0.1, "alpha_v": 0.3, "specular_reflectance": {"type": "rgb", "value": [0.9, 0.8, 0.7]}},
    # (alpha 0.3: an ulp of the frame is amplified by about 1 / alpha^2 -- with the bitmap map, whose texel the product interpolates in float32 and the restatement in float64,
    # the sample pdf of an alpha = 0.15 coating differs by 1.2e-4 absolute, 2.5e-5 relative: above the 1e-4 of the reference's test02, which caps the per-call bars)
    "roughplastic": {"type": "roughplastic", "diffuse_reflectance": {"type": "rgb", "value": [0.7, 0.3, 0.1]}, "alpha": 0.3},
    # ... and that coating: held to the project's bars through the float32-interpolating lookup (lookup_colour32), where the cause is absent
    "roughplastic_015": {"type": "roughplastic", "diffuse_reflectance": {"type": "rgb", "value": [0.7, 0.3, 0.1]}, "alpha": 0.15},
    "plastic": {"type": "plastic", "diffuse_reflectance": {"type": "rgb", "value": [0.1, 0.27, 0.36]}, "int_ior": 1.9},
    "dielectric": {"type": "dielectric", "specular_reflectance": 0.3, "specular_transmittance": 0.6, "int_ior": 1.5, "ext_ior": 1.0},
    "twosided(diffuse)": {"type": "twosided", "inner": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.6, 0.6, 0.2]}}},
}
NESTED_NAMES = [n for n in NESTED if n != "roughplastic_015"]
NON_DELTA = [n for n in NESTED_NAMES if n != "dielectric"]
MAP_NAMES = ["identity", "tilt30", "bitmap_bilinear_to_uv"]
SWITCHES = [(True, True), (True, False), (False, True), (False, False)]          # (flip_invalid_normals, use_shadowing_function)
TO_UV = B.TO_UV
TILT30 = (0.5 * 0.5 + 0.5, 0.5, 0.5 * (0.5 * np.sqrt(3.0)) + 0.5)               # n * 0.5 + 0.5 of n = (sin 30, 0, cos 30): the reference's test02


def nested_dict(name):
    d = NESTED[name]
    return {k: (dict(v) if isinstance(v, dict) else v) for k, v in d.items()}


def component_count(name):
    d = NESTED[name]
    if d["type"] != "twosided":
        return COUNT[d["type"]]
    kids = [v for k, v in d.items() if isinstance(v, dict)]
    return COUNT[kids[0]["type"]] + COUNT[kids[-1]["type"]]


def tilted_texels(h, w, lo_deg, hi_deg, seed):
    """h x w x 3 normal-map texels n * 0.5 + 0.5 of unit normals tilted between lo_deg and hi_deg from +z, at random azimuths"""
    rng = np.random.default_rng(seed)
    th = np.radians(rng.uniform(lo_deg, hi_deg, (h, w))); ph = rng.uniform(0, 2 * np.pi, (h, w))
    n = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1)
    return (n * 0.5 + 0.5).astype(np.float32)


def _bitmap():
    """5 x 3 texels, tilts up to 60 degrees"""
    return tilted_texels(3, 5, 0.0, 60.0, 23)


def map_prop(mi, name):
    if name == "identity":
        return {"type": "rgb", "value": [0.5, 0.5, 1.0]}
    if name == "tilt30":
        return {"type": "rgb", "value": [float(x) for x in TILT30]}
    m = np.eye(3); m[:2, :] = TO_UV
    return {"type": "bitmap", "data": _bitmap(), "raw": True, "to_uv": mi.ScalarTransform3f(m)}


def normalmap_dict(mi, nested, nmap, flip=True, shadow=True):
    d = {"type": "normalmap", "normalmap": map_prop(mi, nmap) if isinstance(nmap, str) else nmap, "inner": nested_dict(nested) if isinstance(nested, str) else dict(nested)}
    if not flip:
        d["flip_invalid_normals"] = False
    if not shadow:
        d["use_shadowing_function"] = False
    return d


def lookup_colour(tex, uv, to_uv=None, nearest=False):
    """Texture::eval_3 of a bilinear (or nearest) + repeat bitmap by an independent lookup: the texel coordinates in float32 as the texture unit forms them (uv through
    to_uv, times the resolution, minus a half), the interpolation in float64 on a np.pad'ed image -- tests/blend_cases.py::lookup_weight without the luminance.  3 x n float64"""
    n = uv.shape[1]
    Hh, Ww = tex.shape[:2]; R = 12
    big = np.pad(tex, ((R * Hh, R * Hh), (R * Ww, R * Ww), (0, 0)), mode="wrap").astype(np.float64)
    out = np.zeros((3, n), np.float64)
    m = None if to_uv is None else np.asarray(to_uv, np.float32)
    for i in range(n):
        u, v = np.float32(uv[0, i]), np.float32(uv[1, i])
        if m is not None:
            u, v = B._fma32(m[0, 1], v, B._fma32(m[0, 0], u, m[0, 2])), B._fma32(m[1, 1], v, B._fma32(m[1, 0], u, m[1, 2]))
        t = lambda x, y: big[y + R * Hh, x + R * Ww]
        if nearest:
            out[:, i] = t(int(np.floor(u * np.float32(Ww))), int(np.floor(v * np.float32(Hh))))
            continue
        px, py = B._fma32(u, Ww, -0.5), B._fma32(v, Hh, -0.5)
        x0, y0 = int(np.floor(px)), int(np.floor(py)); fx, fy = float(px - np.float32(x0)), float(py - np.float32(y0))
        out[:, i] = (1 - fy) * ((1 - fx) * t(x0, y0) + fx * t(x0 + 1, y0)) + fy * ((1 - fx) * t(x0, y0 + 1) + fx * t(x0 + 1, y0 + 1))
    return out


def lookup_colour32(tex, uv, to_uv=None):
    """the same bilinear + repeat lookup with the INTERPOLATION in float32 too, in the order the texture unit of this project takes (weights w1 = p - floor(p),
    w0 = 1 - w1; fmadd(w0x, t00, w1x * t10) per row, then the same across the rows): what the product computes, up to the last bit of a fused operation.  3 x n float32"""
    f = F32
    u, v = np.asarray(uv[0], f), np.asarray(uv[1], f)
    if to_uv is not None:
        m = np.asarray(to_uv, f)
        u, v = _fma(np.full_like(u, m[0, 1]), v, _fma(np.full_like(u, m[0, 0]), u, m[0, 2])), _fma(np.full_like(u, m[1, 1]), v, _fma(np.full_like(u, m[1, 0]), u, m[1, 2]))
    Hh, Ww = tex.shape[:2]
    px, py = _fma(u, f(Ww), f(-0.5)), _fma(v, f(Hh), f(-0.5))
    fx, fy = np.floor(px), np.floor(py)
    w1x, w1y = (px - fx).astype(f), (py - fy).astype(f); w0x, w0y = (f(1) - w1x).astype(f), (f(1) - w1y).astype(f)
    x0 = fx.astype(np.int64) % Ww; x1 = (fx.astype(np.int64) + 1) % Ww; y0 = fy.astype(np.int64) % Hh; y1 = (fy.astype(np.int64) + 1) % Hh
    out = np.zeros((3, u.size), f)
    for ch in range(3):
        t = tex[:, :, ch].astype(f)
        r0 = _fma(w0x, t[y0, x0], (w1x * t[y0, x1]).astype(f)); r1 = _fma(w0x, t[y1, x0], (w1x * t[y1, x1]).astype(f))
        out[ch] = _fma(w0y, r0, (w1y * r1).astype(f))
    return out


def map_colour(name, uv):
    """the looked-up normal-map colour of the named map at uv: 3 x n float32"""
    n = uv.shape[1]
    if name == "identity":
        return np.repeat(np.array([[0.5], [0.5], [1.0]], F32), n, 1)
    if name == "tilt30":
        return np.repeat(np.array(TILT30, F32)[:, None], n, 1)
    return lookup_colour(_bitmap(), uv, TO_UV).astype(F32)


def tuples(n=20000, seed=7):
    """n tuples (wi 3 x n, uv 2 x n, wo 3 x n, sample1 n, sample2 2 x n): wi and wo over the whole sphere (both sides of the surface, and -- the normals being tilted by up
    to 60 degrees -- wo on either side of the perturbed horizon, wi for which the flip triggers and for which it does not), an eighth of wi and an eighth of wo grazing
    (0.002 <= |z| < 0.02), an eighth with sample1 at 0, at the floats next to 0.5 and at the float below 1 (in turn), as in tests/mask_cases.py"""
    rng = np.random.default_rng(seed)

    def sphere(m, grazing):
        # |z| >= 0.002: with the identity map the flip product is wi.z^2 and the orientation product wo.z^2, and lanes within 1e-6 of a switch are left out of the
        # discrete comparison -- at most 0.1 % of them may be (checked on the restatement, test_normalmap_cpu.py)
        z = rng.uniform(0.002, 1, m)
        z[grazing] = rng.uniform(0.002, 0.02, int(grazing.sum()))
        z = z * np.where(rng.random(m) < 0.5, -1.0, 1.0)
        ph = rng.uniform(0, 2 * np.pi, m); r = np.sqrt(1 - z * z)
        return np.stack([r * np.cos(ph), r * np.sin(ph), z]).astype(F32)

    k = np.arange(n)
    wi = sphere(n, k % 8 == 1); wo = sphere(n, k % 8 == 2)
    uv = rng.uniform(-1.5, 2.5, (2, n)).astype(F32)
    s1 = rng.random(n).astype(F32)
    one_below = np.nextafter(F32(1), F32(0))
    idx = np.nonzero(k % 8 == 3)[0]
    for j, i in enumerate(idx):
        s1[i] = (F32(0), F32(0.5), np.nextafter(F32(0.5), F32(-1)), np.nextafter(F32(0.5), F32(2)), one_below)[j % 5]
    s1 = np.clip(s1, F32(0), one_below)
    s2 = rng.random((2, n)).astype(F32)
    return wi, uv, wo, s1, s2


def contexts(nested):
    """(mode, type_mask, component) the nested models are tested with (tests/blend_cases.py::contexts): default, every component, a type mask without the diffuse lobe;
    and TransportMode::Importance (the dielectric's transmission is NonSymmetric)"""
    n = component_count(nested)
    return [(0, 0x1ff, ALL)] + [(0, 0x1ff, c) for c in range(n)] + [(0, 0x1ff & ~0x2, ALL), (1, 0x1ff, ALL)]


class Nested:
    """the nested BSDF alone in an oracle scene (the oracle resolves a `twosided` record itself)"""

    def __init__(self, mi, O, name):
        self.name = name
        obj = mi.load_dict(nested_dict(name))
        self.obj = obj
        self.scene = mi.core.Scene({"c0": obj}); self.index = obj.index
        self.osc, _ = O.scene_from_product(self.scene)

    def eval_pdf(self, ctx, wi, uv, wo):
        return self.osc.bsdf_evaluate_ctx(self.index, ctx, 2, np.ascontiguousarray(wi, F32), np.ascontiguousarray(uv, F32), np.ascontiguousarray(wo, F32))

    def sample(self, ctx, wi, uv, s1, s2):
        return self.osc.bsdf_sample_ctx(self.index, ctx, np.ascontiguousarray(wi, F32), np.ascontiguousarray(uv, F32), np.ascontiguousarray(s1, F32), np.ascontiguousarray(s2, F32))


# ---- normalmap.cpp in NumPy float32 (fused operations formed in float64 and rounded once more: within an ulp of a float32 fma)

def _fma(a, b, c):
    return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _dot(a, b):
    """dr::dot: mul, then an fma chain"""
    return _fma(a[2], b[2], _fma(a[1], b[1], (a[0] * b[0]).astype(F32)))


def _normalize(v):
    return (v * (F32(1) / np.sqrt(_dot(v, v)))[None, :]).astype(F32)


def _cross(a, b):
    """dr::cross: fmsub of the rotated components"""
    return np.stack([_fma(a[1], b[2], -(a[2] * b[1]).astype(F32)), _fma(a[2], b[0], -(a[0] * b[2]).astype(F32)), _fma(a[0], b[1], -(a[1] * b[0]).astype(F32))])


class Frame:
    def __init__(self, s, t, n):
        self.s, self.t, self.n = s, t, n

    def to_local(self, v):
        return np.stack([_dot(v, self.s), _dot(v, self.t), _dot(v, self.n)])

    def to_world(self, v):
        return np.stack([_fma(self.n[k], v[2], _fma(self.t[k], v[1], (self.s[k] * v[0]).astype(F32))) for k in range(3)])


def frame(c, wi, flip):
    """NormalMap::frame (normalmap.cpp:224-236) relative to si.sh_frame: (Frame, the flip product cos_theta(wi) * dot(wi, n) -- all ones where flip is off)"""
    c = np.asarray(c, F32); wi = np.asarray(wi, F32)
    n = _fma(c, F32(2), F32(-1))
    prod = np.ones(c.shape[1], F32)
    if flip:
        prod = (wi[2] * _dot(wi, n)).astype(F32)
        f = prod <= 0
        n = np.where(f[None, :], np.stack([-n[0], -n[1], n[2]]), n)
    n = _normalize(n)
    s = _normalize(np.stack([_fma(-n[0], n[0], F32(1)), _fma(-n[1], n[0], F32(0)), _fma(-n[2], n[0], F32(0))]))
    t = _cross(n, s)
    return Frame(s, t, n), prod


def tan_theta_2(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.maximum(_fma(-v[2], v[2], F32(1)), F32(0)) / (v[2] * v[2]).astype(F32)).astype(F32)


def shadow_terminator(n, wo):
    """eval_shadow_terminator (normalmap_helpers.h:20-25)"""
    with np.errstate(invalid="ignore", over="ignore"):
        alpha2 = np.minimum((F32(0.125) * tan_theta_2(n)).astype(F32), F32(1))
        return (F32(2) / (F32(1) + np.sqrt((F32(1) + (alpha2 * tan_theta_2(wo)).astype(F32)).astype(F32))).astype(F32)).astype(F32)


def expected_eval_pdf(ch, ctx, c, wi, uv, wo, flip, shadow):
    """NormalMap::eval_pdf (normalmap.cpp:198-219): (value 3 x n, pdf n, active lanes, lanes within 1e-6 of a switch of the orientation or the flip product)"""
    Fm, fprod = frame(c, wi, flip)
    pwi = Fm.to_local(wi); pwo = Fm.to_local(wo)
    oprod = (wo[2] * pwo[2]).astype(F32)
    active = oprod > 0
    val, pdf = ch.eval_pdf(ctx, pwi, uv, pwo)
    if shadow:
        with np.errstate(invalid="ignore"):
            val = (val * shadow_terminator(Fm.n, wo)[None, :]).astype(F32)
    val = np.where(active[None, :], val, F32(0)); pdf = np.where(active, pdf, F32(0))
    near = (np.abs(oprod) <= 1e-6) | (np.abs(fprod) <= 1e-6)
    return val.astype(F32), pdf.astype(F32), active, near


def expected_sample(ch, ctx, c, wi, uv, s1, s2, flip, shadow):
    """NormalMap::sample (normalmap.cpp:134-160) per lane of a wavefront: dict as OracleScene.bsdf_sample_ctx returns it, plus `near`"""
    Fm, fprod = frame(c, wi, flip)
    pwi = Fm.to_local(wi)
    r = ch.sample(ctx, pwi, uv, s1, s2)
    nonzero = (r["weight"] != 0).any(0)
    pwo = r["wo"].astype(F32)
    wo = Fm.to_world(pwo)
    oprod = (pwo[2] * wo[2]).astype(F32)
    active = nonzero & (oprod > 0)
    weight = r["weight"]
    if shadow:
        with np.errstate(invalid="ignore"):
            weight = (weight * shadow_terminator(Fm.n, wo)[None, :]).astype(F32)
    out = dict(wo=wo, pdf=np.where(active, r["pdf"], F32(0)).astype(F32), weight=np.where(active[None, :], weight, F32(0)).astype(F32), eta=r["eta"],
               sampled_type=r["sampled_type"], sampled_component=r["sampled_component"], active=active,
               near=(nonzero & (np.abs(oprod) <= 1e-6)) | (np.abs(fprod) <= 1e-6))
    return out


def fold(wi, wo=None):
    """an outer TwoSidedBRDF with one nested BSDF (twosided.cpp:124-127, 159-162): wo.z = mulsign(wo.z, wi.z), wi.z = |wi.z|"""
    neg = np.signbit(wi[2])
    wi2 = wi.copy(); wi2[2] = np.abs(wi2[2])
    wo2 = None
    if wo is not None:
        wo2 = wo.copy(); wo2[2] = np.where(neg, -wo2[2], wo2[2])
    return wi2, wo2, neg


# ---- the shading frame of a rectangle under a NormalMapped BSDF, float64

def rectangle_frame(to_world, flip_normals, inst=None):
    """(n, s, t) of a rectangle's shading frame in the reference, float64: n = normalize(T^-T (0, 0, 1)) with T = to_world * scale(1, 1, -1) under flip_normals
    (rectangle.cpp:110-121), the packed tangent normalize(T (1, 0, 0)) (mesh.cpp:1269-1350 on the unit rectangle, :1160-1193), FaceUVFlipped = det(T) < 0 (:1195-1197);
    through an instance n = normalize(I^-T n), s = I s, flipped ^= det(I) < 0 (instance.cpp:196-222); then finalize_surface_interaction (interaction.h:570-598):
    s = normalize(s - n dot(n, s)), t = cross(n, s), negated where flipped"""
    T = np.asarray(to_world, np.float64).reshape(4, 4)[:3, :3].copy()
    if flip_normals:
        T = T @ np.diag([1.0, 1.0, -1.0])
    n = np.linalg.inv(T).T @ np.array([0.0, 0.0, 1.0]); n /= np.linalg.norm(n)
    s = T @ np.array([1.0, 0.0, 0.0]); s /= np.linalg.norm(s)
    flipped = np.linalg.det(T) < 0
    if inst is not None:
        I = np.asarray(inst, np.float64).reshape(4, 4)[:3, :3]
        n = np.linalg.inv(I).T @ n; n /= np.linalg.norm(n)
        s = I @ s
        flipped ^= np.linalg.det(I) < 0
    s = s - n * np.dot(n, s); s /= np.linalg.norm(s)
    t = np.cross(n, s)
    return n, s, (-t if flipped else t)


def frame64(c, wi, flip):
    """NormalMap::frame in float64 (per lane columns): (s, t, n)"""
    c = np.asarray(c, np.float64); wi = np.asarray(wi, np.float64)
    n = 2.0 * c - 1.0
    if flip:
        f = wi[2] * (wi * n).sum(0) <= 0
        n = np.where(f[None, :], np.stack([-n[0], -n[1], n[2]]), n)
    n = n / np.linalg.norm(n, axis=0)
    s = np.stack([1.0 - n[0] * n[0], -n[1] * n[0], -n[2] * n[0]]); s = s / np.linalg.norm(s, axis=0)
    t = np.cross(n.T, s.T).T
    return s, t, n


# ---- the per-call derivative dF / dc

def host_grad(mi, scene, index, wi, uv, wo, A):
    """har_normalmap_grad_host: (F n, dF/dc 3 x n) for F = sum_k A_k value_k"""
    n = wo.shape[1]
    f = lambda a: np.ascontiguousarray(a, np.float32)
    wi, uv, wo, A = f(wi), f(uv), f(wo), f(A)
    val = np.zeros(n, np.float32); grad = np.zeros((3, n), np.float32)
    desc = scene.desc()
    rc = mi.lib().har_normalmap_grad_host(C.byref(desc), index, n, B._fp(wi), B._fp(uv), B._fp(wo), B._fp(A), B._fp(val), B._fp(grad))
    assert rc == 0, mi.lib().har_last_error()
    return val, grad


def weighted_value64(ch, c, wi, uv, wo, A, flip, shadow, flip_mask=None):
    """F = sum_k A_k value_k of normalmap.cpp with the FRAME and the shadow term in float64; the nested values come from OracleScene.bsdf_evaluate_ctx (float32) at the
    perturbed directions rounded to float32.  `flip_mask`: the flip decided beforehand (a finite difference keeps the branch of its centre).  Returns (F, flip product,
    orientation product)."""
    c = np.asarray(c, np.float64); wi64 = np.asarray(wi, np.float64); wo64 = np.asarray(wo, np.float64)
    n = 2.0 * c - 1.0
    fprod = wi64[2] * (wi64 * n).sum(0) if flip else np.ones(c.shape[1])
    f = (fprod <= 0) if flip_mask is None else flip_mask
    if flip:
        n = np.where(f[None, :], np.stack([-n[0], -n[1], n[2]]), n)
    n = n / np.linalg.norm(n, axis=0)
    s = np.stack([1.0 - n[0] * n[0], -n[1] * n[0], -n[2] * n[0]]); s = s / np.linalg.norm(s, axis=0)
    t = np.cross(n.T, s.T).T
    loc = lambda w: np.stack([(w * s).sum(0), (w * t).sum(0), (w * n).sum(0)])
    pwi, pwo = loc(wi64), loc(wo64)
    oprod = wo64[2] * pwo[2]
    val, _ = ch.eval_pdf((0, 0x1ff, ALL), pwi.astype(F32), uv, pwo.astype(F32))
    val = val.astype(np.float64)
    if shadow:
        tan2 = lambda w: np.maximum(1.0 - w[2] * w[2], 0.0) / (w[2] * w[2])
        val = val * (2.0 / (1.0 + np.sqrt(1.0 + np.minimum(0.125 * tan2(n), 1.0) * tan2(wo64))))[None, :]
    val = np.where((oprod > 0)[None, :], val, 0.0)
    return (np.asarray(A, np.float64) * val).sum(0), fprod, oprod


def grad_tuples(n=5000, seed=11):
    """(wi, uv, wo, A, c): directions over the upper hemisphere mostly (a fifth below: zero lanes), colours n * 0.5 + 0.5 of normals tilted by 5 to 50 degrees"""
    rng = np.random.default_rng(seed)

    def hemi(m):
        z = rng.uniform(0.05, 1, m) * np.where(rng.random(m) < 0.1, -1.0, 1.0)
        ph = rng.uniform(0, 2 * np.pi, m); r = np.sqrt(1 - z * z)
        return np.stack([r * np.cos(ph), r * np.sin(ph), z]).astype(F32)

    wi, wo = hemi(n), hemi(n)
    th = np.radians(rng.uniform(5.0, 50.0, n)); ph = rng.uniform(0, 2 * np.pi, n)
    nrm = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    c = (nrm * rng.uniform(0.6, 1.0, n)[None, :] * 0.5 + 0.5).astype(F32)          # (not unit length: the value must not depend on the length)
    # tuple i reads texel i of a 100-wide nearest bitmap that holds the colours (grad_map): the record looks its colour up, the restatement is handed it
    k = np.arange(n); rows = (n + 99) // 100
    uv = np.stack([(k % 100 + 0.5) / 100.0, (k // 100 + 0.5) / rows]).astype(F32)
    return wi, uv, wo, rng.uniform(0.2, 1.5, (3, n)).astype(F32), c


def grad_map(c):
    """the colours of grad_tuples as a (rows x 100 x 3) nearest bitmap property"""
    n = c.shape[1]; rows = (n + 99) // 100
    tex = np.full((rows * 100, 3), (0.5, 0.5, 1.0), np.float32); tex[:n] = c.T
    return {"type": "bitmap", "data": tex.reshape(rows, 100, 3), "raw": True, "filter_type": "nearest"}


def host_si(mi, scene, d, t, u, v, prim, shape, inst, ray_flags=1, active=None):
    """har_surface_interaction_host: the 33 x n rows of the array-valued compute_surface_interaction, on the host"""
    n = t.size
    f = lambda a: np.ascontiguousarray(a, np.float32)
    u32 = lambda a: np.ascontiguousarray(a, np.uint32)
    d, t, u, v = f(d), f(t), f(u), f(v); prim, shape, inst = u32(prim), u32(shape), u32(inst)
    out = np.zeros((33, n), np.float32)
    desc = scene.desc()
    act = np.ascontiguousarray(active, np.uint8) if active is not None else None
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    rc = mi.lib().har_surface_interaction_host(C.byref(desc), n, B._fp(d), B._fp(t), B._fp(u), B._fp(v), up(prim), up(shape), up(inst), int(ray_flags),
                                               act.ctypes.data_as(C.c_void_p) if act is not None else None, B._fp(out))
    assert rc == 0, mi.lib().har_last_error()
    return out


# ---- scenes

def _T(mi):
    return mi.ScalarTransform4f


def rectangle_transforms(mi):
    """to_world values of the frame tests: a rotation, a non-uniform scale, a shear, a mirroring scale"""
    T = _T(mi)
    shear = np.eye(4); shear[0, 1] = 0.6; shear[2, 0] = 0.3; shear[:3, 3] = (0.1, -0.2, 0.3)
    unit = lambda a: [float(x) for x in np.asarray(a, np.float64) / np.linalg.norm(a)]
    return {"rotation": T().translate([0.2, -0.1, 0.4]).rotate(unit([0.3, 1.0, 0.2]), 50.0),
            "scale": T().translate([0.0, 0.3, 0.0]).rotate([1, 0, 0], -30.0).scale([1.7, 0.6, 1.0]),
            "shear": T(np.concatenate([shear.ravel(), np.linalg.inv(shear).T.ravel()])),          # (the matrix, then its inverse transpose)
            "mirror": T().rotate([0, 1, 0], 25.0).scale([-1.3, 0.8, 1.0])}


INSTANCE_XF = ("inst_rot", "inst_mirror")


def instance_transform(mi, name):
    T = _T(mi)
    return T().translate([0.3, 0.2, -0.1]).rotate([float(np.sqrt(0.5)), float(np.sqrt(0.5)), 0.0], 35.0).scale([1.2, 0.9, -1.1] if name == "inst_mirror" else [1.2, 0.9, 1.1])


def frame_scene(mi, to_world, flip_normals, bsdf, instanced=None):
    """one rectangle carrying `bsdf` (a dict), at top level or inside a shape group placed by the instance transform `instanced`"""
    rect = {"type": "rectangle", "to_world": to_world, "bsdf": bsdf}
    if flip_normals:
        rect["flip_normals"] = True
    d = {"type": "scene"}
    if instanced is None:
        d["rect"] = rect
    else:
        d["grp"] = {"type": "shapegroup", "rect": rect}
        d["placed"] = {"type": "instance", "to_world": instanced, "g": {"type": "ref", "id": "grp"}}
    return d


def flat_mesh(z=0.0, half=1.0, texcoords=True):
    """a square of two triangles in the plane z, normal +z, WITHOUT vertex normals (case 1: coordinate_system(n)); texcoords = the unit square"""
    P = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]], np.float32)
    d = {"type": "mesh", "positions": P, "faces": np.array([[0, 1, 2], [0, 2, 3]], np.uint32)}
    if texcoords:
        d["texcoords"] = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    return d


def bumpy_texels(h=6, w=8, seed=5, lo=5.0, hi=50.0):
    return tilted_texels(h, w, lo, hi, seed)


def lit_scene(mi, bsdf, shape="rectangle", res=(16, 12), spp=4, integrator="path", max_depth=2, rr_depth=8, area_light=False, hide_emitters=False, low_camera=False, top_camera=False):
    """a rectangle (case 2) or a flat mesh without vertex normals (case 1) carrying `bsdf`, seen from above -- or, `low_camera`, at about ten degrees over the surface, where
    bumps turn away from the camera and flip_invalid_normals acts; or, `top_camera`, from within 35 degrees of the normal, where no bump of at most 50 degrees does, so that
    the render has no flip seam (the gradient tests) -- and lit by one point light (and an area light)"""
    T = _T(mi)
    d = {"type": "scene",
         "integrator": {"type": integrator, "max_depth": max_depth, "rr_depth": rr_depth},
         "sensor": {"type": "perspective", "fov": 40, "to_world": T().look_at([0.3, -2.6, 0.45] if low_camera else [0.1, -0.6, 2.6] if top_camera else [0.3, -1.9, 2.0], [0, 0, 0], [0, 0, 1]),
                    "film": {"type": "hdrfilm", "width": res[0], "height": res[1], "rfilter": {"type": "box"}}, "sampler": {"type": "independent", "sample_count": spp}},
         "mat": bsdf,
         "lamp": {"type": "point", "position": [0.6, 0.4, 1.5], "intensity": {"type": "rgb", "value": [6.0, 5.0, 4.0]}}}
    if hide_emitters:
        d["integrator"]["hide_emitters"] = True
    if shape == "rectangle":
        d["card"] = {"type": "rectangle", "to_world": T().rotate([0, 0, 1], 20.0).scale([1.1, 0.9, 1.0]), "bsdf": {"type": "ref", "id": "mat"}}
    else:
        d["card"] = dict(flat_mesh(), bsdf={"type": "ref", "id": "mat"})
    if area_light:
        d["panel"] = {"type": "rectangle", "to_world": T().translate([-0.8, 0.2, 1.4]).rotate([0, 1, 0], 150.0).scale([0.4, 0.4, 1.0]),
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [9, 10, 12]}}}
    return d


# the Cornell walls whose tangent frame (s along dp_du) IS the coordinate_system frame they have without a normal map, up to rounding (4e-8): floor, ceiling and back wall.
# The red and the green wall have n.z = -0, for which coordinate_system returns the tangent frame turned by half a turn about the normal: a sampler that does not depend on
# wi (the diffuse lobe's) then draws other world directions, in the reference as here -- those two keep the plain BSDF in the identity renders (the frames test covers them)
WALLS = ("floor", "ceiling", "back")
ALL_WALLS = WALLS + ("green-wall", "red-wall")
# nested models for which the half turn changes nothing: a microfacet lobe with the isotropic or the axis-aligned anisotropic distribution maps (wi, sample) to a wo that
# turns with wi (the distribution is even in x and in y), and a delta lobe depends on wi alone -- with them the map can sit on all five walls
HALF_TURN_INVARIANT = ("roughconductor_beckmann", "dielectric")


def walls_box(mi, res, spp, wall_bsdf, other_bsdf, integrator="path", max_depth=6, rr_depth=7, instanced=False, walls=WALLS):
    """mi.cornell_box() whose walls `walls` (rectangles) carry `wall_bsdf` and whose other shapes carry `other_bsdf` (dicts; the cubes have vertex normals and texture
    coordinates, so they cannot carry a normal map).  `instanced`: the floor and the back wall move into a shape group that one instance places where they were"""
    d = mi.cornell_box()
    d["sensor"]["film"]["width"] = res[0]; d["sensor"]["film"]["height"] = res[1]
    d["sensor"]["sampler"] = {"type": "independent", "sample_count": spp}
    d["integrator"] = {"type": integrator, "max_depth": max_depth, "rr_depth": rr_depth}
    d["white"] = other_bsdf; d["wallmat"] = wall_bsdf
    for k in ("green", "red"):
        d.pop(k, None)
    for k, v in d.items():
        if isinstance(v, dict) and isinstance(v.get("bsdf"), dict) and v["bsdf"].get("type") == "ref":
            v["bsdf"] = {"type": "ref", "id": "wallmat" if k in walls else "white"}
    if instanced:
        group = {"type": "shapegroup"}
        for k in ("floor", "back"):
            group[k] = d.pop(k)
        d["walls"] = group
        d["placed"] = {"type": "instance", "g": {"type": "ref", "id": "walls"}}
    return d
