"""Shared cases of the `bumpmap` tests (test_bumpmap_cpu.py, test_gpu_bumpmap.py): synthetic height bitmaps, BitmapTexture::eval_1_grad restated in NumPy (float64, and
float32 in the product's order), the interactions of three geometries, src/bsdfs/bumpmap.cpp:137-253 restated in NumPy float32 over the oracle's answers for the nested
BSDF alone (tests/normalmap_cases.py: Nested, Frame, shadow_terminator), the same in float64 for the per-call derivative, the host entries, and the render scenes."""
import ctypes as C

import numpy as np

from tests import blend_cases as B
from tests import normalmap_cases as N

ALL = N.ALL
F32 = np.float32
LUM = np.array([0.212671, 0.715160, 0.072169])
NESTED_NAMES = N.NESTED_NAMES            # seven nested models, as in the normalmap test
NON_DELTA = N.NON_DELTA
SWITCHES = N.SWITCHES
GEOMETRIES = ("rectangle", "scaled_rectangle", "smooth_mesh")
TAN60 = float(np.tan(np.radians(60.0)))


# ---- height bitmaps and eval_1_grad

def noise(h, w, channels, seed):
    """h x w x channels synthetic noise texels in [0, 1)"""
    return np.random.default_rng(seed).random((h, w, channels)).astype(F32)


def to_uv_cases(mi):
    """the to_uv transforms of tests/test_bitmap.py:32-52 in spirit: none, a scale + offset, a rotation about the centre, a rotation with a non-uniform scale; name -> 3 x 3"""
    out = {"identity": None}
    s = np.eye(3); s[0, 0] = 2.0; s[1, 1] = 0.5; s[0, 2] = 0.25; s[1, 2] = -0.1
    out["scale_offset"] = s
    for name, deg, sc in (("rot30", 30.0, (1.0, 1.0)), ("rot75_scaled", 75.0, (1.5, 0.7))):
        a = np.radians(deg); r = np.eye(3)
        r[:2, :2] = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) @ np.diag(sc)
        r[:2, 2] = np.array([0.5, 0.5]) - r[:2, :2] @ np.array([0.5, 0.5])
        out[name] = r
    return out


def bitmap_prop(mi, tex, to_uv=None, wrap="repeat", nearest=False):
    d = {"type": "bitmap", "data": np.ascontiguousarray(tex, F32), "raw": True}
    if to_uv is not None:
        d["to_uv"] = mi.ScalarTransform3f(np.asarray(to_uv, np.float64))
    if wrap != "repeat":
        d["wrap_mode"] = wrap
    if nearest:
        d["filter_type"] = "nearest"
    return d


def _wrap(i, n, mode):
    if mode == "clamp":
        return np.clip(i, 0, n - 1)
    if mode == "mirror":
        j = np.mod(i, 2 * n)
        return np.where(j < n, j, 2 * n - 1 - j)
    return np.mod(i, n)


def _texel_coords32(uv, to_uv, w, h):
    """the texel coordinates as the texture unit forms them, float32: uv through to_uv (two fused multiply-adds per row), times the resolution, minus a half"""
    u, v = np.asarray(uv[0], F32), np.asarray(uv[1], F32)
    if to_uv is not None:
        m = np.asarray(to_uv, F32)
        u, v = (N._fma(np.full_like(u, m[0, 1]), v, N._fma(np.full_like(u, m[0, 0]), u, m[0, 2])),
                N._fma(np.full_like(u, m[1, 1]), v, N._fma(np.full_like(u, m[1, 0]), u, m[1, 2])))
    return N._fma(u, F32(w), F32(-0.5)), N._fma(v, F32(h), F32(-0.5))


def eval_1_grad64(tex, uv, to_uv=None, wrap="repeat", nearest=False, values=None):
    """BitmapTexture::eval_1_grad (bitmap.cpp:543-599) in float64: the texel coordinates in float32 (the gradient is piecewise constant in one direction: the cell must be
    the product's), everything behind them in float64.  tex: h x w x 1 or x 3.  `values`: h x w float64 per-texel values instead of the channel / luminance.  2 x n"""
    h, w = tex.shape[:2]
    n = uv.shape[1]
    if nearest:
        return np.zeros((2, n))
    f = values if values is not None else (tex[:, :, 0].astype(np.float64) if tex.shape[2] == 1 else (tex.astype(np.float64) * LUM).sum(2))
    px, py = _texel_coords32(uv, to_uv, w, h)
    fx, fy = np.floor(px), np.floor(py)
    w1x, w1y = (px - fx).astype(np.float64), (py - fy).astype(np.float64); w0x, w0y = 1.0 - w1x, 1.0 - w1y
    x0, x1 = _wrap(fx.astype(np.int64), w, wrap), _wrap(fx.astype(np.int64) + 1, w, wrap)
    y0, y1 = _wrap(fy.astype(np.int64), h, wrap), _wrap(fy.astype(np.int64) + 1, h, wrap)
    f00, f10, f01, f11 = f[y0, x0], f[y0, x1], f[y1, x0], f[y1, x1]
    dfx = w0y * (f10 - f00) + w1y * (f11 - f01)
    dfy = w0x * (f01 - f00) + w1x * (f11 - f10)
    m = np.eye(3) if to_uv is None else np.asarray(to_uv, F32).astype(np.float64)
    return np.stack([w * (m[0, 0] * dfx + m[1, 0] * dfy), h * (m[0, 1] * dfx + m[1, 1] * dfy)])


def eval_1_grad32(tex, uv, to_uv=None):
    """the same for a bilinear + repeat bitmap with every operation in float32, in the order the product takes (tex_eval_1_grad, har_scene.h): the luminance as two adds of
    three products, the two differences as fmadd(w0, a, w1 * b), the matrix row as fmadd(m0, dfx, m1 * dfy), times the resolution.  2 x n float32"""
    f = F32
    h, w = tex.shape[:2]
    px, py = _texel_coords32(uv, to_uv, w, h)
    fx, fy = np.floor(px), np.floor(py)
    w1x, w1y = (px - fx).astype(f), (py - fy).astype(f); w0x, w0y = (f(1) - w1x).astype(f), (f(1) - w1y).astype(f)
    x0 = fx.astype(np.int64) % w; x1 = (fx.astype(np.int64) + 1) % w; y0 = fy.astype(np.int64) % h; y1 = (fy.astype(np.int64) + 1) % h
    t = tex.astype(f)
    if tex.shape[2] == 1:
        val = t[:, :, 0]
    else:
        val = (((t[:, :, 0] * f(LUM[0])).astype(f) + (t[:, :, 1] * f(LUM[1])).astype(f)).astype(f) + (t[:, :, 2] * f(LUM[2])).astype(f)).astype(f)
    f00, f10, f01, f11 = val[y0, x0], val[y0, x1], val[y1, x0], val[y1, x1]
    dfx = N._fma(w0y, (f10 - f00).astype(f), (w1y * (f11 - f01).astype(f)).astype(f))
    dfy = N._fma(w0x, (f01 - f00).astype(f), (w1x * (f11 - f10).astype(f)).astype(f))
    m = np.eye(3, dtype=f) if to_uv is None else np.asarray(to_uv, f)
    gu = (f(w) * N._fma(np.full_like(dfx, m[0, 0]), dfx, (m[1, 0] * dfy).astype(f))).astype(f)
    gv = (f(h) * N._fma(np.full_like(dfx, m[0, 1]), dfx, (m[1, 1] * dfy).astype(f))).astype(f)
    return np.stack([gu, gv])


def cell_margin(tex, uv, to_uv=None):
    """distance of the lookup from the nearest texel-cell border, in texels (the gradient jumps there)"""
    h, w = tex.shape[:2]
    px, py = _texel_coords32(uv, to_uv, w, h)
    frac = lambda p: np.minimum(p - np.floor(p), np.ceil(p) - p)
    return np.minimum(frac(px.astype(np.float64)), frac(py.astype(np.float64)))


def host_eval_1_grad(mi, scene, texture, uv, g=None, deposit=None):
    """har_texture_eval_1_grad_host: grad 2 x n (and, with g, the deposit accumulated into `deposit`, h x w x 3)"""
    n = uv.shape[1]
    uv = np.ascontiguousarray(uv, F32)
    grad = np.zeros((2, n), F32)
    d = scene.desc()
    gg = np.ascontiguousarray(g, F32) if g is not None else None
    rc = mi.lib().har_texture_eval_1_grad_host(C.byref(d), texture, n, B._fp(uv), B._fp(grad), B._fp(gg) if gg is not None else None, B._fp(deposit) if gg is not None else None)
    assert rc == 0, mi.lib().har_last_error()
    return grad


# ---- interactions

def _unit(v):
    return v / np.linalg.norm(v, axis=0, keepdims=True)


def _frame_about(sn, seed):
    """an orthonormal (s, t) pair about the unit normals sn (3 x n float64), at a random rotation about the normal: 3 x n each"""
    rng = np.random.default_rng(seed)
    a = np.where(np.abs(sn[0:1]) < 0.9, np.array([[1.0], [0.0], [0.0]]), np.array([[0.0], [1.0], [0.0]])) * np.ones_like(sn)
    s = _unit(a - sn * (a * sn).sum(0)); t = np.cross(sn.T, s.T).T
    ph = rng.uniform(0, 2 * np.pi, sn.shape[1])
    return s * np.cos(ph) + t * np.sin(ph), -s * np.sin(ph) + t * np.cos(ph)


def geometry(name, n, seed=41):
    """the fields of the interaction a bump frame reads, 18 x n float32 (si.n, sh_frame.n, .s, .t, dp_du, dp_dv):
      rectangle         a +z rectangle (rectangle.cpp: dp_du = (2, 0, 0), dp_dv = (0, 2, 0), the frame of coordinate_system)
      scaled_rectangle  the same rotated and scaled by (1.7, 0.6): dp_du, dp_dv of different lengths, a rotated frame
      smooth_mesh       a smooth-shaded mesh: the shading normal leans up to 25 degrees away from the geometric one, so it is NOT orthogonal to dp_du / dp_dv, which are
                        neither orthogonal nor of equal length"""
    rng = np.random.default_rng(seed)
    one = np.ones((1, n))
    if name == "rectangle":
        gn = np.array([[0.0], [0.0], [1.0]]) * one; sn = gn.copy()
        ss = np.array([[1.0], [0.0], [0.0]]) * one; st = np.array([[0.0], [1.0], [0.0]]) * one
        du = np.array([[2.0], [0.0], [0.0]]) * one; dv = np.array([[0.0], [2.0], [0.0]]) * one
    elif name == "scaled_rectangle":
        ax = np.array([0.3, 1.0, 0.2]); ax /= np.linalg.norm(ax); a = np.radians(50.0)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
        gn = (R @ np.array([0.0, 0.0, 1.0]))[:, None] * one; sn = gn.copy()
        ss, st = _frame_about(sn, seed + 1)
        du = (R @ np.array([3.4, 0.0, 0.0]))[:, None] * one; dv = (R @ np.array([0.0, 1.2, 0.0]))[:, None] * one
    else:
        gn = _unit(rng.normal(size=(3, n)))
        s0, t0 = _frame_about(gn, seed + 2)
        lean = np.tan(np.radians(rng.uniform(0.0, 25.0, n))); ph = rng.uniform(0, 2 * np.pi, n)
        sn = _unit(gn + (s0 * np.cos(ph) + t0 * np.sin(ph)) * lean)
        ss, st = _frame_about(sn, seed + 3)
        la, lb = rng.uniform(0.5, 2.5, n), rng.uniform(0.5, 2.5, n); skew = rng.uniform(-0.4, 0.4, n)
        du = s0 * la; dv = (t0 + s0 * skew) * lb          # in the face's plane, right-handed about gn
    return np.concatenate([gn, sn, ss, st, du, dv]).astype(F32)


def tilt_tan(geom, g):
    """tan of the angle between the bumped normal and the shading normal for the scaled height gradient g (2 x n), float64"""
    G = geom.astype(np.float64); sn, du, dv = G[3:6], G[12:15], G[15:18]
    dpu = sn * (g[0] - (sn * du).sum(0)) + du; dpv = sn * (g[1] - (sn * dv).sum(0)) + dv
    nrm = _unit(np.cross(dpu.T, dpv.T).T)
    c = np.abs((nrm * sn).sum(0))
    return np.sqrt(np.maximum(1 - c * c, 0)) / c


def height_case(mi, geom_name, uv, channels=1, seed=17):
    """(texels 3 x 5 x channels, to_uv 3 x 3, scale): a bilinear + repeat noise bitmap with to_uv (tests/blend_cases.py::TO_UV) whose `scale` is chosen so that the steepest
    lookup of the tuples tilts the normal by 60 degrees"""
    tex = noise(3, 5, channels, seed)
    m = np.eye(3); m[:2, :] = N.TO_UV
    g = eval_1_grad64(tex, uv, m)
    worst = float(tilt_tan(geometry(geom_name, uv.shape[1]), g).max())
    # tilt_tan is not linear in the scale for a leaning shading normal: bisect the scale at which the steepest lookup reaches 60 degrees
    lo, hi = 0.0, 4.0 * TAN60 / max(worst, 1e-9)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if float(tilt_tan(geometry(geom_name, uv.shape[1]), g * mid).max()) > TAN60:
            hi = mid
        else:
            lo = mid
    return tex, m, float(F32(lo))


def bumpmap_dict(mi, nested, texture, scale=1.0, flip=True, shadow=True):
    d = {"type": "bumpmap", "height": texture, "inner": N.nested_dict(nested) if isinstance(nested, str) else dict(nested)}
    if scale != 1.0:
        d["scale"] = float(scale)
    if not flip:
        d["flip_invalid_normals"] = False
    if not shadow:
        d["use_shadowing_function"] = False
    return d


# ---- bumpmap.cpp:224-253 in NumPy float32

def frame32(geom, g, wi, flip):
    """BumpMap::frame with float32 operations: (N.Frame relative to si.sh_frame, the geometric-flip product dot(si.n, n), the wi-flip product -- ones where flip is off)"""
    G = np.asarray(geom, F32); g = np.asarray(g, F32); wi = np.asarray(wi, F32)
    gn, sn, ss, st, du, dv = G[0:3], G[3:6], G[6:9], G[9:12], G[12:15], G[15:18]
    a = (g[0] - N._dot(sn, du)).astype(F32); b = (g[1] - N._dot(sn, dv)).astype(F32)
    dpu = np.stack([N._fma(sn[k], a, du[k]) for k in range(3)]); dpv = np.stack([N._fma(sn[k], b, dv[k]) for k in range(3)])
    n = N._normalize(N._cross(dpu, dpv))
    gprod = N._dot(gn, n)
    n = np.where((gprod < 0)[None, :], -n, n)
    n = np.stack([N._dot(n, ss), N._dot(n, st), N._dot(n, sn)])
    fprod = np.ones(n.shape[1], F32)
    if flip:
        fprod = (wi[2] * N._dot(wi, n)).astype(F32)
        n = np.where((fprod <= 0)[None, :], np.stack([-n[0], -n[1], n[2]]), n)
    q = N._dot(n, du)                                           # the literal line :249: the LOCAL n against the WORLD-space dp_du
    s = N._normalize(np.stack([N._fma(-n[k], q, du[k]) for k in range(3)]))
    t = N._cross(n, s)
    return N.Frame(s, t, n), gprod, fprod


def expected_eval_pdf(ch, ctx, geom, g, wi, uv, wo, flip, shadow):
    """BumpMap::eval_pdf (bumpmap.cpp:201-222): (value 3 x n, pdf n, active lanes, lanes within 1e-6 of one of the three switches)"""
    Fm, gprod, fprod = frame32(geom, g, wi, flip)
    pwi = Fm.to_local(wi); pwo = Fm.to_local(wo)
    oprod = (wo[2] * pwo[2]).astype(F32)
    active = oprod > 0
    val, pdf = ch.eval_pdf(ctx, pwi, uv, pwo)
    if shadow:
        with np.errstate(invalid="ignore"):
            val = (val * N.shadow_terminator(Fm.n, wo)[None, :]).astype(F32)
    val = np.where(active[None, :], val, F32(0)); pdf = np.where(active, pdf, F32(0))
    near = (np.abs(oprod) <= 1e-6) | (np.abs(fprod) <= 1e-6) | (np.abs(gprod) <= 1e-6)
    return val.astype(F32), pdf.astype(F32), active, near


def expected_sample(ch, ctx, geom, g, wi, uv, s1, s2, flip, shadow):
    """BumpMap::sample (bumpmap.cpp:137-162) per lane of a wavefront: dict as OracleScene.bsdf_sample_ctx returns it, plus `near`"""
    Fm, gprod, fprod = frame32(geom, g, wi, flip)
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
            weight = (weight * N.shadow_terminator(Fm.n, wo)[None, :]).astype(F32)
    return dict(wo=wo, pdf=np.where(active, r["pdf"], F32(0)).astype(F32), weight=np.where(active[None, :], weight, F32(0)).astype(F32), eta=r["eta"],
                sampled_type=r["sampled_type"], sampled_component=r["sampled_component"], active=active,
                near=(nonzero & (np.abs(oprod) <= 1e-6)) | (np.abs(fprod) <= 1e-6) | (np.abs(gprod) <= 1e-6))


# ---- the host entries that carry the interaction

def host_eval_pdf_si(mi, scene, index, ctx, wi, uv, wo, geom, active=None):
    from mitsuba3_amd import _capi
    n = wo.shape[1]
    f = lambda a: np.ascontiguousarray(a, F32)
    wi, uv, wo, geom = f(wi), f(uv), f(wo), f(geom)
    val = np.zeros((3, n), F32); pdf = np.zeros(n, F32)
    d = scene.desc()
    c = _capi.HarBSDFContext(ctx[0], ctx[1] & ALL, ctx[2] & ALL) if ctx is not None else None
    act = np.ascontiguousarray(active, np.uint8) if active is not None else None
    rc = mi.lib().har_bsdf_eval_pdf_si_host(C.byref(d), index, C.byref(c) if c is not None else None, n, B._fp(wi), B._fp(uv), B._fp(wo), B._fp(geom),
                                            act.ctypes.data_as(C.c_void_p) if act is not None else None, B._fp(val), B._fp(pdf))
    assert rc == 0, mi.lib().har_last_error()
    return val, pdf


def host_sample_si(mi, scene, index, ctx, wi, uv, s1, s2, geom, active=None):
    from mitsuba3_amd import _capi
    n = s2.shape[1]
    f = lambda a: np.ascontiguousarray(a, F32)
    wi, uv, s1, s2, geom = f(wi), f(uv), f(s1), f(s2), f(geom)
    wo = np.zeros((3, n), F32); pdf = np.zeros(n, F32); w = np.zeros((3, n), F32); eta = np.zeros(n, F32)
    st = np.zeros(n, np.uint32); sc = np.zeros(n, np.uint32)
    d = scene.desc()
    c = _capi.HarBSDFContext(ctx[0], ctx[1] & ALL, ctx[2] & ALL) if ctx is not None else None
    act = np.ascontiguousarray(active, np.uint8) if active is not None else None
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    rc = mi.lib().har_bsdf_sample_si_host(C.byref(d), index, C.byref(c) if c is not None else None, n, B._fp(wi), B._fp(uv), B._fp(s1), B._fp(s2), B._fp(geom),
                                          act.ctypes.data_as(C.c_void_p) if act is not None else None, B._fp(wo), B._fp(pdf), B._fp(w), B._fp(eta), u32(st), u32(sc))
    assert rc == 0, mi.lib().har_last_error()
    return dict(wo=wo, pdf=pdf, weight=w, eta=eta, sampled_type=st, sampled_component=sc)


def host_bump_grad(mi, scene, index, wi, uv, wo, geom, A, grad_uv=None):
    """har_bumpmap_grad_host: (F n, dF / d grad_uv 2 x n) for F = sum_k A_k value_k; grad_uv replaces the looked-up gradient"""
    n = wo.shape[1]
    f = lambda a: np.ascontiguousarray(a, F32)
    wi, uv, wo, geom, A = f(wi), f(uv), f(wo), f(geom), f(A)
    g = f(grad_uv) if grad_uv is not None else None
    val = np.zeros(n, F32); grad = np.zeros((2, n), F32)
    d = scene.desc()
    rc = mi.lib().har_bumpmap_grad_host(C.byref(d), index, n, B._fp(wi), B._fp(uv), B._fp(wo), B._fp(geom), B._fp(A), B._fp(g) if g is not None else None, B._fp(val), B._fp(grad))
    assert rc == 0, mi.lib().har_last_error()
    return val, grad


class SI:
    """what BSDF.eval / pdf / sample read of an interaction when the BSDF is a bumpmap"""

    def __init__(self, wi, uv, geom):
        self.wi, self.uv = wi, uv
        self.n = geom[0:3]; self.sh_frame = type("Frame3f", (), dict(n=geom[3:6], s=geom[6:9], t=geom[9:12]))()
        self.dp_du, self.dp_dv = geom[12:15], geom[15:18]


# ---- the per-call derivative: bumpmap.cpp in float64 as a function of grad_uv

def weighted_value64(ch, geom, g, wi, uv, wo, A, flip, shadow, masks=None):
    """F = sum_k A_k value_k with the FRAME and the shadow term in float64; the nested values come from OracleScene.bsdf_evaluate_ctx (float32) at the perturbed directions
    rounded to float32.  `masks`: the two flips decided beforehand (a finite difference keeps the branches of its centre).  Returns (F, (geometric flip, wi flip) masks,
    the three switch products)."""
    G = np.asarray(geom, np.float64); g = np.asarray(g, np.float64); wi64 = np.asarray(wi, np.float64); wo64 = np.asarray(wo, np.float64)
    gn, sn, ss, st, du, dv = G[0:3], G[3:6], G[6:9], G[9:12], G[12:15], G[15:18]
    dpu = sn * (g[0] - (sn * du).sum(0)) + du; dpv = sn * (g[1] - (sn * dv).sum(0)) + dv
    n = _unit(np.cross(dpu.T, dpv.T).T)
    gprod = (gn * n).sum(0)
    gf = (gprod < 0) if masks is None else masks[0]
    n = np.where(gf[None, :], -n, n)
    n = np.stack([(n * ss).sum(0), (n * st).sum(0), (n * sn).sum(0)])
    fprod = wi64[2] * (wi64 * n).sum(0) if flip else np.ones(n.shape[1])
    ff = ((fprod <= 0) if masks is None else masks[1]) if flip else np.zeros(n.shape[1], bool)
    n = np.where(ff[None, :], np.stack([-n[0], -n[1], n[2]]), n)
    s = _unit(du - n * (n * du).sum(0))
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
    return (np.asarray(A, np.float64) * val).sum(0), (gf, ff), (gprod, fprod, oprod)


def grad_tuples(n=5000, seed=11):
    """(wi, uv, wo, A, geom, g): directions over the upper hemisphere mostly (a tenth below: zero lanes), the smooth-mesh interactions, scaled height gradients that tilt
    the normal by up to about 50 degrees"""
    rng = np.random.default_rng(seed)

    def hemi(m):
        z = rng.uniform(0.05, 1, m) * np.where(rng.random(m) < 0.1, -1.0, 1.0)
        ph = rng.uniform(0, 2 * np.pi, m); r = np.sqrt(1 - z * z)
        return np.stack([r * np.cos(ph), r * np.sin(ph), z]).astype(F32)

    wi, wo = hemi(n), hemi(n)
    geom = geometry("smooth_mesh", n, seed + 1)
    mag = np.tan(np.radians(rng.uniform(5.0, 50.0, n))); ph = rng.uniform(0, 2 * np.pi, n)
    G = geom.astype(np.float64)
    g = np.stack([mag * np.cos(ph) * np.linalg.norm(G[12:15], axis=0), mag * np.sin(ph) * np.linalg.norm(G[15:18], axis=0)]).astype(F32)
    uv = rng.uniform(0, 1, (2, n)).astype(F32)
    return wi, uv, wo, rng.uniform(0.2, 1.5, (3, n)).astype(F32), geom, g


# ---- scenes

def plane_height(a, b, res=8):
    """res x res x 1 texels of the height a u + b v over the SURFACE's uv, for a bitmap looked up through to_uv = scale 0.5, offset 0.25 (texture uv' = 0.5 uv + 0.25) with
    clamp wrapping: no lookup of uv in [0, 1]^2 reaches the border, and the bilinear interpolation of a plane is the plane; (texels, to_uv 3 x 3)"""
    yy, xx = np.mgrid[0:res, 0:res]
    up = (xx + 0.5) / res; vp = (yy + 0.5) / res
    h = a * (up - 0.25) / 0.5 + b * (vp - 0.25) / 0.5
    m = np.eye(3); m[0, 0] = m[1, 1] = 0.5; m[0, 2] = m[1, 2] = 0.25
    return h.astype(F32)[:, :, None], m


def plane_normal_colour(a, b):
    """the constant normal-map colour of the plane height on the untransformed rectangle (dp_du = (2, 0, 0), dp_dv = (0, 2, 0)): 0.5 + 0.5 normalize(-2a, -2b, 4)"""
    n = np.array([-2.0 * a, -2.0 * b, 4.0]); n /= np.linalg.norm(n)
    return [float(x) for x in 0.5 + 0.5 * n]


def unit_rectangle_scene(mi, bsdf, res=(16, 12), spp=4, integrator="path", max_depth=4, rr_depth=8):
    d = N.lit_scene(mi, bsdf, "rectangle", res, spp, integrator=integrator, max_depth=max_depth, rr_depth=rr_depth, area_light=True)
    d["card"] = {"type": "rectangle", "bsdf": {"type": "ref", "id": "mat"}}
    return d


def smooth_mesh(k=6, half=1.0, bulge=0.25):
    """an OBJ-style smooth-shaded mesh WITH vertex normals and texture coordinates (what a `normalmap` refuses): a (k + 1)^2 grid over [-half, half]^2 bulging upwards, the
    normals those of the bulge -- so that sh_n is not orthogonal to the faces' dp_du"""
    xs = np.linspace(-half, half, k + 1)
    X, Y = np.meshgrid(xs, xs)
    Z = bulge * (1 - (X / half) ** 2) * (1 - (Y / half) ** 2)
    P = np.stack([X, Y, Z], -1).reshape(-1, 3)
    dzx = bulge * (-2 * X / half ** 2) * (1 - (Y / half) ** 2); dzy = bulge * (1 - (X / half) ** 2) * (-2 * Y / half ** 2)
    Nn = np.stack([-dzx, -dzy, np.ones_like(X)], -1).reshape(-1, 3); Nn /= np.linalg.norm(Nn, axis=1, keepdims=True)
    UV = np.stack([(X + half) / (2 * half), (Y + half) / (2 * half)], -1).reshape(-1, 2)
    F = []
    for j in range(k):
        for i in range(k):
            a = j * (k + 1) + i
            F += [[a, a + 1, a + k + 2], [a, a + k + 2, a + k + 1]]
    return {"type": "mesh", "positions": P.astype(F32), "faces": np.array(F, np.uint32), "normals": Nn.astype(F32), "texcoords": UV.astype(F32)}


def bumpy_height(h=6, w=8, channels=1, seed=5, amplitude=0.12):
    """h x w x channels noise whose steepest texel difference tilts the unit rectangle's normal by less than 50 degrees at scale 1 (gradient = resolution * difference / |dp_du|)"""
    return (noise(h, w, channels, seed) * amplitude).astype(F32)


def lit_scene(mi, bsdf, shape="rectangle", res=(32, 24), spp=16, integrator="path", max_depth=6, rr_depth=7, area_light=True, top_camera=False, wrap=None, instanced=False):
    """N.lit_scene with the shapes of the bump tests: a rectangle, a flat mesh, the smooth mesh with normals and texcoords; `wrap`: a function applied to the BSDF dict (an
    outer twosided); `instanced`: the shape moves into a shape group that one instance places"""
    d = N.lit_scene(mi, wrap(bsdf) if wrap else bsdf, "rectangle" if shape != "flat_mesh" else "mesh", res, spp, integrator=integrator, max_depth=max_depth, rr_depth=rr_depth,
                    area_light=area_light, top_camera=top_camera)
    if shape == "smooth_mesh":
        d["card"] = dict(smooth_mesh(), bsdf={"type": "ref", "id": "mat"})
    if instanced:
        T = mi.ScalarTransform4f
        d["grp"] = {"type": "shapegroup", "card": d.pop("card")}
        d["placed"] = {"type": "instance", "to_world": T().translate([0.05, -0.05, 0.1]).rotate([0, 0, 1], 15.0), "g": {"type": "ref", "id": "grp"}}
    return d


def bump_bsdf(mi, nested="roughplastic", channels=1, seed=5, scale=1.0, to_uv=True, amplitude=0.12):
    m = np.eye(3); m[:2, :] = N.TO_UV
    return bumpmap_dict(mi, nested, bitmap_prop(mi, bumpy_height(6, 8, channels, seed, amplitude), m if to_uv else None), scale)
