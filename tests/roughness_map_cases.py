"""Shared cases of the roughness-map tests (test_roughness_map_cpu.py, test_gpu_roughness_map.py): a `roughconductor` whose `alpha` (or `alpha_u` / `alpha_v`) is a bitmap.

THE TWIN.  The product renders the K x K quad card of the mask tests (tests/mask_cases.py: card_quads) with ONE roughconductor whose alpha is a K x K map; the oracle, which
knows constant roughness only, renders the same quads with K * K constant-alpha records:
  * nearest: the texcoords of quad (j, i) lie strictly inside texel (j, i) (card_quads), record (j, i) gets that texel;
  * bilinear / wrap / mirror / clamp / to_uv / luminance: the uv island of quad q is shrunk to a square of half-width ISLAND around an arbitrary point uv_q (outside
    [0, 1] and off the texel centres included), and record q gets exactly the float32 value the host alpha entry (har_bsdf_alpha_host) returns at uv_q.
ISLAND = 2e-6, the half-width the issue names.  It does NOT hold alpha to 1e-6 relative across a quad, as the issue supposes: a bilinear lookup of a 4 x 4 map with
texels in [0.05, 0.6] moves by up to |d alpha / d uv| * ISLAND * sqrt(2) <= (0.55 * 4 * |to_uv| 1.7) * 2.8e-6 = 1.1e-5 absolute, i.e. up to 2e-4 of the smallest alpha, and the
float32 texcoords of an island near |uv| = 2 are themselves 2.4e-7 apart.  The bound that is verified on the cases themselves (island_spread, asserted in
test_roughness_map_cpu.py::test_island_bound) is 3e-5 of the smallest alpha of the card; measured 1.6e-5.  That is far inside what the render bar needs: a relative change d
of alpha changes the radiance of that quad by O(d), and the measured render difference to the oracle's twin is 9.1e-8 on the host and 1.6e-7 on the device (docs/parity.md).  Both sides draw the same numbers
along the same rays, and the quads' texcoords are the only difference between the scenes."""
import ctypes as C

import numpy as np

from tests import blend_cases as B
from tests import mask_cases as MC

K = MC.K
ISLAND = 2e-6
LUM = np.array([0.212671, 0.715160, 0.072169], np.float64)
ETA = [0.2, 0.9, 1.1]; KC = [3.9, 2.4, 2.2]; SPEC = [0.9, 0.8, 0.7]


def texels(seed, h=K, w=K, channels=1):
    """h x w x channels texels whose eval_1 value lies in [0.05, 0.6]"""
    r = np.random.default_rng(seed)
    return (0.05 + 0.55 * r.random((h, w, channels))).astype(np.float32)


def bitmap(mi, data, filter_type="bilinear", wrap_mode="repeat", to_uv=None):
    d = {"type": "bitmap", "data": np.asarray(data, np.float32), "raw": True, "filter_type": filter_type, "wrap_mode": wrap_mode}
    if to_uv is not None:
        d["to_uv"] = to_uv
    return d


def to_uv(mi):
    return mi.ScalarTransform3f().translate([0.13, -0.21]).rotate(25.0).scale([1.7, 0.8])


def conductor(alpha=None, alpha_u=None, alpha_v=None, distribution="ggx", sample_visible=True, spec=None):
    d = {"type": "roughconductor", "distribution": distribution, "sample_visible": sample_visible, "eta": {"type": "rgb", "value": ETA}, "k": {"type": "rgb", "value": KC},
         "specular_reflectance": {"type": "rgb", "value": SPEC if spec is None else spec}}
    if alpha is not None:
        d["alpha"] = alpha
    else:
        d["alpha_u"] = alpha_u; d["alpha_v"] = alpha_v
    return d


def uv_points(seed, k=K):
    """one arbitrary uv point per quad: outside [0, 1] and off the texel centres"""
    return (np.random.default_rng(seed).random((k, k, 2)) * 3.0 - 1.0).astype(np.float32)


def quads(z=0.55, points=None, tilt=0.0):
    """card_quads, with the uv island of quad (j, i) shrunk around points[j, i] when `points` is given"""
    out = []
    for P, F, uv, (j, i) in MC.card_quads(z, tilt=tilt):
        if points is not None:
            c = points[j, i].astype(np.float64)
            uv = np.array([[c[0] - ISLAND, c[1] - ISLAND], [c[0] + ISLAND, c[1] - ISLAND], [c[0] + ISLAND, c[1] + ISLAND], [c[0] - ISLAND, c[1] + ISLAND]], np.float32)
        out.append((P, F, uv, (j, i)))
    return out


def card_scene(mi, res, spp, records, ref, integrator="path", max_depth=6, rr_depth=7, points=None, instanced=False, extra=None):
    """mi.cornell_box() with the K x K quad card in front of the boxes.  records: {id: bsdf dict} added to the scene; ref(j, i) -> the id quad (j, i) carries."""
    d = mi.cornell_box()
    d["sensor"]["film"]["width"] = res[0]; d["sensor"]["film"]["height"] = res[1]
    d["sensor"]["sampler"] = {"type": "independent", "sample_count": spp}
    d["integrator"] = dict({"type": integrator, "max_depth": max_depth, "rr_depth": rr_depth}, **(extra or {}))
    for k, v in records.items():
        d[k] = v
    shapes = {}
    for P, F, uv, (j, i) in quads(points=points):
        shapes["card_%d_%d" % (j, i)] = {"type": "mesh", "faces": F, "positions": P, "texcoords": uv, "bsdf": {"type": "ref", "id": ref(j, i)}}
    if instanced:
        group = {"type": "shapegroup"}; group.update(shapes)
        d["cards"] = group; d["placed"] = {"type": "instance", "g": {"type": "ref", "id": "cards"}}
    else:
        d.update(shapes)
    return d


def product_scene(mi, res, spp, bsdf, **kw):
    """ONE record `rough` (a roughconductor with a roughness map, possibly wrapped) on every quad"""
    return card_scene(mi, res, spp, {"rough": bsdf}, lambda j, i: "rough", **kw)


def twin_scene(mi, res, spp, alpha_u, alpha_v, wrap=None, **kw):
    """K * K records `rough_<j>_<i>` with the constant float32 roughness alpha_u[j, i], alpha_v[j, i]; wrap(bsdf) -> the dict that carries it (twosided, ...)"""
    recs = {}
    for j in range(K):
        for i in range(K):
            b = conductor(alpha_u=float(alpha_u[j, i]), alpha_v=float(alpha_v[j, i]), **kw.get("bsdf_kw", {}))
            recs["rough_%d_%d" % (j, i)] = wrap(b, j, i) if wrap else b
    kw = {k: v for k, v in kw.items() if k != "bsdf_kw"}
    return card_scene(mi, res, spp, recs, lambda j, i: "rough_%d_%d" % (j, i), **kw)


def host_alpha(mi, scene, index, uv):
    """har_bsdf_alpha_host of record `index` of a product scene at uv (2 x n): (alpha_u, alpha_v), float32"""
    uv = np.ascontiguousarray(uv, np.float32); n = uv.shape[1]
    au = np.zeros(n, np.float32); av = np.zeros(n, np.float32)
    d = scene.desc()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = mi.lib().har_bsdf_alpha_host(C.byref(d), int(index), n, fp(uv), fp(au), fp(av))
    assert rc == 0, mi.lib().har_last_error()
    return au, av


def quad_alphas(mi, scene, index, points):
    """the K x K float32 roughness the host entry returns at the quads' uv points (nearest twin: pass the centres of the card_quads islands)"""
    uv = points.reshape(-1, 2).T
    au, av = host_alpha(mi, scene, index, uv)
    return au.reshape(K, K), av.reshape(K, K)


def centres():
    """the uv centre of quad (j, i) of card_quads: the centre of texel (j, i)"""
    c = np.zeros((K, K, 2), np.float32)
    for j in range(K):
        for i in range(K):
            c[j, i] = ((i + 0.5) / K, (j + 0.5) / K)
    return c


def island_spread(mi, scene, index, points):
    """max over the quads of |alpha(corner) - alpha(uv_q)| / alpha(uv_q) over the four corners of the island"""
    worst = 0.0
    a0u, a0v = quad_alphas(mi, scene, index, points)
    for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
        p = (points.astype(np.float64) + np.array([sx * ISLAND, sy * ISLAND])).astype(np.float32)
        au, av = quad_alphas(mi, scene, index, p)
        worst = max(worst, float(np.abs(au - a0u).max() / a0u.min()), float(np.abs(av - a0v).max() / a0v.min()))
    return worst


def rough_record(scene, name="rough"):
    """the roughconductor LEAF record(s) of the scene-level BSDF `name`: [front] or [front, back]"""
    b = next(x for x in scene.bsdf_objs if x.id == name)
    return [b] + ([b.back] if b.back is not None else [])


def lookup64(data, filter_type, wrap_mode, rows, uv):
    """Texture::eval_1 of an h x w x {1, 3} bitmap at uv (2 x n) by an independent lookup, after blend_cases.lookup_weight: the texel coordinates in float32 as the texture
    unit forms them (uv through the 2 x 3 `rows` of to_uv, times the resolution, minus a half), the interpolation and the luminance in float64 on a np.pad'ed image
    ('wrap' = repeat, 'symmetric' = mirror, 'edge' = clamp)"""
    tex = np.asarray(data, np.float64); Hh, Ww = tex.shape[:2]; R = 16
    big = np.pad(tex, ((R * Hh, R * Hh), (R * Ww, R * Ww), (0, 0)), mode={"repeat": "wrap", "mirror": "symmetric", "clamp": "edge"}[wrap_mode])
    t = lambda x, y: big[y + R * Hh, x + R * Ww]
    uv = np.asarray(uv); n = uv.shape[1]; out = np.zeros(n, np.float64)
    m = None if rows is None else np.asarray(rows, np.float32).reshape(2, 3)
    for i in range(n):
        u, v = np.float32(uv[0, i]), np.float32(uv[1, i])
        if m is not None:
            u, v = B._fma32(m[0, 1], v, B._fma32(m[0, 0], u, m[0, 2])), B._fma32(m[1, 1], v, B._fma32(m[1, 0], u, m[1, 2]))
        if filter_type == "nearest":
            c = t(int(np.floor(u * np.float32(Ww))), int(np.floor(v * np.float32(Hh))))
        else:
            px, py = B._fma32(u, Ww, -0.5), B._fma32(v, Hh, -0.5)
            x0, y0 = int(np.floor(px)), int(np.floor(py)); fx, fy = float(px - np.float32(x0)), float(py - np.float32(y0))
            c = (1 - fy) * ((1 - fx) * t(x0, y0) + fx * t(x0 + 1, y0)) + fy * ((1 - fx) * t(x0, y0 + 1) + fx * t(x0 + 1, y0 + 1))
        out[i] = c[0] if tex.shape[2] == 1 else float(c @ LUM)
    return out


def tap_weights64(h, w, filter_type, wrap_mode, rows, uv):
    """the float64 transpose of the lookup at ONE uv point: dense h x w weights (taps that wrap or mirror onto the same texel add up), by probing lookup64 with unit
    texels -- the lookup is linear in the texels"""
    out = np.zeros((h, w))
    for y in range(h):
        for x in range(w):
            e = np.zeros((h, w, 1)); e[y, x, 0] = 1.0
            out[y, x] = lookup64(e, filter_type, wrap_mode, rows, np.asarray(uv, np.float64).reshape(2, 1))[0]
    return out


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
