"""Shared cases of the `projector` tests (tests/test_projector_cpu.py, tests/test_gpu_projector.py): the emitter's configurations, an independent float64 restatement of
Projector::sample_direction (src/emitters/projector.cpp:202-244) with a float64 bitmap lookup in the pattern of tests/blend_cases.py::lookup_weight, the product's per-call
entries over arrays, the render scenes (the directional twin, the tilted textured plane, the projector-lit box), and the per-lane composition of a textured render from
oracle entries under a unit point light at the apex."""
import ctypes as C

import numpy as np

EPS1 = float(np.spacing(np.float32(1.0)))          # one float32 ulp at 1


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ---- bitmaps

def map53():
    """5 x 3 texels, three channels, in [0.1, 0.9]"""
    return np.random.default_rng(11).uniform(0.1, 0.9, (3, 5, 3)).astype(np.float32)


def map44(channels=1):
    """4 x 4 texels in [0.2, 1.2]"""
    return np.random.default_rng(12).uniform(0.2, 1.2, (4, 4, channels)).astype(np.float32)


TO_UV = np.array([[0.9, 0.2, 0.05], [-0.3, 1.1, 0.2]], np.float64)          # rows of the 2 x 3 affine map of the bilinear 5 x 3 map


def to_uv_prop(mi):
    m = np.eye(3); m[:2, :] = TO_UV
    return mi.ScalarTransform3f(m)


def lookup(tex, uv, nearest=False, wrap="repeat", to_uv=None):
    """BitmapTexture::eval at float64 uv (2 x n) -> (3 x n values in float64, distance of the texel coordinates to the nearest texel boundary in float32 ulp of the coordinates: a nearest
    lookup within rounding of one may pick the other texel).  np.pad supplies the wrap modes: 'wrap' = repeat, 'symmetric' = mirror, 'edge' = clamp."""
    tex = np.asarray(tex, np.float64)
    if tex.shape[2] == 1:
        tex = np.repeat(tex, 3, axis=2)
    H, W = tex.shape[:2]; R = 8
    big = np.pad(tex, ((R * H, R * H), (R * W, R * W), (0, 0)), mode={"repeat": "wrap", "mirror": "symmetric", "clamp": "edge"}[wrap])
    u, v = uv[0].astype(np.float64), uv[1].astype(np.float64)
    if to_uv is not None:
        u, v = to_uv[0, 0] * u + to_uv[0, 1] * v + to_uv[0, 2], to_uv[1, 0] * u + to_uv[1, 1] * v + to_uv[1, 2]
    t = lambda x, y: big[y + R * H, x + R * W]
    if nearest:
        px, py = u * W, v * H
        x, y = np.floor(px).astype(int), np.floor(py).astype(int)
        edge = np.minimum(np.abs(px - np.round(px)), np.abs(py - np.round(py))) / np.spacing(np.maximum(np.maximum(np.abs(px), np.abs(py)), 1.0).astype(np.float32)).astype(np.float64)
        return t(x, y).T, edge
    px, py = u * W - 0.5, v * H - 0.5
    x0, y0 = np.floor(px).astype(int), np.floor(py).astype(int)
    fx, fy = (px - x0)[:, None], (py - y0)[:, None]
    c = (1 - fy) * ((1 - fx) * t(x0, y0) + fx * t(x0 + 1, y0)) + fy * ((1 - fx) * t(x0, y0 + 1) + fx * t(x0 + 1, y0 + 1))
    return c.T, np.full(u.shape, 1e9)


# ---- the emitter's configurations of the per-call test

def transforms(mi):
    T = mi.ScalarTransform4f
    return {"identity": T(),
            "rotated": T().rotate([0, 1, 0], 35.0).rotate([1, 0, 0], -20.0),                            # rotation about two axes, no translation: every distance
            "placed": T().translate([0.4, -0.7, 1.3]).rotate([0, 0, 1], 50.0).rotate([1, 0, 0], 115.0)}      # ... and a position


def configs(mi):
    """name -> (projector properties without `type`, (bitmap or None, nearest, wrap, to_uv rows or None), transform name, (z_lo, z_hi)).
    A placed projector keeps z >= 1: the reference point's local z is a difference of world coordinates of the size of the translation, so its float32 value carries an
    ABSOLUTE error of that size's ulp, which a z of 1e-3 would turn into a relative error far above every bar (the arithmetic's, not the product's)."""
    t = transforms(mi)
    bm = lambda data, **kw: dict({"type": "bitmap", "data": data, "raw": True}, **kw)
    return {
        "constant_x": (dict(irradiance={"type": "rgb", "value": [0.9, 0.5, 0.3]}, scale=1.7, fov=40.0), (None, False, "repeat", None), "rotated", (1e-3, 1e3)),
        "constant_focal": (dict(irradiance={"type": "rgb", "value": [0.2, 0.4, 0.8]}, scale=0.6, focal_length="35mm"), (None, False, "repeat", None), "placed", (1.0, 1e3)),
        "bilinear53_to_uv_y": (dict(irradiance=bm(map53(), to_uv=to_uv_prop(mi)), scale=2.5, fov=50.0, fov_axis="y"), (map53(), False, "repeat", TO_UV), "placed", (1.0, 1e3)),
        "bilinear53_clamp_smaller": (dict(irradiance=bm(map53(), wrap_mode="clamp"), scale=1.0, fov=30.0, fov_axis="smaller"), (map53(), False, "clamp", None), "rotated", (1e-3, 1e3)),
        "bilinear53_mirror_larger": (dict(irradiance=bm(map53(), wrap_mode="mirror"), scale=0.8, fov=70.0, fov_axis="larger"), (map53(), False, "mirror", None), "identity", (1e-3, 1e3)),
        "nearest44_diagonal": (dict(irradiance=bm(map44(1), filter_type="nearest"), scale=1.2, fov=60.0, fov_axis="diagonal"), (map44(1), True, "repeat", None), "identity", (1e-3, 1e3)),
        "nearest44_rgb_mirror": (dict(irradiance=bm(map44(3), filter_type="nearest", wrap_mode="mirror"), scale=3.0, fov=45.0), (map44(3), True, "mirror", None), "rotated", (1e-3, 1e3)),
        "one_texel": (dict(irradiance=bm(np.full((1, 1, 3), 0.75, np.float32)), scale=1.5, fov=55.0, fov_axis="x"), (np.full((1, 1, 3), 0.75, np.float32), False, "repeat", None), "placed", (1.0, 1e3)),
    }


def x_fov_of(props, aspect):
    """parse_fov (src/render/sensor.cpp:142-196) restated"""
    if "fov" in props:
        fov = float(props["fov"]); axis = props.get("fov_axis", "x")
        if axis == "smaller":
            axis = "y" if aspect > 1 else "x"
        elif axis == "larger":
            axis = "x" if aspect > 1 else "y"
    else:
        fov = 2.0 * np.degrees(np.arctan(np.sqrt(36.0 ** 2 + 24.0 ** 2) / (2.0 * float(props["focal_length"][:-2])))); axis = "diagonal"
    if axis == "x":
        return fov
    if axis == "y":
        return float(np.degrees(2.0 * np.arctan(np.tan(0.5 * np.radians(fov)) * aspect)))
    return float(np.degrees(2.0 * np.arctan(np.tan(0.5 * np.radians(fov)) / np.sqrt(1.0 + 1.0 / aspect ** 2))))


def matrix64(T):
    m = np.eye(4); m[:3, :] = np.asarray(T.col_major_3x4(), np.float64).reshape(4, 3).T
    return m


def points(name, cfg, mi, n, seed=5):
    """n world-space reference points (3 x n, float32) for configuration `cfg`: random ones whose uv covers [-0.25, 1.25]^2 at log-uniform distances, and the special
    ones -- the frustum's four faces and four corners (uv at 0 / 1 and one float to either side), z at and one float around 0, z < 0, the axis."""
    props, (tex, _, _, _), tname, (z_lo, z_hi) = cfg
    M = matrix64(transforms(mi)[tname])
    rng = np.random.default_rng(seed + len(name))
    aspect = 1.0 if tex is None else tex.shape[1] / float(tex.shape[0])
    cot = 1.0 / np.tan(0.5 * np.radians(float(np.float32(x_fov_of(props, aspect)))))
    m00, m11 = -0.5 * cot, -0.5 * aspect * cot
    u = rng.uniform(-0.25, 1.25, n); v = rng.uniform(-0.25, 1.25, n)
    z = np.exp(rng.uniform(np.log(z_lo), np.log(z_hi), n))
    one = np.float32(1.0)
    # the borders of the unit square: exactly on them and one float to either side (lanes the comparison leaves out: at most 0.5 % of all lanes may be, so eight per
    # configuration, rotating through the six values), and 16 floats to either side (lanes it keeps)
    exact = np.array([0.0, -EPS1 / 2, EPS1 / 2, 1.0, float(np.nextafter(one, np.float32(0))), float(np.nextafter(one, np.float32(2)))])
    near = np.array([-16 * EPS1, 16 * EPS1, 1 - 16 * EPS1, 1 + 16 * EPS1])
    r = len(name)
    u[0:2] = exact[[r % 6, (r + 3) % 6]]; v[2:4] = exact[[(r + 1) % 6, (r + 4) % 6]]          # the four faces ...
    u[4:8] = exact[[r % 6, (r + 3) % 6, (r + 2) % 6, (r + 5) % 6]]; v[4:8] = exact[[(r + 3) % 6, r % 6, (r + 5) % 6, (r + 2) % 6]]      # ... and the four corners
    u[8:24] = np.repeat(near, 4); v[8:24] = np.tile(near, 4)
    u[24:32] = np.tile(near, 2); v[32:40] = np.tile(near, 2)
    u[40:44] = 0.5; v[40:44] = 0.5                                          # the axis (a texel boundary of an even-sized nearest map: left out there)
    x = (u - 0.5) / m00 * z; y = (v - 0.5) / m11 * z
    z[64:67] = [0.0, 1e-45, -1e-45]                                        # z at 0 and one float to either side (left out) ...
    z[67:80] = -np.exp(rng.uniform(np.log(max(z_lo, 0.05)), 0.0, 13))      # ... and behind the projector (kept)
    x[64:80] = rng.uniform(-0.2, 0.2, 16); y[64:80] = rng.uniform(-0.2, 0.2, 16)
    local = np.stack([x, y, z, np.ones(n)])
    return np.ascontiguousarray((M @ local)[:3], np.float32)


def expected(cfg, mi, ref_p):
    """Projector::sample_direction in float64 from the matrices: dict of d, dist, pdf, p, n, uv, spec (spec already masked), active, and `unsure`: the lanes whose
    float64 uv lies within 4 float32 ulp (at 1: the uv are O(1) sums) of a border of the unit square, whose |z| lies within 4 ulp (at the size of the world coordinates it
    is a difference of) of 0, or -- a nearest map -- whose texel coordinates lie within 4 ulp of a texel boundary"""
    props, (tex, nearest, wrap, to_uv), tname, _ = cfg
    T = transforms(mi)[tname] if isinstance(tname, str) else tname
    M = matrix64(T); Minv = matrix64(T.inverse())
    p = ref_p.astype(np.float64)
    n = p.shape[1]
    local = (Minv @ np.concatenate([p, np.ones((1, n))]))[:3]
    aspect = 1.0 if tex is None else tex.shape[1] / float(tex.shape[0])
    cot = 1.0 / np.tan(0.5 * np.radians(float(np.float32(x_fov_of(props, aspect)))))
    with np.errstate(all="ignore"):
        uv = np.stack([-0.5 * cot * local[0] / local[2] + 0.5, -0.5 * aspect * cot * local[1] / local[2] + 0.5])
        active = (uv >= 0).all(axis=0) & (uv <= 1).all(axis=0) & (local[2] > 0)
        size = np.maximum(np.abs(p).max(axis=0), np.abs(M[:3, 3]).max())
        unsure = (np.minimum(np.abs(uv), np.abs(uv - 1)).min(axis=0) <= 4 * EPS1) | (np.abs(local[2]) <= 4 * np.spacing(size.astype(np.float32)).astype(np.float64)) | ~np.isfinite(uv).all(axis=0)
        pos = M[:3, 3]; nrm = M[:3, 2]
        d = pos[:, None] - p
        dist = np.sqrt((d * d).sum(axis=0)); d = d / dist
        scale = float(np.float32(props["scale"]))
        if tex is None:
            val = np.repeat(np.asarray(props["irradiance"]["value"], np.float32).astype(np.float64)[:, None], n, axis=1)
        else:
            safe = np.where(active, uv, 0.5)
            val, edge = lookup(tex, safe, nearest, wrap, to_uv)
            unsure |= active & (edge <= 4)
        spec = val * (np.pi * scale / (local[2] ** 2 * -(nrm[:, None] * d).sum(axis=0)))
    spec = np.where(active, spec, 0.0)
    return dict(d=d, dist=dist, pdf=active.astype(np.float64), p=np.repeat(pos[:, None], n, axis=1), n=np.repeat(nrm[:, None], n, axis=1), uv=uv, spec=spec,
                active=active, unsure=unsure)


def config_scene(mi, cfg):
    """a scene that holds the configuration's projector as emitter 0 (and one rectangle: a scene needs a shape)"""
    props, _, tname, _ = cfg
    return mi.load_dict({"type": "scene", "rect": {"type": "rectangle"}, "light": dict({"type": "projector", "to_world": transforms(mi)[tname]}, **props)})


def host_sample_direction(mi, scene, emitter, ref_p, active=None):
    """har_emitter_sample_direction_host over arrays -> dict of d, dist, pdf, p, n, uv, spec"""
    n = ref_p.shape[1]
    ref_p = np.ascontiguousarray(ref_p, np.float32)
    out = dict(d=np.zeros((3, n), np.float32), dist=np.zeros(n, np.float32), pdf=np.zeros(n, np.float32), p=np.zeros((3, n), np.float32), n=np.zeros((3, n), np.float32),
               uv=np.zeros((2, n), np.float32), spec=np.zeros((3, n), np.float32))
    act = np.ascontiguousarray(active, np.uint8) if active is not None else None
    d = scene.desc()
    rc = mi.lib().har_emitter_sample_direction_host(C.byref(d), emitter, n, _fp(ref_p), None, act.ctypes.data_as(C.c_void_p) if act is not None else None,
                                                    *[_fp(out[k]) for k in ("d", "dist", "pdf", "p", "n", "uv", "spec")])
    assert rc == 0, mi.lib().har_last_error()
    return out


def device_sample_direction(mi, scene, emitter, ref_p, active=None):
    """har_emitter_sample_direction on the scene's device handle -> the same dict (numpy)"""
    import torch
    n = ref_p.shape[1]
    dev = torch.device("cuda")
    rp = torch.as_tensor(np.ascontiguousarray(ref_p, np.float32), device=dev)
    shapes = dict(d=(3, n), dist=(n,), pdf=(n,), p=(3, n), n=(3, n), uv=(2, n), spec=(3, n))
    out = {k: torch.full(s, -7.0, dtype=torch.float32, device=dev) for k, s in shapes.items()}
    act = torch.as_tensor(np.ascontiguousarray(active, np.uint8), device=dev) if active is not None else None
    mi.core.check(mi.lib().har_emitter_sample_direction(scene._handle(), emitter, n, rp.data_ptr(), None, act.data_ptr() if act is not None else None,
                                                        *[out[k].data_ptr() for k in ("d", "dist", "pdf", "p", "n", "uv", "spec")], None))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- render scenes

RHO = [0.6, 0.7, 0.8]


def twin_scene(mi, light, res=(16, 12), spp=4, integrator="path", max_depth=4, area=False, weights=(1.0, 1.0), batch=False, **iprops):
    """The directional twin's geometry with `light` as its delta emitter: a diffuse floor (the square |x|, |y| <= 0.5 at z = 0) perpendicular to the axis of a projector
    at (0, 0, h) looking down -- strictly inside the footprint of a 40 degree frustum at h = 2 (half width 0.728) -- and two diffuse walls |x| = 1.2 parallel to the axis,
    facing inward, strictly outside the frustum at every height.  `area`: an area light beside the floor as a second emitter; `weights`: (delta light, area light)."""
    T = mi.ScalarTransform4f
    cam = lambda ox: {"type": "perspective", "fov": 60, "to_world": T().look_at(origin=[ox, -3, 2.5], target=[0, 0, 0.5], up=[0, 0, 1]),
                      "film": {"type": "hdrfilm", "width": res[0], "height": res[1], "rfilter": {"type": "gaussian"}}}
    d = {"type": "scene", "integrator": dict({"type": integrator, "max_depth": max_depth, "rr_depth": 5}, **iprops),
         "floor": {"type": "rectangle", "to_world": T().scale([0.5, 0.5, 1]), "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": RHO}}},
         "w1": {"type": "rectangle", "to_world": T().translate([1.2, 0, 1]).rotate([0, 1, 0], -90), "bsdf": {"type": "diffuse"}},
         "w2": {"type": "rectangle", "to_world": T().translate([-1.2, 0, 1]).rotate([0, 1, 0], 90), "bsdf": {"type": "diffuse"}},
         "light": dict(light, sampling_weight=weights[0])}
    if area:
        # beside the floor, facing it: neither the vertical column under it (the directional light's shadow) nor the cone from the apex (the projector's) reaches a surface
        d["lamp"] = {"type": "rectangle", "to_world": T().look_at(origin=[0, 1.7, 1.2], target=[0, 0, 0.3], up=[0, 0, 1]).scale([0.3, 0.3, 1]),
                     "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [4.0, 3.0, 2.0]}, "sampling_weight": weights[1]}}
    if batch:
        d["sensor"] = {"type": "batch", "a": cam(0.3), "b": cam(-0.8), "film": {"type": "hdrfilm", "width": 2 * res[0], "height": res[1], "rfilter": {"type": "gaussian"}},
                       "sampler": {"type": "independent", "sample_count": spp}}
        for k in ("a", "b"):
            del d["sensor"][k]["film"]
    else:
        d["sensor"] = dict(cam(0.3), sampler={"type": "independent", "sample_count": spp})
    return d


TWIN_H = 2.0


def twin_lights(mi, s, c):
    """(projector, directional) of the twin: constant irradiance c and scale s at height h against E = pi s c / h^2 along the same axis"""
    tw = mi.ScalarTransform4f().look_at(origin=[0, 0, TWIN_H], target=[0, 0, 0], up=[0, 1, 0])
    E = [float(np.float32(np.pi * s * x / TWIN_H ** 2)) for x in c]
    return ({"type": "projector", "irradiance": {"type": "rgb", "value": list(c)}, "scale": s, "fov": 40.0, "to_world": tw},
            {"type": "directional", "irradiance": {"type": "rgb", "value": E}, "to_world": tw})


def pattern(w=16, h=12, seed=3, zero_block=False):
    t = np.random.default_rng(seed).uniform(0.2, 1.5, (h, w, 3)).astype(np.float32)
    if zero_block:
        t[2:6, 3:9] = 0.0
    return t


def projector_box(mi, data, scale=2.0, res=(32, 24), spp=16, integrator="prb", max_depth=6, nearest=False, **iprops):
    """mi.cornell_box() lit only by a textured projector under the ceiling that looks down"""
    d = mi.cornell_box()
    d["sensor"]["film"]["width"] = res[0]; d["sensor"]["film"]["height"] = res[1]
    d["sensor"]["sampler"] = {"type": "independent", "sample_count": spp}
    d["integrator"] = dict({"type": integrator, "max_depth": max_depth, "rr_depth": 5}, **iprops)
    d.pop("light", None)
    for k in [k for k, v in d.items() if isinstance(v, dict) and "emitter" in v]:
        del d[k]
    bm = {"type": "bitmap", "data": data, "raw": True}
    if nearest:
        bm["filter_type"] = "nearest"
    d["projector"] = {"type": "projector", "irradiance": bm, "scale": scale, "fov": 70.0,
                      "to_world": mi.ScalarTransform4f().look_at(origin=[0.0, 0.9, 0.0], target=[0.05, -1.0, 0.1], up=[0, 0, 1])}
    return d


# ---- the textured render, lane by lane, from oracle entries

def apex_transform(mi):
    return mi.ScalarTransform4f().look_at(origin=[0.3, -0.2, 2.2], target=[0.1, 0.1, 0.0], up=[0, 1, 0])


PLANE_MAPS = {
    "bilinear53_to_uv": (dict(data=map53(), to_uv=True), (map53(), False, "repeat", TO_UV)),
    "nearest44": (dict(data=map44(3), filter_type="nearest"), (map44(3), True, "repeat", None)),
}
PLANE_SCALE = 1.9
PLANE_FOV = 40.0


def plane_scene(mi, light, res=(32, 24), spp=16, integrator="path", max_depth=2, **iprops):
    """a diffuse plane tilted against the projector's axis (z and cos vary over it), wider than the 40 degree frustum's footprint (part of it is outside), with a small
    cube above it that shadows a patch; `light`: the projector, or the unit point light at its apex"""
    T = mi.ScalarTransform4f
    return {"type": "scene", "integrator": dict({"type": integrator, "max_depth": max_depth, "rr_depth": 5}, **iprops),
            "plane": {"type": "rectangle", "to_world": T().rotate([1, 0, 0], 28.0).rotate([0, 1, 0], -22.0).scale([1.6, 1.3, 1.0]),
                      "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": RHO}}},
            "block": {"type": "cube", "to_world": T().translate([0.25, -0.05, 0.9]).rotate([0, 0, 1], 30.0).scale(0.12), "bsdf": {"type": "diffuse"}},
            "light": light,
            "sensor": {"type": "perspective", "fov": 50, "to_world": T().look_at(origin=[-0.6, 0.5, 3.4], target=[0, 0, 0], up=[0, 1, 0]),
                       "film": {"type": "hdrfilm", "width": res[0], "height": res[1], "rfilter": {"type": "gaussian"}, "pixel_format": "rgb"},
                       "sampler": {"type": "independent", "sample_count": spp}}}


def plane_lights(mi, which, data=None):
    """(projector over bitmap `which` of PLANE_MAPS -- `data`: other texels of the same shape --, the unit point light at its apex, the configuration for `expected`)"""
    props, (tex, nearest, wrap, to_uv) = PLANE_MAPS[which]
    tex = tex if data is None else np.asarray(data, np.float32)
    bm = {"type": "bitmap", "data": tex, "raw": True}
    if props.get("to_uv"):
        bm["to_uv"] = to_uv_prop(mi)
    if "filter_type" in props:
        bm["filter_type"] = props["filter_type"]
    tw = apex_transform(mi)
    pj = {"type": "projector", "irradiance": bm, "scale": PLANE_SCALE, "fov": PLANE_FOV, "to_world": tw}
    pt = {"type": "point", "position": [float(x) for x in tw.col_major_3x4()[9:12]], "intensity": {"type": "rgb", "value": 1.0}}
    cfg = (dict(scale=PLANE_SCALE, fov=PLANE_FOV), (tex, nearest, wrap, to_uv), tw, None)
    return pj, pt, cfg


def composed_plane(mi, O, which, seed, spp, res=(32, 24), prb=False, data=None):
    """The expected per-lane radiance and raw film of the plane scene under the projector, composed from oracle entries: orc_sample_tea_32 + orc_pcg32_* for a lane's
    jitter and the sampler state behind it, orc_sensor_sample_ray for its ray, OracleScene.integrator_sample of the SAME scene under a unit point light at the apex
    (max_depth 2: only the camera ray's hit is lit, radiance f cos V / d^2; the projector draws the same sampler numbers), times the float64 factor
    pi s T(uv(x)) d^2 / (z^2 cos) at the hit x from OracleScene.ray_intersect (0 outside the frustum), then orc_film_put.  Returns a dict with the lanes (o, d, maxt,
    state), `rgb` (3 x n), `film` (H x W x 4), `unit` (the lanes' radiance per unit of the looked-up texel, 3 x n), `texel` (the nearest map's texel index y * W + x of
    every lit lane, -1 elsewhere)."""
    from tests import batch_cases as BC
    pj, pt, cfg = plane_lights(mi, which, data)
    scene = mi.load_dict(plane_scene(mi, pt, res=res, spp=spp, integrator="prb" if prb else "path"))
    osc, _ = O.scene_from_product(scene)
    wide = BC.oracle_sensor(O, scene.sensors()[0].har)
    W, H = wide.crop_width, wide.crop_height
    n = W * H * spp
    jit, state = BC.lane_streams(O, seed, n)
    p = np.arange(n) // spp
    ipos = np.stack([(p % W), (p // W)]).astype(np.float32); pos = (ipos + jit).astype(np.float32)
    px = np.ascontiguousarray((pos[0].astype(np.float64) * np.float64(np.float32(1.0) / np.float32(W))).astype(np.float32))
    py = np.ascontiguousarray((pos[1].astype(np.float64) * np.float64(np.float32(1.0) / np.float32(H))).astype(np.float32))
    o = np.zeros((3, n), np.float32); d = np.zeros((3, n), np.float32); mt = np.zeros(n, np.float32)
    O.lib().orc_sensor_sample_ray(C.byref(wide), n, O.fp(px), O.fp(py), O.fp(o), O.fp(d), O.fp(mt))
    unit_pt, _, _ = osc.integrator_sample(o, d, mt, seed=seed, lane_offset=0, state=state, max_depth=2, rr_depth=5, prb=prb)
    t = osc.ray_intersect(o, d, mt)[0]
    hit = np.isfinite(t)
    x = o.astype(np.float64) + np.where(hit, t, 0.0).astype(np.float64) * d.astype(np.float64)
    exp = expected(cfg, mi, x)          # spec = T(uv) pi s / (z^2 cos), masked by the frustum; dist = d
    lit = hit & exp["active"]
    with np.errstate(all="ignore"):
        factor = np.where(lit, exp["spec"] * exp["dist"] ** 2, 0.0)
        ones = (dict(scale=PLANE_SCALE, fov=PLANE_FOV, irradiance={"type": "rgb", "value": [1.0, 1.0, 1.0]}), (None, False, "repeat", None), cfg[2], None)
        e1 = expected((ones[0], (np.ones_like(cfg[1][0]), cfg[1][1], cfg[1][2], cfg[1][3]), cfg[2], None), mi, x)
        unit = np.where(lit, e1["spec"] * e1["dist"] ** 2, 0.0) * unit_pt.astype(np.float64)
    rgb = (unit_pt.astype(np.float64) * factor).astype(np.float32)
    lanes = dict(n=n, ipos=ipos, pos=pos)
    film = BC.film_put(O, wide, "gaussian", lanes, rgb)
    tex = cfg[1][0]; th, tw_ = tex.shape[:2]
    texel = np.where(lit, (np.floor(exp["uv"][1] * th).astype(np.int64) % th) * tw_ + (np.floor(exp["uv"][0] * tw_).astype(np.int64) % tw_), -1) if cfg[1][1] else None
    return dict(o=o, d=d, maxt=mt, state=state, rgb=rgb, film=film, unit=unit, texel=texel, lanes=lanes, wide=wide, lit=lit, hit=hit, unsure=exp["unsure"] & hit, n=n)


def composed_texel_gradient(O, comp, grad_in, shape):
    """d sum(grad_in * developed image) / d T_t of the nearest map from the composition restricted to texel t: film_put of the lanes that look texel t up, per unit of
    the texel, developed with the film's weights"""
    from tests import batch_cases as BC
    th, tw_ = shape[:2]
    w = comp["film"][:, :, 3:4].astype(np.float64)
    g = np.zeros((th, tw_, 3))
    for t in range(th * tw_):
        part = np.where(comp["texel"] == t, comp["unit"], 0.0).astype(np.float32)
        film = BC.film_put(O, comp["wide"], "gaussian", comp["lanes"], part)
        g[t // tw_, t % tw_] = (np.asarray(grad_in, np.float64) * film[:, :, :3] / np.where(w == 0, 1.0, w)).sum(axis=(0, 1))
    return g


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
