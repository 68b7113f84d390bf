"""Shared inputs and the oracle-side composition of the `aov` tests (tests/test_aov_cpu.py, tests/test_gpu_aov.py).

An AOV is a function of the camera ray's surface interaction, so the expected values are composed from oracle calls that exist for other reasons:
OracleScene.ray_intersect -> .surface_interaction_flags rows -> (albedo) an independent NumPy texture lookup or .bsdf_evaluate_ctx(eval, wo = (0, 0, 1)) * pi.
The expected film is those values accumulated with orc_film_put at film positions rebuilt from orc_sampler_stream."""
import ctypes as C

import numpy as np

ALL_TYPES = ["albedo", "depth", "position", "uv", "geo_normal", "sh_normal", "dp_du", "dp_dv", "prim_index", "shape_index"]
CHANNELS = {"albedo": 3, "depth": 1, "position": 3, "uv": 2, "geo_normal": 3, "sh_normal": 3, "dp_du": 3, "dp_dv": 3, "prim_index": 1, "shape_index": 1}
ALL_SPEC = ",".join("a%d:%s" % (i, t) for i, t in enumerate(ALL_TYPES))
RADIUS = {"box": 0.5, "gaussian": 2.0, "catmullrom": 2.0}          # gaussian: 4 * stddev at the default stddev of 0.5
RAY_EPS = 5.9604644775390625e-8 * 1500.0


def channel_slices(types):
    out = {}; c = 0
    for t in types:
        out[t] = slice(c, c + CHANNELS[t]); c += CHANNELS[t]
    return out, c


def curved_patch(n=9):
    """a spherical cap as a triangle grid with vertex normals and texcoords"""
    u, v = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing="xy")
    a = (u - 0.5) * 1.2; b = (v - 0.5) * 1.2
    nrm = np.stack([np.sin(a) * np.cos(b), np.sin(b), np.cos(a) * np.cos(b)], -1).reshape(-1, 3)
    pos = nrm * 0.8
    uv = np.stack([u, v], -1).reshape(-1, 2)
    faces = []
    for j in range(n - 1):
        for i in range(n - 1):
            k = j * n + i
            faces += [[k, k + 1, k + n + 1], [k, k + n + 1, k + n]]
    return pos.astype(np.float32), nrm.astype(np.float32), uv.astype(np.float32), np.asarray(faces, np.uint32)


def feature_scene(mi, res=48, spp=8, rfilter="gaussian", film_extra=None, integrator=None):
    """every BSDF model, a bitmap albedo with a non-identity to_uv, a `twosided` front / back pair that is seen from both sides, an instanced shape group and a
    mesh with vertex normals"""
    T = mi.ScalarTransform4f
    tex = np.random.default_rng(5).uniform(0.05, 0.95, (6, 11, 3)).astype(np.float32)
    pos, nrm, uv, faces = curved_patch()
    film = {"type": "hdrfilm", "width": res, "height": res, "rfilter": {"type": rfilter}, "pixel_format": "rgb"}
    film.update(film_extra or {})
    d = {
        "type": "scene",
        "integrator": integrator or {"type": "path", "max_depth": 4},
        "sensor": {"type": "perspective", "fov": 50.0, "near_clip": 0.01, "far_clip": 100.0,
                   "to_world": T().look_at(origin=[0.4, 1.2, 6.0], target=[0, 0, 0], up=[0, 1, 0]),
                   "sampler": {"type": "independent", "sample_count": spp}, "film": film},
        "lamp": {"type": "rectangle", "to_world": T().translate([0.0, 3.5, 0.0]).rotate([1, 0, 0], 90).scale([0.8, 0.8, 0.8]),
                 "bsdf": {"type": "diffuse"}, "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [9.0, 8.0, 7.0]}}},
        "floor": {"type": "rectangle", "to_world": T().translate([0.0, -1.5, 0.0]).rotate([1, 0, 0], -90).scale([3.0, 3.0, 1.0]),
                  "bsdf": {"type": "diffuse", "reflectance": {"type": "bitmap", "data": tex, "raw": True,
                                                              "to_uv": mi.ScalarTransform3f().translate([0.13, -0.27]).rotate(25.0).scale([2.0, 3.0])}}},
        "pair": {"type": "rectangle", "to_world": T().translate([-1.6, 0.2, 0.0]).rotate([0, 1, 0], 60).scale([0.7, 0.9, 1.0]),
                 "bsdf": {"type": "twosided",
                          "front": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.1, 0.1]}},
                          "back": {"type": "plastic", "diffuse_reflectance": {"type": "rgb", "value": [0.1, 0.2, 0.8]}}}},
        "single": {"type": "rectangle", "to_world": T().translate([1.7, 0.3, -0.4]).rotate([0, 1, 0], -55).scale([0.6, 0.8, 1.0]),
                   "bsdf": {"type": "twosided", "only": {"type": "roughconductor", "alpha": 0.3}}},
        "glass": {"type": "cube", "to_world": T().translate([-0.7, -1.1, 1.2]).rotate([0, 1, 0], 20).scale(0.35), "bsdf": {"type": "dielectric"}},
        "metal": {"type": "cube", "to_world": T().translate([0.8, -1.1, 1.3]).rotate([0, 1, 0], -30).scale(0.3), "bsdf": {"type": "conductor"}},
        "rough": {"type": "rectangle", "to_world": T().translate([0.0, 0.4, -2.0]).scale([2.5, 1.8, 1.0]),
                  "bsdf": {"type": "roughplastic", "alpha": 0.15, "diffuse_reflectance": {"type": "rgb", "value": [0.3, 0.6, 0.2]}}},
        "cap": {"type": "mesh", "faces": faces, "positions": pos, "normals": nrm, "texcoords": uv, "to_world": T().translate([0.0, -0.2, 0.3]),
                "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.5, 0.5, 0.2]}}},
        "group": {"type": "shapegroup",
                  "box": {"type": "cube", "to_world": T().scale(0.25), "bsdf": {"type": "plastic", "diffuse_reflectance": {"type": "rgb", "value": [0.2, 0.7, 0.7]}}}},
        "inst0": {"type": "instance", "shapegroup": {"type": "ref", "id": "group"}, "to_world": T().translate([-1.2, 1.4, 0.5]).rotate([1, 1, 0], 35)},
        "inst1": {"type": "instance", "shapegroup": {"type": "ref", "id": "group"}, "to_world": T().translate([1.3, 1.5, 0.2]).rotate([0, 1, 1], -50).scale([1.5, 0.8, 1.0])},
    }
    return d


def feature_rays(n=20480, seed=3):
    """rays from all around the scene (both sides of every rectangle) towards points of its bounding box and beyond it: a share of them miss"""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=(3, n)); w /= np.linalg.norm(w, axis=0)
    o = (7.0 * w).astype(np.float32)
    target = rng.uniform(-3.2, 3.2, (3, n))
    d = target - o; d /= np.linalg.norm(d, axis=0)
    d = d.astype(np.float32); d /= np.linalg.norm(d, axis=0).astype(np.float32)
    maxt = np.full(n, np.inf, np.float32)
    active = rng.uniform(size=n) > 0.1
    return o, d.astype(np.float32), maxt, active


def numpy_texture(tex, to_uv, u, v):
    """bilinear + repeat lookup of a raw H x W x 3 bitmap at to_uv * (u, v) (the independent lookup of tests/test_bsdfs_cpu.py, with the affine map in front)"""
    Hh, Ww, _ = tex.shape
    if to_uv is not None:
        m = np.asarray(to_uv, np.float64).reshape(2, 3)
        u, v = m[0, 0] * u + m[0, 1] * v + m[0, 2], m[1, 0] * u + m[1, 1] * v + m[1, 2]
    px, py = u * Ww - 0.5, v * Hh - 0.5
    x0, y0 = int(np.floor(px)), int(np.floor(py)); fx, fy = float(px - x0), float(py - y0)
    t = lambda x, y: tex[y % Hh, x % Ww].astype(np.float64)
    return (1 - fy) * ((1 - fx) * t(x0, y0) + fx * t(x0 + 1, y0)) + fy * ((1 - fx) * t(x0, y0 + 1) + fx * t(x0 + 1, y0 + 1))


def oracle_aovs(O, scene, osc, types, o, d, maxt, active=None):
    """(C x n expected values, hit mask, per-lane albedo kind: 0 none, 1 texture / constant, 2 base-class eval) from oracle calls"""
    n = maxt.shape[0]
    act = np.ones(n, bool) if active is None else np.asarray(active, bool)
    t, u, v, prim, shape, inst = osc.ray_intersect_masked(o, d, maxt, act.astype(np.uint8)) if active is not None else osc.ray_intersect(o, d, maxt)
    hit = act & np.isfinite(t)
    rows = osc.surface_interaction_flags(o, d, t, u, v, prim, shape, inst, ray_flags=1, active=hit)
    sl, count = channel_slices(types)
    out = np.zeros((count, n), np.float64); kind = np.zeros(n, np.int32)
    for name, r in (("position", slice(0, 3)), ("geo_normal", slice(3, 6)), ("sh_normal", slice(6, 9)), ("uv", slice(18, 20)), ("depth", slice(20, 21)),
                    ("dp_du", slice(21, 24)), ("dp_dv", slice(24, 27))):
        if name in sl:
            out[sl[name]] = np.where(hit, rows[r], 0.0)
    if "prim_index" in sl:
        out[sl["prim_index"]] = np.where(hit, prim.astype(np.float64), 0.0)
    if "shape_index" in sl:
        has_inst = inst != 0xffffffff
        out[sl["shape_index"]] = np.where(hit, np.where(has_inst, scene.top_mesh_count + inst.astype(np.int64) + 1, shape.astype(np.int64) + 1), 0)
    if "albedo" in sl:
        base = {}            # BSDF record -> lanes served by the base-class eval
        for i in np.nonzero(hit)[0]:
            b = scene.bsdf_objs[scene.meshes[int(shape[i])]["bsdf"]]
            wi = rows[15:18, i].astype(np.float32).copy()
            if b.flags & 1:                                  # twosided.cpp:284-307
                if b.back is None:
                    wi[2] = abs(wi[2])
                elif wi[2] < 0:
                    b = b.back; wi[2] = -wi[2]
                elif wi[2] == 0:
                    continue
            if b.kind in ("diffuse", "plastic", "roughplastic"):
                kind[i] = 1
                out[sl["albedo"], i] = numpy_texture(b.texture, b.tex_to_uv, float(rows[18, i]), float(rows[19, i])) if b.texture is not None else np.asarray(b.value, np.float64)
            else:
                kind[i] = 2
                base.setdefault(b.index, []).append((i, wi))
        for index, lanes in base.items():
            ids = np.asarray([l[0] for l in lanes]); wi = np.stack([l[1] for l in lanes], 1)
            wo = np.zeros((3, len(ids)), np.float32); wo[2] = 1.0
            val, _ = osc.bsdf_evaluate_ctx(index, (0, 0x1ff, 0xffffffff), 0, wi, rows[18:20, ids], wo)
            out[sl["albedo"]][:, ids] = (val * np.float32(np.pi)).astype(np.float64)
    return out, hit, kind


def border_of(rfilter):
    return int(np.ceil(RADIUS[rfilter] - 0.5 - 2.0 * RAY_EPS))


def lane_positions(O, sensor, rfilter, seed, spp):
    """film positions of the lanes of render() (integrator.cpp:322-345): lane = pixel * spp + sample over the sample grid (the crop window, enlarged by the filter border
    with Film::sample_border), position = pixel - border + crop offset + the first two numbers of the lane's sampler stream.  Returns (ipos 2 x n, pos 2 x n)."""
    border = border_of(rfilter) if sensor.sample_border else 0
    gw, gh = sensor.crop_width + 2 * border, sensor.crop_height + 2 * border
    n = gw * gh * spp
    lane = np.arange(n); p = lane // spp
    ipos = np.stack([(p % gw).astype(np.int64) + sensor.crop_offset_x - border, (p // gw).astype(np.int64) + sensor.crop_offset_y - border]).astype(np.float32)
    jit = np.zeros((2, n), np.float32); s2 = np.zeros(2, np.float32)
    for i in range(n):
        O.lib().orc_sampler_stream(seed, i, 2, O.fp(s2)); jit[:, i] = s2
    return ipos, (ipos + jit).astype(np.float32)


def oracle_aov_film(O, scene, osc, sensor, rfilter, types, seed, spp):
    """the expected raw AOV film H x W x (C + 1) and the per-lane data it was built from"""
    ipos, pos = lane_positions(O, sensor, rfilter, seed, spp)
    n = pos.shape[1]
    sx = np.float32(1.0) / np.float32(sensor.crop_width); sy = np.float32(1.0) / np.float32(sensor.crop_height)
    px = (pos[0].astype(np.float64) * sx - np.float64(np.float32(sensor.crop_offset_x) * sx)).astype(np.float32)
    py = (pos[1].astype(np.float64) * sy - np.float64(np.float32(sensor.crop_offset_y) * sy)).astype(np.float32)
    o = np.zeros((3, n), np.float32); d = np.zeros((3, n), np.float32); mt = np.zeros(n, np.float32)
    O.lib().orc_sensor_sample_ray(C.byref(sensor), n, O.fp(px), O.fp(py), O.fp(o), O.fp(d), O.fp(mt))
    vals, hit, _ = oracle_aovs(O, scene, osc, types, o, d, mt)
    count = vals.shape[0]
    H, W = sensor.crop_height, sensor.crop_width
    film = np.zeros((H, W, count + 1), np.float32)
    put = ipos if rfilter == "box" else pos           # a box filter puts at the pixel, the others at the sample position (SamplingIntegrator::render_sample)
    fx = np.ascontiguousarray(put[0]); fy = np.ascontiguousarray(put[1])
    for c0 in range(0, count, 3):                     # three channels at a time through the {R, G, B, W} put
        v4 = np.zeros((n, 4), np.float32); k = min(3, count - c0)
        v4[:, :k] = vals[c0:c0 + k].T.astype(np.float32); v4[:, 3] = 1.0
        tmp = np.zeros((H, W, 4), np.float32)
        O.lib().orc_film_put(C.byref(sensor), n, O.fp(fx), O.fp(fy), O.fp(v4), O.fp(tmp))
        film[:, :, c0:c0 + k] = tmp[:, :, :k]; film[:, :, count] = tmp[:, :, 3]
    return film, dict(ipos=ipos, pos=pos, vals=vals, hit=hit, o=o, d=d)


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
