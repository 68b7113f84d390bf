"""Shared inputs and the oracle-side composition of the `thinlens` sensor tests (tests/test_thinlens_cpu.py, tests/test_gpu_thinlens.py).

A thin-lens render is a composition of oracle entries that exist for other reasons: orc_sample_tea_32 + orc_pcg32_seed + orc_pcg32_next_float32 give a lane's pixel
jitter, its aperture sample (the NEXT two numbers, integrator.cpp:464-470) and the sampler state behind the four draws; OracleScene.integrator_sample(state = ...) gives
the radiance along a ray and orc_film_put the splat.  Only ThinLensCamera::sample_ray (thinlens.cpp:219-257) is new arithmetic: restated here in NumPy float64 from the
record's matrices (`thinlens_rays64`), with the disk point from orc_square_to_uniform_disk_concentric, and held against the product's host twin; the composed film then
takes its rays from that twin."""
import ctypes as C

import numpy as np

from tests import batch_cases as B

rel_l2 = B.rel_l2


def oracle_film_record(O, har):
    """the oracle's record of a product sensor: a prefix copy; the oracle only uses its film part, so the copy is a perspective camera to it"""
    s = B.oracle_sensor(O, har)
    s.projection = 0
    return s


def thinlens_dict(mi, aperture_radius=0.1, focus_distance=3.9, fov=39.3077, origin=(0.0, 0.0, 3.9), target=(0.0, 0.0, 0.0), film=None, spp=4, **extra):
    d = {"type": "thinlens", "fov": fov, "near_clip": 0.01, "far_clip": 100.0, "aperture_radius": aperture_radius, "focus_distance": focus_distance,
         "to_world": mi.ScalarTransform4f().look_at(origin=list(origin), target=list(target), up=[0, 1, 0]),
         "film": film or {"type": "hdrfilm", "width": 24, "height": 16, "rfilter": {"type": "gaussian"}, "pixel_format": "rgb"},
         "sampler": {"type": "independent", "sample_count": spp}}
    d.update(extra)
    return d


def film_dict(width, height, rfilter="gaussian", crop=None, sample_border=False):
    f = {"type": "hdrfilm", "width": width, "height": height, "rfilter": {"type": rfilter}, "pixel_format": "rgb"}
    if crop:
        f.update(crop_offset_x=crop[0], crop_offset_y=crop[1], crop_width=crop[2], crop_height=crop[3])
    if sample_border:
        f["sample_border"] = True
    return f


def lens_scene(mi, sensor, integrator=None, textured=False, spp=4):
    d = mi.textured_cornell_box(res=32, tex_res=16, spp=spp) if textured else mi.cornell_box()
    d["integrator"] = integrator or {"type": "path", "max_depth": 4}
    d["sensor"] = sensor
    return d


def lens_batch_dict(mi, kinds, width, height, rfilter="gaussian", spp=4, aperture_radius=0.15, focus_distance=3.2):
    """a batch sensor whose children of kind 't' are thin lenses ('p': perspective), around the Cornell box"""
    d = B.batch_dict(mi, kinds.replace("t", "p"), width, height, rfilter, spp)
    for i, k in enumerate(kinds):
        if k == "t":
            c = d["cam%d" % i]
            c["type"] = "thinlens"; c["aperture_radius"] = aperture_radius; c["focus_distance"] = focus_distance
    return d


def next_draws(O, seed, n, k, state=None):
    """k numbers of every lane's stream (k x n float32) and the PCG32 state behind them: from the seed (Sampler::seed, sampler.cpp:129-148), or continued from `state`"""
    L = O.lib()
    out = np.zeros((k, n), np.float32); after = np.zeros(n, np.uint64)
    v = (C.c_uint32 * 2)(); si = (C.c_uint64 * 2)()
    for i in range(n):
        L.orc_sample_tea_32(seed, i, 4, v)
        L.orc_pcg32_seed(v[0], v[1], si)
        if state is not None:
            si[0] = int(state[i])
        for j in range(k):
            out[j, i] = L.orc_pcg32_next_float32(si)
        after[i] = si[0]
    return out, after


def lane_streams4(O, seed, n):
    """(jitter 2 x n, aperture sample 2 x n, sampler state after the FOUR draws) of lanes 0..n-1"""
    u, state = next_draws(O, seed, n, 4)
    return u[:2].copy(), u[2:].copy(), state


def disk(O, ax, ay):
    """orc_square_to_uniform_disk_concentric over arrays: 2 x n float32"""
    L = O.lib()
    L.orc_square_to_uniform_disk_concentric.restype = None
    L.orc_square_to_uniform_disk_concentric.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    out = np.zeros((2, len(ax)), np.float32)
    s = (C.c_float * 2)(); r = (C.c_float * 2)()
    for i in range(len(ax)):
        s[0] = float(ax[i]); s[1] = float(ay[i])
        L.orc_square_to_uniform_disk_concentric(s, r)
        out[0, i] = r[0]; out[1, i] = r[1]
    return out


def thinlens_rays64(O, har, px, py, ax, ay):
    """ThinLensCamera::sample_ray (thinlens.cpp:233-254) in float64 from the record's float32 matrices: (o 3 x n, d 3 x n, maxt n, focus point in world space 3 x n)"""
    M = np.asarray(list(har.sample_to_camera), np.float64).reshape(4, 4); T = np.asarray(list(har.to_world), np.float64).reshape(4, 4)
    n = len(px)
    p = M @ np.stack([np.asarray(px, np.float64), np.asarray(py, np.float64), np.zeros(n), np.ones(n)])
    near_p = p[:3] / p[3]
    lens = np.float64(har.aperture_radius) * disk(O, ax, ay).astype(np.float64)
    aperture_p = np.stack([lens[0], lens[1], np.zeros(n)])
    focus_p = near_p * (np.float64(har.focus_distance) / near_p[2])
    d = focus_p - aperture_p
    d = d / np.linalg.norm(d, axis=0)
    dw = T[:3, :3] @ d
    o = T[:3, :3] @ aperture_p + T[:3, 3:4] + dw * (np.float64(har.near_clip) / d[2])
    maxt = (np.float64(har.far_clip) - np.float64(har.near_clip)) / d[2]
    return o, dw, maxt, T[:3, :3] @ focus_p + T[:3, 3:4]


def sample_pairs(n=20000, seed=17):
    """(position 2 x n, aperture 2 x n) in [0,1)^2, with the corners of both squares, the centre and the disk's diagonals |x| == |y| among them"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, 1, (2, n)).astype(np.float32); ap = rng.uniform(0, 1, (2, n)).astype(np.float32)
    one = np.nextafter(np.float32(1), np.float32(0))
    corners = np.array([[0, 0], [0, one], [one, 0], [one, one], [0.5, 0.5], [0, 0.5], [0.5, 0], [one, 0.5], [0.5, one]], np.float32).T
    k = corners.shape[1]
    pos[:, :k] = corners; ap[:, k:2 * k] = corners            # the special positions against random apertures, and the other way round
    pos[:, 2 * k:3 * k] = corners; ap[:, 2 * k:3 * k] = corners[:, ::-1]
    t = rng.uniform(0, 1, 64).astype(np.float32)                # 2 sx - 1 == +-(2 sy - 1): sy = sx, and sy = 1 - sx
    ap[0, 3 * k:3 * k + 64] = t; ap[1, 3 * k:3 * k + 32] = t[:32]; ap[1, 3 * k + 32:3 * k + 64] = (np.float32(1) - t[32:]).astype(np.float32)
    return pos, ap


def lanes_of(mi, O, sensor, seed, spp, draws=None):
    """per-lane data of a render through `sensor` (a thin lens, or a batch sensor -- then `four` says whether a child is a thin lens) at `seed` / `spp`: lane = pixel * spp +
    sample over the sample grid (integrator.cpp:322-345).  The rays come from the product's HOST twin.  `draws` = (numbers k x n, state): given draws instead of the streams'
    first numbers (later passes of a multi-pass render)."""
    har = sensor.har
    wide = oracle_film_record(O, har)
    f = sensor.film()
    sw, sh = f.sample_grid(); border = f.border_size_
    n = sw * sh * spp
    four = sensor.needs_aperture_sample()
    if draws is None:
        u, state = next_draws(O, seed, n, 4 if four else 2)
    else:
        u, state = draws
    jit = u[:2]; ap = u[2:4] if four else None
    p = np.arange(n) // spp
    ipos = np.stack([(p % sw) + wide.crop_offset_x - border, (p // sw) + wide.crop_offset_y - border]).astype(np.float32)
    pos = (ipos + jit).astype(np.float32)
    sx = np.float32(1.0) / np.float32(wide.crop_width); sy = np.float32(1.0) / np.float32(wide.crop_height)
    ox = np.float32(-np.float32(wide.crop_offset_x) * sx); oy = np.float32(-np.float32(wide.crop_offset_y) * sy)
    px = (pos[0].astype(np.float64) * np.float64(sx) + np.float64(ox)).astype(np.float32)      # fma(pos, 1 / crop size, -crop offset / crop size)
    py = (pos[1].astype(np.float64) * np.float64(sy) + np.float64(oy)).astype(np.float32)
    o, d, mt = sensor.sample_ray_host(np.stack([px, py]), ap)
    return dict(wide=wide, n=n, ipos=ipos, pos=pos, px=px, py=py, ap=ap, o=o, d=d, maxt=mt, state=state)


def composed_film(mi, O, osc, sensor, rfilter, seed, spp, max_depth, rr_depth=5, prb=False):
    """the expected raw film H x W x 4 of a render through `sensor`, and the per-lane data (with `hit`: the camera ray met geometry)"""
    lanes = lanes_of(mi, O, sensor, seed, spp)
    rgb, _, state = osc.integrator_sample(lanes["o"], lanes["d"], lanes["maxt"], seed=seed, lane_offset=0, state=lanes["state"], max_depth=max_depth, rr_depth=rr_depth, prb=prb)
    t = osc.ray_intersect(lanes["o"], lanes["d"], lanes["maxt"])[0]
    lanes["hit"] = np.isfinite(t); lanes["rgb"] = rgb; lanes["state_out"] = state
    return B.film_put(O, lanes["wide"], rfilter, lanes, rgb), lanes


def host_raygen(mi, sensor, seed, spp, n, resume=None):
    """har_raygen_lanes_host over lanes 0..n-1: (o, d, maxt, pos 2 x n, state)"""
    o = np.empty((3, n), np.float32); d = np.empty((3, n), np.float32); mt = np.empty(n, np.float32); pos = np.empty((2, n), np.float32); st = np.empty(n, np.uint64)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ch = sensor.children_har() if sensor.kind == "batch" else None
    res = None if resume is None else np.ascontiguousarray(resume, np.uint64)
    mi.core.check(mi.lib().har_raygen_lanes_host(C.byref(sensor.har), ch, 0 if ch is None else len(ch), seed, spp, 0, n, None if res is None else res.ctypes.data_as(C.c_void_p),
                                                 fp(o), fp(d), fp(mt), fp(pos), st.ctypes.data_as(C.c_void_p)))
    return o, d, mt, pos, st


def host_render(mi, scene, sensor, seed, spp, max_depth, rr_depth=5):
    """har_render_lanes_host: the raw film H x W x 4 of the forward `path` render, computed on the host by the functions the kernels run"""
    w, h = sensor.film().crop_size()
    film = np.zeros((h, w, 4), np.float32)
    desc = scene.desc()
    ch = sensor.children_har() if sensor.kind == "batch" else None
    mi.core.check(mi.lib().har_render_lanes_host(C.byref(desc), C.byref(sensor.har), ch, 0 if ch is None else len(ch), seed, spp, max_depth, rr_depth,
                                                 film.ctypes.data_as(C.POINTER(C.c_float))))
    return film
