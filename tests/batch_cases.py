"""Shared inputs and the oracle-side composition of the `batch` sensor tests (tests/test_batch_sensor_cpu.py, tests/test_gpu_batch_sensor.py).

A batch render is a composition of oracle entries that exist for other reasons: orc_sample_tea_32 + orc_pcg32_seed + orc_pcg32_next_float32 give a lane's pixel jitter
and the sampler state after it, BatchSensor::sample_ray's four lines (batch.cpp:138-145) restated in NumPy float32 pick the child and the position on its film,
orc_sensor_sample_ray on that child's record gives the ray, OracleScene.integrator_sample(state = ...) the radiance and orc_film_put on the wide film the splat."""
import ctypes as C

import numpy as np


def batch_select(px, n):
    """batch.cpp:138-145 in float32: (index, position on the child's film)"""
    px = np.asarray(px, np.float32)
    idx_f = (px * np.float32(n)).astype(np.float32)              # one rounded product
    idx_u = idx_f.astype(np.uint32)
    index = np.minimum(idx_u, np.uint32(n - 1))
    px2 = (idx_f - idx_u.astype(np.float32)).astype(np.float32)  # one rounded difference
    return index, px2


def child_dicts(mi, kinds):
    """child sensors around the Cornell box; `kinds`: 'p' perspective, 'o' orthographic.  Every one sees the inside of the box with almost every ray."""
    T = mi.ScalarTransform4f
    views = [([0.0, 0.0, 3.9], [0.0, 0.0, 0.0], 39.3077), ([0.6, 0.3, 3.2], [-0.2, -0.2, 0.0], 45.0), ([-0.7, -0.2, 3.0], [0.2, 0.0, -0.5], 50.0), ([0.1, 0.5, 2.6], [0.0, -0.4, 0.0], 60.0)]
    out = []
    for i, k in enumerate(kinds):
        o, t, fov = views[i % len(views)]
        film = {"type": "hdrfilm", "width": 24, "height": 24}
        if k == "o":          # the scale of an orthographic camera's to_world sets the size of its view (orthographic.cpp:104-121)
            out.append({"type": "orthographic", "near_clip": 0.01, "far_clip": 100.0, "to_world": T().look_at(origin=o, target=t, up=[0, 1, 0]).scale([0.9, 0.9, 1.0]), "film": film})
        else:
            out.append({"type": "perspective", "fov": fov, "near_clip": 0.01, "far_clip": 100.0, "to_world": T().look_at(origin=o, target=t, up=[0, 1, 0]), "film": film})
    return out


def batch_dict(mi, kinds, width, height, rfilter="gaussian", spp=4, names=None):
    d = {"type": "batch", "sampler": {"type": "independent", "sample_count": spp},
         "film": {"type": "hdrfilm", "width": width, "height": height, "rfilter": {"type": rfilter}, "pixel_format": "rgb"}}
    for i, c in enumerate(child_dicts(mi, kinds)):
        d[names[i] if names else "cam%d" % i] = c
    return d


def batch_scene(mi, kinds="pp", width=96, height=32, rfilter="gaussian", spp=4, integrator=None, textured=False):
    d = mi.textured_cornell_box(res=32, tex_res=16, spp=spp) if textured else mi.cornell_box()
    d["integrator"] = integrator or {"type": "path", "max_depth": 4}
    d["sensor"] = batch_dict(mi, kinds, width, height, rfilter, spp)
    return d


def oracle_sensor(O, har):
    s = O.Sensor()
    C.memmove(C.byref(s), C.byref(har), C.sizeof(s))
    return s


def lane_streams(O, seed, n):
    """(jitter 2 x n, sampler state after the two draws) of lanes 0..n-1: Sampler::seed (sampler.cpp:129-148) from the oracle's tea / pcg32 entries"""
    L = O.lib()
    jit = np.zeros((2, n), np.float32); state = np.zeros(n, np.uint64)
    v = (C.c_uint32 * 2)(); si = (C.c_uint64 * 2)()
    for i in range(n):
        L.orc_sample_tea_32(seed, i, 4, v)
        L.orc_pcg32_seed(v[0], v[1], si)
        jit[0, i] = L.orc_pcg32_next_float32(si); jit[1, i] = L.orc_pcg32_next_float32(si)
        state[i] = si[0]
    return jit, state


def oracle_batch_rays(O, children, px, py):
    """BatchSensor::sample_ray composed from batch_select + orc_sensor_sample_ray per child: (o 3 x n, d 3 x n, maxt n, child index n)"""
    px = np.ascontiguousarray(px, np.float32); py = np.ascontiguousarray(py, np.float32); n = px.shape[0]
    index, px2 = batch_select(px, len(children))
    o = np.zeros((3, n), np.float32); d = np.zeros((3, n), np.float32); mt = np.zeros(n, np.float32)
    for k, child in enumerate(children):
        ids = np.nonzero(index == k)[0]
        if ids.size == 0:
            continue
        qx = np.ascontiguousarray(px2[ids]); qy = np.ascontiguousarray(py[ids]); m = ids.size
        oo = np.zeros((3, m), np.float32); dd = np.zeros((3, m), np.float32); tt = np.zeros(m, np.float32)
        O.lib().orc_sensor_sample_ray(C.byref(child), m, O.fp(qx), O.fp(qy), O.fp(oo), O.fp(dd), O.fp(tt))
        o[:, ids] = oo; d[:, ids] = dd; mt[ids] = tt
    return o, d, mt, index


def oracle_batch_lanes(O, batch, seed, spp, jitter=None):
    """per-lane data of a batch render at `seed` / `spp` (lane = pixel * spp + sample over the wide film, integrator.cpp:322-345): film positions, rays, child index,
    sampler state after the jitter.  `jitter` (2 x n): given jitters instead of the streams' first two numbers (later passes of a multi-pass render)."""
    wide = oracle_sensor(O, batch.har)
    children = [oracle_sensor(O, c.har) for c in batch.sensors()]
    W, H = wide.crop_width, wide.crop_height
    n = W * H * spp
    jit, state = lane_streams(O, seed, n)
    if jitter is not None:
        jit = jitter
    p = np.arange(n) // spp
    ipos = np.stack([(p % W), (p // W)]).astype(np.float32)
    pos = (ipos + jit).astype(np.float32)
    sx = np.float32(1.0) / np.float32(W); sy = np.float32(1.0) / np.float32(H)
    px = (pos[0].astype(np.float64) * sx - np.float64(np.float32(0.0) * sx)).astype(np.float32)      # fma(pos, 1 / size, -offset / size), offset 0
    py = (pos[1].astype(np.float64) * sy - np.float64(np.float32(0.0) * sy)).astype(np.float32)
    o, d, mt, index = oracle_batch_rays(O, children, px, py)
    return dict(wide=wide, children=children, n=n, ipos=ipos, pos=pos, px=px, py=py, o=o, d=d, maxt=mt, index=index, state=state)


def film_put(O, wide, rfilter, lanes, rgb):
    """orc_film_put of per-lane rgb (3 x n) with weight 1 on the wide film: H x W x 4"""
    n = lanes["n"]
    put = lanes["ipos"] if rfilter == "box" else lanes["pos"]       # a box filter puts at the pixel, the others at the sample position (SamplingIntegrator::render_sample)
    fx = np.ascontiguousarray(put[0]); fy = np.ascontiguousarray(put[1])
    v4 = np.ones((n, 4), np.float32); v4[:, :3] = np.asarray(rgb, np.float32).T
    film = np.zeros((wide.crop_height, wide.crop_width, 4), np.float32)
    O.lib().orc_film_put(C.byref(wide), n, O.fp(fx), O.fp(fy), O.fp(v4), O.fp(film))
    return film


def oracle_batch_film(O, osc, batch, rfilter, seed, spp, max_depth, rr_depth=5, prb=False):
    """the expected raw film H x W x 4 of a batch render and the per-lane data (with `hit`: the camera ray met geometry)"""
    lanes = oracle_batch_lanes(O, batch, seed, spp)
    rgb, valid, _ = osc.integrator_sample(lanes["o"], lanes["d"], lanes["maxt"], seed=seed, lane_offset=0, state=lanes["state"], max_depth=max_depth, rr_depth=rr_depth, prb=prb)
    t = osc.ray_intersect(lanes["o"], lanes["d"], lanes["maxt"])[0]
    lanes["hit"] = np.isfinite(t); lanes["rgb"] = rgb
    return film_put(O, lanes["wide"], rfilter, lanes, rgb), lanes


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
