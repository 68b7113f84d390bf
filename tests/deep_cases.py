"""Scenes shared by tests/test_deep_bvh_cpu.py and tests/test_gpu_stack_spill.py: small meshes whose BVH is DEEP (HostScene::stack_need() above the 13 LDS
entries of the wavefront kernels, up to and past the 30 entries the kernels hold at all), and scenes whose rays reach stack levels >= 5, which a
library built with 3 LDS entries (-DHAR_LDS_STACK_SMALL=3) keeps in the HBM columns.  All generators are seeded; the host harness tells
(stack_need, deepest level a camera ray reached)."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LARGEST = np.float32(3.402823466e+38)
STACK_LDS = 13           # HAR_LDS_STACK_SMALL of the default library
STACK_CAP = 30           # min(HAR_LDS_STACK_DEPTH, HAR_LDS_STACK_SMALL + HAR_STACK_SPILL)
STACK3_CAP = 23          # the same bound of the 3-entry library: min(30, 3 + 20)


# ------------------------------------------------------------------ meshes

def nest(n, ratio, seed=1):
    """n concentric triangles around the origin, each `ratio` times smaller than the one before: (faces, positions)"""
    rng = np.random.default_rng(seed)
    s = ratio ** -np.arange(n)
    P = (s[:, None, None] * 0.5 * rng.normal(size=(n, 3, 3))).astype(np.float32)
    return np.arange(3 * n, dtype=np.uint32).reshape(n, 3), P.reshape(-1, 3)


def comb(clusters=110, per=40, ratio=1.2, seed=2):
    """`clusters` clusters of `per` triangles on the z axis: cluster j has size ratio^-j and sits at z = 3 ratio^-j, so a ray along the axis
    meets every cluster's bounds"""
    rng = np.random.default_rng(seed)
    P = []
    for j in range(clusters):
        s = ratio ** -j
        c = rng.normal(size=(per, 1, 3)) * [0.5, 0.5, 0.1] + [0.0, 0.0, 3.0]
        P.append(s * (c + 0.25 * rng.normal(size=(per, 3, 3))))
    P = np.concatenate(P).astype(np.float32)
    return np.arange(3 * P.shape[0], dtype=np.uint32).reshape(-1, 3), P.reshape(-1, 3)


def soup(n, seed=4):
    """n random triangles in [-1, 1]^3 whose sizes span two orders of magnitude"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3)); s = 10 ** rng.uniform(-2.0, -0.3, (n, 1, 1))
    P = (c + s * rng.normal(size=(n, 3, 3))).astype(np.float32)
    return np.arange(3 * n, dtype=np.uint32).reshape(n, 3), P.reshape(-1, 3)


# ------------------------------------------------------------------ scenes

def _frame(mi, integrator, res, spp, origin, target, fov=45.0, sky=True, max_depth=4):
    T = mi.ScalarTransform4f
    d = {"type": "scene", "integrator": {"type": integrator, "max_depth": max_depth, "rr_depth": 3},
         "sensor": {"type": "perspective", "fov": fov, "to_world": T().look_at(origin=origin, target=target, up=[0, 1, 0]),
                    "film": {"type": "hdrfilm", "width": res, "height": res, "rfilter": {"type": "box"}, "pixel_format": "rgb"},
                    "sampler": {"type": "independent", "sample_count": spp}},
         "grey": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.6, 0.5, 0.4]}}}
    if sky:
        d["sky"] = {"type": "constant", "radiance": {"type": "rgb", "value": [0.9, 1.0, 1.1]}}
    return d


def _mesh(F, P):
    return {"type": "mesh", "faces": F, "positions": P, "bsdf": {"type": "ref", "id": "grey"}}


def nest_scene(mi, n, ratio, integrator="path", res=32, spp=4):
    d = _frame(mi, integrator, res, spp, [0.3, 0.2, 2.5], [0, 0, 0])
    d["deep"] = _mesh(*nest(n, ratio))
    return d


def instanced_nest_scene(mi, n, ratio, instances, inst_ratio, integrator="path", res=32, spp=4):
    """the nest in a shapegroup, `instances` copies, copy k turned by 7k degrees about (1, 1, 0) and scaled by inst_ratio^-k"""
    T = mi.ScalarTransform4f
    d = _frame(mi, integrator, res, spp, [0.3, 0.2, 2.5], [0, 0, 0])
    d["grp"] = {"type": "shapegroup", "deep": _mesh(*nest(n, ratio))}
    for k in range(instances):
        d["inst%02d" % k] = {"type": "instance", "g": {"type": "ref", "id": "grp"}, "to_world": T().rotate([1, 1, 0], 7.0 * k).scale(inst_ratio ** -k)}
    return d


def comb_scene(mi, integrator="path", res=32, spp=4, **kw):
    """the comb seen along its axis from its FINE end: the small clusters are the near ones, so a ray that walks front to back leaves the large ones
    (one entry per level of the chain of ever larger bounds) on its stack"""
    d = _frame(mi, integrator, res, spp, [0.0002, 0.0001, -0.01], [0, 0, 3], fov=60.0)
    d["deep"] = _mesh(*comb(**kw))
    return d


def instanced_soup_scene(mi, integrator="path", res=32, spp=4, panel=False):
    """five overlapping instances of a 600-triangle soup (one mirrored, one strongly non-uniform) next to a top-level soup; panel: an area light between the
    camera and the soups (with `hide_emitters` the camera rays that meet it are continued THROUGH the soups: Integrator::skip_area_emitters)"""
    T = mi.ScalarTransform4f
    d = _frame(mi, integrator, res, spp, [0.2, 0.3, 4.0], [0, 0, 0])
    d["deep"] = _mesh(*soup(400, seed=5))
    F, P = soup(600, seed=6)
    d["grp"] = {"type": "shapegroup", "m": _mesh(F, (0.5 * P).astype(np.float32))}
    xf = [T().translate([0.3, 0.1, -0.2]).rotate([1, 1, 0], 33.0).scale([1.0, 0.3, 2.0]), T().translate([-0.2, 0.0, 0.1]).scale([-1.0, 1.0, 1.0]),
          T().translate([0.25, 0.12, -0.15]).rotate([0, 0, 1], 80.0).scale(0.7), T().scale(1.3), T().translate([0.0, -0.4, 0.0]).rotate([0, 1, 0], 170.0)]
    for k, t in enumerate(xf):
        d["inst%d" % k] = {"type": "instance", "g": {"type": "ref", "id": "grp"}, "to_world": t}
    if panel:
        d["panel"] = {"type": "rectangle", "to_world": T().translate([0.1, 0.15, 1.6]).scale([0.25, 0.25, 1.0]), "bsdf": {"type": "ref", "id": "grey"},
                      "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [3.0, 2.5, 2.0]}}}
    return d


def update_case(mi, res=32, spp=1):
    """(scene dictionary, key, new positions): 42 instances of the 600-triangle nest STRETCHED ten times along x -- its depth-first bound is exactly the 30 entries the
    kernels hold -- and the positions of the nest itself, which make the rebuilt instance level one node deeper (a vertex update refits the mesh's own tree, which
    keeps its depth): 31, refused"""
    d = instanced_nest_scene(mi, 600, 1.1, 42, 1.2, res=res, spp=spp)
    P = d["grp"]["deep"]["positions"]
    d["grp"]["deep"]["positions"] = np.ascontiguousarray(P * np.float32([10.0, 1.0, 1.0]), np.float32)
    return d, "grp.deep.positions", P


# the deep cases (default library): name -> scene dictionary; stack_need as measured with today's builder, asserted only as bands
DEEP = {
    "nest300": lambda mi, **kw: nest_scene(mi, 300, 1.1, **kw),                                  # 18
    "nest600": lambda mi, **kw: nest_scene(mi, 600, 1.1, **kw),                                  # 22
    "nest700": lambda mi, **kw: nest_scene(mi, 700, 1.08, **kw),                                 # 26
    "instanced_nest": lambda mi, **kw: instanced_nest_scene(mi, 300, 1.1, 40, 1.3, **kw),        # 25
    "comb": lambda mi, **kw: comb_scene(mi, **kw),                                               # 17
}
OVER_DEEP = lambda mi, **kw: instanced_nest_scene(mi, 600, 1.1, 60, 1.2, **kw)                   # 31: refused
# scenes for the 3-entry library: stack_need <= 23 and camera paths that reach level >= 5 (tests/test_deep_bvh_cpu.py holds both)
SPILL3 = {
    "comb": lambda mi, **kw: comb_scene(mi, **kw),
    "instanced_soup": lambda mi, **kw: instanced_soup_scene(mi, **kw),
    "instanced_soup_panel": lambda mi, **kw: instanced_soup_scene(mi, panel=True, **kw),
}


def aimed_rays(n, target, origin_radius, seed=1, spread=0.05):
    """n rays: half aimed at `target` (+- spread) from a sphere of radius origin_radius around it, half random in [-1, 1]^3 (random_rays of test_gpu_parity.py)"""
    rng = np.random.default_rng(seed)
    h = n // 2
    u = rng.normal(size=(3, h)); u /= np.linalg.norm(u, axis=0)
    o1 = np.asarray(target, np.float64).reshape(3, 1) + origin_radius * u
    d1 = -u + spread * rng.normal(size=(3, h)); d1 /= np.linalg.norm(d1, axis=0)
    o2 = rng.uniform(-1, 1, (3, n - h)); d2 = rng.normal(size=(3, n - h)); d2 /= np.linalg.norm(d2, axis=0)
    o = np.ascontiguousarray(np.concatenate([o1, o2], axis=1), np.float32); d = np.ascontiguousarray(np.concatenate([d1, d2], axis=1), np.float32)
    return o, d, np.full(n, LARGEST, np.float32)


def case_rays(name, n, seed=1):
    """the rays of a case: at the nest's centre / along the comb's axis, mixed with random ones"""
    if name.startswith("comb"):
        rng = np.random.default_rng(seed)
        h = n // 2
        z = np.where(rng.random(h) < 0.5, 8.0, -10.0 ** rng.uniform(-3.0, 0.3, h))              # from the coarse end, and from the fine end at many distances
        o1 = np.stack([0.1 * np.abs(z) * rng.normal(size=h), 0.1 * np.abs(z) * rng.normal(size=h), z])
        d1 = np.stack([0.03 * rng.normal(size=h), 0.03 * rng.normal(size=h), -np.sign(z)]); d1 /= np.linalg.norm(d1, axis=0)
        o2, d2, _ = aimed_rays(2 * (n - h), [0, 0, 0], 2.0, seed + 1)
        o = np.ascontiguousarray(np.concatenate([o1, o2[:, n - h:]], axis=1), np.float32); d = np.ascontiguousarray(np.concatenate([d1, d2[:, n - h:]], axis=1), np.float32)
        return o, d, np.full(n, LARGEST, np.float32)
    return aimed_rays(n, [0, 0, 0], 2.0, seed)


# ------------------------------------------------------------------ the host harness

def harness():
    L = C.CDLL(os.path.join(ROOT, "tests", "host_harness", "libhost_harness.so"))
    L.hh_scene_create.restype = C.c_void_p; L.hh_scene_create.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.hh_scene_destroy.argtypes = [C.c_void_p]; L.hh_set_order.argtypes = [C.c_int]; L.hh_max_sp.restype = C.c_int
    L.hh_node_layout.restype = C.c_uint32; L.hh_node_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.hh_trace_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    L.hh_trace.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 7
    return L


def harness_scene(L, scene):
    desc = scene.desc(); err = C.create_string_buffer(512)
    h = C.c_void_p(L.hh_scene_create(C.byref(desc), err, 512)); assert h, err.value
    return h


def stack_need(L, h):
    """HostScene::stack_need(): the last word of hh_node_layout"""
    k = L.hh_node_layout(h, None, 0)
    out = np.zeros(k, np.uint32); L.hh_node_layout(h, out.ctypes.data, k)
    return int(out[-1])


def stack_levels(L, scene, bounces=4):
    """(stack_need, deepest stack level reached by the rays of the scene's camera paths): hh_trace_stats(policy = 0), then hh_max_sp()"""
    h = harness_scene(L, scene)
    try:
        need = stack_need(L, h)
        sensor = scene.sensors()[0]; film = sensor.film()
        w, hgt = film.size(); spp = sensor.sampler().sample_count()
        integ = scene.integrator()
        L.hh_set_order(2)                                                    # the kernels' child order; resets the level counter
        out = np.zeros(32 * bounces, np.float64)
        rc = L.hh_trace_stats(h, C.byref(sensor.har), 0, spp, integ.max_depth, integ.rr_depth, 0, int(w) * int(hgt) * int(spp), bounces, 0, 0, out.ctypes.data)
        assert rc == 0, rc
        assert out.reshape(bounces, 32)[:, 10].sum() == 0                    # the resumable traversal agreed with the reference loop on every ray
        return need, int(L.hh_max_sp())
    finally:
        L.hh_scene_destroy(h)


def host_trace(L, h, o, d, maxt, naive):
    """hh_trace: (t, u, v, prim, shape, inst) of the product's host code -- naive = 1 brute force, 2 the kernels' resumable traversal"""
    n = o.shape[1]
    out = [np.zeros(n, np.float32) for _ in range(3)] + [np.zeros(n, np.uint32) for _ in range(3)]
    p = lambda a: a.ctypes.data
    st = L.hh_trace(h, n, p(o), p(d), p(maxt), naive, 0, *[p(a) for a in out], None)
    assert st == 0, st
    return out


def nest_with_need(L, mi, target, ratio=1.1):
    """the first nest(n, ratio) whose stack_need equals `target` (the cap tests need scenes exactly at and one past a bound), or None"""
    for n in range(100, 1200, 10):
        scene = mi.load_dict(nest_scene(mi, n, ratio, res=16))
        h = harness_scene(L, scene)
        need = stack_need(L, h); L.hh_scene_destroy(h)
        if need == target:
            return n
        if need > target + 2:
            break
    return None
