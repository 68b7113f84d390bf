"""Scenes and rays shared by tests/test_top_seed_cpu.py and tests/test_gpu_top_seed.py: a box of top-level triangles around three rotated and scaled
instances of a 32-triangle mesh, in variants with 0, 1, 12, 16 and 17 top-level triangles (Accel::top_seed: 1 .. 16 are eligible)."""
import numpy as np

BOX = 4.0            # the box spans [-BOX, BOX]^3
INF = np.float32(np.inf)
LARGEST = np.float32(3.402823466e+38)


def grid_mesh():
    """32 triangles: a 4 x 4 grid of quads over [-1, 1]^2, bumpy inside, FLAT (z = 0) in the corner quad [-1, -0.5]^2 -- the instance triangles there are
    the ones a top-level triangle is made coplanar with"""
    xs = np.linspace(-1.0, 1.0, 5)
    P = np.array([[x, y, 0.0] for y in xs for x in xs], np.float32)
    rng = np.random.default_rng(3)
    for j in range(5):
        for i in range(5):
            if i > 1 or j > 1:
                P[5 * j + i, 2] = np.float32(rng.uniform(-0.3, 0.3))
    F = []
    for j in range(4):
        for i in range(4):
            a = 5 * j + i
            F += [[a, a + 1, a + 6], [a, a + 6, a + 5]]
    return np.array(F, np.uint32), P


def box_mesh(s=BOX):
    P = np.array([[x, y, z] for z in (-s, s) for y in (-s, s) for x in (-s, s)], np.float32)
    F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.uint32)
    return F, P


# instance 2: an exact transform (quarter turn about z, scale 2, dyadic translation) -- an axis-parallel ray with a dyadic origin then meets the flat corner of the
# mesh and the coplanar top-level triangle at bit-equal t
EXACT = np.array([[0, -2, 0, 1.0], [2, 0, 0, 0.5], [0, 0, 2, -1.5], [0, 0, 0, 1]], np.float64)
EXACT_INV = np.array([[0, 0.5, 0, -0.25], [-0.5, 0, 0, 0.5], [0, 0, 0.5, 0.75], [0, 0, 0, 1]], np.float64)
assert np.array_equal(EXACT @ EXACT_INV, np.eye(4))
FLAT_Z = -1.5        # world z of instance 2's flat corner, which spans x in [2, 3], y in [-1.5, -0.5]


def extra_triangles(k):
    """k extra top-level triangles next to the 12 of the box; the first is coplanar with instance 2's flat corner, the second has zero area"""
    T = [
        [[1.5, -2.0, FLAT_Z], [3.5, -2.0, FLAT_Z], [1.5, 0.0, FLAT_Z]],
        [[0.5, 0.5, 3.0], [1.0, 1.0, 3.0], [1.5, 1.5, 3.0]],            # degenerate: det = 0 for every ray
        [[-3.0, -3.0, -2.0], [-1.0, -3.0, -2.5], [-3.0, -1.0, -2.0]],
        [[-3.5, 3.0, 1.0], [-2.0, 3.5, 2.0], [-3.0, 2.0, 3.0]],
        [[0.0, 3.0, -3.0], [2.0, 3.5, -3.0], [1.0, 2.5, -1.0]],
    ]
    P = np.array(T[:k], np.float32).reshape(-1, 3)
    return np.arange(3 * k, dtype=np.uint32).reshape(-1, 3), P


def scene_dict(mi, n_top=12, integrator="path", res=24, top_seed=None, instances=True):
    """n_top top-level triangles: 0 (no top-level geometry), 1 (one huge floor triangle), 12 (the box), 13 .. 17 (box + extra_triangles)"""
    T = mi.ScalarTransform4f
    integ = {"type": integrator, "max_depth": 4, "rr_depth": 3}
    if top_seed is not None:
        integ["top_seed"] = bool(top_seed)
    d = {"type": "scene", "integrator": integ,
         "sensor": {"type": "perspective", "fov": 60.0, "to_world": T().look_at(origin=[0.3, 0.4, 3.8], target=[0.0, -0.2, 0.0], up=[0, 1, 0]),
                    "film": {"type": "hdrfilm", "width": res, "height": res, "rfilter": {"type": "box"}},
                    "sampler": {"type": "independent", "sample_count": 4}},
         "white": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.7, 0.7]}},
         "blue": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.2, 0.3, 0.8]}}}
    if n_top == 1:
        d["floor"] = {"type": "mesh", "faces": np.array([[0, 1, 2]], np.uint32), "positions": np.array([[-40, -BOX, 40], [40, -BOX, 40], [0, -BOX, -40]], np.float32),
                      "bsdf": {"type": "ref", "id": "white"}}
    elif n_top >= 12:
        F, P = box_mesh()
        d["box"] = {"type": "mesh", "faces": F, "positions": P, "bsdf": {"type": "ref", "id": "white"}}
        if n_top > 12:
            F, P = extra_triangles(n_top - 12)
            d["extra"] = {"type": "mesh", "faces": F, "positions": P, "bsdf": {"type": "ref", "id": "blue"}}
    elif n_top != 0:
        raise ValueError(n_top)
    F, P = grid_mesh()
    if instances:
        d["grp"] = {"type": "shapegroup", "grid": {"type": "mesh", "faces": F, "positions": P, "bsdf": {"type": "ref", "id": "blue"}}}
        d["inst0"] = {"type": "instance", "g": {"type": "ref", "id": "grp"}, "to_world": T().translate([-1.2, 0.6, 0.4]).rotate([1, 1, 0], 35).scale([1.3, 0.8, 1.0])}
        d["inst1"] = {"type": "instance", "g": {"type": "ref", "id": "grp"}, "to_world": T().translate([0.4, -1.5, -1.0]).rotate([0, 1, 1], -50).scale([1.5, 1.5, 0.6])}
        d["inst2"] = {"type": "instance", "g": {"type": "ref", "id": "grp"}, "to_world": T(np.concatenate([EXACT.ravel(), EXACT_INV.T.ravel()]))}      # {matrix, inverse transpose}
    # a point light: an area light would add top-level triangles
    d["lamp"] = {"type": "point", "position": [0.5, 2.5, 1.0], "intensity": {"type": "rgb", "value": [30.0, 28.0, 25.0]}}
    return d


def _unit(v):
    return (v / np.linalg.norm(v, axis=0)).astype(np.float32)


def rays(n_random=4500, seed=1):
    """(o[3][n], d[3][n], maxt[n]) float32: the classes of the issue, about 20 000 rays"""
    rng = np.random.default_rng(seed)
    O, D, M = [], [], []

    def add(o, d, m):
        o = np.asarray(o, np.float32).reshape(3, -1); d = np.asarray(d, np.float32).reshape(3, -1)
        O.append(o); D.append(d); M.append(np.broadcast_to(np.asarray(m, np.float32), (o.shape[1],)).copy())

    def rdir(n):
        return _unit(rng.normal(size=(3, n)))

    # random rays from inside the box
    add(rng.uniform(-3.5, 3.5, (3, n_random)), rdir(n_random), INF)
    # origins on walls, wall edges and wall vertices (coordinates exactly +-BOX), random directions and the walls' normals
    n = 800
    for fixed in (1, 2, 3):
        o = rng.uniform(-BOX, BOX, (3, n)).astype(np.float32)
        for k in range(fixed):
            ax = (rng.integers(0, 3, n) + k) % 3
            o[ax, np.arange(n)] = np.where(rng.random(n) < 0.5, -BOX, BOX)
        add(o, rdir(n), INF)
        dn = np.zeros((3, n), np.float32); ax = rng.integers(0, 3, n); dn[ax, np.arange(n)] = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        add(o, dn, INF)                                   # along +-axis: t = +-0 on the wall the origin lies in
    # the coplanar pair: straight down / up onto instance 2's flat corner and the top-level triangle in the same plane, dyadic origins
    g = np.arange(0, 64) / 32.0
    X, Y = np.meshgrid(1.5 + g, -2.0 + g)
    for z0, dz in ((1.0, -1.0), (-3.0, 1.0), (FLAT_Z, -1.0), (FLAT_Z, 1.0)):
        o = np.stack([X.ravel(), Y.ravel(), np.full(X.size, z0)]); d = np.zeros_like(o); d[2] = dz
        add(o[:, ::4], d[:, ::4], INF)
    # maxt: in front of the walls, zero, the largest float
    n = 800
    add(rng.uniform(-1.0, 1.0, (3, n)), rdir(n), 0.75)
    add(rng.uniform(-3.5, 3.5, (3, n)), rdir(n), rng.uniform(0.0, 3.0, n))
    add(rng.uniform(-3.5, 3.5, (3, n)), rdir(n), 0.0)
    add(rng.uniform(-3.5, 3.5, (3, n)), rdir(n), LARGEST)
    # rays that miss everything: from outside the box, pointing away
    o = rdir(n) * np.float32(9.0)
    add(o, _unit(o + 0.3 * rng.normal(size=(3, n))), INF)
    # towards the zero-area triangle
    tgt = np.array([[1.0], [1.0], [3.0]]) + 0.02 * rng.normal(size=(3, n)); o = rng.uniform(-2.0, 2.0, (3, n))
    add(o, _unit(tgt - o), INF)
    # |d| over 12 orders of magnitude
    n = 1500
    add(rng.uniform(-3.5, 3.5, (3, n)), rdir(n) * (10.0 ** rng.uniform(-6.0, 6.0, n)).astype(np.float32), INF)
    o = np.ascontiguousarray(np.concatenate(O, axis=1), np.float32); d = np.ascontiguousarray(np.concatenate(D, axis=1), np.float32)
    return o, d, np.ascontiguousarray(np.concatenate(M), np.float32)
