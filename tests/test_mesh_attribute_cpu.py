"""Mesh attributes and the `mesh_attribute` texture on the CPU: the attribute table of a mesh, the PLY and serialized readers, XML against dict, mi.traverse, every
refusal, and the host render (har_render_lanes_stats_host runs the HAR_HD code the kernels run) of the product's indexed mesh against the oracle's render of the twin
scene of tests/attribute_cases.py -- which also shows that the oracle alone renders the twin scenes."""
import os
import struct
import warnings

import numpy as np
import pytest

from tests import attribute_cases as A
from tests import blend_cases as B
from tests.test_cpu_host import rel_l2

RES, SPP = (16, 12), 4


# ------------------------------------------------------------------------------------------------ 1. the attribute table of a mesh

def _tri_mesh(mi):
    P, F = A.grid_mesh(2, 1)
    return mi.core.Mesh("m").from_fields(F, P), P, F


def test_add_attribute_and_its_errors(mi):
    m, P, F = _tri_mesh(mi)
    m.add_attribute("vertex_color", np.ones((len(P), 3), np.float32)); m.add_attribute("face_id", np.arange(len(F), dtype=np.float32).reshape(-1, 1))
    assert m.has_attribute("vertex_color") and m.has_attribute("face_id") and not m.has_attribute("vertex_x")
    assert m.attribute("face_id").shape == (len(F), 1) and m.attribute("face_id").dtype == np.float32
    with pytest.raises(RuntimeError, match=r'add_attribute\(\): attribute "vertex_color" already exists\.'):
        m.add_attribute("vertex_color", np.ones((len(P), 3)))
    with pytest.raises(RuntimeError, match=r'attribute name must start with either "vertex_" or "face_"\.'):
        m.add_attribute("color", np.ones((len(P), 3)))
    with pytest.raises(RuntimeError, match=r'attribute "vertex_a": expected a \(%d, dim\) tensor with one row per vertex\.' % len(P)):
        m.add_attribute("vertex_a", np.ones((len(P) + 1, 3)))
    with pytest.raises(RuntimeError, match=r'attribute "face_a": expected a \(%d, dim\) tensor with one row per face\.' % len(F)):
        m.add_attribute("face_a", np.ones(len(F)))
    with pytest.raises(RuntimeError, match=r'attribute "vertex_b": 1 to 4 channels are supported, got 5\.'):
        m.add_attribute("vertex_b", np.ones((len(P), 5)))
    with pytest.raises(RuntimeError, match=r'attribute "vertex_c": 1 to 4 channels are supported, got 0\.'):
        m.add_attribute("vertex_c", np.ones((len(P), 0)))
    with pytest.raises(RuntimeError, match=r'attribute\(\): attribute "vertex_q" doesn\'t exist\.'):
        m.attribute("vertex_q")
    m.remove_attribute("face_id")
    assert not m.has_attribute("face_id")
    before = m.attribute("vertex_color").copy()
    m.transform(mi.ScalarTransform4f().translate([1, 2, 3]).scale([2, -1, 1]))          # to_world leaves attributes alone
    assert np.array_equal(m.attribute("vertex_color"), before)


# ------------------------------------------------------------------------------------------------ 2. loaders

VERTEX_PROPS = [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"), ("uchar", "green"), ("uchar", "blue"), ("float", "foo_x"), ("float", "foo_y"), ("float", "foo_z"),
                ("float", "bar_r"), ("float", "bar_g"), ("float", "bar_b"), ("float", "quality_0"), ("float", "pair_x"), ("float", "pair_y")]
FACE_PROPS = [("float", "r"), ("float", "g"), ("float", "b"), ("float", "a"), ("short", "mat_0")]
FMT = {"float": "f", "uchar": "B", "short": "h"}


def _write_ply(path, binary, P, F, vcols, fcols):
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "element vertex %d" % len(P)]
    head += ["property %s %s" % p for p in VERTEX_PROPS]
    head += ["element face %d" % len(F), "property list uchar int vertex_indices"] + ["property %s %s" % p for p in FACE_PROPS] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        for i in range(len(P)):
            row = list(P[i]) + list(vcols[i])
            if binary:
                f.write(struct.pack("<" + "".join(FMT[t] for t, _ in VERTEX_PROPS), *[int(v) if FMT[t] != "f" else float(v) for (t, _), v in zip(VERTEX_PROPS, row)]))
            else:
                f.write((" ".join(str(int(v)) if FMT[t] != "f" else repr(float(np.float32(v))) for (t, _), v in zip(VERTEX_PROPS, row)) + "\n").encode())
        for i in range(len(F)):
            if binary:
                f.write(struct.pack("<Biii", 3, *[int(v) for v in F[i]]) + struct.pack("<" + "".join(FMT[t] for t, _ in FACE_PROPS), *[int(v) if FMT[t] != "f" else float(v) for (t, _), v in zip(FACE_PROPS, fcols[i])]))
            else:
                f.write(("3 %d %d %d " % tuple(F[i]) + " ".join(str(int(v)) if FMT[t] != "f" else repr(float(np.float32(v))) for (t, _), v in zip(FACE_PROPS, fcols[i])) + "\n").encode())


@pytest.mark.parametrize("binary", [False, True])
def test_ply_attributes(mi, tmp_path, binary):
    """`red green blue` (uchar: the values 0 .. 255 are kept), `foo_x foo_y foo_z`, `bar_r bar_g bar_b` -> vertex_bar_color, a single `quality_0`, a two-field run (dropped),
    and on the faces `r g b a` next to vertex_indices and an integer `mat_0`; ASCII and binary little-endian, written here"""
    P, F = A.grid_mesh(3, 2); rng = np.random.default_rng(3)
    vcols = np.concatenate([rng.integers(0, 256, (len(P), 3)).astype(np.float32), rng.uniform(-1, 1, (len(P), 9)).astype(np.float32)], 1)
    fcols = np.concatenate([rng.uniform(0, 1, (len(F), 4)).astype(np.float32), rng.integers(-5, 5, (len(F), 1)).astype(np.float32)], 1)
    path = os.path.join(tmp_path, "a.ply"); _write_ply(path, binary, P, F, vcols, fcols)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m = mi.core.Mesh("p").from_ply(path, face_normals=True)
    assert sorted(m.attributes) == ["face_color", "face_mat", "vertex_bar_color", "vertex_color", "vertex_foo", "vertex_quality"]
    assert np.array_equal(m.V[:, :3], P) and np.array_equal(m.F[:, :3], F)
    assert np.array_equal(m.attribute("vertex_color"), vcols[:, 0:3]) and m.attribute("vertex_color").max() > 1          # uchar colours are not rescaled
    assert np.array_equal(m.attribute("vertex_foo"), vcols[:, 3:6]) and np.array_equal(m.attribute("vertex_bar_color"), vcols[:, 6:9])
    assert np.array_equal(m.attribute("vertex_quality"), vcols[:, 9:10])
    assert np.array_equal(m.attribute("face_color"), fcols[:, 0:4]) and np.array_equal(m.attribute("face_mat"), fcols[:, 4:5])
    text = " ".join(str(x.message) for x in w)
    assert "vertex_pair" in text and "1 or 3 fields" in text and "integer fields" in text
    # a flipped winding permutes a face's indices, not the faces: face rows follow the face order the loader produces
    m2 = mi.core.Mesh("p").from_ply(path, face_normals=True, flip_normals=True)
    assert np.array_equal(m2.F[:, :3], F[:, ::-1]) and np.array_equal(m2.attribute("face_color"), fcols[:, 0:4]) and np.array_equal(m2.attribute("vertex_foo"), vcols[:, 3:6])


def test_serialized_v5_attributes(mi, tmp_path):
    from tests.test_mesh_formats_cpu import serialized_v5_blob, write_serialized
    P, F = A.grid_mesh(3, 2); rng = np.random.default_rng(5)
    V = np.zeros((len(P), 8), np.float32); V[:, :3] = P
    F4 = np.zeros((len(F), 4), np.uint32); F4[:, :3] = F
    col = rng.uniform(0, 1, (len(P), 3)).astype(np.float32); fid = np.arange(len(F), dtype=np.float32).reshape(-1, 1); w4 = rng.uniform(0, 1, (len(F), 4)).astype(np.float32)
    path = os.path.join(tmp_path, "v5.serialized")
    write_serialized(path, 4, [serialized_v5_blob(V, F4, 0, attrs=[("vertex_color", 3, col), ("face_id", 1, fid), ("face_w", 4, w4)]), serialized_v5_blob(V, F4, 0)])
    m = mi.core.Mesh("s").from_serialized(path, to_world=mi.ScalarTransform4f().translate([0, 1, 0]))
    assert sorted(m.attributes) == ["face_id", "face_w", "vertex_color"]
    assert np.array_equal(m.attribute("vertex_color"), col) and np.array_equal(m.attribute("face_id"), fid) and np.array_equal(m.attribute("face_w"), w4)
    assert mi.core.Mesh("s").from_serialized(path, shape_index=1).attributes == {}


# ------------------------------------------------------------------------------------------------ 3. the plugin: dict, XML, traverse, update

def _ply_scene_file(tmp_path, P, F, col):
    path = os.path.join(tmp_path, "m.ply")
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty float r\nproperty float g\nproperty float b\n" % len(P))
        f.write("element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(F))
        for p, c in zip(P, col):
            f.write(" ".join(repr(float(v)) for v in list(p) + list(c)) + "\n")
        for t in F:
            f.write("3 %d %d %d\n" % tuple(t))
    return path


def test_xml_equals_dict_and_traverse(mi, tmp_path):
    P, F = A.grid_mesh(3, 2); col = A.vertex_colors(len(P))
    path = _ply_scene_file(tmp_path, P, F, col)
    d = A.base_scene(mi, RES, SPP)
    d["M"] = {"type": "ply", "filename": path, "face_normals": True, "bsdf": {"type": "diffuse", "reflectance": {"type": "mesh_attribute", "name": "vertex_color", "scale": 0.75}}}
    a = mi.load_dict(d)
    xml = """<scene version="3.0.0">
      <shape type="ply" id="M"><string name="filename" value="%s"/><boolean name="face_normals" value="true"/>
        <bsdf type="diffuse"><texture type="mesh_attribute" name="reflectance"><string name="name" value="vertex_color"/><float name="scale" value="0.75"/></texture></bsdf>
      </shape></scene>""" % path
    b = mi.load_string(xml)
    ma, mb = a.meshes[-1], b.meshes[-1]
    assert np.array_equal(ma["attributes"]["vertex_color"], col) and np.array_equal(mb["attributes"]["vertex_color"], col)
    ta, tb = a.textures[a.bsdf_objs[ma["bsdf"]].tex_index], b.textures[b.bsdf_objs[mb["bsdf"]].tex_index]
    assert np.array_equal(ta, tb) and ta.shape == (len(P), 1, 3) and a.bsdf_objs[ma["bsdf"]].attr == b.bsdf_objs[mb["bsdf"]].attr == ("vertex_color", 0.75)
    params = mi.traverse(a)
    assert tuple(params["M.vertex_color"].shape) == (len(P), 3) and params.flags("M.vertex_color") == mi.ParamFlags.Differentiable
    assert float(params["M.bsdf.reflectance.scale"][0]) == 0.75 and params.flags("M.bsdf.reflectance.scale") == mi.ParamFlags.NonDifferentiable
    assert "M.bsdf.reflectance.data" not in params and "M.bsdf.reflectance.to_uv" not in params
    with pytest.raises(RuntimeError, match="Unreferenced property \"filter_type\""):
        mi.load_dict({"type": "diffuse", "reflectance": {"type": "mesh_attribute", "name": "vertex_color", "filter_type": "nearest"}})
    with pytest.raises(RuntimeError, match=r'Invalid mesh attribute name: must be start with either "vertex_" or "face_" but was "color"\.'):
        mi.load_dict({"type": "diffuse", "reflectance": {"type": "mesh_attribute", "name": "color"}})


def test_update_equals_fresh_load(mi):
    """after params.update() the scene equals one freshly loaded with those values: the host render of both, bit for bit; a write of another shape is a RuntimeError"""
    import torch
    P, F = A.grid_mesh(3, 2); col = A.vertex_colors(len(P)); new = A.vertex_colors(len(P), seed=77)
    mk = lambda values, scale=None: mi.load_dict(dict(A.base_scene(mi, RES, SPP), M=A.product_shape(P, F, "vertex_color", values, scale), N=A.product_shape(P - np.float32(0.25), F, "vertex_other", col)))
    a = mk(col); params = mi.traverse(a)
    assert "N.vertex_other" in params and "N.vertex_color" not in params
    params["M.vertex_color"] = torch.tensor(new); params["M.bsdf.reflectance.scale"] = torch.tensor([0.5]); params.update()
    b = mk(new, 0.5)
    fa, _ = B.host_render_stats(mi, a, 3, SPP, 6, 7); fb, _ = B.host_render_stats(mi, b, 3, SPP, 6, 7)
    assert np.array_equal(fa, fb) and np.array_equal(a.meshes[-2]["attributes"]["vertex_color"], new)
    fc, _ = B.host_render_stats(mi, mk(col), 3, SPP, 6, 7)
    assert not np.array_equal(fa, fc)
    with pytest.raises(RuntimeError, match="M.vertex_color"):
        params["M.vertex_color"] = torch.zeros(len(P), 1); params.update()


def test_refusals_name_the_shape_and_the_attribute(mi):
    P, F = A.grid_mesh(2, 2); col = A.vertex_colors(len(P))
    base = lambda: A.base_scene(mi, RES, SPP)
    d = base(); d["M"] = A.product_shape(P, F, "vertex_color", col); d["M"]["bsdf"] = A.attr_bsdf("vertex_tint")
    with pytest.raises(RuntimeError, match=r'shape "M" has no attribute "vertex_tint"'):
        mi.load_dict(d)
    d = base(); d["shared"] = A.attr_bsdf("vertex_color")
    for k in ("M", "N"):
        d[k] = {"type": "mesh", "faces": F, "positions": P + np.float32(0.1 * (k == "N")), "attributes": {"vertex_color": col}, "bsdf": {"type": "ref", "id": "shared"}}
    with pytest.raises(RuntimeError, match=r'mesh_attribute: BSDF "shared" reads the attribute "vertex_color".*"M" and "N"'):
        mi.load_dict(d)
    d = base(); d["g"] = {"type": "shapegroup", "M": A.product_shape(P, F, "vertex_color", col)}; d["i"] = {"type": "instance", "g": {"type": "ref", "id": "g"}}
    with pytest.raises(RuntimeError, match=r'mesh_attribute: shape "g.M" lies inside a shapegroup.*"vertex_color"'):
        mi.load_dict(d)
    d = base(); d["light"]["emitter"]["radiance"] = {"type": "mesh_attribute", "name": "vertex_color"}
    with pytest.raises(RuntimeError, match="mesh_attribute"):
        mi.load_dict(d)
    with pytest.raises(RuntimeError, match="mesh_attribute"):
        mi.load_dict({"type": "spot", "texture": {"type": "mesh_attribute", "name": "vertex_color"}})


def test_record_validation(mi):
    """har_scene_create's checks of a HAR_TEX_MESH_ATTRIBUTE record through the host lowering: the row count against the mesh, and a record read from another mesh"""
    import ctypes as C
    P, F = A.grid_mesh(2, 2); col = A.vertex_colors(len(P))
    scene = mi.load_dict(dict(A.base_scene(mi, RES, SPP), M=A.product_shape(P, F, "vertex_color", col)))
    film = np.zeros((RES[1], RES[0], 4), np.float32); sensor = scene.sensors()[0]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    d = scene.desc(); i = scene.bsdf_objs[scene.meshes[-1]["bsdf"]].tex_index
    assert d.textures[i].mode == 8 and d.textures[i].reserved == len(scene.meshes) - 1 and d.textures[i].height == len(P)
    d.textures[i].reserved = 0
    assert mi.lib().har_render_lanes_host(C.byref(d), C.byref(sensor.har), None, 0, 1, 1, 2, 5, fp(film)) != 0 and b"mesh_attribute" in mi.lib().har_last_error()
    d = scene.desc(); d.textures[i].height = len(P) - 1
    assert mi.lib().har_render_lanes_host(C.byref(d), C.byref(sensor.har), None, 0, 1, 1, 2, 5, fp(film)) != 0 and b"rows" in mi.lib().har_last_error()
    d = scene.desc(); d.meshes[0].bsdf = scene.meshes[-1]["bsdf"]
    assert mi.lib().har_render_lanes_host(C.byref(d), C.byref(sensor.har), None, 0, 1, 1, 2, 5, fp(film)) != 0 and b"is carried by mesh 0" in mi.lib().har_last_error()
    # an emitter cannot read such a record: as the radiance of an area light (type 7) and as an environment map (type 2)
    d = scene.desc(); d.emitters[0].type = 7; d.emitters[0].radiance_texture = i
    assert mi.lib().har_render_lanes_host(C.byref(d), C.byref(sensor.har), None, 0, 1, 1, 2, 5, fp(film)) != 0 and b"mesh_attribute: an emitter cannot read a mesh attribute" in mi.lib().har_last_error()
    d = scene.desc(); d.emitters[0].type = 2; d.emitters[0].mesh = i
    assert mi.lib().har_render_lanes_host(C.byref(d), C.byref(sensor.har), None, 0, 1, 1, 2, 5, fp(film)) != 0 and b"mesh_attribute: an emitter cannot read a mesh attribute" in mi.lib().har_last_error()
    d = scene.desc()
    assert mi.lib().har_render_lanes_host(C.byref(d), C.byref(sensor.har), None, 0, 1, 1, 2, 5, fp(film)) == 0


def test_a_bsdf_object_in_a_second_scene_is_bound_again(mi):
    """the binding of a `mesh_attribute` belongs to the scene: the same BSDF object placed in a second scene is bound to that scene's shape, not refused as shared"""
    P, F = A.grid_mesh(2, 2); col = A.vertex_colors(len(P))
    bsdf = mi.load_dict(A.attr_bsdf("vertex_color"))
    for k in range(2):
        m = mi.core.Mesh("m").from_fields(F, P); m.add_attribute("vertex_color", col * np.float32(1.0 - 0.5 * k)); m.bsdf = bsdf
        sc = mi.core.Scene({"other": mi.core.Mesh("o").from_fields(F, P + np.float32(1.0)), "M": m} if k else {"M": m})
        assert bsdf.scene is sc and bsdf.attr_mesh == k and len(sc.textures) == 1 and np.array_equal(sc.textures[bsdf.tex_index][:, 0, :], sc.meshes[k]["attributes"]["vertex_color"])


# ------------------------------------------------------------------------------------------------ 3b. the lookup and its transpose on the host

def _host_lookup(mi, scene, tex, prim, p, g=None, rows=0):
    import ctypes as C
    n = len(prim); fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    prim = np.ascontiguousarray(prim, np.uint32); p = np.ascontiguousarray(p.T, np.float32)
    value = np.zeros((3, n), np.float32); grad = np.zeros((rows, 3), np.float32) if g is not None else None
    gg = np.ascontiguousarray(g.T, np.float32) if g is not None else None
    d = scene.desc()
    rc = mi.lib().har_attribute_lookup_host(C.byref(d), tex, n, prim.ctypes.data_as(C.c_void_p), fp(p), fp(value), fp(gg) if g is not None else None, fp(grad) if g is not None else None)
    assert rc == 0, mi.lib().har_last_error()
    return value.T, grad


@pytest.mark.parametrize("kind", ["vertex", "vertex_scaled", "face"])
def test_host_deposit_against_the_twins_texel_gradients(mi, kind):
    """The transpose of the lookup on the host (har_attribute_lookup_host runs attr_addr / attr_taps / tap_weights, the lines of the in-place commit): random hits with random
    adjoints g.  (1) it is the transpose: <deposit, attr> == sum g . value, 1e-5 (float32 sums of ~20 000 terms).  (2) against the twin: the same samples scattered into the
    twin bitmap's texels through the transposed bilinear / nearest lookup at the island uv of the hit (NumPy float64), carried to the vertices by
    vertex_gradient_from_texels -- the map the device test applies to the oracle's texel gradients -- equal the deposit at 1e-3 (the project's gradient bar)"""
    P, F = A.grid_mesh(16, 16, jitter=0.3); rng = np.random.default_rng(9); scale = 0.5 if kind == "vertex_scaled" else None
    name = "face_color" if kind == "face" else "vertex_color"; nrows = len(F) if kind == "face" else len(P)
    col = A.vertex_colors(nrows, lo=0.05, hi=0.95)
    scene = mi.load_dict(dict(A.base_scene(mi, RES, SPP), M=A.product_shape(P, F, name, col, scale)))
    tex = scene.bsdf_objs[scene.meshes[-1]["bsdf"]].tex_index
    n = 20000; prim = rng.integers(0, len(F), n); b = rng.dirichlet([1, 1, 1], n)
    p = (P[F[prim, 0]].astype(np.float64) * b[:, 0:1] + P[F[prim, 1]] * b[:, 1:2] + P[F[prim, 2]] * b[:, 2:3]).astype(np.float32)
    g = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    value, dep = _host_lookup(mi, scene, tex, prim, p, g, nrows)
    s = float(scale or 1.0)
    lhs = float((dep.astype(np.float64) * col).sum()); rhs = float((g.astype(np.float64) * value).sum())
    assert abs(rhs) > 0 and abs(lhs - rhs) <= 1e-5 * np.abs(g.astype(np.float64) * value).sum()
    bb = A.barycentric_reference(P, F, prim, p)             # float64 barycentrics of the float32 hit point
    cols, _ = A.cell_layout(len(F))
    if kind == "face":
        G = np.zeros((A.cell_layout(len(F))[1], cols, 3)); np.add.at(G, (prim // cols, prim % cols), g.astype(np.float64))
        want = A.face_gradient_from_texels(len(F), G) * s
    else:
        x = 0.1 + 0.8 * bb[:, 1]; y = 0.1 + 0.8 * bb[:, 2]; r, c = prim // cols, prim % cols
        G = np.zeros((2 * A.cell_layout(len(F))[1], 2 * cols, 3))
        for dy, dx, w in ((0, 0, (1 - x) * (1 - y)), (0, 1, x * (1 - y)), (1, 0, (1 - x) * y), (1, 1, x * y)):
            np.add.at(G, (2 * r + dy, 2 * c + dx), g.astype(np.float64) * w[:, None])
        want = A.vertex_gradient_from_texels(F, len(P), G) * s
    e = rel_l2(dep, want)
    print("host deposit against the twin's texel gradients, %s: %.3g" % (kind, e))
    assert np.abs(want).max() > 0 and e <= 1e-3


# ------------------------------------------------------------------------------------------------ 4. host renders against the oracle's twin

def _cases():
    P, F = A.grid_mesh(1, 1); yield "quad", [("M", P, F, "vertex_color", A.vertex_colors(4), {})], True
    P, F = A.grid_mesh(16, 16, jitter=0.3); yield "grid16", [("M", P, F, "vertex_color", A.vertex_colors(len(P)), {})], False
    P, F = A.grid_mesh(4, 3); yield "twosided_scaled", [("M", P, F, "vertex_color", A.vertex_colors(len(P)), {"twosided": True, "scale": 0.5})], False
    P, F = A.grid_mesh(4, 3); yield "mono", [("M", P, F, "vertex_gray", A.vertex_colors(len(P), dim=1), {})], False
    P, F = A.grid_mesh(6, 5); yield "face", [("M", P, F, "face_color", A.vertex_colors(len(F), seed=6), {})], False


@pytest.mark.parametrize("case", [c[0] for c in _cases()])
def test_host_render_against_oracle_twin(mi, O, case):
    """16 x 12 at 4 spp: relative L2 1e-4, path and vertex counters equal"""
    _, meshes, first = [c for c in _cases() if c[0] == case][0]
    product, twin = A.pair(mi, RES, SPP, meshes, first=first)
    scene = mi.load_dict(product); osc, osensor = O.scene_from_product(mi.load_dict(twin))
    got, gst = B.host_render_stats(mi, scene, 3, SPP, 6, 7)
    want, st = osc.render_path(osensor, seed=3, spp=SPP, max_depth=6, rr_depth=7, raw=True, threads=2)
    e = rel_l2(O.develop(got), O.develop(want))
    print("mesh_attribute host render %s: rel L2 %.3g, (paths, vertices) %s vs %s" % (case, e, (gst.paths, gst.vertices), (st.paths, st.vertices)))
    assert np.isfinite(got).all() and np.linalg.norm(want[..., :3]) > 0 and e <= 1e-4 and (gst.paths, gst.vertices) == (st.paths, st.vertices)


def test_per_ray_lookup_host_against_float64(mi):
    """the host twin of the aov albedo against Mesh::barycentric_coordinates + interpolate_attribute restated in float64 from the hit's p: 2e-5 for mixed values"""
    P, F = A.grid_mesh(16, 16, jitter=0.3); col = A.vertex_colors(len(P), lo=0.05, hi=0.95)
    scene = mi.load_dict(dict(A.base_scene(mi, RES, SPP), M=A.product_shape(P, F, "vertex_color", col)))
    n = 20480; rng = np.random.default_rng(6)
    target = np.asarray([0.0, -0.15, 0.35])[:, None] + np.asarray([0.6, 0.0, 0.12])[:, None] * rng.uniform(-1, 1, n) + np.asarray([0.0, 0.53, -0.2])[:, None] * rng.uniform(-1, 1, n)
    o = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), np.full(n, 3.5)]); d = target - o; d = d / np.linalg.norm(d, axis=0)
    aov = mi.load_dict({"type": "aov", "aovs": "ab:albedo,pp:position,pi:prim_index,si:shape_index"})
    out = aov.sample_host(scene, o.astype(np.float32), d.astype(np.float32), np.full(n, np.inf, np.float32))
    on = out[7] == float(len(scene.meshes)); assert on.sum() > 15000
    prim = out[6, on].astype(np.int64); b = A.barycentric_reference(P, F, prim, out[3:6, on].T)
    c = col.astype(np.float64)
    want = c[F[prim, 0]] * b[:, 0:1] + c[F[prim, 1]] * b[:, 1:2] + c[F[prim, 2]] * b[:, 2:3]
    got = out[0:3, on].T.astype(np.float64)
    print("per-ray lookup (host) against float64: largest absolute difference %.3g" % float(np.abs(got - want).max()))
    assert np.allclose(got, want, rtol=2e-5, atol=1e-7)
