"""Host-side mirror of the Mitsuba 3 Python surface for the `hip_ad_rgb` variant.

Names, argument meaning and error behaviour follow the reference
(`mi.load_dict`, `mi.cornell_box`, `mi.render`, `mi.traverse`,
`Scene.ray_intersect_preliminary`, `Integrator.render/render_backward`,
`Sampler.seed/next_1d/next_2d`, `BSDF.eval/pdf/sample`); all computation is
done by the HIP kernels behind the C ABI (mitsuba3_amd/_capi.py).  PyTorch is
used for device memory, streams and torch.distributed only.
"""
import ctypes as C
import math
import os
import re
import warnings

import numpy as np

from . import _capi
from ._capi import lib, check, HarError

VARIANT = "hip_ad_rgb"
SCALAR_VARIANT = "scalar_rgb"        # BASELINE config 1: the reference's CPU plumbing path (har_render_scalar), forward `path` renders only
_variant = None


def set_variant(name):
    """mi.set_variant: `hip_ad_rgb` (the HIP hot path; needs a GPU, no fallback) or `scalar_rgb` (config 1: the scalar branch of
    SamplingIntegrator::render on the host, forward `path` only -- an explicit choice, never a fallback of the former)."""
    global _variant
    if name not in (VARIANT, SCALAR_VARIANT):
        raise ImportError("Requested an unsupported variant \"%s\". The following variants are available: %s, %s." % (name, VARIANT, SCALAR_VARIANT))
    _variant = name


def variant():
    return _variant


def variants():
    return [VARIANT, SCALAR_VARIANT]


def _render_scalar(scene, integrator, sensor, seed, spp, threads=0, block_size=0):
    """SamplingIntegrator::render, non-JIT branch (integrator.cpp:190-274) through har_render_scalar: developed image as a numpy array"""
    if integrator.type == 'aov':
        raise RuntimeError("scalar_rgb: the `aov` integrator is not implemented by the scalar_rgb variant (hip_ad_rgb only)")
    if integrator.type != 'path':
        raise RuntimeError("scalar_rgb: only the `path` integrator is part of the config-1 plumbing path")
    _refuse_batch(sensor, "scalar_rgb (har_render_scalar)")
    if getattr(sensor, 'kind', None) == 'thinlens':
        raise RuntimeError("scalar_rgb: the `thinlens` sensor is not implemented by the scalar_rgb variant (hip_ad_rgb only)")
    if integrator.hide_emitters or sensor.film().alpha or integrator.samples_per_pass is not None:
        raise RuntimeError("scalar_rgb: hide_emitters, rgba films and samples_per_pass are not part of the config-1 plumbing path")
    if spp:
        sensor.sampler().set_sample_count(spp)
    spp = sensor.sampler().sample_count()
    w, h = sensor.film().crop_size()
    film = np.zeros((h, w, 4), np.float32)
    d = scene.desc()
    used = C.c_uint32(0)
    # the scalar driver passes `seed` through Sampler::seed, which adds the sampler's own `seed` property (sampler.cpp:129-131)
    check(lib().har_render_scalar(C.byref(d), C.byref(sensor.har), int(seed) & 0xffffffff, spp, integrator.max_depth, integrator.rr_depth, block_size, threads,
                                   film.ctypes.data_as(C.c_void_p), C.byref(used)))
    wgt = film[..., 3:4]
    rgb = film[..., :3]
    rows = _COLOUR_ROWS[sensor.film().colour]           # `luminance` / `xyz` films: the colour transform of HDRFilm::develop on the weighted sums, then / W
    if rows is not None:
        rgb = rgb @ np.asarray(rows, np.float32).T
    return rgb / np.where(wgt == 0, 1.0, wgt).astype(np.float32)


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(_capi.f32p)


def _up(a):
    return a.ctypes.data_as(_capi.u32p)


def _torch():
    import torch
    return torch


def _device():
    torch = _torch()
    if not torch.cuda.is_available():
        raise HarError("hip_ad_rgb requires a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
    _capi.install_torch_allocator()         # once: the library allocates through PyTorch's caching allocator (har_set_allocator)
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# ---------------------------------------------------------------------------
#  ScalarTransform4f (include/mitsuba/core/transform.h) -- evaluated in C++
# ---------------------------------------------------------------------------

class ScalarTransform4f:
    def __init__(self, data=None):
        if data is None:
            data = np.concatenate([np.eye(4, dtype=np.float32).ravel()] * 2)
        self.data = _f32(data).reshape(32)

    def _chain(self, other):
        out = np.empty(32, np.float32)
        check(lib().har_transform_mul(_fp(self.data), _fp(other), _fp(out)))
        return ScalarTransform4f(out)

    def translate(self, v):
        out = np.empty(32, np.float32); check(lib().har_transform_translate(_fp(_f32(v)), _fp(out))); return self._chain(out)

    def scale(self, v):
        v = _f32([v, v, v]) if np.isscalar(v) else _f32(v)
        out = np.empty(32, np.float32); check(lib().har_transform_scale(_fp(v), _fp(out))); return self._chain(out)

    def rotate(self, axis, angle):
        out = np.empty(32, np.float32); check(lib().har_transform_rotate(_fp(_f32(axis)), float(angle), _fp(out))); return self._chain(out)

    def look_at(self, origin, target, up):
        out = np.empty(32, np.float32)
        check(lib().har_transform_look_at(_fp(_f32(origin)), _fp(_f32(target)), _fp(_f32(up)), _fp(out))); return self._chain(out)

    def inverse(self):
        out = np.empty(32, np.float32); check(lib().har_transform_inverse(_fp(self.data), _fp(out))); return ScalarTransform4f(out)

    def __matmul__(self, other):
        return self._chain(other.data)

    @property
    def matrix(self):
        return self.data[:16].reshape(4, 4)

    def col_major_3x4(self):
        return np.ascontiguousarray(self.matrix[:3, :].T).ravel().astype(np.float32)

    def has_scale(self):
        m = self.matrix[:3, :3].astype(np.float64)
        return not np.allclose(m @ m.T, np.eye(3), atol=1e-3)


Transform4f = ScalarTransform4f


class ScalarTransform3f:
    """ScalarAffineTransform3f (include/mitsuba/core/transform.h): 2-D affine maps, the type of BitmapTexture's `to_uv`.  Chained like the reference's Python API:
    T().translate(v).rotate(deg).scale(v) = translate * rotate * scale (the last call acts first on a point)."""

    def __init__(self, matrix=None):
        self.matrix = np.eye(3, dtype=np.float32) if matrix is None else np.asarray(matrix, np.float32).reshape(3, 3).copy()

    def _chain(self, m):
        # Transform::operator*, affine branch (transform.h:364-400): sums of fmadd in float32 -- float64 accumulation rounded once is the same value for these 2-term sums
        # except in the last bit; `to_uv` is consumed as six float32 numbers, so the stored matrix IS the parameter
        return ScalarTransform3f((self.matrix.astype(np.float64) @ np.asarray(m, np.float64)).astype(np.float32))

    def translate(self, v):
        m = np.eye(3, dtype=np.float32); m[0, 2] = v[0]; m[1, 2] = v[1]; return self._chain(m)

    def scale(self, v):
        v = [v, v] if np.isscalar(v) else v
        m = np.eye(3, dtype=np.float32); m[0, 0] = v[0]; m[1, 1] = v[1]; return self._chain(m)

    def rotate(self, angle):
        a = math.radians(float(angle)); c, sn = math.cos(a), math.sin(a)
        m = np.eye(3, dtype=np.float32); m[0, 0] = c; m[0, 1] = -sn; m[1, 0] = sn; m[1, 1] = c; return self._chain(m)

    def inverse(self):
        return ScalarTransform3f(np.linalg.inv(self.matrix.astype(np.float64)).astype(np.float32))

    def __matmul__(self, other):
        return self._chain(other.matrix)

    def rows_2x3(self):
        return [float(x) for x in self.matrix[:2, :].reshape(-1)]


Transform3f = ScalarTransform3f


def cornell_box():
    """mi.cornell_box() (src/python/python/util.py:569-703)."""
    T = ScalarTransform4f
    return {
        'type': 'scene',
        'integrator': {'type': 'path', 'max_depth': 8},
        'sensor': {
            'type': 'perspective', 'fov_axis': 'smaller', 'near_clip': 0.001, 'far_clip': 100.0,
            'focus_distance': 1000, 'fov': 39.3077,
            'to_world': T().look_at(origin=[0, 0, 3.90], target=[0, 0, 0], up=[0, 1, 0]),
            'sampler': {'type': 'independent', 'sample_count': 64},
            'film': {'type': 'hdrfilm', 'width': 256, 'height': 256, 'rfilter': {'type': 'gaussian'},
                     'pixel_format': 'rgb', 'component_format': 'float32'},
        },
        'white': {'type': 'diffuse', 'reflectance': {'type': 'rgb', 'value': [0.885809, 0.698859, 0.666422]}},
        'green': {'type': 'diffuse', 'reflectance': {'type': 'rgb', 'value': [0.105421, 0.37798, 0.076425]}},
        'red': {'type': 'diffuse', 'reflectance': {'type': 'rgb', 'value': [0.570068, 0.0430135, 0.0443706]}},
        'light': {'type': 'rectangle',
                  'to_world': T().translate([0.0, 0.99, 0.01]).rotate([1, 0, 0], 90).scale([0.23, 0.19, 0.19]),
                  'bsdf': {'type': 'ref', 'id': 'white'},
                  'emitter': {'type': 'area', 'radiance': {'type': 'rgb', 'value': [18.387, 13.9873, 6.75357]}}},
        'floor': {'type': 'rectangle', 'to_world': T().translate([0.0, -1.0, 0.0]).rotate([1, 0, 0], -90), 'bsdf': {'type': 'ref', 'id': 'white'}},
        'ceiling': {'type': 'rectangle', 'to_world': T().translate([0.0, 1.0, 0.0]).rotate([1, 0, 0], 90), 'bsdf': {'type': 'ref', 'id': 'white'}},
        'back': {'type': 'rectangle', 'to_world': T().translate([0.0, 0.0, -1.0]), 'bsdf': {'type': 'ref', 'id': 'white'}},
        'green-wall': {'type': 'rectangle', 'to_world': T().translate([1.0, 0.0, 0.0]).rotate([0, 1, 0], -90), 'bsdf': {'type': 'ref', 'id': 'green'}},
        'red-wall': {'type': 'rectangle', 'to_world': T().translate([-1.0, 0.0, 0.0]).rotate([0, 1, 0], 90), 'bsdf': {'type': 'ref', 'id': 'red'}},
        'small-box': {'type': 'cube', 'to_world': T().translate([0.335, -0.7, 0.38]).rotate([0, 1, 0], -17).scale(0.3), 'bsdf': {'type': 'ref', 'id': 'white'}},
        'large-box': {'type': 'cube', 'to_world': T().translate([-0.33, -0.4, -0.28]).rotate([0, 1, 0], 18.25).scale([0.3, 0.61, 0.3]), 'bsdf': {'type': 'ref', 'id': 'white'}},
    }


# ---------------------------------------------------------------------------
#  Wavefront record types (SoA torch tensors on the GPU)
# ---------------------------------------------------------------------------

class Ray3f:
    """Ray3f wavefront: o, d are float32 tensors [3, n]; maxt [n] (default Largest)."""

    def __init__(self, o, d, maxt=None):
        torch = _torch(); dev = _device()
        self.o = torch.as_tensor(o, dtype=torch.float32, device=dev).reshape(3, -1).contiguous()
        self.d = torch.as_tensor(d, dtype=torch.float32, device=dev).reshape(3, -1).contiguous()
        n = self.o.shape[1]
        if maxt is None:
            maxt = torch.full((n,), 3.402823466e+38, dtype=torch.float32, device=dev)
        self.maxt = torch.as_tensor(maxt, dtype=torch.float32, device=dev).reshape(-1).contiguous()
        if self.maxt.numel() == 1 and n > 1:
            self.maxt = self.maxt.expand(n).contiguous()

    def __len__(self):
        return self.o.shape[1]


class PreliminaryIntersection3f:
    """include/mitsuba/render/interaction.h:717-836"""

    def __init__(self, scene, t, u, v, prim_index, shape_index, inst_index):
        self.scene = scene
        self.t = t; self.prim_uv = (u, v); self.prim_index = prim_index
        self.shape_index = shape_index; self.instance = inst_index

    def is_valid(self):
        return ~_torch().isinf(self.t)

    def compute_surface_interaction(self, ray, ray_flags=None, active=True):
        """PreliminaryIntersection::compute_surface_interaction(ray, ray_flags = RayFlags::Default, active) (interaction.h:804-829)"""
        return self.scene._compute_si(ray, self, RayFlags.Default if ray_flags is None else ray_flags, active)


class SurfaceInteraction3f:
    """rows of har_compute_surface_interaction's output (include/hip_ad_rgb.h HAR_SI_ROWS; interaction.h:345-420)"""

    def __init__(self, raw):
        self.p = raw[0:3]; self.n = raw[3:6]
        self.sh_frame = type("Frame3f", (), dict(n=raw[6:9], s=raw[9:12], t=raw[12:15]))()
        self.wi = raw[15:18]; self.uv = raw[18:20]; self.t = raw[20]
        self.dp_du = raw[21:24]; self.dp_dv = raw[24:27]; self.dn_du = raw[27:30]; self.dn_dv = raw[30:33]

    def is_valid(self):
        return ~_torch().isinf(self.t)


class RayFlags:
    """include/mitsuba/render/interaction.h:19-87"""
    Minimal = 0x0; Shading = 0x1; NormalPartials = 0x2; Default = 0x1; All = 0x1; FollowShape = 0x4; DetachShape = 0x8


class TransportMode:
    """include/mitsuba/render/fwd.h / bsdf.h: Radiance = 0, Importance = 1"""
    Radiance = 0; Importance = 1


class BSDFFlags:
    """include/mitsuba/render/bsdf.h:31-125 (the lobe types and their unions)"""
    Empty = 0x0; Null = 0x1; DiffuseReflection = 0x2; DiffuseTransmission = 0x4; GlossyReflection = 0x8; GlossyTransmission = 0x10
    DeltaReflection = 0x20; DeltaTransmission = 0x40; Delta1DReflection = 0x80; Delta1DTransmission = 0x100
    Reflection = 0x2 | 0x20 | 0x80 | 0x8; Transmission = 0x4 | 0x40 | 0x100 | 0x10 | 0x1
    Diffuse = 0x2 | 0x4; Glossy = 0x8 | 0x10; Smooth = 0x2 | 0x4 | 0x8 | 0x10; Delta = 0x1 | 0x20 | 0x40; Delta1D = 0x80 | 0x100; All = 0x1ff
    Anisotropic = 0x1000; NonSymmetric = 0x4000; FrontSide = 0x8000; BackSide = 0x10000          # lobe attributes (bsdf.h:71-83): reported by BSDF.flags(), not part of a type mask


class BSDFContext:
    """include/mitsuba/render/bsdf.h:140-186: transport mode, lobe type mask, component index; every BSDF call honours all three (har_bsdf_*)"""

    def __init__(self, mode=TransportMode.Radiance, type_mask=0x1ff, component=0xffffffff):
        self.mode = int(mode); self.type_mask = int(type_mask) & 0xffffffff; self.component = int(component) & 0xffffffff

    def reverse(self):
        self.mode = 1 - self.mode

    def is_enabled(self, type_, component_=0):
        t = int(type_)
        return (self.type_mask == 0xffffffff or (self.type_mask & t) == t) and (self.component == 0xffffffff or self.component == component_)

    def _c(self):
        from ._capi import HarBSDFContext
        if self.mode not in (0, 1):
            raise RuntimeError("BSDFContext.mode must be TransportMode.Radiance or TransportMode.Importance")
        return C.byref(HarBSDFContext(self.mode, self.type_mask, self.component))


def _mask(active, n):
    """the reference's `Mask active` argument -> device uint8[n] (None when every lane is active: the C ABI's NULL)"""
    if active is True or active is None:
        return None
    torch = _torch()
    if active is False:
        return torch.zeros(n, dtype=torch.uint8, device=_device())
    a = torch.as_tensor(active, device=_device()).reshape(-1)
    a = (a != 0).to(torch.uint8)
    if a.numel() == 1 and n != 1:
        a = a.expand(n)
    if a.numel() != n:
        raise RuntimeError("active: mask of %d entries for a wavefront of %d lanes" % (a.numel(), n))
    return a.contiguous()


def _ctx(ctx):
    if ctx is None:
        return None
    if not isinstance(ctx, BSDFContext):
        raise RuntimeError("ctx must be a BSDFContext (or None for the default context)")
    return ctx._c()


# ---------------------------------------------------------------------------
#  Plugins
# ---------------------------------------------------------------------------

class Mesh:
    """Triangle mesh in the packed layout (mesh_utils.h:19-34)."""

    def __init__(self, name="mesh"):
        self.name = name
        self.V = np.zeros((0, 8), np.float32); self.F = np.zeros((0, 4), np.uint32); self.flags = 0
        self.bsdf = None; self.emitter = None
        self.attributes = {}          # Mesh::m_mesh_attributes: name -> float32 (rows, dim), one row per vertex ('vertex_*') or per face ('face_*')

    # -- mesh attributes (Mesh::add_attribute / remove_attribute / has_attribute / attribute, src/render/mesh.cpp:2538-2601).  `to_world` and `flip_normals` leave them alone.
    def add_attribute(self, name, values):
        name = str(name)
        if name in self.attributes:
            raise RuntimeError("add_attribute(): attribute \"%s\" already exists." % name)
        vertex = name.startswith("vertex_")
        if not vertex and not name.startswith("face_"):
            raise RuntimeError("add_attribute(): attribute name must start with either \"vertex_\" or \"face_\".")
        if hasattr(values, 'detach'):
            values = values.detach().cpu().numpy()
        values = np.asarray(values, np.float32)
        rows = self.vertex_count() if vertex else self.face_count()
        if values.ndim != 2 or values.shape[0] != rows:
            raise RuntimeError("add_attribute(): attribute \"%s\": expected a (%d, dim) tensor with one row per %s." % (name, rows, "vertex" if vertex else "face"))
        dim = values.shape[1]
        if dim == 0 or dim > 4:
            raise RuntimeError("add_attribute(): attribute \"%s\": 1 to 4 channels are supported, got %d." % (name, dim))
        self.attributes[name] = np.ascontiguousarray(values, np.float32).copy()
        return self

    def remove_attribute(self, name):
        if name not in self.attributes:
            raise RuntimeError("remove_attribute(): attribute \"%s\" doesn't exist." % name)       # (Shape::remove_attribute: this variant has no texture attributes on shapes)
        del self.attributes[name]

    def has_attribute(self, name):
        return name in self.attributes

    def attribute(self, name):
        if name not in self.attributes:
            raise RuntimeError("attribute(): attribute \"%s\" doesn't exist." % name)
        return self.attributes[name]

    def from_fields(self, faces, positions, normals=None, texcoords=None):
        positions = _f32(positions).reshape(-1, 3)
        V = np.zeros((positions.shape[0], 8), np.float32); V[:, 0:3] = positions
        flags = 0
        if normals is not None:
            V[:, 3:6] = _f32(normals).reshape(-1, 3); flags |= 1
        if texcoords is not None:
            V[:, 6:8] = _f32(texcoords).reshape(-1, 2); flags |= 2
        F = np.zeros((np.asarray(faces).reshape(-1, 3).shape[0], 4), np.uint32)
        F[:, :3] = np.asarray(faces, dtype=np.uint32).reshape(-1, 3)
        self.V, self.F, self.flags = V, F, flags
        return self

    def _adopt(self, md):
        try:
            nv, nf = md.vertex_count, md.face_count
            self.V = np.ctypeslib.as_array(md.vertices, shape=(max(nv, 1), 8))[:nv].copy() if nv else np.zeros((0, 8), np.float32)
            self.F = np.ctypeslib.as_array(md.faces, shape=(max(nf, 1), 4))[:nf].copy() if nf else np.zeros((0, 4), np.uint32)
            self.flags = int(md.flags)
        finally:
            lib().har_mesh_free(C.byref(md))
        return self

    @staticmethod
    def _tw(to_world):
        return _fp(to_world.data) if to_world is not None else None

    def from_ply(self, filename, face_normals=False, flip_tex_coords=False, to_world=None, flip_normals=False):
        """PLYMesh (src/shapes/ply.cpp): parsed by the C++ host library into the packed layout; `to_world` / `flip_normals` are
        baked before missing normals are regenerated, as PackedMesh::set_transform does (mesh_utils.cpp:33-44)."""
        md = _capi.HarMeshData(); fields = _capi.HarMeshFields()
        check(lib().har_mesh_load_ply_fields(str(filename).encode(), int(bool(face_normals)), int(bool(flip_tex_coords)), self._tw(to_world), int(bool(flip_normals)), C.byref(md),
                                             C.byref(fields)))
        try:
            nv, nf = int(md.vertex_count), int(md.face_count)
            groups = []
            for prefix, names, data, cols, rows in (("vertex_", fields.vertex_names, fields.vertex_data, int(fields.vertex_cols), nv), ("face_", fields.face_names, fields.face_data, int(fields.face_cols), nf)):
                cols_named = [ln.split(":", 1) for ln in C.string_at(names).decode().split("\n") if ln] if names else []
                table = np.ctypeslib.as_array(data, shape=(max(rows * cols, 1), ))[:rows * cols].reshape(rows, cols).copy() if rows * cols else np.zeros((rows, cols), np.float32)
                reserved = ("x", "y", "z", "nx", "ny", "nz", "u", "v") if prefix == "vertex_" else ()
                for name, idx in _ply_other_fields(prefix, [(n, t == "f") for t, n in cols_named], reserved, str(filename)):
                    groups.append((name, np.ascontiguousarray(table[:, idx], np.float32)))
        finally:
            lib().har_mesh_fields_free(C.byref(fields))
        self._adopt(md)
        self.attributes = {}
        for name, values in groups:          # PLYMesh: pm.add_attribute(descr.name, descr.dim) (ply.cpp:259-262, 308-311); rows in the order of the vertex / face records
            self.add_attribute(name, values)
        return self

    def from_obj(self, filename, face_normals=False, flip_tex_coords=True, to_world=None, flip_normals=False):
        """OBJMesh (src/shapes/obj.cpp) + Mesh::from_corners (mesh_utils.cpp:210-560)"""
        md = _capi.HarMeshData()
        check(lib().har_mesh_load_obj(str(filename).encode(), int(bool(face_normals)), int(bool(flip_tex_coords)), self._tw(to_world), int(bool(flip_normals)), C.byref(md)))
        return self._adopt(md)

    def from_serialized(self, filename, shape_index=0, face_normals=None, to_world=None, flip_normals=False):
        """SerializedMesh (src/shapes/serialized.cpp), container versions 3, 4 and 5; face_normals=None: the property is unset (a v5 file's own flag applies)"""
        md = _capi.HarMeshData(); fields = _capi.HarMeshFields()
        fn = -1 if face_normals is None else int(bool(face_normals))
        check(lib().har_mesh_load_serialized_fields(str(filename).encode(), int(shape_index), fn, self._tw(to_world), int(bool(flip_normals)), C.byref(md), C.byref(fields)))
        try:
            groups = []
            for names, data, rows in ((fields.vertex_names, fields.vertex_data, int(md.vertex_count)), (fields.face_names, fields.face_data, int(md.face_count))):
                at = 0
                for ln in (C.string_at(names).decode().split("\n") if names else []):
                    if not ln:
                        continue
                    name, dim = ln.rsplit(":", 1); dim = int(dim)
                    n = rows * dim
                    vals = np.ctypeslib.as_array(data, shape=(max(at + n, 1), ))[at:at + n].reshape(rows, dim).copy() if n else np.zeros((rows, dim), np.float32)
                    groups.append((name, vals)); at += n
        finally:
            lib().har_mesh_fields_free(C.byref(fields))
        self._adopt(md)
        self.attributes = {}
        for name, values in groups:          # the custom attributes of a version-5 file (SerializedMesh::load_v5 -> add_attribute)
            self.add_attribute(name, values)
        return self

    def recompute_vertex_normals(self):
        """Mesh::compute_normals (src/render/mesh.cpp:1218-1267)"""
        self.V = np.ascontiguousarray(self.V); self.F = np.ascontiguousarray(self.F)
        check(lib().har_mesh_compute_normals(self.V.shape[0], _fp(self.V), self.F.shape[0], _up(self.F)))
        self.flags |= 1
        return self

    def transform(self, to_world):
        self.V = np.ascontiguousarray(self.V); self.F = np.ascontiguousarray(self.F)
        check(lib().har_mesh_transform(_fp(to_world.data), self.V.shape[0], _fp(self.V), self.F.shape[0], _up(self.F), self.flags & 1))
        return self

    def face_count(self):
        return self.F.shape[0]

    def vertex_count(self):
        return self.V.shape[0]


# Shape(props) (src/render/shape.cpp:17-60) + Mesh(props) (src/render/mesh.cpp:160-175): rectangle and cube are Mesh plugins in this tree.
# `silhouette_sampling_weight` only feeds the projective integrators' boundary sampling: queried, no effect on `path` / `prb`.
_SHAPE_PROPS = ('to_world', 'flip_normals', 'face_normals', 'silhouette_sampling_weight')
_SHAPE_CHILDREN = ('bsdf', 'emitter')       # Shape(props) (shape.cpp:22-49) also takes sensors, media and texture attributes: not part of this variant, refused


def _ply_other_fields(prefix, fields, reserved, filename):
    """find_other_fields (src/shapes/ply.h:272-422): the attributes PLYMesh forms from the properties of an element that are not positions, normals, texcoords or indices.
    `fields` = [(property name, is float)] in file order -> [(attribute name, [column indices])].  `r g b [a]` / `red green blue [alpha]` become `<prefix>color` (3 or 4
    fields); contiguous runs `<p>_{x,y,z,w | r,g,b,a | 0,1,2,3 | 1,2,3,4}` become `<prefix><p>` (`<prefix><p>_color` for the r g b a scheme) when they have 1 or 3 fields,
    and are dropped with a warning otherwise.  Integer fields are converted to float without rescaling (a warning, as there)."""
    names = [n for n, _ in fields]
    if prefix == "vertex_":            # ply.cpp:238-246: texture_u / texture_v, or s / t, are the texcoords
        if "texture_u" in names and "texture_v" in names:
            names = ["u" if n == "texture_u" else "v" if n == "texture_v" else n for n in names]
        elif "s" in names and "t" in names:
            names = ["u" if n == "s" else "v" if n == "t" else n for n in names]
    if not ("r" in names and "g" in names and "b" in names) and "red" in names and "green" in names and "blue" in names:
        ren = {"red": "r", "green": "g", "blue": "b"}
        if "alpha" in names:
            ren["alpha"] = "a"
        names = [ren.get(n, n) for n in names]
    out = []
    if "r" in names and "g" in names and "b" in names:
        idx = [names.index(c) for c in ("r", "g", "b")] + ([names.index("a")] if "a" in names else [])
        out.append((prefix + "color", idx))
        if not fields[idx[0]][1]:
            warnings.warn("\"%s\": Mesh attribute \"%s\" has integer fields: color attributes are expected to be in the [0, 1] range." % (filename, prefix + "color"))
    reserved = set(reserved) | {"r", "g", "b", "a"}
    if prefix == "face_":
        reserved |= {"vertex_index.count", "vertex_indices.count", "i0", "i1", "i2"}
    postfixes = ("xr01", "yg12", "zb23", "wa34")
    seen = set(); state = dict(prefix="", scheme=0, level=0, reading=False, cols=[], is_float=True)

    def ignore():
        state.update(prefix="", scheme=0, level=0, reading=False, cols=[])

    def flush():
        if state["level"] not in (1, 3):
            warnings.warn("\"%s\": attribute must have either 1 or 3 fields (had %d) : attribute \"%s\" ignored" % (filename, state["level"], prefix + state["prefix"]))
            ignore(); return
        if not state["is_float"] and state["level"] == 3:
            warnings.warn("\"%s\": attribute \"%s\" has integer fields: color attributes are expected to be in the [0, 1] range." % (filename, prefix + state["prefix"]))
        out.append((prefix + state["prefix"] + ("_color" if state["scheme"] == 1 else ""), list(state["cols"])))
        seen.add(state["prefix"]); ignore()

    i = 0; n = len(names)
    while i < n:
        name = names[i]
        if name in reserved:
            i += 1; continue
        state["is_float"] = fields[i][1]
        pos = name.rfind("_")
        if pos < 0:
            warnings.warn("\"%s\": attributes without postfix are not handled for now: attribute \"%s\" ignored." % (filename, name))
            if state["reading"]:
                flush()
            i += 1; continue
        post = name[pos + 1:]
        if len(post) != 1:
            warnings.warn("\"%s\": attribute postfix can only be one letter long." % filename)
            if state["reading"]:
                flush()
            i += 1; continue
        pre = name[:pos]
        if state["reading"] and pre != state["prefix"]:
            flush()
        if not state["reading"] and pre in seen:
            warnings.warn("\"%s\": attribute prefix has already been encountered: attribute \"%s\" ignored." % (filename, name))
            while i < n and names[i].startswith(pre):
                i += 1
            if i == n:
                break
            i += 1; continue           # (the reference's loop increment skips the field it stopped at)
        if not state["reading"]:
            if post not in postfixes[0]:
                warnings.warn("\"%s\": attribute can't start with postfix %s." % (filename, post))
                i += 1; continue
            state.update(reading=True, scheme=postfixes[0].index(post), prefix=pre, cols=[])
        elif state["level"] >= 4 or post != postfixes[state["level"]][state["scheme"]]:
            warnings.warn("\"%s\": attribute postfix sequence is invalid: attribute \"%s\" ignored." % (filename, state["prefix"]))
            ignore()
            while i < n and names[i].startswith(pre):
                i += 1
            if i == n:
                break
        state["level"] += 1; state["cols"].append(i)
        i += 1
    if state["reading"]:
        flush()
    return out


def _rectangle(props):
    _check_props('rectangle', props, _SHAPE_PROPS, unsupported=(('face_normals', False),), children=_SHAPE_CHILDREN)
    tw = props.get('to_world', ScalarTransform4f())
    m = Mesh("rectangle")
    V = np.empty((4, 8), np.float32); F = np.empty((2, 4), np.uint32); n = np.empty(3, np.float32); ia = C.c_float()
    check(lib().har_shape_rectangle(_fp(tw.data), 1 if props.get('flip_normals', False) else 0, _fp(V), _up(F), _fp(n), C.byref(ia)))
    m.V, m.F, m.flags = V, F, 3
    m.rect = dict(to_world=tw, normal=n, inv_area=ia.value, flip=bool(props.get('flip_normals', False)))
    return m


def _cube(props):
    _check_props('cube', props, _SHAPE_PROPS, unsupported=(('face_normals', False), ('flip_normals', False)), children=_SHAPE_CHILDREN)
    tw = props.get('to_world', ScalarTransform4f())
    m = Mesh("cube")
    V = np.empty((24, 8), np.float32); F = np.empty((12, 4), np.uint32)
    check(lib().har_shape_cube(_fp(tw.data), _fp(V), _up(F)))
    m.V, m.F, m.flags = V, F, 3
    return m


# ObjectType of every plugin this variant has (include/mitsuba/core/object.h: ObjectType; PluginManager::create_object checks it, plugin.cpp:258-263).
# `rgb` is the dict form of a colour property, which the reference's loader turns into an `srgb` texture object (src/core/python/parser.cpp) -- a texture here.
_PLUGIN_KINDS = {
    'scene': 'scene', 'path': 'integrator', 'prb': 'integrator', 'aov': 'integrator', 'perspective': 'sensor', 'orthographic': 'sensor', 'thinlens': 'sensor', 'batch': 'sensor', 'hdrfilm': 'film', 'independent': 'sampler',
    'diffuse': 'bsdf', 'dielectric': 'bsdf', 'conductor': 'bsdf', 'plastic': 'bsdf', 'roughconductor': 'bsdf', 'roughplastic': 'bsdf', 'thindielectric': 'bsdf', 'twosided': 'bsdf', 'blendbsdf': 'bsdf', 'mask': 'bsdf', 'normalmap': 'bsdf', 'bumpmap': 'bsdf',
    'area': 'emitter', 'constant': 'emitter', 'envmap': 'emitter', 'point': 'emitter', 'spot': 'emitter', 'directional': 'emitter', 'projector': 'emitter',
    'rectangle': 'shape', 'cube': 'shape', 'mesh': 'shape', 'ply': 'shape', 'obj': 'shape', 'serialized': 'shape', 'shapegroup': 'shape', 'instance': 'shape',
    'gaussian': 'rfilter', 'box': 'rfilter', 'tent': 'rfilter', 'mitchell': 'rfilter', 'catmullrom': 'rfilter', 'lanczos': 'rfilter',
    'rgb': 'texture', 'bitmap': 'texture', 'mesh_attribute': 'texture',
}
_ALL_KINDS = tuple(sorted(set(_PLUGIN_KINDS.values())))


def _plugin_kind(t):
    """The ObjectType of plugin `t`; an unknown name is the reference's `Plugin "..." could not be found` (plugin.cpp:189)."""
    k = _PLUGIN_KINDS.get(t)
    if k is None and (t, VARIANT) in _REGISTRY:
        k = 'integrator'                     # mi.register_integrator is the only way a plugin gets into the registry from outside
    if k is None:
        raise RuntimeError("Plugin \"%s\" not found for variant \"%s\" (could not be found). Available: %s" % (t, VARIANT, sorted(_PLUGIN_KINDS)))
    return k


def _object_kind(v):
    """ObjectType of a child value: a dict by its plugin name, an instantiated object by its class; None: not an object (a number, a transform, a `ref`)"""
    if isinstance(v, dict):
        if 'type' not in v or v['type'] == 'ref':
            return None
        return _plugin_kind(v['type'])
    for cls, kind in ((Film, 'film'), (Sampler, 'sampler'), (BSDF, 'bsdf'), (Mesh, 'shape')):
        if isinstance(v, cls):
            return kind
    g = globals()
    for name, kind in (('Sensor', 'sensor'), ('Integrator', 'integrator'), ('ShapeGroup', 'shape'), ('Instance', 'shape'), ('Scene', 'scene'), ('AreaLight', 'emitter'),
                       ('ConstantEmitter', 'emitter'), ('EnvmapEmitter', 'emitter'), ('PointLight', 'emitter'), ('SpotLight', 'emitter'), ('DirectionalEmitter', 'emitter'), ('Projector', 'emitter')):
        if name in g and isinstance(v, g[name]):
            return kind
    return None


def _type_mismatch(v, actual, expected):
    name = v.get('type') if isinstance(v, dict) else {'Film': 'hdrfilm', 'Sampler': 'independent'}.get(type(v).__name__, getattr(v, 'kind', None) or getattr(v, 'type', None) or type(v).__name__)
    return RuntimeError("Type mismatch: the instantiated plugin \"%s\" is of type \"%s\", which does not match the expected type \"%s\"." % (name, actual, "|".join(expected)))


def _check_props(plugin, props, known, unsupported=(), free_children=True, children=(), slots=None, slot_kind=('texture',)):
    """The reference's plugin loader rejects properties a plugin never queried ("Unreferenced property", src/core/plugin.cpp / properties.cpp)
    -- a silently ignored property would be a silently different picture.  `unsupported`: (name, neutral value) pairs the reference knows
    but hip_ad_rgb does not implement; anything but the neutral value is refused.

    Child OBJECTS are held to the same rule by their plugin type (round 6): every dict with a `type` names a plugin that must exist
    (plugin.cpp:189) and be of the ObjectType its position wants (plugin.cpp:258-263 "Type mismatch") --
      * under a name of `known`: the kinds of `slots[name]`, else `slot_kind` (object-valued properties of BSDFs / emitters are textures);
      * under a free name (`free_children`: plugins that walk props.objects()): one of `children`; another kind is an object the constructor
        never casts successfully, i.e. an unreferenced property (properties.h:700-725)."""
    for name, neutral in unsupported:
        if name in props and props[name] != neutral:
            raise RuntimeError("%s: property \"%s\" = %r is not implemented by hip_ad_rgb" % (plugin, name, props[name]))
    slots = slots or {}
    for k, v in props.items():
        if k in ('type', 'id'):
            continue
        kind = _object_kind(v)                               # raises for a plugin that does not exist, wherever it sits
        if k in known or any(k == u[0] for u in unsupported):
            want = slots.get(k, slot_kind)
            if kind is not None and kind not in want:
                raise _type_mismatch(v, kind, want)
            continue
        if kind is not None or (isinstance(v, dict) and v.get('type') == 'ref'):
            if not free_children:
                raise RuntimeError("Unreferenced property \"%s\" in plugin of type \"%s\"!" % (k, plugin))
            if kind is not None and kind not in children:
                raise RuntimeError("Unreferenced property \"%s\" in plugin of type \"%s\": an object of type \"%s\" (plugin \"%s\") is not a child this plugin takes (%s)"
                                   % (k, plugin, kind, v.get('type') if isinstance(v, dict) else type(v).__name__, "|".join(children) or "none"))
            continue
        if k.startswith('_arg_'):
            continue
        if free_children and hasattr(v, 'har'):
            continue
        raise RuntimeError("Unreferenced property \"%s\" in plugin of type \"%s\"!" % (k, plugin))


class Sampler:
    """IndependentSampler (src/samplers/independent.cpp) over PCG32Sampler (src/render/sampler.cpp)."""

    def __init__(self, props=None):
        props = props or {}
        if props.get('type', 'independent') != 'independent':        # the other samplers of the reference (stratified, multijitter, orthogonal, ldsampler) draw DIFFERENT streams
            _plugin_kind(props['type'])                               # not a plugin at all: plugin.cpp:189
            raise _type_mismatch(props, _plugin_kind(props['type']), ('sampler',))
        _check_props('independent', props, ('sample_count', 'seed'), free_children=False)
        self.m_sample_count = int(props.get('sample_count', 4))
        self.m_base_seed = int(props.get('seed', 0))
        self.m_samples_per_wavefront = 1
        self.m_wavefront_size = 0
        self.state = None; self.inc = None

    def sample_count(self):
        return self.m_sample_count

    def set_sample_count(self, spp):
        self.m_sample_count = int(spp)

    def set_samples_per_wavefront(self, n):
        self.m_samples_per_wavefront = int(n)
        if self.m_sample_count % self.m_samples_per_wavefront != 0:
            raise RuntimeError("sample_count should be a multiple of samples_per_wavefront!")

    def wavefront_size(self):
        return self.m_wavefront_size

    def seeded(self):
        return self.state is not None

    def clone(self):
        """Sampler::clone (sampler.h:89-99): same configuration and the same streams (har_sampler_clone)"""
        s = Sampler(); s.__dict__.update(self.__dict__)
        if self.state is not None:
            torch = _torch()
            s.state = torch.empty_like(self.state); s.inc = torch.empty_like(self.inc)
            check(lib().har_sampler_clone(self.m_wavefront_size, _ptr(self.state), _ptr(self.inc), _ptr(s.state), _ptr(s.inc), _stream()))
        return s

    def advance(self):
        """Sampler::advance (sampler.h:109-115, independent.cpp:69-72): next sample, dimension index 0; the PCG32 streams are not reseeded"""
        self.m_sample_index = getattr(self, "m_sample_index", 0) + 1
        if self.state is not None:
            check(lib().har_sampler_advance(self.m_wavefront_size, _ptr(self.state), _ptr(self.inc), _stream()))

    def schedule_state(self):
        """Sampler::schedule_state (sampler.h:127): nothing to schedule -- there is no tracing JIT on this path"""

    def fork(self):
        s = Sampler(); s.m_sample_count = self.m_sample_count; s.m_base_seed = self.m_base_seed
        return s

    def seed(self, seed, wavefront_size=None):
        torch = _torch(); dev = _device()
        if wavefront_size is None:
            if self.m_wavefront_size == 0:
                raise RuntimeError("Sampler::seed(): wavefront_size should be specified!")
        else:
            self.m_wavefront_size = int(wavefront_size)
        n = self.m_wavefront_size
        self.state = torch.empty(n, dtype=torch.int64, device=dev); self.inc = torch.empty(n, dtype=torch.int64, device=dev)
        self.m_seed_value = (self.m_base_seed + int(seed)) & 0xffffffff          # the streams' increments are a function of (seed value, lane)
        check(lib().har_sampler_seed(self.m_seed_value, 0, n, _ptr(self.state), _ptr(self.inc), _stream()))

    def _active(self, active):
        if active is None:
            return None
        torch = _torch()
        return torch.as_tensor(active, device=_device()).to(torch.uint8).contiguous()

    def next_1d(self, active=None):
        assert self.seeded()
        torch = _torch(); n = self.m_wavefront_size
        out = torch.empty(n, dtype=torch.float32, device=_device()); a = self._active(active)
        check(lib().har_sampler_next_1d(n, _ptr(self.state), _ptr(self.inc), _ptr(a), _ptr(out), _stream()))
        return out

    def next_2d(self, active=None):
        assert self.seeded()
        torch = _torch(); n = self.m_wavefront_size
        out = torch.empty((2, n), dtype=torch.float32, device=_device()); a = self._active(active)
        check(lib().har_sampler_next_2d(n, _ptr(self.state), _ptr(self.inc), _ptr(a), _ptr(out), _stream()))
        return out


class Film:
    """HDRFilm (src/films/hdrfilm.cpp) + its reconstruction filter."""

    def __init__(self, props=None):
        props = props or {}
        if props.get('type', 'hdrfilm') != 'hdrfilm':                 # specfilm is not part of an RGB variant's path
            raise _type_mismatch(props, _plugin_kind(props['type']), ('film',))
        # hdrfilm.cpp:146-208; file_format / component_format only concern Film::write (har_image_write_*: float32 / half channels)
        _check_props('hdrfilm', props, ('width', 'height', 'crop_offset_x', 'crop_offset_y', 'crop_width', 'crop_height', 'pixel_format', 'file_format', 'component_format',
                                        'sample_border', 'compensate', 'banner'), children=('rfilter',))
        if 'compensate' in props:          # hdrfilm.cpp:218-225: marked as queried, warned about, ignored
            import warnings
            warnings.warn("The \"compensate\" (Kahan-style error-compensated accumulation) parameter has been removed and is now ignored.")
        self.width = int(props.get('width', 768)); self.height = int(props.get('height', 576))
        self.crop_offset_ = (int(props.get('crop_offset_x', 0)), int(props.get('crop_offset_y', 0)))
        self.crop_size_ = (int(props.get('crop_width', self.width)), int(props.get('crop_height', self.height)))
        if min(self.width, self.height, *self.crop_offset_, *self.crop_size_) < 0:
            raise RuntimeError("hdrfilm: sizes and offsets are unsigned")
        # Film::set_crop_window (src/render/film.cpp:90-99)
        if self.crop_offset_[0] + self.crop_size_[0] > self.width or self.crop_offset_[1] + self.crop_size_[1] > self.height:
            raise RuntimeError("Invalid crop window specification: crop_offset(%u, %u) + crop_size(%u, %u) > size(%u, %u)"
                               % (self.crop_offset_ + self.crop_size_ + (self.width, self.height)))
        pf = str(props.get('pixel_format', 'rgb')).lower()          # hdrfilm.cpp:149-176
        formats = {'rgb': (0, False), 'rgba': (0, True), 'luminance': (1, False), 'luminance_alpha': (1, True), 'xyz': (2, False), 'xyza': (2, True)}
        if pf not in formats:
            raise RuntimeError("The \"pixel_format\" parameter must either be equal to \"luminance\", \"luminance_alpha\", \"rgb\", \"rgba\",  \"xyz\", \"xyza\". Found %s." % pf)
        self.pixel_format = pf
        self.colour, self.alpha = formats[pf]        # colour: HAR_PIXEL_RGB / _Y / _XYZ of har_film_develop_format; alpha: FilmFlags::Alpha
        rf = next((v for v in props.values() if isinstance(v, dict) and 'type' in v), {'type': 'gaussian'})     # the film's only child object is its rfilter
        self.rf_param1 = 1.0 / 3.0
        if rf['type'] == 'gaussian':                     # src/rfilters/gaussian.cpp:48-55
            self.rfilter = 1; self.stddev = float(rf.get('stddev', 0.5))
        elif rf['type'] == 'box':
            self.rfilter = 0; self.stddev = 0.5
        elif rf['type'] == 'tent':                       # tent.cpp:48-52
            self.rfilter = 2; self.stddev = float(rf.get('radius', 1.0))
        elif rf['type'] == 'mitchell':                   # mitchell.cpp:50-58
            self.rfilter = 3; self.stddev = float(rf.get('B', 1.0 / 3.0)); self.rf_param1 = float(rf.get('C', 1.0 / 3.0))
        elif rf['type'] == 'catmullrom':
            self.rfilter = 4; self.stddev = 0.0
        elif rf['type'] == 'lanczos':                    # lanczos.cpp:52-55
            self.rfilter = 5; self.stddev = float(int(rf.get('lobes', 3)))
        else:
            raise RuntimeError("Plugin \"%s\" not found for variant hip_ad_rgb (rfilters: box, gaussian, tent, mitchell, catmullrom, lanczos)" % rf['type'])

        # Film::sample_border (film.cpp:29-32): samples are also drawn in a border of rfilter->border_size() = ceil(radius - 1/2 - 2 RayEpsilon) pixels
        # (rfilter.cpp:22) around the crop window; the film keeps its size, the splats of border samples are clipped to it
        radius = {0: 0.5, 1: 4.0 * self.stddev, 2: self.stddev, 3: 2.0, 4: 2.0, 5: self.stddev}[self.rfilter]
        self.sample_border_ = bool(props.get('sample_border', False))
        self.border_size_ = max(0, int(math.ceil(np.float32(np.float32(radius) - np.float32(0.5)) - np.float32(2.0 * 1500.0 * 2.0 ** -24)))) if self.sample_border_ else 0

    def splat_reach(self):
        """film rows a sample can reach above / below its own pixel row: the filter footprint of ImageBlock::put (imageblock.cpp:444-470), ceil(radius - 1/2) -- 0 for
        the box filter (film_footprint, har_path.h)"""
        if self.rfilter == 0:
            return 0
        radius = {1: 4.0 * self.stddev, 2: self.stddev, 3: 2.0, 4: 2.0, 5: self.stddev}[self.rfilter]
        return int(math.ceil(np.float32(np.float32(radius) - np.float32(0.5))))

    def band_rows(self, y0, y1):
        """the rows [lo, hi) of the crop window that samples of the sample-grid rows [y0, y1) splat into (sample border + filter reach)"""
        reach = self.splat_reach()
        return max(0, y0 - self.border_size_ - reach), min(self.crop_size_[1], y1 - self.border_size_ + reach)

    def sample_grid(self):
        """pixels of the lane -> pixel map of render(): crop_size + 2 * border_size with sample_border (integrator.cpp:162-165), else the crop size"""
        return (self.crop_size_[0] + 2 * self.border_size_, self.crop_size_[1] + 2 * self.border_size_)

    def sample_border(self):
        return self.sample_border_

    def size(self):
        return (self.width, self.height)

    def crop_size(self):
        return self.crop_size_

    def crop_offset(self):
        return self.crop_offset_


class Sensor:
    """PerspectiveCamera (src/sensors/perspective.cpp), OrthographicCamera (src/sensors/orthographic.cpp) and ThinLensCamera (src/sensors/thinlens.cpp)."""

    def __init__(self, props):
        self.props = dict(props)
        self.kind = props.get('type', 'perspective')
        # sensor.cpp:24-97, perspective.cpp:137-172, orthographic.cpp:93-97
        if self.kind == 'orthographic':
            _check_props('orthographic', props, ('to_world', 'near_clip', 'far_clip', 'film', 'sampler', 'shutter_open', 'shutter_close'), children=('film', 'sampler'),
                         slots={'film': ('film',), 'sampler': ('sampler',)}, slot_kind=())
        elif self.kind == 'thinlens':            # thinlens.cpp:152-169: no principal point offsets; `aperture_radius` is required
            _check_props('thinlens', props, ('to_world', 'fov', 'fov_axis', 'focal_length', 'near_clip', 'far_clip', 'film', 'sampler', 'shutter_open', 'shutter_close', 'focus_distance',
                                             'aperture_radius'), children=('film', 'sampler'), slots={'film': ('film',), 'sampler': ('sampler',)}, slot_kind=())
            if 'aperture_radius' not in props:
                raise RuntimeError("Property \"aperture_radius\" has not been specified!")
        else:
            _check_props('perspective', props, ('to_world', 'fov', 'fov_axis', 'focal_length', 'near_clip', 'far_clip', 'film', 'sampler', 'shutter_open', 'shutter_close', 'focus_distance',
                                                'principal_point_offset_x', 'principal_point_offset_y'), children=('film', 'sampler'),
                         slots={'film': ('film',), 'sampler': ('sampler',)}, slot_kind=())
        # child objects are recognised by their class, whatever the property is called (XML children are anonymous: `_arg_0`, ...)
        film = next((v for v in props.values() if isinstance(v, Film)), props.get('film'))
        sampler = next((v for v in props.values() if isinstance(v, Sampler)), props.get('sampler'))
        self.m_film = film if isinstance(film, Film) else Film(film)
        self.m_sampler = sampler if isinstance(sampler, Sampler) else Sampler(sampler)
        self.to_world = props.get('to_world', ScalarTransform4f())
        if self.kind != 'orthographic' and self.to_world.has_scale():            # perspective.cpp:143-146; an orthographic camera's scale sets the size of its view
            raise RuntimeError("Scale factors in the camera-to-world transformation are not allowed!")
        if 'fov' in props and 'focal_length' in props:
            raise RuntimeError("Please specify either a focal length ('focal_length') or a field of view ('fov')!")
        self.near_clip = float(props.get('near_clip', 1e-2)); self.far_clip = float(props.get('far_clip', 1e4))
        if self.kind == 'thinlens':
            self.aperture_radius = float(props['aperture_radius'])
            self.focus_distance_ = float(props.get('focus_distance', self.far_clip))        # sensor.cpp:127
            if self.aperture_radius == 0.0:          # thinlens.cpp:158-161
                self.aperture_radius = float(np.float32(2.0 ** -24))
                warnings.warn("Can't have a zero aperture radius -- setting to %f" % self.aperture_radius)
        self.update()

    def needs_aperture_sample(self):
        """Sensor::needs_aperture_sample() (sensor.h): render() draws an aperture sample per lane right behind the pixel jitter"""
        return self.kind == 'thinlens'

    def focus_distance(self):
        """ProjectiveCamera::focus_distance() (sensor.cpp:127): `focus_distance`, by default far_clip"""
        return self.focus_distance_ if self.kind == 'thinlens' else float(self.props.get('focus_distance', self.far_clip))

    def update(self):
        f = self.m_film
        if self.kind == 'orthographic':            # OrthographicCamera::update_camera_transforms (orthographic.cpp:104-121)
            s = _capi.HarSensor()
            if lib().har_orthographic_sensor(_fp(self.to_world.data), self.near_clip, self.far_clip, f.width, f.height, f.crop_offset_[0], f.crop_offset_[1],
                                             f.crop_size_[0], f.crop_size_[1], f.rfilter, f.stddev, C.byref(s)):
                raise RuntimeError("invalid sensor parameters")
            s.rfilter_param1 = f.rf_param1
            s.sample_border = 1 if f.sample_border_ else 0
            self.har = s
            return
        fov_axis = self.props.get('fov_axis', 'x')
        if 'fov' in self.props:
            fov = float(self.props['fov'])
        else:
            fl = str(self.props.get('focal_length', '50mm'))
            value = float(fl[:-2] if fl.endswith('mm') else fl)
            fov = 2.0 * math.degrees(math.atan(math.sqrt(36 * 36 + 24 * 24) / (2.0 * value))); fov_axis = 'diagonal'
        s = _capi.HarSensor()
        if self.kind == 'thinlens':          # ThinLensCamera::update_camera_transforms (thinlens.cpp:190-213)
            rc = lib().har_thinlens_sensor(_fp(self.to_world.data), fov, fov_axis.encode(), self.near_clip, self.far_clip, self.aperture_radius, self.focus_distance_,
                                           f.width, f.height, f.crop_offset_[0], f.crop_offset_[1], f.crop_size_[0], f.crop_size_[1], f.rfilter, f.stddev, C.byref(s))
            if rc == 4:
                raise RuntimeError("thinlens: aperture_radius must be non-negative and finite")
            if rc == 5:
                raise RuntimeError("thinlens: focus_distance must be positive and finite")
        else:
            rc = lib().har_perspective_sensor(_fp(self.to_world.data), fov, fov_axis.encode(), self.near_clip, self.far_clip,
                                              f.width, f.height, f.crop_offset_[0], f.crop_offset_[1], f.crop_size_[0], f.crop_size_[1],
                                              f.rfilter, f.stddev, C.byref(s))
        s.rfilter_param1 = f.rf_param1
        s.sample_border = 1 if f.sample_border_ else 0
        if self.kind != 'thinlens':
            # perspective.cpp:147-150: the principal point, as a fraction of the film size
            s.principal_point_offset_x = float(self.props.get('principal_point_offset_x', 0.0)); s.principal_point_offset_y = float(self.props.get('principal_point_offset_y', 0.0))
        if rc == 2:
            raise RuntimeError("The 'fov_axis' parameter must be set to one of 'smaller', 'larger', 'diagonal', 'x', or 'y'!")
        if rc == 3:
            raise RuntimeError("The horizontal field of view must be in the range [0, 180]!")
        if rc:
            raise RuntimeError("invalid sensor parameters")
        self.har = s

    def x_fov(self):
        """the horizontal field of view in degrees: parse_fov (src/render/sensor.cpp:142-195) of the sensor's `fov` / `fov_axis` / `focal_length` at the film's aspect ratio --
        what PerspectiveCamera::traverse registers as 'x_fov' (perspective.cpp:157)"""
        w, h = self.m_film.width, self.m_film.height
        aspect = w / float(h)
        axis = str(self.props.get('fov_axis', 'x')).lower()
        if 'fov' in self.props:
            fov = float(self.props['fov'])
            if axis == 'smaller':
                axis = 'y' if aspect > 1 else 'x'
            elif axis == 'larger':
                axis = 'x' if aspect > 1 else 'y'
        else:
            fl = str(self.props.get('focal_length', '50mm'))
            fov = 2.0 * math.degrees(math.atan(math.sqrt(36 * 36 + 24 * 24) / (2.0 * float(fl[:-2] if fl.endswith('mm') else fl)))); axis = 'diagonal'
        if axis == 'x':
            return fov
        if axis == 'y':
            return math.degrees(2.0 * math.atan(math.tan(0.5 * math.radians(fov)) * aspect))
        width = 2.0 * math.tan(0.5 * math.radians(fov)) / math.sqrt(1.0 + 1.0 / (aspect * aspect))
        return math.degrees(2.0 * math.atan(width * 0.5))

    def film(self):
        return self.m_film

    def sampler(self):
        return self.m_sampler

    def sample_ray(self, time, sample1, sample2, sample3=None):
        """Sensor::sample_ray: sample2 is the film position in [0,1]^2, tensor [2, n]; sample3 the aperture sample of a thin lens, tensor [2, n] (None: the centre of the
        lens; pinhole cameras ignore it)."""
        torch = _torch(); dev = _device()
        p = torch.as_tensor(sample2, dtype=torch.float32, device=dev).reshape(2, -1).contiguous(); n = p.shape[1]
        a = _aperture_tensor(sample3, n) if self.kind == 'thinlens' else None
        o = torch.empty((3, n), dtype=torch.float32, device=dev); d = torch.empty_like(o); mt = torch.empty(n, dtype=torch.float32, device=dev)
        if a is None:
            check(lib().har_sensor_sample_ray(C.byref(self.har), n, _ptr(p[0]), _ptr(p[1]), _ptr(o), _ptr(d), _ptr(mt), _stream()))
        else:
            check(lib().har_sensor_sample_ray_aperture(C.byref(self.har), n, _ptr(p[0]), _ptr(p[1]), _ptr(a[0]), _ptr(a[1]), _ptr(o), _ptr(d), _ptr(mt), _stream()))
        return Ray3f(o, d, mt), torch.ones(n, device=dev)

    def sample_ray_host(self, sample2, sample3=None):
        """the same on the host (har_sensor_sample_ray_aperture_host; no GPU): sample2, sample3 = 2 x n numpy arrays -> (o 3 x n, d 3 x n, maxt n)"""
        p = np.ascontiguousarray(np.asarray(sample2, np.float32).reshape(2, -1)); n = p.shape[1]
        px = np.ascontiguousarray(p[0]); py = np.ascontiguousarray(p[1])
        ax, ay = _aperture_host(sample3, n)
        o = np.empty((3, n), np.float32); d = np.empty((3, n), np.float32); mt = np.empty(n, np.float32)
        check(lib().har_sensor_sample_ray_aperture_host(C.byref(self.har), n, _fp(px), _fp(py), ax if ax is None else _fp(ax), ay if ay is None else _fp(ay), _fp(o), _fp(d), _fp(mt)))
        return o, d, mt


def _aperture_tensor(sample3, n):
    """the aperture samples as a contiguous 2 x n device tensor, or None"""
    if sample3 is None:
        return None
    torch = _torch()
    a = torch.as_tensor(sample3, dtype=torch.float32, device=_device()).reshape(2, -1).contiguous()
    if a.shape[1] != n:
        raise RuntimeError("sample_ray(): sample3 (the aperture sample) must have as many entries as sample2")
    return a


def _aperture_host(sample3, n):
    if sample3 is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(sample3, np.float32).reshape(2, -1))
    if a.shape[1] != n:
        raise RuntimeError("sample_ray(): sample3 (the aperture sample) must have as many entries as sample2")
    return np.ascontiguousarray(a[0]), np.ascontiguousarray(a[1])


class BatchSensor(Sensor):
    """BatchSensor (src/sensors/batch.cpp): N child sensors share one film N times as wide as theirs; the x coordinate of a film position picks the child
    (batch.cpp:138-145).  `har` describes the wide film (size, filter) -- its camera part is unused; `children_har()` is the table har_integrator_set_batch_sensors takes."""

    def __init__(self, props):
        self.props = dict(props)
        self.kind = 'batch'
        # Sensor(props) (sensor.cpp:24-97) + props.objects() (batch.cpp:94-109): sensors, and shapes that carry one -- no shape of hip_ad_rgb does
        _check_props('batch', props, ('to_world', 'film', 'sampler', 'shutter_open', 'shutter_close'), children=('film', 'sampler', 'sensor', 'shape'),
                     slots={'film': ('film',), 'sampler': ('sampler',)}, slot_kind=())
        film = next((v for v in props.values() if isinstance(v, Film)), props.get('film'))
        sampler = next((v for v in props.values() if isinstance(v, Sampler)), props.get('sampler'))
        self.m_film = film if isinstance(film, Film) else Film(film)
        self.m_sampler = sampler if isinstance(sampler, Sampler) else Sampler(sampler)
        self.to_world = props.get('to_world', ScalarTransform4f())
        self.near_clip = 1e-2; self.far_clip = 1e4
        self.m_sensors = []; self.child_names = []
        for k, v in props.items():
            if isinstance(v, BatchSensor):
                raise RuntimeError("batch: a nested `batch` sensor (child \"%s\") is not implemented by hip_ad_rgb" % k)
            if isinstance(v, Sensor):
                # batch.cpp:277-279: the child's id, or sensor<i> for an unnamed one (anonymous XML children are `_arg_<n>` here)
                self.child_names.append("sensor%d" % len(self.m_sensors) if k.startswith('_arg_') else k)
                self.m_sensors.append(v)
            elif _object_kind(v) == 'shape':                  # batch.cpp:97-107
                raise RuntimeError("BatchSensor: shapes can only be specified as children if a sensor is associated with them!")
        n = len(self.m_sensors)
        if n == 0:                                               # batch.cpp:111-112
            raise RuntimeError("BatchSensor: at least one child sensor must be specified!")
        f = self.m_film
        if f.width // n * n != f.width:                          # batch.cpp:114-119
            raise RuntimeError("BatchSensor: the horizontal resolution (currently %u) must be divisible by the number of child sensors (%u)!" % (f.width, n))
        # the reference hands the children position samples of the crop-adjusted wide film and divides a crop window between them; refused rather than restated
        if f.crop_offset_ != (0, 0) or f.crop_size_ != (f.width, f.height):
            raise RuntimeError("batch: a crop window on the batch sensor's film is not implemented by hip_ad_rgb")
        if f.sample_border_:
            raise RuntimeError("batch: `sample_border` on the batch sensor's film is not implemented by hip_ad_rgb")
        for name, c in zip(self.child_names, self.m_sensors):
            cf = c.m_film
            if cf.crop_offset_ != (0, 0) or cf.crop_size_ != (cf.width, cf.height):
                raise RuntimeError("batch: a crop window on the film of child sensor \"%s\" is not implemented by hip_ad_rgb" % name)
            # batch.cpp:122-124: film()->set_size(sub_size, size.y) -- which resets the crop window to the whole film (film.cpp:82-88) -- then parameters_changed()
            cf.width = f.width // n; cf.height = f.height; cf.crop_size_ = (cf.width, cf.height); cf.crop_offset_ = (0, 0)
            c.update()
        self.update()

    def update(self):
        f = self.m_film
        s = _capi.HarSensor()
        if lib().har_perspective_sensor(_fp(ScalarTransform4f().data), 45.0, b'x', self.near_clip, self.far_clip, f.width, f.height, 0, 0, f.width, f.height,
                                        f.rfilter, f.stddev, C.byref(s)):
            raise RuntimeError("invalid film parameters of the batch sensor")
        s.rfilter_param1 = f.rf_param1
        s.sample_border = 0
        self.har = s

    def sensors(self):
        return list(self.m_sensors)

    def children_har(self):
        """the children's records as one ctypes array (har_integrator_set_batch_sensors / har_batch_sample_ray), taken anew on every call: params.update() re-lowers a child in place"""
        return (_capi.HarSensor * len(self.m_sensors))(*[c.har for c in self.m_sensors])

    def x_fov(self):
        raise RuntimeError("batch: the batch sensor has no field of view of its own; see its children")

    def needs_aperture_sample(self):
        """batch.cpp:121-125: as soon as ONE child needs an aperture sample, every lane of the batch draws one"""
        return any(c.needs_aperture_sample() for c in self.m_sensors)

    def focus_distance(self):
        raise RuntimeError("batch: the batch sensor has no focus distance of its own; see its children")

    def sample_ray(self, time, sample1, sample2, sample3=None):
        """BatchSensor::sample_ray (batch.cpp:132-159): sample2 is the position on the wide film in [0,1]^2, tensor [2, n]; sample3 the aperture sample that thin-lens
        children use."""
        torch = _torch(); dev = _device()
        p = torch.as_tensor(sample2, dtype=torch.float32, device=dev).reshape(2, -1).contiguous(); n = p.shape[1]
        a = _aperture_tensor(sample3, n) if self.needs_aperture_sample() else None
        o = torch.empty((3, n), dtype=torch.float32, device=dev); d = torch.empty_like(o); mt = torch.empty(n, dtype=torch.float32, device=dev)
        ch = self.children_har()
        if a is None:
            check(lib().har_batch_sample_ray(ch, len(ch), n, _ptr(p[0]), _ptr(p[1]), _ptr(o), _ptr(d), _ptr(mt), _stream()))
        else:
            check(lib().har_batch_sample_ray_aperture(ch, len(ch), n, _ptr(p[0]), _ptr(p[1]), _ptr(a[0]), _ptr(a[1]), _ptr(o), _ptr(d), _ptr(mt), _stream()))
        return Ray3f(o, d, mt), torch.ones(n, device=dev)

    def sample_ray_host(self, sample2, sample3=None):
        """the same on the host (har_batch_sample_ray_aperture_host; no GPU): sample2, sample3 = 2 x n numpy arrays -> (o 3 x n, d 3 x n, maxt n)"""
        p = np.ascontiguousarray(np.asarray(sample2, np.float32).reshape(2, -1)); n = p.shape[1]
        px = np.ascontiguousarray(p[0]); py = np.ascontiguousarray(p[1])
        ax, ay = _aperture_host(sample3, n)
        o = np.empty((3, n), np.float32); d = np.empty((3, n), np.float32); mt = np.empty(n, np.float32)
        ch = self.children_har()
        if ax is None:
            check(lib().har_batch_sample_ray_host(ch, len(ch), n, _fp(px), _fp(py), _fp(o), _fp(d), _fp(mt)))
        else:
            check(lib().har_batch_sample_ray_aperture_host(ch, len(ch), n, _fp(px), _fp(py), _fp(ax), _fp(ay), _fp(o), _fp(d), _fp(mt)))
        return o, d, mt


def _refuse_batch(sensor, what):
    if getattr(sensor, 'kind', None) == 'batch':
        raise RuntimeError("batch: the batch sensor is not implemented by %s in hip_ad_rgb; render it with mi.render / Integrator.render on one device" % what)


# include/mitsuba/render/ior.h:24-48
_IOR = {"vacuum": 1.0, "helium": 1.000036, "hydrogen": 1.000132, "air": 1.000277, "carbon dioxide": 1.00045, "water": 1.3330,
        "acetone": 1.36, "ethanol": 1.361, "carbon tetrachloride": 1.461, "glycerol": 1.4729, "benzene": 1.501, "silicone oil": 1.52045,
        "bromine": 1.661, "water ice": 1.31, "fused quartz": 1.458, "pyrex": 1.470, "acrylic glass": 1.49, "polypropylene": 1.49,
        "bk7": 1.5046, "sodium chloride": 1.544, "amber": 1.55, "pet": 1.5750, "diamond": 2.419}


def _lookup_ior(props, name, default):
    v = props.get(name, default)
    if isinstance(v, str):
        if v.lower() not in _IOR:
            raise RuntimeError("Could not find a material named \"%s\"" % v)
        return float(_IOR[v.lower()])
    return float(v)


def _rgb_value(v, default, bounded=True, uniform=None):
    """Properties colour value: float, list or {'type': 'rgb', 'value': ...} -> float32[3].  `uniform` = the quantity's name where the reference itself refuses a
    spatially varying texture (point.cpp:80-81, spot.cpp:96-97, directional.cpp:84-85, constant.cpp:60-61): same words"""
    if v is None:
        v = default
    if isinstance(v, dict):
        if v.get('type') != 'rgb' and uniform:
            raise RuntimeError("Expected a non-spatially varying %s spectra!" % uniform)
        if v.get('type') != 'rgb':
            raise RuntimeError("only `rgb` values are implemented for this parameter")
        v = v['value']
    out = _f32([v] * 3 if np.isscalar(v) else list(v))
    if bounded and (np.any(out < 0) or np.any(out > 1)):
        raise RuntimeError("Invalid RGB reflectance value %s, must be in the range [0, 1]!" % out)
    return out


# the properties each BSDF plugin queries (src/bsdfs/*.cpp constructors; MicrofacetDistribution(props), microfacet.h:103-144)
_BSDF_PROPS = {'diffuse': ('reflectance',),
               'dielectric': ('int_ior', 'ext_ior', 'specular_reflectance', 'specular_transmittance'),
               'thindielectric': ('int_ior', 'ext_ior', 'specular_reflectance', 'specular_transmittance'),
               'conductor': ('material', 'eta', 'k', 'specular_reflectance'),
               'plastic': ('int_ior', 'ext_ior', 'diffuse_reflectance', 'specular_reflectance', 'nonlinear'),
               'roughconductor': ('material', 'eta', 'k', 'distribution', 'sample_visible', 'alpha', 'alpha_u', 'alpha_v', 'specular_reflectance'),
               'roughplastic': ('distribution', 'sample_visible', 'alpha', 'alpha_u', 'alpha_v', 'int_ior', 'ext_ior', 'diffuse_reflectance', 'specular_reflectance', 'nonlinear')}
# BitmapTexture(props) (src/textures/bitmap.cpp:175-260); `raw` only silences a range warning for float data in RGB variants, `accel` picks Dr.Jit's texture
# hardware path on CUDA (no effect on values), `format` = the storage type of the texels ("auto" / "variant" / "fp16": this path keeps float32)
_BITMAP_PROPS = ('filename', 'bitmap', 'data', 'to_uv', 'raw', 'accel', 'filter_type', 'wrap_mode', 'format')
BSDF_TYPES = {'diffuse': 0, 'dielectric': 1, 'roughconductor': 2, 'roughplastic': 3, 'conductor': 4, 'plastic': 5, 'blendbsdf': 6, 'mask': 7, 'normalmap': 8, 'bumpmap': 9, 'thindielectric': 10}
_NESTING_BSDFS = ('blendbsdf', 'mask', 'normalmap', 'bumpmap')          # records that name nested records: built by the plugin factory
_MONO_TEX_BSDFS = ('blendbsdf', 'mask', 'bumpmap', 'alphamap')          # records whose bitmap may have ONE channel (stored three times; `weight_channels`); 'alphamap': a roughconductor's roughness map (_AlphaMap)
_THIN_PARAMS = ('thin_ior', 'thin_r')          # `eta` and `specular_reflectance` of a `thindielectric`: differentiable in the reference's traverse(), and `prb` gives zero for them (the model's eval() is zero: prb.py:288-297)
_NOGRAD_PARAMS = ('ior', 'scale')          # non-colour parameters that are updatable and carry no gradient (ParamFlags::NonDifferentiable)
_WEIGHTED_BSDFS = ('blendbsdf', 'mask')          # records whose slot 0 is a scalar texture (Texture::eval_1): the blend weight, the mask opacity
_LUMINANCE = (0.212671, 0.715160, 0.072169)          # luminance() of an RGB colour (include/mitsuba/core/spectrum.h:439-442)
# (parameter name of slot 0, default), (parameter name of slot 1, default)
_BSDF_SLOTS = {'diffuse': (('reflectance', 0.5), None), 'dielectric': (('specular_reflectance', 1.0), ('specular_transmittance', 1.0)),
               'roughconductor': (('specular_reflectance', 1.0), None), 'roughplastic': (('diffuse_reflectance', 0.5), ('specular_reflectance', 1.0)),
               'conductor': (('specular_reflectance', 1.0), None), 'plastic': (('diffuse_reflectance', 0.5), ('specular_reflectance', 1.0)),
               # HAR_BSDF_THINDIELECTRIC: slot 0 is the TRANSMITTANCE (it may be a bitmap: stained glass), slot 1 the reflectance (a constant)
               'thindielectric': (('specular_transmittance', 1.0), ('specular_reflectance', 1.0))}


def _bitmap_from_props(refl):
    """BitmapTexture(props) -> (H x W x 3 float32 texels, HarTexture::mode, to_uv rows or None)"""
    # BitmapTexture (src/textures/bitmap.cpp:175-260): texels from a tensor (`data`), a Bitmap object (`bitmap`) or a file (`filename`:
    # OpenEXR / PFM, read by the C++ host library).  Float data is linear; in RGB variants `raw` only silences the [0, 1] range warning.
    if sum(k in refl for k in ('data', 'bitmap', 'filename')) != 1:
        raise RuntimeError("bitmap: exactly one of 'filename', 'bitmap' and 'data' must be specified")
    # filter_type / wrap_mode (bitmap.cpp:182-206) -> HarTexture::mode
    ft = str(refl.get('filter_type', 'bilinear')); wm = str(refl.get('wrap_mode', 'repeat'))
    if ft not in ('nearest', 'bilinear'):
        raise RuntimeError("Invalid filter type \"%s\", must be one of: \"nearest\", or \"bilinear\"!" % ft)
    if wm not in ('repeat', 'mirror', 'clamp'):
        raise RuntimeError("Invalid wrap mode \"%s\", must be one of: \"repeat\", \"mirror\", or \"clamp\"!" % wm)
    tex_mode = (1 if ft == 'nearest' else 0) | {'repeat': 0, 'mirror': 2, 'clamp': 4}[wm]
    _check_props('bitmap', refl, _BITMAP_PROPS, unsupported=(('format', 'auto'),), free_children=False)
    # to_uv (bitmap.cpp:175): uv = m_transform * si.uv before every lookup (:565,792,831,847) -> HarTexture::to_uv, row-major 2 x 3
    tex_to_uv = None
    if 'to_uv' in refl:
        tuv = refl['to_uv']
        if isinstance(tuv, ScalarTransform4f):        # Properties::get<AffineTransform3f> of a stored 4 x 4 (an XML <transform>): Transform::extract (transform.h:441-456)
            m4 = tuv.matrix; tuv = ScalarTransform3f([[m4[0, 0], m4[0, 1], m4[0, 3]], [m4[1, 0], m4[1, 1], m4[1, 3]], [0.0, 0.0, 1.0]])
        if not isinstance(tuv, ScalarTransform3f):
            raise RuntimeError("bitmap: 'to_uv' must be a ScalarTransform3f")
        if abs(float(np.linalg.det(tuv.matrix[:2, :2].astype(np.float64)))) == 0.0:
            raise RuntimeError("bitmap: 'to_uv' is singular")
        tex_to_uv = tuv.rows_2x3()
    if 'data' in refl:
        t = refl['data']
        if hasattr(t, 'detach'):
            t = t.detach().cpu().numpy()
    else:
        b = refl['bitmap'] if 'bitmap' in refl else Bitmap(refl['filename'])
        if not isinstance(b, Bitmap):
            raise RuntimeError("Property \"bitmap\" must be a Bitmap instance.")
        t = b.data
    t = _f32(t)
    if t.ndim == 2:
        t = t[:, :, None]
    if t.ndim != 3 or t.shape[2] not in (1, 3, 4):
        raise RuntimeError("Bitmap raw tensor has dimension %d, expected 3 (H x W x {1, 3, 4})" % t.ndim)
    t = np.repeat(t, 3, axis=2) if t.shape[2] == 1 else t[:, :, :3]
    return np.ascontiguousarray(t, np.float32), tex_mode, tex_to_uv


def _mesh_attribute_from_props(refl):
    """MeshAttribute(props) (src/textures/mesh_attribute.cpp:79-86) -> (name, scale).  The attribute itself belongs to the SHAPE that is hit (si.shape->eval_attribute):
    it is bound when a shape that carries the BSDF joins a scene (Scene._bind_attributes)"""
    _check_props('mesh_attribute', refl, ('name', 'scale'), free_children=False)
    if 'name' not in refl:
        raise RuntimeError("Property \"name\" has not been specified!")
    name = str(refl['name'])
    if "vertex_" not in name and "face_" not in name:
        raise RuntimeError("Invalid mesh attribute name: must be start with either \"vertex_\" or \"face_\" but was \"%s\"." % name)
    scale = float(np.float32(refl.get('scale', 1.0)))
    if not math.isfinite(scale):
        raise RuntimeError("mesh_attribute: `scale` must be finite")
    return name, scale


class _RecordFlags(int):
    """BlendBSDF.flags: an int (the record's flag word, as on every BSDF) that answers BSDF::flags() / BSDF::flags(i) when called"""

    def __new__(cls, value, owner):
        obj = int.__new__(cls, value); obj._owner = owner
        return obj

    def __call__(self, index=None):
        return self._owner._lobe_flags(index)


class _AlphaMap:
    """`alpha` / `alpha_u` / `alpha_v` of a `roughconductor` given as a `bitmap` (get_unbounded_texture, roughconductor.cpp:195-198; read by Texture::eval_1): a texture of
    the scene that no colour slot names.  It carries what the parameter tables read of a textured slot (`texture`, `tex_mode`, `tex_to_uv`, `tex_index`, `slot0_name`,
    `weight_channels`), so '<bsdf>.<name>.data' / '.to_uv' are shown, updated and differentiated like any other bitmap's"""
    kind = 'alphamap'; attr = None

    def __init__(self, name, props):
        src = props['data'] if 'data' in props else (props['bitmap'].data if isinstance(props.get('bitmap'), Bitmap) else Bitmap(props['filename']).data if 'filename' in props else None)
        ch = None if src is None else (1 if len(tuple(src.shape)) == 2 else int(src.shape[2]))
        if ch is not None and ch not in (1, 3):
            raise RuntimeError("roughconductor: the `%s` bitmap has %d channels, expected 1 or 3" % (name, ch))
        self.texture, self.tex_mode, self.tex_to_uv = _bitmap_from_props(props)
        self.slot0_name = name; self.weight_channels = ch; self.tex_index = None; self.owner = None

    def mean(self):
        """the mean of Texture::eval_1 over the texels: the constant the record carries next to the map (nothing shades with it)"""
        t = np.asarray(self.texture, np.float64)
        return float(t[:, :, 0].mean() if self.weight_channels == 1 else (t * np.asarray(_LUMINANCE)).sum(axis=2).mean())


class BSDF:
    """diffuse / dielectric / conductor / plastic / roughconductor / roughplastic (src/bsdfs/*.cpp), optionally wrapped by `twosided`.
    Colour parameters live in two slots (include/hip_ad_rgb.h HarBSDF); slot 0 may be a raw `bitmap`, and so may the roughness of a `roughconductor`."""

    def _alpha_prop(self, props, name):
        """`alpha` / `alpha_u` / `alpha_v` of a rough model: a float, or -- `roughconductor` only -- a `bitmap` of 1 or 3 channels, kept in self.alpha_maps[name]"""
        v = props.get(name, 0.1)
        if not isinstance(v, dict):
            return float(v)
        if self.kind != 'roughconductor':
            raise RuntimeError("roughplastic: `%s` is a float (roughplastic.cpp:210: a Float member); an alpha bitmap is supported on `roughconductor`" % name)
        if v.get('type') == 'mesh_attribute':
            raise RuntimeError("roughconductor: a `mesh_attribute` texture as `%s` is not supported in hip_ad_rgb (a float or a `bitmap` is)" % name)
        if v.get('type') != 'bitmap':
            raise RuntimeError("roughconductor: `%s` is a float or a `bitmap` texture in hip_ad_rgb (got \"%s\")" % (name, v.get('type')))
        am = _AlphaMap(name, v); am.owner = self
        self.alpha_maps[name] = am
        return am.mean()

    def __init__(self, props=None, id=None):
        props = props or {}
        self.id = id
        self.kind = props.get('type', 'diffuse')
        if self.kind in _NESTING_BSDFS:
            raise RuntimeError("%s: built by the plugin factory (mi.load_dict), which resolves its nested BSDFs" % self.kind)
        if self.kind not in BSDF_TYPES:
            raise RuntimeError("Plugin \"%s\" not found for variant hip_ad_rgb" % self.kind)
        _check_props(self.kind, props, _BSDF_PROPS[self.kind], free_children=False)
        (name0, def0), slot1 = _BSDF_SLOTS[self.kind]
        self.slot0_name = name0; self.slot1_name = slot1[0] if slot1 else None
        refl = props.get(name0, {'type': 'rgb', 'value': [def0] * 3})
        # thindielectric.cpp:119-122: the two colours are null members when the property is absent -- traverse() shows them only when they were given
        self.given = tuple(n for n in (name0, self.slot1_name) if n is not None and n in props) if self.kind == 'thindielectric' else None
        if self.kind == 'thindielectric':
            if isinstance(refl, dict) and refl.get('type') == 'mesh_attribute':
                raise RuntimeError("thindielectric: a `mesh_attribute` texture as `specular_transmittance` is not supported in hip_ad_rgb (an rgb value or a `bitmap` is)")
            r1 = props.get(self.slot1_name)
            if isinstance(r1, dict) and r1.get('type') != 'rgb':
                raise RuntimeError("thindielectric: `specular_reflectance` is a `%s`: slot 1 is constant in this variant (an rgb value; `specular_transmittance` may be a `bitmap`)" % r1.get('type'))
        if isinstance(refl, (int, float)):
            refl = {'type': 'rgb', 'value': [refl] * 3}
        self.texture = None; self.tex_mode = 0; self.tex_to_uv = None
        self.attr = None; self.attr_mesh = None          # slot 0 is a `mesh_attribute`: (name, scale), and the scene's mesh it was bound to
        if refl['type'] == 'rgb':
            self.value = _rgb_value(refl, def0)
        elif refl['type'] == 'bitmap':
            self.texture, self.tex_mode, self.tex_to_uv = _bitmap_from_props(refl)
            self.value = _f32([0.5, 0.5, 0.5])
        elif refl['type'] == 'mesh_attribute':
            self.attr = _mesh_attribute_from_props(refl)
            self.value = _f32([0.5, 0.5, 0.5])
        else:
            raise RuntimeError("Plugin \"%s\" not found for variant hip_ad_rgb (textures: rgb, bitmap, mesh_attribute)" % refl['type'])
        self.value2 = _rgb_value(props.get(slot1[0]), slot1[1]) if slot1 else _f32([0, 0, 0])
        self.flags = 0; self.alpha_u = self.alpha_v = 0.1; self.eta = 1.0; self.anisotropic = False
        self.alpha_maps = {}          # roughconductor: 'alpha', or 'alpha_u' / 'alpha_v', -> _AlphaMap where that roughness is a bitmap
        self.eta_c = _f32([0, 0, 0]); self.k_c = _f32([1, 1, 1]); self.back = None
        if self.kind in ('roughconductor', 'roughplastic'):          # MicrofacetDistribution(props), microfacet.h:103-144
            distr = str(props.get('distribution', 'beckmann')).lower()
            if distr not in ('beckmann', 'ggx'):
                raise RuntimeError("Specified an invalid distribution \"%s\", must be \"beckmann\" or \"ggx\"!" % distr)
            if distr == 'ggx':
                self.flags |= 2
            if props.get('sample_visible', True):
                self.flags |= 4
            if 'alpha_u' in props or 'alpha_v' in props:
                if not ('alpha_u' in props and 'alpha_v' in props):
                    raise RuntimeError("Microfacet model: both 'alpha_u' and 'alpha_v' must be specified.")
                if 'alpha' in props:
                    raise RuntimeError("Microfacet model: please specifyeither 'alpha' or 'alpha_u'/'alpha_v'.")
                self.alpha_u = self._alpha_prop(props, 'alpha_u'); self.alpha_v = self._alpha_prop(props, 'alpha_v'); self.anisotropic = True
            else:
                self.alpha_u = self.alpha_v = self._alpha_prop(props, 'alpha')
            if self.alpha_maps:          # HAR_BSDF_ALPHA_TEX, and HAR_BSDF_ALPHA_MONO_U / _V for a one-channel map on that axis
                mu = self.alpha_maps.get('alpha', self.alpha_maps.get('alpha_u')); mv = self.alpha_maps.get('alpha', self.alpha_maps.get('alpha_v'))
                self.flags |= 256 | (512 if mu is not None and mu.weight_channels == 1 else 0) | (1024 if mv is not None and mv.weight_channels == 1 else 0)
        if self.kind in ('roughconductor', 'conductor'):             # roughconductor.cpp:163-172, conductor.cpp:228-237
            if props.get('material', 'none') != 'none':
                if 'eta' in props:
                    raise RuntimeError("Should specify either (eta, k) or material, not both.")
                raise RuntimeError("%s: `material` presets need the spectral IOR data files, give (eta, k) instead" % self.kind)
            self.eta_c = _rgb_value(props.get('eta'), 0.0, bounded=False); self.k_c = _rgb_value(props.get('k'), 1.0, bounded=False)
        if self.kind in ('dielectric', 'thindielectric', 'roughplastic', 'plastic'):
            int_ior = _lookup_ior(props, 'int_ior', 'bk7' if self.kind in ('dielectric', 'thindielectric') else 'polypropylene')
            ext_ior = _lookup_ior(props, 'ext_ior', 'air')
            if int_ior < 0 or ext_ior < 0 or (self.kind == 'roughplastic' and int_ior == ext_ior):
                raise RuntimeError("The interior and exterior indices of refraction must be positive" + (" and differ!" if self.kind == 'roughplastic' else "!"))
            self.eta = float(np.float32(int_ior) / np.float32(ext_ior))
            if self.kind == 'roughplastic' and self.alpha_u != self.alpha_v:
                raise RuntimeError("The 'roughplastic' plugin currently does not support anisotropic microfacet distributions!")
            if self.kind in ('roughplastic', 'plastic') and props.get('nonlinear', False):
                self.flags |= 8
        self.scene = None; self.index = None

    def _bind(self):
        if self.scene is None:          # stand-alone BSDF: private scene holding just this plugin
            Scene({'_bsdf': self})
        return self.scene._handle(), self.index

    def _prep(self, si_wi, si_uv, n):
        torch = _torch(); dev = _device()
        wi = torch.as_tensor(si_wi, dtype=torch.float32, device=dev).reshape(3, -1)
        wi = wi.expand(3, n).contiguous() if wi.shape[1] != n else wi.contiguous()
        uv = torch.zeros((2, n), dtype=torch.float32, device=dev) if si_uv is None else torch.as_tensor(si_uv, dtype=torch.float32, device=dev).reshape(2, -1).contiguous()
        return wi, uv

    def _eval(self, which, ctx, si, wo, active):
        torch = _torch(); dev = _device(); h, idx = self._bind()
        wo = torch.as_tensor(wo, dtype=torch.float32, device=dev).reshape(3, -1).contiguous(); n = wo.shape[1]
        wi, uv = self._prep(si.wi, getattr(si, 'uv', None), n)
        a = _mask(active, n); c = _ctx(ctx)
        val = torch.empty((3, n), dtype=torch.float32, device=dev) if which != 'pdf' else None
        pdf = torch.empty(n, dtype=torch.float32, device=dev) if which != 'eval' else None
        if self._reads_interaction():
            # a `bumpmap` (also under a `twosided`): its frame reads si.n, si.sh_frame, si.dp_du and si.dp_dv (bumpmap.cpp:224-253) -- the entries that carry them
            geom = self._geom(si, n)
            check(lib().har_bsdf_eval_pdf_si(h, idx, c, n, _ptr(wi), _ptr(uv), _ptr(wo), _ptr(geom), _ptr(a), _ptr(val), _ptr(pdf), _stream()))
        elif which == 'eval_pdf':
            check(lib().har_bsdf_eval_pdf(h, idx, c, n, _ptr(wi), _ptr(uv), _ptr(wo), _ptr(a), _ptr(val), _ptr(pdf), _stream()))
        elif which == 'eval':
            check(lib().har_bsdf_eval(h, idx, c, n, _ptr(wi), _ptr(uv), _ptr(wo), _ptr(a), _ptr(val), _stream()))
        else:
            check(lib().har_bsdf_pdf(h, idx, c, n, _ptr(wi), _ptr(uv), _ptr(wo), _ptr(a), _ptr(pdf), _stream()))
        return val, pdf

    def _reads_interaction(self):
        return self.kind == 'bumpmap'

    @staticmethod
    def _geom(si, n):
        """the 18 x n rows a bumpmap's frame reads: si.n, si.sh_frame.n / .s / .t, si.dp_du, si.dp_dv"""
        torch = _torch(); dev = _device()
        frame = getattr(si, 'sh_frame', None)
        rows = []
        for name, v in (("n", getattr(si, 'n', None)), ("sh_frame.n", getattr(frame, 'n', None)), ("sh_frame.s", getattr(frame, 's', None)),
                        ("sh_frame.t", getattr(frame, 't', None)), ("dp_du", getattr(si, 'dp_du', None)), ("dp_dv", getattr(si, 'dp_dv', None))):
            if v is None:
                raise RuntimeError("bumpmap: BSDF::eval / pdf / sample read si.%s (bumpmap.cpp:224-253), which this interaction does not carry" % name)
            v = torch.as_tensor(v, dtype=torch.float32, device=dev).reshape(3, -1)
            rows.append(v.expand(3, n) if v.shape[1] != n else v)
        return torch.cat(rows, 0).contiguous()

    def eval_pdf(self, ctx, si, wo, active=True):
        """BSDF::eval_pdf(ctx, si, wo, active) (bsdf.h:431-465)"""
        return self._eval('eval_pdf', ctx, si, wo, active)

    def eval(self, ctx, si, wo, active=True):
        return self._eval('eval', ctx, si, wo, active)[0]

    def pdf(self, ctx, si, wo, active=True):
        return self._eval('pdf', ctx, si, wo, active)[1]

    def sample(self, ctx, si, sample1, sample2, active=True):
        """BSDF::sample(ctx, si, sample1, sample2, active) -> (BSDFSample3f, weight) (bsdf.h:322-373)"""
        torch = _torch(); dev = _device(); h, idx = self._bind()
        s2 = torch.as_tensor(sample2, dtype=torch.float32, device=dev).reshape(2, -1).contiguous(); n = s2.shape[1]
        wi, uv = self._prep(si.wi, getattr(si, 'uv', None), n)
        wo = torch.empty((3, n), dtype=torch.float32, device=dev); pdf = torch.empty(n, dtype=torch.float32, device=dev); w = torch.empty_like(wo)
        s1 = torch.as_tensor(sample1, dtype=torch.float32, device=dev).reshape(-1)
        s1 = (s1.expand(n) if s1.numel() != n else s1).contiguous()
        eta = torch.empty(n, dtype=torch.float32, device=dev)
        st = torch.empty(n, dtype=torch.int32, device=dev); sc = torch.empty(n, dtype=torch.int32, device=dev)
        a = _mask(active, n)
        if self._reads_interaction():
            geom = self._geom(si, n)
            check(lib().har_bsdf_sample_si(h, idx, _ctx(ctx), n, _ptr(wi), _ptr(uv), _ptr(s1), _ptr(s2), _ptr(geom), _ptr(a), _ptr(wo), _ptr(pdf), _ptr(w), _ptr(eta), _ptr(st), _ptr(sc), _stream()))
        else:
            check(lib().har_bsdf_sample(h, idx, _ctx(ctx), n, _ptr(wi), _ptr(uv), _ptr(s1), _ptr(s2), _ptr(a), _ptr(wo), _ptr(pdf), _ptr(w), _ptr(eta), _ptr(st), _ptr(sc), _stream()))
        bs = type("BSDFSample3f", (), dict(wo=wo, pdf=pdf, eta=eta, sampled_type=st, sampled_component=sc, delta=(st & BSDFFlags.Delta) != 0))()
        return bs, w

    def _own_lobes(self):
        """BSDFFlags of the components of this plugin without a `twosided` wrapper (the constructors of src/bsdfs/*.cpp)"""
        F = BSDFFlags; fs = F.FrontSide
        return {'diffuse': [F.DiffuseReflection | fs], 'dielectric': [F.DeltaReflection | fs | F.BackSide, F.DeltaTransmission | fs | F.BackSide | F.NonSymmetric],
                'thindielectric': [F.DeltaReflection | fs | F.BackSide, F.Null | fs | F.BackSide],          # thindielectric.cpp:124-127
                # (Anisotropic: m_alpha_u != m_alpha_v compares the texture OBJECTS, roughconductor.cpp:205 -- with a roughness map, whether the two were given separately)
                'roughconductor': [F.GlossyReflection | fs | (F.Anisotropic if (self.anisotropic if getattr(self, 'alpha_maps', None) else self.alpha_u != self.alpha_v) else 0)],
                'roughplastic': [F.GlossyReflection | fs, F.DiffuseReflection | fs], 'conductor': [F.DeltaReflection | fs], 'plastic': [F.DeltaReflection | fs, F.DiffuseReflection | fs]}[self.kind]

    def _lobe_flags(self, index=None):
        """BSDF::flags() / BSDF::flags(i): the union of the lobes' BSDFFlags, or those of component i (twosided.cpp:86-99: the front BSDF's lobes on the front side, then the back's
        on the back side)"""
        lobes = self._own_lobes()
        if int(self.flags) & 1:
            back = self.back._own_lobes() if self.back is not None else lobes
            side = BSDFFlags.FrontSide | BSDFFlags.BackSide
            lobes = [(c & ~side) | BSDFFlags.FrontSide for c in lobes] + [(c & ~side) | BSDFFlags.BackSide for c in back]
        if index is None:
            out = 0
            for c in lobes:
                out |= c
            return out
        return lobes[index]

    def component_count(self):
        """BSDF::component_count(): the lobes of this plugin (twosided: the front BSDF's, then the back's, twosided.cpp:86-99; blendbsdf: the two nested BSDFs')"""
        n = len(self._own_lobes())
        if self.flags & 1:
            return n + (len(self.back._own_lobes()) if self.back is not None else n)
        return n


class BlendBSDF(BSDF):
    """BlendBSDF (src/bsdfs/blendbsdf.cpp:80-100): a BSDF record whose colour slot 0 is the `weight` (a float, or a raw bitmap of 1 or 3 channels) and which names two nested
    BSDFs; these become records of their own (Scene._add_bsdf)."""

    _plugin = 'blendbsdf'; _weight_name = 'weight'

    def __init__(self, weight, nested, id=None):
        self.id = id; self.kind = self._plugin; self.slot0_name = self._weight_name; self.slot1_name = None
        self.texture = None; self.tex_mode = 0; self.tex_to_uv = None; self.weight_channels = 0
        self.attr = None; self.attr_mesh = None
        if isinstance(weight, (int, float)) and not isinstance(weight, bool):
            self.value = _f32([float(weight)] * 3)
        elif isinstance(weight, dict) and weight.get('type') == 'mesh_attribute':
            # Texture::eval_1 of a mesh attribute (Mesh::eval_attribute_1, mesh.cpp:2619-2624): the value of a one-channel attribute, 0 for any other
            self.attr = _mesh_attribute_from_props(weight); self.weight_channels = 1
            self.value = _f32([0.5, 0.5, 0.5])
        elif isinstance(weight, dict) and weight.get('type') == 'bitmap':
            self.texture, self.tex_mode, self.tex_to_uv = _bitmap_from_props(weight)
            src = weight['data'] if 'data' in weight else (weight['bitmap'].data if isinstance(weight.get('bitmap'), Bitmap) else Bitmap(weight['filename']).data)
            ch = 1 if len(tuple(src.shape)) == 2 else int(src.shape[2])
            if ch not in (1, 3):
                raise RuntimeError("%s: the `%s` bitmap has %d channels, expected 1 or 3" % (self._plugin, self._weight_name, ch))
            self.weight_channels = ch
            self.value = _f32([0.5, 0.5, 0.5])
        else:
            raise RuntimeError("%s: `%s` is a float, a `bitmap` or a `mesh_attribute` texture" % (self._plugin, self._weight_name))
        self.value2 = _f32([0, 0, 0]); self.flags = 16 if self.weight_channels == 1 else 0          # (16: slot 0 is a one-channel bitmap, read channel 0)
        self.alpha_u = self.alpha_v = 0.1; self.eta = 1.0; self.anisotropic = False
        self.eta_c = _f32([0, 0, 0]); self.k_c = _f32([1, 1, 1]); self.back = None
        self.scene = None; self.index = None
        self.nested = list(nested)
        for k, c in enumerate(self.nested if self._plugin == 'blendbsdf' else ()):
            if getattr(c, 'blend_parent', None) is None and c.scene is None:
                c.blend_parent = (self, k)        # NAMES its parameters '<blend>.bsdf_<k>.*' (BlendBSDF::traverse, blendbsdf.cpp:102-106); what is refused for a nested record is decided from the scene's records, Scene._blend_nested

    def _own_lobes(self):
        """the nested BSDFs' components in order (blendbsdf.cpp:94-97)"""
        return self.nested[0]._own_lobes() + self.nested[1]._own_lobes()

    # the record's flag word (HarBSDF::flags: twosided, GGX, ...) wherever it is read or written, BSDF::flags() / BSDF::flags(i) when called
    @property
    def flags(self):
        return _RecordFlags(self._flags, self)

    @flags.setter
    def flags(self, value):
        self._flags = int(value)


class MaskBSDF(BlendBSDF):
    """MaskBSDF (src/bsdfs/mask.cpp:93-119): a BSDF record whose colour slot 0 is the `opacity` (a float, or a raw bitmap of 1 or 3 channels) and which names ONE nested
    BSDF -- a plain model, or a `twosided` over one or two of them; it becomes a record of its own (Scene._add_bsdf)."""
    _plugin = 'mask'; _weight_name = 'opacity'

    def __init__(self, opacity, nested, id=None):
        BlendBSDF.__init__(self, opacity, [nested], id=id)
        if getattr(nested, 'mask_parent', None) is None and nested.scene is None:
            nested.mask_parent = self          # NAMES its parameters '<mask>.nested_bsdf.*' (MaskBSDF::traverse, mask.cpp:116-119): Scene._bsdf_key_base

    def _own_lobes(self):
        """the nested BSDF's components -- those of its `twosided`, if it is one --, then the null lobe at the last index (mask.cpp:107-113)"""
        n = self.nested[0]
        lobes = [n._lobe_flags(i) for i in range(n.component_count())]
        return lobes + [BSDFFlags.Null | BSDFFlags.FrontSide | BSDFFlags.BackSide]


def _mk_mask(props, named, key):
    """the `mask` plugin: `opacity` (default 0.5) and exactly one nested BSDF under a free name (mask.cpp:93-105)"""
    _check_props('mask', props, ('opacity',), children=('bsdf',))
    nested = None
    for k, v in props.items():
        if k in ('type', 'id', 'opacity'):
            continue
        obj = _resolve(v, named, k) if isinstance(v, dict) else v
        if isinstance(obj, BSDF):
            if nested is not None:
                raise RuntimeError("Cannot specify more than one child BSDF")
            nested = obj
    if nested is None:
        raise RuntimeError("Child BSDF not specified")
    if nested.kind in _NESTING_BSDFS or (nested.back is not None and nested.back.kind in _NESTING_BSDFS):
        raise RuntimeError("mask: a nested `%s` is not supported in hip_ad_rgb (nested BSDFs are plain BSDF models, or `twosided` over them)"
                           % (nested.kind if nested.kind in _NESTING_BSDFS else nested.back.kind))
    return MaskBSDF(props.get('opacity', 0.5), nested, id=key)


class NormalMapBSDF(BSDF):
    """NormalMap (src/bsdfs/normalmap.cpp:100-132): a BSDF record whose colour slot 0 is the `normalmap` texture -- an `rgb` colour or a three-channel raw `bitmap`, read by
    Texture::eval_3 -- and which names ONE nested BSDF: a plain model, or a `twosided` over one or two of them; it becomes a record of its own (Scene._add_bsdf).
    flags: 64 = flip_invalid_normals, 128 = use_shadowing_function (HAR_BSDF_NM_FLIP / _SHADOW), 1 = wrapped by a `twosided`."""

    def __init__(self, normalmap, nested, flip_invalid_normals=True, use_shadowing_function=True, id=None):
        self.id = id; self.kind = 'normalmap'; self.slot0_name = 'normalmap'; self.slot1_name = None
        self.texture = None; self.tex_mode = 0; self.tex_to_uv = None
        self.attr = None; self.attr_mesh = None
        if isinstance(normalmap, dict) and normalmap.get('type') == 'rgb':
            self.value = _rgb_value(normalmap, 0.5, bounded=False)
        elif isinstance(normalmap, dict) and normalmap.get('type') == 'bitmap':
            src = normalmap['data'] if 'data' in normalmap else (normalmap['bitmap'].data if isinstance(normalmap.get('bitmap'), Bitmap) else Bitmap(normalmap['filename']).data)
            ch = 1 if len(tuple(src.shape)) == 2 else int(src.shape[2])
            if ch != 3:
                raise RuntimeError("normalmap: the `normalmap` bitmap has %d channel%s, expected 3 (a one-channel bitmap is not a normal map)" % (ch, "" if ch == 1 else "s"))
            self.texture, self.tex_mode, self.tex_to_uv = _bitmap_from_props(normalmap)
            self.value = _f32([0.5, 0.5, 1.0])
        else:
            raise RuntimeError("normalmap: `normalmap` is an `rgb` colour or a three-channel `bitmap` texture")
        self.value2 = _f32([0, 0, 0]); self.flags = (64 if flip_invalid_normals else 0) | (128 if use_shadowing_function else 0)
        self.alpha_u = self.alpha_v = 0.1; self.eta = 1.0; self.anisotropic = False
        self.eta_c = _f32([0, 0, 0]); self.k_c = _f32([1, 1, 1]); self.back = None
        self.scene = None; self.index = None
        self.nested = [nested]
        if getattr(nested, 'mask_parent', None) is None and nested.scene is None:
            nested.mask_parent = self          # NAMES its parameters '<normalmap>.nested_bsdf.*' (NormalMap::traverse, normalmap.cpp:129-132): Scene._bsdf_key_base

    def _own_lobes(self):
        """the nested BSDF's components -- those of its `twosided`, if it is one (normalmap.cpp:117-122); BSDFFlags::NormalMapped marks the BSDF, not a lobe"""
        n = self.nested[0]
        return [n._lobe_flags(i) for i in range(n.component_count())]

    # the record's flag word wherever it is read or written, BSDF::flags() / BSDF::flags(i) when called (as on a blend record)
    @property
    def flags(self):
        return _RecordFlags(self._flags, self)

    @flags.setter
    def flags(self, value):
        self._flags = int(value)


def _mk_normalmap(props, named, key):
    """the `normalmap` plugin: the `normalmap` texture, exactly one nested BSDF under a free name, `flip_invalid_normals` and `use_shadowing_function` (normalmap.cpp:100-115)"""
    _check_props('normalmap', props, ('normalmap', 'flip_invalid_normals', 'use_shadowing_function'), children=('bsdf',))
    nested = None
    for k, v in props.items():
        if k in ('type', 'id', 'normalmap', 'flip_invalid_normals', 'use_shadowing_function'):
            continue
        obj = _resolve(v, named, k) if isinstance(v, dict) else v
        if isinstance(obj, BSDF):
            if nested is not None:
                raise RuntimeError("Only a single BSDF child object can be specified.")
            nested = obj
    if nested is None:
        raise RuntimeError("Exactly one BSDF child object must be specified.")
    if 'normalmap' not in props:
        raise RuntimeError("Property \"normalmap\" has not been specified!")
    if nested.kind in _NESTING_BSDFS or (nested.back is not None and nested.back.kind in _NESTING_BSDFS):
        raise RuntimeError("normalmap: a nested `%s` is not supported in hip_ad_rgb (nested BSDFs are plain BSDF models, or `twosided` over them)"
                           % (nested.kind if nested.kind in _NESTING_BSDFS else nested.back.kind))
    if getattr(nested, 'attr', None) is not None or (nested.back is not None and getattr(nested.back, 'attr', None) is not None):
        raise RuntimeError("normalmap: a `mesh_attribute` texture on the nested BSDF is not supported in hip_ad_rgb")
    nm = props['normalmap']
    if isinstance(nm, (list, tuple, np.ndarray)) and len(nm) == 3:
        nm = {'type': 'rgb', 'value': [float(x) for x in nm]}
    return NormalMapBSDF(nm, nested, bool(props.get('flip_invalid_normals', True)), bool(props.get('use_shadowing_function', True)), id=key)


class Texture(dict):
    """A texture plugin as mi.load_dict returns it: the plugin's properties (every consumer reads them as a dict), with the one method of the Texture interface that a
    `bumpmap` calls.  eval_1_grad(si): BitmapTexture::eval_1_grad (bitmap.cpp:543-599) for a `bitmap` -- the gradient of eval_1 with respect to si.uv, a 2 x n tensor,
    computed by the library's host entry (har_texture_eval_1_grad_host: the per-lane code of the kernels).  The call does NOT run on the device: it is a convenience entry
    (uv is copied to the host and the result back); renders evaluate the gradient inside the shading kernels.  Every other texture raises
    NotImplementedError("eval_1_grad"), as the base class does (src/render/texture.cpp:38-39)."""

    def eval_1_grad(self, si, active=True):
        if self.get('type') != 'bitmap':
            raise NotImplementedError("eval_1_grad")
        torch = _torch()
        uv = torch.as_tensor(si.uv, dtype=torch.float32).reshape(2, -1)
        n = uv.shape[1]
        host = np.ascontiguousarray(uv.detach().cpu().numpy(), np.float32)
        probe = self.__dict__.get('_probe')          # the private scene that holds the bitmap: lowered once per Texture object
        if probe is None:
            probe = BumpMapBSDF(dict(self), BSDF({'type': 'diffuse'}))
            Scene({'_bsdf': probe})
            self.__dict__['_probe'] = probe
        d = probe.scene.desc()
        out = np.zeros((2, n), np.float32)
        check(lib().har_texture_eval_1_grad_host(C.byref(d), int(probe.tex_index), n, _fp(host), _fp(out), None, None))
        if active is not True:
            out = out * np.asarray(torch.as_tensor(active).detach().cpu().numpy(), np.float32).reshape(1, -1)
        return torch.as_tensor(out, device=uv.device)


class BumpMapBSDF(BSDF):
    """BumpMap (src/bsdfs/bumpmap.cpp:102-135): a BSDF record whose texture is the height map -- a raw `bitmap` of one or three channels, read by Texture::eval_1_grad -- and
    which names ONE nested BSDF: a plain model, or a `twosided` over one or two of them; it becomes a record of its own (Scene._add_bsdf).  `scale` rides in the record's
    alpha_u.  flags: 16 = a one-channel height map, 64 = flip_invalid_normals, 128 = use_shadowing_function, 1 = wrapped by a `twosided`."""

    def __init__(self, texture, nested, scale=1.0, flip_invalid_normals=True, use_shadowing_function=True, id=None):
        self.id = id; self.kind = 'bumpmap'; self.slot0_name = 'nested_texture'; self.slot1_name = None
        self.attr = None; self.attr_mesh = None
        if not (isinstance(texture, dict) and texture.get('type') == 'bitmap'):
            what = texture.get('type') if isinstance(texture, dict) else type(texture).__name__
            raise RuntimeError("bumpmap: the nested texture is a `%s`: only a `bitmap` texture is supported in hip_ad_rgb (Texture::eval_1_grad is implemented by bitmaps; "
                               "`rgb`, a float and `mesh_attribute` have none)" % what)
        src = texture['data'] if 'data' in texture else (texture['bitmap'].data if isinstance(texture.get('bitmap'), Bitmap) else Bitmap(texture['filename']).data)
        ch = 1 if len(tuple(src.shape)) == 2 else int(src.shape[2])
        if ch not in (1, 3):
            raise RuntimeError("bumpmap: the height bitmap has %d channels, expected 1 or 3" % ch)
        self.texture, self.tex_mode, self.tex_to_uv = _bitmap_from_props(texture)
        self.weight_channels = ch
        self.value = _f32([0.5, 0.5, 0.5]); self.value2 = _f32([0, 0, 0])
        self.flags = (16 if ch == 1 else 0) | (64 if flip_invalid_normals else 0) | (128 if use_shadowing_function else 0)
        scale = float(np.float32(scale))
        if not math.isfinite(scale):
            raise RuntimeError("bumpmap: `scale` must be finite")
        self.alpha_u = self.alpha_v = scale; self.eta = 1.0; self.anisotropic = False
        self.eta_c = _f32([0, 0, 0]); self.k_c = _f32([1, 1, 1]); self.back = None
        self.scene = None; self.index = None
        self.nested = [nested]
        if getattr(nested, 'mask_parent', None) is None and nested.scene is None:
            nested.mask_parent = self          # NAMES its parameters '<bumpmap>.nested_bsdf.*' (BumpMap::traverse, bumpmap.cpp:131-135): Scene._bsdf_key_base

    def _own_lobes(self):
        """the nested BSDF's components -- those of its `twosided`, if it is one (bumpmap.cpp:124-128)"""
        n = self.nested[0]
        return [n._lobe_flags(i) for i in range(n.component_count())]

    @property
    def flags(self):
        return _RecordFlags(self._flags, self)

    @flags.setter
    def flags(self, value):
        self._flags = int(value)


def _mk_bumpmap(props, named, key):
    """the `bumpmap` plugin: exactly one nested texture and exactly one nested BSDF, both under free names (the constructor walks props.objects()), `scale`,
    `flip_invalid_normals` and `use_shadowing_function` (bumpmap.cpp:102-122)"""
    known = ('scale', 'flip_invalid_normals', 'use_shadowing_function')
    for k, v in props.items():          # a plain number where the height map belongs: no object in the reference either; refused by name here
        if k not in ('type', 'id') + known and isinstance(v, (int, float)) and not isinstance(v, bool):
            raise RuntimeError("bumpmap: the nested texture \"%s\" is a `float`: only a `bitmap` texture is supported in hip_ad_rgb (Texture::eval_1_grad is implemented by "
                               "bitmaps; `rgb`, a float and `mesh_attribute` have none)" % k)
    _check_props('bumpmap', props, known, children=('bsdf', 'texture'))
    nested = None; texture = None
    for k, v in props.items():
        if k in ('type', 'id') + known:
            continue
        obj = v
        if isinstance(v, dict) and _PLUGIN_KINDS.get(v.get('type')) == 'texture':
            obj = Texture(v)
        elif isinstance(v, dict):
            obj = _resolve(v, named, k)
        if isinstance(obj, BSDF):
            if nested is not None:
                raise RuntimeError("Only a single BSDF child object can be specified.")
            nested = obj
        elif isinstance(obj, dict) and _PLUGIN_KINDS.get(obj.get('type')) == 'texture':
            if texture is not None:
                raise RuntimeError("Only a single Texture child object can be specified.")
            texture = obj
    if nested is None:
        raise RuntimeError("Exactly one BSDF child object must be specified.")
    if texture is None:
        raise RuntimeError("Exactly one Texture child object must be specified.")
    if nested.kind in _NESTING_BSDFS or (nested.back is not None and nested.back.kind in _NESTING_BSDFS):
        raise RuntimeError("bumpmap: a nested `%s` is not supported in hip_ad_rgb (nested BSDFs are plain BSDF models, or `twosided` over them)"
                           % (nested.kind if nested.kind in _NESTING_BSDFS else nested.back.kind))
    if getattr(nested, 'attr', None) is not None or (nested.back is not None and getattr(nested.back, 'attr', None) is not None):
        raise RuntimeError("bumpmap: a `mesh_attribute` texture on the nested BSDF is not supported in hip_ad_rgb")
    return BumpMapBSDF(texture, nested, props.get('scale', 1.0), bool(props.get('flip_invalid_normals', True)), bool(props.get('use_shadowing_function', True)), id=key)


def _mk_blendbsdf(props, named, key):
    """the `blendbsdf` plugin: `weight` and exactly two nested BSDFs under free names, in declaration order (blendbsdf.cpp:80-92)"""
    _check_props('blendbsdf', props, ('weight',), children=('bsdf',))
    nested = []
    for k, v in props.items():
        if k in ('type', 'id', 'weight'):
            continue
        obj = _resolve(v, named, k) if isinstance(v, dict) else v
        if isinstance(obj, BSDF):
            if len(nested) == 2:
                raise RuntimeError("BlendBSDF: Cannot specify more than two child BSDFs")
            nested.append(obj)
    if 'weight' not in props:
        raise RuntimeError("Property \"weight\" has not been specified!")
    if len(nested) != 2:
        raise RuntimeError("BlendBSDF: Two child BSDFs must be specified!")
    for c in nested:
        if c.kind == 'mask':
            raise RuntimeError("blendbsdf: a nested `mask` is not supported in hip_ad_rgb (put the `mask` outside, over plain BSDF models)")
        if c.kind in ('normalmap', 'bumpmap'):
            raise RuntimeError("blendbsdf: a nested `%s` is not supported in hip_ad_rgb (nested BSDFs are plain BSDF models)" % c.kind)
        if c.kind == 'blendbsdf' or (c.flags & 1):
            raise RuntimeError("blendbsdf: nested BSDFs must be plain BSDF models in this variant")
    return BlendBSDF(props['weight'], nested, id=key)


def _transmits(b):
    """does the BSDF have a transmission lobe (what `twosided` refuses, twosided.cpp:79-83)"""
    return b.kind in ('dielectric', 'thindielectric') or (b.kind == 'blendbsdf' and any(c.kind in ('dielectric', 'thindielectric') for c in b.nested)) or b.kind == 'mask' or (b.kind in ('normalmap', 'bumpmap') and _transmits(b.nested[0]))      # (BSDFFlags::Null is part of BSDFFlags::Transmission; a normalmap has its nested BSDF's lobes)


def _mk_twosided(props, named, key):
    """TwoSidedBRDF (src/bsdfs/twosided.cpp:70-110): one or two nested BSDFs without a transmission component."""
    _check_props('twosided', props, ('allow_transmission',), unsupported=(('allow_transmission', False),), children=('bsdf',))      # twosided.cpp:76-104: nested BSDFs under any name
    nested = []
    for k, v in props.items():
        if k in ('type', 'id', 'allow_transmission'):
            continue
        obj = _resolve(v, named, k) if isinstance(v, dict) else v
        if isinstance(obj, BSDF):
            nested.append(obj)
    if not nested or len(nested) > 2:
        raise RuntimeError("twosided: a maximum of two nested BSDFs can be specified (and at least one)!")
    for b in nested:
        if _transmits(b):
            raise RuntimeError("Only materials without a transmission component can be nested!")
    if len(nested) == 2 and nested[1] is not nested[0] and any(b.kind == 'normalmap' for b in nested):
        raise RuntimeError("twosided: two nested BSDFs with a `normalmap` among them are not supported in hip_ad_rgb (nest ONE normalmap: twosided(normalmap(X)))")
    if len(nested) == 2 and nested[1] is not nested[0] and any(b.kind == 'bumpmap' for b in nested):
        raise RuntimeError("twosided: two nested BSDFs with a `bumpmap` among them are not supported in hip_ad_rgb (nest ONE bumpmap: twosided(bumpmap(X)))")
    front = nested[0]
    if front.flags & 1:
        raise RuntimeError("twosided: nested BSDF is already two-sided")
    front.flags |= 1; front.id = front.id or key
    front.back = nested[1] if len(nested) == 2 and nested[1] is not nested[0] else None
    if front.back is not None:
        front.back.twosided_parent = front          # (its parameters are '<twosided>.brdf_1.*': Scene._bsdf_key_base)
    if key:
        front.id = key
    return front


def _sampling_weight(props):
    """Emitter(props) (src/render/emitter.cpp:9): `sampling_weight`, default 1 -- Scene::update_emitter_sampling_distribution (scene.cpp:120-141) switches from the
    uniform emitter choice to a DiscreteDistribution over the weights as soon as one of them is not 1"""
    w = float(np.float32(props.get('sampling_weight', 1.0)))
    if not (w >= 0.0) or not math.isfinite(w):
        raise RuntimeError("DiscreteDistribution: entries must be non-negative!")
    return w


def _emissive_rgb(plugin, name, v):
    """Properties::get_emissive_texture in RGB variants: a float, an `rgb` colour (unbounded) -- spatially varying textures are refused where the path needs the
    texture-importance-sampling branch (area.cpp:133-165) or is not written for them"""
    if isinstance(v, dict) and v.get('type') not in (None, 'rgb') and plugin == 'constant':
        raise RuntimeError("Expected a non-spatially varying radiance spectra!")           # the reference's own refusal: constant.cpp:60-61
    if isinstance(v, dict) and v.get('type') not in (None, 'rgb'):
        raise RuntimeError("%s: a spatially varying \"%s\" (texture plugin \"%s\") is not implemented by hip_ad_rgb -- the reference then importance-samples the "
                           "texture and maps the sample through Shape::eval_parameterization (src/emitters/area.cpp:133-165); use an `rgb` value" % (plugin, name, v.get('type')))
    return _rgb_value(v, 1.0, bounded=False)


def _check_sampling_transform(rows):
    """BitmapTextureImpl::check_sampling_transform (src/textures/bitmap.cpp:976-992): position sampling needs a to_uv that maps the unit square's corners onto themselves"""
    m = np.asarray(rows if rows is not None else [1, 0, 0, 0, 1, 0], np.float32).reshape(2, 3)
    corners = np.asarray([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    hits = 0
    for c in corners:
        q = m[:, :2] @ c + m[:, 2]
        for j, d in enumerate(corners):
            if float(((q - d) ** 2).sum()) < 1e-8:
                hits |= 1 << j
    if hits != 0xF:
        raise RuntimeError("Bitmap texture: position sampling (e.g. of an area emitter's radiance) requires a 'to_uv' transformation that maps the unit square onto "
                           "itself, such as a flip, a transpose or a multiple of a 90 degree rotation.")


class AreaLight:
    """AreaLight (src/emitters/area.cpp): a uniform `radiance`, or a `bitmap` on a rectangle; it inherits the placement of its parent shape (a `to_world` is an error, :66-69)."""

    def __init__(self, props):
        if 'to_world' in props:
            raise RuntimeError("Found a 'to_world' transformation -- this is not allowed. The area light inherits this transformation from its parent shape.")
        _check_props('area', props, ('radiance', 'sampling_weight'), free_children=False)
        rad = props.get('radiance', {'type': 'rgb', 'value': 1.0})
        self.texture = None; self.tex_mode = 0; self.tex_to_uv = None; self.tex_index = None
        if isinstance(rad, dict) and rad.get('type') == 'bitmap':
            # a spatially varying radiance (is_spatially_varying(), area.cpp:74-75): the texture is importance-sampled and mapped onto the shape by
            # Shape::eval_parameterization (:133-165) -- built for rectangles (HarEmitter type 7); the parent shape decides (Scene._add_mesh)
            self.texture, self.tex_mode, self.tex_to_uv = _bitmap_from_props(rad)
            _check_sampling_transform(self.tex_to_uv)
            self.radiance = _f32([0.0, 0.0, 0.0])
        else:
            self.radiance = _emissive_rgb('area', 'radiance', rad)       # get_emissive_texture("radiance", 1.f), :71
        self.sampling_weight = _sampling_weight(props)


class ConstantEmitter:
    """ConstantBackgroundEmitter (src/emitters/constant.cpp): uniform environment radiance."""

    def __init__(self, props):
        _check_props('constant', props, ('radiance', 'sampling_weight', 'to_world'), free_children=False)      # Endpoint(props) queries to_world (endpoint.cpp:12); a uniform environment does not depend on it
        self.radiance = _emissive_rgb('constant', 'radiance', props.get('radiance', {'type': 'rgb', 'value': 1.0}))
        self.sampling_weight = _sampling_weight(props)


class PointLight:
    """PointLight (src/emitters/point.cpp): isotropic point source of radiant `intensity` at `position` (or the translation of `to_world`);
    EmitterFlags::DeltaPosition -- only emitter sampling finds it, with MIS weight 1 (path.cpp:274, prb.py:211)."""

    def __init__(self, props):
        _check_props("point", props, ('position', 'to_world', 'intensity', 'sampling_weight'), free_children=False)
        self.sampling_weight = _sampling_weight(props)
        if 'position' in props:
            if 'to_world' in props:                                  # point.cpp:65-68
                raise RuntimeError("Only one of the parameters 'position' and 'to_world' can be specified at the same time!'")
            self.position = _f32(list(props['position'])).reshape(3)
        else:
            self.position = _f32(props.get('to_world', ScalarTransform4f()).col_major_3x4()[9:12])      # m_to_world.translation(), point.cpp:72
        self.intensity = _rgb_value(props.get('intensity', {'type': 'rgb', 'value': 1.0}), 1.0, bounded=False, uniform='intensity')   # get_emissive_texture("intensity", 1.f), :77


class SpotLight:
    """SpotLight (src/emitters/spot.cpp) without a `texture`: a point source at the origin of `to_world` that radiates `intensity` along the local +z axis inside
    `beam_width` degrees, falling off linearly in the angle to zero at `cutoff_angle` (falloff_curve, :143-151); EmitterFlags::DeltaPosition."""

    def __init__(self, props):
        _check_props("spot", props, ('to_world', 'intensity', 'cutoff_angle', 'beam_width', 'texture', 'sampling_weight'), free_children=False)
        self.sampling_weight = _sampling_weight(props)
        if 'texture' in props:
            if isinstance(props['texture'], dict) and props['texture'].get('type') == 'mesh_attribute':
                raise RuntimeError("spot: a `mesh_attribute` as property \"texture\" is not implemented by hip_ad_rgb")
            raise RuntimeError("spot: property \"texture\" is not implemented by hip_ad_rgb")
        self.to_world = props.get('to_world', ScalarTransform4f())
        self.intensity = _rgb_value(props.get('intensity', {'type': 'rgb', 'value': 1.0}), 1.0, bounded=False, uniform='intensity')      # get_emissive_texture("intensity", 1.f), :93
        self.cutoff_angle = float(np.float32(props.get('cutoff_angle', 20.0)))                                        # :105-107
        self.beam_width = float(np.float32(props.get('beam_width', np.float32(self.cutoff_angle) * np.float32(3.0) / np.float32(4.0))))
        if not (self.cutoff_angle >= self.beam_width and self.cutoff_angle > 0):
            raise RuntimeError("spot: cutoff_angle must be positive and not smaller than beam_width")


class DirectionalEmitter:
    """DirectionalEmitter (src/emitters/directional.cpp): a distant source that delivers `irradiance` onto surfaces perpendicular to its direction of travel,
    the +z axis of `to_world` (or `direction`, lowered to look_at(0, direction, up) as in :69-78); EmitterFlags::Infinite | DeltaDirection -- sampled with
    MIS weight 1, invisible to escaping rays."""

    def __init__(self, props):
        _check_props("directional", props, ('to_world', 'direction', 'irradiance', 'sampling_weight'), free_children=False)
        self.sampling_weight = _sampling_weight(props)
        if 'direction' in props:
            if 'to_world' in props:                                   # directional.cpp:70-72
                raise RuntimeError("Only one of the parameters 'direction' and 'to_world' can be specified at the same time!'")
            d = _f32(list(props['direction'])).reshape(3); d = (d / np.sqrt(np.float32((d * d).sum()))).astype(np.float32)
            # coordinate_system(direction).first (vector.h:118-138, Duff et al.) in float32
            sign = np.float32(np.copysign(1.0, d[2])); a = np.float32(-1.0) / (sign + d[2]); b = d[0] * d[1] * a
            up = _f32([np.copysign(1.0, d[2]) * (d[0] * d[0] * a) + 1.0, np.copysign(1.0, d[2]) * b, -np.copysign(1.0, d[2]) * d[0]])
            self.to_world = ScalarTransform4f().look_at(origin=[0.0, 0.0, 0.0], target=[float(x) for x in d], up=[float(x) for x in up])
        else:
            self.to_world = props.get('to_world', ScalarTransform4f())
        self.irradiance = _rgb_value(props.get('irradiance', {'type': 'rgb', 'value': 1.0}), 1.0, bounded=False, uniform='irradiance')      # get_emissive_texture("irradiance", 1.f), :80


def _parse_fov(props, aspect):
    """parse_fov (src/render/sensor.cpp:142-196): the horizontal field of view in degrees from `fov` + `fov_axis`, or `focal_length`, at `aspect` = width / height"""
    if 'fov' in props and 'focal_length' in props:
        raise RuntimeError("Please specify either a focal length ('focal_length') or a field of view ('fov')!")
    if 'fov' in props:
        fov = float(props['fov']); axis = str(props.get('fov_axis', 'x')).lower()
        if axis == 'smaller':
            axis = 'y' if aspect > 1 else 'x'
        elif axis == 'larger':
            axis = 'x' if aspect > 1 else 'y'
    else:
        fl = str(props.get('focal_length', '50mm'))
        try:
            value = float(fl[:-2] if fl.endswith('mm') else fl)
        except ValueError:
            raise RuntimeError("Could not parse the focal length (must be of the form <x>mm, where <x> is a positive integer)!")
        fov = 2.0 * math.degrees(math.atan(math.sqrt(36 * 36 + 24 * 24) / (2.0 * value))); axis = 'diagonal'
    if axis == 'x':
        result = fov
    elif axis == 'y':
        result = math.degrees(2.0 * math.atan(math.tan(0.5 * math.radians(fov)) * aspect))
    elif axis == 'diagonal':
        width = 2.0 * math.tan(0.5 * math.radians(fov)) / math.sqrt(1.0 + 1.0 / (aspect * aspect))
        result = math.degrees(2.0 * math.atan(width * 0.5))
    else:
        raise RuntimeError("The 'fov_axis' parameter must be set to one of 'smaller', 'larger', 'diagonal', 'x', or 'y'!")
    if result <= 0.0 or result >= 180.0:
        raise RuntimeError("The horizontal field of view must be in the range [0, 180]!")
    return result


class Projector:
    """Projector (src/emitters/projector.cpp): the reciprocal of the perspective camera -- a point at the origin of `to_world` that projects `irradiance` (an `rgb`
    value, or a `bitmap` of three channels or one) along the local +z axis through the perspective camera's pixel-to-direction map, times `scale`.  `fov`, `focal_length`
    and `fov_axis` are read as a sensor reads them (parse_fov), at the aspect of the irradiance texture (1 for a constant).  EmitterFlags::DeltaPosition: only emitter
    sampling finds it, with MIS weight 1.  Not implemented (nothing on the `path` / `prb` route calls them): sample_ray, sample_position, sample_wavelengths and
    eval_direction on its own."""

    def __init__(self, props):
        _check_props("projector", props, ('irradiance', 'scale', 'to_world', 'fov', 'focal_length', 'fov_axis', 'sampling_weight'), free_children=False)
        self.sampling_weight = _sampling_weight(props)
        self.to_world = props.get('to_world', ScalarTransform4f())
        if abs(float(np.linalg.det(np.asarray(self.to_world.matrix, np.float64).reshape(4, 4)))) == 0.0:
            raise RuntimeError("projector: to_world is singular")
        self.scale = float(np.float32(props.get('scale', 1.0)))                    # :124
        if not math.isfinite(self.scale):
            raise RuntimeError("projector: `scale` is not finite")
        irr = props.get('irradiance', {'type': 'rgb', 'value': 1.0})              # get_emissive_texture("irradiance", 1.f), :126
        self.texture = None; self.tex_mode = 0; self.tex_to_uv = None; self.tex_index = None; self.channels = 3
        if isinstance(irr, dict) and irr.get('type') == 'mesh_attribute':
            raise RuntimeError("projector: a `mesh_attribute` as property \"irradiance\" is not implemented by hip_ad_rgb (an emitter has no shape to read an attribute of)")
        if isinstance(irr, dict) and irr.get('type') == 'bitmap':
            raw = irr['data'] if 'data' in irr else (irr['bitmap'].data if isinstance(irr.get('bitmap'), Bitmap) else None)
            if raw is not None and (len(raw.shape) == 2 or raw.shape[2] == 1):
                self.channels = 1
            self.texture, self.tex_mode, self.tex_to_uv = _bitmap_from_props(irr)
            if not np.isfinite(self.texture).all():
                raise RuntimeError("projector: the irradiance bitmap must be finite")
            self.irradiance = _f32([0.0, 0.0, 0.0])
            h, w = self.texture.shape[:2]
        else:
            if isinstance(irr, dict) and irr.get('type') != 'rgb':
                raise RuntimeError("projector: property \"irradiance\" takes an `rgb` value or a `bitmap` in hip_ad_rgb (texture plugin \"%s\" is not implemented for it)" % irr.get('type'))
            self.irradiance = _rgb_value(irr, 1.0, bounded=False)
            h, w = 1, 1                                                            # a uniform texture's resolution() is 1 x 1 (texture.cpp)
        self.x_fov = float(np.float32(_parse_fov(props, w / float(h))))            # :128-129


class EnvmapEmitter:
    """EnvironmentMapEmitter (src/emitters/envmap.cpp): lat-long radiance image, importance sampled by luminance * sin(theta)."""

    def __init__(self, props):
        _check_props('envmap', props, ('filename', 'bitmap', 'scale', 'mis_compensation', 'to_world', 'sampling_weight'), free_children=False)      # envmap.cpp:118-200
        self.sampling_weight = _sampling_weight(props)
        if 'bitmap' in props:
            if 'filename' in props:
                raise RuntimeError("Cannot specify both \"bitmap\" and \"filename\".")
            b = props['bitmap']
            if not isinstance(b, Bitmap):
                raise RuntimeError("Property \"bitmap\" must be a Bitmap instance.")
        elif 'filename' in props:
            b = Bitmap(props['filename'])
        else:
            raise RuntimeError("envmap: one of \"filename\" / \"bitmap\" is required")
        a = b.data
        if a.shape[2] == 1:                                  # Bitmap::convert(PixelFormat::RGB): luminance is replicated
            a = np.repeat(a, 3, axis=2)
        elif a.shape[2] == 4:
            a = a[:, :, :3]
        elif a.shape[2] != 3:
            raise RuntimeError("envmap: unsupported channel count %d" % a.shape[2])
        self.data = np.ascontiguousarray(a, np.float32)
        self.scale = float(props.get('scale', 1.0))
        self.mis_compensation = bool(props.get('mis_compensation', False))
        self.to_world = props.get('to_world', ScalarTransform4f())


class ShapeGroup:
    def __init__(self, shapes, keys=None):
        self.shapes = shapes
        self.keys = list(keys) if keys else [str(i) for i in range(len(shapes))]      # the children's names: '<group>.<child>' in mi.traverse, as in the reference


class Instance:
    def __init__(self, group, to_world):
        self.group = group; self.to_world = to_world


class Integrator:
    """PathIntegrator (src/integrators/path.cpp) / PRBIntegrator (ad/integrators/prb.py)."""

    def __init__(self, props):
        self.type = props['type']
        # integrator.cpp:26-33,128-147,539-550; block_size only shapes the scalar / LLVM-parallel drivers; the last four are hip_ad_rgb extensions
        _check_props(self.type, props, ('max_depth', 'rr_depth', 'hide_emitters', 'samples_per_pass', 'block_size', 'chunk_lanes', 'replay_cache', 'material_queues', 'packet_tracing', 'top_seed', 'emitter_gradients', 'shape_gradients', 'bsdf_parameter_gradients', 'light_texel_gradients', 'envmap_gradients'),
                     unsupported=(('timeout', -1.0),), free_children=False, slot_kind=())
        default_depth = -1 if self.type == 'path' else 6        # integrator.cpp:539, common.py:31
        self.max_depth = int(props.get('max_depth', default_depth))
        self.rr_depth = int(props.get('rr_depth', 5))
        self.hide_emitters = bool(props.get('hide_emitters', False))      # integrator.cpp:29
        if self.max_depth < 0 and self.max_depth != -1:
            raise RuntimeError("\"max_depth\" must be set to -1 (infinite) or a value >= 0")
        if self.rr_depth <= 0:
            raise RuntimeError("\"rr_depth\" must be set to a value greater than zero!")
        self.chunk_lanes = int(props.get('chunk_lanes', 0))
        self.replay_cache = bool(props.get('replay_cache', True))      # hip_ad_rgb extension, see har_integrator_set_replay_cache
        self.material_queues = bool(props.get('material_queues', False))   # hip_ad_rgb extension, see har_integrator_set_material_queues
        # hip_ad_rgb extension, see har_integrator_set_packet_tracing: None = automatic, False / True force the wave-shared descent of the camera rays off / on
        self.packet_tracing = props.get('packet_tracing', None)
        # hip_ad_rgb extension, see har_integrator_set_top_seed: None = the scene's choice, False / True force the seeded start of the per-ray closest-hit launches off / on
        self.top_seed = props.get('top_seed', None)
        self.emitter_gradients = bool(props.get('emitter_gradients', True))   # d / d radiance of area / constant emitters (har_integrator_set_grad_emitters)
        # d / d vertex positions (har_integrator_set_grad_positions): False, True (every eligible mesh) or a list of '<shape>.positions' keys --
        # the stand-in for dr.enable_grad(params[key]) of the reference
        self.shape_gradients = props.get('shape_gradients', False)
        # gradients of `alpha` / `alpha_u` / `alpha_v`, `eta`, `k` (roughconductor) and `alpha`, `specular_reflectance` (roughplastic): har_integrator_set_grad_bsdf_params
        self.bsdf_parameter_gradients = bool(props.get('bsdf_parameter_gradients', False))
        # gradients w.r.t. the texels of a bitmap `radiance` of area lights ('<shape>.emitter.radiance.data'; area.cpp:64-70): har_integrator_set_grad_light_texels
        self.light_texel_gradients = bool(props.get('light_texel_gradients', False))
        # gradients w.r.t. the texels and the `scale` of an environment map ('<emitter>.data', '<emitter>.scale'; envmap.cpp:203-208): har_integrator_set_grad_envmap
        if 'envmap_gradients' in props and self.type != 'prb':
            raise RuntimeError("Unreferenced property \"envmap_gradients\" in plugin of type \"%s\"" % self.type)
        self.envmap_gradients = bool(props.get('envmap_gradients', False))
        # SamplingIntegrator property (integrator.cpp:140-147); the Python AD integrators do not query it, and an
        # unqueried property is an error in the reference's plugin loader
        self.samples_per_pass = props.get('samples_per_pass', None)
        if self.samples_per_pass is not None:
            if self.type != 'path':
                raise RuntimeError("Unreferenced property \"samples_per_pass\" in plugin of type \"%s\"" % self.type)
            self.samples_per_pass = int(self.samples_per_pass)
        self._h = None

    def _bind_sensor(self, sensor):
        """the child table of a batch sensor goes to the library integrator before the render call that names its wide film (har_integrator_set_batch_sensors);
        a plain sensor rendered next clears it.  The table is compared by value: params.update() re-lowers children in place."""
        bound = self.__dict__.get('_batch_bound')
        if getattr(sensor, 'kind', None) == 'batch':
            ch = sensor.children_har()
            sig = bytes(ch)
            if bound != sig:
                check(lib().har_integrator_set_batch_sensors(self._handle(), ch, len(ch), _stream()))
                self._batch_bound = sig
        elif bound is not None:
            check(lib().har_integrator_set_batch_sensors(self._handle(), None, 0, None))
            self._batch_bound = None

    def _handle(self):
        if self._h is None:
            h = C.c_void_p()
            check(lib().har_integrator_create(0 if self.type == 'path' else 1, self.max_depth, self.rr_depth, self.chunk_lanes, C.byref(h)))
            self._h = h
            self._apply_settings(h)
        return self._h

    def _apply_settings(self, h):
        """the settings har_integrator_create does not take, on a library integrator `h` (this one's, or a DeviceGroup replica's)"""
        if not self.replay_cache:
            check(lib().har_integrator_set_replay_cache(h, 0))
        if self.material_queues:
            check(lib().har_integrator_set_material_queues(h, 1))
        if self.packet_tracing is not None:
            check(lib().har_integrator_set_packet_tracing(h, 1 if self.packet_tracing else 0))
        if self.top_seed is not None:
            check(lib().har_integrator_set_top_seed(h, 1 if self.top_seed else 0))
        if self.hide_emitters:
            check(lib().har_integrator_set_hide_emitters(h, 1))
        if self.samples_per_pass is not None:
            check(lib().har_integrator_set_samples_per_pass(h, self.samples_per_pass))

    def pass_layout(self, sensor, spp=0):
        """(spp_per_pass, n_passes) of a render() with `spp` samples (integrator.cpp:173-183,276-294)"""
        spp = spp or sensor.sampler().sample_count()
        a = C.c_uint32(); b = C.c_uint32()
        check(lib().har_render_pass_layout(self._handle(), C.byref(sensor.har), spp, C.byref(a), C.byref(b)))
        return a.value, b.value

    def __del__(self):
        try:
            if self._h is not None:
                lib().har_integrator_destroy(self._h)
        except Exception:
            pass

    def set_profiling(self, enable):
        check(lib().har_integrator_set_profiling(self._handle(), 1 if enable else 0))

    def timing(self):
        """average per frame since set_profiling(True): {class: (milliseconds, launches)}; "frames" = (frames averaged, 0)"""
        ms = (C.c_float * 8)(); cnt = (C.c_uint32 * 8)()
        check(lib().har_render_timing(self._handle(), ms, cnt))
        names = ["raygen", "trace_closest", "shade", "resolve", "splat", "total", "other", "frames"]
        return {names[i]: (ms[i], cnt[i]) for i in range(8)}

    def stats(self):
        st = _capi.HarStats()
        check(lib().har_render_stats(self._handle(), C.byref(st)))
        return dict(paths=st.paths, vertices=st.vertices, closest_rays=st.closest_rays, shadow_rays=st.shadow_rays)

    def _sensor(self, scene, sensor):
        sensor = scene.sensors()[sensor] if isinstance(sensor, int) else sensor
        self._bind_sensor(sensor)
        return sensor

    def render_film(self, scene, sensor=0, seed=0, spp=0, lanes=None, film=None, alpha_film=None, film_window=None):
        """Raw {R,G,B,W} accumulation of lanes [begin, end) (all when None); no develop.  `alpha_film` (H x W x 4 zeros): also accumulate
        w * alpha into its channel 3 (`rgba` films, har_integrator_set_alpha_film).  `film_window` = (first row, rows): `film` / `alpha_film` hold only those rows
        of the crop window (har_integrator_set_film_window: a rank's band + the filter's reach)."""
        torch = _torch(); dev = _device()
        sensor = self._sensor(scene, sensor)
        if spp:
            sensor.sampler().set_sample_count(spp)
        spp = sensor.sampler().sample_count()
        w, h = sensor.film().crop_size()
        if film is None:
            film = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        lb, le = lanes if lanes else (0, 0)
        check(lib().har_integrator_set_alpha_film(self._handle(), _ptr(alpha_film) if alpha_film is not None else None))
        if film_window is not None:
            if film.shape[0] < film_window[1] or (alpha_film is not None and alpha_film.shape[0] < film_window[1]):
                raise RuntimeError("render_film(): the film holds %d rows, the window %d" % (film.shape[0], film_window[1]))
            check(lib().har_integrator_set_film_window(self._handle(), int(film_window[0]), int(film_window[1])))
        try:
            check(lib().har_render(scene._handle(), self._handle(), C.byref(sensor.har), (sensor.sampler().m_base_seed + int(seed)) & 0xffffffff,
                                   spp, lb, le, _ptr(film), _stream()))
        finally:
            if alpha_film is not None:        # the integrator must not keep a pointer into a tensor it does not own
                check(lib().har_integrator_set_alpha_film(self._handle(), None))
            if film_window is not None:
                check(lib().har_integrator_set_film_window(self._handle(), 0, 0))
        return film

    def render(self, scene, sensor=0, seed=0, spp=0, develop=True, evaluate=True):
        """SamplingIntegrator::render (integrator.cpp:151) / ADIntegrator.render (common.py:46)."""
        torch = _torch()
        sensor = self._sensor(scene, sensor)
        alpha = None
        if sensor.film().alpha and develop:
            w, h = sensor.film().crop_size()
            alpha = torch.zeros((h, w, 4), dtype=torch.float32, device=_device())
        film = self.render_film(scene, sensor, seed, spp, alpha_film=alpha)
        if not develop:
            if self.type == 'prb':
                raise Exception("develop=True must be specified when invoking AD integrators")
            out = film
        else:
            out = develop_film(film, alpha, sensor.film().colour)
        if evaluate:
            torch.cuda.current_stream().synchronize()
            self.stats()                 # surfaces device-side errors (traversal stack overflow)
        return out

    def sample(self, scene, sampler, ray, medium=None, active=True, seed=None):
        """SamplingIntegrator::sample (integrator.h:432-437): (spec 3 x n, valid n) for the rays `ray` (mi.Ray3f) with the sampler's streams.
        `sampler` is a seeded mi.Sampler whose wavefront size equals the number of rays; its state is advanced (`path`) as the call draws from it."""
        torch = _torch(); dev = _device()
        if medium is not None:
            raise RuntimeError("Integrator.sample(): participating media are not part of the hip_ad_rgb path")
        n = len(ray)
        if not sampler.seeded() or sampler.wavefront_size() != n:
            raise RuntimeError("Integrator.sample(): the sampler must be seeded with wavefront_size == number of rays")
        rgb = torch.empty((3, n), dtype=torch.float32, device=dev); valid = torch.empty(n, dtype=torch.uint8, device=dev)
        state_out = torch.empty_like(sampler.state) if self.type == 'path' else None
        sd = sampler.m_seed_value if seed is None else (sampler.m_base_seed + int(seed)) & 0xffffffff
        # `active`: a masked ray never enters the loop -- zero radiance, invalid, and its sampler stream is not advanced (handled inside the call)
        # the mask tensor must OUTLIVE the call: a temporary would go back to the allocator pool the moment its pointer is taken, and the workspace the call
        # allocates through the same pool on first use could be handed its block (round 4's latent fault: the first masked sample() of an integrator read a
        # mask that the workspace's counters had overwritten)
        mask = _mask(active, n)
        check(lib().har_integrator_sample(scene._handle(), self._handle(), sd, 0, n, _ptr(ray.o), _ptr(ray.d), _ptr(ray.maxt), _ptr(sampler.state),
                                          _ptr(mask), _ptr(rgb), _ptr(valid), _ptr(state_out), _stream()))
        del mask
        if state_out is not None:
            sampler.state = state_out
        return rgb, valid.to(torch.bool)

    def render_weights(self, scene, sensor=0, seed=0, spp=0, lanes=None):
        """the weight-only splat of RBIntegrator.render_backward (common.py:716-746: a dummy L = 1 film) for lanes [begin, end) (all when None):
        raw H x W x 4 film whose channel 3 is the accumulated filter weight W[px]"""
        torch = _torch(); dev = _device()
        sensor = self._sensor(scene, sensor)
        if spp:
            sensor.sampler().set_sample_count(spp)
        spp = sensor.sampler().sample_count()
        w, h = sensor.film().crop_size()
        film = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
        lb, le = lanes if lanes else (0, 0)
        check(lib().har_render_weights(C.byref(sensor.har), (sensor.sampler().m_base_seed + int(seed)) & 0xffffffff, spp, lb, le, _ptr(film), _stream()))
        return film

    def _check_envmap_routes(self, scene, envmap_keys):
        """what har_render_backward refuses for the texel terms of an environment map (they are committed in place by the re-shading replay), said before anything is allocated"""
        if self.shape_gradients:
            raise RuntimeError("envmap gradients cannot be combined with vertex-position gradients (`envmap_gradients` with `shape_gradients`)")
        if not self.replay_cache:
            raise RuntimeError("envmap gradients need the replay cache (`replay_cache` is off)")
        if self.max_depth < 0 or self.max_depth > 12:
            raise RuntimeError("envmap gradients: max_depth must not exceed 12 (the cached bounces)")
        img = scene.textures[scene.emitters[envmap_keys["env_data"][1]]["mesh"]]
        if img.shape[0] < 3 or img.shape[1] < 2:
            raise RuntimeError("envmap gradients: an environment map smaller than 2 x 3 texels (padded by the emitter) is not differentiated")

    def render_backward(self, scene, params, grad_in, sensor=0, seed=0, spp=0, lanes=None, weight_film=None):
        """RBIntegrator.render_backward (common.py:625-783): returns {key: gradient tensor}."""
        if self.type != 'prb':
            raise RuntimeError("render_backward(): only the `prb` integrator implements the adjoint pass in hip_ad_rgb")
        # `envmap_gradients`: the environment map's keys of this scene, {kind: (key, emitter)} -- none: the switch stays off in the library.  What the library would refuse
        # (har_render_backward: the routes of the texel terms) is said here, before anything is allocated
        envmap_keys = {kind: (k, i) for k, (kind, i) in scene._pose_keys().items() if kind in ("env_data", "env_scale")} if getattr(self, 'envmap_gradients', False) else {}
        if envmap_keys:
            self._check_envmap_routes(scene, envmap_keys)
        torch = _torch(); dev = _device()
        sensor = self._sensor(scene, sensor)
        if spp:
            sensor.sampler().set_sample_count(spp)
        spp = sensor.sampler().sample_count()
        w, h = sensor.film().crop_size()
        sd = (sensor.sampler().m_base_seed + int(seed)) & 0xffffffff
        lb, le = lanes if lanes else (0, 0)
        if weight_film is None:
            weight_film = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
            check(lib().har_render_weights(C.byref(sensor.har), sd, spp, lb, le, _ptr(weight_film), _stream()))
        grad_in = torch.as_tensor(grad_in, dtype=torch.float32, device=dev)
        colour = sensor.film().colour
        nc = 1 if colour == 1 else 3
        if sensor.film().alpha and grad_in.numel() == h * w * (nc + 1):
            grad_in = grad_in.reshape(h, w, nc + 1)[:, :, :nc]           # alpha is a mask of detached decisions: no gradient
        grad_in = grad_in.reshape(h, w, nc)
        if colour:            # adjoint of develop's colour transform (linear: rows of luminance() / srgb_to_xyz()): d loss / d rgb = M^T d loss / d colour
            m = torch.tensor(_COLOUR_ROWS[colour], dtype=torch.float32, device=dev)
            grad_in = grad_in @ m
        grad_in = grad_in.contiguous()
        g_refl = torch.zeros((len(scene.bsdfs), 3), dtype=torch.float32, device=dev)
        g_tex = [torch.zeros(tuple(t.shape), dtype=torch.float32, device=dev) for t in scene.textures]
        ptrs = (C.c_void_p * max(1, len(g_tex)))(*[t.data_ptr() for t in g_tex])
        g_emit = torch.zeros((max(1, len(scene.emitters)), 3), dtype=torch.float32, device=dev)
        g_pos = {}; g_inst = None; inst_wanted = {}; rect_wanted = {}
        if self.shape_gradients:
            keys = scene._position_keys(); ikeys = scene._instance_keys()
            if self.shape_gradients is True:         # "every eligible mesh / instance": the meshes the adjoint can differentiate, instances if no instanced mesh is purely specular
                wanted = scene._differentiable_position_keys()
                inst_wanted = ikeys if all(scene._bsdf_has_smooth_lobe(m["bsdf"]) for m in scene.meshes[scene.top_mesh_count:]) else {}
            else:
                inst_wanted = {k: ikeys[k] for k in self.shape_gradients if k in ikeys}
                # a rectangle's 'to_world' (rectangle.cpp:199: Differentiable): its four vertices ARE to_world * (+-1, +-1, 0), so the matrix gradient is the chain rule over
                # the vertex-position gradients (rect_wanted: key -> (mesh, its positions key, whether the caller asked for the positions too))
                rkeys = scene._rect_keys()
                for k in self.shape_gradients:
                    if k in rkeys:
                        pk = scene.meshes[rkeys[k]]["key"] + ".positions"
                        if scene.meshes[rkeys[k]]["emitter"] >= 0 or pk not in scene._differentiable_position_keys():
                            raise RuntimeError("%s: only a rectangle without an area light and with a non-delta BSDF lobe can be differentiated through its 'to_world' in hip_ad_rgb" % k)
                        rect_wanted[k] = (rkeys[k], pk, pk in self.shape_gradients)
                wanted = {k: keys[k] for k in list(self.shape_gradients) + [v[1] for v in rect_wanted.values()] if k not in ikeys and k not in rkeys}    # KeyError: not a differentiable mesh / instance
            g_pos = {k: torch.zeros((scene.meshes[m]["V"].shape[0], 3), dtype=torch.float32, device=dev) for k, m in wanted.items()}      # the parameter's shape: N x 3
            by_mesh = {wanted[k]: g for k, g in g_pos.items()}
            pp = (C.c_void_p * max(1, len(scene.meshes)))(*[by_mesh[m].data_ptr() if m in by_mesh else None for m in range(len(scene.meshes))])
            # what the previous call left on must not veto this call's selection (nested vertex positions and instance transforms exclude each other): instances
            # that are no longer wanted go first, then the positions REPLACE the previous selection.  An unchanged selection changes nothing in the library, so an
            # optimisation loop keeps its adjoint workspace from step to step (both setters only rebuild it when the offset table / instance count differs).
            if not inst_wanted:
                check(lib().har_integrator_set_grad_instances(self._handle(), None, None))
            elif any(m >= scene.top_mesh_count for m in by_mesh):
                raise RuntimeError("Cannot differentiate instance parameters and shapegroup internal parameters at the same time!")     # instance.cpp:162-166
            check(lib().har_integrator_set_grad_positions(self._handle(), scene._handle(), pp if g_pos else None))
            if inst_wanted:
                g_inst = torch.zeros((len(scene.instances), 12), dtype=torch.float32, device=dev)
            check(lib().har_integrator_set_grad_instances(self._handle(), scene._handle() if inst_wanted else None, _ptr(g_inst) if inst_wanted else None))
        else:
            check(lib().har_integrator_set_grad_positions(self._handle(), None, None))
            check(lib().har_integrator_set_grad_instances(self._handle(), None, None))
        amap_keys = sorted(k for k, (kind, b) in scene._param_keys().items() if getattr(b, 'kind', None) == 'alphamap')
        if self.bsdf_parameter_gradients and amap_keys and any(b.kind in _NESTING_BSDFS for b in scene.bsdfs):
            raise RuntimeError("%s: the alpha texel gradients of a roughness map are not produced for a scene that also holds a `%s` in hip_ad_rgb (a roughconductor nested in a "
                               "`blendbsdf` / `mask` / `normalmap` / `bumpmap` renders; its alpha texels have no gradient)" % (amap_keys, next(b.kind for b in scene.bsdfs if b.kind in _NESTING_BSDFS)))
        if self.bsdf_parameter_gradients and amap_keys and self.shape_gradients:
            raise RuntimeError("%s: the alpha texel gradients of a roughness map cannot be combined with vertex-position / instance gradients (`shape_gradients`) in hip_ad_rgb" % amap_keys)
        if self.bsdf_parameter_gradients and any(b.kind == 'mask' for b in scene.bsdfs):
            raise RuntimeError("%s: `bsdf_parameter_gradients` is not implemented for a scene with a `mask` in hip_ad_rgb (its `opacity` and the nested BSDF's colour slot 0 have gradients)"
                               % sorted(k for k, (what, b) in scene._bsdf_param_keys().items() if what not in _NOGRAD_PARAMS))
        if self.bsdf_parameter_gradients and any(b.kind == 'blendbsdf' for b in scene.bsdfs):
            raise RuntimeError("%s: `bsdf_parameter_gradients` is not implemented for a scene with a `blendbsdf` in hip_ad_rgb (its `weight` and the nested BSDFs' colour slot 0 have gradients)"
                               % sorted(k for k, (what, b) in scene._bsdf_param_keys().items() if what not in _NOGRAD_PARAMS))
        g_extra = torch.zeros((max(1, len(scene.bsdfs)), 15), dtype=torch.float32, device=dev) if self.bsdf_parameter_gradients else None
        try:
            check(lib().har_integrator_set_grad_emitters(self._handle(), _ptr(g_emit) if self.emitter_gradients else None))
            check(lib().har_integrator_set_grad_bsdf_params(self._handle(), _ptr(g_extra) if g_extra is not None else None))
            check(lib().har_integrator_set_grad_light_texels(self._handle(), 1 if self.light_texel_gradients else 0))
            check(lib().har_integrator_set_grad_envmap(self._handle(), 1 if envmap_keys else 0))
            check(lib().har_render_backward(scene._handle(), self._handle(), C.byref(sensor.har), _ptr(grad_in), _ptr(weight_film), sd, spp,
                                            lb, le, _ptr(g_refl), ptrs, _stream()))
        finally:
            # no pointer into this call's tensors and no switch of it outlives the call: the primal pass of a later mi.render reads all three (HAR_SHADE_EMITTER_GRADS,
            # HAR_SHADE_LIGHT_TEXELS: extra shadow rays), and a forward render must not depend on what ran before it
            check(lib().har_integrator_set_grad_emitters(self._handle(), None))
            check(lib().har_integrator_set_grad_bsdf_params(self._handle(), None))
            check(lib().har_integrator_set_grad_light_texels(self._handle(), 0))
            check(lib().har_integrator_set_grad_envmap(self._handle(), 0))
        out = scene._gradients(g_refl, g_tex, g_emit if self.emitter_gradients else None, alpha_maps=g_extra is not None)
        if g_extra is not None:
            for k, (what, b) in scene._bsdf_param_keys().items():
                if what in _NOGRAD_PARAMS or what in _THIN_PARAMS:
                    continue                  # (no gradient w.r.t. the scalar index of refraction or a bump map's `scale`; a pane's own entries: below)
                rec = g_extra[b.index]
                out[k] = {"alpha": rec[0:6].sum().reshape(1), "alpha_u": rec[0:3].sum().reshape(1), "alpha_v": rec[3:6].sum().reshape(1),
                          "eta": rec[6:9], "k": rec[9:12], "slot1": rec[12:15]}[what]
        # a `thindielectric`'s own entries: eval() is zero for every direction, so prb.py:288-297 forms relative_grad(0) -- zeros of the parameter's shape, as the reference
        # returns for every delta model (its colour in slot 0 comes back as the untouched row / bitmap of the gradient buffers)
        for k, (what, b) in scene._bsdf_param_keys().items():
            if what in _THIN_PARAMS:
                out[k] = torch.zeros(1 if what == "thin_ior" else 3, dtype=torch.float32, device=dev)
        if self.light_texel_gradients:            # the light's bitmap is a texture of the scene like any other: its gradient sits in its entry of grad_textures
            for k, (kind, i) in scene._pose_keys().items():
                if kind == "emitter_tex" and scene.emitters[i].get("type") != 8:
                    out[k] = g_tex[scene.emitters[i]["light"].tex_index]
        out.update(scene._projector_gradients(g_tex if self.light_texel_gradients else None, g_emit if self.emitter_gradients else None, out))
        if envmap_keys:
            out.update(scene._envmap_gradients(g_tex[scene.emitters[envmap_keys["env_data"][1]]["mesh"]], envmap_keys))
        out.update(g_pos)
        for k, (mi_, pk, keep) in rect_wanted.items():         # d loss / d to_world[r, :] = sum over the vertices of  d loss / d p_v[r] * (local corner of v, 1);  fourth row constant
            rect = scene.meshes[mi_]["rect"]
            M = np.asarray(rect["to_world"].matrix, np.float64).reshape(4, 4)
            Pw = np.concatenate([scene.meshes[mi_]["V"][:, :3].astype(np.float64), np.ones((4, 1))], axis=1)
            local = torch.as_tensor((np.linalg.inv(M) @ Pw.T).T, dtype=torch.float32, device=dev)              # 4 vertices x (x, y, 0, 1)
            g = torch.zeros((4, 4), dtype=torch.float32, device=dev); g[:3, :] = g_pos[pk].reshape(4, 3).T @ local
            out[k] = g
            if not keep:
                out.pop(pk, None)
        for k, i in inst_wanted.items():                      # column-major 3x4 -> the reference's 4x4 (constant fourth row: zero gradient)
            m = torch.zeros((4, 4), dtype=torch.float32, device=dev); m[:3, :] = g_inst[i].reshape(4, 3).T
            out[k] = m
        return out


def _render_forward(self, scene, params=None, sensor=0, seed=0, spp=0, tangents=None, lanes=None, develop=True):
    """RBIntegrator.render_forward (common.py:497-623): the forward-mode derivative image for the parameter tangents.
    `tangents` = {key: tensor} (the values dr.set_grad() would carry); without it, the `.grad` fields of the `params` entries that have
    requires_grad are used.  Keys are those of mi.traverse(scene); missing keys have a zero tangent.  Returns the gradient image H x W x 3."""
    if self.type != 'prb':
        raise RuntimeError("render_forward(): only the `prb` integrator implements the differential pass in hip_ad_rgb")
    torch = _torch(); dev = _device()
    sensor = self._sensor(scene, sensor)
    if spp:
        sensor.sampler().set_sample_count(spp)
    spp = sensor.sampler().sample_count()
    w, h = sensor.film().crop_size()
    if tangents is None:
        tangents = {k: v.grad for k, v in (params or {}).items() if getattr(v, 'requires_grad', False) and getattr(v, 'grad', None) is not None}
    keys = scene._param_keys(); akeys = scene._attr_keys()
    proj = [k for k in tangents if scene._pose_keys().get(k, (None,))[0] in ("proj_scale", "emitter_tex") and scene.emitters[scene._pose_keys()[k][1]].get("type") == 8]
    proj += [k for k in tangents if k in scene._param_keys() and scene._param_keys()[k][0] == "emit" and scene.emitters[scene._param_keys()[k][1]].get("type") == 8]
    if proj:
        raise RuntimeError("projector: render_forward(): forward-mode tangents of %s are not implemented in hip_ad_rgb (use render_backward)" % proj)
    unknown = [k for k in tangents if k not in keys and k not in akeys]
    if unknown:
        raise RuntimeError("render_forward(): %s are not differentiable parameters of the `prb` forward mode (available: %s)" % (unknown, sorted(keys)))
    t_refl = torch.zeros((max(1, len(scene.bsdfs)), 3), dtype=torch.float32, device=dev)
    t_tex = [torch.zeros(tuple(t.shape), dtype=torch.float32, device=dev) for t in scene.textures]
    t_emit = torch.zeros((max(1, len(scene.emitters)), 3), dtype=torch.float32, device=dev)
    any_emit = False
    for k, v in tangents.items():
        if k in akeys:
            # the tangent of a mesh attribute, in the rows x 1 x 3 layout of every record that reads it (one channel: stored three times; what evaluates to 0: none)
            mesh, name = akeys[k]; rows, dim = scene.meshes[mesh]["attributes"][name].shape
            v = torch.as_tensor(v, dtype=torch.float32, device=dev)
            if tuple(v.shape) != (rows, dim):
                raise RuntimeError("render_forward(): %s: expected a tangent of shape %s" % (k, (rows, dim)))
            for b in scene._attr_readers(mesh, name):
                if id(b) in scene._blend_nested():
                    raise RuntimeError("render_forward(): %s -- forward-mode tangents of the BSDFs nested in a `blendbsdf` / `mask` / `normalmap` / `bumpmap` are not produced in hip_ad_rgb (a blend weight's / mask opacity's are; use render_backward)" % k)
                if dim == 1:
                    t_tex[b.tex_index].copy_(v.expand(rows, 3).reshape(rows, 1, 3))
                elif dim == 3 and b.kind not in _WEIGHTED_BSDFS:
                    t_tex[b.tex_index].copy_(v.reshape(rows, 1, 3))
            continue
        kind, b = keys[k]
        v = torch.as_tensor(v, dtype=torch.float32, device=dev)
        if kind != "emit" and id(b) in scene._blend_nested():
            raise RuntimeError("render_forward(): %s -- forward-mode tangents of the BSDFs nested in a `blendbsdf` / `mask` / `normalmap` / `bumpmap` are not produced in hip_ad_rgb (a blend weight's / mask opacity's are; use render_backward)" % k)
        if kind != "emit" and b.kind in _WEIGHTED_BSDFS:
            # the tangent of the weight, in every colour channel of the record's slot 0 (a three-channel bitmap: of its luminance)
            if kind == "tex" and b.weight_channels == 3:
                shape = t_tex[b.tex_index].shape
                v = (v.reshape(shape) * v.new_tensor(_LUMINANCE).reshape(1, 1, 3)).sum(dim=2, keepdim=True).expand(shape).contiguous()
            else:
                v = scene._colour_store(kind, b, v, k)
        if kind == "tex":
            t_tex[b.tex_index].copy_(v.reshape(t_tex[b.tex_index].shape))
        elif kind == "emit":
            t_emit[b].copy_(v.reshape(3)); any_emit = True
        else:
            t_refl[b.index].copy_(v.reshape(3))
    ptrs = (C.c_void_p * max(1, len(t_tex)))(*[t.data_ptr() for t in t_tex])
    film = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    lb, le = lanes if lanes else (0, 0)
    check(lib().har_render_forward(scene._handle(), self._handle(), C.byref(sensor.har), (sensor.sampler().m_base_seed + int(seed)) & 0xffffffff, spp, lb, le,
                                   _ptr(t_refl), ptrs if t_tex else None, _ptr(t_emit) if any_emit else None, _ptr(film), _stream()))
    return develop_film(film, None, sensor.film().colour) if develop else film


Integrator.render_forward = _render_forward


# AOV types of the `aov` integrator: name -> (HAR_AOV_* value, channel suffixes) (aov.cpp:117-168)
_AOV_TYPES = {'albedo': (0, 'RGB'), 'depth': (1, 'T'), 'position': (2, 'XYZ'), 'uv': (3, 'UV'), 'geo_normal': (4, 'XYZ'), 'sh_normal': (5, 'XYZ'),
              'dp_du': (6, 'XYZ'), 'dp_dv': (7, 'XYZ'), 'prim_index': (8, 'I'), 'shape_index': (9, 'I')}


def _parse_aovs(spec):
    """AOVIntegratorImpl(aovs_spec) (aov.cpp:108-173): "<name>:<type>, ..." -> ([HAR_AOV_* values], [channel names])"""
    types = []; names = []
    for token in [t for t in str(spec).replace(',', ' ').split(' ') if t]:
        item = token.split(':')
        if len(item) != 2 or not item[0] or not item[1]:
            raise RuntimeError("Invalid AOV specification: require <name>:<type> pair")
        if item[1] in ('duv_dx', 'duv_dy'):      # need ray differentials, which the sensors of this variant do not carry
            raise RuntimeError("aov: AOV type \"%s\" is not implemented by hip_ad_rgb" % item[1])
        if item[1] not in _AOV_TYPES:
            raise RuntimeError("Invalid AOV type \"%s\"!" % item[1])
        value, suffixes = _AOV_TYPES[item[1]]
        types.append(value); names += ["%s.%s" % (item[0], c) for c in suffixes]
    return types, names


class AOVIntegrator(Integrator):
    """AOVIntegrator (src/integrators/aov.cpp): per-pixel depth / position / normals / albedo / uv / partials / ids next to the images of its child integrators."""

    def __init__(self, props, named=None):
        self.type = 'aov'
        for k, v in props.items():
            kind = _object_kind(v)
            if isinstance(v, dict) and v.get('type') == 'aov' or isinstance(v, AOVIntegrator):
                raise RuntimeError("aov: a nested `aov` integrator is not implemented by hip_ad_rgb")
            if kind is not None and kind != 'integrator':
                raise RuntimeError("Child objects must be of type 'SamplingIntegrator'!")          # aov.cpp:358-360
        # SamplingIntegrator / Integrator properties (integrator.cpp:26-33,128-147): hide_emitters is read by the base class and does not reach the AOV pass, whose inner
        # integrator is built from empty properties (aov.cpp:108); chunk_lanes is the hip_ad_rgb extension of `path`
        _check_props('aov', props, ('aovs', 'hide_emitters', 'block_size', 'chunk_lanes'), unsupported=(('timeout', -1.0), ('samples_per_pass', None)),
                     free_children=True, children=('integrator',), slot_kind=())
        if 'aovs' not in props:
            raise RuntimeError("Property \"aovs\" has not been specified!")                          # aov.cpp:373
        if not isinstance(props['aovs'], str):
            raise RuntimeError("The property \"aovs\" has the wrong type (expected string)")
        self.children = []; self.child_names = []
        for k, v in props.items():
            if k in ('type', 'id', 'aovs', 'hide_emitters', 'block_size', 'chunk_lanes', 'timeout', 'samples_per_pass'):
                continue
            obj = _resolve(v, named if named is not None else {}, k) if isinstance(v, dict) else v
            if not isinstance(obj, Integrator):
                raise RuntimeError("Child objects must be of type 'SamplingIntegrator'!")
            self.children.append(obj); self.child_names.append(k)
        self.aov_types, self._own_names = _parse_aovs(props['aovs'])
        self.channels = len(self._own_names)
        self.max_depth = -1; self.rr_depth = 5; self.hide_emitters = bool(props.get('hide_emitters', False)); self.samples_per_pass = None
        self.chunk_lanes = int(props.get('chunk_lanes', 0))
        self.replay_cache = True; self.material_queues = False; self.packet_tracing = None; self.top_seed = None
        self._h = None

    def _handle(self):
        if self._h is None:             # carries the chunk size, the film window and the profiling events of the AOV pass
            h = C.c_void_p()
            check(lib().har_integrator_create(0, -1, 5, self.chunk_lanes, C.byref(h)))
            self._h = h
        return self._h

    def aov_names(self):
        """AOVIntegrator::aov_names (aov.cpp:357-382): per child <name>.R/.G/.B/.A and its own AOVs, then this integrator's"""
        out = []
        for name, child in zip(self.child_names, self.children):
            out += ["%s.%s" % (name, c) for c in 'RGBA']
            out += ["%s.%s" % (name, n) for n in (child.aov_names() if hasattr(child, 'aov_names') else [])]
        return out + list(self._own_names)

    def _types(self):
        return (C.c_uint32 * max(1, len(self.aov_types)))(*self.aov_types)

    def render_aov_film(self, scene, sensor=0, seed=0, spp=0, lanes=None, film=None, film_window=None):
        """Raw accumulation of the AOV pass (har_render_aovs): H x W x (C + 1) -- the C channels of aov_names(), then the filter weight -- for lanes [begin, end)
        (all when None) of the wavefront render() traces at this seed; not developed.  `film_window` as in render_film."""
        torch = _torch(); dev = _device()
        sensor = self._sensor(scene, sensor)
        if spp:
            sensor.sampler().set_sample_count(spp)
        spp = sensor.sampler().sample_count()
        w, h = sensor.film().crop_size()
        if film is None:
            film = torch.zeros((h if film_window is None else int(film_window[1]), w, self.channels + 1), dtype=torch.float32, device=dev)
        lb, le = lanes if lanes else (0, 0)
        if film_window is not None:
            if film.shape[0] < film_window[1]:
                raise RuntimeError("render_aov_film(): the film holds %d rows, the window %d" % (film.shape[0], film_window[1]))
            check(lib().har_integrator_set_film_window(self._handle(), int(film_window[0]), int(film_window[1])))
        try:
            check(lib().har_render_aovs(scene._handle(), self._handle(), C.byref(sensor.har), (sensor.sampler().m_base_seed + int(seed)) & 0xffffffff, spp, lb, le,
                                        len(self.aov_types), self._types(), _ptr(film), _stream()))
        finally:
            if film_window is not None:
                check(lib().har_integrator_set_film_window(self._handle(), 0, 0))
        return film

    def render(self, scene, sensor=0, seed=0, spp=0, develop=True, evaluate=True):
        """AOVIntegrator::render (aov.cpp:389-470): the children render with the same seed / spp, the AOV pass is one more pass over the same lanes; merge_channels
        (:591-617): every child's developed image (3 channels, 4 on an `rgba` film) in order, then the AOV channels / W.  develop=False: the raw AOV film."""
        torch = _torch()
        if _variant == SCALAR_VARIANT:
            raise RuntimeError("scalar_rgb: the `aov` integrator is not implemented by the scalar_rgb variant (hip_ad_rgb only)")
        sensor = self._sensor(scene, sensor)
        film = self.render_aov_film(scene, sensor, seed, spp)
        if not develop:
            out = film
        else:
            images = [c.render(scene, sensor, seed, spp, develop=True, evaluate=False) for c in self.children]
            weight = film[:, :, self.channels:]
            images.append(film[:, :, :self.channels] / torch.where(weight == 0, torch.ones_like(weight), weight))
            out = torch.cat(images, dim=2)
        if evaluate:
            torch.cuda.current_stream().synchronize()
        return out

    def sample(self, scene, *args, active=True):
        """AOVIntegratorImpl::sample (aov.cpp:175-306), array-valued: the C x n AOV values of the rays `ray` (mi.Ray3f; a sampler argument before it is accepted and
        not used -- the function draws nothing); masked and missed lanes are zero."""
        torch = _torch(); dev = _device()
        ray = args[-1]; n = len(ray)
        out = torch.empty((self.channels, n), dtype=torch.float32, device=dev)
        mask = _mask(active, n)          # kept alive across the call (see Integrator.sample)
        check(lib().har_aov_sample(scene._handle(), n, _ptr(ray.o), _ptr(ray.d), _ptr(ray.maxt), _ptr(mask), len(self.aov_types), self._types(), _ptr(out), _stream()))
        del mask
        return out

    def sample_host(self, scene, o, d, maxt, active=None):
        """the same function on the host (har_aov_sample_host; no GPU): o, d = 3 x n, maxt = n numpy arrays -> C x n"""
        o = np.ascontiguousarray(_f32(o)); d = np.ascontiguousarray(_f32(d)); maxt = np.ascontiguousarray(_f32(maxt)); n = maxt.shape[0]
        out = np.zeros((self.channels, n), np.float32)
        act = None if active is None else np.ascontiguousarray(np.asarray(active).astype(np.uint8))
        desc = scene.desc()
        check(lib().har_aov_sample_host(C.byref(desc), n, _fp(o), _fp(d), _fp(maxt), act.ctypes.data_as(C.c_void_p) if act is not None else None,
                                        len(self.aov_types), self._types(), _fp(out)))
        return out

    def _child_slices(self, sensor):
        per = 4 if sensor.film().alpha else 3
        return [(i * per, (i + 1) * per) for i in range(len(self.children))], per * len(self.children)

    def render_backward(self, scene, params, grad_in, sensor=0, seed=0, spp=0, lanes=None, weight_film=None):
        """split_channels (aov.cpp:620-637): every child gets its slice of the image gradient, the parameter gradients are summed over the children.  Gradients THROUGH
        the AOV channels are not implemented: a non-zero gradient on them is an error, never a silently incomplete result."""
        torch = _torch()
        sensor = self._sensor(scene, sensor)
        grad_in = torch.as_tensor(grad_in, dtype=torch.float32, device=_device())
        slices, first_aov = self._child_slices(sensor)
        if grad_in.shape[-1] != first_aov + self.channels:
            raise RuntimeError("aov.render_backward(): the gradient has %d channels, the image %d" % (grad_in.shape[-1], first_aov + self.channels))
        if bool((grad_in[..., first_aov:] != 0).any().item()):
            raise RuntimeError("aov: gradients through the AOV channels (%s) are not implemented by hip_ad_rgb -- the incoming gradient on them is not zero; "
                               "take the loss on the children's radiance channels only" % ", ".join(self._own_names))
        total = {}
        for child, (a, b) in zip(self.children, slices):
            g = child.render_backward(scene, params, grad_in[..., a:b].contiguous(), sensor, seed, spp, lanes=lanes, weight_film=weight_film)
            for k, v in g.items():
                total[k] = v if k not in total else total[k] + v
        return total

    def render_forward(self, *args, **kwargs):
        raise RuntimeError("render_forward(): the `aov` integrator is not implemented by hip_ad_rgb for forward-mode derivatives; use its `prb` child")

    def render_film(self, *args, **kwargs):
        raise RuntimeError("render_film(): the `aov` integrator has no {R, G, B, W} film; use render_aov_film() or its children")


class Bitmap:
    """Bitmap (src/core/bitmap.cpp) restricted to what HDRFilm::write needs: float32 H x W x {1,3,4}, write() to .exr / .pfm"""

    def __init__(self, array):
        if isinstance(array, (str, os.PathLike)):             # Bitmap(filename): OpenEXR (NO / ZIPS / ZIP) and PFM, read by the C++ host library
            img = _capi.HarImage()
            check(lib().har_image_read(str(array).encode(), C.byref(img)))
            try:
                array = np.ctypeslib.as_array(img.data, shape=(img.height, img.width, img.channels)).copy()
            finally:
                lib().har_image_free(C.byref(img))
        if hasattr(array, 'detach'):
            array = array.detach().cpu().numpy()
        a = _f32(array)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3:
            raise RuntimeError("Bitmap: expected an H x W x C array")
        self.data = np.ascontiguousarray(a)

    def size(self):
        return (self.data.shape[1], self.data.shape[0])

    def channel_count(self):
        return self.data.shape[2]

    def write(self, filename):
        h, w, c = self.data.shape
        ext = str(filename).lower().rsplit('.', 1)[-1]
        if ext == 'exr':
            check(lib().har_image_write_exr(str(filename).encode(), _fp(self.data), w, h, c))
        elif ext == 'pfm':
            check(lib().har_image_write_pfm(str(filename).encode(), _fp(self.data), w, h, c))
        else:
            raise RuntimeError("Bitmap.write(): unsupported file format \"%s\" (exr and pfm are implemented)" % ext)


def write_bitmap(filename, data):
    """mi.util.write_bitmap (src/python/python/util.py)"""
    Bitmap(data).write(filename)


# luminance() and srgb_to_xyz() (include/mitsuba/core/spectrum.h:439-442, 402-410): rows of the colour transform HDRFilm::develop applies for `luminance*` / `xyz*` films
_COLOUR_ROWS = {0: None, 1: ((0.212671, 0.715160, 0.072169),),
                2: ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))}


def develop_film(film, alpha_film=None, colour=0):
    """HDRFilm::develop (hdrfilm.cpp:301-404): colour / W -- RGB, Y = luminance(rgb) or XYZ = srgb_to_xyz(rgb) by the film's pixel format -- and A / W for films with
    an alpha channel (alpha_film: channel 3 holds the accumulated w * alpha)"""
    torch = _torch()
    h, w, _ = film.shape
    img = torch.empty((h, w, 1 if colour == 1 else 3), dtype=torch.float32, device=film.device)
    check(lib().har_film_develop_format(_ptr(film), w, h, int(colour), _ptr(img), _stream()))
    if alpha_film is None:
        return img
    weight = film[:, :, 3:4]
    a = alpha_film[:, :, 3:4] / torch.where(weight == 0, torch.ones_like(weight), weight)
    return torch.cat([img, a], dim=2)


# ---------------------------------------------------------------------------
#  Scene
# ---------------------------------------------------------------------------

def _static_table(fn):
    """the key tables of a scene (which parameters exist, under which names) are fixed at construction: built once (an optimisation loop asks every step)"""
    name = "_memo" + fn.__name__

    def get(self):
        t = self.__dict__.get(name)
        if t is None:
            t = self.__dict__[name] = fn(self)
        return t
    get.__name__ = fn.__name__; get.__doc__ = fn.__doc__
    return get


class Scene:
    """Scene (src/render/scene.cpp): owns the flat SceneIR arrays and the device accel."""

    def __init__(self, children):
        self.bsdf_objs = []; self.meshes = []; self.top_mesh_count = 0
        self.groups = []; self.instances = []; self.instance_keys = []; self.emitters = []
        self.m_sensors = []; self.sensor_keys = []; self.m_integrator = None; self.textures = []; self.texture_modes = []; self.texture_to_uv = []
        self._h = None; self._keep = []
        self._attr_tex = {}           # texture index -> (mesh index, attribute name, BSDF): the `mesh_attribute` records, one per (BSDF, shape) pair
        self._device_attrs = {}       # (mesh index, name) -> device tensor: attribute values params.update() pushed device-to-device (sync_host refreshes the mirrors)
        self._device_values = {}      # (kind, index) -> (device tensor, record): values params.update() pushed device-to-device; the numpy mirrors are refreshed by sync_host()
        named = {}
        shapes = []; groups = []; insts = []
        # Scene::emitters() order = declaration order of the children (scene.cpp:40-70): shapes with an area emitter and
        # stand-alone emitters; the uniform emitter selection of sample_emitter() depends on it
        self._emitter_order = [key for key, obj in children.items()
                               if (isinstance(obj, Mesh) and obj.emitter is not None) or isinstance(obj, (ConstantEmitter, EnvmapEmitter, PointLight, SpotLight, DirectionalEmitter, Projector))]
        self.emitters = [None] * len(self._emitter_order)
        if sum(isinstance(o, (ConstantEmitter, EnvmapEmitter)) for o in children.values()) > 1:
            raise RuntimeError("Only one environment emitter can be specified per scene.")
        for key, obj in children.items():
            if isinstance(obj, ConstantEmitter):
                self.emitters[self._emitter_order.index(key)] = dict(type=1, mesh=0xffffffff, radiance=obj.radiance, to_world=[0.0] * 12,
                                                                     normal=[0.0] * 3, inv_area=0.0, sampling_weight=obj.sampling_weight)
            elif isinstance(obj, PointLight):                   # HarEmitter type 4: `radiance` = intensity, to_world[9..11] = position
                self.emitters[self._emitter_order.index(key)] = dict(type=4, mesh=0xffffffff, radiance=obj.intensity,
                                                                     to_world=[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] + [float(x) for x in obj.position],
                                                                     normal=[0.0] * 3, inv_area=0.0, sampling_weight=obj.sampling_weight)
            elif isinstance(obj, SpotLight):                    # HarEmitter type 5: transform + inverse, normal = (cutoff_angle, beam_width, -) in degrees
                self.emitters[self._emitter_order.index(key)] = dict(type=5, mesh=0xffffffff, radiance=obj.intensity, to_world=obj.to_world.col_major_3x4(),
                                                                     to_local=obj.to_world.inverse().col_major_3x4(),
                                                                     normal=[obj.cutoff_angle, obj.beam_width, 0.0], inv_area=0.0, sampling_weight=obj.sampling_weight)
            elif isinstance(obj, DirectionalEmitter):           # HarEmitter type 6: `radiance` = irradiance, the transform (light travels along its +z)
                self.emitters[self._emitter_order.index(key)] = dict(type=6, mesh=0xffffffff, radiance=obj.irradiance, to_world=obj.to_world.col_major_3x4(),
                                                                     to_local=obj.to_world.inverse().col_major_3x4(), normal=[0.0] * 3, inv_area=0.0, sampling_weight=obj.sampling_weight)
            elif isinstance(obj, Projector):                    # HarEmitter type 8: transform + inverse, normal = (scale, x_fov, -), the bitmap in the texture table
                tex = 0xffffffff
                if obj.texture is not None:
                    tex = obj.tex_index = len(self.textures)
                    self.textures.append(obj.texture); self.texture_modes.append(obj.tex_mode); self.texture_to_uv.append(obj.tex_to_uv)
                self.emitters[self._emitter_order.index(key)] = dict(type=8, mesh=0xffffffff, radiance=obj.irradiance, to_world=obj.to_world.col_major_3x4(),
                                                                     to_local=obj.to_world.inverse().col_major_3x4(), normal=[obj.scale, obj.x_fov, 0.0], inv_area=0.0,
                                                                     sampling_weight=obj.sampling_weight, radiance_texture=tex, light=obj if obj.texture is not None else None)
            elif isinstance(obj, EnvmapEmitter):                # the radiance image travels in the texture table
                self.emitters[self._emitter_order.index(key)] = dict(
                    type=2, mesh=len(self.textures), radiance=[obj.scale, 1.0 if obj.mis_compensation else 0.0, 0.0],
                    to_world=obj.to_world.col_major_3x4(), to_local=obj.to_world.inverse().col_major_3x4(), normal=[0.0] * 3, inv_area=0.0, sampling_weight=obj.sampling_weight)
                self.textures.append(obj.data); self.texture_modes.append(0); self.texture_to_uv.append(None)
        for key, obj in children.items():
            if isinstance(obj, BSDF):
                named[key] = obj
                if obj.id is None:
                    obj.id = key
                self._add_bsdf(obj)
        for key, obj in children.items():
            if isinstance(obj, Sensor):
                self.m_sensors.append(obj); self.sensor_keys.append(key)
            elif isinstance(obj, Integrator):
                self.m_integrator = obj
            elif isinstance(obj, Mesh):
                shapes.append((key, obj))
            elif isinstance(obj, ShapeGroup):
                groups.append((key, obj))
            elif isinstance(obj, Instance):
                insts.append((key, obj))
        for key, m in shapes:
            self._add_mesh(key, m)
        self.top_mesh_count = len(self.meshes)
        self._in_group = True
        gindex = {}
        for key, g in groups:
            first = len(self.meshes)
            for i, m in enumerate(g.shapes):
                if m.emitter is not None:
                    raise RuntimeError("Instancing of emitters is not supported")
                self._add_mesh("%s.%s" % (key, g.keys[i]), m)
            gindex[id(g)] = len(self.groups)
            self.groups.append((first, len(self.meshes) - first))
        for key, it in insts:
            if id(it.group) not in gindex:
                raise RuntimeError("A reference to a 'shapegroup' must be specified!")
            self.instances.append((gindex[id(it.group)], it.to_world.col_major_3x4(), it.to_world.inverse().col_major_3x4()))
            self.instance_keys.append(key)

    # -- construction helpers
    def _add_bsdf(self, b):
        if b.scene is self:
            return b.index
        if getattr(b, 'attr', None) is not None:          # a `mesh_attribute` is bound per scene (Scene._bind_attributes): nothing of another scene's binding stays
            b.texture = None; b.attr_mesh = None
        b.scene = self; b.index = len(self.bsdf_objs)
        if b.texture is not None:
            b.tex_index = len(self.textures); self.textures.append(b.texture); self.texture_modes.append(b.tex_mode); self.texture_to_uv.append(b.tex_to_uv)
        for am in (getattr(b, 'alpha_maps', None) or {}).values():          # a roughness map is a texture of the scene that no colour slot names
            am.tex_index = len(self.textures); self.textures.append(am.texture); self.texture_modes.append(am.tex_mode); self.texture_to_uv.append(am.tex_to_uv)
        self.bsdf_objs.append(b)
        for c in getattr(b, 'nested', ()):           # blendbsdf: the nested BSDFs are records of their own (an object referenced from several places is lowered once)
            self._add_bsdf(c)
        if getattr(b, 'back', None) is not None:
            self._add_bsdf(b.back)
        return b.index

    @property
    def bsdfs(self):
        return self.bsdf_objs

    def _blend_nested(self):
        """ids of the BSDF objects whose record is nested in a blend record of this scene -- also one that a shape or another blend references besides"""
        out = {id(c) for b in self.bsdf_objs for c in getattr(b, 'nested', ())}
        return out | {id(c.back) for b in self.bsdf_objs if b.kind in ('mask', 'normalmap', 'bumpmap') for c in b.nested if c.back is not None}          # (mask: both sides of a nested `twosided` pair)

    def _add_mesh(self, key, m):
        if m.bsdf is None:          # Shape(props), shape.cpp:50-57: a default diffuse BSDF -- black when the shape carries an emitter
            m.bsdf = BSDF({'type': 'diffuse', 'reflectance': {'type': 'rgb', 'value': [0.0, 0.0, 0.0]}} if m.emitter is not None else None)
        if m.bsdf.scene is None:
            m.bsdf.id = key + ".bsdf"             # a BSDF nested in a shape (not a scene-level object): '<shape>.bsdf.reflectance.value' as in mi.traverse() (Shape::traverse registers it as "bsdf")
        bi = self._add_bsdf(m.bsdf)
        em = -1
        if m.emitter is not None:
            em = self._emitter_order.index(key)
            light = getattr(m, 'emitter_light', None)
            if light is not None and light.texture is not None:
                if not hasattr(m, 'rect'):
                    raise RuntimeError("area: a bitmap `radiance` is implemented on `rectangle` shapes (Rectangle::eval_parameterization, src/shapes/rectangle.cpp:215-237); on a "
                                       "triangle mesh the reference maps the sampled uv through Mesh::eval_parameterization (a ray cast against the mesh in uv space, "
                                       "src/render/mesh.cpp), which hip_ad_rgb does not have")
                light.tex_index = len(self.textures); self.textures.append(light.texture); self.texture_modes.append(light.tex_mode); self.texture_to_uv.append(light.tex_to_uv)
                self.emitters[em] = dict(type=7, mesh=len(self.meshes), radiance=[0.0, 0.0, 0.0], to_world=m.rect['to_world'].col_major_3x4(), normal=m.rect['normal'],
                                         inv_area=m.rect['inv_area'], sampling_weight=getattr(m, 'emitter_weight', 1.0), radiance_texture=light.tex_index, light=light)
            elif hasattr(m, 'rect'):        # Rectangle::sample_position (analytic parameterisation)
                self.emitters[em] = (dict(type=0, mesh=len(self.meshes), radiance=m.emitter, to_world=m.rect['to_world'].col_major_3x4(),
                                          normal=m.rect['normal'], inv_area=m.rect['inv_area'], sampling_weight=getattr(m, 'emitter_weight', 1.0)))
            else:                         # any other triangle mesh: Mesh::sample_position (area-weighted face selection)
                self.emitters[em] = dict(type=3, mesh=len(self.meshes), radiance=m.emitter, to_world=[0.0] * 12, normal=[0.0] * 3, inv_area=0.0,
                                         sampling_weight=getattr(m, 'emitter_weight', 1.0))
        if m.bsdf.kind == 'normalmap' and (m.flags & 3) == 3 and not hasattr(m, 'rect'):
            # the perturbation is relative to the shading frame, which such a mesh builds from packed per-vertex tangents in the reference (mesh.cpp:612-623, 1269-1350):
            # rendering it with another frame would be a silent parity error
            raise RuntimeError("normalmap: shape \"%s\" has vertex normals and texture coordinates -- under a `normalmap` its shading frame needs per-vertex tangents "
                               "(Mesh::compute_tangents), which are not implemented in hip_ad_rgb; a `rectangle`, and meshes without vertex normals or without texture "
                               "coordinates, are supported" % key)
        attrs = {k: np.ascontiguousarray(v, np.float32).copy() for k, v in getattr(m, 'attributes', {}).items()}
        self._bind_attributes(key, m.bsdf, attrs, len(self.meshes))
        self.meshes.append(dict(key=key, V=np.ascontiguousarray(m.V), F=np.ascontiguousarray(m.F), bsdf=bi, emitter=em, flags=m.flags, rect=getattr(m, 'rect', None), attributes=attrs))

    def _tangent_flags(self, m):
        """HAR_MESH_TANGENT_FRAME / HAR_MESH_FRAME_FLIPPED of a mesh under a `normalmap` (BSDFFlags::NormalMapped: the shape packs a tangent).  A rectangle's is the direction of
        to_world * (1, 0, 0) at all four vertices (rectangle.cpp:131-153); its FaceUVFlipped bit is toggled by a mirroring to_world, the scale(1, 1, -1) of `flip_normals`
        included (mesh.cpp:1160-1215).  Taken from the rectangle's current record, so it follows '<rectangle>.to_world' updates."""
        if self.bsdf_objs[m["bsdf"]].kind != 'normalmap' or m.get("rect") is None:
            return 0
        det = float(np.linalg.det(np.asarray(m["rect"]["to_world"].matrix, np.float32)[:3, :3]))
        return 4 | (8 if (det < 0.0) != bool(m["rect"].get("flip")) else 0)

    @staticmethod
    def _bsdf_tree(b):
        """the BSDF objects a shape's BSDF evaluates: itself, the back side of a `twosided`, the BSDFs nested in a blend / mask (and their back sides)"""
        out = []; todo = [b]
        while todo:
            x = todo.pop(0)
            if x is None or any(x is y for y in out):
                continue
            out.append(x); todo.extend(getattr(x, 'nested', ())); todo.append(getattr(x, 'back', None))
        return out

    @staticmethod
    def _attr_rows(b, values):
        """the rows x 1 x 3 record of a `mesh_attribute` in slot 0 of BSDF `b`.  A colour (Texture::eval -> Mesh::eval_attribute, mesh.cpp:2603-2617): one channel is
        broadcast, three are the colour, anything else is 0.  A blend weight / mask opacity (eval_1, :2619-2624): the value of a one-channel attribute, else 0."""
        v = np.asarray(values, np.float32); rows, dim = v.shape
        if dim == 1:
            t = np.repeat(v, 3, axis=1)
        elif dim == 3 and b.kind not in _WEIGHTED_BSDFS:
            t = v
        else:
            t = np.zeros((rows, 3), np.float32)
        return np.ascontiguousarray(t.reshape(rows, 1, 3), np.float32)

    def _bind_attributes(self, key, bsdf, attrs, mesh_index):
        """The attribute a `mesh_attribute` texture reads belongs to the shape that was hit (mesh_attribute.cpp:94-107: si.shape->eval_attribute): every BSDF of this
        shape's tree that holds one gets a texture record of THIS shape's rows.  A BSDF object carries one record, so a BSDF with such a texture that several shapes
        share is refused by name (docs/widening.md); a shape without the attribute is an error here, not a zero at render time."""
        for b in self._bsdf_tree(bsdf):
            if getattr(b, 'attr', None) is None:
                continue
            name, scale = b.attr
            who = self._bsdf_key_base(b) if b.id or b.index is not None else b.kind
            if getattr(self, '_in_group', False):
                raise RuntimeError("mesh_attribute: shape \"%s\" lies inside a shapegroup -- a `mesh_attribute` texture (\"%s\", BSDF \"%s\") on an instanced mesh is not supported in hip_ad_rgb" % (key, name, who))
            if b.attr_mesh is not None:
                raise RuntimeError("mesh_attribute: BSDF \"%s\" reads the attribute \"%s\" of the shape it is on, and the shapes \"%s\" and \"%s\" share it -- not supported in "
                                   "hip_ad_rgb: give every shape a BSDF of its own" % (who, name, self.meshes[b.attr_mesh]["key"], key))
            if name not in attrs:
                raise RuntimeError("mesh_attribute: shape \"%s\" has no attribute \"%s\" (read by BSDF \"%s\"); it has %s" % (key, name, who, sorted(attrs) or "none"))
            self._add_bsdf(b)          # (already a record of this scene: Scene._add_mesh added the shape's whole tree, without a texture)
            b.attr_mesh = mesh_index
            b.texture = self._attr_rows(b, attrs[name]); b.tex_mode = 8 | (0 if name.startswith("vertex_") else 16); b.tex_to_uv = [scale, 0.0, 0.0, 0.0, 0.0, 0.0]
            b.tex_index = len(self.textures); self.textures.append(b.texture); self.texture_modes.append(b.tex_mode); self.texture_to_uv.append(b.tex_to_uv)
            self._attr_tex[b.tex_index] = (mesh_index, name, b)

    def sync_host(self):
        """refresh the host mirrors (Scene.textures, BSDF.value / .texture, emitters[i]['radiance']) from the values params.update() pushed device-to-device"""
        for (kind, idx), (t, b) in list(self._device_values.items()):
            v = t.detach().to("cpu").numpy().astype(np.float32)
            if kind == "emit":
                self.emitters[idx]["radiance"] = np.ascontiguousarray(v.reshape(3))
            elif kind == "tex":
                b.texture = np.ascontiguousarray(v.reshape(b.texture.shape)); self.textures[idx] = b.texture
            else:
                b.value = np.ascontiguousarray(v.reshape(3))
        self._device_values.clear()
        for (mesh, name), t in list(self._device_attrs.items()):
            self.meshes[mesh]["attributes"][name] = np.ascontiguousarray(t.detach().to("cpu").numpy().astype(np.float32).reshape(self.meshes[mesh]["attributes"][name].shape))
        self._device_attrs.clear()
        self._sync_host_geometry()

    def _sync_host_geometry(self):
        """the packed vertex records of the meshes whose positions were updated ON THE DEVICE (har_scene_update_vertices_device): positions and regenerated normals
        back into meshes[i]['V'] -- needed before anything rebuilds the scene from the host mirrors or reads them"""
        stale = getattr(self, "_stale_meshes", None)
        if stale:
            if self._h is not None:
                for i in sorted(stale):
                    V = self.meshes[i]["V"] = np.ascontiguousarray(self.meshes[i]["V"], np.float32)
                    check(lib().har_scene_get_vertices(self._h, int(i), _fp(V), _stream()))
            stale.clear()
        if getattr(self, "_stale_instances", False):       # to_world / to_object of the instances were updated on the device (har_scene_update_instances_device)
            if self._h is not None and self.instances:
                n = len(self.instances)
                tw = np.zeros((n, 12), np.float32); to = np.zeros((n, 12), np.float32)
                check(lib().har_scene_get_instances(self._h, 0, n, _fp(tw), _fp(to), _stream()))
                self.instances = [(self.instances[i][0], [float(x) for x in tw[i]], [float(x) for x in to[i]]) for i in range(n)]
            self._stale_instances = False

    def _drop_handle(self, keep_geometry=True):
        """the next render builds a new scene handle from the host mirrors: bring them up to date first.  When the handle is dropped BECAUSE an update failed
        (keep_geometry=False), what the device-resident updates before the failing one wrote is still valid and is read back as well -- except vertex records that are
        not finite (the update a late "not finite" reports): that mesh keeps its last valid mirror.  (Instances: the device keeps the old transform of a singular one.)"""
        if self._h is None:
            return
        if keep_geometry:
            self._sync_host_geometry()
        else:
            for i in sorted(getattr(self, "_stale_meshes", ())):
                V = np.array(self.meshes[i]["V"], np.float32)
                if lib().har_scene_get_vertices(self._h, int(i), _fp(V), _stream()) == 0 and np.isfinite(V).all():
                    self.meshes[i]["V"] = V
            getattr(self, "_stale_meshes", set()).clear()
            if getattr(self, "_stale_instances", False) and self.instances:
                n = len(self.instances)
                tw = np.zeros((n, 12), np.float32); to = np.zeros((n, 12), np.float32)
                if lib().har_scene_get_instances(self._h, 0, n, _fp(tw), _fp(to), _stream()) == 0 and np.isfinite(tw).all() and np.isfinite(to).all():
                    self.instances = [(self.instances[i][0], [float(x) for x in tw[i]], [float(x) for x in to[i]]) for i in range(n)]
            self._stale_instances = False
            self._update_failures = getattr(self, "_update_failures", 0) + 1       # (SceneParameters._changed_keys: keys it remembers as applied are looked at again)
        lib().har_scene_destroy(self._h); self._h = None

    # -- C ABI description
    def desc(self):
        self.sync_host()
        M = _capi
        meshes = (M.HarMesh * max(1, len(self.meshes)))()
        for i, m in enumerate(self.meshes):
            meshes[i].vertex_ptr = _fp(m["V"]); meshes[i].index_ptr = _up(m["F"])
            meshes[i].vertex_count = m["V"].shape[0]; meshes[i].face_count = m["F"].shape[0]
            meshes[i].bsdf = m["bsdf"]; meshes[i].emitter = m["emitter"]; meshes[i].flags = m["flags"] | self._tangent_flags(m)
        groups = (M.HarShapeGroup * max(1, len(self.groups)))()
        for i, (a, b) in enumerate(self.groups):
            groups[i].first_mesh = a; groups[i].mesh_count = b
        insts = (M.HarInstance * max(1, len(self.instances)))()
        for i, (g, tw, to) in enumerate(self.instances):
            insts[i].group = g
            insts[i].to_world = (C.c_float * 12)(*[float(x) for x in tw]); insts[i].to_object = (C.c_float * 12)(*[float(x) for x in to])
        bsdfs = (M.HarBSDF * max(1, len(self.bsdf_objs)))()
        for i, b in enumerate(self.bsdf_objs):
            bsdfs[i].type = BSDF_TYPES[b.kind]; bsdfs[i].texture = b.tex_index if b.texture is not None else -1
            bsdfs[i].reflectance = (C.c_float * 3)(*[float(x) for x in b.value])
            bsdfs[i].flags = b.flags; bsdfs[i].reflectance2 = (C.c_float * 3)(*[float(x) for x in b.value2])
            bsdfs[i].alpha_u = b.alpha_u; bsdfs[i].alpha_v = b.alpha_v; bsdfs[i].eta = b.eta
            bsdfs[i].eta_c = (C.c_float * 3)(*[float(x) for x in b.eta_c]); bsdfs[i].k_c = (C.c_float * 3)(*[float(x) for x in b.k_c])
            bsdfs[i].back = b.back.index if b.back is not None else -1
            if b.kind == 'blendbsdf':
                bsdfs[i].nested = (C.c_int32 * 2)(b.nested[0].index, b.nested[1].index)
            elif b.kind in ('mask', 'normalmap', 'bumpmap'):
                bsdfs[i].nested = (C.c_int32 * 2)(b.nested[0].index, -1)
            elif getattr(b, 'alpha_maps', None):          # HAR_BSDF_ALPHA_TEX: the texture indices of alpha_u / alpha_v (-1: that axis is a float)
                mu = b.alpha_maps.get('alpha', b.alpha_maps.get('alpha_u')); mv = b.alpha_maps.get('alpha', b.alpha_maps.get('alpha_v'))
                bsdfs[i].nested = (C.c_int32 * 2)(mu.tex_index if mu is not None else -1, mv.tex_index if mv is not None else -1)
        texs = (M.HarTexture * max(1, len(self.textures)))()
        for i, t in enumerate(self.textures):
            texs[i].data = _fp(t); texs[i].height = t.shape[0]; texs[i].width = t.shape[1]; texs[i].mode = self.texture_modes[i] if i < len(self.texture_modes) else 0
            if i in self._attr_tex:               # a `mesh_attribute` record (HAR_TEX_MESH_ATTRIBUTE): the mesh it belongs to; its `scale` rides in to_uv[0]
                texs[i].reserved = self._attr_tex[i][0]
            if i < len(self.texture_to_uv) and self.texture_to_uv[i] is not None:
                texs[i].to_uv = (C.c_float * 6)(*self.texture_to_uv[i])
        ems = (M.HarEmitter * max(1, len(self.emitters)))()
        for i, e in enumerate(self.emitters):
            self._fill_emitter_record(ems[i], e)
        d = M.HarSceneDesc()
        d.meshes = meshes; d.mesh_count = len(self.meshes); d.top_mesh_count = self.top_mesh_count
        d.groups = groups; d.group_count = len(self.groups)
        d.instances = insts; d.instance_count = len(self.instances)
        d.bsdfs = bsdfs; d.bsdf_count = len(self.bsdf_objs)
        d.textures = texs; d.texture_count = len(self.textures)
        d.emitters = ems; d.emitter_count = len(self.emitters)
        self._keep = [meshes, groups, insts, bsdfs, texs, ems]
        return d

    @staticmethod
    def _fill_emitter_record(rec, e):
        rec.type = e.get("type", 0); rec.mesh = e["mesh"]
        rec.radiance = (C.c_float * 3)(*[float(x) for x in e["radiance"]])
        rec.to_world = (C.c_float * 12)(*[float(x) for x in e["to_world"]])
        rec.normal = (C.c_float * 3)(*[float(x) for x in e["normal"]]); rec.inv_area = float(e["inv_area"])
        rec.to_local = (C.c_float * 12)(*[float(x) for x in e.get("to_local", [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])])
        rec.sampling_weight = float(e.get("sampling_weight", 1.0)); rec.radiance_texture = int(e.get("radiance_texture", 0))

    def _handle(self):
        if self._h is None:
            _device()
            d = self.desc(); h = C.c_void_p()
            check(lib().har_scene_create(C.byref(d), C.byref(h)))
            self._h = h
        return self._h

    def __del__(self):
        try:
            if self._h is not None:
                lib().har_scene_destroy(self._h)
        except Exception:
            pass

    # -- reference API
    def sensors(self):
        return self.m_sensors

    def integrator(self):
        return self.m_integrator

    def shapes(self):
        return self.meshes

    def accel_info(self):
        info = (C.c_uint64 * 4)()
        check(lib().har_scene_accel_info(self._handle(), info))
        return dict(nodes=info[0], triangles=info[1], bytes=info[2], depth=info[3])

    def _intersect(self, ray, naive, active=True):
        torch = _torch(); dev = _device(); n = len(ray)
        t = torch.empty(n, dtype=torch.float32, device=dev); u = torch.empty_like(t); v = torch.empty_like(t)
        prim = torch.empty(n, dtype=torch.int32, device=dev); shape = torch.empty_like(prim); inst = torch.empty_like(prim)
        mask = _mask(active, n)          # kept alive across the call (see Integrator.sample)
        check(lib().har_ray_intersect_preliminary(self._handle(), n, _ptr(ray.o), _ptr(ray.d), _ptr(ray.maxt), _ptr(mask), 1 if naive else 0,
                                                  _ptr(t), _ptr(u), _ptr(v), _ptr(prim), _ptr(shape), _ptr(inst), _stream()))
        return PreliminaryIntersection3f(self, t, u, v, prim, shape, inst)

    def ray_intersect_preliminary(self, ray, coherent=False, reorder=False, reorder_hint=0, reorder_hint_bits=0, active=True):
        """Scene::ray_intersect_preliminary (scene.cpp:216-230).  coherent / reorder* are scheduling hints of the reference's backends (DRJIT_MARK_USED)."""
        return self._intersect(ray, False, active)

    def _intersect_si(self, ray, ray_flags, active, naive):
        torch = _torch(); dev = _device(); n = len(ray)
        t = torch.empty(n, dtype=torch.float32, device=dev); u = torch.empty_like(t); v = torch.empty_like(t)
        prim = torch.empty(n, dtype=torch.int32, device=dev); shape = torch.empty_like(prim); inst = torch.empty_like(prim)
        out = torch.empty((33, n), dtype=torch.float32, device=dev)
        flags = RayFlags.Default if ray_flags is None else int(ray_flags)
        mask = _mask(active, n)          # kept alive across the call (see Integrator.sample)
        check(lib().har_ray_intersect(self._handle(), n, _ptr(ray.o), _ptr(ray.d), _ptr(ray.maxt), flags, _ptr(mask), 1 if naive else 0,
                                      _ptr(t), _ptr(u), _ptr(v), _ptr(prim), _ptr(shape), _ptr(inst), _ptr(out), _stream()))
        si = SurfaceInteraction3f(out)
        si.prim_index = prim; si.shape_index = shape; si.instance = inst
        return si

    def ray_intersect(self, ray, ray_flags=None, coherent=False, reorder=False, reorder_hint=0, reorder_hint_bits=0, active=True):
        """Scene::ray_intersect(ray, ray_flags, coherent, ..., active) (scene.cpp:197-214)"""
        return self._intersect_si(ray, ray_flags, active, False)

    def ray_intersect_naive(self, ray, active=True):
        return self._intersect_si(ray, None, active, True)

    def ray_test(self, ray, coherent=False, active=True, naive=False):
        torch = _torch(); dev = _device(); n = len(ray)
        hit = torch.empty(n, dtype=torch.uint8, device=dev)
        mask = _mask(active, n)          # kept alive across the call (see Integrator.sample)
        check(lib().har_ray_test(self._handle(), n, _ptr(ray.o), _ptr(ray.d), _ptr(ray.maxt), _ptr(mask), 1 if naive else 0, _ptr(hit), _stream()))
        return hit.bool()

    def _compute_si(self, ray, pi, ray_flags=1, active=True):
        torch = _torch(); dev = _device(); n = len(ray)
        out = torch.empty((33, n), dtype=torch.float32, device=dev)
        mask = _mask(active, n)          # kept alive across the call (see Integrator.sample)
        check(lib().har_compute_surface_interaction(self._handle(), n, _ptr(ray.o), _ptr(ray.d), _ptr(pi.t), _ptr(pi.prim_uv[0]), _ptr(pi.prim_uv[1]),
                                                    _ptr(pi.prim_index), _ptr(pi.shape_index), _ptr(pi.instance), int(ray_flags), _ptr(mask),
                                                    _ptr(out), _stream()))
        return SurfaceInteraction3f(out)

    # -- parameters (mi.traverse)
    @staticmethod
    def _bsdf_key_base(b):
        """the prefix of a BSDF's parameters in mi.traverse(): its id -- the scene-level key, or '<shape>.bsdf' -- and, for the BSDFs nested in a `twosided`, the names
        TwoSidedBRDF::traverse registers them under (twosided.cpp:106-109): '<twosided>.brdf_0' and, when the back side is a BSDF of its own, '<twosided>.brdf_1'
        (util.py:320-334 walks an object once, so a twosided with ONE nested BSDF has no brdf_1 entries)"""
        bp = getattr(b, 'blend_parent', None)
        if bp is not None:          # nested in a blendbsdf (BlendBSDF::traverse, blendbsdf.cpp:102-106): '<blend>.bsdf_0' / '<blend>.bsdf_1'
            return Scene._bsdf_key_base(bp[0]) + ".bsdf_%d" % bp[1]
        mp = getattr(b, 'mask_parent', None)
        if mp is not None:          # nested in a mask (MaskBSDF::traverse, mask.cpp:116-119): '<mask>.nested_bsdf', under a nested `twosided` '<mask>.nested_bsdf.brdf_0'
            base = Scene._bsdf_key_base(mp) + ".nested_bsdf"
            return base + ".brdf_0" if (b.flags & 1) else base
        parent = getattr(b, 'twosided_parent', None)
        if parent is not None and getattr(parent, 'mask_parent', None) is not None:
            return Scene._bsdf_key_base(parent.mask_parent) + ".nested_bsdf.brdf_1"
        if parent is not None:
            return (parent.id if parent.id else "bsdf%d" % parent.index) + ".brdf_1"
        base = b.id if b.id else "bsdf%d" % b.index
        return base + ".brdf_0" if (b.flags & 1) else base

    @_static_table
    def _param_keys(self):
        keys = {}
        for b in self.bsdf_objs:
            base = self._bsdf_key_base(b)
            if getattr(b, 'attr', None) is not None:
                continue                   # a `mesh_attribute`: its values are the SHAPE's parameter '<shape>.<name>' (_attr_keys), its own is the `scale` (_attr_scale_keys)
            if getattr(b, 'given', None) is not None and b.slot0_name not in b.given:
                pass                       # a `thindielectric` without `specular_transmittance`: a null member, no entry (thindielectric.cpp:132-133)
            elif b.texture is not None:
                keys[base + "." + b.slot0_name + ".data"] = ("tex", b)
            else:
                keys[base + "." + b.slot0_name + ".value"] = ("rgb", b)
            for name, am in (getattr(b, 'alpha_maps', None) or {}).items():          # '<bsdf>.alpha.data' (BitmapTexture::traverse under roughconductor.cpp:216-220)
                keys[base + "." + name + ".data"] = ("tex", am)
        # emitter radiances: `<shape>.emitter.radiance.value` for area lights, `<emitter>.radiance.value` for `constant` (type 2 = envmap: none)
        for i, key in enumerate(self._emitter_order):
            e = self.emitters[i]
            if e.get("type", 0) in (0, 3):
                keys[key + ".emitter.radiance.value"] = ("emit", i)
            elif e["type"] == 1:
                keys[key + ".radiance.value"] = ("emit", i)
            elif e["type"] in (4, 5):                             # PointLight::traverse (point.cpp:84-88), SpotLight::traverse (spot.cpp:111-118): `intensity`
                keys[key + ".intensity.value"] = ("emit", i)
            elif e["type"] == 6:                                  # DirectionalEmitter::traverse (directional.cpp:93-97)
                keys[key + ".irradiance.value"] = ("emit", i)
            elif e["type"] == 8 and e.get("light") is None:       # Projector::traverse (projector.cpp:136-141): `irradiance` -- a uniform one here, a bitmap under _pose_keys
                keys[key + ".irradiance.value"] = ("emit", i)
        return keys

    @_static_table
    def _attr_keys(self):
        """'<shape>.<name>' -> (mesh index, name) of every mesh attribute (Mesh::traverse, src/render/mesh.cpp:844-845): a (rows, dim) tensor, differentiable"""
        return {m["key"] + "." + name: (i, name) for i, m in enumerate(self.meshes) for name in m.get("attributes", {})}

    @_static_table
    def _attr_scale_keys(self):
        """'<bsdf>.<slot>.scale' of the `mesh_attribute` textures (MeshAttribute::traverse, mesh_attribute.cpp:88-90: NonDifferentiable)"""
        return {self._bsdf_key_base(b) + "." + b.slot0_name + ".scale": b for b in self.bsdf_objs if getattr(b, 'attr', None) is not None}

    def _attr_readers(self, mesh, name):
        return [b for (mi_, n, b) in self._attr_tex.values() if mi_ == mesh and n == name]

    def _set_attribute(self, mesh, name, t, key):
        """params.update() of '<shape>.<name>': the host mirror, and the record of every BSDF that reads the attribute -- device-to-device when the tensor lives on the GPU"""
        shape = self.meshes[mesh]["attributes"][name].shape
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError("%s: expected a tensor of shape %s, got %s" % (key, tuple(shape), tuple(t.shape)))
        on_gpu = hasattr(t, "is_cuda") and t.is_cuda and self._h is not None
        if on_gpu:
            torch = _torch()
            v = t.detach().to(torch.float32).contiguous()
            self._device_attrs[(mesh, name)] = v.clone()
            for b in self._attr_readers(mesh, name):
                rows, dim = shape
                if dim == 1:
                    r = v.expand(rows, 3).contiguous()
                elif dim == 3 and b.kind not in _WEIGHTED_BSDFS:
                    r = v if v.data_ptr() != t.data_ptr() else v.clone()
                else:
                    r = torch.zeros((rows, 3), dtype=torch.float32, device=v.device)
                check(lib().har_scene_set_texture_device(self._h, b.tex_index, _ptr(r), _stream()))
                self._device_values[("tex", b.tex_index)] = (r, b)
            return
        v = t.detach().to("cpu").numpy().astype(np.float32) if hasattr(t, "detach") else np.asarray(t, np.float32)
        self._device_attrs.pop((mesh, name), None)
        self.meshes[mesh]["attributes"][name] = np.ascontiguousarray(v).copy()
        for b in self._attr_readers(mesh, name):
            self._device_values.pop(("tex", b.tex_index), None)
            b.texture = self._attr_rows(b, v); self.textures[b.tex_index] = b.texture
            if self._h is not None:
                check(lib().har_scene_set_texture(self._h, b.tex_index, _fp(b.texture)))

    def _set_attr_scale(self, b, value, key):
        v = np.asarray(value.detach().cpu().numpy() if hasattr(value, 'detach') else value, np.float32).reshape(-1)
        if v.size != 1 or not math.isfinite(float(v[0])):
            raise RuntimeError("%s: expected 1 finite value" % key)
        b.attr = (b.attr[0], float(v[0]))
        if b.texture is not None:
            b.tex_to_uv = [float(v[0]), 0.0, 0.0, 0.0, 0.0, 0.0]; self.texture_to_uv[b.tex_index] = b.tex_to_uv
            if self._h is not None:
                check(lib().har_scene_set_texture_to_uv(self._h, b.tex_index, (C.c_float * 6)(*b.tex_to_uv)))

    @_static_table
    def _bsdf_param_keys(self):
        """the non-slot-0 parameters of the rough models: '<bsdf>.alpha.value' (or alpha_u / alpha_v), '<bsdf>.eta.value', '<bsdf>.k.value' of
        roughconductor (roughconductor.cpp:212-225 traverse), '<bsdf>.alpha' and '<bsdf>.specular_reflectance.value' of roughplastic (roughplastic.cpp:208-215)"""
        keys = {}
        for b in self.bsdf_objs:
            base = self._bsdf_key_base(b)
            if b.kind == 'roughplastic':
                keys[base + ".alpha"] = ("alpha", b)                  # a Float member, not a texture: no '.value' (roughplastic.cpp:210, :534)
            elif b.kind == 'roughconductor':
                for name in (("alpha_u", "alpha_v") if b.anisotropic else ("alpha",)):          # (a roughness map shows '.data' / '.to_uv' instead: _param_keys, _pose_keys)
                    if name not in (getattr(b, 'alpha_maps', None) or {}):
                        keys[base + "." + name + ".value"] = (name, b)
            if b.kind == 'roughconductor':
                keys[base + ".eta.value"] = ("eta", b); keys[base + ".k.value"] = ("k", b)
            if b.kind == 'roughplastic' and b.slot1_name:
                keys[base + "." + b.slot1_name + ".value"] = ("slot1", b)
            if b.kind == 'bumpmap':
                keys[base + ".scale"] = ("scale", b)                  # BumpMap::traverse (bumpmap.cpp:134): a ScalarFloat, NonDifferentiable
            if b.kind == 'thindielectric':
                # ThinDielectric::traverse (thindielectric.cpp:130-136): `eta`, and `specular_reflectance` when it was given (slot 1 here)
                keys[base + ".eta"] = ("thin_ior", b)
                if b.slot1_name in b.given:
                    keys[base + "." + b.slot1_name + ".value"] = ("thin_r", b)
            if b.kind in ('dielectric', 'plastic', 'roughplastic'):
                # the relative index of refraction int_ior / ext_ior, a plain float: dielectric.cpp:238, plastic.cpp:185 (NonDifferentiable), roughplastic.cpp:211 (Differentiable
                # there; updatable without a gradient here)
                keys[base + ".eta"] = ("ior", b)
        return keys

    def _bsdf_param_value(self, what, b):
        return {"alpha": [b.alpha_u], "alpha_u": [b.alpha_u], "alpha_v": [b.alpha_v], "eta": b.eta_c, "k": b.k_c, "slot1": b.value2, "ior": [b.eta], "scale": [b.alpha_u], "thin_ior": [b.eta], "thin_r": b.value2}[what]

    def _set_bsdf_param(self, what, b, v):
        """params.update() of a non-slot-0 BSDF parameter: the record is re-lowered IN PLACE when a scene handle exists (har_scene_set_bsdf_params), else with the first handle (roughplastic's sampling weights and
        transmittance tables depend on alpha / the colours: RoughPlastic::parameters_changed, roughplastic.cpp:204-242)"""
        v = np.asarray(v, np.float32).reshape(-1)
        if what == "thin_r" and (np.any(v[:3] < 0) or np.any(v[:3] > 1) or not np.isfinite(v[:3]).all()):
            raise RuntimeError("Invalid RGB reflectance value %s, must be in the range [0, 1]!" % v[:3])
        if what in ("ior", "thin_ior"):              # Dielectric / SmoothPlastic / RoughPlastic::parameters_changed: Fresnel terms, plastic's internal reflectance and tables follow eta --
            if not (float(v[0]) > 0.0) or not math.isfinite(float(v[0])) or (b.kind == 'roughplastic' and float(v[0]) == 1.0):      # all re-derived when the next scene handle lowers the record
                raise RuntimeError("The interior and exterior indices of refraction must be positive" + (" and differ!" if b.kind == 'roughplastic' else "!"))
            b.eta = float(v[0])
            self._drop_handle()
            return
        if what == "scale":
            if not math.isfinite(float(v[0])):
                raise RuntimeError("bumpmap: `scale` must be finite")
            b.alpha_u = b.alpha_v = float(v[0])
        elif what == "alpha":
            b.alpha_u = b.alpha_v = float(v[0])
        elif what == "alpha_u":
            b.alpha_u = float(v[0])
        elif what == "alpha_v":
            b.alpha_v = float(v[0])
        elif what == "eta":
            b.eta_c = _f32(v[:3])
        elif what == "k":
            b.k_c = _f32(v[:3])
        else:
            b.value2 = _f32(v[:3])
        if self._h is not None:
            # the record is re-lowered IN PLACE (har_scene_set_bsdf_params: alpha / eta / k / slot 1 + roughplastic's table, internal reflectance, sampling weight); the scene
            # handle and the acceleration data survive -- rounds 3-5 rebuilt the whole scene for every step of a roughness optimisation
            rec = _capi.HarBSDF()
            rec.type = BSDF_TYPES[b.kind]; rec.flags = b.flags
            rec.reflectance2 = (C.c_float * 3)(*[float(x) for x in b.value2])
            rec.alpha_u = b.alpha_u; rec.alpha_v = b.alpha_v; rec.eta = b.eta
            rec.eta_c = (C.c_float * 3)(*[float(x) for x in b.eta_c]); rec.k_c = (C.c_float * 3)(*[float(x) for x in b.k_c])
            rc = lib().har_scene_set_bsdf_params(self._h, int(b.index), C.byref(rec))
            if rc != 0:
                msg = (lib().har_last_error() or b"").decode()
                self._drop_handle()
                raise RuntimeError(msg or "BSDF parameter update failed")

    @_static_table
    def _position_keys(self):
        """'<shape>.positions' (an N x 3 tensor: Mesh::traverse, src/render/mesh.cpp:827; a flat array of 3 N floats is accepted on write) of the top-level meshes and, as '<group>.<child>.positions', of the
        meshes inside shape groups (object space, shared by all instances); writing them regenerates the vertex normals of a smooth-shaded mesh (mesh.cpp:876-878),
        see _set_vertex_positions"""
        return {m["key"] + ".positions": i for i, m in enumerate(self.meshes) if m["V"].shape[0]}

    def _bsdf_has_smooth_lobe(self, index):
        """BSDFFlags::Smooth on every side: models made of delta lobes only (`dielectric`, `conductor`) cannot sit on MOVING geometry -- their eval() is zero,
        so prb.py:288 would form relative_grad(0) (har_integrator_set_grad_positions)"""
        b = self.bsdf_objs[index]
        delta = ("dielectric", "conductor", "thindielectric")
        return b.kind not in delta and (b.back is None or b.back.kind not in delta)

    def _differentiable_position_keys(self):
        """the subset of _position_keys() the `prb` adjoint can differentiate with `shape_gradients=True`: top-level meshes whose BSDF has a non-delta lobe (any of
        diffuse, roughconductor, roughplastic, plastic, plain or inside `twosided`) and, if they carry vertex normals, carry the REGENERATED ones (Mesh::compute_normals:
        what a position update produces, mesh.cpp:876-878) -- a mesh with normals of another origin is left out here and refused when named explicitly; the other
        meshes of the scene may carry any BSDF"""
        out = {}
        for k, i in self._position_keys().items():
            m = self.meshes[i]
            if i >= self.top_mesh_count:         # nested meshes exclude the instances' to_world (instance.cpp:162-166): only when named explicitly
                continue
            if not self._bsdf_has_smooth_lobe(m["bsdf"]):
                continue
            if (m["flags"] & 1) and i not in getattr(self, "_stale_meshes", ()):        # (a mesh updated on the device carries the normals that update regenerated)
                V = np.ascontiguousarray(m["V"]).copy(); F = np.ascontiguousarray(m["F"])
                check(lib().har_mesh_compute_normals(V.shape[0], _fp(V), F.shape[0], _up(F)))
                if np.abs(V[:, 3:6] - m["V"][:, 3:6]).max() > 1e-4:
                    continue
            out[k] = i
        return out

    @_static_table
    def _rect_keys(self):
        """'<rectangle>.to_world' (4 x 4, Rectangle::traverse, src/shapes/rectangle.cpp:197-200 -- the one entry that plugin registers besides its BSDF / emitter) of the
        top-level rectangles"""
        return {m["key"] + ".to_world": i for i, m in enumerate(self.meshes[:self.top_mesh_count]) if m.get("rect") is not None}

    def _rect_matrix(self, i):
        return np.asarray(self.meshes[i]["rect"]["to_world"].matrix, np.float32).reshape(4, 4).copy()

    def _set_rect_to_world(self, i, m4):
        """params['<rectangle>.to_world'] = ...; params.update(): Rectangle::parameters_changed (rectangle.cpp:202-214) re-initialises the shape from the new transform --
        here the four vertex records (positions, normal, uv), the winding, and for a rectangle that carries an area light its sampling record (frame, normal, 1 / area)
        are re-baked by the code that built them (har_shape_rectangle); the next render builds a new scene handle from them"""
        m4 = np.asarray(m4, np.float64).reshape(4, 4)
        if abs(np.linalg.det(m4[:3, :3])) == 0.0 or not np.isfinite(m4).all():
            raise RuntimeError("rectangle: 'to_world' is singular or not finite")
        tw = ScalarTransform4f(np.concatenate([m4.ravel(), np.linalg.inv(m4).T.ravel()]).astype(np.float32))
        mesh = self.meshes[i]; rect = mesh["rect"]
        V = np.empty((4, 8), np.float32); F = np.empty((2, 4), np.uint32); n = np.empty(3, np.float32); ia = C.c_float()
        check(lib().har_shape_rectangle(_fp(tw.data), 1 if rect.get("flip") else 0, _fp(V), _up(F), _fp(n), C.byref(ia)))
        self._drop_handle()
        mesh["V"], mesh["F"] = V, F
        rect.update(to_world=tw, normal=n, inv_area=ia.value)
        em = mesh["emitter"]
        if em >= 0:
            e = self.emitters[em]
            e["to_world"] = tw.col_major_3x4(); e["normal"] = n; e["inv_area"] = ia.value
        self._drop_handle()

    def _rect_frame(self, i, p):
        """the 'to_world' of rectangle i whose corners (-1, -1), (1, -1), (-1, 1), (1, 1) -- har_shape_rectangle's vertex order -- are the four positions `p`: the first two
        columns and the translation come from the corners; the third, which no corner reaches, is the unit normal of the new frame at the old column's length and
        orientation (T * to_world for any T that maps the plane's normal to the new plane's normal at the same length: rigid motions, stretches within the plane)"""
        p = np.asarray(p, np.float64).reshape(4, 3)
        key = self.meshes[i]["key"] + ".to_world"
        c = p.mean(axis=0); x = (p[1] - p[0] + p[3] - p[2]) / 4.0; y = (p[2] - p[0] + p[3] - p[1]) / 4.0
        n = np.cross(x, y); nn = np.linalg.norm(n)
        fit = np.stack([c - x - y, c + x - y, c - x + y, c + x + y])
        if not nn > 0.0 or np.abs(fit - p).max() > 1e-5 * max(np.abs(p).max(), np.linalg.norm(x), np.linalg.norm(y)):
            raise RuntimeError("%s.positions: the four vertices of a rectangle light must form a non-degenerate parallelogram (its sampling record is its frame); "
                               "move it through '%s'" % (self.meshes[i]["key"], key))
        old = self._rect_matrix(i).astype(np.float64)
        z = old[:3, 2]
        side = 1.0 if np.dot(np.cross(old[:3, 0], old[:3, 1]), z) >= 0.0 else -1.0
        m4 = np.eye(4)
        m4[:3, 0] = x; m4[:3, 1] = y; m4[:3, 2] = side * np.linalg.norm(z) * n / nn; m4[:3, 3] = c
        return m4

    @_static_table
    def _instance_keys(self):
        """'<instance>.to_world' (4 x 4, Instance::traverse, instance.cpp:79-85)"""
        return {k + ".to_world": i for i, k in enumerate(self.instance_keys)}

    def _set_instance_matrices_device(self, first, to_world):
        """params['<instance>.to_world'] as CUDA tensors + params.update(): `to_world` = device tensor (count, 12), column-major 3 x 4 rows for instances first .. first + count - 1.
        Inverses, shading / TLAS leaf records, instance bounds and the refit of the instance level are kernels on the current stream (har_scene_update_instances_device); the
        Python mirror self.instances is refreshed lazily (sync_host)."""
        torch = _torch()
        t = to_world.detach().to(torch.float32).contiguous()
        self._stale_instances = True
        self.device_instance_updates = getattr(self, "device_instance_updates", 0) + 1
        rc = lib().har_scene_update_instances_device(self._h, int(first), int(t.shape[0]), _ptr(t), _stream())
        if rc != 0:
            msg = (lib().har_last_error() or b"").decode()
            self._drop_handle(keep_geometry=False)
            raise RuntimeError(msg or "instance update failed")

    def _instance_matrix(self, i):
        self._sync_host_geometry()
        m = np.eye(4, dtype=np.float32); m[:3, :] = np.asarray(self.instances[i][1], np.float32).reshape(4, 3).T
        return m

    def _set_instance_matrix(self, i, m4):
        self._set_instance_matrices([(i, m4)])

    def _set_instance_matrices(self, items):
        """params['<instance>.to_world'] = ...; params.update(): the instance level of the acceleration structure is rebuilt IN PLACE (har_scene_update_instances:
        the bottom-level BVHs, the scene handle and every workspace stay; Scene::parameters_changed, scene.cpp:517-540 / scene_optix.inl:351-372) -- one call per
        run of consecutive instances"""
        self._sync_host_geometry()          # other instances may have moved on the device since: the mirror is read and rewritten below
        recs = {}
        for i, m4 in items:                 # every matrix is checked before the mirror takes any of them
            m = np.asarray(m4, np.float64).reshape(4, 4)
            if not np.isfinite(m).all() or np.linalg.det(m[:3, :3]) == 0.0:
                raise RuntimeError("instance transform is singular or not finite")
            inv = np.linalg.inv(m)
            recs[int(i)] = (_f32(m[:3, :].T.reshape(-1)), _f32(inv[:3, :].T.reshape(-1)))
        for i, (tw, to) in recs.items():
            self.instances[i] = (self.instances[i][0], [float(x) for x in tw], [float(x) for x in to])
        if self._h is None or not recs:
            return
        idx = sorted(recs); start = 0
        while start < len(idx):
            end = start
            while end + 1 < len(idx) and idx[end + 1] == idx[end] + 1:
                end += 1
            tw = np.ascontiguousarray(np.concatenate([recs[i][0] for i in idx[start:end + 1]]), np.float32)
            to = np.ascontiguousarray(np.concatenate([recs[i][1] for i in idx[start:end + 1]]), np.float32)
            rc = lib().har_scene_update_instances(self._h, idx[start], end - start + 1, _fp(tw), _fp(to), _stream())
            if rc != 0:          # the host mirror of the instance level may already differ from the device's: rebuild from self.instances at the next render
                msg = (lib().har_last_error() or b"").decode()
                self._drop_handle(keep_geometry=False)
                raise RuntimeError(msg or "instance update failed")
            start = end + 1

    def _set_vertex_positions(self, mesh, positions):
        """params['<shape>.positions'] = ... (a host tensor / array) + params.update(): normals regenerated on the host, the BLAS refitted on the device
        (har_scene_update_vertices); CUDA tensors take _set_vertex_positions_device instead"""
        V = self.meshes[mesh]["V"]
        p = np.asarray(positions, np.float32).reshape(V.shape[0], 3)
        if not np.isfinite(p).all():
            raise RuntimeError("%s.positions: a vertex position is not finite" % self.meshes[mesh]["key"])
        if self.meshes[mesh].get("rect") is not None and self.meshes[mesh]["emitter"] >= 0:
            # a rectangle light samples its frame, not its triangles (Rectangle::sample_position): the frame follows the positions, and the vertex records and the
            # sampling record are re-baked from it -- what '<rect>.to_world' reads back
            self._set_rect_to_world(mesh, self._rect_frame(mesh, p))
            return
        held = np.array(V, np.float32)        # a refused update (below) leaves the mirror as it was: the next scene handle is built from it
        V[:, :3] = p
        if self.meshes[mesh]["flags"] & 1:
            # Mesh::parameters_changed (mesh.cpp:876-878): pack(regenerate_normals = positions written and normals not) -> compute_normals (:1216-1267)
            F = np.ascontiguousarray(self.meshes[mesh]["F"])
            if not V.flags["C_CONTIGUOUS"]:
                V = self.meshes[mesh]["V"] = np.ascontiguousarray(V)
            check(lib().har_mesh_compute_normals(V.shape[0], _fp(V), F.shape[0], _up(F)))
        if self._h is not None:
            # the BLAS that holds the mesh is REFITTED on the device (har_scene_update_vertices); a new scene only when the library asks for one: the mesh carries
            # an emitter (its sampling records are lowered from the positions), or the refitted tree has degraded (HAR_UPDATE_REBUILD_ADVISED: still valid, but a
            # fresh build traces faster -- the next render creates it)
            Vc = np.ascontiguousarray(self.meshes[mesh]["V"], np.float32)
            getattr(self, "_stale_meshes", set()).discard(mesh)
            try:
                self._after_vertex_update(mesh, lib().har_scene_update_vertices(self._h, int(mesh), _fp(Vc), _stream()))
            except RuntimeError:
                # e.g. an instance level that no longer fits the traversal stacks: the handle is gone, and the scene goes on with the positions it held -- as after a
                # refused device-resident update, whose mirror was never written
                self.meshes[mesh]["V"] = held
                raise

    def _after_vertex_update(self, mesh, rc):
        """return codes of har_scene_update_vertices(_device): 2 / 3 = valid scene, but the next render needs / is better off with a new handle; anything else but 0 is an
        error AFTER the call may have touched the host mirror and the device arrays (allocation failure of the refit scratch, a HIP error mid-refit, a TLAS that no
        longer fits the traversal stacks): the handle is dropped so that the next render rebuilds from self.meshes instead of tracing a half-updated BVH"""
        if rc in (2, 3):
            if os.environ.get("HAR_VERBOSE"):
                import sys
                sys.stderr.write("[mitsuba3_amd] vertex update of mesh %d: %s -> new scene at the next render\n" % (mesh, (lib().har_last_error() or b"").decode() if rc == 2 else "refit cost ratio %.2f: rebuild advised" % self.refit_info()["ratio"]))
            self.accel_rebuilds = getattr(self, "accel_rebuilds", 0) + 1
            self._drop_handle()
        elif rc != 0:
            msg = (lib().har_last_error() or b"").decode()
            self._drop_handle(keep_geometry=False)
            raise RuntimeError(msg or "vertex update failed")

    def _set_vertex_positions_device(self, mesh, positions):
        """params['<shape>.positions'] (a CUDA tensor) + params.update(): the positions stay on the GPU -- vertex records, regenerated normals, shading triangles and the
        BLAS refit are kernels on the current stream (har_scene_update_vertices_device; Mesh::parameters_changed, mesh.cpp:848-899).  The numpy mirror meshes[mesh]['V'] is
        refreshed lazily (sync_host)."""
        torch = _torch()
        V = self.meshes[mesh]["V"]
        p = positions.detach().to(torch.float32).contiguous()
        if p.numel() != 3 * V.shape[0]:
            raise RuntimeError("positions: expected %d rows of 3 values" % V.shape[0])
        if self.meshes[mesh]["emitter"] >= 0:
            # the library refuses an emitter mesh before it writes anything (its sampling records are lowered from the positions): the host route, new scene included
            self._set_vertex_positions(mesh, p.cpu().numpy())
            return
        if not hasattr(self, "_stale_meshes"):
            self._stale_meshes = set()
        self.device_vertex_updates = getattr(self, "device_vertex_updates", 0) + 1
        self._keep_positions = p                  # alive until the kernels that read it were enqueued on this stream (they were: the call below enqueues them)
        rc = lib().har_scene_update_vertices_device(self._h, int(mesh), _ptr(p), _stream())
        if rc in (0, 3):                          # (3: HAR_UPDATE_REBUILD_ADVISED) the device arrays hold the new positions, the mirror does not yet
            self._stale_meshes.add(mesh)
        self._after_vertex_update(mesh, rc)

    def refit_info(self):
        """(refits since the scene handle was created, cost figure of the last refit, its ratio to the first refit's, nodes)"""
        info = (C.c_double * 4)()
        check(lib().har_scene_refit_info(self._handle(), info))
        return dict(refits=int(info[0]), cost=info[1], ratio=info[2], nodes=int(info[3]), rebuilds=getattr(self, "accel_rebuilds", 0))

    @_static_table
    def _pose_keys(self):
        """the NON-differentiable placement parameters the reference's traverse() exposes (ParamFlags::NonDifferentiable): '<sensor>.to_world' (perspective.cpp:177,
        orthographic.cpp:95), '<emitter>.position' of a point light (point.cpp:86), '<emitter>.to_world' of spot and directional lights (spot.cpp:117,
        directional.cpp:96) -- 4 x 4 matrices / a 3-vector; params.update() re-lowers the sensor or the scene"""
        keys = {}
        sensors = []
        for k, s in zip(self.sensor_keys, self.m_sensors):
            if s.kind == 'batch':        # BatchSensor::traverse (batch.cpp:273-282): the children under their names, each with its own sensor's entries
                sensors += [(k + "." + name, c) for name, c in zip(s.child_names, s.m_sensors)]
            else:
                sensors.append((k, s))
        for k, s in sensors:
            keys[k + ".to_world"] = ("sensor", s)
            if s.kind == 'thinlens':              # ThinLensCamera::traverse (thinlens.cpp:171-177)
                keys[k + ".aperture_radius"] = ("aperture_radius", s); keys[k + ".focus_distance"] = ("focus_distance", s); keys[k + ".x_fov"] = ("x_fov", s)
            elif s.kind != 'orthographic':        # PerspectiveCamera::traverse (perspective.cpp:155-160)
                keys[k + ".x_fov"] = ("x_fov", s)
                keys[k + ".principal_point_offset_x"] = ("ppo_x", s); keys[k + ".principal_point_offset_y"] = ("ppo_y", s)
        for i, key in enumerate(self._emitter_order):
            t = self.emitters[i].get("type", 0)
            if t == 4:
                keys[key + ".position"] = ("position", i)
            elif t in (5, 6):
                keys[key + ".to_world"] = ("emitter_to_world", i)
            elif t == 2:        # EnvironmentMapEmitter::traverse (envmap.cpp:204-208): `scale`, `to_world` -- updatable here (the record is rebuilt with the next scene handle);
                                # and so is `data`; `data` and `scale` are Differentiable: the `prb` integrator's `envmap_gradients` (switched on by mi.render for a key with
                                # requires_grad) produces their gradients
                keys[key + ".scale"] = ("env_scale", i); keys[key + ".to_world"] = ("emitter_to_world", i)
                keys[key + ".data"] = ("env_data", i)          # the texel tensor in the reference's layout: H x (W + 2) x 3, real column x at x + 1 (envmap.cpp:146-188)
            if t == 8:          # Projector::traverse (projector.cpp:136-141): `scale` (Differentiable: with the irradiance's gradient switch), `to_world` (NonDifferentiable);
                                # a bitmap irradiance: `data` (Differentiable: `light_texel_gradients`) and `to_uv`, BitmapTexture::traverse (bitmap.cpp:463-475)
                keys[key + ".scale"] = ("proj_scale", i); keys[key + ".to_world"] = ("emitter_to_world", i)
                if self.emitters[i].get("light") is not None:
                    keys[key + ".irradiance.data"] = ("emitter_tex", i); keys[key + ".irradiance.to_uv"] = ("emitter_to_uv", i)
            if t == 5:          # SpotLight::traverse (spot.cpp:115-116): the cone, in degrees -- updatable here; their gradient (the reference marks them Differentiable) is refused
                keys[key + ".cutoff_angle"] = ("cutoff_angle", i); keys[key + ".beam_width"] = ("beam_width", i)
            # Emitter::traverse (src/render/emitter.cpp:13): `sampling_weight`, NonDifferentiable; an area light is a child of its shape ('<shape>.emitter.*')
            keys[key + (".emitter" if t in (0, 3, 7) else "") + ".sampling_weight"] = ("sampling_weight", i)
            if t == 7:          # AreaLight::traverse -> "radiance" -> BitmapTexture::traverse: `data` and `to_uv` (bitmap.cpp:463-475).  `data` is Differentiable: the `prb`
                                # integrator's `light_texel_gradients` (switched on by mi.render for a key with requires_grad) produces its gradient
                keys[key + ".emitter.radiance.data"] = ("emitter_tex", i); keys[key + ".emitter.radiance.to_uv"] = ("emitter_to_uv", i)
        for b in self.bsdf_objs:            # BitmapTexture::traverse: `to_uv` (src/textures/bitmap.cpp), NonDifferentiable
            if b.texture is not None and getattr(b, 'attr', None) is None:          # (a `mesh_attribute` has no to_uv: its only own parameter is `scale`)
                keys[self._bsdf_key_base(b) + "." + b.slot0_name + ".to_uv"] = ("to_uv", b)
            for name, am in (getattr(b, 'alpha_maps', None) or {}).items():
                keys[self._bsdf_key_base(b) + "." + name + ".to_uv"] = ("to_uv", am)
        return keys

    def _pose_value(self, kind, b):
        if kind == "sensor":
            return np.asarray(b.to_world.matrix, np.float32).reshape(4, 4).copy()
        if kind == "x_fov":
            return np.asarray([b.x_fov()], np.float32)
        if kind in ("ppo_x", "ppo_y"):
            return np.asarray([float(b.props.get('principal_point_offset_' + kind[-1], 0.0))], np.float32)
        if kind == "aperture_radius":
            return np.asarray([b.aperture_radius], np.float32)
        if kind == "focus_distance":
            return np.asarray([b.focus_distance_], np.float32)
        if kind == "position":
            return np.asarray(self.emitters[b]["to_world"][9:12], np.float32).copy()
        if kind in ("cutoff_angle", "beam_width"):
            return np.asarray([self.emitters[b]["normal"][0 if kind == "cutoff_angle" else 1]], np.float32)
        if kind == "sampling_weight":
            return np.asarray([self.emitters[b].get("sampling_weight", 1.0)], np.float32)
        if kind == "env_scale":
            return np.asarray([self.emitters[b]["radiance"][0]], np.float32)
        if kind == "env_data":             # one halo column on each side carrying a copy of the opposite edge (envmap.cpp:146-188, refresh_halo)
            t = np.asarray(self.textures[self.emitters[b]["mesh"]], np.float32)
            return np.ascontiguousarray(np.concatenate([t[:, -1:], t, t[:, :1]], axis=1))
        if kind == "proj_scale":
            return np.asarray([self.emitters[b]["normal"][0]], np.float32)
        if kind == "emitter_tex":
            light = self.emitters[b]["light"]
            return np.array(light.texture[:, :, :1] if getattr(light, 'channels', 3) == 1 else light.texture, np.float32)
        if kind in ("to_uv", "emitter_to_uv"):
            if kind == "emitter_to_uv":
                b = self.emitters[b]["light"]
            m = np.eye(3, dtype=np.float32)
            if b.tex_to_uv is not None:
                m[:2, :] = np.asarray(b.tex_to_uv, np.float32).reshape(2, 3)
            return m
        m = np.eye(4, dtype=np.float32); m[:3, :] = np.asarray(self.emitters[b]["to_world"], np.float32).reshape(4, 3).T
        return m

    def _validate_spots(self):
        for e in self.emitters:                                      # SpotLight::update, spot.cpp:300-306
            if e.get("type") == 5 and not (e["normal"][0] >= e["normal"][1] and e["normal"][0] > 0):
                raise RuntimeError("spot: cutoff_angle must be positive and not smaller than beam_width")
        pending = self.__dict__.get("_emitters_to_push")
        if pending:                                                  # spot cones whose pair of angles is complete and valid: the record goes to the scene in place
            todo = sorted(pending); pending.clear()
            if self._h is not None:
                for b in todo:
                    self._push_delta_emitter(b)
        if getattr(self, "_weights_dirty", False):                   # Scene::parameters_changed -> update_emitter_sampling_distribution (scene.cpp:523-528)
            self._weights_dirty = False
            if self._h is not None:
                w = _f32([e.get("sampling_weight", 1.0) for e in self.emitters])
                check(lib().har_scene_set_emitter_sampling_weights(self._h, _fp(w), len(self.emitters)))

    def sample_emitter(self, index_sample, active=True):
        """Scene::sample_emitter(index_sample, active) -> (index, emitter_weight, reused sample) (src/render/scene.cpp:248-271), array-valued"""
        torch = _torch(); dev = _device()
        s = torch.as_tensor(index_sample, dtype=torch.float32, device=dev).reshape(-1).contiguous(); n = s.numel()
        index = torch.empty(n, dtype=torch.int32, device=dev); weight = torch.empty(n, dtype=torch.float32, device=dev); reused = torch.empty_like(weight)
        mask = _mask(active, n)
        check(lib().har_scene_sample_emitter(self._handle(), n, _ptr(s), _ptr(mask), _ptr(index), _ptr(weight), _ptr(reused), _stream()))
        return index, weight, reused

    def pdf_emitter(self, index, active=True):
        """Scene::pdf_emitter(index, active) (scene.cpp:273-279)"""
        torch = _torch(); dev = _device()
        i = torch.as_tensor(index, device=dev).to(torch.int32).reshape(-1).contiguous(); n = i.numel()
        pdf = torch.empty(n, dtype=torch.float32, device=dev)
        mask = _mask(active, n)
        check(lib().har_scene_pdf_emitter(self._handle(), n, _ptr(i), _ptr(mask), _ptr(pdf), _stream()))
        return pdf

    def _set_pose(self, kind, b, value):
        # validate first, assign last: a rejected value leaves the scene (and the params entry's counterpart) as it was
        if kind == "sensor":
            m = np.asarray(value, np.float64).reshape(4, 4)
            if not np.isfinite(m).all() or abs(np.linalg.det(m)) < 1e-30:
                raise RuntimeError("sensor to_world: the matrix is singular or not finite")
            new = ScalarTransform4f(np.concatenate([m.astype(np.float32).ravel(), np.linalg.inv(m).T.astype(np.float32).ravel()]))
            if b.kind != 'orthographic' and new.has_scale():
                raise RuntimeError("Scale factors in the camera-to-world transformation are not allowed!")
            old = b.to_world
            b.to_world = new
            try:
                b.update()                                       # the sensor record travels with every render call: no scene handle involved
            except Exception:
                b.to_world = old; b.update()
                raise
            return
        if kind in ("ppo_x", "ppo_y"):       # perspective.cpp:158-159: the principal point, a fraction of the film size; the projection is re-lowered
            v = float(np.asarray(value, np.float32).reshape(-1)[0])
            if not math.isfinite(v):
                raise RuntimeError("perspective: the principal point offset is not finite")
            b.props['principal_point_offset_' + kind[-1]] = v
            b.update()
            return
        if kind in ("aperture_radius", "focus_distance"):      # ThinLensCamera::parameters_changed -> update_camera_transforms (thinlens.cpp:179-188); the record is re-lowered
            v = float(np.asarray(value, np.float32).reshape(-1)[0])
            if kind == "aperture_radius":
                if not (v >= 0.0) or not math.isfinite(v):
                    raise RuntimeError("thinlens: aperture_radius must be non-negative and finite")
                old = b.aperture_radius
                b.aperture_radius = v if v != 0.0 else float(np.float32(2.0 ** -24))
                b.props['aperture_radius'] = b.aperture_radius
            else:
                if not (v > 0.0) or not math.isfinite(v):
                    raise RuntimeError("thinlens: focus_distance must be positive and finite")
                old = b.focus_distance_
                b.focus_distance_ = v
                b.props['focus_distance'] = v
            try:
                b.update()
            except Exception:
                if kind == "aperture_radius":
                    b.aperture_radius = old; b.props['aperture_radius'] = old
                else:
                    b.focus_distance_ = old; b.props['focus_distance'] = old
                b.update()
                raise
            return
        if kind == "x_fov":                  # PerspectiveCamera::parameters_changed -> update_camera_transforms (perspective.cpp:163-198): the projection follows the new angle
            fov = float(np.asarray(value, np.float32).reshape(-1)[0])
            if not (0.0 < fov < 180.0):
                raise RuntimeError("The horizontal field of view must be in the range [0, 180]!")
            old = dict(b.props)
            b.props.pop('focal_length', None); b.props['fov'] = fov; b.props['fov_axis'] = 'x'
            try:
                b.update()
            except Exception:
                b.props = old; b.update()
                raise
            return
        if kind == "sampling_weight":
            w = float(np.asarray(value, np.float32).reshape(-1)[0])
            if not (w >= 0.0) or not math.isfinite(w):
                raise RuntimeError("DiscreteDistribution: entries must be non-negative!")
            e = dict(self.emitters[b]); e["sampling_weight"] = w; self.emitters[b] = e
            self._weights_dirty = True               # the distribution is rebuilt once, after every weight of this update() is in (_validate_spots)
            return
        if kind == "emitter_tex":      # BitmapTexture::parameters_changed -> rebuild_internals (bitmap.cpp:484-493): new texels, new texel distribution
            light = self.emitters[b]["light"]
            v = np.ascontiguousarray(np.asarray(value, np.float32))
            if self.emitters[b].get("type") == 8:      # a projector's irradiance: any finite texels (nothing is sampled from them); a bitmap of another resolution is refused
                h, w = light.texture.shape[:2]
                if v.shape != (h, w, light.channels) or not np.isfinite(v).all():
                    raise RuntimeError("projector: the irradiance bitmap must keep its shape %s and be finite" % ((h, w, light.channels),))
                v = np.ascontiguousarray(np.repeat(v, 3, axis=2)) if light.channels == 1 else v
                light.texture = v; self.textures[light.tex_index] = v
                if self._h is not None:
                    check(lib().har_scene_set_texture(self._h, light.tex_index, _fp(v)))
                return
            if v.shape != light.texture.shape or not np.isfinite(v).all():
                raise RuntimeError("area: the radiance bitmap must keep its shape %s and be finite" % (light.texture.shape,))
            if not (v >= 0).all() or float(v.sum()) <= 0.0:
                raise RuntimeError("area: the radiance bitmap must be non-negative with some luminance to sample")
            light.texture = v; self.textures[light.tex_index] = v
            if self._h is not None:
                check(lib().har_scene_set_texture(self._h, light.tex_index, _fp(v)))
            return
        if kind in ("to_uv", "emitter_to_uv"):
            if kind == "emitter_to_uv":
                b = self.emitters[b]["light"]
            m = np.asarray(value.matrix if isinstance(value, (ScalarTransform3f, ScalarTransform4f)) else value, np.float32)
            if m.shape == (4, 4):
                m = np.array([[m[0, 0], m[0, 1], m[0, 3]], [m[1, 0], m[1, 1], m[1, 3]], [0.0, 0.0, 1.0]], np.float32)
            m = m.reshape(3, 3)
            if not np.isfinite(m).all() or float(np.linalg.det(m[:2, :2].astype(np.float64))) == 0.0:
                raise RuntimeError("bitmap: 'to_uv' is singular")
            rows = [float(x) for x in m[:2, :].reshape(-1)]
            if kind == "emitter_to_uv" and not isinstance(b, Projector):          # (a projector never samples positions from its bitmap)
                _check_sampling_transform(rows)
            b.tex_to_uv = rows; self.texture_to_uv[b.tex_index] = rows
            if self._h is not None:
                check(lib().har_scene_set_texture_to_uv(self._h, b.tex_index, _fp(_f32(rows))))
            return
        if kind == "env_data":             # EnvironmentMapEmitter::parameters_changed (envmap.cpp:208-256): the real columns are what was written, the halo is refreshed from
            v = np.asarray(value, np.float32)  # them, the sampling distribution is rebuilt (here: with the next scene handle, from the texture table)
            if v.ndim != 3:
                raise RuntimeError("Environment map data has dimension %d, expected 3" % v.ndim)
            if v.shape[2] != 3:
                raise RuntimeError("Environment map data has %d channels, expected 3" % v.shape[2])
            if v.shape[1] < 4 or v.shape[0] < 3 or not np.isfinite(v).all():
                raise RuntimeError("Environment map data: at least 3 rows and 2 real columns of finite values")
            self._drop_handle()
            self.textures[self.emitters[b]["mesh"]] = np.ascontiguousarray(v[:, 1:-1, :])
            self._drop_handle()
            return
        e = dict(self.emitters[b])
        if kind == "env_scale":
            sc = float(np.asarray(value, np.float32).reshape(-1)[0])
            if not math.isfinite(sc):
                raise RuntimeError("envmap: 'scale' is not finite")
            e["radiance"] = [sc] + [float(x) for x in e["radiance"][1:]]
        elif kind == "proj_scale":
            sc = float(np.asarray(value, np.float32).reshape(-1)[0])
            if not math.isfinite(sc):
                raise RuntimeError("projector: `scale` is not finite")
            e["normal"] = [sc] + [float(x) for x in e["normal"][1:]]
        elif kind in ("cutoff_angle", "beam_width"):
            nrm = [float(x) for x in e["normal"]]; nrm[0 if kind == "cutoff_angle" else 1] = float(np.asarray(value, np.float32).reshape(-1)[0])
            e["normal"] = nrm                                        # the pair is validated once both values of an update() are in (_validate_spots)
        elif kind == "position":
            pos = np.asarray(value, np.float32).reshape(3)
            if not np.isfinite(pos).all():
                raise RuntimeError("emitter position is not finite")
            e["to_world"] = list(e["to_world"][:9]) + [float(x) for x in pos]
        else:
            m = np.asarray(value, np.float64).reshape(4, 4)
            if not np.isfinite(m).all() or abs(np.linalg.det(m)) < 1e-30:
                raise RuntimeError("emitter to_world: the matrix is singular or not finite")
            inv = np.linalg.inv(m)
            e["to_world"] = [float(x) for x in m[:3, :].T.reshape(-1)]; e["to_local"] = [float(x) for x in inv[:3, :].T.reshape(-1)]
        self.emitters[b] = e
        if self._h is not None and e.get("type", 0) in (4, 5, 6, 8) and kind not in ("cutoff_angle", "beam_width"):
            # the record of a delta emitter is re-lowered IN PLACE (har_scene_set_delta_emitter): the scene handle and the acceleration data survive a moved light.
            # (cone values arrive one by one and are validated as a pair at the end of update(): _validate_spots pushes the record then)
            self._push_delta_emitter(b)
        elif self._h is not None and e.get("type", 0) in (4, 5, 6):
            self.__dict__.setdefault("_emitters_to_push", set()).add(b)
        else:
            self._drop_handle()                                  # other emitter records are part of the scene's tables: rebuilt with the next handle

    def _push_delta_emitter(self, b):
        rec = _capi.HarEmitter()
        self._fill_emitter_record(rec, self.emitters[b])
        rc = lib().har_scene_set_delta_emitter(self._h, int(b), C.byref(rec))
        if rc != 0:
            msg = (lib().har_last_error() or b"").decode()
            self._drop_handle()
            raise RuntimeError(msg or "emitter update failed")

    def _envmap_gradients(self, D, envmap_keys):
        """the gradients of an environment map's `data` and `scale` from what the library deposits with har_integrator_set_grad_envmap: D, the adjoint of the map's bilinear
        lookup over the REAL texels (H x W x 3), without `scale`.  d / d data = scale * D in the parameter's layout H x (W + 2) x 3 with ZERO halo columns (the halo is a copy
        the emitter refreshes from the real edge columns, envmap.cpp:229-246: what reaches it is folded onto its source column, as the reference's AD-tracked scatter does);
        d / d scale = <D, data> -- exact at scale = 0.  envmap_keys: {"env_data": (key, emitter), "env_scale": (key, emitter)}"""
        torch = _torch()
        key_d, i = envmap_keys["env_data"]; key_s, _ = envmap_keys["env_scale"]
        data = torch.as_tensor(np.asarray(self.textures[self.emitters[i]["mesh"]], np.float32), device=D.device)
        g_data = torch.zeros((D.shape[0], D.shape[1] + 2, 3), dtype=torch.float32, device=D.device)
        g_data[:, 1:-1, :] = D * float(self.emitters[i]["radiance"][0])
        return {key_d: g_data, key_s: (D.double() * data.double()).sum().to(torch.float32).reshape(1)}

    def _projector_gradients(self, g_tex, g_emit, out):
        """the gradients of the projectors' `irradiance` and `scale` from what the library deposits.  A bitmap (with `light_texel_gradients`): D, the adjoint of the
        lookup WITHOUT `scale` in the bitmap's entry of grad_textures -- d / d data = scale * D (summed over the channels of a one-channel bitmap, which is stored three
        times), d / d scale = <D, data>.  A constant (with `emitter_gradients`): the row of grad_emitters is d / d (irradiance * scale) -- d / d irradiance = scale * row,
        d / d scale = <row, irradiance>.  Both are exact where `scale`, texels or the colour are zero."""
        torch = _torch(); res = {}
        keys = {(kind, i): k for k, (kind, i) in self._pose_keys().items() if kind in ("proj_scale", "emitter_tex")}
        for i, e in enumerate(self.emitters):
            if e.get("type") != 8:
                continue
            scale = float(np.float32(e["normal"][0])); light = e.get("light")
            if light is not None and g_tex is not None:
                D = g_tex[light.tex_index]
                data = torch.as_tensor(np.asarray(light.texture, np.float32), device=D.device)
                g = D * scale
                res[keys[("emitter_tex", i)]] = g.sum(dim=2, keepdim=True) if light.channels == 1 else g
                res[keys[("proj_scale", i)]] = (D.double() * data.double()).sum().to(torch.float32).reshape(1)
            elif light is None and g_emit is not None:
                row = g_emit[i]
                c = torch.as_tensor(np.asarray(e["radiance"], np.float32), device=row.device)
                for k, (kind, b) in self._param_keys().items():
                    if kind == "emit" and b == i:
                        res[k] = row * scale
                res[keys[("proj_scale", i)]] = (row.double() * c.double()).sum().to(torch.float32).reshape(1)
        return res

    def _gradients(self, g_refl, g_tex, g_emit=None, alpha_maps=False):
        out = {}
        for k, (kind, b) in self._param_keys().items():
            if kind == "emit":
                if g_emit is not None:
                    out[k] = g_emit[b]
            elif b.kind == 'alphamap':
                # a roughness map: filled by the alpha terms of the adjoint (`bsdf_parameter_gradients`) alone, through the transpose of eval_1 -- the luminance coefficients
                # are in it; a one-channel map received channel 0.  Without those terms the key has no gradient (not a zero one)
                if alpha_maps:
                    out[k] = g_tex[b.tex_index] if b.weight_channels == 3 else g_tex[b.tex_index][:, :, :1].contiguous()
            elif b.kind in _WEIGHTED_BSDFS:
                # the weight of a blend (the opacity of a mask): the buffers hold d L / d w per colour channel of the radiance; the parameter is a scalar (sum of the row, as `alpha` is summed), a
                # one-channel bitmap (channel sum) or a three-channel one whose luminance is the weight (d w / d texel_k = lum_k)
                if kind == "tex":
                    s = g_tex[b.tex_index].sum(dim=2, keepdim=True)
                    out[k] = s if b.weight_channels == 1 else s * s.new_tensor(_LUMINANCE).reshape(1, 1, 3)
                else:
                    out[k] = g_refl[b.index].sum().reshape(1)
            elif b.kind == 'bumpmap':
                # the height map: the commit deposited through the transpose of eval_1_grad -- the luminance coefficients are in it; a one-channel map received channel 0
                out[k] = g_tex[b.tex_index] if b.weight_channels == 3 else g_tex[b.tex_index][:, :, :1].contiguous()
            else:
                out[k] = g_tex[b.tex_index] if kind == "tex" else g_refl[b.index]
        # mesh attributes: the records of the BSDFs that read '<shape>.<name>' hold d L / d (row, channel) of their rows x 1 x 3 copy; back to the parameter's (rows, dim)
        # -- a one-channel attribute was stored three times (sum), a weight / opacity record holds d L / d w per colour channel (sum), what evaluates to 0 has none
        for k, (mesh, name) in self._attr_keys().items():
            rows, dim = self.meshes[mesh]["attributes"][name].shape
            total = None
            for b in self._attr_readers(mesh, name):
                g = g_tex[b.tex_index].reshape(rows, 3)
                if dim == 1:
                    g = g.sum(dim=1, keepdim=True)
                elif not (dim == 3 and b.kind not in _WEIGHTED_BSDFS):
                    continue
                total = g if total is None else total + g
            out[k] = total if total is not None else g_refl.new_zeros((rows, dim))
        return out

    @staticmethod
    def _colour_view(kind, b, value):
        """the value mi.traverse() shows for slot 0 of a BSDF: the stored one, except a blend's weight -- a scalar, or the H x W x 1 / x 3 bitmap it was given"""
        if b.kind not in _MONO_TEX_BSDFS:
            return value
        v = np.asarray(value, np.float32)
        if kind == "tex":
            return np.ascontiguousarray(v[:, :, :1]) if b.weight_channels == 1 else v
        return v.reshape(-1)[:1].copy()

    @staticmethod
    def _colour_store(kind, b, t, key):
        """the inverse for a blend's weight, on a torch tensor or a numpy array: a scalar is stored as (w, w, w), a one-channel bitmap three times"""
        if b.kind not in _MONO_TEX_BSDFS:
            return t
        if kind == "tex":
            h, w = b.texture.shape[:2]; c = b.weight_channels
            if int(np.prod(tuple(t.shape))) != h * w * c:
                raise RuntimeError("%s: expected a tensor of shape %s" % (key, (h, w, c)))
            t = t.reshape(h, w, c)
            return t if c == 3 else (t.expand(h, w, 3).contiguous() if hasattr(t, 'expand') else np.ascontiguousarray(np.repeat(t, 3, axis=2)))
        if int(np.prod(tuple(t.shape))) != 1:
            raise RuntimeError("%s: expected 1 value" % key)
        t = t.reshape(1)
        return t.expand(3).contiguous() if hasattr(t, 'expand') else np.repeat(t, 3)


class ParamFlags:
    """include/mitsuba/core/object.h:363-372"""
    Differentiable = 0
    NonDifferentiable = 1
    Discontinuous = 2
    ReadOnly = 4


class SceneParameters(dict):
    """mi.traverse(scene): differentiable parameters as torch tensors (util.py SceneParameters)."""

    def flags(self, key):
        """SceneParameters.flags (util.py:146-148): what THIS variant can do with the entry -- Differentiable where `prb` produces its gradient (| Discontinuous where the
        reference's traverse() says so: geometry, roughness, complex IOR, texels of a light), NonDifferentiable for placements and plain values, ReadOnly for what is only shown"""
        if key not in self:
            raise KeyError(key)
        sc = self.scene
        if key in self._read_only:
            return ParamFlags.ReadOnly | ParamFlags.NonDifferentiable
        if key in sc._param_keys() or key in sc._attr_keys():
            return ParamFlags.Differentiable
        if key in sc._bsdf_param_keys():
            return ParamFlags.NonDifferentiable if sc._bsdf_param_keys()[key][0] in _NOGRAD_PARAMS else (ParamFlags.Differentiable if sc._bsdf_param_keys()[key][0] in ("slot1", "thin_r") else ParamFlags.Differentiable | ParamFlags.Discontinuous)
        if key in sc._position_keys() or key in sc._instance_keys() or key in sc._rect_keys():
            return ParamFlags.Differentiable | ParamFlags.Discontinuous
        if sc._pose_keys().get(key, (None,))[0] == "emitter_tex":
            if sc.emitters[sc._pose_keys()[key][1]].get("type") == 8:          # projector.cpp:139: Differentiable
                return ParamFlags.Differentiable
            return ParamFlags.Differentiable | ParamFlags.Discontinuous
        if sc._pose_keys().get(key, (None,))[0] in ("env_data", "env_scale", "proj_scale"):          # envmap.cpp:203-208; `prb` with `envmap_gradients`; projector.cpp:138
            return ParamFlags.Differentiable
        return ParamFlags.NonDifferentiable

    def set_dirty(self, key):
        """SceneParameters.set_dirty (util.py:150-185): the next update() treats the entry as written (for writes the version counter does not see)"""
        if key not in self:
            raise KeyError(key)
        self._written.add(key)

    def keep(self, keys):
        """SceneParameters.keep (util.py:238-256): only the entries whose names match one of `keys` (regular expressions, `re.match`) stay in the table"""
        import re
        if not isinstance(keys, list):
            keys = [keys]
        regexps = [re.compile(k).match for k in keys]
        for k in [k for k in list(self.keys()) if not any(r(k) for r in regexps)]:
            dict.__delitem__(self, k)
            self._read_only.discard(k); self._written.discard(k)
        self._host_table = None            # the update tables are rebuilt over the entries that are left

    def __init__(self, scene):
        super().__init__()
        torch = _torch()
        self.scene = scene
        scene.sync_host()
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        for k, (kind, b) in scene._param_keys().items():
            value = scene.emitters[b]["radiance"] if kind == "emit" else scene._colour_view(kind, b, b.texture if kind == "tex" else b.value)
            self[k] = torch.tensor(np.asarray(value, np.float32), dtype=torch.float32, device=dev)
        for k, (what, b) in scene._bsdf_param_keys().items():
            self[k] = torch.tensor(np.asarray(scene._bsdf_param_value(what, b), np.float32), dtype=torch.float32, device=dev)
        for k, (m, name) in scene._attr_keys().items():
            self[k] = torch.tensor(scene.meshes[m]["attributes"][name], dtype=torch.float32, device=dev)            # rows x dim (Mesh::traverse, mesh.cpp:844-845)
        for k, b in scene._attr_scale_keys().items():
            self[k] = torch.tensor([b.attr[1]], dtype=torch.float32, device=dev)
        for k, m in scene._position_keys().items():
            self[k] = torch.tensor(np.ascontiguousarray(scene.meshes[m]["V"][:, :3]), dtype=torch.float32, device=dev)            # N x 3, as the reference's `positions` tensor
        for k, i in scene._instance_keys().items():
            self[k] = torch.tensor(scene._instance_matrix(i), dtype=torch.float32, device=dev)
        for k, i in scene._rect_keys().items():
            self[k] = torch.tensor(scene._rect_matrix(i), dtype=torch.float32, device=dev)
        for k, (kind, b) in scene._pose_keys().items():
            self[k] = torch.tensor(scene._pose_value(kind, b), dtype=torch.float32, device=dev)
        # what Mesh::traverse (src/render/mesh.cpp:822-843) also registers and this variant can only SHOW: the index buffer and the texture coordinates (N x 2) of the
        # triangle meshes -- readable under the reference's names, refused on write like a ParamFlags::ReadOnly entry (util.py:59-60)
        self._read_only = set()
        for k, m in scene._position_keys().items():
            mesh = scene.meshes[m]; base = k[:-len(".positions")]
            self[base + ".faces"] = torch.tensor(np.ascontiguousarray(mesh["F"][:, :3]).astype(np.int64), dtype=torch.int64, device=dev)
            self._read_only.add(base + ".faces")
            if mesh["flags"] & 2:
                self[base + ".texcoords"] = torch.tensor(np.ascontiguousarray(mesh["V"][:, 6:8]), dtype=torch.float32, device=dev)
                self._read_only.add(base + ".texcoords")
        # ... and of the sensors: what ProjectiveCamera / Sensor / Film register next to `to_world` (sensor.h:135-141,206-210, film.cpp:55-57), all NonDifferentiable there;
        # shown, not updatable here (a new film size is a new scene description)
        for k, sn in zip(scene.sensor_keys, scene.m_sensors):
            f = sn.film()
            for name, val in (("near_clip", [sn.near_clip]), ("far_clip", [sn.far_clip]), ("shutter_open", [0.0]), ("shutter_open_time", [0.0]),
                              ("film.size", [f.width, f.height]), ("film.crop_size", list(f.crop_size_)), ("film.crop_offset", list(f.crop_offset_))):
                key = k + "." + name
                self[key] = torch.tensor(val, dtype=torch.float32 if "clip" in name or "shutter" in name else torch.int64, device=dev)
                self._read_only.add(key)
        self._failures_seen = getattr(scene, "_update_failures", 0)
        self._written = set()           # keys assigned since the last update() (SceneParameters.__setitem__ flags them in the reference, util.py)
        # the tensors above ARE the scene's values: recorded as applied, so that the first update() touches only what was written or stepped since (vertex positions on
        # the GPU are never compared -- a mesh is updated when its tensor's version counter moved, see _changed_keys)
        snap = self.__dict__.setdefault("_snapshot", {}); seen = self.__dict__.setdefault("_seen", {})
        for k, what, _ in self._host_kinds():
            t = self[k]
            seen[k] = (t, t._version)
            snap[k] = None if (what in ("pos", "inst") and t.is_cuda) else t.detach().clone()

    def __setitem__(self, key, value):
        if hasattr(self, "_written"):                 # (the constructor fills the table before `_written` exists)
            if key not in self:
                raise KeyError(key)                   # util.py:57: `self.properties[key]` -- a name traverse() did not register is not a parameter
            if key in self._read_only:
                raise Exception("%s is a read-only parameter!" % key)      # util.py:59-60
        super().__setitem__(key, value)
        if hasattr(self, "_written"):
            self._written.add(key)

    def _host_kinds(self):
        """(key, setter) of the parameters whose update runs on the host (geometry: accel update; poses; the non-colour BSDF parameters, whose records are
        re-lowered): the key tables are those of the scene at traverse() time -- the set of parameters of a scene does not change"""
        if getattr(self, "_host_table", None) is None:
            sc = self.scene; t = []
            for k, m in sc._position_keys().items():
                t.append((k, "pos", m))
            for k, i in sc._instance_keys().items():
                t.append((k, "inst", i))
            for k, i in sc._rect_keys().items():
                t.append((k, "rect", i))
            for k, (kind, b) in sc._pose_keys().items():
                t.append((k, "pose", (kind, b)))
            for k, (what, b) in sc._bsdf_param_keys().items():
                t.append((k, "bsdf", (what, b)))
            self._host_table = [e for e in t if e[0] in self]                      # (keep() may have dropped entries)
            self._colour_table = [e for e in sc._param_keys().items() if e[0] in self]
            self._attr_table = [(k, ("attr", ref)) for k, ref in sc._attr_keys().items() if k in self] + [(k, ("scale", b)) for k, b in sc._attr_scale_keys().items() if k in self]
        return self._host_table

    def _changed_keys(self, written):
        """which host-updated keys hold other values than at the last update(): WRITTEN keys (SceneParameters.__setitem__ flags them, util.py) and tensors modified
        in place (an optimiser step).  A tensor that is the same object with the same version counter as at the last update() is unchanged without looking at it;
        the others are compared with the snapshot of the last update() ON THE TENSOR'S DEVICE, one flag per key, ONE read-back for all of them (round 4 copied
        every parameter to the host, every step).  Vertex positions that live on the GPU are not even compared: a new version counter IS the change (the device
        update costs less than the comparison's synchronisation).  Values without a version counter (numpy arrays, lists) are compared every call.
        (Writes that bypass the version counter -- `tensor.data.add_()`, raw pointers -- need `params[key] = params[key]`, as every update does in the reference.)
        Returns (changed keys, marks): `marks[k]()` records key k as applied -- update() calls it AFTER the key's setter succeeded, so that a rejected value
        (singular matrix, wrong size, a C error) is looked at again by the next update() instead of being remembered as pushed."""
        torch = _torch()
        table = self._host_kinds()
        snap = self.__dict__.setdefault("_snapshot", {})
        seen = self.__dict__.setdefault("_seen", {})          # key -> (the tensor object, its version counter) at the last update()
        fails = getattr(self.scene, "_update_failures", 0)
        if self.__dict__.get("_failures_seen", 0) != fails:
            # an update failed since the last call and took the scene handle with it: what the device held is in the mirrors as far as it was valid, so every geometry
            # key is compared with its mirror again -- a value the device rejected late (not finite, singular) is not remembered as applied
            for k, what, _ in table:
                if what in ("pos", "inst"):
                    seen.pop(k, None); snap.pop(k, None)
            self._failures_seen = fails
        changed = set(k for k, _, _ in table if k in written or k not in snap)
        flags = []; names = []
        device_pos = set()
        for k, what, _ in table:
            t = self[k]
            if what in ("pos", "inst") and getattr(t, "is_cuda", False) and self.scene._h is not None and not os.environ.get("HAR_HOST_VERTEX_UPDATE"):
                device_pos.add(k)
                mark = seen.get(k)
                if mark is None or mark[0] is not t or mark[1] != t._version:
                    changed.add(k)
                continue
            if k in changed:
                continue
            if not hasattr(t, "detach") or not hasattr(t, "_version"):
                changed.add(k); continue
            mark = seen.get(k)
            if mark is not None and mark[0] is t and mark[1] == t._version:
                continue                    # the same tensor object, never written in place since (torch bumps _version on every in-place op): nothing to compare
            t = t.detach(); old = snap[k]
            if old is None or old.shape != t.shape or old.device != t.device or old.dtype != t.dtype:
                changed.add(k); continue
            flags.append((t != old).any()); names.append(k)
        if flags:
            by_dev = {}
            for f, k in zip(flags, names):
                by_dev.setdefault(f.device, []).append((f, k))
            for dev, items in by_dev.items():
                got = torch.stack([f for f, _ in items]).tolist()          # one synchronisation per device
                changed.update(k for (_, k), g in zip(items, got) if g)

        def marker(k):
            t = self[k]

            def apply():
                mark = seen.get(k)
                if mark is not None and mark[0] is t and hasattr(t, "_version") and mark[1] == t._version and k in snap:
                    return                       # the same tensor at the same version as at the last update(): the snapshot and the mark are current (no clone per key and step)
                if k in device_pos:
                    snap[k] = None               # never compared (see above): no clone of a million vertices per step, no read-back of a flag
                else:
                    snap[k] = t.detach().clone() if hasattr(t, "detach") else torch.as_tensor(np.array(t, np.float32, copy=True))
                if hasattr(t, "_version"):
                    seen[k] = (t, t._version)
            return apply
        marks = {k: marker(k) for k, _, _ in table}
        return changed, marks

    def update(self, values=None):
        """SceneParameters.update (src/python/python/util.py): push the values to the scene.  Colours, bitmaps, emitter radiances AND VERTEX POSITIONS that live on the
        GPU go to the scene's device arrays directly (har_scene_set_*_device, har_scene_update_vertices_device: device-to-device on the current stream, no host round
        trip, no synchronisation); instance transforms, poses and the non-colour BSDF parameters are compared on their device and only the ones that changed travel to
        the host (accel update / re-lowering)."""
        if values:
            for k, v in values.items():
                if k in self:                  # util.py:210-213: names that are not parameters are skipped
                    self[k] = v
        torch = _torch()
        written, self._written = self._written, set()
        sc = self.scene
        changed, marks = self._changed_keys(written)
        moved = []; moved_keys = []; moved_dev = []
        for k, what, ref in self._host_kinds():
            if k not in changed:
                if what not in ("pos", "inst") or not getattr(self[k], "is_cuda", False):
                    marks[k]()              # unchanged: remember the (possibly new) tensor object and version
                continue
            v = self[k]
            if what == "inst" and getattr(v, "is_cuda", False) and sc._h is not None and not os.environ.get("HAR_HOST_VERTEX_UPDATE"):
                moved_dev.append((ref, k, v))
                continue
            if what == "pos" and getattr(v, "is_cuda", False) and sc._h is not None and not os.environ.get("HAR_HOST_VERTEX_UPDATE"):
                sc._set_vertex_positions_device(ref, v)
                marks[k]()
                continue
            v = v.detach().to("cpu").numpy().astype(np.float32) if hasattr(v, "detach") else np.asarray(v, np.float32)
            if what == "pos":
                v = v.reshape(-1, 3)
                sc._sync_host_geometry()
                # a WRITTEN key notifies the mesh even when the values are the old ones: the vertex normals are regenerated (mesh.cpp:876-878)
                if k in written or not np.array_equal(v, sc.meshes[ref]["V"][:, :3]):
                    sc._set_vertex_positions(ref, v)
            elif what == "inst":
                if not np.array_equal(v.reshape(4, 4), sc._instance_matrix(ref)):
                    moved.append((ref, v.reshape(4, 4))); moved_keys.append(k)
                    continue                # marked once the whole run of instances went through
            elif what == "rect":
                if not np.array_equal(v.reshape(4, 4), sc._rect_matrix(ref)):
                    sc._set_rect_to_world(ref, v.reshape(4, 4))
            elif what == "pose":
                if not np.array_equal(v.reshape(-1), sc._pose_value(*ref).reshape(-1)):
                    sc._set_pose(ref[0], ref[1], v)
            else:
                if not np.array_equal(v.reshape(-1), np.asarray(sc._bsdf_param_value(*ref), np.float32).reshape(-1)):
                    sc._set_bsdf_param(ref[0], ref[1], v.reshape(-1))
            marks[k]()
        if moved:
            sc._set_instance_matrices(moved)
            for k in moved_keys:
                marks[k]()
        if moved_dev and sc._h is None:          # a later key of this update() (a rectangle's to_world) asked for a new scene: the matrices go to the host mirrors it is built from
            sc._set_instance_matrices([(ref, v.detach().to("cpu").numpy().astype(np.float32).reshape(4, 4)) for ref, _, v in moved_dev])
            for _, k, _ in moved_dev:
                marks[k]()
            moved_dev = []
        if moved_dev:          # instance transforms that live on the GPU: one call per run of consecutive instances, nothing leaves the device
            moved_dev.sort(key=lambda e: e[0]); start = 0
            while start < len(moved_dev):
                end = start
                while end + 1 < len(moved_dev) and moved_dev[end + 1][0] == moved_dev[end][0] + 1:
                    end += 1
                rows = torch.stack([e[2].detach().to(torch.float32).reshape(4, 4)[:3, :].T.reshape(-1) for e in moved_dev[start:end + 1]])
                sc._set_instance_matrices_device(moved_dev[start][0], rows)
                for e in moved_dev[start:end + 1]:
                    marks[e[1]]()
                start = end + 1
        sc._validate_spots()
        stream = None
        pushed = self.__dict__.setdefault("_pushed", {})      # key -> (tensor object, version counter, scene handle) of the last push
        for k, (kind, ref) in self._attr_table:               # mesh attributes ('<shape>.<name>') and the `scale` of the textures that read them
            t = self[k]
            mark = pushed.get(k)
            if k not in written and mark is not None and hasattr(t, "_version") and mark[0] is t and mark[1] == t._version and mark[2] == (sc._h.value if sc._h is not None else None):
                continue
            new_mark = (t, getattr(t, "_version", None), sc._h.value if sc._h is not None else None)
            if kind == "attr":
                sc._set_attribute(ref[0], ref[1], t if hasattr(t, "shape") else np.asarray(t, np.float32), k)
            else:
                sc._set_attr_scale(ref, t, k)
            pushed[k] = new_mark
        for k, (kind, b) in self._colour_table:
            t = self[k]
            mark = pushed.get(k)
            if k not in written and mark is not None and hasattr(t, "_version") and mark[0] is t and mark[1] == t._version and mark[2] == (sc._h.value if sc._h is not None else None):
                continue                    # the value the scene already holds (values without a version counter -- numpy arrays -- are pushed every call)
            new_mark = (t, getattr(t, "_version", None), sc._h.value if sc._h is not None else None)      # recorded once the push below went through
            on_gpu = hasattr(t, "is_cuda") and t.is_cuda and sc._h is not None
            if kind == "emit" and sc.emitters[b].get("type") == 8:
                on_gpu = False          # a projector's record holds irradiance * scale: re-lowered on the host (har_scene_set_delta_emitter)
            if on_gpu:
                # the scene's copy is the value AT update(): snapshot on the device (a later in-place edit of the tensor is not an update), host mirror refreshed lazily
                v = t.detach().to(torch.float32).contiguous()
                if kind != "emit":
                    v = sc._colour_store(kind, b, v, k)
                stream = stream or _stream()
                if kind == "emit":
                    if v.numel() != 3:
                        raise RuntimeError("%s: expected 3 values" % k)
                    check(lib().har_scene_set_emitter_radiance_device(sc._h, b, _ptr(v), stream))
                elif kind == "tex":
                    if v.numel() != b.texture.size:
                        raise RuntimeError("%s: expected a tensor of shape %s" % (k, b.texture.shape))
                    check(lib().har_scene_set_texture_device(sc._h, b.tex_index, _ptr(v), stream))
                else:
                    if v.numel() != 3:
                        raise RuntimeError("%s: expected 3 values" % k)
                    check(lib().har_scene_set_reflectance_device(sc._h, b.index, _ptr(v), stream))
                sc._device_values[(kind, b if kind == "emit" else (b.tex_index if kind == "tex" else b.index))] = (v if v.data_ptr() != t.data_ptr() else v.clone(), b)
                pushed[k] = new_mark
                continue
            v = t.detach().to("cpu").numpy().astype(np.float32) if hasattr(t, "detach") else np.asarray(t, np.float32)
            if kind != "emit":
                v = sc._colour_store(kind, b, v, k)
            if kind == "emit":
                sc._device_values.pop(("emit", b), None)
                sc.emitters[b]["radiance"] = np.ascontiguousarray(v.reshape(3))
                if sc._h is not None and sc.emitters[b].get("type") == 8:
                    sc._push_delta_emitter(b)
                elif sc._h is not None:
                    check(lib().har_scene_set_emitter_radiance(sc._h, b, _fp(sc.emitters[b]["radiance"])))
            elif kind == "tex":
                sc._device_values.pop(("tex", b.tex_index), None)
                b.texture = np.ascontiguousarray(v.reshape(b.texture.shape)); sc.textures[b.tex_index] = b.texture
                if sc._h is not None:
                    check(lib().har_scene_set_texture(sc._h, b.tex_index, _fp(b.texture)))
            else:
                sc._device_values.pop(("rgb", b.index), None)
                b.value = np.ascontiguousarray(v.reshape(3))
                if sc._h is not None:
                    check(lib().har_scene_set_reflectance(sc._h, b.index, _fp(b.value)))
            pushed[k] = new_mark


class ObjectParameters:
    """mi.traverse(<a plugin object>): the reference walks any Object (util.py:263-341); its tests traverse emitters, shapes and BSDFs on their own and read the entries without
    a prefix (`params['cutoff_angle']`, test_spot.py:189-212).  The object is placed in a private scene under the name `obj`; this view strips and adds that prefix."""

    def __init__(self, obj):
        if isinstance(obj, BSDF):
            if obj.scene is None:
                Scene({'obj': obj})
            self.scene = obj.scene
            self._prefix = (obj.id if obj.id else "bsdf%d" % obj.index) + "."
        else:
            # one private scene per object, kept with it: a second traverse() of the same object sees what the first one's update() did (the reference updates the object itself)
            sc = getattr(obj, '_traverse_scene', None)
            if sc is None:
                sc = Scene({'obj': obj})
                try:
                    obj._traverse_scene = sc
                except AttributeError:
                    pass
            self.scene = sc
            self._prefix = "obj."
        self._inner = SceneParameters(self.scene)
        self._inner.keep(["^" + re.escape(self._prefix)])

    def keys(self):
        return [k[len(self._prefix):] for k in self._inner.keys()]

    def items(self):
        return [(k[len(self._prefix):], v) for k, v in self._inner.items()]

    def __iter__(self):
        return iter(self.items())

    def __len__(self):
        return len(self._inner)

    def __contains__(self, key):
        return self._prefix + key in self._inner

    def __getitem__(self, key):
        return self._inner[self._prefix + key]

    def __setitem__(self, key, value):
        self._inner[self._prefix + key] = value

    def flags(self, key):
        return self._inner.flags(self._prefix + key)

    def set_dirty(self, key):
        self._inner.set_dirty(self._prefix + key)

    def keep(self, keys):
        keys = keys if isinstance(keys, list) else [keys]
        regexps = [re.compile(k).match for k in keys]
        self._inner.keep(["^" + re.escape(self._prefix + k) + "$" for k in self.keys() if any(r(k) for r in regexps)])

    def update(self, values=None):
        return self._inner.update({self._prefix + k: v for k, v in values.items()} if values else None)


def traverse(node):
    """mi.traverse (util.py:263-341): the parameter table of a scene, or of a single plugin object (names without a prefix)"""
    return SceneParameters(node) if isinstance(node, Scene) else ObjectParameters(node)


class DeviceGroup:
    """N GPUs driven by ONE host thread through the C ABI (har_multi_*: a replica of the scene, an integrator and a stream per device; row bands with global lane
    indices; one RCCL reduce of the film on devices[0]).  The single-call counterpart of render_distributed (one process per GPU, torch.distributed), for hosts that
    call Integrator::render once from one thread (include/mitsuba/render/integrator.h:74-79).  `path` renders; parameters are those of the scene at construction
    (replica(k) hands out the per-device handles for updates)."""

    def __init__(self, scene, devices=(0,), integrator=None):
        integrator = integrator or scene.integrator()
        if integrator is None:
            raise Exception('No integrator specified!')
        if integrator.type == 'aov':
            raise RuntimeError("DeviceGroup: the `aov` integrator is not implemented by hip_ad_rgb for device groups")
        _device()
        self.scene, self.integrator, self.devices = scene, integrator, [int(d) for d in devices]
        d = scene.desc(); h = C.c_void_p()
        devs = (C.c_int * len(self.devices))(*self.devices)
        check(lib().har_multi_create(C.byref(d), 0 if integrator.type == 'path' else 1, integrator.max_depth, integrator.rr_depth, integrator.chunk_lanes or 0,
                                     devs, len(self.devices), C.byref(h)))
        self._h = h
        for k in range(len(self.devices)):          # every replica renders with the integrator's own settings (Integrator._handle)
            _, it, dev = self.replica(k)
            with _torch().cuda.device(dev):
                integrator._apply_settings(it)

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None:
                lib().har_multi_destroy(self._h); self._h = None
        except Exception:
            pass

    def render(self, sensor=0, seed=0, spp=0, develop=True):
        torch = _torch()
        s = self.scene.sensors()[sensor] if isinstance(sensor, int) else sensor
        _refuse_batch(s, "DeviceGroup (har_multi_render)")
        if getattr(s.film(), "alpha", False):
            raise RuntimeError("DeviceGroup.render(): the group's film has no alpha channel; an `rgba` film renders with render_distributed or mi.render")
        if spp:
            s.sampler().set_sample_count(spp)
        spp = s.sampler().sample_count()
        w, h = s.film().crop_size()
        dev = torch.device("cuda", self.devices[0])
        with torch.cuda.device(dev):
            colour = getattr(s.film(), "colour", 0)
            out = torch.empty((h, w, 1 if colour == 1 else 3) if develop else (h, w, 4), dtype=torch.float32, device=dev)
            check(lib().har_multi_render(self._h, C.byref(s.har), (s.sampler().m_base_seed + int(seed)) & 0xffffffff, spp, colour,
                                         _ptr(out) if develop else None, None if develop else _ptr(out), _stream()))
        return out

    def render_backward(self, grad_in, sensor=0, seed=0, spp=0):
        """RBIntegrator.render_backward over the group (har_multi_render_backward): {key: gradient tensor on devices[0]} for the colour, bitmap and -- with the
        integrator's `emitter_gradients` -- emitter-radiance parameters"""
        if self.integrator.type != 'prb':
            raise RuntimeError("render_backward(): only the `prb` integrator implements the adjoint pass in hip_ad_rgb")
        if getattr(self.integrator, 'envmap_gradients', False):
            raise RuntimeError("envmap gradients are not produced by DeviceGroup.render_backward() (har_multi_render_backward has no switch for them); use one device")
        if getattr(self.integrator, 'bsdf_parameter_gradients', False) and any(getattr(b, 'alpha_maps', None) for b in self.scene.bsdfs):
            raise RuntimeError("roughness map: the alpha texel gradients %s are not produced by DeviceGroup.render_backward() (har_multi_render_backward routes no BSDF-parameter gradients); use one device"
                               % sorted(k for k, (kind, b) in self.scene._param_keys().items() if getattr(b, 'kind', None) == 'alphamap'))
        torch = _torch()
        s = self.scene.sensors()[sensor] if isinstance(sensor, int) else sensor
        _refuse_batch(s, "DeviceGroup (har_multi_render_backward)")
        if spp:
            s.sampler().set_sample_count(spp)
        spp = s.sampler().sample_count()
        w, h = s.film().crop_size()
        if getattr(s.film(), "colour", 0) or getattr(s.film(), "alpha", False):
            raise RuntimeError("DeviceGroup.render_backward(): rgb films only")
        sc = self.scene
        dev = torch.device("cuda", self.devices[0])
        with torch.cuda.device(dev):
            g_in = torch.as_tensor(grad_in, dtype=torch.float32, device=dev).reshape(h, w, 3).contiguous()
            g_refl = torch.zeros((len(sc.bsdfs), 3), dtype=torch.float32, device=dev)
            g_tex = [torch.zeros(tuple(t.shape), dtype=torch.float32, device=dev) for t in sc.textures]
            ptrs = (C.c_void_p * max(1, len(g_tex)))(*[t.data_ptr() for t in g_tex])
            g_emit = torch.zeros((max(1, len(sc.emitters)), 3), dtype=torch.float32, device=dev) if self.integrator.emitter_gradients else None
            check(lib().har_multi_render_backward(self._h, C.byref(s.har), _ptr(g_in), (s.sampler().m_base_seed + int(seed)) & 0xffffffff, spp, _ptr(g_refl), ptrs,
                                                  _ptr(g_emit) if g_emit is not None else None, _stream()))
        for k in range(len(self.devices)):          # the replicas keep no pointer into the group's gradient buffers: their next primal pass is a plain render
            check(lib().har_integrator_set_grad_emitters(self.replica(k)[1], None))
        return sc._gradients(g_refl, g_tex, g_emit)

    def replica(self, k):
        sc = C.c_void_p(); it = C.c_void_p(); dev = C.c_int()
        check(lib().har_multi_replica(self._h, int(k), C.byref(sc), C.byref(it), C.byref(dev)))
        return sc, it, dev.value

    def stats(self):
        """device counters summed over the replicas (paths, vertices, rays)"""
        tot = {}
        for k in range(len(self.devices)):
            _, it, _ = self.replica(k)
            st = _capi.HarStats()
            check(lib().har_render_stats(it, C.byref(st)))
            for f, _t in st._fields_:
                tot[f] = tot.get(f, 0) + int(getattr(st, f))
        return tot

    def info(self):
        n = len(self.devices)
        rows = (C.c_uint32 * (n + 1))(); ms = (C.c_float * n)(); note = C.create_string_buffer(160); nd = C.c_uint32()
        check(lib().har_multi_info(self._h, C.byref(nd), rows, ms, note, 160))
        return dict(devices=list(self.devices), band_rows=list(rows), band_ms=list(ms), reduce=note.value.decode())


# ---------------------------------------------------------------------------
#  PluginManager (src/core/plugin.cpp:157-282): registry keyed by (name, variant)
# ---------------------------------------------------------------------------

_REGISTRY = {}
_BSDF_PLUGINS = ('diffuse', 'dielectric', 'thindielectric', 'conductor', 'plastic', 'roughconductor', 'roughplastic', 'twosided', 'blendbsdf', 'mask', 'normalmap', 'bumpmap')


def register_plugin(name, variant_name, instantiate):
    """PluginManager::register_plugin (plugin.cpp:209-214)."""
    _REGISTRY[(name, variant_name)] = instantiate


def _resolve(value, named, parent_key=None):
    if isinstance(value, dict) and 'type' in value:
        if value['type'] == 'ref':
            if value['id'] not in named:
                raise RuntimeError("Referenced id \"%s\" not found" % value['id'])
            return named[value['id']]
        return _create(value, named, parent_key)
    return value


def _create(props, named, key=None):
    t = props['type']
    ctor = _REGISTRY.get((t, VARIANT))
    if ctor is None:
        raise RuntimeError("Plugin \"%s\" not found for variant \"%s\". Available: %s" % (t, VARIANT, sorted(k[0] for k in _REGISTRY)))
    return ctor(props, named, key)


def _shape_common(m, props, named):
    for k, v in props.items():
        if isinstance(v, dict) and v.get('type') in ('ref',) or isinstance(v, dict) and v.get('type') in _BSDF_PLUGINS:
            obj = _resolve(v, named, k)
            if isinstance(obj, BSDF):
                m.bsdf = obj
        elif isinstance(v, BSDF):
            m.bsdf = v
        elif isinstance(v, dict) and v.get('type') == 'area':
            if m.emitter is not None:
                raise RuntimeError("Only a single Emitter child object can be specified per shape.")       # shape.cpp:25-27
            a = AreaLight(v)
            m.emitter = a.radiance; m.emitter_weight = a.sampling_weight; m.emitter_light = a
        elif isinstance(v, dict) and 'type' in v and k not in ('to_world',):
            if _plugin_kind(v['type']) == 'emitter':     # Shape::initialize -> Emitter::set_shape: only surface emitters attach to a shape (point.cpp / spot.cpp / ... have no set_shape use)
                raise RuntimeError("Plugin \"%s\" is not a surface emitter: only `area` can be the child of a shape" % v['type'])
    return m


def _mk_scene(props, named, key):
    _check_props('scene', props, (), children=_ALL_KINDS)                 # Scene(props) (scene.cpp:26-70) walks props.objects(): children under any name, no other property
    children = {}
    for k, v in props.items():
        if k == 'type':
            continue
        if isinstance(v, dict) and v.get('type') in _BSDF_PLUGINS:
            named[k] = _create(v, named, k); children[k] = named[k]
    for k, v in props.items():
        if k == 'type' or k in children:
            continue
        obj = _resolve(v, named, k) if isinstance(v, dict) else v
        if isinstance(obj, (Mesh, Sensor, Integrator, BSDF, ShapeGroup, Instance, ConstantEmitter, EnvmapEmitter, PointLight, SpotLight, DirectionalEmitter, Projector)):
            if isinstance(obj, ShapeGroup):
                named[k] = obj
            children[k] = obj
    return Scene(children)


def _mk_shapegroup(props, named, key):
    _check_props('shapegroup', props, (), children=('shape',))            # ShapeGroup(props) (src/shapes/shapegroup.cpp): the child shapes, nothing else
    shapes = []; keys = []
    for k, v in props.items():
        if isinstance(v, dict) and 'type' in v:
            obj = _resolve(v, named, k)
            if isinstance(obj, Mesh):
                shapes.append(obj); keys.append(k)
        elif isinstance(v, Mesh):
            shapes.append(v); keys.append(k)
    g = ShapeGroup(shapes, keys)
    if key:
        named[key] = g
    return g


def _mk_instance(props, named, key):
    _check_props('instance', props, ('to_world',), children=('shape',))   # Instance(props) (src/shapes/instance.cpp:60-77)
    group = None
    for k, v in props.items():
        obj = _resolve(v, named, k) if isinstance(v, dict) else v
        if isinstance(obj, ShapeGroup):
            if group is not None:
                raise RuntimeError("Only a single shapegroup can be specified per instance.")
            group = obj
    if group is None:
        raise RuntimeError("A reference to a 'shapegroup' must be specified!")
    return Instance(group, props.get('to_world', ScalarTransform4f()))


def _mk_ply(props, named, key):
    _check_props('ply', props, _SHAPE_PROPS + ('filename', 'flip_tex_coords'), children=_SHAPE_CHILDREN)      # ply.cpp:113-118 over Mesh(props)
    if 'filename' not in props:
        raise RuntimeError("ply: the `filename` parameter is required")
    m = Mesh(key or "ply").from_ply(props['filename'], props.get('face_normals', False), props.get('flip_tex_coords', False),
                                    props.get('to_world'), props.get('flip_normals', False))
    return _shape_common(m, props, named)


def _mk_obj(props, named, key):
    _check_props('obj', props, _SHAPE_PROPS + ('filename', 'flip_tex_coords'), children=_SHAPE_CHILDREN)      # obj.cpp:98-113
    if 'filename' not in props:
        raise RuntimeError("obj: the `filename` parameter is required")
    m = Mesh(key or "obj").from_obj(props['filename'], props.get('face_normals', False), props.get('flip_tex_coords', True),
                                    props.get('to_world'), props.get('flip_normals', False))
    return _shape_common(m, props, named)


def _mk_serialized(props, named, key):
    _check_props('serialized', props, _SHAPE_PROPS + ('filename', 'shape_index'), children=_SHAPE_CHILDREN)   # serialized.cpp:225-244
    if 'filename' not in props:
        raise RuntimeError("serialized: the `filename` parameter is required")
    m = Mesh(key or "serialized").from_serialized(props['filename'], props.get('shape_index', 0), props.get('face_normals', None),
                                                  props.get('to_world'), props.get('flip_normals', False))
    return _shape_common(m, props, named)


def _mk_mesh(props, named, key):
    # not a reference plugin: the dict form of mi.Mesh(...) + params (faces / positions / normals / texcoords arrays)
    _check_props('mesh', props, ('faces', 'positions', 'normals', 'texcoords', 'attributes', 'to_world', 'silhouette_sampling_weight'), children=_SHAPE_CHILDREN)
    m = Mesh(key or "mesh").from_fields(props['faces'], props['positions'], props.get('normals'), props.get('texcoords'))
    for name, values in (props.get('attributes') or {}).items():          # {name: (rows, dim) array}: Mesh::add_attribute for each
        m.add_attribute(name, values)
    if 'to_world' in props:
        m.transform(props['to_world'])
    return _shape_common(m, props, named)


for _name, _fn in {
    'scene': _mk_scene,
    'path': lambda p, n, k: Integrator(p),
    'prb': lambda p, n, k: Integrator(p),
    'aov': lambda p, n, k: AOVIntegrator(p, n),
    'perspective': lambda p, n, k: Sensor({kk: (_resolve(v, n, kk) if isinstance(v, dict) and 'type' in v else v) for kk, v in p.items()}),      # EVERY child object through the registry
    'orthographic': lambda p, n, k: Sensor({kk: (_resolve(v, n, kk) if isinstance(v, dict) and 'type' in v else v) for kk, v in p.items()}),
    'thinlens': lambda p, n, k: Sensor({kk: (_resolve(v, n, kk) if isinstance(v, dict) and 'type' in v else v) for kk, v in p.items()}),
    'batch': lambda p, n, k: BatchSensor({kk: (_resolve(v, n, kk) if isinstance(v, dict) and 'type' in v else v) for kk, v in p.items()}),
    'hdrfilm': lambda p, n, k: Film(p),
    'independent': lambda p, n, k: Sampler(p),
    'diffuse': lambda p, n, k: BSDF(p, id=k), 'dielectric': lambda p, n, k: BSDF(p, id=k), 'roughconductor': lambda p, n, k: BSDF(p, id=k),
    'roughplastic': lambda p, n, k: BSDF(p, id=k), 'conductor': lambda p, n, k: BSDF(p, id=k), 'plastic': lambda p, n, k: BSDF(p, id=k), 'thindielectric': lambda p, n, k: BSDF(p, id=k), 'twosided': _mk_twosided, 'blendbsdf': _mk_blendbsdf, 'mask': _mk_mask, 'normalmap': _mk_normalmap, 'bumpmap': _mk_bumpmap, 'constant': lambda p, n, k: ConstantEmitter(p), 'envmap': lambda p, n, k: EnvmapEmitter(p), 'point': lambda p, n, k: PointLight(p), 'spot': lambda p, n, k: SpotLight(p), 'directional': lambda p, n, k: DirectionalEmitter(p), 'projector': lambda p, n, k: Projector(p),
    'rectangle': lambda p, n, k: _shape_common(_rectangle(p), p, n),
    'cube': lambda p, n, k: _shape_common(_cube(p), p, n),
    'mesh': _mk_mesh, 'ply': _mk_ply, 'obj': _mk_obj, 'serialized': _mk_serialized,
    'shapegroup': _mk_shapegroup,
    'instance': _mk_instance,
    'gaussian': lambda p, n, k: p, 'box': lambda p, n, k: p, 'rgb': lambda p, n, k: Texture(p), 'bitmap': lambda p, n, k: Texture(p), 'mesh_attribute': lambda p, n, k: Texture(p), 'area': lambda p, n, k: p,
}.items():
    register_plugin(_name, VARIANT, _fn)


def register_integrator(name, fn):
    """mi.register_integrator (src/render/python/scene_v.cpp:166-171)."""
    register_plugin(name, VARIANT, lambda p, n, k: fn(p))


def load_dict(d):
    """mi.load_dict (src/core/python/parser.cpp:561)."""
    if _variant is None:
        set_variant(VARIANT)
    return _create(d, {}, None)


# ---------------------------------------------------------------------------
#  mi.render + _RenderOp (src/python/python/util.py:344-528) as a torch autograd Function
# ---------------------------------------------------------------------------

def sample_tea_32(v0, v1, rounds=4):
    v0 &= 0xffffffff; v1 &= 0xffffffff; s = 0
    for _ in range(rounds):
        s = (s + 0x9e3779b9) & 0xffffffff
        v0 = (v0 + ((((v1 << 4) & 0xffffffff) + 0xa341316c) ^ ((v1 + s) & 0xffffffff) ^ ((v1 >> 5) + 0xc8013ea4))) & 0xffffffff
        v1 = (v1 + ((((v0 << 4) & 0xffffffff) + 0xad90777d) ^ ((v0 + s) & 0xffffffff) ^ ((v0 >> 5) + 0x7e95761e))) & 0xffffffff
    return v0, v1


def render(scene, params=None, sensor=0, integrator=None, seed=0, seed_grad=0, spp=0, spp_grad=0):
    torch = _torch()
    if integrator is None:
        integrator = scene.integrator()
    if integrator is None:
        raise Exception('No integrator specified! Add an integrator in the scene description or provide an integrator directly as argument.')
    if isinstance(sensor, int):
        if len(scene.sensors()) == 0:
            raise Exception('No sensor specified! Add a sensor in the scene description or provide a sensor directly as argument.')
        sensor = scene.sensors()[sensor]
    if spp_grad == 0:
        spp_grad = spp
    if seed_grad == 0:
        seed_grad = sample_tea_32(seed, 1)[0]
    elif seed_grad == seed:
        raise Exception('The primal and differential seed should be different to ensure unbiased gradient computation!')
    if _variant == SCALAR_VARIANT:
        if any(getattr(v, 'requires_grad', False) for v in (params or {}).values()):
            raise RuntimeError("scalar_rgb renders are not differentiable (the reference's scalar variants have no AD either); use hip_ad_rgb")
        return _render_scalar(scene, integrator, sensor, seed, spp)
    keys = [k for k, v in (params or {}).items() if getattr(v, 'requires_grad', False)]
    fixed = [k for k in keys if k in scene._pose_keys() and scene._pose_keys()[k][0] not in ("emitter_tex", "env_data", "env_scale", "proj_scale")]      # (a light's radiance bitmap IS differentiable: area.cpp:64-70; an environment map's `data` and `scale`: envmap.cpp:203-208)
    if fixed:       # ParamFlags::NonDifferentiable in the reference's traverse(): dr.enable_grad on them has no effect there; here it is said
        raise RuntimeError("%s are not differentiable parameters in hip_ad_rgb (placement of sensors and delta emitters: ParamFlags::NonDifferentiable in the reference; "
                           "a spot light's cutoff_angle / beam_width: Differentiable there, updatable but without a gradient here)" % fixed)
    scales = [k for k in keys if scene._bsdf_param_keys().get(k, (None,))[0] == "scale"]
    if scales:       # BumpMap::traverse registers `scale` as ParamFlags::NonDifferentiable (bumpmap.cpp:134)
        raise RuntimeError("%s: the `scale` of a `bumpmap` is not a differentiable parameter (ParamFlags::NonDifferentiable; the height map's texels are)" % scales)
    nested = [k for k in keys if k in scene._bsdf_param_keys() and id(scene._bsdf_param_keys()[k][1]) in scene._blend_nested()]
    if nested:
        raise RuntimeError("%s: the non-colour parameters of a BSDF nested in a `blendbsdf` / `mask` / `normalmap` / `bumpmap` have no gradient in hip_ad_rgb (a blend's `weight`, a mask's `opacity` and the colour slot 0 of the BSDFs nested in them do)" % nested)
    amap_nested = [k for k in keys if getattr(scene._param_keys().get(k, (None, None))[1], 'kind', None) == 'alphamap' and id(scene._param_keys()[k][1].owner) in scene._blend_nested()]
    if amap_nested:
        raise RuntimeError("%s: the alpha texels of a roughness map on a BSDF nested in a `blendbsdf` / `mask` / `normalmap` / `bumpmap` have no gradient in hip_ad_rgb (the map renders there; "
                           "under a plain or `twosided` roughconductor its texels are differentiated)" % amap_nested)
    if not keys:
        return integrator.render(scene, sensor, seed, spp)
    params.update()
    # dr.enable_grad(params[key]) is what makes a parameter differentiable in the reference: the adjoint terms the requested keys need are switched
    # on for THIS call's backward pass only -- the caller's integrator keeps its own properties (optimising vertex positions first and alpha
    # second with one integrator must not leave `shape_gradients` on for the second render)
    overrides = {}
    ad_targets = [integrator] if integrator.type == 'prb' else [c for c in integrator.children if c.type == 'prb'] if integrator.type == 'aov' else []
    if ad_targets:
        integrator_ad = ad_targets[0]
        shape_keys = [k for k in keys if k in scene._position_keys() or k in scene._instance_keys() or k in scene._rect_keys()]
        if shape_keys and integrator_ad.shape_gradients is not True:
            overrides['shape_gradients'] = sorted(set(list(integrator_ad.shape_gradients or [])) | set(shape_keys))
        if any((k in scene._bsdf_param_keys() and scene._bsdf_param_keys()[k][0] not in _THIN_PARAMS) or getattr(scene._param_keys().get(k, (None, None))[1], 'kind', None) == 'alphamap' for k in keys) and not integrator_ad.bsdf_parameter_gradients:
            overrides['bsdf_parameter_gradients'] = True
        proj_scales = [scene._pose_keys()[k][1] for k in keys if scene._pose_keys().get(k, (None,))[0] == "proj_scale"]          # a projector's `scale`: the switch of its irradiance
        if (any(scene._pose_keys().get(k, (None,))[0] == "emitter_tex" for k in keys) or any(scene.emitters[i].get("light") is not None for i in proj_scales)) and not integrator_ad.light_texel_gradients:
            overrides['light_texel_gradients'] = True
        if any(scene.emitters[i].get("light") is None for i in proj_scales) and not integrator_ad.emitter_gradients:
            overrides['emitter_gradients'] = True
        if any(scene._pose_keys().get(k, (None,))[0] in ("env_data", "env_scale") for k in keys) and not integrator_ad.envmap_gradients:
            overrides['envmap_gradients'] = True
        if any(v[0] == "emit" for k, v in scene._param_keys().items() if k in keys) and not integrator_ad.emitter_gradients:
            overrides['emitter_gradients'] = True

    class _RenderOp(torch.autograd.Function):
        @staticmethod
        def forward(ctx, *tensors):
            # no synchronisation: the frame is enqueued on the current stream like any torch op (a scene whose BVH is too deep for the traversal stacks is refused
            # at creation, so there is no device-side error left to wait for); Integrator.render() called directly still evaluates
            return integrator.render(scene, sensor, seed, spp, evaluate=False)

        @staticmethod
        def backward(ctx, grad_out):
            saved = [{k: getattr(t, k) for k in overrides} for t in ad_targets]
            try:
                for t in ad_targets:
                    for k, v in overrides.items():
                        setattr(t, k, v)
                grads = integrator.render_backward(scene, params, grad_out, sensor, seed_grad, spp_grad)
            finally:
                for t, old in zip(ad_targets, saved):
                    for k, v in old.items():
                        setattr(t, k, v)
            missing = [k for k in keys if k not in grads]
            if missing:       # e.g. emitter radiance with emitter_gradients=False, vertex positions without shape_gradients
                raise RuntimeError("mi.render(): the `prb` integrator cannot differentiate %s (integrator properties `emitter_gradients`, "
                                   "`shape_gradients`, `bsdf_parameter_gradients`, `light_texel_gradients`, `envmap_gradients`); differentiable keys of this render: %s" % (missing, sorted(grads)))
            return tuple(grads[k].reshape(params[k].shape) for k in keys)

    return _RenderOp.apply(*[params[k] for k in keys])
