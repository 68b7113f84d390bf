"""Shared scenes of the `mesh_attribute` tests (test_mesh_attribute_cpu.py, test_gpu_mesh_attribute.py).

The product renders an indexed mesh M (shared vertices, no normals, no texcoords: flat shading) whose BSDF reads a mesh attribute.  The oracle has no such texture; it
renders the TWIN: the same triangles in the same order as a triangle soup with texcoords and a `bitmap` --

  * face attribute: a nearest bitmap with one texel per face, triangle f's uvs strictly inside texel f, texel f = face_color[f];
  * vertex attribute: a bilinear, clamped bitmap with one 2 x 2 texel cell per face.  In cell coordinates (x, y) in [0, 1]^2 between the four texel centres the face's
    uv island is (0.1, 0.1), (0.9, 0.1), (0.1, 0.9); the texels are the values at the cell's corners of the affine function through the three vertex colours at the
    island's corners (float64).  Bilinear interpolation of affine texels is that function, i.e. the barycentric blend.

The cells are laid out on a near-square grid, so that a float32 uv resolves a cell coordinate to about cols * 2^-23.
"""
import numpy as np

ISLAND = ((0.1, 0.1), (0.9, 0.1), (0.1, 0.9))
# b_k = alpha_k + beta_k x + gamma_k y on the island: b1 = (x - 0.1) / 0.8, b2 = (y - 0.1) / 0.8, b0 = 1 - b1 - b2
ALPHA = np.array([1.25, -0.125, -0.125]); BETA = np.array([-1.25, 1.25, 0.0]); GAMMA = np.array([-1.25, 0.0, 1.25])


def grid_mesh(nx, ny, center=(0.0, -0.15, 0.35), ex=(0.62, 0.0, 0.12), ey=(0.0, 0.55, -0.2), jitter=0.0, seed=1):
    """an indexed nx x ny grid (2 nx ny triangles, (nx + 1)(ny + 1) shared vertices) spanned by +-ex, +-ey around `center`, facing the camera of mi.cornell_box()"""
    c, ex, ey = (np.asarray(a, np.float64) for a in (center, ex, ey))
    rng = np.random.default_rng(seed)
    P = []
    for j in range(ny + 1):
        for i in range(nx + 1):
            s, t = 2.0 * i / nx - 1.0, 2.0 * j / ny - 1.0
            if jitter and 0 < i < nx and 0 < j < ny:
                s += jitter * rng.uniform(-1, 1) / nx; t += jitter * rng.uniform(-1, 1) / ny
            P.append(c + s * ex + t * ey)
    F = []
    for j in range(ny):
        for i in range(nx):
            v00 = j * (nx + 1) + i; v10 = v00 + 1; v01 = v00 + nx + 1; v11 = v01 + 1
            F.append([v00, v10, v11]); F.append([v00, v11, v01])
    return np.asarray(P, np.float32), np.asarray(F, np.uint32)


def vertex_colors(n, dim=3, seed=5, lo=0.35, hi=0.6):
    """colours from [0.35, 0.6] (a sub-range of [0.3, 0.6]): the affine function of a face reaches c0 + 1.125 (d1 + d2) at the far corner of its cell, which [0.35, 0.6] keeps inside (0, 1)"""
    return np.random.default_rng(seed).uniform(lo, hi, (n, dim)).astype(np.float32)


def cell_layout(nf):
    cols = int(np.ceil(np.sqrt(nf))); rows = (nf + cols - 1) // cols
    return cols, rows


def soup(P, F):
    """the same triangles in the same order without shared vertices: (positions 3 nf x 3, faces nf x 3)"""
    return np.ascontiguousarray(P[F.reshape(-1)], np.float32), np.arange(3 * F.shape[0], dtype=np.uint32).reshape(-1, 3)


def vertex_twin(P, F, colors):
    """(soup positions, soup faces, texcoords, bitmap H x W x 3) of the vertex-attribute twin; a one-channel attribute is broadcast first"""
    col = np.asarray(colors, np.float64)
    if col.shape[1] == 1:
        col = np.repeat(col, 3, axis=1)
    nf = F.shape[0]; cols, rows = cell_layout(nf)
    W, H = 2 * cols, 2 * rows
    tex = np.full((H, W, 3), 0.5, np.float64); uv = np.zeros((3 * nf, 2), np.float64)
    for f in range(nf):
        r, c = divmod(f, cols)
        c0, c1, c2 = col[F[f, 0]], col[F[f, 1]], col[F[f, 2]]
        B = (c1 - c0) / 0.8; Cc = (c2 - c0) / 0.8; A = c0 - 0.1 * B - 0.1 * Cc
        tex[2 * r, 2 * c] = A; tex[2 * r, 2 * c + 1] = A + B; tex[2 * r + 1, 2 * c] = A + Cc; tex[2 * r + 1, 2 * c + 1] = A + B + Cc
        for k, (x, y) in enumerate(ISLAND):
            uv[3 * f + k] = ((2 * c + 0.5 + x) / W, (2 * r + 0.5 + y) / H)
    assert tex.min() > 0.0 and tex.max() < 1.0
    Ps, Fs = soup(P, F)
    return Ps, Fs, uv.astype(np.float32), tex.astype(np.float32)


def vertex_gradient_from_texels(F, n_vertices, G):
    """the twin's texel gradients G (H x W x 3) carried to the vertices: face f contributes alpha_k Sg + beta_k Sxg + gamma_k Syg to its k-th vertex, with
    Sg = G00 + G10 + G01 + G11, Sxg = G10 + G11, Syg = G01 + G11 of its cell"""
    G = np.asarray(G, np.float64); nf = F.shape[0]; cols, _ = cell_layout(nf)
    out = np.zeros((n_vertices, 3), np.float64)
    for f in range(nf):
        r, c = divmod(f, cols)
        g00, g10, g01, g11 = G[2 * r, 2 * c], G[2 * r, 2 * c + 1], G[2 * r + 1, 2 * c], G[2 * r + 1, 2 * c + 1]
        sg, sxg, syg = g00 + g10 + g01 + g11, g10 + g11, g01 + g11
        for k in range(3):
            out[F[f, k]] += ALPHA[k] * sg + BETA[k] * sxg + GAMMA[k] * syg
    return out


def face_twin(P, F, colors):
    """(soup positions, soup faces, texcoords, nearest bitmap rows x cols x 3): triangle f strictly inside texel f"""
    col = np.asarray(colors, np.float32)
    if col.shape[1] == 1:
        col = np.repeat(col, 3, axis=1)
    nf = F.shape[0]; cols, rows = cell_layout(nf)
    tex = np.full((rows, cols, 3), 0.5, np.float32); uv = np.zeros((3 * nf, 2), np.float64)
    for f in range(nf):
        r, c = divmod(f, cols)
        tex[r, c] = col[f]
        for k, (x, y) in enumerate(((0.3, 0.3), (0.7, 0.3), (0.3, 0.7))):
            uv[3 * f + k] = ((c + x) / cols, (r + y) / rows)
    Ps, Fs = soup(P, F)
    return Ps, Fs, uv.astype(np.float32), tex


def face_gradient_from_texels(nf, G):
    G = np.asarray(G, np.float64); cols, _ = cell_layout(nf)
    return np.stack([G[divmod(f, cols)] for f in range(nf)])


def base_scene(mi, res, spp, integrator="path", max_depth=6, rr_depth=7):
    d = mi.cornell_box()
    d["sensor"]["film"]["width"] = res[0]; d["sensor"]["film"]["height"] = res[1]
    d["sensor"]["sampler"] = {"type": "independent", "sample_count": spp}
    d["integrator"] = {"type": integrator, "max_depth": max_depth, "rr_depth": rr_depth}
    return d


def attr_bsdf(name, scale=None, twosided=False):
    tex = {"type": "mesh_attribute", "name": name}
    if scale is not None:
        tex["scale"] = scale
    b = {"type": "diffuse", "reflectance": tex}
    return {"type": "twosided", "inner": b} if twosided else b


def bitmap_bsdf(tex, nearest, twosided=False):
    t = {"type": "bitmap", "data": tex, "raw": True, "filter_type": "nearest" if nearest else "bilinear", "wrap_mode": "clamp"}
    b = {"type": "diffuse", "reflectance": t}
    return {"type": "twosided", "inner": b} if twosided else b


def product_shape(P, F, name, values, scale=None, twosided=False):
    return {"type": "mesh", "faces": F, "positions": P, "attributes": {name: values}, "bsdf": attr_bsdf(name, scale, twosided)}


def twin_shape(P, F, name, values, twosided=False):
    if name.startswith("vertex_"):
        Ps, Fs, uv, tex = vertex_twin(P, F, values)
        return {"type": "mesh", "faces": Fs, "positions": Ps, "texcoords": uv, "bsdf": bitmap_bsdf(tex, False, twosided)}
    Ps, Fs, uv, tex = face_twin(P, F, values)
    return {"type": "mesh", "faces": Fs, "positions": Ps, "texcoords": uv, "bsdf": bitmap_bsdf(tex, True, twosided)}


def pair(mi, res, spp, meshes, first=False, **kw):
    """(product dict, twin dict): mi.cornell_box() plus the meshes [(key, P, F, attribute name, values, options)]; `first`: the meshes are declared BEFORE the box's
    shapes (vertex / face offsets 0), otherwise behind the two cubes"""
    out = []
    for product in (True, False):
        base = base_scene(mi, res, spp, **kw)
        shapes = {}
        for key, P, F, name, values, opt in meshes:
            if product:
                shapes[key] = product_shape(P, F, name, values, opt.get("scale"), opt.get("twosided", False))
            else:
                v = np.asarray(values, np.float32) * np.float32(opt.get("scale", 1.0) if opt.get("scale") is not None else 1.0)
                shapes[key] = twin_shape(P, F, name, v, opt.get("twosided", False))
        if first:
            d = {k: v for k, v in base.items() if not (isinstance(v, dict) and v.get("type") in ("rectangle", "cube"))}
            d.update(shapes); d.update({k: v for k, v in base.items() if k not in d})
        else:
            d = dict(base); d.update(shapes)
        out.append(d)
    return out


def barycentric_reference(P, F, prim, p):
    """Mesh::barycentric_coordinates (src/render/mesh.cpp:2227-2251) in float64: rows of (b0, b1, b2) for hits at points p (n x 3) on faces `prim`"""
    P = np.asarray(P, np.float64); p = np.asarray(p, np.float64)
    p0, p1, p2 = P[F[prim, 0]], P[F[prim, 1]], P[F[prim, 2]]
    rel, du, dv = p - p0, p1 - p0, p2 - p0
    dot = lambda a, b: (a * b).sum(1)
    b1, b2, a11, a12, a22 = dot(du, rel), dot(dv, rel), dot(du, du), dot(du, dv), dot(dv, dv)
    inv_det = 1.0 / (a11 * a22 - a12 * a12)
    u = (a22 * b1 - a12 * b2) * inv_det; v = (a11 * b2 - a12 * b1) * inv_det
    return np.stack([1.0 - u - v, u, v], 1)
