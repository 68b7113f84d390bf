"""Scenes and helpers shared by tests/test_envmap_grad_cpu.py and tests/test_gpu_envmap_grad.py: a floor, a diffuse box and a rough-conductor box under an environment map
(envmap.cpp), the maps the gradient tests run over, luminance-free texel directions and the float64 restatement of the transpose of the map's bilinear lookup."""
import numpy as np

LUMINANCE = np.float64([0.212671, 0.715160, 0.072169])         # luminance() of linear sRGB (color.h), what the map's sampling distribution is built from (envmap.cpp:468-528)
FILM = (32, 24)                                                  # width, height of the device tests; spp 16
MAPS = ("8x4", "6x5", "rotated", "mis", "zeros")


def env_image(name, seed=11):
    """H x W x 3 texels in [0.2, 1.2]: 8 x 4; 6 x 5 (no power of two: the hierarchy pads it); `zeros`: 8 x 4 with a 2 x 2 block of texels that are exactly 0"""
    w, h = (6, 5) if name == "6x5" else (8, 4)
    img = np.random.default_rng(seed).uniform(0.2, 1.2, (h, w, 3)).astype(np.float32)
    if name == "zeros":
        img[1:3, 2:4] = 0.0
    return img


ZERO_BLOCK = (slice(1, 3), slice(2, 4))


def env_scene_dict(mi, name="8x4", *, scale=0.7, hide=False, area=False, closed=False, wall=None, grey=False, integrator="prb", max_depth=4, rr_depth=3, spp=16,
                   film=FILM, image=None, props=None):
    """the scene of the gradient tests as a dictionary.  `name`: one of MAPS (`rotated`: to_world turned about two axes, `mis`: mis_compensation); `area`: an area light next to
    the map; `closed`: a back wall so that no camera ray escapes (hide_emitters changes nothing then); `wall`: texels of a bitmap on that wall; `grey`: colourless materials"""
    T = mi.ScalarTransform4f
    img = env_image(name) if image is None else np.asarray(image, np.float32)
    d = {"type": "scene",
         "integrator": dict({"type": integrator, "max_depth": max_depth, "rr_depth": rr_depth}, **(props or {})),
         "sensor": mi.cornell_box()["sensor"],
         "white": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.6, 0.6, 0.6] if grey else [0.75, 0.6, 0.45]}},
         "metal": {"type": "roughconductor", "alpha": 0.35} if grey else {"type": "roughconductor", "alpha": 0.35, "eta": {"type": "rgb", "value": [0.2, 0.92, 1.1]}, "k": {"type": "rgb", "value": [3.9, 2.45, 2.14]}},
         "floor": {"type": "rectangle", "to_world": T().translate([0.0, -1.0, 0.0]).rotate([1, 0, 0], -90).scale(3.0), "bsdf": {"type": "ref", "id": "white"}},
         "box": {"type": "cube", "to_world": T().translate([-0.45, -0.6, 0.1]).rotate([0, 1, 0], 25).scale(0.4), "bsdf": {"type": "ref", "id": "white"}},
         "rough": {"type": "cube", "to_world": T().translate([0.5, -0.65, -0.2]).rotate([0, 1, 0], -20).scale(0.35), "bsdf": {"type": "ref", "id": "metal"}},
         "env": {"type": "envmap", "bitmap": mi.Bitmap(img), "scale": scale, "mis_compensation": name == "mis"}}
    if hide:
        d["integrator"]["hide_emitters"] = True
    d["sensor"]["film"]["width"], d["sensor"]["film"]["height"] = film
    d["sensor"]["sampler"]["sample_count"] = spp
    if name == "rotated":
        d["env"]["to_world"] = T().rotate([0, 1, 0], 40).rotate([1, 0, 0], 25)
    if area:
        d["lamp"] = {"type": "rectangle", "to_world": T().translate([0.0, 0.6, 0.3]).rotate([1, 0, 0], 90).scale(0.25), "bsdf": {"type": "ref", "id": "white"},
                     "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [4.0, 3.0, 2.0]}}}
    if closed or wall is not None:
        bsdf = {"type": "ref", "id": "white"} if wall is None else {"type": "diffuse", "reflectance": {"type": "bitmap", "data": np.asarray(wall, np.float32)}}
        d["back"] = {"type": "rectangle", "to_world": T().translate([0.0, 1.0, -1.5]).scale([4.0, 2.0, 1.0]), "bsdf": bsdf}
    return d


def halo(img):
    """the parameter's layout H x (W + 2) x 3 (envmap.cpp:146-188): real column x at x + 1, halo columns copy the opposite edge"""
    return np.ascontiguousarray(np.concatenate([img[:, -1:], img, img[:, :1]], axis=1))


def luminance_free(img, support, rng, amplitude=0.9):
    """a direction delta (H x W x 3, zero outside the boolean mask `support`) with luminance(delta_t) = 0 at every texel and |delta_tc| <= amplitude * img_tc: the map's sampling
    distribution, built from the texels' luminance alone, does not change along it, and img +- eps * delta stays positive for eps <= 1.  Per texel a random vector is projected
    onto the plane orthogonal to the luminance coefficients (float64), then scaled to the largest admissible length"""
    h, w, _ = img.shape
    out = np.zeros((h, w, 3), np.float64)
    for y, x in zip(*np.nonzero(support)):
        v = rng.normal(size=3)
        v -= LUMINANCE * (v @ LUMINANCE) / (LUMINANCE @ LUMINANCE)
        out[y, x] = v * amplitude * np.min(img[y, x].astype(np.float64) / np.maximum(np.abs(v), 1e-12))
    return out


def block_masks(h, w):
    """eight disjoint texel blocks covering an h x w map: the columns split in four, the rows in two"""
    xs = np.array_split(np.arange(w), 4); ys = np.array_split(np.arange(h), 2)
    masks = []
    for ry in ys:
        for rx in xs:
            m = np.zeros((h, w), bool); m[np.ix_(ry, rx)] = True; masks.append(m)
    return masks


def taps_f64(u, v, w, h):
    """the four taps of the map's bilinear lookup, restated in float64 and independently of the library: the lookup runs on the halo'ed storage (W + 2 columns, clamped;
    envmap.cpp:531-548), whose column 0 copies real column W - 1 and whose column W + 1 copies real column 0 -- [(row, real column, weight)] * 4"""
    u = np.float64(u); v = np.float64(v)
    u = u - np.floor(u); v = min(max(v, 0.0), 1.0)
    px = (u * w + 1.0) / (w + 2.0) * (w + 2.0) - 0.5          # texel coordinates in the storage
    py = (v * (h - 1.0) + 0.5) / h * h - 0.5
    x0 = int(np.floor(px)); y0 = int(np.floor(py)); fx = px - x0; fy = py - y0
    out = []
    for dy, wy in ((0, 1.0 - fy), (1, fy)):
        for dx, wx in ((0, 1.0 - fx), (1, fx)):
            sx = min(max(x0 + dx, 0), w + 1); sy = min(max(y0 + dy, 0), h - 1)
            out.append((sy, (sx - 1) % w, wx * wy))
    return out


def uv_to_direction(u, v):
    """the local direction whose lookup is (u, v) (envmap.cpp:454-459 inverted)"""
    phi = 2.0 * np.pi * np.asarray(u, np.float64); theta = np.pi * np.asarray(v, np.float64)
    return np.stack([np.sin(phi) * np.sin(theta), np.cos(theta), -np.cos(phi) * np.sin(theta)], -1)


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
