"""'<rect>.positions' of a rectangle that carries an area light: the light samples the rectangle's frame (Rectangle::sample_position), not its triangles, so params.update() must
move the frame with the vertices -- the scene afterwards equals the scene loaded with to_world = T * to_world: same vertex records, same emitter record, same oracle render.
Positions that are not a parallelogram have no frame and are refused, the scene left as it was."""
import copy

import numpy as np
import pytest

from tests.test_textured_area_light_cpu import _bitmap, lit_box


def rect_light_box(mi, textured, res=24):
    """the Cornell box with its ceiling light: `rgb` radiance (emitter type 0) or a bitmap (type 7)"""
    if textured:
        return lit_box(mi, _bitmap(4), res)
    d = mi.cornell_box(); d["sensor"]["film"]["width"] = res; d["sensor"]["film"]["height"] = res
    return d


def light_move(mi):
    """translates, rotates and stretches -- the stretch along x, which lies in the light's plane, so that T keeps the length of the plane's normal (see Scene._rect_frame)"""
    return mi.ScalarTransform4f().translate([0.12, -0.15, 0.1]).rotate([0.6, 0.0, 0.8], 20.0).scale([1.4, 1.0, 1.0])


def moved(mi, d, positions):
    """(T * positions, the scene dict with the light at T * to_world)"""
    M = np.asarray(light_move(mi).matrix, np.float64).reshape(4, 4)
    P = np.asarray(positions, np.float64).reshape(-1, 3)
    d2 = copy.deepcopy(d); d2["light"]["to_world"] = light_move(mi) @ d["light"]["to_world"]
    return (P @ M[:3, :3].T + M[:3, 3]).astype(np.float32), d2


def light_records(scene):
    """(vertex records of the light's mesh, its emitter record)"""
    i = [m["key"] for m in scene.meshes].index("light")
    e = scene.emitters[scene.meshes[i]["emitter"]]
    rec = np.concatenate([np.asarray(e["to_world"], np.float64).ravel(), np.asarray(e["normal"], np.float64).ravel(), [e["inv_area"]]])
    return np.array(scene.meshes[i]["V"], np.float64), rec, e["type"]


def render_tolerance(textured):
    """the frame derived from the positions equals T * to_world to the last bit or two; a bitmap light turns that into texel-sampling differences of a few 1e-5"""
    return 1e-4 if textured else 1e-5


def assert_same_light(a, b, tol=1e-6):
    Va, ra, ta = light_records(a); Vb, rb, tb = light_records(b)
    assert ta == tb
    assert np.abs(Va - Vb).max() <= tol, np.abs(Va - Vb).max()
    assert np.abs(ra - rb).max() <= tol * max(1.0, np.abs(rb).max()), (ra, rb)


@pytest.mark.parametrize("textured", [False, True], ids=["rgb", "bitmap"])
def test_rect_light_positions_equal_a_fresh_load(mi, O, textured):
    import torch
    d = rect_light_box(mi, textured)
    a = mi.load_dict(d)
    params = mi.traverse(a)
    P, d2 = moved(mi, d, params["light.positions"].cpu().numpy())
    params["light.positions"] = torch.tensor(P); params.update()
    b = mi.load_dict(d2)
    assert_same_light(a, b)
    tw = mi.traverse(a)["light.to_world"].cpu().numpy()                 # the frame reads back too
    assert np.abs(tw - mi.traverse(b)["light.to_world"].cpu().numpy()).max() <= 1e-6
    oa, sa = O.scene_from_product(a); ob, sb = O.scene_from_product(b)
    ia, _ = oa.render_path(sa, seed=1, spp=8, max_depth=3); ib, _ = ob.render_path(sb, seed=1, spp=8, max_depth=3)
    assert np.abs(ib).max() > 0 and np.linalg.norm(ia - ib) <= render_tolerance(textured) * np.linalg.norm(ib)
    o0, s0 = O.scene_from_product(mi.load_dict(d))
    i0, _ = o0.render_path(s0, seed=1, spp=8, max_depth=3)
    assert np.linalg.norm(i0 - ib) > 0.05 * np.linalg.norm(ib)              # the light did move


@pytest.mark.parametrize("textured", [False, True], ids=["rgb", "bitmap"])
def test_rect_light_positions_that_are_no_parallelogram_are_refused(mi, textured):
    import torch
    scene = mi.load_dict(rect_light_box(mi, textured))
    params = mi.traverse(scene)
    V0, rec0, _ = light_records(scene)
    bad = params["light.positions"].cpu().numpy().copy(); bad[3] += np.float32(0.05)
    params["light.positions"] = torch.tensor(bad)
    with pytest.raises(RuntimeError, match=r"'light\.to_world'"):
        params.update()
    V1, rec1, _ = light_records(scene)
    assert np.array_equal(V0, V1) and np.array_equal(rec0, rec1)
