"""An independent reference for scenes changed through mi.traverse / params.update(): a FRESH load of the original scene dict with the final values written before its first
render (no scene handle: the plain host path; never a refit, a device-resident update or a failure path), and a read-back of what was written through a NEW mi.traverse.
The oracle renders of an updated scene are made from the scene's own host mirrors (oracle.scene_from_product): an update that loses a value loses it in the mirror too, and
the oracle then agrees with the wrong picture -- these helpers do not take the scene under test as their reference."""
import copy

import numpy as np

# keys whose stored form is derived from the written value, and how they are compared (everything else reads back bit for bit):
#   env_data        the reference's layout H x (W + 2) x 3: the halo columns are recomputed from the opposite edges (envmap.cpp:146-188) -- interior columns only, bit for bit
#   rect_positions  the four vertices of a rectangle LIGHT: its frame is derived from them and the vertices are re-baked from the frame (Scene._rect_frame) -- to 1e-6 of
#                   the largest coordinate
DERIVED = {"env_data": 0.0, "rect_positions": 1e-6}


def _numpy(v):
    return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float32)


def final_values(params, keys):
    """{key: a host copy of params[key]} -- what was last written, independent of later in-place edits of the parameter tensors"""
    import torch
    return {k: torch.as_tensor(_numpy(params[k]).copy()) for k in keys}


def fresh_reference(d, values):
    """the original scene dict loaded again, the final value of every written key set through mi.traverse before the first render"""
    import mitsuba3_amd as mi
    scene = mi.load_dict(copy.deepcopy(d))
    params = mi.traverse(scene)
    for k, v in values.items():
        params[k] = v
    params.update()
    assert scene._h is None
    return scene


def _derived_kind(scene, key):
    kind = scene._pose_keys().get(key, (None,))[0]
    if kind == "env_data":
        return kind
    m = scene._position_keys().get(key)
    if m is not None and scene.meshes[m].get("rect") is not None and scene.meshes[m]["emitter"] >= 0:
        return "rect_positions"
    return None


def assert_values_kept(scene, values):
    """every written key reads back what was last written, through a new mi.traverse after sync_host(): bit for bit, except the DERIVED kinds"""
    import mitsuba3_amd as mi
    scene.sync_host()
    params = mi.traverse(scene)
    for k, v in values.items():
        got = _numpy(params[k]); want = _numpy(v).reshape(got.shape)
        kind = _derived_kind(scene, k)
        if kind == "env_data":
            got, want = got[:, 1:-1], want[:, 1:-1]
        if kind is None or DERIVED[kind] == 0.0:
            assert np.array_equal(got, want), (k, np.abs(got.astype(np.float64) - want).max())
        else:
            err = np.abs(got.astype(np.float64) - want).max()
            assert err <= DERIVED[kind] * max(1.0, np.abs(want).max()), (k, kind, err)
