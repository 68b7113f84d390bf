"""Child process of tests/test_gpu_stack_spill.py: `python tests/stack_spill_worker.py <job> <out.npz>`.  The switches (HAR_FORCE_STACK_SPILL, HAR_TRACE_GRID,
HAR_STREAMS) are parsed once per process and a second build of the library cannot share a process with the first, so every configuration is a process of
its own; the environment comes from the parent.  A job renders / traces / differentiates and writes its arrays to one .npz -- it compares nothing: the
parent holds the oracle.  The scene and job tables below are imported by the parent too, so both sides describe the same work.

jobs: wave   -- the wavefront kernels on scenes that fit the LDS stack (parent: with and without HAR_FORCE_STACK_SPILL)
      stack3 -- the library built with -DHAR_LDS_STACK_SMALL=3 on scenes whose rays reach stack level >= 5 (entries in the HBM columns)
      grid8  -- the same library under HAR_TRACE_GRID=8: another gridDim.x, i.e. another column stride
      deep   -- scenes with a depth-first bound of 14 .. 30 (and 31: refused) on the default library"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import deep_cases as D               # noqa: E402

MD, RR = 5, 3                                   # max_depth / rr_depth of every job
STACK3_LIB = os.path.join(ROOT, "mitsuba3_amd", "libhip_ad_rgb_stack3.so")
LARGEST = np.float32(3.402823466e+38)
N_SAMPLE = 7680 - 37                            # full and partial batches on all eight shards, a ragged end
N_QUERY = 200000
AOV_TYPES = ["depth", "sh_normal", "shape_index"]
WAVE_PAIRS = [(name, kind) for name in ("cornell", "materials", "instanced_top") for kind in ("path", "prb")]


def integ(kind, **kw):
    return dict({"type": kind, "max_depth": MD, "rr_depth": RR}, **kw)


def scene_dict(mi, name, kind="path", res=32, **kw):
    if name == "cornell":
        d = mi.cornell_box(); d["sensor"]["film"]["width"] = res; d["sensor"]["film"]["height"] = res
    elif name == "materials":
        from tests.test_bsdfs_cpu import _material_cbox
        d = _material_cbox(mi, res)
    elif name == "instanced_top":               # 16 top-level triangles around three instances: the seeded closest-hit kernel without spill, bypassed with it
        from tests import top_seed_cases as TS
        d = TS.scene_dict(mi, 16, res=res)
    elif name == "hide":
        from tests.test_emitters_cpu import hide_emitters_scene
        d = hide_emitters_scene(mi, res); kw["hide_emitters"] = True
    elif name == "textured":
        d = mi.textured_cornell_box(res=res, tex_res=16, spp=8)
    elif name == "slab":
        from tests.test_shape_gradients_cpu import slab_scene
        d = slab_scene(mi, res); kw["shape_gradients"] = ["floor.positions", "ceiling.positions"]
    elif name in D.SPILL3:
        d = D.SPILL3[name](mi, res=res)
        if name.endswith("_panel"):
            kw["hide_emitters"] = True
    elif name in D.DEEP:
        d = D.DEEP[name](mi, res=res)
    else:
        raise KeyError(name)
    d["integrator"] = integ(kind, **kw)
    return d


def grad_image(res, seed=4):
    return np.random.default_rng(seed).uniform(0.5, 1.5, (res, res, 3)).astype(np.float32)


def sample_rays(name, n=N_SAMPLE, seed=11):
    if name in D.SPILL3 or name in D.DEEP:
        return D.case_rays(name, n, seed)
    rng = np.random.default_rng(seed)
    r = 3.5 if name == "instanced_top" else 0.8
    o = rng.uniform(-r, r, (3, n)).astype(np.float32)
    d = rng.normal(size=(3, n)); d = np.ascontiguousarray(d / np.linalg.norm(d, axis=0), np.float32)
    return o, d, np.full(n, LARGEST, np.float32)


def query_rays(name, n=N_QUERY):
    o, d, maxt = D.case_rays(name, n, seed=5)
    return o, d, maxt, np.random.default_rng(3).uniform(0.01, 3.0, n).astype(np.float32)


def forward_tangents(scene):
    """(tangents by key, t_refl, t_tex, t_emit): seeded, every key of the gradient tables"""
    trng = np.random.default_rng(17)
    tangents, t_refl, t_emit = {}, np.zeros((len(scene.bsdfs), 3), np.float32), np.zeros((max(1, len(scene.emitters)), 3), np.float32)
    t_tex = [np.zeros_like(np.asarray(t, np.float32)) for t in scene.textures]
    for k, (kind, b) in scene._param_keys().items():
        if kind == "tex":
            t_tex[b.tex_index] = trng.uniform(-1, 1, t_tex[b.tex_index].shape).astype(np.float32); tangents[k] = t_tex[b.tex_index]
        elif kind == "emit":
            t_emit[b] = trng.uniform(-1, 1, 3); tangents[k] = t_emit[b]
        else:
            t_refl[b.index] = trng.uniform(-1, 1, 3); tangents[k] = t_refl[b.index]
    return tangents, t_refl, t_tex, t_emit


# ------------------------------------------------------------------ what a job records

class Recorder:
    def __init__(self, mi):
        self.mi = mi; self.R = {}

    def render(self, key, d, spp, seed):
        scene = self.mi.load_dict(d)
        self.R["img." + key] = self.mi.render(scene, spp=spp, seed=seed).cpu().numpy()
        st = scene.integrator().stats()
        self.R["stats." + key] = np.array([st["paths"], st["vertices"]], np.int64)
        return scene

    def backward(self, key, d, res, spp, seed):
        scene = self.mi.load_dict(d)
        grads = scene.integrator().render_backward(scene, None, grad_image(res), seed=seed, spp=spp)
        for k, g in grads.items():
            self.R["grad.%s.%s" % (key, k)] = g.cpu().numpy()

    def sample(self, key, d, rays):
        mi = self.mi
        scene = mi.load_dict(d); o, dd, maxt = rays; n = o.shape[1]
        sampler = mi.Sampler({"sample_count": 4, "seed": 5}); sampler.seed(3, n)
        spec, valid = scene.integrator().sample(scene, sampler, mi.Ray3f(o, dd, maxt))
        self.R["sample.%s.spec" % key] = spec.cpu().numpy(); self.R["sample.%s.valid" % key] = valid.cpu().numpy().astype(np.uint8)
        self.R["sample.%s.state" % key] = sampler.state.cpu().numpy().view(np.uint64)

    def queries(self, key, scene, rays):
        mi = self.mi; o, d, maxt, maxt2 = rays
        for naive in (False, True):
            pi = scene._intersect(mi.Ray3f(o, d, maxt), naive)
            rec = [pi.t, pi.prim_uv[0], pi.prim_uv[1], pi.prim_index, pi.shape_index, pi.instance]
            for f, a in zip("tuvpsi", rec):
                a = a.cpu().numpy()
                self.R["rq.%s.%d.%s" % (key, naive, f)] = a if f in "tuv" else a.astype(np.uint32)
            self.R["rq.%s.%d.occluded" % (key, naive)] = scene.ray_test(mi.Ray3f(o, d, maxt2), naive=naive).cpu().numpy()


def job_wave(mi, rec):
    for name, kind in WAVE_PAIRS:
        rec.render("%s.%s" % (name, kind), scene_dict(mi, name, kind), 8, 3)
    rec.render("packet", scene_dict(mi, "cornell", res=16), 64, 2)                   # the packet kernel, then k_trace_closest<.., LIST> on what it hands over
    rec.render("hide", scene_dict(mi, "hide"), 8, 5)
    rec.render("chunks", scene_dict(mi, "cornell", chunk_lanes=2048), 8, 3)          # 32 x 32 x 8 lanes: four chunks
    rec.render("passes", scene_dict(mi, "cornell", samples_per_pass=2), 8, 3)
    rec.backward("textured", scene_dict(mi, "textured", "prb"), 32, 8, 11)           # record tape / replay cache
    rec.backward("textured_nocache", scene_dict(mi, "textured", "prb", replay_cache=False), 32, 8, 11)      # the adjoint through k_resolve<MODE_PRB_ADJOINT>
    rec.backward("slab", scene_dict(mi, "slab", "prb", res=24), 24, 16, 3)
    scene = mi.load_dict(scene_dict(mi, "textured", "prb"))
    rec.R["img.forward"] = scene.integrator().render_forward(scene, None, seed=6, spp=8, tangents=forward_tangents(scene)[0]).cpu().numpy()
    for name in ("cornell", "instanced_top"):
        for kind in ("path", "prb"):
            rec.sample("%s.%s" % (name, kind), scene_dict(mi, name, kind), sample_rays(name))


def job_stack3(mi, rec):
    L = D.harness()
    for name in ("comb", "instanced_soup"):
        scene = rec.render(name, scene_dict(mi, name), 8, 3)
        rec.R["depth." + name] = np.int64(scene.accel_info()["depth"])
        rec.queries(name, scene, query_rays(name))
        rec.backward(name, scene_dict(mi, name, "prb"), 32, 8, 11)
        rec.sample(name + ".path", scene_dict(mi, name), sample_rays(name))
    rec.render("hide", scene_dict(mi, "instanced_soup_panel"), 8, 5)
    rec.render("packet", scene_dict(mi, "comb", res=16), 64, 2)
    # the cap of this library: 3 + 20 entries
    for target in (D.STACK3_CAP, D.STACK3_CAP + 1):
        n = D.nest_with_need(L, mi, target)
        rec.R["cap.n%d" % target] = np.int64(-1 if n is None else n)
        try:
            rec.R["cap.depth%d" % target] = np.int64(mi.load_dict(D.nest_scene(mi, n, 1.1, res=16)).accel_info()["depth"])
        except mi.HarError as e:
            rec.R["cap.error%d" % target] = np.array(str(e))
    # two launch sequences in flight (the parent sets HAR_STREAMS=2): 2^20 lanes is the smallest job that is cut in two
    rec.render("two_streams", scene_dict(mi, "instanced_soup", res=256), 16, 7)


def job_grid8(mi, rec):
    rec.render("instanced_soup", scene_dict(mi, "instanced_soup"), 8, 3)
    rec.sample("comb.path", scene_dict(mi, "comb"), sample_rays("comb"))


def job_deep(mi, rec):
    for name in sorted(D.DEEP):
        scene = rec.render(name, scene_dict(mi, name), 8, 3)
        rec.R["depth." + name] = np.int64(scene.accel_info()["depth"])
        rec.queries(name, scene, query_rays(name))
        aov = mi.load_dict({"type": "aov", "aovs": ",".join("f%d:%s" % (i, t) for i, t in enumerate(AOV_TYPES))})
        rec.R["aov." + name] = aov.render(scene, seed=5, spp=8, develop=False).cpu().numpy()
        rec.backward(name, scene_dict(mi, name, "prb"), 32, 8, 11)
    try:
        mi.load_dict(D.OVER_DEEP(mi)).accel_info()
        rec.R["overdeep.error"] = np.array("")
    except mi.HarError as e:
        rec.R["overdeep.error"] = np.array(str(e))
    rec.render("after_refusal", scene_dict(mi, "cornell"), 8, 3)
    # a vertex update that makes a fitting scene one entry too deep: refused, and the scene keeps rendering what it held (1 spp, box filter: one sample per pixel,
    # so the film does not depend on the order of the atomics)
    d, key, P = D.update_case(mi)
    scene = mi.load_dict(d)
    rec.R["depth.update_before"] = np.int64(scene.accel_info()["depth"])
    rec.R["img.update_before"] = mi.render(scene, spp=1, seed=2).cpu().numpy()
    params = mi.traverse(scene)
    params[key] = P
    try:
        params.update()
        rec.R["update.error"] = np.array("")
    except RuntimeError as e:
        rec.R["update.error"] = np.array(str(e))
    rec.R["img.update_after"] = mi.render(scene, spp=1, seed=2).cpu().numpy()
    rec.R["depth.update_after"] = np.int64(scene.accel_info()["depth"])


JOBS = {"wave": job_wave, "stack3": job_stack3, "grid8": job_grid8, "deep": job_deep}


def main(job, out):
    from mitsuba3_amd import _capi
    if job in ("stack3", "grid8"):
        assert _capi._LIB is None, "the library was loaded before the variant could be chosen"
        _capi.LIB_PATH = STACK3_LIB
    import mitsuba3_amd as mi
    mi.set_variant("hip_ad_rgb")
    import torch
    rec = Recorder(mi)
    JOBS[job](mi, rec)
    torch.cuda.synchronize()
    np.savez(out, **rec.R)
    print("WORKER_OK", job, len(rec.R))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
