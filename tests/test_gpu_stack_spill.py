"""The traversal kernels' SECOND family on the GPU: HybridStack<13, 20> (13 stack entries in LDS, the rest in per-thread HBM columns) with the loop it keeps
(kSelectRefill = false), and the 30-entry ray-query / aov kernels -- what runs when HostScene::stack_need() exceeds the LDS entries or HAR_FORCE_STACK_SPILL is set.

  A  the spill kernels on scenes that fit (default library, HAR_FORCE_STACK_SPILL=1) against the oracle, and against the same process without the switch;
  B  entries really in HBM: a library built with -DHAR_LDS_STACK_SMALL=3 on scenes whose rays reach stack level >= 5 (tests/test_deep_bvh_cpu.py holds that),
     two grid sizes (= column strides), two launch sequences in flight, its cap of 23 entries;
  C  scenes with a depth-first bound of 14 .. 30 on the default library (dispatch, k_aov_trace<30>, the 30-entry ray queries), 31 refused at creation and
     at a vertex update.  Their rays reach levels 1 .. 8 only: on the default library NO test touches the HBM columns -- B does that.

Every configuration is a child process (tests/stack_spill_worker.py; the switches are parsed once per process) that writes its arrays to tmp_path; the parent
compares them with the oracle.  A child that dies of a signal, aborts, or runs into its time limit ends the module: nothing more is started on the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import deep_cases as D
from tests import stack_spill_worker as W

pytestmark = pytest.mark.gpu
ROOT = W.ROOT
MD, RR = W.MD, W.RR

# films of the same lanes whose atomic sums ran in another order: the bound tests/test_gpu_parity.py::test_forward_chunked_equals_single holds chunked / banded
# films to (`assert rel_l2(a, ref) < 1e-4`); gradients: tests/test_gpu_workspace_fallback.py (`< 2e-4`: "same lanes, same seeds: only the order of the atomic sums differs")
FILM_ORDER_TOL = 1e-4
GRAD_ORDER_TOL = 2e-4

_DEAD = []                      # why the module stopped starting processes
_RESULTS = {}
TIMEOUT = {"spill": 150, "plain": 150, "stack3": 200, "grid8": 90, "deep": 200}
CHILD = {"spill": ("wave", {"HAR_FORCE_STACK_SPILL": "1"}), "plain": ("wave", {}), "stack3": ("stack3", {"HAR_STREAMS": "2"}), "grid8": ("grid8", {"HAR_TRACE_GRID": "8"}),
         "deep": ("deep", {})}
FAULT_WORDS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "Aborted", "Segmentation fault")


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


def _child(name, tmp):
    """the arrays of child `name`, run once per session"""
    if name in _RESULTS:
        if _RESULTS[name] is None:
            pytest.fail("child %r failed earlier in this module" % name)
        return _RESULTS[name]
    if _DEAD:
        pytest.fail("no further GPU process is started: " + _DEAD[0])
    job, extra = CHILD[name]
    env = {k: v for k, v in os.environ.items() if k not in ("HAR_FORCE_STACK_SPILL", "HAR_TRACE_GRID", "HAR_STREAMS", "HAR_LIB_PATH")}
    env.update(extra)
    out = str(tmp / (name + ".npz"))
    _RESULTS[name] = None
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stack_spill_worker.py"), job, out], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=TIMEOUT[name])
    except subprocess.TimeoutExpired as e:
        _DEAD.append("child %r ran into its time limit of %d s" % (name, TIMEOUT[name]))
        pytest.fail(_DEAD[0] + "\n" + str(e.stdout or "")[-3000:])
    if p.returncode < 0 or p.returncode in (134, 139) or any(w in p.stdout for w in FAULT_WORDS):
        _DEAD.append("child %r ended with return code %d" % (name, p.returncode))
        pytest.fail(_DEAD[0] + "\n" + p.stdout[-3000:])
    assert p.returncode == 0 and "WORKER_OK" in p.stdout, p.stdout[-4000:]
    with np.load(out) as z:
        _RESULTS[name] = {k: z[k] for k in z.files}
    return _RESULTS[name]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("stack_spill")


@pytest.fixture(scope="module", autouse=True)
def stack3_lib():
    """the 3-entry library, built on the host if it is missing (a minute of hipcc; no GPU involved), before the module's first GPU process"""
    if not os.path.exists(W.STACK3_LIB):
        if _DEAD:
            pytest.fail("no further GPU process is started: " + _DEAD[0])
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "mitsuba3_amd", "csrc"), "OUT=../libhip_ad_rgb_stack3.so", "OBJDIR=obj_stack3", "EXTRA=-DHAR_LDS_STACK_SMALL=3", "-j16"],
                              stdout=subprocess.DEVNULL)
    return W.STACK3_LIB


# ------------------------------------------------------------------ the oracle's side, computed once per key

_REF = {}


def _memo(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _oracle(mi, O, d, hide=False):
    scene = mi.load_dict(d)
    osc, sensor = O.scene_from_product(scene)
    if hide:
        osc.set_hide_emitters(True)
    return scene, osc, sensor


def _ref_render(mi, O, key, d, spp, seed, prb=False, hide=False, per_pass=None):
    def run():
        _, osc, sensor = _oracle(mi, O, d, hide)
        if per_pass:
            img, st = osc.render_path_passes(sensor, seed=seed, spp=spp, spp_per_pass=per_pass, max_depth=MD, rr_depth=RR)
        else:
            img, st = (osc.render_prb if prb else osc.render_path)(sensor, seed=seed, spp=spp, max_depth=MD, rr_depth=RR)
        return img, np.array([st.paths, st.vertices], np.int64)
    return _memo(("render", key), run)


def _check_render(R, mi, O, key, d, spp, seed, ref_key=None, **kw):
    ref, st = _ref_render(mi, O, ref_key or key, d, spp, seed, **kw)
    e = rel_l2(R["img." + key], ref)
    print("render", key, "rel_l2", e, "stats", R["stats." + key], st)
    assert np.isfinite(R["img." + key]).all() and e < 1e-4, (key, e)
    assert np.array_equal(R["stats." + key], st), (key, R["stats." + key], st)


def _ref_backward(mi, O, key, d, res, spp, seed):
    def run():
        scene, osc, sensor = _oracle(mi, O, d)
        g_refl, g_tex, _ = osc.render_prb_backward(sensor, W.grad_image(res), seed=seed, spp=spp, max_depth=MD, rr_depth=RR)
        return {k: (g_tex[b.tex_index] if kind == "tex" else g_refl[b.index]) for k, (kind, b) in scene._param_keys().items() if kind != "emit"}
    return _memo(("backward", key), run)


def _check_backward(R, mi, O, key, d, res, spp, seed, ref_key=None):
    want = _ref_backward(mi, O, ref_key or key, d, res, spp, seed)
    live = 0
    for k, ref in want.items():
        got = R["grad.%s.%s" % (key, k)]
        if not ref.any():
            assert not got.any(), k
            continue
        e = rel_l2(got.reshape(ref.shape), ref); live += 1
        print("backward", key, k, "rel_l2", e)
        assert e < 1e-3, (key, k, e)
    assert live >= 1


def _check_sample(R, mi, O, key, d, rays, prb):
    """the assertions of tests/test_gpu_boundary.py::test_integrator_sample_vs_oracle: mask and (path) sampler state lane by lane, radiance to 1e-4.  Returns the
    number of lanes whose radiance differs from the oracle's in any bit."""
    def run():
        _, osc, _ = _oracle(mi, O, d)
        return osc.integrator_sample(*rays, seed=5 + 3, max_depth=MD, rr_depth=RR, prb=prb)
    ref, rvalid, rstate = _memo(("sample", key), run)
    spec = R["sample.%s.spec" % key]
    diff = int((spec.view(np.uint32) != ref.view(np.uint32)).any(0).sum())
    print("sample", key, "lanes that differ from the oracle in any bit:", diff, "of", spec.shape[1], "rel_l2", rel_l2(spec, ref))
    assert np.array_equal(R["sample.%s.valid" % key], rvalid), key
    assert ref.max() > 0 and rel_l2(spec, ref) < 1e-4, key
    if not prb:
        assert np.array_equal(R["sample.%s.state" % key], rstate), key
    return diff


def _check_queries(R, mi, O, key, d, rays):
    def run():
        _, osc, _ = _oracle(mi, O, d)
        o, dd, maxt, maxt2 = rays
        return osc.ray_intersect(o, dd, maxt, naive=True), osc.ray_test(o, dd, maxt2)
    ref, occluded = _memo(("queries", key), run)
    hit = np.isfinite(ref[0])
    assert 0.05 < hit.mean() < 0.999, hit.mean()
    for naive in (0, 1):
        assert np.array_equal(R["rq.%s.%d.t" % (key, naive)].view(np.uint32), ref[0].view(np.uint32)), (key, naive)
        for f, r in zip("uvpsi", ref[1:]):
            assert np.array_equal(R["rq.%s.%d.%s" % (key, naive, f)][hit].view(np.uint32), np.asarray(r)[hit].view(np.uint32)), (key, naive, f)
        assert np.array_equal(R["rq.%s.%d.occluded" % (key, naive)], occluded), (key, naive)


# ------------------------------------------------------------------ A: the spill kernels on scenes that fit

@pytest.mark.parametrize("name,kind", W.WAVE_PAIRS)
def test_spill_renders_against_oracle(mi, O, tmp, name, kind):
    """k_trace_closest<true, false, false> and k_resolve<MODE_PATH | MODE_PRB_PRIMAL, true> on the Cornell box, the all-materials box and an instanced scene with
    top-level geometry: film and path / vertex counts"""
    R = _child("spill", tmp)
    _check_render(R, mi, O, "%s.%s" % (name, kind), W.scene_dict(mi, name, kind), 8, 3, prb=kind == "prb")


def test_spill_packet_list_hide_emitters_chunks_passes(mi, O, tmp):
    """64 spp on a 16-px film: the camera rays take the packet kernel and what it hands over takes k_trace_closest<true, false, true>; hide_emitters: skip_area_emitters
    with a spill pointer; four chunks; four passes"""
    R = _child("spill", tmp)
    _check_render(R, mi, O, "packet", W.scene_dict(mi, "cornell", res=16), 64, 2)
    _check_render(R, mi, O, "hide", W.scene_dict(mi, "hide"), 8, 5, hide=True)
    _check_render(R, mi, O, "chunks", W.scene_dict(mi, "cornell"), 8, 3, ref_key="cornell.path")
    _check_render(R, mi, O, "passes", W.scene_dict(mi, "cornell"), 8, 3, per_pass=2)


def test_spill_backward_and_forward_mode(mi, O, tmp):
    """texel and albedo gradients of the textured Cornell box with the replay cache and without it (the adjoint through k_resolve<MODE_PRB_ADJOINT, true>); the forward-mode
    resolve flavour"""
    R = _child("spill", tmp)
    d = W.scene_dict(mi, "textured", "prb")
    _check_backward(R, mi, O, "textured", d, 32, 8, 11)
    _check_backward(R, mi, O, "textured_nocache", d, 32, 8, 11, ref_key="textured")
    scene, osc, sensor = _oracle(mi, O, d)
    _, t_refl, t_tex, t_emit = W.forward_tangents(scene)
    ref = _memo(("forward",), lambda: osc.render_prb_forward(sensor, t_refl, t_tex, t_emit, seed=6, spp=8, max_depth=MD, rr_depth=RR))
    e = rel_l2(R["img.forward"], ref)
    print("forward mode rel_l2", e)
    assert e < 1e-3


def test_spill_vertex_position_gradients(mi, O, tmp):
    """`slab` of test_prb_vertex_position_gradients, at its bound (2e-3 of the largest component per mesh; colours 1e-3)"""
    from tests.test_shape_gradients_cpu import mesh_index
    R = _child("spill", tmp)
    names = ["floor", "ceiling"]

    def run():
        scene, osc, sensor = _oracle(mi, O, W.scene_dict(mi, "slab", "prb", res=24))
        ids = [mesh_index(scene, n) for n in names]
        want, w_refl, w_tex, _ = osc.render_prb_backward_shape(sensor, W.grad_image(24), ids, seed=3, spp=16, max_depth=MD, rr_depth=RR)
        colours = {k: (w_tex[b.tex_index] if kind == "tex" else w_refl[b.index]) for k, (kind, b) in scene._param_keys().items() if kind != "emit"}
        return {n: want[m] for n, m in zip(names, ids)}, colours
    want, colours = _memo(("slab",), run)
    for n in names:
        got = R["grad.slab.%s.positions" % n].reshape(-1, 3); scale = np.abs(want[n]).max()
        print("slab", n, np.abs(got - want[n]).max() / scale)
        assert scale > 0 and np.abs(got - want[n]).max() < 2e-3 * scale, n
    for k, ref in colours.items():
        if ref.any():
            assert rel_l2(R["grad.slab." + k].reshape(ref.shape), ref) < 1e-3, k


SAMPLE_PAIRS = [(n, k) for n in ("cornell", "instanced_top") for k in ("path", "prb")]


@pytest.mark.parametrize("name,kind", SAMPLE_PAIRS)
def test_spill_integrator_sample(mi, O, tmp, name, kind):
    R = _child("spill", tmp)
    _check_sample(R, mi, O, "%s.%s" % (name, kind), W.scene_dict(mi, name, kind), W.sample_rays(name), kind == "prb")


def test_spill_sample_radiance_bit_equal_to_oracle(mi, O, tmp):
    """Integrator.sample's per-lane radiance is the oracle's bit for bit, `path` and `prb`.  This test found a difference that had nothing to do with the spill
    family: 1113 (cornell) and 2729 (instanced_top) of 7643 `path` lanes were off in the last bit (rel L2 3.5e-9, 3.4e-8), `prb` lanes none, with and without
    HAR_FORCE_STACK_SPILL alike.  path.cpp adds the emitter-sampling term with ONE rounding, `result = fmadd(throughput, bsdf_val * em_weight * mis_em, result)`;
    the wavefront stored the rounded product in the shadow-ray item and k_resolve added it.  On caller-supplied rays the item now carries the second factor and
    k_resolve fuses it with the throughput it reads back from the bounce's input wavefront (HAR_SHADE_FUSED_NEE)."""
    R = _child("spill", tmp)
    diff = {"%s.%s" % (n, k): _check_sample(R, mi, O, "%s.%s" % (n, k), W.scene_dict(mi, n, k), W.sample_rays(n), k == "prb") for n, k in SAMPLE_PAIRS}
    assert not any(diff.values()), diff


def test_spill_equals_lds_only(tmp):
    """the same process without the switch (the LDS-only kernels, the seeded closest-hit start on the instanced scene, the shadow-ray overlap): only where the stack
    lives differs -- per-lane outputs and counters bit for bit, films and gradients up to the order of the atomic sums"""
    A = _child("spill", tmp); B = _child("plain", tmp)
    assert sorted(A) == sorted(B)
    n = {"img": 0, "grad": 0, "stats": 0, "sample": 0}
    for k in sorted(A):
        fam = k.split(".")[0]; n[fam] += 1
        if fam in ("stats", "sample"):
            assert np.array_equal(A[k].view(np.uint8), B[k].view(np.uint8)), k
        elif B[k].any():
            e = rel_l2(A[k], B[k])
            print(k, e)
            assert e < (FILM_ORDER_TOL if fam == "img" else GRAD_ORDER_TOL), (k, e)
        else:
            assert not A[k].any(), k
    assert n["img"] >= 11 and n["sample"] >= 12 and n["stats"] >= 10 and n["grad"] >= 6, n


# ------------------------------------------------------------------ B: entries in HBM (the 3-entry library)

@pytest.mark.parametrize("name", ["comb", "instanced_soup"])
def test_stack3_path_backward_sample_queries(mi, O, tmp, stack3_lib, name):
    """the scenes tests/test_deep_bvh_cpu.py qualified (rays reach level >= 5: two or more entries of a ray's stack in the HBM columns): `path` film and counters, `prb`
    reflectance gradient, Integrator.sample, and 2 x 10^5 closest-hit / any-hit queries -- the ray-query kernels keep their 30 LDS entries in every build and are the
    control here"""
    R = _child("stack3", tmp)
    assert 3 < int(R["depth." + name]) <= D.STACK3_CAP
    _check_render(R, mi, O, name, W.scene_dict(mi, name), 8, 3)
    _check_backward(R, mi, O, name, W.scene_dict(mi, name, "prb"), 32, 8, 11)
    _check_sample(R, mi, O, name + ".path", W.scene_dict(mi, name), W.sample_rays(name), False)
    _check_queries(R, mi, O, name, W.scene_dict(mi, name), W.query_rays(name))


def test_stack3_sample_radiance_bit_equal_to_oracle(mi, O, tmp, stack3_lib):
    """the same with stack entries in the HBM columns (see test_spill_sample_radiance_bit_equal_to_oracle; before the fused add: comb 2 lanes, instanced_soup 5)"""
    R = _child("stack3", tmp)
    diff = {n: _check_sample(R, mi, O, n + ".path", W.scene_dict(mi, n), W.sample_rays(n), False) for n in ("comb", "instanced_soup")}
    assert not any(diff.values()), diff


def test_stack3_hide_emitters_and_packet_list(mi, O, tmp, stack3_lib):
    R = _child("stack3", tmp)
    _check_render(R, mi, O, "hide", W.scene_dict(mi, "instanced_soup_panel"), 8, 5, hide=True, ref_key="stack3.hide")
    _check_render(R, mi, O, "packet", W.scene_dict(mi, "comb", res=16), 64, 2, ref_key="stack3.packet")


def test_stack3_column_stride(mi, O, tmp, stack3_lib):
    """gridDim.x is the stride of the HBM columns: 32 blocks (8192 lanes) and HAR_TRACE_GRID=8 give the oracle's film and counters and each other's per-lane radiance"""
    A = _child("stack3", tmp); B = _child("grid8", tmp)
    d = W.scene_dict(mi, "instanced_soup")
    _check_render(A, mi, O, "instanced_soup", d, 8, 3)
    _check_render(B, mi, O, "instanced_soup", d, 8, 3)
    assert rel_l2(A["img.instanced_soup"], B["img.instanced_soup"]) < FILM_ORDER_TOL
    _check_sample(B, mi, O, "comb.path", W.scene_dict(mi, "comb"), W.sample_rays("comb"), False)
    assert A["sample.comb.path.spec"].max() > 0
    for f in ("spec", "valid", "state"):
        assert np.array_equal(A["sample.comb.path." + f].view(np.uint8), B["sample.comb.path." + f].view(np.uint8)), f


def test_stack3_cap(tmp, stack3_lib):
    """3 + 20 entries: a scene that needs 23 loads, one that needs 24 is refused with both numbers"""
    R = _child("stack3", tmp)
    assert int(R["cap.n23"]) > 0 and int(R["cap.n24"]) > 0
    assert int(R["cap.depth23"]) == 23 and "cap.error23" not in R
    assert "cap.depth24" not in R
    msg = str(R["cap.error24"])
    assert "needs 24 " in msg and "hold 23 " in msg, msg


def test_stack3_two_streams(mi, O, tmp, stack3_lib):
    """HAR_STREAMS=2, 2^20 lanes: the two halves run concurrently, each on an integrator of its own (dual_split: `I->twin = new HarIntegratorImpl()`, whose
    ensure_workspace allocates its own stack_spill) -- the columns are not shared, and the film is the oracle's"""
    R = _child("stack3", tmp)
    _check_render(R, mi, O, "two_streams", W.scene_dict(mi, "instanced_soup", res=256), 16, 7)


# ------------------------------------------------------------------ C: deep scenes, default library

@pytest.mark.parametrize("name", sorted(D.DEEP))
def test_deep_scene(mi, O, tmp, name):
    """depth-first bound 14 .. 30: the ray queries (30 LDS entries), `path` (HybridStack), `aov` (k_aov_trace<30>) and a `prb` backward of the mesh's reflectance"""
    from tests import aov_cases as A
    R = _child("deep", tmp)
    L = D.harness()
    scene = mi.load_dict(W.scene_dict(mi, name))
    h = D.harness_scene(L, scene); need = D.stack_need(L, h); L.hh_scene_destroy(h)
    assert int(R["depth." + name]) == need and D.STACK_LDS < need <= D.STACK_CAP
    _check_queries(R, mi, O, name, W.scene_dict(mi, name), W.query_rays(name))
    _check_render(R, mi, O, name, W.scene_dict(mi, name), 8, 3)
    _check_backward(R, mi, O, name, W.scene_dict(mi, name, "prb"), 32, 8, 11)
    osc, sensor = O.scene_from_product(scene)
    want, _ = A.oracle_aov_film(O, scene, osc, sensor, "box", W.AOV_TYPES, 5, 8)
    got = R["aov." + name]
    sl, count = A.channel_slices(W.AOV_TYPES)
    assert got.shape == want.shape
    assert A.rel_l2(got[:, :, count], O.render_weights(sensor, 5, 8)[:, :, 3]) < 2e-6
    for t in W.AOV_TYPES:
        e = A.rel_l2(got[:, :, sl[t]], want[:, :, sl[t]])
        print("aov", name, t, e)
        assert e <= 1e-4, (t, e)


def test_over_deep_scene_is_refused(mi, O, tmp):
    R = _child("deep", tmp)
    msg = str(R["overdeep.error"])
    L = D.harness()
    h = D.harness_scene(L, mi.load_dict(D.OVER_DEEP(mi))); need = D.stack_need(L, h); L.hh_scene_destroy(h)
    assert need > D.STACK_CAP
    assert "needs %d " % need in msg and "hold %d " % D.STACK_CAP in msg, msg
    _check_render(R, mi, O, "after_refusal", W.scene_dict(mi, "cornell"), 8, 3, ref_key="cornell.path")


def test_vertex_update_past_the_cap_is_refused(tmp):
    """stack_fits (har_scene_api.hip): the update is refused with both numbers, and the scene renders what it held before, bit for bit"""
    R = _child("deep", tmp)
    assert int(R["depth.update_before"]) == D.STACK_CAP
    msg = str(R["update.error"])
    assert "needs %d " % (D.STACK_CAP + 1) in msg and "hold %d" % D.STACK_CAP in msg, msg
    assert int(R["depth.update_after"]) == D.STACK_CAP
    assert R["img.update_before"].any() and np.array_equal(R["img.update_before"].view(np.uint32), R["img.update_after"].view(np.uint32))
