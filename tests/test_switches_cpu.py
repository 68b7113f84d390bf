"""The switch table (har_switches.h: parse_switches) and the per-chunk plan (har_plan.h: plan_chunk) on the host.  The library under test is built here, into a
temporary directory, from tests/switches/switches_lib.cpp and the two HIP-free headers.  Every expected value below is written out from the expressions the
render driver used before the table and the plan existed (one `static const ... getenv(...)` per use; the conditions between the launches of run_chunk)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ["debug_guard", "debug_sync", "texel_queues", "tq_lds", "tq_bpq", "overlap", "force_stack_spill", "first_vertex", "material_queues", "sort_window", "trace_grid",
          "adjoint_inline", "late_overlap", "packet", "packet_budget", "refit_max_inflation", "refit_max_steps", "host_tlas_update", "streams", "dual_frac", "dual_stagger",
          "prb_tape", "verbose"]
# docs/switches.md: the defaults
DEFAULTS = dict(debug_guard=0, debug_sync=0, texel_queues=1, tq_lds=0, tq_bpq=0, overlap=-1, force_stack_spill=0, first_vertex=1, material_queues=-1, sort_window=8,
                trace_grid=0, adjoint_inline=1, late_overlap=-2, packet=-1, packet_budget=160, refit_max_inflation=1.5, refit_max_steps=0, host_tlas_update=0, streams=0,
                dual_frac=50, dual_stagger=0, prb_tape=2, verbose=0)
# variable -> (field, [(text, value)]): the neutral value, each forcing value, the clamp edges
CASES = {
    "HAR_DEBUG_GUARD": ("debug_guard", [("0", 0), ("1", 1), ("2", 2)]),
    "HAR_DEBUG_SYNC": ("debug_sync", [("0", 1), ("1", 1)]),                                    # presence only
    "HAR_TEXEL_QUEUES": ("texel_queues", [("0", 0), ("1", 1), ("2", 1)]),
    "HAR_TQ_LDS": ("tq_lds", [("0", 0), ("24576", 24576), ("65536", 65536)]),
    "HAR_TQ_BPQ": ("tq_bpq", [("0", 0), ("1", 1), ("4", 4)]),
    "HAR_OVERLAP": ("overlap", [("-1", -1), ("0", 0), ("1", 1)]),
    "HAR_FORCE_STACK_SPILL": ("force_stack_spill", [("0", 1), ("1", 1)]),                      # presence only
    "HAR_FIRST_VERTEX": ("first_vertex", [("0", 0), ("1", 1)]),
    "HAR_MATERIAL_QUEUES": ("material_queues", [("-1", -1), ("0", 0), ("1", 1)]),
    "HAR_SORT_WINDOW": ("sort_window", [("-3", 1), ("0", 1), ("1", 1), ("8", 8)]),            # max(1, .)
    "HAR_TRACE_GRID": ("trace_grid", [("0", 8), ("1", 8), ("1279", 1272), ("1280", 1280), ("4096", 4096)]),      # a multiple of the 8 shards, at least 8
    "HAR_ADJOINT_INLINE": ("adjoint_inline", [("0", 0), ("1", 1)]),
    "HAR_LATE_OVERLAP": ("late_overlap", [("-1", -1), ("0", 0), ("3", 3)]),
    "HAR_PACKET": ("packet", [("-1", -1), ("0", 0), ("1", 1)]),
    "HAR_PACKET_BUDGET": ("packet_budget", [("0", 0), ("64", 64), ("160", 160)]),
    "HAR_REFIT_MAX_INFLATION": ("refit_max_inflation", [("1.5", 1.5), ("2.25", 2.25), ("0", 0.0)]),
    "HAR_REFIT_MAX_STEPS": ("refit_max_steps", [("0", 0), ("7", 7)]),
    "HAR_HOST_TLAS_UPDATE": ("host_tlas_update", [("0", 1), ("1", 1)]),                        # presence only
    "HAR_STREAMS": ("streams", [("0", 0), ("1", 1), ("2", 2)]),
    "HAR_DUAL_FRAC": ("dual_frac", [("5", 10), ("10", 10), ("50", 50), ("90", 90), ("95", 90)]),      # clamped to 10..90
    "HAR_DUAL_STAGGER": ("dual_stagger", [("0", 0), ("1", 1)]),
    "HAR_PRB_TAPE": ("prb_tape", [("0", 0), ("1", 1), ("2", 2)]),
    "HAR_VERBOSE": ("verbose", [("0", 1), ("1", 1)]),                                          # presence only
}

PLAN_OUT = ["mq_on", "first_regen", "use_mq", "overlap", "late_on", "late_from", "inline_commit", "spill", "shape", "fwd", "packet", "alpha_flags", "grid", "tgrid", "shade_flags"]
PATH, PRIMAL, ADJOINT = 0, 1, 2                                                                # MODE_* of har_path.h
CACHE_WRITE, CACHE_READ, TAPE_WRITE, TAPE_READ, RECORD_WRITE, RECORD_READ = 1, 2, 3, 4, 5, 6   # ReplayCache::mode
ENVMAP, TEXLIGHT = 0x100, 0x400                                                                # HAR_SCENE_* of har_bsdf.h
EMITTER_GRADS, HIDE_EMITTERS, FORWARD_MODE, EXTRA_GRADS, LIGHT_TEXELS = 1, 2, 4, 16, 64       # HAR_SHADE_* of har_path.h


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("switches") / "libswitches.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-parameter", "-shared", "-o", so, os.path.join(ROOT, "tests", "switches", "switches_lib.cpp")])
    L = C.CDLL(so)
    L.sw_name.restype = C.c_char_p
    return L


def _env(env):
    n = len(env)
    names = (C.c_char_p * max(n, 1))(*[k.encode() for k in env]); values = (C.c_char_p * max(n, 1))(*[v.encode() for v in env.values()])
    return names, values, n


def parse(L, env):
    out = (C.c_double * len(FIELDS))()
    L.sw_parse(*_env(env), out)
    return dict(zip(FIELDS, out))


def plan(L, env=None, mode=PATH, cache_mode=0, n=2048, spp=4, lane_base=0, nb=8, rays=0, valid_lane=0, pass_rng=0, projection=0, forward_mode=0, shape_on=0, adjoint_image=0,
         alpha_lane=0, max_depth=8, rr_depth=5, hide_emitters=0, material_queues=0, packet_tracing=-1, grad_emitters=0, grad_bsdf_params=0, grad_light_texels=0, alpha_film=0,
         batch_n=0, stack_need=10, lds_stack=13, mat_classes=1, bsdf_types=0, env_emitter=-1):
    ll = lambda *v: (C.c_longlong * len(v))(*v)
    out = (C.c_longlong * len(PLAN_OUT))()
    L.sw_plan(*_env(env or {}), ll(max_depth, rr_depth, hide_emitters, material_queues, packet_tracing, grad_emitters, grad_bsdf_params, grad_light_texels, alpha_film, batch_n),
              ll(stack_need, lds_stack, mat_classes, bsdf_types, env_emitter),
              ll(mode, cache_mode, n, spp, lane_base, nb, rays, valid_lane, pass_rng, projection, forward_mode, shape_on, adjoint_image, alpha_lane), out)
    return dict(zip(PLAN_OUT, out))


def test_defaults(lib):
    assert parse(lib, {}) == DEFAULTS


def test_table_is_complete(lib):
    names = [lib.sw_name(k).decode() for k in range(lib.sw_name_count())]
    assert sorted(names) == sorted(CASES) and len(FIELDS) == len(CASES)
    assert "HAR_TOP_SEED" not in names            # read per integrator / per scene, never cached


@pytest.mark.parametrize("name", sorted(CASES))
def test_parsing(lib, name):
    field, cases = CASES[name]
    for text, value in cases:
        expected = dict(DEFAULTS); expected[field] = value
        assert parse(lib, {name: text}) == expected, (name, text)


def test_documentation(lib):
    doc = open(os.path.join(ROOT, "docs", "switches.md")).read()
    for k in range(lib.sw_name_count()):
        assert "`" + lib.sw_name(k).decode() in doc, lib.sw_name(k)


def test_plan_first_vertex(lib):
    assert plan(lib)["first_regen"] == 1                                     # `path`, forward, one pass, perspective
    for other in (dict(projection=2), dict(batch_n=2), dict(alpha_film=1, alpha_lane=1), dict(material_queues=1), dict(rays=1), dict(rays=1, valid_lane=1),
                  dict(env={"HAR_FIRST_VERTEX": "0"}), dict(env={"HAR_MATERIAL_QUEUES": "1"}), dict(cache_mode=CACHE_WRITE), dict(mode=ADJOINT, cache_mode=RECORD_READ)):
        assert plan(lib, **other)["first_regen"] == 0, other
    assert plan(lib, alpha_film=1, alpha_lane=0)["first_regen"] == 1        # an alpha film whose lanes are not allocated is not read
    assert plan(lib, material_queues=1, env={"HAR_MATERIAL_QUEUES": "0"})["first_regen"] == 1
    # the passes of a multi-pass `path` render resume their samplers in both kernels and keep the first-vertex flavour; the recording pass of `prb` does not
    assert plan(lib, pass_rng=1)["first_regen"] == 1
    rec = dict(mode=PRIMAL, cache_mode=RECORD_WRITE, adjoint_image=1)
    assert plan(lib, **rec)["first_regen"] == 1
    for other in (dict(pass_rng=1), dict(forward_mode=1), dict(adjoint_image=0), dict(cache_mode=TAPE_WRITE), dict(cache_mode=CACHE_WRITE)):
        assert plan(lib, **{**rec, **other})["first_regen"] == 0, other


def test_plan_adjoint_commit(lib):
    adj = dict(mode=ADJOINT, cache_mode=CACHE_READ)
    p = plan(lib, **adj); assert (p["inline_commit"], p["shape"], p["fwd"]) == (1, 0, 0)
    p = plan(lib, shape_on=1, **adj); assert (p["inline_commit"], p["shape"], p["fwd"]) == (0, 1, 0)
    p = plan(lib, forward_mode=1, **adj); assert (p["inline_commit"], p["shape"], p["fwd"]) == (0, 0, 1)
    assert plan(lib, env={"HAR_ADJOINT_INLINE": "0"}, **adj)["inline_commit"] == 0
    p = plan(lib, mode=PRIMAL, cache_mode=CACHE_WRITE, shape_on=1, forward_mode=1); assert (p["inline_commit"], p["shape"], p["fwd"]) == (0, 0, 0)


def test_plan_material_queues(lib):
    two = dict(material_queues=1, mat_classes=0b101)
    p = plan(lib, **two); assert (p["mq_on"], p["use_mq"]) == (1, 1)
    assert plan(lib, mode=PRIMAL, cache_mode=CACHE_WRITE, **two)["use_mq"] == 1
    for other in (dict(bsdf_types=ENVMAP), dict(mat_classes=0b100), dict(mode=ADJOINT, cache_mode=CACHE_READ), dict(mode=PRIMAL, cache_mode=RECORD_WRITE),
                  dict(material_queues=0), dict(env={"HAR_MATERIAL_QUEUES": "0"})):
        assert plan(lib, **{**two, **other})["use_mq"] == 0, other
    p = plan(lib, mat_classes=0b11, env={"HAR_MATERIAL_QUEUES": "1"}); assert (p["mq_on"], p["use_mq"]) == (1, 1)
    p = plan(lib, mat_classes=0b11, bsdf_types=TEXLIGHT, env={"HAR_MATERIAL_QUEUES": "-1"}, material_queues=1); assert (p["mq_on"], p["use_mq"]) == (1, 1)


def test_plan_overlap(lib):
    big = 1 << 25
    p = plan(lib, n=big); assert (p["overlap"], p["late_on"], p["spill"]) == (1, 0, 0)
    assert plan(lib, n=big + 2048)["overlap"] == 0
    for other in (dict(hide_emitters=1), dict(stack_need=14), dict(rays=1), dict(mode=ADJOINT, cache_mode=CACHE_READ), dict(env={"HAR_OVERLAP": "0"}),
                  dict(env={"HAR_FORCE_STACK_SPILL": "1"})):
        assert plan(lib, n=big, **other)["overlap"] == 0, other
    assert plan(lib, n=big, stack_need=13)["spill"] == 0 and plan(lib, n=big, stack_need=14)["spill"] == 1 and plan(lib, env={"HAR_FORCE_STACK_SPILL": "0"})["spill"] == 1
    assert plan(lib, n=big + 2048, env={"HAR_OVERLAP": "1"})["overlap"] == 1
    assert plan(lib, n=big + 2048, env={"HAR_OVERLAP": "1"}, hide_emitters=1)["overlap"] == 0
    assert plan(lib, n=big, mode=PRIMAL, cache_mode=RECORD_WRITE)["overlap"] == 1
    # late overlap: only where the full overlap is off for the job's size alone; default off
    assert plan(lib, n=big + 2048)["late_from"] == 0xffffffff
    p = plan(lib, n=big + 2048, env={"HAR_LATE_OVERLAP": "2"}); assert (p["overlap"], p["late_on"], p["late_from"]) == (0, 1, 2)
    for other in (dict(nb=2), dict(n=big), dict(hide_emitters=1), dict(stack_need=14), dict(rays=1), dict(mode=ADJOINT, cache_mode=CACHE_READ)):
        assert plan(lib, **{**dict(n=big + 2048, env={"HAR_LATE_OVERLAP": "2"}), **other})["late_on"] == 0, other
    assert plan(lib, n=big + 2048, env={"HAR_LATE_OVERLAP": "-1"})["late_on"] == 0
    assert plan(lib, n=big + 2048, env={"HAR_LATE_OVERLAP": "2", "HAR_OVERLAP": "0"})["late_on"] == 0      # overlap_applies(n = 0) is the switch then


def test_plan_packet(lib):
    assert plan(lib, spp=64, lane_base=0)["packet"] == 1 and plan(lib, spp=63, lane_base=0)["packet"] == 0
    assert plan(lib, spp=64, lane_base=32)["packet"] == 0 and plan(lib, spp=63, lane_base=32)["packet"] == 0
    assert plan(lib, spp=128, lane_base=64)["packet"] == 1 and plan(lib, spp=32)["packet"] == 0 and plan(lib, spp=96)["packet"] == 0
    assert plan(lib, spp=64, rays=1)["packet"] == 0
    assert plan(lib, spp=4, packet_tracing=1)["packet"] == 1 and plan(lib, spp=64, packet_tracing=0)["packet"] == 0
    assert plan(lib, spp=64, env={"HAR_PACKET": "0"})["packet"] == 0 and plan(lib, spp=4, packet_tracing=0, env={"HAR_PACKET": "1"})["packet"] == 1
    assert plan(lib, spp=64, packet_tracing=1, mode=ADJOINT, cache_mode=TAPE_READ)["packet"] == 0       # the replay of the state tape traces nothing at bounce 0


def test_plan_grids(lib):
    for n, grid, tgrid in ((1, 8, 8), (2048, 8, 8), (2049, 16, 16), (1 << 19, 2048, 2048), (1 << 22, 4096, 2048)):
        p = plan(lib, n=n); assert (p["grid"], p["tgrid"]) == (grid, tgrid), n
    p = plan(lib, n=1 << 22, env={"HAR_TRACE_GRID": "1280"}); assert (p["grid"], p["tgrid"]) == (4096, 1280)
    p = plan(lib, n=1 << 22, env={"HAR_TRACE_GRID": "4096"}); assert (p["grid"], p["tgrid"]) == (4096, 2048)
    p = plan(lib, n=2048, env={"HAR_TRACE_GRID": "1280"}); assert (p["grid"], p["tgrid"]) == (8, 8)


def test_plan_shade_flags(lib):
    assert plan(lib)["shade_flags"] == 0 and plan(lib, hide_emitters=1)["shade_flags"] == HIDE_EMITTERS
    assert plan(lib, grad_emitters=1, grad_bsdf_params=1, grad_light_texels=1, bsdf_types=TEXLIGHT)["shade_flags"] == 0                  # `path` differentiates nothing
    both = dict(grad_emitters=1, grad_bsdf_params=1, grad_light_texels=1, bsdf_types=TEXLIGHT)
    assert plan(lib, mode=PRIMAL, cache_mode=CACHE_WRITE, **both)["shade_flags"] == EMITTER_GRADS | LIGHT_TEXELS
    assert plan(lib, mode=ADJOINT, cache_mode=CACHE_READ, **both)["shade_flags"] == EMITTER_GRADS | EXTRA_GRADS | LIGHT_TEXELS
    assert plan(lib, mode=ADJOINT, cache_mode=CACHE_READ, forward_mode=1, **both)["shade_flags"] == EMITTER_GRADS | FORWARD_MODE
    assert plan(lib, mode=ADJOINT, cache_mode=CACHE_READ, grad_light_texels=1)["shade_flags"] == 0                                        # no bitmap light in the scene
    # alpha / validity flags of the camera samples
    assert plan(lib, alpha_film=1, alpha_lane=1)["alpha_flags"] == 1 and plan(lib, rays=1, valid_lane=1)["alpha_flags"] == 1 and plan(lib, alpha_film=1)["alpha_flags"] == 0
    assert plan(lib, mode=ADJOINT, cache_mode=CACHE_READ, alpha_film=1, alpha_lane=1)["alpha_flags"] == 0
