#!/usr/bin/env python3
"""Host model of the seeded closest-hit launches (Accel::top_seed) against the parent's, no GPU: blocks and modelled VALU instructions per 64 closest-hit
rays of bounces >= 1 (tools/seed_model.cpp, built here into a temporary directory).  Block costs as in tools/trace_stats.py: node 250, triangle 60,
instance 100, 30 per step; the seeded prologue is priced at 45 instructions per top-level triangle and pass of 64 rays plus 40 for loading the rays and
storing the records.
Usage: python tools/seed_model.py [res] [spp] [refill] > profiles/r07_model_top_seed.txt"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mitsuba3_amd as mi                                     # noqa: E402

CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2", "-Wall", "-Wno-unused-parameter"]
TRI_TEST, HANDOVER = 45, 40


def build(tmp):
    csrc = os.path.join(ROOT, "mitsuba3_amd", "csrc")
    srcs = [os.path.join(ROOT, "tools", "seed_model.cpp"), os.path.join(csrc, "har_scene_host.cpp"), os.path.join(csrc, "har_accel_build.cpp")]
    objs = [os.path.join(tmp, os.path.basename(s) + ".o") for s in srcs]
    jobs = [subprocess.Popen(["g++"] + CXXFLAGS + ["-c", "-o", o, s]) for s, o in zip(srcs, objs)]
    assert all(j.wait() == 0 for j in jobs)
    so = os.path.join(tmp, "libseed_model.so")
    subprocess.check_call(["g++", "-shared", "-o", so] + objs)
    L = C.CDLL(so)
    L.sm_scene_create.restype = C.c_void_p; L.sm_scene_create.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.sm_top_count.argtypes = [C.c_void_p]; L.sm_scene_destroy.argtypes = [C.c_void_p]
    L.sm_model.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p]
    return L


def run(L, name, d, res, spp, refill):
    scene = mi.load_dict(d)
    desc = scene.desc(); err = C.create_string_buffer(256)
    h = C.c_void_p(L.sm_scene_create(C.byref(desc), err, 256)); assert h, err.value
    top = L.sm_top_count(h)
    out = np.zeros((2, 10), np.float64)
    bad = L.sm_model(h, C.byref(scene.sensors()[0].har), 0, spp, 8, 5, res * res * spp, 8, refill, out.ctypes.data)
    L.sm_scene_destroy(h)
    assert bad >= 0
    print("%s %dx%dx%d, %d top-level triangles, refill at %d idle lanes, closest-hit rays of bounces >= 1: %d; hit records that differ: %d" % (name, res, res, spp, top, refill, int(out[0, 0]), bad))
    print("  %-8s | per ray: %6s %6s %6s | per 64 rays: %6s %8s %8s %8s %9s | %s" % ("", "nodes", "tris", "insts", "steps", "nodeblk", "triblk", "instblk", "prologue", "modelled VALU instructions per 64 rays"))
    cost = []
    for k, kind in enumerate(("parent", "seeded")):
        q = out[k]; r = q[0]; g = r / 64
        c = (250 * q[2] + 60 * q[3] + 100 * q[4] + 30 * q[1] + q[6] * (TRI_TEST * top + HANDOVER)) / g
        cost.append(c)
        print("  %-8s | %15.2f %6.2f %6.2f | %19.1f %8.1f %8.1f %8.1f %9.2f | %.0f" % (kind, q[7] / r, q[8] / r, q[9] / r, q[1] / g, q[2] / g, q[3] / g, q[4] / g, q[6] / g, c))
    print("  seeded / parent: %.3f (%.1f %% fewer modelled instructions)" % (cost[1] / cost[0], 100 * (1 - cost[1] / cost[0])))
    return bad


def main():
    res = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    spp = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    refill = int(sys.argv[3]) if len(sys.argv) > 3 else 12
    mi.set_variant("hip_ad_rgb")
    os.environ.pop("HAR_TOP_SEED", None)
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        bad = run(L, "instanced1m", mi.instanced_spheres_scene(width=res, height=res, spp=spp), res, spp, refill)
        # the same scene with four more top-level triangles (two small plinths' tops on the floor): 16, the largest eligible count
        d = mi.instanced_spheres_scene(width=res, height=res, spp=spp)
        P = np.array([[-0.9, -0.97, 0.5], [-0.6, -0.97, 0.5], [-0.6, -0.97, 0.8], [-0.9, -0.97, 0.8], [0.6, -0.97, 0.5], [0.9, -0.97, 0.5], [0.9, -0.97, 0.8], [0.6, -0.97, 0.8]], np.float32)
        d["plinths"] = {"type": "mesh", "faces": np.array([[0, 2, 1], [0, 3, 2], [4, 6, 5], [4, 7, 6]], np.uint32), "positions": P, "bsdf": {"type": "ref", "id": "white"}}
        bad += run(L, "instanced1m + 4 top-level triangles", d, res, spp, refill)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
