"""Seeded closest-hit start (Accel::top_seed; har_accel.h: top_seed_hit + Traversal::begin_seeded) on the host: the brute-force seed over the top-level
triangles followed by the TLAS walk must give accel_trace_naive's hit record bit for bit.  The library under test is built here, into a temporary
directory, from tests/top_seed/top_seed_lib.cpp and the product's host sources."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import top_seed_cases as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitsuba3_amd", "csrc")
CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2", "-Wall", "-Wno-unused-parameter"]     # those of the host harness
NONE = 0xffffffff


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("top_seed")
    srcs = [os.path.join(ROOT, "tests", "top_seed", "top_seed_lib.cpp"), os.path.join(CSRC, "har_scene_host.cpp"), os.path.join(CSRC, "har_accel_build.cpp")]
    objs = [str(out / (os.path.basename(s) + ".o")) for s in srcs]
    jobs = [subprocess.Popen(["g++"] + CXXFLAGS + ["-c", "-o", o, s]) for s, o in zip(srcs, objs)]       # three compilers side by side: a few seconds
    assert all(j.wait() == 0 for j in jobs)
    so = str(out / "libtop_seed.so")
    subprocess.check_call(["g++", "-shared", "-o", so] + objs)
    L = C.CDLL(so)
    L.ts_scene_create.restype = C.c_void_p; L.ts_scene_create.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.ts_scene_destroy.argtypes = [C.c_void_p]; L.ts_scene_info.argtypes = [C.c_void_p, C.c_void_p]
    L.ts_trace.argtypes = [C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 9
    return L


@pytest.fixture(scope="module")
def ray_set():
    return TS.rays()


class HostScene:
    def __init__(self, L, mi, n_top, env=None, **kw):
        old = os.environ.pop("HAR_TOP_SEED", None)
        if env is not None:
            os.environ["HAR_TOP_SEED"] = env
        try:
            self.scene = mi.load_dict(TS.scene_dict(mi, n_top, **kw))
            desc = self.scene.desc(); err = C.create_string_buffer(256)
            self.L = L; self.h = C.c_void_p(L.ts_scene_create(C.byref(desc), err, 256)); assert self.h, err.value
        finally:
            os.environ.pop("HAR_TOP_SEED", None)
            if old is not None:
                os.environ["HAR_TOP_SEED"] = old
        info = (C.c_uint32 * 6)(); L.ts_scene_info(self.h, info)
        self.has_tlas, self.top_count, self.top_seed, self.eligible, self.seed_max, self.default = [int(x) for x in info]

    def trace(self, mode, o, d, maxt):
        n = o.shape[1]
        out = [np.zeros(n, np.float32) for _ in range(3)] + [np.zeros(n, np.uint32) for _ in range(3)]
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        st = self.L.ts_trace(self.h, mode, n, p(o), p(d), p(maxt), *[p(a) for a in out])
        return st, out

    def close(self):
        self.L.ts_scene_destroy(self.h)


def _mismatches(a, b):
    """rays whose records differ in any bit of t, u, v, prim, shape, inst"""
    bad = np.zeros(a[0].shape[0], bool)
    for x, y in zip(a, b):
        bad |= x.view(np.uint32) != y.view(np.uint32)
    return int(bad.sum())


@pytest.mark.parametrize("n_top", [1, 12, 16, 17])
def test_seeded_traversal_equals_brute_force(lib, mi, ray_set, n_top):
    o, d, maxt = ray_set
    assert 18000 <= o.shape[1] <= 26000
    S = HostScene(lib, mi, n_top)
    try:
        assert S.has_tlas == 1 and S.top_count == n_top and S.seed_max == 16
        # the automatic choice: 1 .. 16 top-level triangles are eligible, 17 are not and keep today's path
        assert S.eligible == (1 if n_top <= 16 else 0)
        assert S.top_seed == (S.default if S.eligible else 0)
        st0, ref = S.trace(0, o, d, maxt)
        st1, seeded = S.trace(1, o, d, maxt)
        st2, plain = S.trace(2, o, d, maxt)
        assert st0 == 0 and st1 == 0 and st2 == 0
        assert _mismatches(seeded, ref) == 0
        assert _mismatches(plain, ref) == 0
        t, inst = ref[0], ref[5]
        hit = np.isfinite(t)
        assert hit.sum() > (0.5 if n_top >= 12 else 0.25) * t.size and (~hit).sum() >= 800                     # the set has both, and rays that miss everything
        if n_top >= 12:
            assert ((inst != NONE) & hit).sum() > 1000 and ((inst == NONE) & hit).sum() > 5000
            assert (np.signbit(t) & (t == 0)).sum() > 0                                # t = -0 is among the results
        if n_top >= 16:
            # the coplanar pair: the seed alone finds the top-level triangle at exactly the t at which the instance triangle is met, and the instance wins
            _, seed = S.trace(3, o, d, maxt)
            tie = np.isfinite(seed[0]) & (seed[0].view(np.uint32) == t.view(np.uint32)) & (inst != NONE)
            assert tie.sum() >= 100
    finally:
        S.close()


def test_scene_without_top_level_geometry(lib, mi, ray_set):
    o, d, maxt = ray_set
    S = HostScene(lib, mi, 0)
    try:
        assert S.has_tlas == 1 and S.top_count == 0 and S.eligible == 0 and S.top_seed == 0
        assert S.trace(1, o[:, :8], d[:, :8], maxt[:8])[0] == -1                       # nothing to seed with
        st0, ref = S.trace(0, o, d, maxt)
        st2, plain = S.trace(2, o, d, maxt)
        assert st0 == 0 and st2 == 0 and _mismatches(plain, ref) == 0
    finally:
        S.close()


def test_switches(lib, mi):
    """HAR_TOP_SEED is read at every build (one process holds both kinds); 0 / 1 force the flag off / on; a flat scene never takes the path"""
    on = HostScene(lib, mi, 12, env="1"); off = HostScene(lib, mi, 12, env="0"); big = HostScene(lib, mi, 17, env="1"); none = HostScene(lib, mi, 0, env="1")
    flat = HostScene(lib, mi, 12, env="1", instances=False)
    try:
        assert on.top_seed == 1 and off.top_seed == 0 and big.top_seed == 1 and none.top_seed == 0
        assert flat.has_tlas == 0 and flat.top_seed == 0
    finally:
        for s in (on, off, big, none, flat):
            s.close()
    with pytest.raises(Exception):
        mi.load_dict({"type": "path", "top_seeds": True})
    assert mi.load_dict({"type": "path", "top_seed": True}).top_seed is True and mi.load_dict({"type": "prb"}).top_seed is None
