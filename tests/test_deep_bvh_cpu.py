"""Preconditions of tests/test_gpu_stack_spill.py, on the host: the deep cases of tests/deep_cases.py really need more than the 13 LDS stack entries of the
wavefront kernels (and the over-deep one more than the 30 the kernels hold), the oracle's brute force agrees with the product's host traversal on
these geometries (scale ratios up to about 1e24 inside one mesh) before the GPU is compared with it, and the scenes rendered with the 3-entry
library send their rays past the LDS entries, so that those tests cannot pass without touching the HBM columns."""
import numpy as np
import pytest

from tests import deep_cases as D


@pytest.fixture(scope="module")
def L():
    return D.harness()


@pytest.mark.parametrize("name", sorted(D.DEEP))
def test_deep_cases_need_the_spill_family(mi, L, name):
    """bands, not values: the builder may change.  Measured: nest300 18, nest600 22, nest700 26, instanced_nest 25, comb 17"""
    need, _ = D.stack_levels(L, mi.load_dict(D.DEEP[name](mi, res=16, spp=1)))
    assert D.STACK_LDS + 1 <= need <= D.STACK_CAP, need


def test_over_deep_case_exceeds_every_kernel(mi, L):
    """measured: 31"""
    need, _ = D.stack_levels(L, mi.load_dict(D.OVER_DEEP(mi, res=16, spp=1)))
    assert need > D.STACK_CAP, need


@pytest.mark.parametrize("name", sorted(D.DEEP) + ["over_deep"] + ["spill3_" + k for k in sorted(D.SPILL3) if k not in D.DEEP])
def test_host_traversal_equals_oracle_brute_force(mi, O, L, name):
    """t, u, v, prim, shape, instance bit for bit on 2 x 10^4 rays (half aimed at the nest's centre / along the comb's axis): the product's brute force and the
    kernels' resumable traversal against the oracle's brute force"""
    make = D.OVER_DEEP if name == "over_deep" else D.SPILL3[name[7:]] if name.startswith("spill3_") else D.DEEP[name]
    scene = mi.load_dict(make(mi, res=16, spp=1))
    osc, _ = O.scene_from_product(scene)
    o, d, maxt = D.case_rays(name[7:] if name.startswith("spill3_") else name, 20000, seed=3)
    ref = osc.ray_intersect(o, d, maxt, naive=True)
    hit = np.isfinite(ref[0])
    assert 0.2 < hit.mean() < 0.999
    h = D.harness_scene(L, scene)
    try:
        for naive in (1, 2):
            got = D.host_trace(L, h, o, d, maxt, naive)
            assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
            for a, b in zip(got[1:], ref[1:]):
                assert np.array_equal(a[hit].view(np.uint32), np.asarray(b)[hit].view(np.uint32))
    finally:
        L.hh_scene_destroy(h)


@pytest.mark.parametrize("name", sorted(D.SPILL3))
def test_spill3_scenes_reach_past_the_lds_entries(mi, L, name):
    """the scenes rendered with the 3-entry library: their depth-first bound fits that library (<= 23) and their camera paths reach level 5 or deeper, i.e. at
    least two entries of some ray's stack lie in HBM there.  Measured (32 x 32 x 4 spp, 4 bounces): comb need 17 / level 8, instanced_soup need 7 / level 5.
    On the default library no case's rays come near level 13: nest300 1, nest600 2, nest700 3, instanced_nest 3 -- one stack entry is a whole group of
    siblings, so chains stay shallow"""
    need, level = D.stack_levels(L, mi.load_dict(D.SPILL3[name](mi)))
    assert 3 < need <= D.STACK3_CAP, need
    assert level >= 5, level


def test_default_library_rays_stay_in_lds(mi, L):
    """what the GPU tests of the deep cases can NOT reach: with 13 LDS entries no camera path of a deep case touches the HBM columns (the dispatch, the 30-entry
    kernels and the refusal are what those cases test); if a builder change ever makes this fail, the deep cases have become a test of the columns too"""
    for name in sorted(D.DEEP):
        _, level = D.stack_levels(L, mi.load_dict(D.DEEP[name](mi)))
        assert level <= D.STACK_LDS, (name, level)


def test_cap_scenes_exist(mi, L):
    """nests exactly at the 3-entry library's bound and one past it, for its cap test"""
    assert D.nest_with_need(L, mi, D.STACK3_CAP) is not None and D.nest_with_need(L, mi, D.STACK3_CAP + 1) is not None
