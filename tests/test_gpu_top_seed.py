"""Seeded closest-hit launches (integrator property `top_seed`, k_trace_closest<.., SEED>) against the unseeded ones on the GPU: the scene of
tests/top_seed_cases.py (box + coplanar + zero-area top-level triangles around three instances) through Integrator.sample and mi.render.
Integrator.sample has no atomics on its path, so its results must be equal bit for bit."""
import numpy as np
import pytest

from tests import top_seed_cases as TS

pytestmark = pytest.mark.gpu

N_TOP = 16


def _rays(n, seed=7):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-3.5, 3.5, (3, n)).astype(np.float32)
    d = rng.normal(size=(3, n)); d = (d / np.linalg.norm(d, axis=0)).astype(np.float32)
    return o, d, np.full(n, np.inf, np.float32)


def _sample(mi, scene, o, d, maxt):
    n = o.shape[1]
    sampler = mi.Sampler({"sample_count": 4, "seed": 5}); sampler.seed(3, n)
    spec, valid = scene.integrator().sample(scene, sampler, mi.Ray3f(o, d, maxt))
    return spec.cpu().numpy(), valid.cpu().numpy(), sampler.state.cpu().numpy()


@pytest.fixture(scope="module")
def scenes(mi):
    """{(kind, top_seed): scene}, built once"""
    return {(kind, ts): mi.load_dict(TS.scene_dict(mi, N_TOP, integrator=kind, top_seed=ts)) for kind in ("path", "prb") for ts in (False, True)}


@pytest.mark.parametrize("kind", ["path", "prb"])
@pytest.mark.parametrize("n", [7680, 9, 7680 - 37])
def test_sample_seeded_equals_unseeded(mi, scenes, kind, n):
    """7 680 incoherent rays: full and partial batches on all eight shards; 9: less than one wave; 7 680 - 37: a ragged end"""
    o, d, maxt = _rays(n)
    a = _sample(mi, scenes[(kind, False)], o, d, maxt)
    b = _sample(mi, scenes[(kind, True)], o, d, maxt)
    assert np.isfinite(a[0]).all() and a[0].max() > 0 and a[1].any()
    for x, y in zip(a, b):                                      # radiance, validity, sampler state
        assert np.array_equal(x.view(np.uint8) if x.dtype != bool else x, y.view(np.uint8) if y.dtype != bool else y)


def test_sample_adversarial_rays(mi, scenes):
    """the ray classes of the CPU test (origins on walls / edges / vertices, the coplanar pair, short and zero maxt, misses, |d| over 12 decades)"""
    o, d, maxt = TS.rays()
    a = _sample(mi, scenes[("path", False)], o, d, maxt)
    b = _sample(mi, scenes[("path", True)], o, d, maxt)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8) if x.dtype != bool else x, y.view(np.uint8) if y.dtype != bool else y)


def test_render_seeded_equals_unseeded(mi, scenes):
    """24 x 24 x 64 spp (the camera rays go through the packet kernel, bounces >= 1 through the seeded one): equal counters; the film is accumulated with
    float atomics, whose order is free: rel L2 < 1e-6"""
    imgs = []; stats = []
    for ts in (False, True):
        sc = scenes[("path", ts)]
        imgs.append(mi.render(sc, spp=64, seed=1).cpu().numpy().astype(np.float64))
        stats.append(sc.integrator().stats())
    assert stats[0] == stats[1] and stats[0]["closest_rays"] > 24 * 24 * 64
    assert np.linalg.norm(imgs[1] - imgs[0]) / np.linalg.norm(imgs[0]) < 1e-6


def test_moved_wall_is_picked_up(mi):
    """a wall vertex moved on the device (params.update() with a CUDA tensor rewrites the triangle records the seed reads): seeded still equals unseeded,
    and both differ from the scene before the move"""
    import torch
    o, d, maxt = _rays(7680, seed=9)
    out = {}
    for ts in (False, True):
        sc = mi.load_dict(TS.scene_dict(mi, N_TOP, top_seed=ts))
        before = _sample(mi, sc, o, d, maxt)
        params = mi.traverse(sc)
        p = params["box.positions"]
        p = (p if hasattr(p, "is_cuda") else torch.as_tensor(np.asarray(p, np.float32))).to("cuda").clone().reshape(-1, 3)
        p[7] = torch.tensor([2.5, 3.0, 2.0], device="cuda")                   # the (+, +, +) corner moves inwards: three walls tilt
        params["box.positions"] = p.reshape(-1); params.update()
        out[ts] = (before, _sample(mi, sc, o, d, maxt))
    for x, y in zip(out[False][1], out[True][1]):
        assert np.array_equal(x.view(np.uint8) if x.dtype != bool else x, y.view(np.uint8) if y.dtype != bool else y)
    assert not np.array_equal(out[True][0][0], out[True][1][0])
