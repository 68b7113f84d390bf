"""The REFERENCE'S OWN test functions, replayed against the CPU oracle and against the product's HAR_HD code compiled for the host, through the
`mitsuba` / `drjit` stand-ins of tests/ref_shim.  tests/golden/reference_suite.json holds what those functions ask of the backend (every call and
every known-answer check, recorded by tests/golden/make_golden.py); the two checks of derived quantities the recording cannot follow are restated
below.  These are the golden vectors that pin the microfacet model."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def suite():
    with open(os.path.join(ROOT, "tests", "golden", "reference_suite.json")) as f:
        return json.load(f)["tests"]


@pytest.fixture(scope="module")
def harness():
    H = C.CDLL(os.path.join(ROOT, "tests", "host_harness", "libhost_harness.so"))
    H.hh_fresnel_conductor.restype = C.c_float
    return H


MICROFACET_TESTS = ["test02_eval_pdf_beckmann", "test03_smith_g1_beckmann", "test04_sample_beckmann", "test03_smith_g1_ggx", "test05_sample_ggx"]


@pytest.mark.parametrize("backend", ["oracle", "product"])
def test_reference_microfacet_golden_vectors(O, harness, suite, backend):
    """src/render/tests/test_microfacet.py:15-285 (Mitsuba 0.6 golden data for eval / pdf / smith_g1 / sample)"""
    from tests.ref_shim import make_modules, replay_reference_checks
    mi, dr = make_modules(backend, O=O, H=harness)
    assert all(suite[n]["untracked"] == 0 for n in MICROFACET_TESTS)
    ran = replay_reference_checks(suite, MICROFACET_TESTS, mi)
    assert ran == MICROFACET_TESTS


FRESNEL_TESTS = ["test01_fresnel", "test02_fresnel_polarized_vec", "test03_fresnel_conductor", "test04_snell"]


@pytest.mark.parametrize("backend", ["oracle", "product"])
def test_reference_fresnel_known_answers(O, harness, suite, backend):
    """src/render/tests/test_fresnel.py:6-82 -- the unpolarised functions the dielectric / conductor / plastic BSDFs call (fresnel.h:38-116): normal incidence
    (4 %), the critical angle, the hyperphysics spot checks at 45 and 10 degrees, index-matched interfaces, conductor == dielectric for a real index, Snell's law.
    (`test02_fresnel_polarized_vec` is the unpolarised `mi.fresnel` on 20 angles despite its name; the polarised tests are outside an rgb variant.)"""
    from tests.ref_shim import make_modules, replay_reference_checks
    mi, dr = make_modules(backend, O=O, H=harness)
    ran = replay_reference_checks(suite, FRESNEL_TESTS, mi)
    assert ran == FRESNEL_TESTS
    # the checks on derived quantities (test_fresnel.py:16-34, 68-75), restated: the transmitted direction is a unit vector at the 45-degree
    # (1 -> 1.5) and 10-degree (1.5 -> 1) spot checks, and Snell's law holds on 20 angles from 0 to 90 degrees
    assert suite["test01_fresnel"]["untracked"] == 2 and suite["test04_snell"]["untracked"] == 1
    assert all(suite[n]["untracked"] == 0 for n in FRESNEL_TESTS if n not in ("test01_fresnel", "test04_snell"))
    for degrees, eta in ((45, 1.5), (10, 1 / 1.5)):
        cos_i = dr.cos(degrees * dr.pi / 180)
        _, cos_t, _, scale = mi.fresnel(cos_i, eta)
        assert dr.allclose((scale * dr.sqrt(1 - cos_i ** 2)) ** 2 + cos_t ** 2, 1), (degrees, eta)
    theta_i = dr.linspace(mi.Float, 0, dr.pi / 2, 20)
    _, cos_t, _, _ = mi.fresnel(dr.cos(theta_i), 1.5)
    assert dr.allclose(dr.sin(theta_i) - 1.5 * dr.sin(dr.acos(cos_t)), dr.zeros(mi.Float, 20), atol=1e-5)


def test_reference_discrete_distribution_known_answers(O, harness, suite):
    """src/core/tests/test_distr_1d.py:46-86,107-113 -- DiscreteDistribution::sample / sample_pmf / sample_reuse / sample_reuse_pmf on the hand-computed
    [1, 3, 2] table (values below 0 and above 1, either side of a bucket boundary, the re-used sample) and on a table with leading and trailing zeros:
    the face choice of the mesh area lights (Mesh::sample_position, src/render/mesh.cpp:1662-1712) in the oracle"""
    from tests.ref_shim import make_modules, replay_reference_checks
    mi, dr = make_modules("oracle", O=O, H=harness)
    names = ["test05_discr_sample", "test07_discr_leading_trailing_zeros"]
    assert all(suite[n]["untracked"] == 0 for n in names)
    assert replay_reference_checks(suite, names, mi) == names
