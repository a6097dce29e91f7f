"""Shading against float64 physics, on the device: yk.bsdf_eval / bsdf_sample / light_sample, yk.camera_rays,
yk.sampler_sequence and Integrator.li (Path and Whitted).

The same cases, seeded inputs, figures and tolerances as tests/test_physics.py (tests/physics_cases.py), answered by the
HIP kernels and compared with tests/physics_ref.py DIRECTLY — the oracle is not consulted, so this file keeps its meaning
even if oracle and device are ever changed together.  The tolerances were measured on the CPU oracle
(profiles/physics_tolerances.json); the device equals the oracle bit for bit, so nothing is calibrated here.

The camera, sampler and estimator cases (at most 65,536 li rays each, a few quads or one sphere, no film) run twice: on the default context and with
{"wide_bvh": 0, "overlap_shadow": 0, "shade_reorder": 0}, which takes the other route through the shade path.
"""
import pytest

import physics_cases as K

pytestmark = pytest.mark.gpu

PLAIN = {"wide_bvh": 0, "overlap_shadow": 0, "shade_reorder": 0}
STAGE_CASES = [c for c in K.deterministic_cases() if c.startswith(("bsdf/", "light/"))]
LI_CASES = [c for c in K.deterministic_cases() if not c.startswith(("bsdf/", "light/"))]


@pytest.fixture(scope="module")
def backends(yk, ctx):
    plain = yk.Context(0, **PLAIN)
    d, p = K.DeviceBackend(yk, ctx), K.DeviceBackend(yk, plain)
    p.name = "device-plain"
    yield {"default": d, "plain": p}
    plain.close()


@pytest.mark.parametrize("case_id", STAGE_CASES)
def test_device_stage_matches_physics(backends, case_id):
    """Bsdf::f / sample_f per material (orthonormal and tilted frames) and Light::sample_li per kind on the device."""
    K.check_deterministic(backends["default"], case_id)


@pytest.mark.parametrize("options", ["default", "plain"])
@pytest.mark.parametrize("case_id", LI_CASES)
def test_device_li_matches_physics(backends, case_id, options):
    """Path::li at depth 1 under a point, a spot and a distant light (closed form per ray) and the exact furnaces; yk_camera_init +
    yk_camera_rays against the float64 pinhole camera and k_raygen's jitter against the sampler stage; the samplers' strata,
    permutations (against Kensler's algorithm in Python integers) and seek rule; k_whitted against the float64 recursion over
    one and three panes up to the device's depth cap; k_shade's roulette through the per-sample radiance classes of a pane and
    the path lengths in a closed sphere; the indirect clamp; the sphere's wo."""
    K.check_deterministic(backends[options], case_id)


@pytest.mark.parametrize("options", ["default", "plain"])
@pytest.mark.parametrize("name", list(K.mc_cases()))
def test_device_li_mean_matches_physics(backends, name, options):
    """Furnace means against B x albedo, with and without a light below the floor, and the rectangular light against
    Lambert's polygon formula, within 4 standard errors at the N the tolerance file records."""
    K.check_monte_carlo(backends[options], name)


@pytest.mark.parametrize("options", ["default", "plain"])
def test_device_whitted_refuses_depth_17(backends, yk, options):
    """The device's Whitted keeps 16 frames: max_depth 17 is refused with YK_ERR_UNSUPPORTED before anything runs."""
    be = backends[options]
    with pytest.raises(yk.YukiError) as e:
        K.run_whitted(be, 1, "clear", 17, K.WHITTED_SEED)
    assert e.value.status == 5, e.value


@pytest.mark.parametrize("options", ["default", "plain"])
def test_device_light_below_the_floor_shifts_the_draws(backends, options):
    r = K.run_dimension_shift(backends[options])
    assert r["shift_mismatch"] == 0 and r["shift_rows_differing"] > 200, r
