"""Shading against float64 physics, on the device: yk.bsdf_eval / bsdf_sample / light_sample, yk.camera_rays,
yk.sampler_sequence, yk.surface (both routes to the SurfaceInteraction) and Integrator.li (Path and Whitted); and the ties of the
surface stage to what a frame is made of: guides, the normal and uv integrators, li_debug's first bounce, Scene.update.

The same cases, seeded inputs, figures and tolerances as tests/test_physics.py (tests/physics_cases.py), answered by the
HIP kernels and compared with tests/physics_ref.py DIRECTLY — the oracle is not consulted, so this file keeps its meaning
even if oracle and device are ever changed together.  The tolerances were measured on the CPU oracle
(profiles/physics_tolerances.json); the device equals the oracle bit for bit, so nothing is calibrated here.

The camera, sampler and estimator cases (at most 65,536 li rays each, a few quads or one sphere, no film) run twice: on the default context and with
{"wide_bvh": 0, "overlap_shadow": 0, "shade_reorder": 0}, which takes the other route through the shade path.
"""
import copy

import numpy as np
import pytest

import physics_cases as K
import physics_ref as P
from yuki_amd import abi

pytestmark = pytest.mark.gpu

PLAIN = {"wide_bvh": 0, "overlap_shadow": 0, "shade_reorder": 0}
STAGE_CASES = [c for c in K.deterministic_cases() if c.startswith(("bsdf/", "light/"))]
SURFACE_CASES = [c for c in K.deterministic_cases() if c.startswith("surface/")]
LI_CASES = [c for c in K.deterministic_cases() if not c.startswith(("bsdf/", "light/", "surface/"))]
SF = abi.SURFACE_FIELDS


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


# ----------------------------------------------------------------------------- the surface stage
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _both_routes(be, sd, o, d):
    sc = be.yk.Scene(be.ctx, sd)
    try:
        return [be.yk.surface(be.ctx, sc, o, d, route) for route in (0, 1)]
    finally:
        sc.close()


@pytest.mark.parametrize("case_id", SURFACE_CASES)
def test_device_surface_matches_physics(backends, case_id):
    """yk_surface against the float64 surface on both routes — hit_surface_prim by the leaf-order slot (k_shade, the debug
    integrators, the guide pass) and hit_surface by the source shape (k_whitted, k_path_debug): each within the tolerances measured on
    the oracle, every id exact, the case's branches reached, and the two records equal bit for bit."""
    be = backends["default"]
    name = case_id.split("/")[1]
    for route in (0, 1):
        score = K.run_surface(be, name, K.SURFACE_SEED, route)
        K._show(f"{case_id} route {route}", score)
        assert K.check_score(case_id, score) == []
        assert score["compared"] > 0.9 and score["nan_mismatch"] == 0
        for rows in K.SURFACE_BRANCH[name]:
            assert score[rows] > 0, rows
    a, b = (K._ANSWERS[(be.name, "surface", name, K.SURFACE_SEED, route)] for route in (0, 1))
    assert np.array_equal(_bits(a), _bits(b))


def _camera_for(sd):
    if sd.spheres:
        c = np.asarray(sd.spheres[0]["o2w"], dtype=np.float64).reshape(4, 4)[:3, 3]
        return dict(position=tuple(c + (0.5, 0.7, 7.0)), target=tuple(c), up=(0.0, 1.0, 0.0), fov_axis=P.FOV_X, fov_degrees=60.0)
    return dict(position=(0.5, 0.7, 9.5), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_axis=P.FOV_X, fov_degrees=50.0)


FILM = 48


@pytest.fixture(scope="module", params=["mixed-meshes", "sphere-scaled"])
def framed(request, yk, ctx):
    """A surface case's scene under a 48 x 48 camera: the scene, the camera, the pixel-centre sampler, its rays and the stage's
    record of them on route 0 (route 1 equals it: test_device_surface_matches_physics)."""
    sd, _, _ = K.surface_inputs(request.param, K.SURFACE_SEED)
    fs = yk.FilmSettings(res=(FILM, FILM), tile_dim=FILM)
    cam = yk.Camera(_camera_for(sd), fs)
    sampler = yk.SamplerType.Stratified((1, 1), False)
    sc = yk.Scene(ctx, sd)
    o, d = yk.camera_rays(ctx, cam, sampler, (0, 0, FILM, FILM), 0)
    rec = yk.surface(ctx, sc, o, d, 0)
    assert np.array_equal(_bits(rec), _bits(yk.surface(ctx, sc, o, d, 1)))
    hit = rec[:, SF["hit"]] != 0
    assert 0.1 < hit.mean() < 1.0  # hits and misses both
    yield dict(sd=sd, sc=sc, fs=fs, cam=cam, sampler=sampler, rec=rec, hit=hit)
    sc.close()


def test_guides_equal_the_surface_stage(framed, yk, ctx):
    """render_guides_ids on the stage's camera rays: ns, p, t, the source shape and the barycentrics, bit for bit; a miss is the
    all-zero guide with shape SURFACE_NONE."""
    guides, ids = yk.render_guides_ids(ctx, framed["sc"], framed["cam"], framed["fs"])
    g, i, rec, hit = guides.reshape(-1), ids.reshape(-1), framed["rec"], framed["hit"]
    assert np.array_equal(g["hit"] != 0, hit)
    assert np.array_equal(_bits(g["ns"]), _bits(rec[:, SF["ns"]])) and np.array_equal(_bits(g["p"]), _bits(rec[:, SF["p"]]))
    assert np.array_equal(_bits(g["t"]), _bits(rec[:, SF["t"]]))
    assert np.array_equal(i["shape"][hit], rec[hit, SF["shape"]].astype(np.uint32)) and (i["shape"][~hit] == abi.SURFACE_NONE).all()
    assert np.array_equal(_bits(i["b"]), _bits(rec[:, SF["b"]]))


@pytest.mark.parametrize("which", ["GeometryNormals", "ShadingNormals", "ShadingUVs"])
def test_debug_integrators_equal_the_surface_stage(framed, yk, ctx, which):
    """The GeometryNormals, ShadingNormals and ShadingUVs renders are the stage's n / 2 + 0.5, ns / 2 + 0.5 and (u, v, 0), bit for
    bit, black on a miss."""
    it = yk.IntegratorType.instantiate(ctx, getattr(yk.IntegratorType, which))
    img, _ = it.render_tiles(framed["sc"], framed["cam"], framed["sampler"], yk.film_tiles(framed["fs"]))
    rec, hit = framed["rec"], framed["hit"]
    if which == "ShadingUVs":
        want = np.stack([rec[:, SF["u"]], rec[:, SF["v"]], np.zeros(len(rec), dtype=np.float32)], axis=-1)
    else:
        want = rec[:, SF["n"] if which == "GeometryNormals" else SF["ns"]] / np.float32(2.0) + np.float32(0.5)
    want = np.where(hit[:, None], want, np.float32(0.0)).astype(np.float32)
    assert np.array_equal(_bits(img.reshape(-1, 3)), _bits(want))


def test_li_debug_first_bounce_leaves_the_stage_surface(yk, ctx):
    """Path::li_debug at max_depth 2 on Lambert triangles with tilted vertex normals (no lights, so the first 2-D draw after the
    camera's is the lobe's): the first Reflection record starts at spawn_origin of the stage's p and n along the record's own
    direction, in f32 exactly; and that direction is to_world(cosine_hemisphere_sample(u), frame(ns, s)) of the float64 surface — the
    ledger's half-turned tangent included — with u from the sampler stage, within bsdf/lambert/tilted's s_wi_abs tolerance."""
    from test_gpu_li_debug import REFLECTION, _spawn

    sd, o, d = K.surface_inputs("normals", K.SURFACE_SEED)
    n = 512
    o, d = o[:n], d[:n]
    sc = yk.Scene(ctx, sd)
    sampler = K._sampler(1)
    pix = np.stack([np.arange(n) % 64, np.arange(n) // 64], axis=-1).astype(np.uint16)
    it = yk.IntegratorType.instantiate(ctx, K._path(2))
    _, _, rays = it.li_debug(sc, sampler, o, d, pix, np.zeros(n, np.uint32))
    rec = yk.surface(ctx, sc, o, d, 0)
    sc.close()
    r = K.surface_reference(sd, o, d)
    ex = K.surface_excluded(r, d)
    fr = P.frame(r["ns"], r["s"])
    wo_l = P.to_local(r["wo"], fr)
    u = np.stack([P.f64(yk.sampler_sequence(ctx, sampler, int(pix[i, 0]), int(pix[i, 1]), 0, [2, 2]))[1] for i in range(n)])
    wi_l = P.cosine_hemisphere_sample(wo_l, u)
    wi = P.to_world(wi_l, fr)
    ex |= (np.abs(wo_l[:, 2]) < K.COS_CUT) | (np.abs(2.0 * u - 1.0).max(axis=1) > 1.0 - 1e-6) | (np.abs(wi_l[:, 2]) < K.COS_CUT)
    tol = K.tolerance("bsdf/lambert/tilted", "s_wi_abs")
    checked, worst = 0, 0.0
    for i in range(n):
        if not r["hit"][i] or ex[i]:
            continue
        refl = rays[i][rays[i]["ray_type"] == REFLECTION]
        assert len(refl) == 1, i
        assert np.array_equal(_bits(refl["o"][0]), _bits(_spawn(rec[i, SF["p"]], rec[i, SF["n"]], refl["d"][0]))), i
        worst = max(worst, float(np.linalg.norm(P.f64(refl["d"][0]) - wi[i])))
        checked += 1
    print("first bounce: rows", checked, "worst direction error", worst, "tolerance", tol)
    assert checked > 0.9 * n and worst <= tol


def test_surface_follows_a_scene_update(backends):
    """Scene.update with every vertex moved and every normal re-tilted: surface/mixed-meshes passes again on both routes against the
    float64 surface of the NEW arrays, so neither the leaf-order copies (tris, prim_attr) nor the index-addressed arrays went stale."""
    be = backends["default"]
    sd, o, d = K.surface_inputs("mixed-meshes", K.SURFACE_SEED)
    rng = np.random.default_rng(K.SURFACE_SEED + 1)
    moved = (sd.points + rng.uniform(-0.05, 0.05, sd.points.shape)).astype(np.float32)
    assert (moved != sd.points).any(axis=1).all()
    tilted = K._tilted_normals(rng, moved, rng.integers(0, 4, len(moved) // 3) == 0)
    after = copy.copy(sd)
    after.points, after.normals = moved, tilted
    sc = be.yk.Scene(be.ctx, sd)
    try:
        before = be.yk.surface(be.ctx, sc, o, d, 0)
        sc.update(moved, tilted)
        got = [be.yk.surface(be.ctx, sc, o, d, route) for route in (0, 1)]
    finally:
        sc.close()
    assert np.array_equal(_bits(got[0]), _bits(got[1])) and not np.array_equal(_bits(got[0]), _bits(before))
    score = K.score_surface(after, o, d, got[0])
    K._show("surface/mixed-meshes after update", score)
    assert K.check_score("surface/mixed-meshes", score) == [] and score["compared"] > 0.9
    assert K.check_score("surface/mixed-meshes", K.score_surface(sd, o, d, got[0])) != []  # and no longer the old geometry's
