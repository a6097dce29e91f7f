"""Shading against float64 physics, on the CPU oracle: BSDF lobes, lights, the camera, the samplers' structure, Whitted's
recursion, the Path estimator with its roulette, and the surface a hit is turned into before any of them sees it.

Every other shading test asks whether the device equals the oracle; these ask whether the oracle (and, in
tests/test_gpu_physics.py, the device) equals the published models, restated in float64 by tests/physics_ref.py from the
textbook and not from our code.  Where the reference renderer knowingly differs, physics_ref.DEVIATIONS says so, and
test_ledger_entry_is_live proves that each entry is needed; test_mutation_is_caught proves that a single misread term in
the physics would be noticed.  Tolerances are measured (tools/physics_tolerances.py -> profiles/physics_tolerances.json):
4 x the oracle's worst error on calibration seeds that these tests do not use.  Cases, inputs and figures: tests/physics_cases.py.
"""
import os
import sys

import pytest

import physics_cases as K
import physics_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z_MAX = K.Z_MAX


@pytest.fixture(scope="module")
def be(oracle):
    return K.OracleBackend(oracle)


@pytest.mark.parametrize("case_id", list(K.deterministic_cases()))
def test_stage_or_estimator_matches_physics(be, case_id):
    """Bsdf::f / sample_f per material (orthonormal frame, and ns != ng), Light::sample_li per kind, Path::li at depth 1 under a
    point, spot and distant light and the exact furnaces; camera rays over five resolutions, three fields of view on either
    axis, a far and a downward camera, and their jittered link to the sampler; the samplers' strata, permutations and seek rule;
    Whitted over one and three panes to depth 16, with ray counts; path lengths under the roulette, per-sample radiance through a
    pane, the indirect clamp and the sphere's wo; the SurfaceInteraction of triangle and sphere hits (ten scenes of
    tests/physics_cases.py SURFACE_CASES) and, at depth 1 above it, Lambert quads with tilted vertex normals and image-textured
    surfaces: every figure within its measured tolerance (a |z| within 4), the zero /
    no-sample / flag / count patterns exactly as float64 predicts, at most 5 % of a batch excluded."""
    K.check_deterministic(be, case_id)


@pytest.mark.parametrize("name", list(K.mc_cases()))
def test_estimator_mean_matches_physics(be, name):
    """Monte-Carlo cases (Uniform sampler, fixed seed, N from the tolerance file): the furnace mean against B x the
    directional albedo by quadrature (or B for the R = T = 1 pane), the same with a light below the floor, and a Lambert
    floor under the rectangular light against Lambert's polygon formula — within 4 standard errors."""
    K.check_monte_carlo(be, name)


def test_light_below_the_floor_shifts_the_draws(be):
    """Quirk 4, per sample: the unused light consumes two dimensions."""
    r = K.run_dimension_shift(be)
    assert r["shift_mismatch"] == 0 and r["shift_rows_differing"] > 200, r


def _figure(be, where):
    case_id, figure = where
    if case_id == "estimator":
        if figure == "emitter_through_pane":
            r = K.run_emitter_through_pane(be)
            assert 0.3 < r["lit_share"] < 0.7
            return r["emission_rel"], 2.0**-20  # beta and beta^2 Le take three f32 roundings
        r = K.run_dimension_shift(be)
        return float(r["shift_mismatch"]), 0.0
    return K.run_case(be, case_id)[figure], _bound(case_id, figure)


def _bound(case_id, figure):
    """What a figure is held to: its measured tolerance, Z_MAX for a |z|, 0 for a count of mismatches."""
    if K.is_toleranced(figure):
        return K.tolerance(case_id, figure)
    return Z_MAX if figure.endswith("_z") else 0.0


@pytest.mark.parametrize("key", [d["key"] for d in P.DEVIATIONS])
def test_ledger_entry_is_live(be, key):
    """With the entry on, its figure passes; with the entry off — the textbook expected — the same figure fails.  So no
    entry can hide a bug: the day the reference's behaviour and the textbook's coincide for these inputs, this fails."""
    entry = next(d for d in P.DEVIATIONS if d["key"] == key)
    value, tol = _figure(be, entry["live"])
    assert value <= tol, (key, value, tol)
    with P.textbook(key):
        off, _ = _figure(be, entry["live"])
    print(key, entry["live"], "on", value, "off", off, "tolerance", tol)
    assert off > max(tol, 0.0) and off > 10 * value, (key, off, tol)


MUTATION_CASES = {
    "schlick_exponent_4": ("bsdf/glossy-0.3/ortho", "f_rel"),
    "oren_nayar_030": ("bsdf/oren-nayar-0.349/ortho", "f_rel"),
    "g_dropped": ("bsdf/metal-0.2/ortho", "f_rel"),
    "pdf_without_jacobian": ("bsdf/metal-0.2/ortho", "s_pdf_rel"),
    "albedo_without_cos": ("mc", "furnace/metal-0.2/45"),
    "fresnel_rpar_swapped_eta": ("bsdf/glass-1.5/ortho", "s_fresnel_abs"),
    "li_inverse_distance": ("light/point", "li_rel"),
    "rect_pdf_without_cos": ("light/rect", "pdf_rel"),
    "snell_eta_inverted": ("bsdf/glass-1.5/ortho", "s_wi_abs"),
    "sigma_to_degrees": ("bsdf/oren-nayar-1.0/ortho", "f_rel"),
    "camera_tan_full_fov": ("camera/y90", "d_angle_abs"),
    "camera_y_up": ("camera/down", "d_angle_abs"),
    "camera_window_on_shorter_axis": ("camera/x170", "d_angle_abs"),
    "strata_cell_transposed": ("sampler/strata-2d-rect", "cells_mismatch"),
    "whitted_child_over_pdf": ("whitted/3-tinted/d16", "li_rel"),
    "whitted_eta2": ("whitted-from-inside/tinted/d8", "li_rel"),
    "rr_from_bounce_3": ("rr-lengths/warm", "length_z"),
    "rr_without_compensation": ("rr-lengths/green", "length_z"),
    "rr_floor_010": ("rr-lengths/green", "length_z"),
    "clamp_after_beta": ("clamp/emitter-through-pane", "emission_rel"),
    "bary_rotated": ("surface/plain", "p_pos"),
    "ns_unnormalised": ("surface/normals", "ns_abs"),
    "swaps_ignored": ("surface/sphere-mirrored", "side_mismatch"),  # a mesh with normals turns n to ns whatever the flag says
    "n_not_faceforwarded": ("surface/normals", "side_mismatch"),
    "tangent_from_dpdv": ("surface/uvs", "s_abs"),
    "sphere_normal_by_m": ("surface/sphere-scaled", "n_abs"),
    "texel_v_not_flipped": ("direct-textured/quad", "li_rel"),
    "spawn_along_ns": ("surface/normals", "origin_pos"),
}


@pytest.mark.parametrize("name", P.MUTATIONS)
def test_mutation_is_caught(be, name):
    """The power check: one single-term mistake planted in the REFERENCE must push its comparison past 10 x the tolerance
    in use (for the Monte-Carlo case and for the counts of path lengths: past 10 x the 4 standard errors, |z| >= 40)."""
    case_id, figure = MUTATION_CASES[name]
    with P.mutated(name):
        if case_id == "mc":
            spec = K.mc_cases()[figure]
            fig = K.mc_figures(K.mc_samples(be, spec, K.tolerances()["monte_carlo"][figure]["n"]), K.mc_truth(spec))
            value, tol = abs(fig["z"]), Z_MAX
        else:
            value, tol = K.run_case(be, case_id)[figure], _bound(case_id, figure)
    print(name, case_id, figure, value, tol)
    assert value >= 10 * tol and value > 0, (name, value, tol)  # a count of mismatches is held to 0: any will do


@pytest.mark.parametrize("name", K.SURFACE_CASES)
def test_surface_case_reaches_its_branch(be, name):
    """Every surface case records how many compared rows took each branch of the surface code; the branches it was built for
    (tests/physics_cases.py SURFACE_BRANCH) have rows, and no output is NaN."""
    score = K.run_case(be, f"surface/{name}")
    for rows in K.SURFACE_BRANCH[name]:
        assert score[rows] > 0, (name, rows)
    if name == "sphere-poles":
        assert score["nudge_rows"] == 64
    assert score["nan_mismatch"] == 0


@pytest.mark.parametrize("case_id", K.surface_stage_cases())
def test_surface_exclusions_stay_under_the_cap(case_id):
    """What a surface case leaves out is decided by the float64 reference alone: evaluated with no back end, on the test seed and on
    every calibration seed, the excluded share stays at or below MAX_EXCLUDED."""
    _, _, seed, calibration = K.all_cases()[case_id]
    for s in (seed,) + tuple(calibration):
        assert K.excluded_share(case_id, s) <= K.MAX_EXCLUDED, (case_id, s)


def test_surface_tolerances_stay_below_the_cap():
    """No figure of the surface stage calibrates above 1e-4, an order below where a misread term shows: one that did would mean a
    missing conditioning factor or a wrong oracle, not a reason for a wider bound."""
    rows = {k: v for k, v in K.tolerances()["rows"].items() if k.split(":")[0] in K.surface_stage_cases()}
    assert len(rows) >= 100
    for key, row in rows.items():
        assert row["tolerance"] <= 1e-4 and row["excluded"] <= K.MAX_EXCLUDED, (key, row)


def test_every_mutation_has_a_case():
    assert set(MUTATION_CASES) == set(P.MUTATIONS) and len(P.MUTATIONS) >= 10


def test_tolerance_file_is_current(be):
    """profiles/physics_tolerances.json covers exactly today's cases with tolerance = 4 x worst (at least one f32 ulp), and
    one row, measured again on its calibration seeds, gives the recorded figures."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import physics_tolerances as T

    doc = K.tolerances()
    assert doc["margin"] == K.MARGIN == 4.0
    want_rows = set()
    for case_id in K.all_cases():
        want_rows |= {f"{case_id}:{k}" for k in K.run_case(be, case_id) if K.is_toleranced(k)}
    assert set(doc["rows"]) == want_rows
    assert set(doc["monte_carlo"]) == set(K.mc_cases())
    for key, row in doc["rows"].items():
        assert row["tolerance"] == pytest.approx(K.adopt(row["worst"]), rel=1e-5), key
        assert row["excluded"] <= K.MAX_EXCLUDED, key
    for name, rec in doc["monte_carlo"].items():
        assert rec["n"] & (rec["n"] - 1) == 0 and 256 <= rec["n"] <= 65536
        assert abs(rec["z"]) <= 3 or rec.get("note"), name
    case_id = "bsdf/metal-0.2/tilted"
    for k, row in T.measure_row(be, case_id).items():
        assert row["worst"] == pytest.approx(doc["rows"][f"{case_id}:{k}"]["worst"], rel=1e-4), k
    rec = T.measure_mc(be, "rect/1")
    assert rec["n"] == doc["monte_carlo"]["rect/1"]["n"] and rec["z"] == pytest.approx(doc["monte_carlo"]["rect/1"]["z"], abs=1e-3)


def test_ledger_is_written_down():
    """Every ledger entry cites the reference and its sentence stands in SURVEY's quirk ledger; the float64 reference does
    not lean on the code it judges."""
    with open(os.path.join(ROOT, "SURVEY.md")) as fh:
        survey = fh.read()
    keys = [d["key"] for d in P.DEVIATIONS]
    assert len(set(keys)) == len(keys)
    for d in P.DEVIATIONS:
        assert ".rs:" in d["where"], d["key"]
        assert d["sentence"] in survey, d["key"]
    for q in (2, 4, 9, 11, 12, 13):
        assert any(d["quirk"] == q for d in P.DEVIATIONS), q
    with open(os.path.join(ROOT, "tests", "physics_ref.py")) as fh:
        src = fh.read()
    imports = [line.split()[1].split(".")[0] for line in src.splitlines() if line.startswith(("import ", "from "))]
    assert sorted(imports) == ["contextlib", "numpy"]
