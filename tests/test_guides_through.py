"""Guides through glass (yuki_amd/csrc/yk_guides_through.h) without a GPU: the declarations and constants of the new entry
points; the independent restatement (tests/guides_through_ref.py) against the float64 optics of a glass slab; that every
branch of the rule occurs on the cameras the GPU tests use; and the quality condition — the host denoiser steered by the
restatement's through-guides against first-hit guides, on oracle-rendered films."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import guides_through_ref as ref
from physics_cases import FLOOR, MARGIN, MAX_EXCLUDED, TOLERANCES
from yuki_amd import _ffi, abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITY_PROFILE = os.path.join(ROOT, "profiles", "guides_through_quality.json")


# ------------------------------------------------------------------ declarations
def test_constants_and_declarations():
    hdr = open(os.path.join(ROOT, "include", "yuki_hip.h")).read()
    assert int(re.search(r"#define YK_GUIDES_THROUGH_MAX (\d+)", hdr).group(1)) == abi.GUIDES_THROUGH_MAX == ref.MAX == 8
    rust = open(os.path.join(ROOT, "integration", "rust", "yuki_hip_sys", "src", "lib.rs")).read()
    assert int(re.search(r"pub const YK_GUIDES_THROUGH_MAX: u32 = (\d+);", rust).group(1)) == 8
    host, dev = _ffi.SYMBOLS["yk_render_guides_through"], _ffi.SYMBOLS["yk_render_guides_through_device"]
    ids = _ffi.SYMBOLS["yk_render_guides_ids"]
    assert host[1][:5] == ids[1][:5] and host[1][5] is C.c_uint32 and len(host[1]) == 9  # ... res_y, max_through, guides, ids, through
    assert dev[1][5] is C.c_uint32 and len(dev[1]) == 10  # ... and the stream
    L = _ffi.lib()
    assert hasattr(L, "yk_render_guides_through") and hasattr(L, "yk_render_guides_through_device")
    # the records are render_guides_ids': the passes downstream take them unchanged
    assert abi.GUIDE_DTYPE.itemsize == 32 and abi.SURFACE_ID_DTYPE.itemsize == 16 and np.dtype(np.uint32).itemsize == 4


def test_refused_without_a_context(yk):
    L = _ffi.lib()
    t = np.zeros(4, np.uint32)
    assert L.yk_render_guides_through(None, None, None, 2, 2, 4, None, None, t.ctypes.data) == 1
    assert L.yk_render_guides_through_device(None, None, None, 2, 2, 4, None, None, t.ctypes.data, None) == 1
    assert not t.any()
    with pytest.raises(ValueError):
        yk.write_output("unused.exr", np.zeros((2, 2, 3), np.float32), denoise=yk.DenoiseParams(), guides_through=(None, None))  # renders on the device: needs ctx
    with pytest.raises(ValueError):
        yk.write_preview("unused.png", np.zeros((2, 2, 3), np.float32), albedo=True)  # albedo=True takes the ids of guides_through's call


# ------------------------------------------------------------------ the restatement against float64 optics
def test_restatement_matches_slab_optics(yk, oracle):
    """Exit parallel to entry, the point on the wall against the closed form with both 1e-3 spawn offsets, T against the
    summed segment lengths.  Tolerances: tools/guides_through_tolerances.py, measured under other cameras."""
    with open(TOLERANCES) as fh:
        tol = json.load(fh)["guides_through"]
    assert tol["margin"] == MARGIN and tol["floor"] == FLOOR and tol["max_excluded"] == MAX_EXCLUDED
    score = ref.slab_score(yk, oracle, ref.CAMERA)
    print("slab optics:", score)
    assert score["compared"] > 1000 and score["excluded"] <= MAX_EXCLUDED
    for k in ref.OPTICS_FIGURES:
        row = tol["rows"][k]
        assert abs(row["tolerance"] - max(MARGIN * row["worst"], FLOOR)) <= 1e-5 * row["tolerance"]  # margin x worst, never below the floor (stored to six digits)
        assert score[k] <= row["tolerance"], (k, score[k], row["tolerance"])
    assert tol["rows"]["p_abs"]["tolerance"] < 1e-4  # the power of the check: one forgotten spawn offset moves the point by 1e-3
    o, d = np.array([[0.2, 0.1, 1.0]]), np.array([[0.1, -0.05, -1.0]])
    d /= np.linalg.norm(d)
    opt = ref.slab_optics(o, d)
    assert opt["ok"][0] and np.abs(opt["d_out"][0] - d[0]).max() < 1e-15  # the closed form itself: a plane-parallel slab shifts, it does not turn
    straight = o[0] + d[0] * (ref.WALL_Z - o[0, 2]) / d[0, 2]
    shift = np.linalg.norm(opt["p_wall"][0] - straight)
    # ... by the textbook h (tan i - tan t) in the wall's plane, plus what the two offsets skip: 1e-3 of glass and 1e-3 of air
    sin_i = np.sqrt(1.0 - d[0, 2] ** 2)
    tan_i, tan_t = sin_i / -d[0, 2], (sin_i / ref.SLAB["eta"]) / np.sqrt(1.0 - (sin_i / ref.SLAB["eta"]) ** 2)
    h = ref.SLAB["z"][1] - ref.SLAB["z"][0]
    assert abs(shift - (h * (tan_i - tan_t) + 1e-3 * (tan_i + tan_t))) < 1e-12 and 0.005 < shift < 0.01


# ------------------------------------------------------------------ the branches
@pytest.fixture(scope="module")
def branches(yk, oracle):
    """(scene, max_through) -> (through, branch) of the restatement on the GPU tests' cameras and film sizes."""
    out = {}
    jobs = [("cornell", (48, 48), 8), ("glass-balls", (48, 48), 8), ("city-small", (96, 54), 8)]
    jobs += [("glass-" + v, ref.RES, mt) for v in ref.VARIANTS for mt in (1, 8)]
    for name, res, mt in jobs:
        sd = ref.slab_scene(name[6:]) if name[6:] in ref.VARIANTS else scenes.by_name(name)
        cam = yk.Camera(sd.camera, yk.FilmSettings(res=res, tile_dim=16))
        osc = oracle.OracleScene(sd)
        g, i, through, branch = ref.guides_through(oracle, osc, sd, cam, res, mt)
        osc.close()
        out[(name, mt)] = (through, branch, g)
    return out


def _count(branch, code, k_min=0):
    return int((branch[..., k_min:] == code).any(axis=-1).sum())


def test_every_branch_occurs(branches):
    b = {k: v[1] for k, v in branches.items()}
    assert _count(b[("glass-slab", 8)], ref.TRANSMIT) > 0
    assert _count(b[("glass-prism", 8)], ref.TIR_REFLECT) > 0
    assert _count(b[("glass-mirror", 8)], ref.KT0_REFLECT) > 0 and _count(b[("glass-mirror", 8)], ref.TRANSMIT) == 0
    assert _count(b[("glass-black", 8)], ref.STOP) > 0 and not branches[("glass-black", 8)][0].any()
    assert _count(b[("glass-mirror", 8)], ref.MISS, 1) > 0  # miss after glass: the mirror shows the background
    assert _count(b[("glass-slab", 1)], ref.CUT) > 0 and _count(b[("glass-two", 1)], ref.CUT) > 0
    assert branches[("glass-two", 8)][0].max() >= 4  # two slabs: four interfaces
    for key, (through, branch, g) in branches.items():
        final = (branch == ref.FINAL) | (branch == ref.CUT) | (branch == ref.STOP)
        assert np.array_equal(final.any(axis=-1), g["hit"] != 0), key  # a record is written exactly where the walk ends on a surface
        assert through.max() <= key[1], key


def test_the_projects_scenes_have_work_for_the_rule(branches):
    """Cornell, glass-balls and city-small at the GPU tests' sizes: transmission and total internal reflection occur in each;
    rays leave Cornell after glass; city-small still holds rays inside glass after 8 interfaces."""
    for name in ("cornell", "glass-balls", "city-small"):
        through, branch, g = branches[(name, 8)]
        hist = ref.crossed_histogram(through, g)
        print(name, "pixels by interfaces crossed:", hist, ref.branch_counts(branch))
        assert _count(branch, ref.TRANSMIT) > 0 and _count(branch, ref.TIR_REFLECT) > 0
        assert sum(hist[1:]) > 0
    assert _count(branches[("cornell", 8)][1], ref.MISS, 1) > 0
    assert _count(branches[("city-small", 8)][1], ref.CUT) > 0


# ------------------------------------------------------------------ quality
def _bound(profile, name, figure):
    """The assertion bound of a figure: the midpoint between the worst ratio measured on the calibration seeds and 1, or
    None where that worst ratio is >= 0.95 (no gain to hold: README says so)."""
    worst = profile["scenes"][name]["worst"][figure]
    return None if worst >= 0.95 else 0.5 * (worst + 1.0)


@pytest.mark.parametrize("name", list(ref.QUALITY_SCENES))
def test_quality_on_oracle_films(yk, oracle, name):
    """4 spp against 1024 spp, host denoiser with default DenoiseParams, error on the pixels seen through glass: through-guides
    against first-hit guides, and on the slab scene also the demodulated filter with each pass's own albedo.  Bounds from
    profiles/guides_through_quality.json (tools/guides_through_quality.py, three other sampler seeds)."""
    with open(QUALITY_PROFILE) as fh:
        profile = json.load(fh)
    assert ref.QUALITY_TEST_SEED not in [int(s, 16) for s in profile["calibration_seeds"]]
    fig = ref.quality_figures(yk, oracle, name, ref.QUALITY_TEST_SEED)
    print(name, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in fig.items()})
    assert fig["masked_pixels"] > 100
    asserted = 0
    for figure in ("ratio", "albedo_ratio") if name == "glass-slab" else ("ratio",):
        bound = _bound(profile, name, figure)
        assert (bound is None) == (profile["scenes"][name]["asserted"][figure] is None)
        if bound is not None:
            assert fig[figure] <= bound, (name, figure, fig[figure], bound)
            asserted += 1
    if name == "glass-slab":
        assert asserted >= 1  # the scene the pass is for: something is held
