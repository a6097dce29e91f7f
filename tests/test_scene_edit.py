"""Scene.edit / yk_scene_apply_edit and the sphere case of the motion pass without a GPU (host-only scenes, ctx=None): an edit
with the scene's own tables leaves the tree as it is; the bound rule restated in numpy (tests/scene_edit_ref.py) is
creation's, bit for bit; moved spheres give the tree of tests/refit_ref.py fed with the restated bounds; refused edits write
nothing; the host instance of the motion pass with a previous sphere table equals its float32 restatement bit for bit and
stays within a measured tolerance (profiles/scene_edit_tolerances.json) of the float64 statement; and every edit a host-only
scene can be given runs as the hand-written table of tests/cpp/scene_change_table.inc says."""
import copy
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

import motion_ref
import refit_ref
import scene_edit_ref as ref
from test_motion import oracle_view
from test_scene_change_plan import row_of
from test_scene_update import SCENES as UPDATE_SCENES
from test_scene_update import sphere_table, tree_state
from test_temporal import camera, same_bits
from yuki_amd import _ffi, abi, scenes

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCES = os.path.join(ROOT, "profiles", "scene_edit_tolerances.json")

SCENES = {name: make for name, make in UPDATE_SCENES.items() if len(make().spheres) or len(make().lights)}
SCENES["glass_balls"] = scenes.glass_balls
CASES = [(m, k) for m in (abi.SPLIT_SAH, abi.SPLIT_MIDDLE) for k in (1, 4)]

EDIT_SYMBOLS = ("yk_scene_apply_edit", "yk_scene_apply_edit_device", "yk_scene_get_edit_info", "yk_surface_motion_spheres", "yk_surface_motion_spheres_device")


def own_tables(sd):
    return dict(spheres=sd.spheres, lights=sd.lights if sd.light_structs is None else sd.light_structs, materials=sd.materials, background=sd.background)


def test_the_abi_lists_the_new_symbols_and_records(yk):
    L = yk.lib()
    hdr = open(os.path.join(ROOT, "include", "yuki_hip.h")).read()
    for name in EDIT_SYMBOLS:
        assert name in _ffi.SYMBOLS and hasattr(L, name) and f" {name}(" in hdr, name
    assert abi.SPHERE_DTYPE.itemsize == C.sizeof(abi.SphereDesc) == 136
    assert [abi.SPHERE_DTYPE.fields[k][1] for k in ("object_to_world", "world_to_object", "radius", "material")] == [0, 64, 128, 132]
    assert C.sizeof(abi.SceneEditInfo) == 56 and C.sizeof(abi.SceneEdit) == 4 * C.sizeof(C.c_void_p)
    sd = scenes.glass_balls()
    packed = abi.pack_spheres(sd.spheres)
    assert packed.tobytes() == bytes(sd.sphere_descs())[: packed.nbytes]


# ---- 1. identity
@pytest.mark.parametrize("name", list(SCENES))
def test_edit_with_the_scenes_own_tables_changes_nothing(yk, name):
    for method, max_shapes in CASES:
        sd = SCENES[name]()
        sd.split_method, sd.max_shapes_in_node = method, max_shapes
        s = yk.Scene(None, sd)
        before = tree_state(s)
        s.edit(**own_tables(sd))
        assert tree_state(s) == before, (method, max_shapes)
        i = s.edit_info()
        assert (i.n_edits, i.route, i.reason) == (1, abi.UPDATE_ROUTE_HOST, 0)
        want = abi.EDIT_LIGHTS * bool(len(sd.lights)) | abi.EDIT_MATERIALS | abi.EDIT_BACKGROUND | (abi.EDIT_SPHERES | abi.EDIT_BOXES) * bool(len(sd.spheres))
        assert i.rewrote == want, (i.rewrote, want)
        for table in ("spheres", "lights", "materials", "background"):  # one table at a time, too
            s.edit(**{table: own_tables(sd)[table]})
            assert tree_state(s) == before, table
        s.close()


# ---- 2. the restated bound is creation's
@pytest.mark.parametrize("name", [n for n in SCENES if len(SCENES[n]().spheres)])
def test_the_restated_sphere_bounds_are_creations(yk, name):
    sd = SCENES[name]()
    assert ref.sphere_bounds(sd.spheres).tobytes() == sphere_table(yk, sd).tobytes()
    for move in ref.MOVES:  # and on spheres that are no plain translations
        msd = copy.copy(sd)
        msd.spheres = ref.moved_spheres(sd.spheres, move)
        assert ref.sphere_bounds(msd.spheres).tobytes() == sphere_table(yk, msd).tobytes(), move


# ---- 3. moved spheres
@pytest.mark.parametrize("move", ref.MOVES)
@pytest.mark.parametrize("name", ["cornell", "glass_balls"])
def test_moved_spheres_give_the_reference_refit(yk, name, move):
    for method, max_shapes in CASES:
        sd = SCENES[name]()
        sd.split_method, sd.max_shapes_in_node = method, max_shapes
        s = yk.Scene(None, sd)
        nodes, order = s.export_bvh()
        moved = ref.moved_spheres(sd.spheres, move)
        s.edit(spheres=moved)
        got, got_order = s.export_bvh()
        want = refit_ref.refit(nodes, order, sd.points, sd.indices, ref.sphere_bounds(moved))
        assert got.tobytes() == want.tobytes(), (method, max_shapes)
        assert got.tobytes() != nodes.tobytes()
        for field in ("a", "count", "axis", "is_leaf"):
            assert np.array_equal(got[field], nodes[field]), field
        assert np.array_equal(got_order, order)
        i = s.info()
        assert bytes(i.bounds_min) == got["bmin"][0].tobytes() and bytes(i.bounds_max) == got["bmax"][0].tobytes()
        e = s.edit_info()
        assert (e.n_edits, e.route, e.rewrote) == (1, abi.UPDATE_ROUTE_HOST, abi.EDIT_SPHERES | abi.EDIT_BOXES)
        assert s.data is not sd and s.data.spheres[0] is moved[0]
        s.edit(spheres=sd.spheres)  # and back
        assert s.export_bvh()[0].tobytes() == nodes.tobytes()
        s.close()


def test_a_sphere_edit_after_an_update_folds_the_updated_vertices(yk):
    from test_scene_update import wobble

    sd = SCENES["glass_balls"]()
    s = yk.Scene(None, sd)
    nodes, order = s.export_bvh()
    points = wobble(sd, 0.05)
    s.update(points)
    moved = ref.moved_spheres(sd.spheres, "rotation")
    s.edit(spheres=moved)
    assert s.export_bvh()[0].tobytes() == refit_ref.refit(nodes, order, points, sd.indices, ref.sphere_bounds(moved)).tobytes()
    s.close()


# ---- 4. refusals
def test_refused_edits_write_nothing(yk):
    sd = scenes.glass_balls()
    s = yk.Scene(None, sd)
    before = tree_state(s)
    data = s.data

    def refused(message, **tables):
        with pytest.raises(_ffi.YukiError) as e:
            s.edit(**tables)
        assert e.value.status == 1 and str(e.value).endswith(message), str(e.value)
        assert tree_state(s) == before and s.edit_info().n_edits == 0 and s.data is data

    lights = list(sd.lights)
    lights[1] = dict(kind="distant", w=(0.0, -1.0, 0.0), L=(1.0, 1.0, 1.0))
    refused("lights: a light's kind cannot change", lights=lights)
    for field, at, value in (("o2w", (1, 2), np.nan), ("w2o", (0, 3), np.nan), ("radius", None, np.inf), ("o2w", (2, 2), -np.inf)):
        spheres = copy.deepcopy(sd.spheres)
        if at is None:
            spheres[2][field] = value
        else:
            spheres[1][field] = np.array(spheres[1][field], dtype=F)
            spheres[1][field][at] = value
        refused("spheres: matrix entry or radius not finite", spheres=spheres)
    for material in (-1, len(sd.materials)):
        spheres = copy.deepcopy(sd.spheres)
        spheres[0]["material"] = material
        refused("sphere material out of range", spheres=spheres)
    materials = copy.deepcopy(sd.materials)
    materials[0]["tex"] = len(sd.textures)
    refused("material texture index out of range", materials=materials)
    # a good table beside a bad one: nothing of the good one is written either
    refused("sphere material out of range", spheres=spheres, lights=sd.lights, background=(1.0, 2.0, 3.0))
    L = yk.lib()
    assert L.yk_scene_apply_edit(None, s.h, None) == 1
    buf = C.create_string_buffer(256)
    L.yk_last_error(None, buf, 256)
    assert buf.value.decode().endswith("null edit")
    e = abi.SceneEdit()
    table = sd.sphere_descs()
    e.spheres = C.cast(table, C.POINTER(abi.SphereDesc))
    assert L.yk_scene_apply_edit_device(None, s.h, C.byref(e), C.c_void_p(C.addressof(table)), None) == 1
    L.yk_last_error(None, buf, 256)
    assert buf.value.decode().endswith("spheres given as a host table and as a device table")
    for wrong in (dict(spheres=sd.spheres[:-1]), dict(lights=sd.lights + sd.lights), dict(materials=sd.materials[1:]), dict(background=(0.0, 1.0))):
        with pytest.raises(ValueError):
            s.edit(**wrong)
    assert tree_state(s) == before and s.edit_info().n_edits == 0
    s.close()


# ---- 4b. the library follows the plan
def glass_for_matte(materials):
    """The table with material 2 (matte in cornell and in glass_balls) turned into glass, or back: its device BSDF kind changes."""
    out = copy.deepcopy(materials)
    out[2] = dict(kind=abi.MAT_GLASS, a=(1, 0.9, 0.9), b=(1, 1, 1), c=1.5) if out[2]["kind"] != abi.MAT_GLASS else dict(kind=abi.MAT_MATTE, a=(0.1, 0.2, 0.7), c=0.0)
    return out


def follow_the_edit_rows(s, sd, scene_kind, sphere_tables):
    """Every combination of sphere table (`sphere_tables`: row name -> what Scene.edit takes), lights, materials (none, the
    same kinds, changed kinds) and background, applied to `s` one after the other: route, reason and rewrote are the row's
    of tests/cpp/scene_change_table.inc, and n_edits rises by one.  Returns the rows it went through."""
    seen = set()
    materials = sd.materials  # as the scene has them now
    for brings, lights, mats, background in itertools.product(sphere_tables, (False, True), (None, "same", "changed"), (False, True)):
        row = row_of(scene_kind, brings, len(sd.spheres), mats == "changed")
        if mats == "changed":
            materials = glass_for_matte(materials)
        before = s.edit_info().n_edits
        s.edit(spheres=sphere_tables[brings], lights=own_tables(sd)["lights"] if lights else None, materials=materials if mats else None, background=(0.25, 0.5, 0.125) if background else None)
        i = s.edit_info()
        want = (abi.EDIT_LIGHTS * (lights and bool(len(sd.lights))) | abi.EDIT_MATERIALS * bool(mats) | abi.EDIT_BACKGROUND * background | abi.EDIT_SPHERES * row.spheres | abi.EDIT_BOXES * row.boxes
                | abi.EDIT_RECORDS * row.records)
        case = (scene_kind, brings, lights, mats, background)
        assert i.n_edits == before + 1, case
        assert (i.route, i.reason) == ({"HOST": abi.UPDATE_ROUTE_HOST, "DEVICE": abi.UPDATE_ROUTE_DEVICE}[row.verdict], 0), (case, i.route, i.reason)
        assert i.rewrote == want, (case, i.rewrote, want)
        assert (row.boxes or i.seconds_boxes == 0.0) and (row.boxes or row.records or i.seconds_records == 0.0), case  # a phase that did not run took no time
        seen.add(row)
    return seen


@pytest.mark.parametrize("name", ["cornell", "glass_balls"])
def test_a_host_only_scene_follows_the_plan(yk, name):
    sd = SCENES[name]()
    s = yk.Scene(None, sd)
    seen = follow_the_edit_rows(s, sd, "HOST_ONLY", {"NONE": None, "SPHERES_HOST": ref.moved_spheres(sd.spheres, "rotation")})
    assert {r[:4] for r in seen} == {("HOST_ONLY", b, 1, k) for b in ("NONE", "SPHERES_HOST") for k in (0, 1)}  # every row such a scene can reach
    with pytest.raises(ValueError):  # the REFUSED rows: Scene.edit sends no device table without a context ...
        s.edit(spheres=0x1000)
    e = abi.SceneEdit()  # ... and neither does the library
    assert yk.lib().yk_scene_apply_edit_device(None, s.h, C.byref(e), C.c_void_p(0x1000), None) == 1
    s.close()


# ---- 5. motion, host instance
@pytest.fixture(scope="module")
def balls(yk):
    sd = scenes.glass_balls()
    s = yk.Scene(None, sd)
    yield sd, s
    s.close()


def test_motion_without_previous_spheres_is_surface_motion(yk, balls):
    sd, s = balls
    rng = np.random.default_rng(20261021)
    ids, g = motion_ref.synthetic_ids(rng, 31, 17, sd.n_triangles, len(sd.spheres))
    prev = motion_ref.rough_points(rng, sd.points)
    assert same_bits(yk.surface_motion(s, ids, g, prev, prev_spheres=None), yk.surface_motion(s, ids, g, prev))


@pytest.mark.parametrize("move", ref.MOVES)
def test_motion_host_equals_the_restatement(yk, balls, move):
    """Hand-made records of every kind — sphere pixels, triangle pixels, misses, shapes out of range, NaN and infinite
    points — under a previous table whose spheres stood elsewhere, one of them with another radius."""
    sd, s = balls
    nt, ns = sd.n_triangles, len(sd.spheres)
    rng = np.random.default_rng(777)
    ids, g = motion_ref.synthetic_ids(rng, 33, 19, nt, ns)
    prev_points = motion_ref.rough_points(rng, sd.points)
    prev = ref.moved_spheres(sd.spheres, move)
    prev[1] = dict(prev[1], radius=float(F(0.045)))
    current, previous = abi.pack_spheres(sd.spheres), abi.pack_spheres(prev)
    got = yk.surface_motion(s, ids, g, prev_points, prev_spheres=prev)
    want = ref.surface_motion(ids, g, sd.indices, prev_points, nt, current, previous)
    assert same_bits(got, want), np.argwhere(got.view(np.uint32).reshape(got.shape + (4,)) != want.view(np.uint32).reshape(got.shape + (4,)))[:4]
    assert same_bits(yk.surface_motion(s, ids, g, prev_points, prev_spheres=previous), want)  # records or dicts
    live = (ids["shape"] != motion_ref.SURFACE_NONE) & (g["hit"] != 0)
    kinds = [int((~live).sum()), int((live & (ids["shape"] >= nt + ns)).sum()), int((live & (ids["shape"] == nt + 1)).sum()), int((live & (ids["shape"] >= nt) & (ids["shape"] < nt + ns)).sum()),
             int((live & (ids["shape"] < nt)).sum())]
    assert min(kinds) > 0, kinds
    old = yk.surface_motion(s, ids, g, prev_points)  # the sphere pixels moved, nothing else did
    sph = live & (ids["shape"] >= nt) & (ids["shape"] < nt + ns)
    assert same_bits(got[~sph], old[~sph]) and not same_bits(got[sph], old[sph])
    with pytest.raises(ValueError):
        yk.surface_motion(s, ids, g, prev_points, prev_spheres=previous[:-1])


def test_motion_of_a_scene_without_triangles_needs_no_points(yk):
    sd = scenes.glass_balls()
    only = copy.copy(sd)
    only.points, only.indices = np.zeros((0, 3), F), np.zeros((0, 3), np.uint32)
    only.tri_mesh, only.tri_material, only.tri_area_light = np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    only.meshes, only.uvs, only.lights = [], None, [sd.lights[1]]
    s = yk.Scene(None, only)
    rng = np.random.default_rng(5)
    ids, g = motion_ref.synthetic_ids(rng, 16, 9, 0, len(only.spheres))
    prev = ref.moved_spheres(only.spheres, "rotation")
    got = yk.surface_motion(s, ids, g, None, prev_spheres=prev)
    assert same_bits(got, ref.surface_motion(ids, g, None, None, 0, abi.pack_spheres(only.spheres), abi.pack_spheres(prev)))
    assert (got["known"] == 1).any()
    with pytest.raises(_ffi.YukiError):
        _ffi.check(yk.lib().yk_surface_motion_spheres(None, s.h, ids.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), None, None, 16, 9, got.ctypes.data_as(C.c_void_p)))
    s.close()


# ---- 6. motion against float64
RES = (24, 24)
TEST_SEED = 0x5CE7E
CALIBRATION_SEEDS = (11, 12, 13, 14, 15, 16, 17, 18)


def motion_case(seed):
    """glass_balls with every sphere translated and rotated, both drawn from `seed`: (the scene's data before, after)."""
    sd = scenes.glass_balls()
    rng = np.random.default_rng(seed)
    diag = float(np.linalg.norm(np.asarray(sd.points).max(axis=0) - np.asarray(sd.points).min(axis=0)))
    moved = []
    for s in sd.spheres:
        c = np.asarray(s["o2w"], np.float64).reshape(4, 4)[:3, 3]
        t = np.eye(4)
        d = rng.standard_normal(3)
        t[:3, 3] = 0.03 * diag * d / np.linalg.norm(d)
        r = ref._about(c + 0.02 * rng.standard_normal(3), ref._rotation(rng.standard_normal(3), rng.uniform(0.1, 0.6)))
        moved.append(ref.transformed(s, t @ r))
    after = copy.copy(sd)
    after.spheres = moved
    return sd, after, diag


def motion_error(yk, oracle, seed):
    """The largest distance, in scene diagonals, between the host instance's p_prev and the float64 statement over the
    sphere pixels of the 24 x 24 view of the moved scene; and how many such pixels there were."""
    before, after, diag = motion_case(seed)
    osc = oracle.OracleScene(after)
    g, ids = oracle_view(oracle, osc, after, camera(yk, after.camera, RES), RES)
    osc.close()
    s = yk.Scene(None, after)
    got = yk.surface_motion(s, ids, g, np.ascontiguousarray(before.points, F), prev_spheres=before.spheres)
    s.close()
    nt = after.n_triangles
    sph = (got["known"] == 1) & (ids["shape"] >= nt)
    k = (ids["shape"][sph] - nt).astype(np.int64)
    want = ref.sphere_p_prev64(g["p"][sph], abi.pack_spheres(after.spheres), abi.pack_spheres(before.spheres), k)
    return float(np.abs(got["p_prev"][sph].astype(np.float64) - want).max() / diag), int(sph.sum())


def motion_tolerance():
    with open(TOLERANCES) as f:
        return json.load(f)["sphere_motion_p_prev"]["tolerance"]


def test_motion_against_float64(yk, oracle):
    """Measured on the calibration seeds by tools/scene_edit_tolerances.py: the worst error of the host instance against
    the float64 statement, times 4 (the margin of tools/physics_tolerances.py for differences that are rounding only)."""
    with open(TOLERANCES) as f:
        rec = json.load(f)["sphere_motion_p_prev"]
    assert rec["tolerance"] == pytest.approx(4 * rec["worst"], rel=1e-5) and TEST_SEED not in rec["seeds"] and list(CALIBRATION_SEEDS) == rec["seeds"]
    err, n = motion_error(yk, oracle, TEST_SEED)
    print(f"sphere motion against float64: {err:.3e} scene diagonals over {n} sphere pixels, tolerance {rec['tolerance']:.3e}")
    assert n >= 20
    assert err <= rec["tolerance"]
    # power: the move itself is four orders of magnitude above the tolerance
    assert 0.03 > 1e3 * rec["tolerance"]
