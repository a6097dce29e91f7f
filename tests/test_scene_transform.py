"""yk_scene_transform without a GPU (host-only scenes, ctx=None), against tests/transform_ref.py and tests/refit_ref.py:
identity records change no byte; moved records give the reference refit of the reference's points; transforms are absolute
(A then B is B, identity afterwards restores creation's bytes, negative zeros and the unreferenced vertex of coplanar-slabs
included); a transform equals the update with the transformed arrays; a mirroring matrix counts as flipped; every refusal
has its message, a fixed precedence, and leaves the tree alone; the motion pass from matrices equals the one from the
previous vertex array; the tree cost is the reference's within the derived bound.  The plan facts and the rule under the host
sanitizers are programs of their own (tests/cpp)."""
import copy
import os
import shutil
import subprocess

import numpy as np
import pytest

import motion_ref
import refit_ref
import transform_ref as ref
from test_scene_update import CASES, SCENES, sphere_table, tree_state
from yuki_amd import _ffi, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MOVED_SCENES = [name for name in SCENES if len(SCENES[name]().meshes)]


def lit_meshes(sd):
    al = np.asarray(sd.tri_area_light) if sd.tri_area_light is not None else np.full(sd.n_triangles, -1)
    tm = np.asarray(sd.tri_mesh) if sd.tri_mesh is not None else np.zeros(sd.n_triangles, np.uint32)
    return set(int(m) for m in np.unique(tm[al >= 0]))


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def matrices(sd, variant="A", mirror=False):
    """One matrix a mesh, None (identity) for the meshes that carry an area light and for every fourth mesh: rotations,
    non-uniform scales and translations of a few percent of the scene's diagonal; every third moved mesh is projective with
    w = 2 (the division of Transform * Point3); with `mirror` every other moved mesh is reflected in x."""
    p = np.asarray(sd.points, np.float64)
    diag = float(np.linalg.norm(p.max(axis=0) - p.min(axis=0))) if len(p) else 1.0
    centre = p.mean(axis=0) if len(p) else np.zeros(3)
    rng = np.random.default_rng(20261021 + (0 if variant == "A" else 77))
    lit, out, moved = lit_meshes(sd), [], 0
    for m in range(len(sd.meshes)):
        r = _rotation(rng.normal(size=3), rng.uniform(-0.4, 0.4)) @ np.diag(rng.uniform(0.8, 1.25, 3))
        t = rng.uniform(-0.05, 0.05, 3) * diag
        if m in lit or (m % 4 == 3 and len(sd.meshes) > 1):
            out.append(None)
            continue
        if mirror and moved % 2 == 0:
            r = r @ np.diag([-1.0, 1.0, 1.0])
        mat = np.eye(4)
        mat[:3, :3] = r
        mat[:3, 3] = centre - r @ centre + t  # about the scene's centre
        if moved % 3 == 2:
            mat = 2.0 * mat  # w = 2: the same points after the division
        moved += 1
        out.append(mat)
    return out


def records(sd, variant="A", mirror=False):
    return abi.pack_mesh_transforms(matrices(sd, variant, mirror))


def overflowing(sd, mesh):
    """Records that move `mesh` alone, by a scale and a shift of 3e38: finite matrices whose results are not."""
    big = np.diag([3e38, 3e38, 3e38, 1.0])
    big[:3, 3] = 3e38
    rec = abi.pack_mesh_transforms([big if m == mesh else None for m in range(len(sd.meshes))])
    assert np.isfinite(rec["rest_to_world"]).all() and np.isfinite(rec["world_to_rest"]).all()
    assert not np.isfinite(ref.transform(sd, rec)[0]).all()
    return rec


def make(yk, name, method=abi.SPLIT_SAH, max_shapes=4):
    sd = SCENES[name]()
    sd.split_method, sd.max_shapes_in_node = method, max_shapes
    return sd, yk.Scene(None, sd)


# ---- the reference itself
def test_reference_rule_pieces():
    eye = np.eye(4, dtype=F).reshape(16)
    minus = eye.copy()
    minus[[1, 7, 12]] = -0.0
    assert ref.is_identity(eye) and np.signbit(minus[7]) and ref.is_identity(minus) and not ref.is_identity(eye * F(2))
    p = np.array([[-0.0, 1.0, 2.0]], F)
    assert np.signbit(p[0, 0]) and not np.signbit(ref.xf_point(eye, p)[0, 0])  # why the identity case copies bits
    m = np.eye(4)
    m[3, 3] = 2.0
    assert np.array_equal(ref.xf_point(m.reshape(16), np.array([[2.0, 4.0, 6.0]], F)), np.array([[1.0, 2.0, 3.0]], F))
    mirror = np.diag([-1.0, 1.0, 1.0, 1.0]).reshape(16)
    assert ref.swaps_handedness(mirror) and not ref.swaps_handedness(eye)
    lo, hi = ref.vertex_mesh_table(np.array([[0, 1, 2], [2, 1, 3]]), np.array([0, 1]), 5)
    assert list(lo) == [0, 0, 0, 1, ref.NO_MESH] and list(hi) == [0, 1, 1, 1, 0] and list(ref.shared_vertices(lo, hi)) == [False, True, True, False, False]
    n = ref.xf_normal(np.diag([0.5, 1.0, 1.0, 1.0]).reshape(16), np.array([[1.0, 1.0, 0.0]], F))
    assert np.array_equal(n, np.array([[0.5, 1.0, 0.0]], F))
    assert abi.MESH_TRANSFORM_DTYPE.itemsize == 128


# ---- 1. identity
@pytest.mark.parametrize("name", list(SCENES))
def test_identity_records_change_nothing(yk, name):
    for method, max_shapes in CASES:
        sd, s = make(yk, name, method, max_shapes)
        before = tree_state(s)
        s.transform([None] * len(sd.meshes))
        assert tree_state(s) == before, (method, max_shapes)
        i = s.transform_info()
        assert (i.n_transforms, i.route, i.reason, i.n_moved_meshes, i.n_flipped_meshes) == (1, abi.UPDATE_ROUTE_HOST, 0, 0, 0)
        assert i.tree_cost == i.tree_cost_rest and i.rest_bytes > 0
        s.close()


# ---- 2. the rule
@pytest.mark.parametrize("name", MOVED_SCENES)
def test_moved_records_give_the_reference_refit(yk, name):
    table = sphere_table(yk, SCENES[name]())
    for method, max_shapes in CASES:
        sd, s = make(yk, name, method, max_shapes)
        nodes, order = s.export_bvh()
        rec = records(sd)
        want_points, _, flipped = ref.transform(sd, rec)
        assert not np.array_equal(want_points, sd.points) and not flipped.any()
        s.transform(rec)
        got, got_order = s.export_bvh()
        want = refit_ref.refit(nodes, order, want_points, sd.indices, table)
        assert got.tobytes() == want.tobytes(), (method, max_shapes)
        assert got.tobytes() != nodes.tobytes() and np.array_equal(got_order, order)
        i = s.info()
        assert bytes(i.bounds_min) == got["bmin"][0].tobytes() and bytes(i.bounds_max) == got["bmax"][0].tobytes()
        ti = s.transform_info()
        assert ti.n_moved_meshes == sum(m is not None for m in matrices(sd)) and ti.n_flipped_meshes == 0
        s.close()


# ---- 3. nothing accumulates
@pytest.mark.parametrize("name", MOVED_SCENES)
def test_transforms_are_absolute_and_identity_restores_creation(yk, name):
    sd, s = make(yk, name)
    created = tree_state(s)
    if name == "coplanar-slabs":  # what makes "byte for byte" hard: negative zeros, and a vertex no triangle indexes
        pts = np.asarray(sd.points, F)
        assert int((np.signbit(pts) & (pts == 0)).sum()) == 60
        assert int((ref.vertex_mesh_table(sd.indices, sd.tri_mesh, len(pts))[0] == ref.NO_MESH).sum()) == 1
    s.transform(records(sd, "A"))
    after_a = tree_state(s)
    s.transform(records(sd, "B"))
    after_ab = tree_state(s)
    sd2, s2 = make(yk, name)
    s2.transform(records(sd2, "B"))
    assert after_ab == tree_state(s2) and after_ab != after_a and after_a != created
    s.transform([None] * len(sd.meshes))
    assert tree_state(s) == created
    assert s.transform_info().n_transforms == 3 and s.transform_info().tree_cost_rest == s2.transform_info().tree_cost_rest
    # an update makes a new rest pose: the next transform is relative to it
    moved, _, _ = ref.transform(sd, records(sd, "A"))
    s.update(moved)
    assert s.transform_info().rest_bytes == 0
    s.transform([None] * len(sd.meshes))
    assert tree_state(s) == after_a and s.transform_info().rest_bytes > 0
    s.close()
    s2.close()


# ---- 4. against update, 5. mirror
@pytest.mark.parametrize("name", MOVED_SCENES)
@pytest.mark.parametrize("mirror", [False, True])
def test_transform_equals_update_with_the_transformed_arrays(yk, name, mirror):
    sd, s = make(yk, name)
    rec = records(sd, "A", mirror)
    points, normals, flipped = ref.transform(sd, rec)
    s.transform(rec)
    other = copy.copy(sd)
    other.meshes = ref.flipped_meshes(sd, flipped)  # the scene created with the mirrored meshes
    u = yk.Scene(None, other)
    u.update(points, normals)
    assert tree_state(s) == tree_state(u)
    assert s.transform_info().n_flipped_meshes == int(flipped.sum()) and bool(flipped.any()) == mirror
    s.close()
    u.close()


# ---- 6. refusals
def _refused(s, rec, message, before):
    with pytest.raises(_ffi.YukiError) as e:
        s.transform(rec)
    assert e.value.status == 1 and str(e.value).endswith(message), str(e.value)
    assert tree_state(s) == before


def _quad_over_two_meshes():
    sd = SCENES["two-shapes"]()
    sd = copy.copy(sd)
    sd.points = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F)
    sd.indices = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    sd.normals, sd.uvs, sd.shape_order, sd.spheres = None, None, None, []
    sd.tri_mesh = np.array([0, 1], np.uint32)
    sd.tri_material = np.zeros(2, np.int32)
    sd.tri_area_light = np.full(2, -1, np.int32)
    sd.meshes = [(False, False, False), (False, False, False)]
    return sd


@pytest.mark.parametrize("name,lit", [("cornell", 0), ("city-tiny", 7)])
def test_refusals_and_their_precedence(yk, name, lit):
    sd, s = make(yk, name)
    assert lit in lit_meshes(sd)
    before = tree_state(s)
    n = len(sd.meshes)
    free = [m for m in range(n) if m not in lit_meshes(sd)][0]
    shift = np.eye(4)
    shift[0, 3] = 0.25
    base = [None] * n
    with pytest.raises(_ffi.YukiError) as e:
        s.transform(None)
    assert e.value.status == 1 and str(e.value).endswith("null transforms")
    with pytest.raises(ValueError):
        s.transform(base[:-1])
    # a matrix entry that is not finite: either matrix of a moved record
    for field, value in (("rest_to_world", np.nan), ("rest_to_world", np.inf), ("world_to_rest", -np.inf), ("world_to_rest", np.nan)):
        rec = abi.pack_mesh_transforms(base[:free] + [shift] + base[free + 1:])
        rec[field][free][5] = value
        _refused(s, rec, "transforms: matrix entry not finite", before)
    rec = abi.pack_mesh_transforms(base)  # the inverse of an identity record is not read
    rec["world_to_rest"][free][3] = np.nan
    s.transform(rec)
    assert tree_state(s) == before
    # a mesh that carries an area light
    lit_rec = base[:lit] + [shift] + base[lit + 1:]
    _refused(s, lit_rec, "transforms: a mesh that carries an area light cannot move", before)
    # a result that is not finite
    over = overflowing(sd, free)
    _refused(s, over, "points: coordinate not finite", before)
    # precedence: matrix, then area light, then (below) shared vertex, then the result
    both = abi.pack_mesh_transforms(lit_rec)
    both["rest_to_world"][lit][0] = np.inf
    _refused(s, both, "transforms: matrix entry not finite", before)
    both = abi.pack_mesh_transforms(lit_rec)
    both["rest_to_world"][free], both["world_to_rest"][free] = over["rest_to_world"][free], over["world_to_rest"][free]
    _refused(s, both, "transforms: a mesh that carries an area light cannot move", before)
    assert s.transform_info().n_transforms == 1
    s.close()


def test_a_vertex_shared_by_two_meshes_refuses_every_transform(yk):
    sd = _quad_over_two_meshes()
    s = yk.Scene(None, sd)
    before = tree_state(s)
    shift = np.eye(4)
    shift[2, 3] = 1.0
    _refused(s, [None, None], "transforms: vertex shared by two meshes", before)
    _refused(s, [shift, None], "transforms: vertex shared by two meshes", before)
    _refused(s, overflowing(sd, 0), "transforms: vertex shared by two meshes", before)  # precedence: shared before the result ...
    bad = abi.pack_mesh_transforms([shift, None])  # ... and after the matrix
    bad["rest_to_world"][0][1] = np.nan
    _refused(s, bad, "transforms: matrix entry not finite", before)
    assert s.transform_info().n_transforms == 0
    s.close()


# ---- 7. motion from matrices
def _moved_spheres(sd):
    out = []
    for k, sp in enumerate(sd.spheres):
        t = np.eye(4)
        t[:3, 3] = [0.1 * (k + 1), -0.05, 0.02]
        o2w = t @ np.asarray(sp["o2w"], np.float64).reshape(4, 4)
        prev = dict(sp)
        prev["o2w"], prev["w2o"] = o2w.astype(F), np.linalg.inv(o2w).astype(F)
        prev["radius"] = float(sp["radius"]) * 1.25
        out.append(prev)
    return out


@pytest.mark.parametrize("name", ["cornell", "city-tiny"])
def test_motion_from_matrices_equals_motion_from_the_previous_vertices(yk, name):
    sd = SCENES[name]()
    prev = records(sd, "A", mirror=True)
    prev_points, _, _ = ref.transform(sd, prev)
    rng = np.random.default_rng(20261021)
    for transformed in (True, False):  # the scene transformed (the rest pose is kept), and never transformed (it is its own)
        sd, s = make(yk, name)
        if transformed:
            s.transform(records(sd, "B"))
        for w, h in ((33, 17), (8, 8)):
            ids, g = motion_ref.synthetic_ids(rng, w, h, sd.n_triangles, len(sd.spheres), True)
            got = yk.surface_motion(s, ids, g, prev_transforms=prev)
            want = yk.surface_motion(s, ids, g, prev_points)
            assert got.tobytes() == want.tobytes(), (name, w, h)
            assert (got["known"] == 1).any() and ((ids["shape"] < sd.n_triangles) & (got["known"] == 1)).any()
            at_rest = yk.surface_motion(s, ids, g, prev_transforms=None)
            assert at_rest.tobytes() == yk.surface_motion(s, ids, g, np.ascontiguousarray(sd.points, F)).tobytes()
            if len(sd.spheres):
                ps = _moved_spheres(sd)
                got = yk.surface_motion(s, ids, g, prev_transforms=prev, prev_spheres=ps)
                want = yk.surface_motion(s, ids, g, prev_points, prev_spheres=ps)
                assert got.tobytes() == want.tobytes() and got.tobytes() != yk.surface_motion(s, ids, g, prev_points).tobytes()
        with pytest.raises(ValueError):
            yk.surface_motion(s, ids, g, prev_points, prev_transforms=prev)
        s.close()


# ---- 8. tree cost
@pytest.mark.parametrize("name", MOVED_SCENES)
def test_tree_cost(yk, name):
    for max_shapes in (1, 4):
        sd, s = make(yk, name, abi.SPLIT_SAH, max_shapes)
        rest = ref.tree_cost(s.export_bvh()[0])
        s.transform(records(sd, "A"))
        i = s.transform_info()
        nodes = s.export_bvh()[0]
        want = ref.tree_cost(nodes)
        print(f"{name} leaves of {max_shapes}: tree_cost {i.tree_cost!r} (reference {want!r}), at rest {i.tree_cost_rest!r} (reference {rest!r}), bound {ref.cost_bound(len(nodes), want):.3e}")
        assert abs(i.tree_cost - want) <= ref.cost_bound(len(nodes), want)
        assert abs(i.tree_cost_rest - rest) <= ref.cost_bound(len(nodes), rest)
        assert i.tree_cost > 0 and i.tree_cost_rest > 0
        s.transform(records(sd, "A"))
        j = s.transform_info()
        assert (j.tree_cost, j.tree_cost_rest) == (i.tree_cost, i.tree_cost_rest)  # exactly reproducible, and the rest's stays
        s.transform(records(sd, "B"))
        assert s.transform_info().tree_cost_rest == i.tree_cost_rest
        s.close()


def test_the_cost_tracks_a_mesh_moved_across_the_scene(yk):
    """What the number is for: one building of city-tiny moved by 0, 0.1 and 1 scene diagonals.  The cost is relative to the
    ROOT's area, and a mesh that leaves the scene's box grows the root too: the ratio to tree_cost_rest may fall while the
    tree gets worse.  What must grow is the sum itself, tree_cost * A(root): every ancestor of a moved leaf now spans both
    places.  (A caller that compares across moves multiplies by the area of Scene.info()'s bounds.)"""
    sd, s = make(yk, "city-tiny")
    p = np.asarray(sd.points, np.float64)
    diag = float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
    free = [m for m in range(len(sd.meshes)) if m not in lit_meshes(sd)][0]
    ratios, sums = [], []
    for distance in (0.0, 0.1, 1.0):
        shift = np.eye(4)
        shift[0, 3] = distance * diag
        s.transform([shift if m == free else None for m in range(len(sd.meshes))])
        i, b = s.transform_info(), s.info()
        d = np.array(b.bounds_max[:], np.float64) - np.array(b.bounds_min[:], np.float64)
        ratios.append(i.tree_cost / i.tree_cost_rest)
        sums.append(i.tree_cost * 2.0 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]))
    print("tree_cost / tree_cost_rest at 0, 0.1 and 1 diagonals:", ratios, "tree_cost * A(root):", sums)
    assert ratios[0] == 1.0 and sums[0] < sums[2]  # (a tenth of a diagonal may move the building towards its neighbours)
    s.close()


# ---- 9. the plan facts and the rule as programs of their own
def test_scene_transform_plan(tmp_path):
    exe = str(tmp_path / "scene_transform_plan_test")
    subprocess.check_call(["hipcc", "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "scene_transform_plan_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "scene_transform_plan_test: ok" in out.stdout, out.stdout + out.stderr


def test_rule_program_under_the_host_sanitizers(tmp_path):
    """tests/cpp/transform_rule.cpp, a program of its own over the rule's header, compiled for the host with AddressSanitizer
    and UBSan (host code only: each sanitizer option goes to the host compilation alone) and run as that program."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "transform_rule"
    csrc = os.path.join(ROOT, "yuki_amd", "csrc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", csrc]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "cpp", "transform_rule.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "bad = 0" in r.stdout.splitlines()[-1] and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
