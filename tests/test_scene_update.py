"""yk_scene_update / yk_bvh_refit without a GPU (host-only scenes, ctx=None): an update with the scene's own points leaves
the tree and the info as they are, bit for bit; an update with moved points gives the tree of tests/refit_ref.py with every
link, axis, count and the leaf order untouched; bad arguments are refused before anything is written; and the moved
geometry itself stays inside the caps of the traversal checks (tests/test_trace_reference.py), so that the GPU tests that
trace through refitted trees judge the refit and not their inputs."""
import copy

import numpy as np
import pytest

import refit_ref
import test_trace_reference as tr
import trace_ref
from test_gpu_scene_layout import SCENES as LAYOUT_SCENES
from test_gpu_scene_layout import _line_of_triangles
from yuki_amd import _ffi, abi

SMALL = ("one-shape", "two-shapes", "cornell", "city-tiny", "city-tiny-permuted", "signed-zeros", "coplanar-slabs")
SCENES = {name: LAYOUT_SCENES[name] for name in SMALL}
TRACED = {"cornell": LAYOUT_SCENES["cornell"], "city-small": LAYOUT_SCENES["city-small"], "deep-line": _line_of_triangles}  # deep-line: a tree deeper than 64
SEED = 0x5CE7E


def wobble(sd, fraction=0.01, phase=0.0):
    """The points of `sd` moved by a smooth wave of `fraction` of the scene's diagonal (about one and a half periods across
    the box, another axis driving each coordinate).  Vertices of triangles that carry an area light stay: a rectangular
    light's record is not moved by an update."""
    p = np.ascontiguousarray(sd.points, dtype=np.float32)
    lo, hi = p.min(axis=0), p.max(axis=0)
    ext = np.maximum(hi - lo, np.float32(1e-3))
    amp = np.float32(fraction) * np.float32(np.linalg.norm(hi - lo))
    u = (p - lo) / ext
    moved = (p + amp * np.sin(np.float32(3.0 * np.pi) * u[:, [1, 2, 0]] + np.float32(phase) + np.arange(3, dtype=np.float32))).astype(np.float32)
    al = np.asarray(sd.tri_area_light) if sd.tri_area_light is not None else np.zeros(0, np.int32)
    lit = np.unique(np.asarray(sd.indices)[np.nonzero(al >= 0)[0]].reshape(-1)).astype(np.int64)
    moved[lit] = p[lit]
    return np.ascontiguousarray(moved)


def moved_scene(sd, points, normals=None):
    out = copy.copy(sd)
    out.points = points
    if normals is not None:
        out.normals = normals
    return out


def sphere_table(yk, sd):
    """(n_spheres, 6): every sphere's bound at creation, read off a tree with one shape per leaf (a leaf that holds one
    shape stores that shape's bound)."""
    if not len(sd.spheres):
        return np.zeros((0, 6), np.float32)
    one = copy.copy(sd)
    one.split_method, one.max_shapes_in_node, one.shape_order = abi.SPLIT_SAH, 1, None
    s = yk.Scene(None, one)
    nodes, order = s.export_bvh()
    s.close()
    leaf_of_slot = {int(n["a"]): n for n in nodes if n["is_leaf"] and n["count"] == 1}
    out = np.zeros((len(sd.spheres), 6), np.float32)
    for k in range(len(sd.spheres)):
        slot = int(np.nonzero(order == sd.n_triangles + k)[0][0])
        out[k, :3], out[k, 3:] = leaf_of_slot[slot]["bmin"], leaf_of_slot[slot]["bmax"]
    return out


def tree_state(s):
    i = s.info()
    nodes, order = s.export_bvh()
    return nodes.tobytes(), order.tobytes(), (i.n_nodes, i.n_interior, i.n_shapes, bytes(i.bounds_min), bytes(i.bounds_max), i.tree_depth, i.max_leaf_shapes)


CASES = [(m, k) for m in (abi.SPLIT_SAH, abi.SPLIT_MIDDLE, abi.SPLIT_EQUAL_COUNTS) for k in (1, 4)]


# ---- 1. identity
@pytest.mark.parametrize("name", list(SCENES))
def test_update_with_the_scenes_own_points_changes_nothing(yk, name):
    for method, max_shapes in CASES:
        sd = SCENES[name]()
        sd.split_method, sd.max_shapes_in_node = method, max_shapes
        s = yk.Scene(None, sd)
        before = tree_state(s)
        s.update(np.array(sd.points, dtype=np.float32))
        assert tree_state(s) == before, (method, max_shapes)
        i = s.update_info()
        assert (i.n_updates, i.route, i.reason) == (1, abi.UPDATE_ROUTE_HOST, 0)
        s.close()


# ---- 2. moved
@pytest.mark.parametrize("name", list(SCENES))
def test_moved_points_give_the_reference_refit(yk, name):
    table = sphere_table(yk, SCENES[name]())
    for method, max_shapes in CASES:
        sd = SCENES[name]()
        sd.split_method, sd.max_shapes_in_node = method, max_shapes
        s = yk.Scene(None, sd)
        nodes, order = s.export_bvh()
        moved = wobble(sd, 0.05)
        assert not np.array_equal(moved, sd.points)
        s.update(moved)
        got, got_order = s.export_bvh()
        want = refit_ref.refit(nodes, order, moved, sd.indices, table)
        assert got.tobytes() == want.tobytes(), (method, max_shapes)
        assert got.tobytes() != nodes.tobytes()
        for field in ("a", "count", "axis", "is_leaf"):
            assert np.array_equal(got[field], nodes[field]), field
        assert np.array_equal(got_order, order)
        i = s.info()
        assert bytes(i.bounds_min) == got["bmin"][0].tobytes() and bytes(i.bounds_max) == got["bmax"][0].tobytes()
        assert s.data is not sd and np.array_equal(s.data.points, moved)
        # the exported entry point on its own, and back again with the old points
        assert yk.refit_bvh(nodes, order, refit_ref.shape_bounds(moved, sd.indices, table)).tobytes() == want.tobytes()
        s.update(np.array(sd.points, dtype=np.float32))
        assert s.export_bvh()[0].tobytes() == nodes.tobytes()
        assert s.update_info().n_updates == 2
        s.close()


def test_refit_bvh_refuses_a_tree_that_does_not_fit(yk):
    sd = SCENES["city-tiny"]()
    s = yk.Scene(None, sd)
    nodes, order = s.export_bvh()
    s.close()
    sb = refit_ref.shape_bounds(sd.points, sd.indices)
    for broken in ("link", "slot", "shape", "short table"):
        n, o, b = nodes.copy(), order.copy(), sb
        if broken == "link":
            n["a"][0] = len(n)
        elif broken == "slot":
            n["a"][np.nonzero(n["is_leaf"])[0][-1]] = len(o)
        elif broken == "shape":
            o[3] = len(o)
        else:
            b = sb[:-1]
        with pytest.raises(_ffi.YukiError) as e:
            yk.refit_bvh(n, o, b)
        assert e.value.status == 1, broken


# ---- 3. refusals
def test_bad_arguments_are_refused_and_nothing_is_written(yk):
    sd = SCENES["city-tiny"]()  # normals on some meshes
    s = yk.Scene(None, sd)
    before = tree_state(s)
    moved = wobble(sd, 0.05)
    for value, message in ((np.nan, "points: coordinate not finite"), (np.inf, "points: coordinate not finite"), (-np.inf, "points: coordinate not finite")):
        bad = moved.copy()
        bad[len(bad) // 2, 1] = value
        with pytest.raises(_ffi.YukiError) as e:
            s.update(bad)
        assert e.value.status == 1 and str(e.value).endswith(message), str(e.value)
        assert tree_state(s) == before
    with pytest.raises(_ffi.YukiError) as e:
        s.update(None)
    assert e.value.status == 1 and str(e.value).endswith("null points")
    with pytest.raises(ValueError):
        s.update(moved[:-1])
    assert tree_state(s) == before and s.update_info().n_updates == 0
    s.close()
    bare = SCENES["signed-zeros"]()  # neither normals nor uvs
    assert bare.normals is None
    s = yk.Scene(None, bare)
    before = tree_state(s)
    with pytest.raises(_ffi.YukiError) as e:
        s.update(np.array(bare.points, dtype=np.float32), normals=np.zeros_like(bare.points, dtype=np.float32))
    assert e.value.status == 1 and str(e.value).endswith("normals given for a scene created without normals")
    assert tree_state(s) == before
    s.close()


# ---- 4. the inputs of the GPU tests
@pytest.mark.parametrize("name", list(TRACED))
@pytest.mark.parametrize("fraction", [0.01, 0.1])
def test_the_moved_geometry_stays_inside_the_traversal_caps(oracle, name, fraction):
    """Passes without the feature: the oracle's own scene of the moved data against the f64 brute force."""
    sd = TRACED[name]()
    msd = moved_scene(sd, wobble(sd, fraction))
    ref = trace_ref.TraceRef(msd)
    osc = oracle.OracleScene(msd)
    o, d = tr.random_rays(msd, 2048, SEED)
    w = osc.intersect(o, d, None)
    rob, hit = tr.check_closest(ref, "random", o, d, None, w["shape"], w["t"])
    diag = float(np.linalg.norm(msd.points.max(axis=0) - msd.points.min(axis=0)))
    tm = np.random.default_rng(SEED).uniform(0.0, 1.5 * diag, len(o)).astype(np.float32)
    al = np.full(len(o), -1, np.int32)
    arob = tr.check_any(ref, "random", o, d, tm, al, osc.any_intersect(o, d, tm, al))
    print(f"{name} moved by {fraction}: {rob.mean():.3f} robust closest-hit rays, {hit.mean():.3f} robust hits, {arob.mean():.3f} robust any-hit rays")
    assert rob.mean() >= 0.5 and arob.mean() >= 0.5
