"""The level-synchronous BVH builder (yuki_amd/csrc/yk_bvh_build.h), host instance: the algorithm the
device builder runs, proven without a GPU.  Its tree is the host recursion's and the oracle's
sequential builder's — same 32-byte nodes in the same depth-first order, same shape order, same
counts and depth — for every small-range limit S, with signed zeros, and where it refuses it says
why and the recursion's tree is what the scene holds."""
import ctypes as C

import numpy as np
import pytest

from yuki_amd import _ffi, abi, scenes

HOST, DEVICE, HOST_LEVELS = 0, 1, 2
REASON_SPLIT_METHOD, REASON_NON_FINITE, REASON_SELECT_NTH = 1, 2, 3

SCENES = {
    "cornell-tris": lambda: scenes.by_name("cornell-tris"),
    "city-tiny": lambda: scenes.by_name("city-tiny"),
    "city-small": lambda: scenes.by_name("city-small"),
    "cfg2": lambda: scenes.by_name("cfg2"),
    "city-12x10": lambda: scenes.city((12, 10), 3, 1, "mixed"),
}
# (nodes, depth) of the host recursion, from the issue's table: SAH 1 per leaf, SAH 4 per leaf, Middle 1 per leaf
TABLE = {
    "cornell-tris": {(abi.SPLIT_SAH, 1): (37, 7), (abi.SPLIT_SAH, 4): (21, 6), (abi.SPLIT_MIDDLE, 1): (37, 9)},
    "city-tiny": {(abi.SPLIT_SAH, 1): (921, 13), (abi.SPLIT_SAH, 4): (331, 11), (abi.SPLIT_MIDDLE, 1): (971, 17)},
    "city-small": {(abi.SPLIT_SAH, 1): (15081, 18), (abi.SPLIT_SAH, 4): (4913, 16), (abi.SPLIT_MIDDLE, 1): (15371, 21)},
    "cfg2": {(abi.SPLIT_SAH, 1): (138279, 21), (abi.SPLIT_SAH, 4): (40391, 18), (abi.SPLIT_MIDDLE, 1): (138405, 22)},
    "city-12x10": {(abi.SPLIT_SAH, 1): (305371, 23), (abi.SPLIT_SAH, 4): (96979, 20), (abi.SPLIT_MIDDLE, 1): (307211, 26)},
}


def _tree(scene):
    n, o = scene.export_bvh()
    i = scene.info()
    return n.tobytes(), o.tobytes(), (int(i.n_nodes), int(i.n_interior), int(i.n_shapes), int(i.max_leaf_shapes), int(i.tree_depth))


def _recursion(yk, sd, monkeypatch):
    monkeypatch.delenv("YK_BVH_BUILDER", raising=False)
    s = yk.Scene(None, sd)
    assert s.build_info().builder == HOST and s.build_info().reason == 0
    return s


def _levels(yk, sd, monkeypatch, small_range=None):
    monkeypatch.setenv("YK_BVH_BUILDER", "levels")
    if small_range is None:
        monkeypatch.delenv("YK_BVH_SMALL_RANGE", raising=False)
    else:
        monkeypatch.setenv("YK_BVH_SMALL_RANGE", str(small_range))
    try:
        return yk.Scene(None, sd)
    finally:
        monkeypatch.delenv("YK_BVH_BUILDER", raising=False)


def _assert_same(a, b):
    assert a[2] == b[2]
    assert a[0] == b[0], "nodes differ"
    assert a[1] == b[1], "shape order differs"


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("method", [abi.SPLIT_SAH, abi.SPLIT_MIDDLE])
@pytest.mark.parametrize("max_shapes", [1, 4])
def test_levels_tree_is_the_recursions_and_the_oracles(yk, oracle, monkeypatch, name, method, max_shapes):
    sd = SCENES[name]()
    sd.split_method, sd.max_shapes_in_node = method, max_shapes
    ref = _tree(_recursion(yk, sd, monkeypatch))
    n2, o2 = oracle.OracleScene(sd).export_bvh()
    s = _levels(yk, sd, monkeypatch)
    bi = s.build_info()
    assert bi.builder == HOST_LEVELS and bi.reason == 0 and bi.levels > 0
    got = _tree(s)
    _assert_same(got, ref)
    assert got[0] == n2.tobytes() and got[1] == o2.tobytes()
    if (method, max_shapes) in TABLE[name]:
        assert (got[2][0], got[2][4]) == TABLE[name][(method, max_shapes)]


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("method,max_shapes", [(abi.SPLIT_SAH, 1), (abi.SPLIT_SAH, 4), (abi.SPLIT_MIDDLE, 1), (abi.SPLIT_MIDDLE, 4)])
def test_every_small_range_limit_builds_the_same_tree(yk, monkeypatch, name, method, max_shapes):
    """S = 0: the level phase is the whole build (and the 2-shape equal-counts fallbacks run on one lane of it);
    S larger than the scene: one small-range job is the whole build; 2 and 64: the seam between the two."""
    sd = SCENES[name]()
    sd.split_method, sd.max_shapes_in_node = method, max_shapes
    ref = _tree(_recursion(yk, sd, monkeypatch))
    for small_range in (0, 2, 64, sd.n_triangles + 1):
        s = _levels(yk, sd, monkeypatch, small_range)
        bi = s.build_info()
        assert (bi.builder, bi.reason, bi.small_range) == (HOST_LEVELS, 0, small_range), small_range
        if small_range == 0:
            assert bi.small_ranges == 0 and bi.levels == ref[2][4]  # one level per depth
        if small_range > sd.n_triangles:
            assert bi.small_ranges == 1 and bi.levels == 0
        _assert_same(_tree(s), ref)


def _one_and_seven():
    base = scenes.by_name("city-tiny")
    out = []
    for k in (1, 7):
        out.append(scenes.SceneData(points=base.points[:3].copy(), indices=np.array([[0, 1, 2]] * k, dtype=np.uint32), tri_mesh=np.zeros(k, np.uint32), tri_material=np.zeros(k, np.int32),
                                    tri_area_light=np.full(k, -1, np.int32), meshes=[(False, False, False)], materials=base.materials[:1], lights=base.lights, camera=base.camera))
    return out


@pytest.mark.parametrize("small_range", [0, 2, 32])
@pytest.mark.parametrize("method", [abi.SPLIT_SAH, abi.SPLIT_MIDDLE])
def test_degenerate_and_special_scenes(yk, oracle, monkeypatch, method, small_range):
    one, dup = _one_and_seven()
    perm = scenes.by_name("city-tiny")
    perm.shape_order = np.random.default_rng(5).permutation(perm.n_triangles).astype(np.uint32)
    for sd in (one, dup, scenes.cornell(), perm):
        sd.split_method = method
        ref = _tree(_recursion(yk, sd, monkeypatch))
        s = _levels(yk, sd, monkeypatch, small_range)
        assert s.build_info().builder == HOST_LEVELS and s.build_info().reason == 0
        got = _tree(s)
        _assert_same(got, ref)
        n2, o2 = oracle.OracleScene(sd).export_bvh()
        assert got[0] == n2.tobytes() and got[1] == o2.tobytes()
    assert _tree(_levels(yk, dup, monkeypatch, small_range))[2][:2] == (1, 0)  # seven duplicates: one leaf


def _signed_zero_scene():
    """Quads standing on the plane x = 0, on either side of it, whose vertices spell the zero as +0.0 in some
    triangles and -0.0 in others.  In index order a +0.0 comes first among the minima (the fold keeps it, a numeric
    minimum would return -0.0) and a -0.0 first among the maxima (the fold keeps it, a numeric maximum gives +0.0)."""
    base = scenes.by_name("city-tiny")
    pts, idx = [], []
    for k in range(48):
        right = k < 24  # the triangle spans x in [0, 1] or, in a group of its own further up, x in [-1, 0]
        y = 0.25 * k + (0.0 if right else 100.0)
        zero = (0.0 if k % 3 != 2 else -0.0) if right else (-0.0 if k % 3 != 2 else 0.0)
        far = 1.0 if right else -1.0
        b = len(pts)
        pts += [(zero, y, 0.0), (far, y + 0.2, 0.0), (zero, y + 0.1, 0.3 + 0.01 * (k % 5))]
        idx.append((b, b + 1, b + 2))
    n = len(idx)
    return scenes.SceneData(points=np.array(pts, dtype=np.float32), indices=np.array(idx, dtype=np.uint32), tri_mesh=np.zeros(n, np.uint32), tri_material=np.zeros(n, np.int32),
                            tri_area_light=np.full(n, -1, np.int32), meshes=[(False, False, False)], materials=base.materials[:1], lights=base.lights, camera=base.camera)


@pytest.mark.parametrize("small_range", [0, 2, 32, 1000])
@pytest.mark.parametrize("method", [abi.SPLIT_SAH, abi.SPLIT_MIDDLE])
@pytest.mark.parametrize("max_shapes", [1, 4, 8])
def test_signed_zeros_keep_the_folds_bits(yk, oracle, monkeypatch, method, max_shapes, small_range):
    sd = _signed_zero_scene()
    sd.split_method, sd.max_shapes_in_node = method, max_shapes
    ref = _tree(_recursion(yk, sd, monkeypatch))
    nodes, order = _recursion(yk, sd, monkeypatch).export_bvh()
    if max_shapes == 1:  # both zeros are stored, below and above
        lo, hi = nodes["bmin"][:, 0].copy().view(np.uint32), nodes["bmax"][:, 0].copy().view(np.uint32)
        assert (lo == 0x80000000).any() and (lo == 0).any() and (hi == 0x80000000).any() and (hi == 0).any()
    else:  # some leaf folds shapes that spell the zero both ways: there the order of the fold decides the stored bits
        zero_bits = sd.points[sd.indices[:, 0], 0].copy().view(np.uint32)
        leaves = nodes[nodes["is_leaf"] == 1]
        assert any(len(set(zero_bits[order[int(l["a"]) : int(l["a"]) + int(l["count"])]].tolist())) == 2 for l in leaves)
    got = _tree(_levels(yk, sd, monkeypatch, small_range))
    _assert_same(got, ref)
    n2, o2 = oracle.OracleScene(sd).export_bvh()
    assert got[0] == n2.tobytes() and got[1] == o2.tobytes()


def test_equal_counts_is_refused_with_its_reason(yk, monkeypatch):
    sd = scenes.by_name("city-tiny")
    sd.split_method, sd.max_shapes_in_node = abi.SPLIT_EQUAL_COUNTS, 2
    ref = _tree(_recursion(yk, sd, monkeypatch))
    s = _levels(yk, sd, monkeypatch)
    assert (s.build_info().builder, s.build_info().reason) == (HOST, REASON_SPLIT_METHOD)
    _assert_same(_tree(s), ref)


def test_non_finite_vertex_changes_nothing(yk, monkeypatch):
    """Whatever the recursion answers for a non-finite bound — a tree or YK_ERR_BVH_BUILD — asking for the level builder
    gives the same answer; where a tree results the build info carries the reason."""
    for bad in (np.inf, -np.inf, np.nan):
        sd = scenes.by_name("city-tiny")
        sd.points = sd.points.copy()
        sd.points[int(sd.indices[5, 1]), 1] = bad

        def outcome(make):
            try:
                s = make()
            except yk.YukiError as e:
                return ("error", e.status), None
            return _tree(s), s

        ref, _ = outcome(lambda: _recursion(yk, sd, monkeypatch))
        got, s = outcome(lambda: _levels(yk, sd, monkeypatch))
        assert got == ref
        if s is not None:  # a NaN coordinate is dropped by Triangle::world_bound's min / max: that shape's bound stays finite
            assert (s.build_info().builder, s.build_info().reason) == ((HOST_LEVELS, 0) if bad != bad else (HOST, REASON_NON_FINITE))


def _two_adjacent_centroids(n):
    """Flat triangles at x = 1 and at the next float above it, alike in y and z: the split axis is x, the Middle
    value (lo + hi) / 2 rounds onto lo, nothing passes `c < mid` and the partition leaves one side empty."""
    base = scenes.by_name("city-tiny")
    x0, x1 = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    pts, idx = [], []
    for k in range(n):
        x = x0 if (k * 7) % 3 else x1
        b = len(pts)
        pts += [(x, 0.0, 0.0), (x, 1.0, 0.0), (x, 0.0, 1.0)]
        idx.append((b, b + 1, b + 2))
    return scenes.SceneData(points=np.array(pts, dtype=np.float32), indices=np.array(idx, dtype=np.uint32), tri_mesh=np.zeros(n, np.uint32), tri_material=np.zeros(n, np.int32),
                            tri_area_light=np.full(n, -1, np.int32), meshes=[(False, False, False)], materials=base.materials[:1], lights=base.lights, camera=base.camera)


def test_select_nth_on_a_long_range_is_refused_with_its_reason(yk, oracle, monkeypatch):
    sd = _two_adjacent_centroids(40)
    sd.split_method, sd.max_shapes_in_node = abi.SPLIT_MIDDLE, 1
    ref = _tree(_recursion(yk, sd, monkeypatch))
    assert ref[2][0] > 1  # the recursion's equal-counts fallback did split
    for small_range in (0, 4, 39):  # 40 shapes > max(S, 2): the level phase meets the fallback and gives up
        s = _levels(yk, sd, monkeypatch, small_range)
        assert (s.build_info().builder, s.build_info().reason) == (HOST, REASON_SELECT_NTH), small_range
        _assert_same(_tree(s), ref)
    s = _levels(yk, sd, monkeypatch, 40)  # within the small-range limit one lane runs select_nth: no refusal
    assert (s.build_info().builder, s.build_info().reason) == (HOST_LEVELS, 0)
    _assert_same(_tree(s), ref)


def _two_ended_partition(order, passes):
    """itertools::partition, the loop of swap_partition; the predicate travels with the element."""
    a = list(zip(order, passes))
    count, front, back = 0, 0, len(a)
    while front < back:
        f = front
        front += 1
        if not a[f][1]:
            swapped = False
            while front < back:
                back -= 1
                if a[back][1]:
                    a[f], a[back] = a[back], a[f]
                    swapped = True
                    break
            if not swapped:
                return count, [x for x, _ in a]
        count += 1
    return count, [x for x, _ in a]


def test_partition_step_is_the_two_ended_swap_partition(yk):
    L = yk.lib()
    rng = np.random.default_rng(11)
    cases = [np.ones(1, np.uint8), np.zeros(1, np.uint8), np.ones(17, np.uint8), np.zeros(17, np.uint8), np.array([0, 1], np.uint8), np.array([1, 0], np.uint8)]
    for n in list(range(2, 40)) + [63, 64, 65, 511, 512, 513, 4097]:
        for p in (0.05, 0.5, 0.95):
            cases.append((rng.random(n) < p).astype(np.uint8))
    for passes in cases:
        order = rng.permutation(len(passes)).astype(np.uint32)
        want_count, want = _two_ended_partition(order.tolist(), passes.tolist())
        got = order.copy()
        count = L.yk_bvh_partition_plan(passes.ctypes.data_as(C.c_void_p), len(passes), got.ctypes.data_as(C.c_void_p))
        assert count == want_count == int(passes.sum())
        assert got.tolist() == want, passes.tolist()


def test_build_info_abi(yk):
    assert yk.lib().yk_sizeof(15) == C.sizeof(_ffi.BvhBuildInfo) == 64
