"""The device scene layout ("scene_layout" = 1, yuki_amd/csrc/yk_scene_layout.hip) writes the bytes the host layout
writes: all seven device record buffers, the root ref, the tree-top sizes and the wide flags — from a device-built tree
in place and from an uploaded host-built one, for every "wide_bvh" / "top_nodes" setting; on every scene named here the
device path is taken (no fallback).  A device-built, device-laid scene fetches its host tree only when asked, and what
is rendered through it is what the default renders, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from yuki_amd import abi, scenes

from test_bvh_levels import _one_and_seven, _signed_zero_scene, _tree
from test_scene_layout_plan import _first_triangles, _seam_scene

pytestmark = pytest.mark.gpu
SEED = 0x73B9642E74AC471C


@pytest.fixture(scope="module")
def contexts(yk):
    """One context per option set, shared by the module."""
    made = {}

    def get(**options):
        key = tuple(sorted(options.items()))
        if key not in made:
            made[key] = yk.Context(0, **options)
        return made[key]

    yield get
    for c in made.values():
        c.close()


def _perm_scene():
    sd = scenes.by_name("city-tiny")
    sd.shape_order = np.random.default_rng(5).permutation(sd.n_triangles).astype(np.uint32)
    return sd


def _two_shapes():
    return _first_triangles(2, (0.0, 10.0))


SCENES = {
    "cornell": scenes.cornell,  # its sphere; uvs on some meshes
    "cornell-tris": lambda: scenes.by_name("cornell-tris"),
    "city-tiny": lambda: scenes.by_name("city-tiny"),  # normals on every second instance, uvs on the boxes
    "city-small": lambda: scenes.by_name("city-small"),
    "one-shape": lambda: _one_and_seven()[0],
    "two-shapes": _two_shapes,
    "signed-zeros": _signed_zero_scene,  # neither normals nor uvs: no prim_attr
    "city-tiny-permuted": _perm_scene,
    "coplanar-slabs": lambda: scenes.by_name("coplanar-slabs"),  # normals, no uvs
}


def _snapshot(yk, ctx, sd):
    s = yk.Scene(ctx, sd)
    li = s.layout_info()
    rec = {name: s.device_records(name).tobytes() for name in abi.RECORD_NAMES}
    head = (li.root_ref, li.n_top, li.n_top_any, li.wide, li.wide_auto)
    who = (li.layout, li.reason, s.build_info().builder, s.build_info().reason)
    s.close()
    return rec, head, who


def _assert_device_layout_equals_host(yk, contexts, sd, builder, **options):
    want, want_head, who = _snapshot(yk, contexts(**options), sd)
    assert who[:2] == (abi.LAYOUT_HOST, 0)
    got, got_head, who = _snapshot(yk, contexts(scene_layout=1, bvh_builder=builder, **options), sd)
    assert who[:2] == (abi.LAYOUT_DEVICE, 0), who  # the share of cases allowed to fall back is zero
    assert got_head == want_head
    for name in abi.RECORD_NAMES:
        assert len(got[name]) == len(want[name]), name
        assert got[name] == want[name], name
    return want, want_head, who


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("wide", [0, 1, 2])
def test_records_are_the_host_layouts(yk, contexts, name, wide):
    sd = SCENES[name]()
    for builder in (0, 1):
        want, head, who = _assert_device_layout_equals_host(yk, contexts, sd, builder, wide_bvh=wide)
        assert who[2] == builder and who[3] == 0
        leaf_root = name == "one-shape"
        assert head[3] == (0 if wide == 0 or leaf_root else 1) and head[4] == (1 if wide == 2 and not leaf_root else 0)
        assert (len(want["nodes4"]) > 0) == bool(head[3])
    if name == "signed-zeros":
        assert len(want["prim_attr"]) == 0
    if name in ("city-tiny", "coplanar-slabs", "cornell"):
        assert len(want["prim_attr"]) == 64 * (len(want["tris"]) // 48) > 0  # four 16-byte words a shape


@pytest.mark.parametrize("top_nodes", [0, 1, 3, None])
def test_every_tree_top_cap(yk, contexts, top_nodes):
    sd = scenes.by_name("city-tiny")
    options = {} if top_nodes is None else {"top_nodes": top_nodes}
    for builder in (0, 1):
        want, head, _ = _assert_device_layout_equals_host(yk, contexts, sd, builder, **options)
        if top_nodes is not None:
            assert head[1] == head[2] == top_nodes and len(want["top"]) == 64 * top_nodes
        else:
            assert head[1] > 3 and head[2] >= head[1]


@pytest.mark.parametrize("method,builder", [(abi.SPLIT_SAH, 0), (abi.SPLIT_SAH, 1), (abi.SPLIT_MIDDLE, 0), (abi.SPLIT_MIDDLE, 1), (abi.SPLIT_EQUAL_COUNTS, 0)])
@pytest.mark.parametrize("max_shapes", [1, 4])
def test_split_methods_and_leaf_sizes(yk, contexts, method, builder, max_shapes):
    for make in (SCENES["city-tiny"], SCENES["cornell"], SCENES["city-tiny-permuted"]):
        sd = make()
        sd.split_method, sd.max_shapes_in_node = method, max_shapes
        _assert_device_layout_equals_host(yk, contexts, sd, builder)


@pytest.mark.parametrize("k", [512, 513])
@pytest.mark.parametrize("method", [abi.SPLIT_SAH, abi.SPLIT_MIDDLE])
@pytest.mark.parametrize("max_shapes", [1, 4])
def test_scans_at_the_block_seam(yk, contexts, k, method, max_shapes):
    """1023 and 1025 nodes (255 and 257 at four shapes per leaf): the layout's two scans on either side of one block of 1024."""
    sd = _seam_scene(k)
    sd.split_method, sd.max_shapes_in_node = method, max_shapes
    for builder in (0, 1):
        for wide in (0, 2):
            want, head, who = _assert_device_layout_equals_host(yk, contexts, sd, builder, wide_bvh=wide)
            assert who[2:] == (builder, 0)
            assert len(want["nodes"]) // 64 == {(512, 1): 511, (513, 1): 512, (512, 4): 127, (513, 4): 128}[(k, max_shapes)]
            assert head[3] == (1 if wide else 0) and (len(want["nodes4"]) > 0) == bool(wide)


def test_equal_counts_with_the_device_builder_asked_for(yk, contexts):
    """The builder refuses EqualCounts; the layout then runs on the uploaded host tree."""
    sd = scenes.by_name("city-tiny")
    sd.split_method, sd.max_shapes_in_node = abi.SPLIT_EQUAL_COUNTS, 2
    _, _, who = _assert_device_layout_equals_host(yk, contexts, sd, 1)
    assert who[2:] == (0, 1)  # host recursion, YK_BVH_REASON_SPLIT_METHOD


def _line_of_triangles(n=128):
    """Triangles in the planes x = 2^-k: Middle halves the centroid range, which splits the one or two largest x off level
    after level (two while the smallest x vanishes in the rounding of lo + hi): 128 triangles give a tree 76 deep."""
    sd = scenes.deep_chain(n)
    xs = (2.0 ** -np.arange(n, dtype=np.float64)).astype(np.float32)
    sd.points = sd.points.copy()
    sd.points[:, 0] = np.repeat(xs, 3)
    sd.split_method, sd.max_shapes_in_node = abi.SPLIT_MIDDLE, 1
    return sd


def test_no_wide_layout_on_a_deep_tree(yk, contexts):
    sd = _line_of_triangles()
    assert yk.Scene(None, sd).info().tree_depth > 64
    for wide in (1, 2):
        for builder in (0, 1):
            want, head, _ = _assert_device_layout_equals_host(yk, contexts, sd, builder, wide_bvh=wide)
            assert len(want["nodes4"]) == 0 and head[3] == 0 and head[4] == 0


def test_the_host_tree_is_fetched_when_asked_for(yk, contexts):
    sd = scenes.by_name("city-small")
    ref_scene = yk.Scene(None, sd)
    ref = _tree(ref_scene)
    # export
    s = yk.Scene(contexts(scene_layout=1, bvh_builder=1), sd)
    assert (s.layout_info().layout, s.build_info().builder) == (abi.LAYOUT_DEVICE, 1)
    assert s.layout_info().tree_fetched == 0
    i, r = s.info(), ref_scene.info()
    assert (i.n_nodes, i.n_interior, i.n_shapes, i.max_leaf_shapes, i.tree_depth) == (r.n_nodes, r.n_interior, r.n_shapes, r.max_leaf_shapes, r.tree_depth)
    assert bytes(i.bounds_min) == bytes(r.bounds_min) and bytes(i.bounds_max) == bytes(r.bounds_max)
    assert s.layout_info().tree_fetched == 0  # the scalars need no arrays
    assert _tree(s) == ref
    assert s.layout_info().tree_fetched == 1
    s.close()
    # node_bounds
    s = yk.Scene(contexts(scene_layout=1, bvh_builder=1), sd)
    assert s.layout_info().tree_fetched == 0
    for level in (2, -1):
        assert np.array_equal(s.node_bounds(level).view(np.uint32), ref_scene.node_bounds(level).view(np.uint32))
    assert s.layout_info().tree_fetched == 1
    s.close()
    # a stage call in the render loop's flavour maps its hit words through the shape order
    c = contexts(scene_layout=1, bvh_builder=1, trace_stage_kernel=1)
    s = yk.Scene(c, sd)
    assert s.layout_info().tree_fetched == 0
    fs = yk.FilmSettings(res=(32, 18), tile_dim=16)
    o, d = yk.camera_rays(c, yk.Camera(sd.camera, fs), yk.SamplerType.Uniform(1, SEED), (0, 0, 32, 18), 0)
    shape = np.zeros(len(o), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    yk.check(yk.lib().yk_trace_closest(c.h, s.h, len(o), p(o), p(d), None, p(shape), None, None, None, None, None), c.h)
    assert s.layout_info().tree_fetched == 1
    plain = yk.Scene(contexts(), sd)
    assert np.array_equal(shape, plain.intersect(o, d)["shape"]) and (shape >= 0).any()
    plain.close()
    s.close()
    # a host-built tree is there from the start
    s = yk.Scene(contexts(scene_layout=1), sd)
    assert (s.layout_info().layout, s.layout_info().tree_fetched) == (abi.LAYOUT_DEVICE, 1)
    s.close()


@pytest.mark.parametrize("wide", [0, 2])
def test_render_through_a_device_laid_scene(yk, wide):
    """city-small, Path 6, both samplers, one tile list: (builder, layout) = (1, 1) renders what (0, 0) renders."""
    sd = scenes.by_name("city-small")
    fs = yk.FilmSettings(res=(160, 90), tile_dim=16)
    cam, tiles = yk.Camera(sd.camera, fs), yk.film_tiles(fs)
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=6))
    images, debug = {}, {}
    for mode in (0, 1):
        c = yk.Context(0, wide_bvh=wide, bvh_builder=mode, scene_layout=mode)
        sc = yk.Scene(c, sd)
        assert sc.layout_info().layout == mode and sc.layout_info().reason == 0 and sc.build_info().builder == mode
        inst = yk.IntegratorType.instantiate(c, integ)
        for k, sampler in enumerate((yk.SamplerType.Uniform(4, SEED), yk.SamplerType.Stratified((2, 2), True, SEED))):
            px, st = inst.render_tiles(sc, cam, sampler, tiles)
            images[(mode, k)] = (np.ascontiguousarray(px, dtype=np.float32).view(np.uint32).copy(), st.rays)
        sampler = yk.SamplerType.Uniform(4, SEED)
        o, d = yk.camera_rays(c, cam, sampler, (72, 40, 88, 56), 1)
        pix = np.array([(x, y) for y in range(40, 56) for x in range(72, 88)], dtype=np.uint16)
        li, counts, rays = inst.li_debug(sc, sampler, o, d, pix, np.ones(len(o), dtype=np.uint32))
        debug[mode] = (li.view(np.uint32).copy(), counts.copy(), [r.tobytes() for r in rays])
        assert sc.layout_info().tree_fetched == (1 if mode == 0 else 0)  # rendering needs no host tree
        sc.close()
        c.close()
    for k in (0, 1):
        assert images[(0, k)][1] == images[(1, k)][1]
        assert np.array_equal(images[(0, k)][0], images[(1, k)][0])
    assert np.array_equal(debug[0][0], debug[1][0]) and np.array_equal(debug[0][1], debug[1][1]) and debug[0][2] == debug[1][2]
    assert debug[0][1].sum() > 0


def test_the_default_is_the_host_layout(yk, contexts):
    s = yk.Scene(contexts(), scenes.by_name("city-tiny"))
    li = s.layout_info()
    assert (li.layout, li.reason, li.tree_fetched) == (abi.LAYOUT_HOST, 0, 1)
    assert (li.seconds_upload, li.seconds_layout) == (0.0, 0.0)
    s.close()
    assert yk.lib().yk_sizeof(17) == C.sizeof(abi.SceneLayoutInfo) == 48


def test_cfg3_at_full_size(yk, contexts, cfg3_scene):
    """2,035,599 nodes: the one case whose scans need more than 1024 blocks, so that the scan of the block sums loops."""
    assert (cfg3_scene.split_method, cfg3_scene.max_shapes_in_node) == (abi.SPLIT_SAH, 1)
    want, head, _ = _assert_device_layout_equals_host(yk, contexts, cfg3_scene, 1)
    assert len(want["nodes"]) // 64 == (2035599 - 1) // 2 and len(want["nodes4"]) > 0 and head[1] > 0
