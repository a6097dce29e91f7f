"""Scene.from_device / yk_scene_create_device (yuki_amd/csrc/yk_scene_input.hip): a scene made from torch tensors on the
device is the scene yk_scene_create makes from the same arrays on the host with the device builder and the device layout
asked for — records, infos, exported tree and rendered bits — on every small scene of the layout test, on either side of a
scan block (512 / 513 shapes) and of a block of the check kernel (255 / 256 / 257 triangles).  Bad indices are refused with
yk_scene_create's message before anything follows them; the arrays are copied; a side stream is waited for; the host copy of
the tree and of the shape kinds is fetched when asked; a refusing builder falls back silently."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from yuki_amd import _ffi, abi, scenes

from test_gpu_scene_layout import SCENES as LAYOUT_SCENES
from test_gpu_scene_layout import SEED
from test_scene_layout_plan import _seam_scene

pytestmark = pytest.mark.gpu

SCENES = {name: LAYOUT_SCENES[name] for name in ("one-shape", "two-shapes", "cornell", "city-tiny", "city-tiny-permuted", "signed-zeros", "coplanar-slabs")}
SCENES.update({"seam-512": lambda: _seam_scene(512), "seam-513": lambda: _seam_scene(513)})  # a scan block's seam
SCENES.update({f"strip-{k}": (lambda k=k: _seam_scene(k)) for k in (255, 256, 257)})  # the check kernel's block of 256

UNSIGNED = ("indices", "tri_mesh", "shape_order")


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


def _tensors(sd, **replaced):
    """The large arrays of `sd` as tensors on the device (unsigned ones by their bits: torch's int32)."""
    out = {}
    for name, dtype in (("points", np.float32), ("normals", np.float32), ("uvs", np.float32), ("indices", np.uint32), ("tri_mesh", np.uint32), ("tri_material", np.int32), ("tri_area_light", np.int32),
                        ("shape_order", np.uint32)):
        a = replaced.get(name, getattr(sd, name))
        if a is not None:
            a = np.ascontiguousarray(a, dtype=dtype)
            out[name] = torch.from_numpy(a.view(np.int32) if name in UNSIGNED else a).to("cuda:0")
    return out


def _snapshot(s):
    li, bi, i = s.layout_info(), s.build_info(), s.info()
    fetched = li.tree_fetched
    nodes, order = s.export_bvh()
    return dict(records={name: s.device_records(name).tobytes() for name in abi.RECORD_NAMES}, head=(li.root_ref, li.n_top, li.n_top_any, li.wide, li.wide_auto),
                info=(i.n_nodes, i.n_interior, i.n_shapes, bytes(i.bounds_min), bytes(i.bounds_max), i.tree_depth, i.max_leaf_shapes), tree=(nodes.tobytes(), order.tobytes()),
                who=(bi.builder, bi.reason, li.layout, li.reason), fetched_before_export=fetched)


def _assert_same_scene(got, want):
    for name in abi.RECORD_NAMES:
        assert len(got["records"][name]) == len(want["records"][name]), name
        assert got["records"][name] == want["records"][name], name
    for key in ("head", "info", "tree", "who"):
        assert got[key] == want[key], key


def _both(yk, contexts, sd, arrays=None, stream=None, **options):
    """The scene from host arrays (device builder and layout asked for) and from device tensors (nothing asked for)."""
    host = yk.Scene(contexts(bvh_builder=1, scene_layout=1, **options), sd)
    want = _snapshot(host)
    host.close()
    dev = yk.Scene.from_device(contexts(**options), sd, _tensors(sd) if arrays is None else arrays, stream=stream)
    got = _snapshot(dev)
    dev.close()
    return got, want


# ---- 1. the same scene, byte for byte
@pytest.mark.parametrize("name", list(SCENES))
def test_the_scene_is_the_host_input_scene(yk, contexts, name):
    for method in (abi.SPLIT_SAH, abi.SPLIT_MIDDLE):
        for max_shapes in (1, 4):
            for wide in (0, 2):
                sd = SCENES[name]()
                sd.split_method, sd.max_shapes_in_node = method, max_shapes
                got, want = _both(yk, contexts, sd, wide_bvh=wide)
                _assert_same_scene(got, want)
                assert got["who"] == (1, 0, abi.LAYOUT_DEVICE, 0), (method, max_shapes, wide)  # nothing may fall back here
                assert got["fetched_before_export"] == 0


# ---- 2, 3. the same image; the arrays are copied
def _render_tile(yk, ctx, scene, sd):
    fs = yk.FilmSettings(res=(32, 32), tile_dim=32)
    integ = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=8)))
    px, stats = integ.render_tiles(scene, yk.Camera(sd.camera, fs), yk.SamplerType.Stratified((2, 2), True, SEED), yk.film_tiles(fs))
    return np.ascontiguousarray(px, dtype=np.float32).view(np.uint32).copy(), stats.rays


@pytest.fixture(scope="module")
def reference_tiles(yk, contexts):
    """The 32x32 tile of cornell and city-tiny through the host-input scene, rendered once."""
    out = {}
    for name in ("cornell", "city-tiny"):
        sd = SCENES[name]()
        c = contexts(bvh_builder=1, scene_layout=1)
        s = yk.Scene(c, sd)
        out[name] = _render_tile(yk, c, s, sd)
        s.close()
        assert out[name][1] >= 32 * 32 * 4 and out[name][0].any()
    return out


@pytest.mark.parametrize("name", ["cornell", "city-tiny"])
def test_the_image_is_the_same_and_the_arrays_are_copied(yk, contexts, reference_tiles, name):
    sd = SCENES[name]()
    c = contexts()
    arrays = _tensors(sd)
    s = yk.Scene.from_device(c, sd, arrays)
    bits, rays = _render_tile(yk, c, s, sd)
    assert rays == reference_tiles[name][1] and np.array_equal(bits, reference_tiles[name][0])
    for t in arrays.values():  # the scene keeps nothing of the caller's
        t.zero_()
    torch.cuda.synchronize()
    bits, rays = _render_tile(yk, c, s, sd)
    assert rays == reference_tiles[name][1] and np.array_equal(bits, reference_tiles[name][0])
    s.close()


# ---- 4. stream order
def test_arrays_produced_on_a_side_stream(yk, contexts):
    sd = SCENES["city-tiny"]()
    arrays = _tensors(sd)
    half = (arrays["points"] * 0.5).contiguous()  # x / 2 + x / 2 == x in float32 for every normal x
    assert torch.equal(half + half, arrays["points"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        busy = torch.ones((2048, 2048), device="cuda:0")
        for _ in range(8):  # work in front of the points on their stream
            busy = busy @ busy * (1.0 / 2048.0)
        arrays["points"] = half + half
    got, want = _both(yk, contexts, sd, arrays=arrays, stream=side)
    _assert_same_scene(got, want)
    assert float(busy[0, 0]) == 1.0


# ---- 5. validation
def _bad_inputs():
    """name -> (field, array) for city-tiny with one violation, or two where the order of the messages is the point."""
    sd = scenes.by_name("city-tiny")
    nt, nv = sd.n_triangles, len(sd.points)
    n_lights, n_materials, n_meshes = len(sd.lights), len(sd.materials), len(sd.meshes)
    point_light = [k for k, l in enumerate(sd.lights) if l["kind"] != "rect"]
    assert point_light and nt > 400

    def changed(field, edits, dtype):
        a = np.array(getattr(sd, field), dtype=dtype).copy()
        for where, value in edits:
            a[where] = value
        return field, a

    cases = {
        "vertex-first": changed("indices", [((0, 2), nv)], np.uint32),
        "vertex-middle": changed("indices", [((nt // 2, 0), nv)], np.uint32),
        "vertex-last": changed("indices", [((nt - 1, 1), nv)], np.uint32),
        "mesh": changed("tri_mesh", [(nt // 3, n_meshes)], np.uint32),
        "material-negative": changed("tri_material", [(300, -1)], np.int32),
        "material-count": changed("tri_material", [(nt - 1, n_materials)], np.int32),
        "light-count": changed("tri_area_light", [(5, n_lights)], np.int32),
        "light-not-rectangular": changed("tri_area_light", [(257, point_light[0])], np.int32),
        "light-minus-two": changed("tri_area_light", [(nt - 2, -2)], np.int32),
        "order-duplicate": ("shape_order", np.concatenate([np.arange(nt - 1), [7]]).astype(np.uint32)),
        "order-out-of-range": ("shape_order", np.concatenate([[nt], np.arange(1, nt)]).astype(np.uint32)),
    }
    return sd, cases


@pytest.mark.parametrize("case", list(_bad_inputs()[1]))
def test_bad_input_is_refused_with_the_host_message(yk, contexts, reference_tiles, case):
    sd, cases = _bad_inputs()
    field, array = cases[case]
    bad = copy.copy(sd)
    setattr(bad, field, array)
    c = contexts()
    with pytest.raises(_ffi.YukiError) as host:
        yk.Scene(c, bad)
    with pytest.raises(_ffi.YukiError) as dev:
        yk.Scene.from_device(c, bad, _tensors(bad))
    assert dev.value.status == host.value.status == 1
    assert str(dev.value) == str(host.value)
    expected = {"vertex": "vertex index out of range", "mesh": "mesh index out of range", "material": "material index out of range", "light-count": "light index out of range",
                "light-not": "tri_area_light must be -1 or index a rectangular light", "light-minus": "tri_area_light must be -1 or index a rectangular light",
                "order": "shape_order is not a permutation of the shapes"}
    assert [m for k, m in expected.items() if case.startswith(k)] == [str(dev.value).split(": ", 1)[1]]
    good = yk.Scene.from_device(c, sd, _tensors(sd))  # the context is as good as before
    bits, rays = _render_tile(yk, c, good, sd)
    assert rays == reference_tiles["city-tiny"][1] and np.array_equal(bits, reference_tiles["city-tiny"][0])
    good.close()


def test_the_lowest_triangle_decides_the_message(yk, contexts):
    """A bad material in triangle 10 and a bad vertex index in triangle 400 (another block): the host loop stops at 10."""
    sd = scenes.by_name("city-tiny")
    bad = copy.copy(sd)
    bad.indices = np.array(sd.indices, dtype=np.uint32).copy()
    bad.indices[400, 1] = len(sd.points) + 5
    bad.tri_material = np.array(sd.tri_material, dtype=np.int32).copy()
    bad.tri_material[10] = len(sd.materials)
    c = contexts()
    messages = []
    for make in (lambda: yk.Scene(c, bad), lambda: yk.Scene.from_device(c, bad, _tensors(bad))):
        with pytest.raises(_ffi.YukiError) as e:
            make()
        messages.append(str(e.value))
    assert messages[0] == messages[1] and messages[1].endswith("material index out of range")
    # two bad vertex indices, in the first and in the last triangle; and a bad light range before a bad light kind
    bad = copy.copy(sd)
    bad.indices = np.array(sd.indices, dtype=np.uint32).copy()
    bad.indices[0, 0] = bad.indices[-1, 2] = 0xFFFFFFFF
    bad.tri_area_light = np.array(sd.tri_area_light, dtype=np.int32).copy()
    bad.tri_area_light[3] = -7
    with pytest.raises(_ffi.YukiError, match="vertex index out of range"):
        yk.Scene.from_device(c, bad, _tensors(bad))


# ---- 6. wrong memory
def test_host_memory_is_refused(yk, contexts):
    sd = scenes.by_name("city-tiny")
    c = contexts()
    arrays = _tensors(sd)
    points = np.ascontiguousarray(sd.points, dtype=np.float32)
    arrays["points"] = int(points.ctypes.data)
    with pytest.raises(_ffi.YukiError) as e:
        yk.Scene.from_device(c, sd, arrays)
    assert e.value.status == 1 and str(e.value).endswith("points is not device memory of this context's device")
    got, want = _both(yk, contexts, sd)
    _assert_same_scene(got, want)


# ---- 7. fallbacks
def test_equal_counts_falls_back_to_the_host_builder(yk, contexts):
    sd = scenes.by_name("city-tiny")
    sd.split_method, sd.max_shapes_in_node = abi.SPLIT_EQUAL_COUNTS, 2
    got, want = _both(yk, contexts, sd)
    _assert_same_scene(got, want)
    assert got["who"] == (0, 1, abi.LAYOUT_DEVICE, 0)  # host recursion, YK_BVH_REASON_SPLIT_METHOD; the layout still on the device


def test_the_fallback_leaves_the_contexts_options_alone(yk):
    """The fallback asks the host path for the device layout (and, where the builder did not refuse, the device builder) as
    an argument: the context's "bvh_builder" and "scene_layout" stay 0 for the scene created next."""
    ctx = yk.Context(0)
    try:
        sd = scenes.by_name("city-tiny")
        sd.split_method, sd.max_shapes_in_node = abi.SPLIT_EQUAL_COUNTS, 2
        s = yk.Scene.from_device(ctx, sd, _tensors(sd))
        bi, li = s.build_info(), s.layout_info()
        assert (bi.builder, bi.reason, li.layout, li.reason) == (0, 1, abi.LAYOUT_DEVICE, 0)  # it fell back: the host recursion, the device layout
        s.close()
        sah = scenes.by_name("city-tiny")
        sah.split_method = abi.SPLIT_SAH
        t = yk.Scene(ctx, sah)
        assert t.layout_info().layout == abi.LAYOUT_HOST
        assert _ffi.BVH_BUILDER_NAMES[t.build_info().builder] == "host recursion"
        t.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_non_finite_coordinate_falls_back(yk, contexts, value):
    """One coordinate of one vertex of city-tiny made NaN, and +inf: reason NON_FINITE, and the host-input scene's records,
    infos and exported tree.  Triangle::world_bound folds with f32::min / max, which drop a NaN operand, so the NaN leaves a
    finite bound that the builder's own test cannot see (from host arrays the device builder accepts that scene: same tree);
    the input stage looks at the coordinates themselves and sends such geometry to the host recursion."""
    sd = scenes.by_name("city-tiny")
    sd.points = np.array(sd.points, dtype=np.float32).copy()
    sd.points[int(np.asarray(sd.indices)[40, 1]), 1] = value
    got, want = _both(yk, contexts, sd)
    print(f"value {value}: device input (builder, reason, layout, reason) = {got['who']}, host input = {want['who']}")
    assert got["who"] == (0, 2, abi.LAYOUT_DEVICE, 0)  # host recursion, YK_BVH_REASON_NON_FINITE; the layout still on the device
    got["who"] = want["who"]  # the tree is the same whoever built it
    _assert_same_scene(got, want)


# ---- 8. lazy host data
def test_host_copies_are_fetched_when_asked_for(yk, contexts):
    sd = scenes.by_name("city-tiny")
    c = contexts()
    for ask in (lambda s: s.export_bvh(), lambda s: s.node_bounds(-1)):
        s = yk.Scene.from_device(c, sd, _tensors(sd))
        assert s.layout_info().tree_fetched == 0
        s.info(), s.build_info(), s.device_records("nodes")
        assert s.layout_info().tree_fetched == 0
        ask(s)
        assert s.layout_info().tree_fetched == 1
        s.close()
    c = contexts(trace_stage_kernel=1)
    fs = yk.FilmSettings(res=(32, 18), tile_dim=16)
    o, d = yk.camera_rays(c, yk.Camera(sd.camera, fs), yk.SamplerType.Uniform(1, SEED), (0, 0, 32, 18), 0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    shapes = []
    for s in (yk.Scene(c, sd), yk.Scene.from_device(c, sd, _tensors(sd))):
        shape = np.zeros(len(o), dtype=np.int32)
        yk.check(yk.lib().yk_trace_closest(c.h, s.h, len(o), p(o), p(d), None, p(shape), None, None, None, None, None), c.h)
        shapes.append(shape)
        assert s.layout_info().tree_fetched == 1
        s.close()
    assert np.array_equal(shapes[0], shapes[1]) and (shapes[1] >= 0).any()
