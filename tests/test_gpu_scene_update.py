"""Scene.update / yk_scene_update[_device] on the device (yuki_amd/csrc/yk_scene_update.hip): a scene updated with its own
points is byte for byte what it was; the device route writes what the host route writes and what tests/refit_ref.py says;
updates do not accumulate; the refitted scene answers rays as the moved geometry does (float64 brute force, every kernel);
images agree between the routes and a render enqueued before an update sees the old geometry; bad input is refused with
nothing written; a side stream is waited for.  The small scenes of the layout test, plus either side of a scan block
(512 / 513 shapes) and of a block of 256 lanes (255 / 256 / 257 triangles)."""
import numpy as np
import pytest
import torch

import refit_ref
import test_trace_reference as tr
import trace_ref
from test_gpu_scene_from_device import SCENES, _assert_same_scene, _render_tile, _snapshot, _tensors
from test_gpu_trace_kernels import closest_ids
from test_scene_update import TRACED, moved_scene, sphere_table, wobble
from yuki_amd import _ffi, abi

pytestmark = pytest.mark.gpu

SEED = 0x5CE7E


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


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


def _same(got, want, keys=("records", "head", "info", "tree")):
    for name in abi.RECORD_NAMES:
        assert len(got["records"][name]) == len(want["records"][name]), name
        assert got["records"][name] == want["records"][name], name
    for key in keys:
        assert got[key] == want[key], key


# ---- 1. identity on the device
@pytest.mark.parametrize("name", list(SCENES))
def test_update_with_the_same_tensors_changes_nothing(yk, contexts, name):
    for method in (abi.SPLIT_SAH, abi.SPLIT_MIDDLE):
        for max_shapes in (1, 4):
            for wide in (0, 2):
                sd = SCENES[name]()
                sd.split_method, sd.max_shapes_in_node = method, max_shapes
                arrays = _tensors(sd)
                s = yk.Scene.from_device(contexts(wide_bvh=wide), sd, arrays)
                before = _snapshot(s)
                s.update(arrays["points"], arrays.get("normals"))
                i = s.update_info()
                assert (i.n_updates, i.route, i.reason) == (1, abi.UPDATE_ROUTE_DEVICE, 0), (method, max_shapes, wide)
                assert s.layout_info().tree_fetched == 0  # the host copy is stale until something asks
                after = _snapshot(s)
                assert after["fetched_before_export"] == 0
                _assert_same_scene(after, before)
                s.close()


# ---- 2. the device route is the host route is the rule
def _routes(yk, contexts, sd, points, normals, **options):
    """Scene A: host layout, updated with numpy arrays; scene B: from device tensors, updated with tensors."""
    a = yk.Scene(contexts(scene_layout=0, **options), sd)
    a.update(points, normals)
    ia = a.update_info()
    assert (ia.route, ia.reason) == (abi.UPDATE_ROUTE_HOST, 0)
    b = yk.Scene.from_device(contexts(**options), sd, _tensors(sd))
    tree_before = b.export_bvh()
    b.update(_dev(points), None if normals is None else _dev(normals))
    ib = b.update_info()
    assert (ib.route, ib.reason) == (abi.UPDATE_ROUTE_DEVICE, 0)
    got, want = _snapshot(b), _snapshot(a)
    a.close()
    b.close()
    _same(got, want)
    return got, tree_before


@pytest.mark.parametrize("name", list(SCENES))
def test_device_route_equals_host_route_and_the_reference(yk, contexts, name):
    sd = SCENES[name]()
    moved = wobble(sd, 0.05)
    got, (nodes, order) = _routes(yk, contexts, sd, moved, None)
    want = refit_ref.refit(nodes, order, moved, sd.indices, sphere_table(yk, sd))
    assert got["tree"] == (want.tobytes(), order.tobytes())
    assert got["tree"][0] != nodes.tobytes()


@pytest.mark.parametrize("case", ["equal-counts", "leaves-of-4-binary", "normals", "normals-kept"])
def test_device_route_equals_host_route_variants(yk, contexts, case):
    sd = SCENES["city-tiny-permuted" if case == "leaves-of-4-binary" else "city-tiny"]()
    options, normals = {}, None
    if case == "equal-counts":  # the host builds the tree; the device route uploads it for its plan
        sd.split_method, sd.max_shapes_in_node = abi.SPLIT_EQUAL_COUNTS, 2
    elif case == "leaves-of-4-binary":
        sd.max_shapes_in_node, options = 4, {"wide_bvh": 0}
    elif case == "normals":
        n = np.asarray(sd.normals, dtype=np.float32)
        normals = np.ascontiguousarray(n[:, [2, 0, 1]] * np.float32(0.5))
    moved = wobble(sd, 0.1)
    got, (nodes, order) = _routes(yk, contexts, sd, moved, normals, **options)
    assert got["who"][0] == (0 if case == "equal-counts" else 1)
    assert got["tree"] == (refit_ref.refit(nodes, order, moved, sd.indices).tobytes(), order.tobytes())
    if case == "normals":  # the new normals are in the records; with None the old ones stay
        kept, _ = _routes(yk, contexts, sd, moved, None, **options)
        assert kept["records"]["prim_attr"] != got["records"]["prim_attr"]
        assert kept["records"]["tris"] == got["records"]["tris"]


# ---- 3. nothing accumulates
@pytest.mark.parametrize("name", ["cornell", "city-tiny", "seam-513"])
def test_two_updates_and_back(yk, contexts, name):
    sd = SCENES[name]()
    arrays = _tensors(sd)
    s = yk.Scene.from_device(contexts(), sd, arrays)
    before = _snapshot(s)
    device_bytes = s.info().device_bytes
    s.update(_dev(wobble(sd, 0.01)))
    plan = s.update_info().plan_bytes
    assert plan > 0 and s.info().device_bytes == device_bytes + plan
    once = _snapshot(s)
    s.update(_dev(wobble(sd, 0.1, phase=1.0)))
    twice = _snapshot(s)
    assert once["tree"] != before["tree"] and twice["tree"] != once["tree"] and twice["records"]["tris"] != once["records"]["tris"]
    s.update(arrays["points"])
    i = s.update_info()
    assert (i.n_updates, i.plan_bytes, i.route) == (3, plan, abi.UPDATE_ROUTE_DEVICE) and s.info().device_bytes == device_bytes + plan
    _assert_same_scene(_snapshot(s), before)
    s.close()


# ---- 4. geometry, not self-agreement
@pytest.mark.parametrize("name", list(TRACED))
def test_the_updated_scene_answers_rays_as_the_moved_geometry_does(yk, oracle, contexts, name):
    """deep-line is a tree 76 levels deep, and a refit keeps it so.  The reference's traversal stack has 64 entries
    (bvh.rs:174) and a ray that runs up the chain (d.x >= 0) defers one child per level: in the scene as created, before any
    update, the oracle dies on such rays of these very sets and the library answers YK_ERR_STACK_OVERFLOW.  So on deep-line
    the sets keep their rays with d.x < 0, which visit the split-off leaf first and hold one entry; nothing else differs."""
    sd = TRACED[name]()
    moved = wobble(sd, 0.1)
    msd = moved_scene(sd, moved)
    ref = trace_ref.TraceRef(msd)
    closest, anyhit = tr.ray_sets(oracle, msd, name)
    o, d = tr.random_rays(msd, 2048, SEED)
    closest.append(("random 2048", o, d, None))
    if name == "deep-line":
        down = lambda dirs: dirs[:, 0] < 0  # noqa: E731
        closest = [(label, ro[down(rd)], rd[down(rd)], None if tm is None else tm[down(rd)]) for label, ro, rd, tm in closest]
        anyhit = [(label, ro[down(rd)], rd[down(rd)], tm[down(rd)], al[down(rd)]) for label, ro, rd, tm, al in anyhit]
        closest = [c for c in closest if len(c[1])]  # the camera looks up the chain: none of its rays is left
        assert sum(len(c[1]) for c in closest) > 2000 and all(len(a[1]) for a in anyhit)
    deep = yk.Scene(None, sd).info().tree_depth > 64
    assert deep == (name == "deep-line")
    for mode, wide in ((0, 0), (0, 1), (1, 0), (1, 1), (2, None)):
        if mode == 2 and deep:
            continue  # the packet kernels refuse a tree deeper than 64 (test_gpu_trace_kernels.py::test_mode_refusals)
        c = contexts(trace_stage_kernel=mode, **({} if wide is None else {"wide_bvh": wide}))
        s = yk.Scene.from_device(c, sd, _tensors(sd))
        s.update(_dev(moved))
        assert s.update_info().route == abi.UPDATE_ROUTE_DEVICE and s.layout_info().tree_fetched == 0
        n_robust = 0
        for label, ro, rd, tm in closest:
            if tm is not None and mode != 0:
                continue  # refused by modes 1 and 2
            shape, t = closest_ids(yk, s, ro, rd, tm, want_t=mode == 0)
            rob, hit = tr.check_closest(ref, label, ro, rd, tm, shape, t)
            n_robust += int(hit.sum())
        assert n_robust > 100, (mode, wide, n_robust)
        for label, ro, rd, tm, al in anyhit:
            tr.check_any(ref, label, ro, rd, tm, al, s.any_intersect(ro, rd, tm, al))
        if mode != 0:
            assert s.layout_info().tree_fetched == 1  # the stage call read the refetched host tree
        s.close()


# ---- 5. images
@pytest.mark.parametrize("name", ["cornell", "city-tiny"])
def test_images_agree_between_the_routes_and_an_enqueued_render_sees_the_old_scene(yk, contexts, name):
    sd = SCENES[name]()
    moved = wobble(sd, 0.05)
    ch = contexts(scene_layout=0)
    a = yk.Scene(ch, sd)
    a.update(moved)
    want_bits, want_rays = _render_tile(yk, ch, a, sd)
    a.close()
    c = contexts()
    b = yk.Scene.from_device(c, sd, _tensors(sd))
    old_bits, old_rays = _render_tile(yk, c, b, sd)
    # a render that is enqueued, not waited for, then the update, then the read
    fs = yk.FilmSettings(res=(32, 32), tile_dim=32)
    integ = yk.IntegratorType.instantiate(c, yk.IntegratorType.Path(yk.PathParams(max_depth=8)))
    sampler = yk.SamplerType.Stratified((2, 2), True, _seed())
    old = torch.zeros((32 * 32, 3), dtype=torch.float32, device="cuda:0")
    out = torch.zeros_like(old)
    new_points = _dev(moved)
    torch.cuda.synchronize()
    integ.render_tiles_device(b, yk.Camera(sd.camera, fs), sampler, yk.film_tiles(fs), old.data_ptr())
    assert old.any()
    integ.render_tiles_device(b, yk.Camera(sd.camera, fs), sampler, yk.film_tiles(fs), out.data_ptr(), want_stats=False)
    b.update(new_points)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), old.view(torch.int32))
    bits, rays = _render_tile(yk, c, b, sd)
    assert rays == want_rays and np.array_equal(bits, want_bits)
    assert not np.array_equal(bits, old_bits)
    b.close()


def _seed():
    from test_gpu_scene_layout import SEED as LAYOUT_SEED

    return LAYOUT_SEED


# ---- 6. refusals
def test_bad_input_is_refused_and_the_records_stay(yk, contexts):
    sd = SCENES["city-tiny"]()
    c = contexts()
    s = yk.Scene.from_device(c, sd, _tensors(sd))
    s.update(_dev(wobble(sd, 0.01)))  # the plan exists: a refusal must not touch it either
    before = _snapshot(s)
    moved = wobble(sd, 0.1)
    for value in (np.nan, np.inf):
        bad = moved.copy()
        bad[len(bad) // 3, 2] = value
        with pytest.raises(_ffi.YukiError) as e:
            s.update(_dev(bad))
        assert e.value.status == 1 and str(e.value).endswith("points: coordinate not finite")
        with pytest.raises(_ffi.YukiError) as e:
            s.update(bad)
        assert e.value.status == 1 and str(e.value).endswith("points: coordinate not finite")
    host = np.ascontiguousarray(moved)
    with pytest.raises(_ffi.YukiError) as e:
        s.update(int(host.ctypes.data))
    assert e.value.status == 1 and str(e.value).endswith("points is not device memory of this context's device")
    torch.cuda.empty_cache()  # so that the next large tensor is an allocation of its own, exactly as long as asked
    big = torch.zeros(32 << 20, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(_ffi.YukiError) as e:
        s.update(int(big.data_ptr()) + (32 << 20) - 64)  # 64 bytes before the allocation's end
    assert e.value.status == 1 and str(e.value).endswith("points is shorter than its count says")
    good = _dev(moved)
    with pytest.raises(_ffi.YukiError) as e:
        s.update(good, int(host.ctypes.data))
    assert str(e.value).endswith("normals is not device memory of this context's device")
    for wrong in (good.double(), good[:-1].contiguous(), good.t(), good.cpu()):
        with pytest.raises(ValueError):
            s.update(wrong)
    assert s.update_info().n_updates == 1
    _assert_same_scene(_snapshot(s), before)
    s.close()
    bare = SCENES["signed-zeros"]()
    s = yk.Scene.from_device(c, bare, _tensors(bare))
    before = _snapshot(s)
    with pytest.raises(_ffi.YukiError) as e:
        s.update(_dev(bare.points), _dev(bare.points))
    assert str(e.value).endswith("normals given for a scene created without normals")
    _assert_same_scene(_snapshot(s), before)
    s.close()


# ---- 7. stream order
def test_points_produced_on_a_side_stream(yk, contexts):
    sd = SCENES["city-tiny"]()
    moved = wobble(sd, 0.05)
    c = contexts()
    s = yk.Scene.from_device(c, sd, _tensors(sd))
    s.update(_dev(moved))
    want = _snapshot(s)
    s.update(_tensors(sd)["points"])
    half = (_dev(moved) * 0.5).contiguous()  # x / 2 + x / 2 == x in float32 for every normal x
    assert torch.equal(half + half, _dev(moved))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        busy = torch.ones((2048, 2048), device="cuda:0")
        for _ in range(8):  # work in front of the points on their stream
            busy = busy @ busy * (1.0 / 2048.0)
        points = half + half
    s.update(points, stream=side)
    _assert_same_scene(_snapshot(s), want)
    assert float(busy[0, 0]) == 1.0
    s.close()


# ---- 9. the options an update lays out with are creation's
@pytest.mark.parametrize("source", ["host-input", "device-input"])
def test_an_update_lays_out_what_creation_did_whatever_the_context_says_today(yk, source):
    """A scene created with top_nodes = 3 and wide_bvh = 2 keeps its three-node tree tops and both node layouts through an
    update made after the context's two options were set to 0, by the host route (host input, host layout) and by the device
    route (device input); a scene created afterwards on the same context has neither, so the update did not touch the
    live options either."""
    sd = SCENES["city-tiny"]()
    ctx = yk.Context(0, top_nodes=3, wide_bvh=2)
    try:
        arrays = _tensors(sd)
        s = yk.Scene(ctx, sd) if source == "host-input" else yk.Scene.from_device(ctx, sd, arrays)
        before = _snapshot(s)
        assert before["head"][1:] == (3, 3, 1, 1)  # n_top, n_top_any, wide, wide_auto
        assert before["who"][2] == (abi.LAYOUT_HOST if source == "host-input" else abi.LAYOUT_DEVICE)
        ctx.set_option("top_nodes", 0)
        ctx.set_option("wide_bvh", 0)
        if source == "host-input":
            s.update(np.ascontiguousarray(sd.points, dtype=np.float32))
        else:
            s.update(arrays["points"])
        i = s.update_info()
        assert (i.n_updates, i.route, i.reason) == (1, abi.UPDATE_ROUTE_HOST if source == "host-input" else abi.UPDATE_ROUTE_DEVICE, 0)
        _assert_same_scene(_snapshot(s), before)
        s.close()
        fresh = yk.Scene(ctx, sd)
        li = fresh.layout_info()
        assert (li.n_top, li.n_top_any, li.wide, li.wide_auto) == (0, 0, 0, 0)
        fresh.close()
    finally:
        ctx.close()
