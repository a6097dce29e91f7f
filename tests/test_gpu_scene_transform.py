"""yk_scene_transform on the device: the device route (records in device memory, or a device-laid scene) writes what the
host route writes — records, head, info and tree — and what yk_scene_update writes for the transformed arrays; identity
changes no byte and fetches no tree; transforms are absolute; a mirroring matrix gives the scene created with the mirrored
mesh; every refusal leaves the scene alone; a table produced on a side stream is waited for; a Path tile agrees with the
updated scene's; the motion pass from matrices equals the host instance and the pass from the previous vertex tensor; the
rest copy is counted once; the tree cost agrees with the host's within the derived bound.  The soups put a 256-lane block's
seam and a scan block's seam inside the vertex kernels, with unreferenced vertices at the seam.  On the library's default
path — a host-laid scene transformed with a host table — the rest pose is in device memory too, so the motion kernel and the
host instance agree there; an update after a mirroring transform gives creation's flags back; a scene that is not the
context's is refused."""
import copy

import numpy as np
import pytest
import torch

import motion_ref
import transform_ref as ref
from test_gpu_scene_from_device import SCENES as DEVICE_SCENES
from test_gpu_scene_from_device import _assert_same_scene, _render_tile, _snapshot, _tensors
from test_scene_transform import _moved_spheres, _quad_over_two_meshes, lit_meshes, overflowing, records
from yuki_amd import _ffi, abi, scenes

pytestmark = pytest.mark.gpu
F = np.float32


def _soup(n_triangles, spare):
    """Disjoint triangles, triangle t in mesh t mod 3, with normals, and `spare` vertices no triangle indexes at the end."""
    rng = np.random.default_rng(1000 + 3 * n_triangles + spare)
    sd = scenes.deep_chain(n_triangles)
    centres = rng.uniform(-4.0, 4.0, (n_triangles, 1, 3))
    pts = (centres + rng.uniform(-0.3, 0.3, (n_triangles, 3, 3))).reshape(-1, 3)
    sd.points = np.ascontiguousarray(np.concatenate([pts, rng.uniform(-4.0, 4.0, (spare, 3))]), dtype=F)
    sd.points[::7, 0] = -0.0  # negative zeros in the rest pose
    n = rng.normal(size=sd.points.shape)
    sd.normals = np.ascontiguousarray(n / np.linalg.norm(n, axis=1, keepdims=True), dtype=F)
    sd.tri_mesh = (np.arange(n_triangles) % 3).astype(np.uint32)
    sd.meshes = [(True, False, False)] * 3
    sd.split_method, sd.max_shapes_in_node = abi.SPLIT_SAH, 4
    sd.name = f"soup-{len(sd.points)}"
    sd.camera = dict(position=(0.0, 0.0, -14.0), target=(0.0, 0.0, 0.0), up=(0, 1, 0), fov_axis=abi.FOV_X, fov_degrees=45.0)
    return sd


SCENES = {name: DEVICE_SCENES[name] for name in ("one-shape", "two-shapes", "cornell", "city-tiny", "coplanar-slabs")}
SCENES.update({"soup-255": lambda: _soup(85, 0), "soup-256": lambda: _soup(85, 1), "soup-257": lambda: _soup(85, 2), "soup-513": lambda: _soup(171, 0)})
MOVED = [name for name in SCENES if len(SCENES[name]().meshes)]


@pytest.fixture(scope="module")
def contexts(yk):
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


def _dev_records(rec):
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.float32).reshape(-1).copy()).to("cuda:0")


def _same(got, want):
    for name in abi.RECORD_NAMES:
        assert len(got["records"][name]) == len(want["records"][name]), name
        assert got["records"][name] == want["records"][name], name
    for key in ("records", "head", "info", "tree"):
        assert got[key] == want[key], key


def _three_ways(yk, contexts, sd, rec, **options):
    """Scene A: host layout, host records (the host route); scene B: from device tensors, records in device memory (the
    device route); scene C: created with the mirrored meshes and updated with the reference's arrays."""
    a = yk.Scene(contexts(scene_layout=0, **options), sd)
    a.transform(rec)
    ia = a.transform_info()
    assert (ia.n_transforms, ia.route, ia.reason) == (1, abi.UPDATE_ROUTE_HOST, 0)
    b = yk.Scene.from_device(contexts(**options), sd, _tensors(sd))
    b.transform(_dev_records(rec))
    ib = b.transform_info()
    assert (ib.n_transforms, ib.route, ib.reason) == (1, abi.UPDATE_ROUTE_DEVICE, 0)
    assert b.layout_info().tree_fetched == 0
    points, normals, flipped = ref.transform(sd, rec)
    assert (ia.n_moved_meshes, ia.n_flipped_meshes) == (ib.n_moved_meshes, ib.n_flipped_meshes) == (int(sum(not ref.is_identity(r["rest_to_world"]) for r in rec)), int(flipped.sum()))
    other = copy.copy(sd)
    other.meshes = ref.flipped_meshes(sd, flipped)
    c = yk.Scene.from_device(contexts(**options), other, _tensors(other))
    c.update(_dev(points), None if normals is None else _dev(normals))
    n_nodes = b.info().n_nodes
    print(f"{sd.name}: tree_cost device {ib.tree_cost!r} host {ia.tree_cost!r}; at rest device {ib.tree_cost_rest!r} host {ia.tree_cost_rest!r}; bound {ref.cost_bound(n_nodes, ia.tree_cost):.3e}")
    assert abs(ib.tree_cost - ia.tree_cost) <= ref.cost_bound(n_nodes, ia.tree_cost)
    assert abs(ib.tree_cost_rest - ia.tree_cost_rest) <= ref.cost_bound(n_nodes, ia.tree_cost_rest)
    got, want, updated = _snapshot(b), _snapshot(a), _snapshot(c)
    for s in (a, b, c):
        s.close()
    _same(got, want)
    _same(got, updated)
    return got


# ---- 1. the device route is the host route is the update
@pytest.mark.parametrize("name", MOVED)
@pytest.mark.parametrize("mirror", [False, True])
def test_device_route_equals_host_route_and_the_update(yk, contexts, name, mirror):
    sd = SCENES[name]()
    _three_ways(yk, contexts, sd, records(sd, "A", mirror))


@pytest.mark.parametrize("wide,max_shapes", [(0, 1), (0, 4), (2, 1), (2, 4)])
def test_device_route_equals_host_route_variants(yk, contexts, wide, max_shapes):
    for name in ("city-tiny", "soup-257"):
        sd = SCENES[name]()
        sd.max_shapes_in_node = max_shapes
        _three_ways(yk, contexts, sd, records(sd, "B", True), wide_bvh=wide)


def test_a_host_table_on_a_device_laid_scene_takes_the_device_route(yk, contexts):
    sd = SCENES["city-tiny"]()
    rec = records(sd, "A", True)
    a = yk.Scene(contexts(bvh_builder=1, scene_layout=1), sd)
    a.transform(rec)
    assert (a.transform_info().route, a.transform_info().reason) == (abi.UPDATE_ROUTE_DEVICE, 0)
    b = yk.Scene(contexts(scene_layout=0), sd)
    b.transform(_dev_records(rec))  # and records in device memory on a host-laid scene
    assert (b.transform_info().route, b.transform_info().reason) == (abi.UPDATE_ROUTE_DEVICE, 0)
    b.transform(rec)  # the rest pose a device-route call kept serves the host route
    assert b.transform_info().route == abi.UPDATE_ROUTE_HOST
    got, want = _snapshot(a), _snapshot(b)
    a.close()
    b.close()
    _same(got, want)


# ---- 2. identity, 3. nothing accumulates
@pytest.mark.parametrize("name", list(SCENES))
def test_identity_changes_no_byte_and_transforms_are_absolute(yk, contexts, name):
    sd = SCENES[name]()
    n = len(sd.meshes)
    s = yk.Scene.from_device(contexts(), sd, _tensors(sd))
    before = _snapshot(s)
    device_bytes = s.info().device_bytes
    s.transform(_dev_records(abi.pack_mesh_transforms([None] * n)))
    i = s.transform_info()
    assert (i.n_transforms, i.route, i.reason, i.n_moved_meshes) == (1, abi.UPDATE_ROUTE_DEVICE, 0, 0)
    assert s.layout_info().tree_fetched == 0
    after = _snapshot(s)
    assert after["fetched_before_export"] == 0
    _assert_same_scene(after, before)
    plan = s.update_info().plan_bytes
    assert i.rest_bytes > 0 and s.info().device_bytes == device_bytes + plan + i.rest_bytes  # counted once
    s.transform(_dev_records(records(sd, "A")))
    once = _snapshot(s)
    s.transform(_dev_records(records(sd, "B", True)))
    twice = _snapshot(s)
    fresh = yk.Scene.from_device(contexts(), sd, _tensors(sd))
    fresh.transform(_dev_records(records(sd, "B", True)))
    _same(twice, _snapshot(fresh))
    fresh.close()
    assert once["tree"] != before["tree"] and twice["tree"] != once["tree"]
    s.transform(_dev_records(abi.pack_mesh_transforms([None] * n)))
    _assert_same_scene(_snapshot(s), before)
    j = s.transform_info()
    assert j.n_transforms == 4 and j.rest_bytes == i.rest_bytes and s.info().device_bytes == device_bytes + plan + i.rest_bytes
    assert j.tree_cost == i.tree_cost == i.tree_cost_rest == j.tree_cost_rest  # exactly reproducible
    s.update(_tensors(sd)["points"])  # an update drops the rest copy
    assert s.transform_info().rest_bytes == 0 and s.info().device_bytes == device_bytes + plan
    s.close()


# ---- 4. refusals
def test_every_refusal_with_device_records_leaves_the_scene_alone(yk, contexts):
    for name, lit in (("cornell", 0), ("city-tiny", 7)):
        sd = SCENES[name]()
        n = len(sd.meshes)
        free = [m for m in range(n) if m not in lit_meshes(sd)][0]
        s = yk.Scene.from_device(contexts(), sd, _tensors(sd))
        before = _snapshot(s)
        shift = np.eye(4)
        shift[0, 3] = 0.25

        def refused(rec, message):
            with pytest.raises(_ffi.YukiError) as e:
                s.transform(_dev_records(rec))
            assert e.value.status == 1 and str(e.value).endswith(message), str(e.value)
            _assert_same_scene(_snapshot(s), before)

        moved = abi.pack_mesh_transforms([shift if m == free else None for m in range(n)])
        for field, value in (("rest_to_world", np.nan), ("world_to_rest", np.inf)):
            bad = moved.copy()
            bad[field][free][6] = value
            refused(bad, "transforms: matrix entry not finite")
        lit_rec = abi.pack_mesh_transforms([shift if m == lit else None for m in range(n)])
        refused(lit_rec, "transforms: a mesh that carries an area light cannot move")
        over = overflowing(sd, free)
        refused(over, "points: coordinate not finite")
        both = lit_rec.copy()  # precedence: the matrix, the area light, the result
        both["rest_to_world"][lit][0] = np.inf
        refused(both, "transforms: matrix entry not finite")
        both = lit_rec.copy()
        both[free] = over[free]
        refused(both, "transforms: a mesh that carries an area light cannot move")
        assert s.transform_info().n_transforms == 0
        with pytest.raises(ValueError):
            s.transform(_dev_records(moved)[:-1])
        with pytest.raises(ValueError):
            s.transform(_dev_records(moved).cpu())
        s.transform(_dev_records(moved))  # and the scene still moves
        assert s.transform_info().n_transforms == 1 and _snapshot(s)["tree"] != before["tree"]
        s.close()


def test_a_shared_vertex_refuses_with_device_records(yk, contexts):
    sd = _quad_over_two_meshes()
    s = yk.Scene.from_device(contexts(), sd, _tensors(sd))
    before = _snapshot(s)
    shift = np.eye(4)
    shift[2, 3] = 1.0
    for rec in (abi.pack_mesh_transforms([None, None]), abi.pack_mesh_transforms([shift, None]), overflowing(sd, 0)):
        with pytest.raises(_ffi.YukiError) as e:
            s.transform(_dev_records(rec))
        assert e.value.status == 1 and str(e.value).endswith("transforms: vertex shared by two meshes")
        _assert_same_scene(_snapshot(s), before)
    bad = abi.pack_mesh_transforms([shift, None])
    bad["rest_to_world"][0][1] = np.nan
    with pytest.raises(_ffi.YukiError) as e:
        s.transform(_dev_records(bad))
    assert str(e.value).endswith("transforms: matrix entry not finite")
    s.close()


# ---- 5. ordering
def test_records_produced_on_a_side_stream_are_waited_for(yk, contexts):
    sd = SCENES["city-tiny"]()
    rec = records(sd, "A")
    want_scene = yk.Scene.from_device(contexts(), sd, _tensors(sd))
    want_scene.transform(_dev_records(rec))
    want = _snapshot(want_scene)
    want_scene.close()
    s = yk.Scene.from_device(contexts(), sd, _tensors(sd))
    side = torch.cuda.Stream()
    host = torch.from_numpy(rec.view(np.float32).reshape(-1).copy()).pin_memory()
    with torch.cuda.stream(side):
        ballast = torch.ones(1 << 24, device="cuda:0")
        for _ in range(8):
            ballast = ballast * 1.0001  # work in front of the copy on the side stream
        d = torch.empty(host.numel(), dtype=torch.float32, device="cuda:0")
        d.copy_(host, non_blocking=True)
    s.transform(d, stream=side)
    _same(_snapshot(s), want)
    s.close()
    torch.cuda.synchronize()


# ---- 6. what is rendered
@pytest.mark.parametrize("name", ["cornell", "city-tiny"])
def test_a_path_tile_after_transform_equals_the_tile_after_update(yk, contexts, name):
    sd = SCENES[name]()
    rec = records(sd, "A", True)
    points, normals, flipped = ref.transform(sd, rec)
    ctx = contexts()
    s = yk.Scene.from_device(ctx, sd, _tensors(sd))
    rest_tile = _render_tile(yk, ctx, s, sd)
    s.transform(_dev_records(rec))
    got = _render_tile(yk, ctx, s, sd)
    s.close()
    other = copy.copy(sd)
    other.meshes = ref.flipped_meshes(sd, flipped)
    u = yk.Scene.from_device(ctx, other, _tensors(other))
    u.update(_dev(points), None if normals is None else _dev(normals))
    want = _render_tile(yk, ctx, u, sd)
    u.close()
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    assert not np.array_equal(got[0], rest_tile[0])


# ---- 7. motion from matrices
@pytest.mark.parametrize("name", ["cornell", "city-tiny"])
def test_motion_from_matrices_on_the_device(yk, contexts, name):
    sd = SCENES[name]()
    ctx = contexts()
    prev = records(sd, "A", True)
    prev_points, _, _ = ref.transform(sd, prev)
    s = yk.Scene.from_device(ctx, sd, _tensors(sd))
    s.transform(_dev_records(records(sd, "B")))
    w, h = 33, 17  # partial tiles
    rng = np.random.default_rng(20261021)
    ids, g = motion_ref.synthetic_ids(rng, w, h, sd.n_triangles, len(sd.spheres), True)
    host = yk.surface_motion(s, ids, g, prev_transforms=prev)  # the host instance: the rest pose comes back from the device
    assert host.tobytes() == yk.surface_motion(s, ids, g, prev_points).tobytes()
    assert yk.surface_motion(s, ids, g, prev_transforms=prev, ctx=ctx).tobytes() == host.tobytes()
    d_ids = torch.from_numpy(ids.view(np.uint32).reshape(h, w, 4).view(np.int32).copy()).to("cuda:0")
    d_g = torch.from_numpy(g.view(np.float32).reshape(h, w, 8).copy()).to("cuda:0")
    d_prev, d_points = _dev_records(prev), _dev(prev_points)
    for spheres in ((None, _moved_spheres(sd)) if len(sd.spheres) else (None,)):
        d_spheres = None if spheres is None else torch.from_numpy(abi.pack_spheres(spheres).view(np.uint8).copy()).to("cuda:0")
        sp = d_spheres.data_ptr() if spheres is not None else None
        want_host = yk.surface_motion(s, ids, g, prev_transforms=prev, prev_spheres=spheres)
        out_a = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda:0")
        out_b = torch.full((h, w, 4), 9.0, dtype=torch.float32, device="cuda:0")
        ctx.surface_motion_device(s, d_ids.data_ptr(), d_g.data_ptr(), None, (w, h), out_a.data_ptr(), d_prev_spheres_ptr=sp, d_prev_transforms_ptr=d_prev.data_ptr())
        ctx.surface_motion_device(s, d_ids.data_ptr(), d_g.data_ptr(), d_points.data_ptr(), (w, h), out_b.data_ptr(), d_prev_spheres_ptr=sp)
        torch.cuda.synchronize()
        a, b = out_a.cpu().numpy().view(np.uint32), out_b.cpu().numpy().view(np.uint32)
        assert np.array_equal(a, b)
        assert a.tobytes() == want_host.tobytes()
    out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    ctx.surface_motion_device(s, d_ids.data_ptr(), d_g.data_ptr(), None, (w, h), out.data_ptr(), d_prev_transforms_ptr=None)  # at rest
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == yk.surface_motion(s, ids, g, np.ascontiguousarray(sd.points, F)).tobytes()
    s.close()


# ---- 8. the default path: a host-laid scene transformed with a host table keeps its rest pose in device memory too
@pytest.mark.parametrize("name", ["cornell", "city-tiny"])
def test_motion_after_a_host_route_transform(yk, contexts, name):
    sd = SCENES[name]()
    ctx = contexts(scene_layout=0)
    prev = records(sd, "A", True)
    prev_points, _, _ = ref.transform(sd, prev)
    s = yk.Scene(ctx, sd)
    device_bytes = s.info().device_bytes
    s.transform(records(sd, "B"))
    i = s.transform_info()
    assert (i.route, i.reason) == (abi.UPDATE_ROUTE_HOST, 0)
    assert i.rest_bytes > 0 and s.info().device_bytes == device_bytes + i.rest_bytes  # in device memory, counted once
    w, h = 33, 17
    ids, g = motion_ref.synthetic_ids(np.random.default_rng(20261021), w, h, sd.n_triangles, len(sd.spheres), True)
    host = yk.surface_motion(s, ids, g, prev_transforms=prev)  # the host instance
    assert host.tobytes() == yk.surface_motion(s, ids, g, prev_points).tobytes()
    assert ((ids["shape"] < sd.n_triangles) & (host["known"] == 1)).any()
    assert host.tobytes() != yk.surface_motion(s, ids, g, prev_transforms=None).tobytes()
    assert yk.surface_motion(s, ids, g, prev_transforms=prev, ctx=ctx).tobytes() == host.tobytes()
    assert yk.surface_motion(s, ids, g, prev_points, ctx=ctx).tobytes() == host.tobytes()
    d_ids = torch.from_numpy(ids.view(np.uint32).reshape(h, w, 4).view(np.int32).copy()).to("cuda:0")
    d_g = torch.from_numpy(g.view(np.float32).reshape(h, w, 8).copy()).to("cuda:0")
    d_prev = _dev_records(prev)
    out = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda:0")
    ctx.surface_motion_device(s, d_ids.data_ptr(), d_g.data_ptr(), None, (w, h), out.data_ptr(), d_prev_transforms_ptr=d_prev.data_ptr())
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == host.tobytes()
    s.update(np.ascontiguousarray(sd.points, F))  # the update drops the copy
    assert s.transform_info().rest_bytes == 0 and s.info().device_bytes == device_bytes
    s.close()


# ---- 9. an update after a mirroring transform: the flags are creation's again
@pytest.mark.parametrize("route", ["device", "host"])
def test_update_after_a_mirroring_transform_resets_the_mesh_flags(yk, contexts, route):
    sd = SCENES["city-tiny"]()
    rec = records(sd, "A", True)
    assert ref.transform(sd, rec)[2].any()
    moved = ref.transform(sd, records(sd, "B"))
    if route == "device":
        s, fresh = (yk.Scene.from_device(contexts(), sd, _tensors(sd)) for _ in range(2))
        s.transform(_dev_records(rec))
        args = (_dev(moved[0]), _dev(moved[1]))
    else:
        s, fresh = (yk.Scene(contexts(scene_layout=0), sd) for _ in range(2))
        s.transform(rec)
        args = (moved[0], moved[1])
    assert s.transform_info().n_flipped_meshes > 0
    mirrored = _snapshot(s)
    s.update(*args)
    fresh.update(*args)
    got, want = _snapshot(s), _snapshot(fresh)
    _same(got, want)
    assert got["records"]["prim_shade"] != mirrored["records"]["prim_shade"]
    s.transform(_dev_records(abi.pack_mesh_transforms([None] * len(sd.meshes))) if route == "device" else [None] * len(sd.meshes))
    _same(_snapshot(s), want)  # the new rest pose, creation's flags
    s.close()
    fresh.close()


# ---- 10. a scene that is not this context's
def test_a_scene_that_is_not_the_contexts_is_refused(yk, contexts):
    sd = SCENES["city-tiny"]()
    ctx = contexts()
    rec = records(sd, "A")
    d_rec = _dev_records(rec)
    lib = _ffi.lib()
    host_only, on_device = yk.Scene(None, sd), yk.Scene(ctx, sd)
    before = _snapshot(on_device)
    calls = (("a host-only scene, a context", lambda: lib.yk_scene_transform(ctx.h, host_only.h, rec.ctypes.data), ctx.h),
             ("a host-only scene, device records", lambda: lib.yk_scene_transform_device(ctx.h, host_only.h, d_rec.data_ptr(), None), ctx.h),
             ("a scene in device memory, no context", lambda: lib.yk_scene_transform(None, on_device.h, rec.ctypes.data), None))
    for what, call, where in calls:
        with pytest.raises(_ffi.YukiError) as e:
            _ffi.check(call(), where)
        assert e.value.status == 1 and str(e.value).endswith("scene was not created on this context's device"), (what, str(e.value))
    assert lib.yk_scene_transform_device(None, on_device.h, d_rec.data_ptr(), None) == 1
    _assert_same_scene(_snapshot(on_device), before)
    assert on_device.transform_info().n_transforms == 0 and host_only.transform_info().n_transforms == 0
    ids, g = motion_ref.synthetic_ids(np.random.default_rng(1), 8, 8, sd.n_triangles, 0, True)
    with pytest.raises(_ffi.YukiError) as e:
        yk.surface_motion(host_only, ids, g, prev_transforms=rec, ctx=ctx)
    assert str(e.value).endswith("scene was not created on this context's device")
    host_only.close()
    on_device.close()
