"""Scene.edit / yk_scene_apply_edit[_device] and yk_surface_motion_spheres on the device (yuki_amd/csrc/yk_scene_edit.hip,
yk_scene_change.cpp, yk_motion.hip): an edit with the scene's own tables changes no byte; an edit of lights, materials or the
background gives the scene creation makes of the edited description, records and rendered bits; the device route of a
sphere edit writes what the host route writes; the edited scene answers rays as the moved geometry does; a render enqueued
before an edit sees the old scene; bad tables are refused with nothing written; the motion pass with a previous sphere table
equals its host instance; the chain carries a moved sphere's history to where the float64 statement says; and every edit and
update of a host-laid and of a device-laid scene runs as the hand-written table of tests/cpp/scene_change_table.inc says."""
import copy

import numpy as np
import pytest
import torch

import scene_edit_ref as ref
import test_trace_reference as tr
import trace_ref
from test_gpu_scene_from_device import SCENES as DEVICE_SCENES
from test_gpu_scene_from_device import _render_tile, _snapshot, _tensors
from test_gpu_scene_layout import SEED as LAYOUT_SEED
from test_gpu_scene_update import _same
from test_gpu_trace_kernels import closest_ids
from test_scene_change_plan import row_of
from test_scene_edit import follow_the_edit_rows, motion_tolerance, own_tables
from test_scene_update import wobble
from test_temporal import same_bits
from yuki_amd import _ffi, abi, scenes

pytestmark = pytest.mark.gpu
F = np.float32
SEED = 0x5CE7E

SCENES = {"cornell": DEVICE_SCENES["cornell"], "glass_balls": scenes.glass_balls, "two-shapes": DEVICE_SCENES["two-shapes"]}
LAYOUTS = {"host-laid": dict(scene_layout=0), "device-laid": dict(bvh_builder=1, scene_layout=1)}


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


def _dev_spheres(spheres):
    """The records of a SceneData sphere list as a uint8 tensor on the device."""
    return torch.from_numpy(abi.pack_spheres(spheres).view(np.uint8).copy()).to("cuda:0")


def _render(yk, ctx, scene, sd, integ):
    fs = yk.FilmSettings(res=(32, 32), tile_dim=32)
    i = yk.IntegratorType.instantiate(ctx, integ)
    px, stats = i.render_tiles(scene, yk.Camera(sd.camera, fs), yk.SamplerType.Stratified((2, 2), True, LAYOUT_SEED), yk.film_tiles(fs))
    return np.ascontiguousarray(px, dtype=np.float32).view(np.uint32).copy(), stats.rays


# ---- 7. identity
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", list(SCENES))
def test_an_edit_with_the_same_tables_changes_nothing(yk, contexts, name, layout):
    sd = SCENES[name]()
    c = contexts(**LAYOUTS[layout])
    s = yk.Scene(c, sd)
    before = _snapshot(s)
    s.edit(**own_tables(sd))
    i = s.edit_info()
    assert (i.n_edits, i.reason) == (1, 0) and i.route == (abi.UPDATE_ROUTE_DEVICE if layout == "device-laid" else abi.UPDATE_ROUTE_HOST)
    _same(_snapshot(s), before)
    if len(sd.spheres):  # the other entry point: the sphere table from device memory always takes the device route
        s.edit(spheres=_dev_spheres(sd.spheres), lights=own_tables(sd)["lights"], materials=sd.materials, background=sd.background)
        i = s.edit_info()
        assert (i.n_edits, i.route, i.reason) == (2, abi.UPDATE_ROUTE_DEVICE, 0)
        assert i.rewrote == abi.EDIT_LIGHTS | abi.EDIT_MATERIALS | abi.EDIT_SPHERES | abi.EDIT_BOXES | abi.EDIT_RECORDS | abi.EDIT_BACKGROUND
        _same(_snapshot(s), before)
    s.close()


# ---- 8. lights, materials, background: the scene creation makes of the edited description
def _matte_sphere_cornell():
    """cornell with its sphere on the red wall's matte material: one material serves a sphere and a wall."""
    sd = scenes.cornell()
    sd.spheres = [dict(sd.spheres[0], material=2)]
    return sd


def _edits():
    out = {}
    sd = scenes.glass_balls()
    lights = copy.deepcopy(sd.lights)
    lights[0]["L"] = tuple(0.5 * float(x) for x in lights[0]["L"])
    lights[1]["l2w"] = np.array(lights[1]["l2w"], dtype=F)
    lights[1]["l2w"][:3, 3] += np.array([-0.2, -0.1, -0.2], F)
    lights[1]["I"] = (0.09, 0.02, 0.05)
    out["lights"] = (sd, dict(lights=lights), abi.EDIT_LIGHTS)
    sd = _matte_sphere_cornell()
    materials = copy.deepcopy(sd.materials)
    materials[2] = dict(kind=abi.MAT_GLASS, a=(1, 0.9, 0.9), b=(1, 1, 1), c=1.5)  # matte -> glass, on the sphere and on a wall
    out["material-kind"] = (sd, dict(materials=materials), abi.EDIT_MATERIALS | abi.EDIT_RECORDS)
    sd = _matte_sphere_cornell()
    materials = copy.deepcopy(sd.materials)
    materials[2] = dict(kind=abi.MAT_MATTE, a=(0.1, 0.2, 0.7), c=0.0)  # the kinds stay: the table alone
    out["material-colour"] = (sd, dict(materials=materials), abi.EDIT_MATERIALS)
    sd = scenes.glass_balls()
    out["background"] = (sd, dict(background=(0.4, 0.1, 0.3)), abi.EDIT_BACKGROUND)
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", ["lights", "material-kind", "material-colour", "background"])
def test_an_edit_of_the_tables_gives_the_created_scene(yk, contexts, case, layout):
    sd, edit, rewrote = _edits()[case]
    c = contexts(**LAYOUTS[layout])
    edited_sd = copy.copy(sd)
    for k, v in edit.items():
        setattr(edited_sd, k, v)
    created = yk.Scene(c, edited_sd)
    want = _snapshot(created)
    integrators = [yk.IntegratorType.Path(yk.PathParams(max_depth=8))] + ([yk.IntegratorType.Whitted(5)] if sd.name == "cornell" else [])
    want_tiles = [_render(yk, c, created, edited_sd, i) for i in integrators]
    created.close()
    for source in ("host-input", "device-input"):
        s = yk.Scene(c, sd) if source == "host-input" else yk.Scene.from_device(c, sd, _tensors(sd))
        old_tiles = [_render(yk, c, s, sd, i) for i in integrators]
        s.edit(**edit)
        i = s.edit_info()
        assert (i.n_edits, i.reason, i.rewrote) == (1, 0, rewrote), (source, i.rewrote)
        assert not i.rewrote & abi.EDIT_BOXES and i.seconds_boxes == 0.0  # no refit
        got = _snapshot(s)
        if source == "host-input" or layout == "device-laid":  # (device input is always device-built and device-laid)
            _same(got, want)
        for k, (integ, (bits, rays), (old_bits, _)) in enumerate(zip(integrators, want_tiles, old_tiles)):
            got_bits, got_rays = _render(yk, c, s, edited_sd, integ)
            assert got_rays == rays and np.array_equal(got_bits, bits), (source, "Path" if k == 0 else "Whitted")
            assert not np.array_equal(got_bits, old_bits)
        assert s.data is not sd
        s.close()


# ---- 9. device route = host route for sphere moves
@pytest.mark.parametrize("move", ref.MOVES)
@pytest.mark.parametrize("name", ["cornell", "glass_balls"])
def test_device_route_equals_host_route(yk, contexts, name, move):
    for method, max_shapes, wide in ((abi.SPLIT_SAH, 1, 0), (abi.SPLIT_MIDDLE, 4, 2)):
        sd = SCENES[name]()
        sd.split_method, sd.max_shapes_in_node = method, max_shapes
        moved = ref.moved_spheres(sd.spheres, move)
        a = yk.Scene(contexts(scene_layout=0, wide_bvh=wide), sd)
        a.edit(spheres=moved)
        ia = a.edit_info()
        assert (ia.route, ia.reason) == (abi.UPDATE_ROUTE_HOST, 0)
        want = _snapshot(a)
        a.close()
        for given in ("records", "tensor", "side-stream"):
            b = yk.Scene.from_device(contexts(wide_bvh=wide), sd, _tensors(sd))
            before = _snapshot(b)
            if given == "records":
                b.edit(spheres=moved)
            elif given == "tensor":
                b.edit(spheres=_dev_spheres(moved))
            else:  # the table is made on a side stream, behind work
                whole = _dev_spheres(moved).view(torch.int32)
                half_a, half_b = whole // 2, whole - whole // 2
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    busy = torch.ones((2048, 2048), device="cuda:0")
                    for _ in range(8):
                        busy = busy @ busy * (1.0 / 2048.0)
                    table = (half_a + half_b).contiguous()
                b.edit(spheres=table, stream=side)
                assert float(busy[0, 0]) == 1.0
            ib = b.edit_info()
            assert (ib.n_edits, ib.route, ib.reason) == (1, abi.UPDATE_ROUTE_DEVICE, 0), given
            assert ib.rewrote == abi.EDIT_SPHERES | abi.EDIT_BOXES | abi.EDIT_RECORDS
            assert b.layout_info().tree_fetched == 0  # the host copy is stale until something asks
            got = _snapshot(b)
            _same(got, want)
            assert got["tree"] != before["tree"] and got["records"]["nodes"] != before["records"]["nodes"]
            b.edit(spheres=sd.spheres)  # and back: nothing accumulates
            _same(_snapshot(b), before)
            b.close()


# ---- 10. geometry, not self-agreement
@pytest.mark.parametrize("name", ["cornell", "glass_balls"])
def test_the_edited_scene_answers_rays_as_the_moved_geometry_does(yk, oracle, contexts, name):
    sd = SCENES[name]()
    msd = copy.copy(sd)
    msd.spheres = ref.moved_spheres(sd.spheres, "rotation", amount=0.05)
    tracer = trace_ref.TraceRef(msd)
    c = contexts()
    created = yk.Scene(c, msd)
    edited = yk.Scene.from_device(c, sd, _tensors(sd))
    edited.edit(spheres=_dev_spheres(msd.spheres))
    assert edited.edit_info().route == abi.UPDATE_ROUTE_DEVICE
    co, cd = tr.camera_rays(oracle, msd, (40, 30), 5)
    ro, rd = tr.random_rays(msd, 4096, SEED)
    n_hits = 0
    for label, o, d in (("camera", co, cd), ("random 4096", ro, rd)):
        shape_e, t_e = closest_ids(yk, edited, o, d, None, want_t=True)
        shape_c, t_c = closest_ids(yk, created, o, d, None, want_t=True)
        rob, hit = tr.check_closest(tracer, label, o, d, None, shape_e, t_e)
        tr.check_closest(tracer, label, o, d, None, shape_c, t_c)
        decided = tracer.closest(o, d, None)["robust_t"]
        same_shape = tr.canon_shape(tracer, shape_e) == tr.canon_shape(tracer, shape_c)
        assert same_shape[rob].all(), (label, int((~same_shape[rob]).sum()))
        both = decided & (shape_e == shape_c)
        assert np.array_equal(t_e[both].view(np.uint32), t_c[both].view(np.uint32)), label
        n_hits += int(hit.sum())
        diag = float(np.linalg.norm(msd.points.max(axis=0) - msd.points.min(axis=0)))
        tm = np.random.default_rng(SEED + 2).uniform(0.0, 1.5 * diag, len(o)).astype(F)
        al = np.random.default_rng(SEED + 3).integers(-1, max(1, len(msd.lights)), len(o)).astype(np.int32)
        any_e, any_c = edited.any_intersect(o, d, tm, al), created.any_intersect(o, d, tm, al)
        arob = tr.check_any(tracer, label, o, d, tm, al, any_e)
        tr.check_any(tracer, label, o, d, tm, al, any_c)
        assert np.array_equal(np.asarray(any_e).astype(bool)[arob], np.asarray(any_c).astype(bool)[arob]), label
    assert n_hits > 1000
    bits_e, rays_e = _render_tile(yk, c, edited, msd)
    bits_c, rays_c = _render_tile(yk, c, created, msd)
    assert rays_e == rays_c and np.array_equal(bits_e, bits_c)
    edited.close()
    created.close()


# ---- 11. ordering
def test_a_render_enqueued_before_an_edit_sees_the_old_scene(yk, contexts):
    sd = SCENES["glass_balls"]()
    moved = ref.moved_spheres(sd.spheres, "translation", amount=0.08)
    c = contexts()
    b = yk.Scene.from_device(c, sd, _tensors(sd))
    fs = yk.FilmSettings(res=(32, 32), tile_dim=32)
    integ = yk.IntegratorType.instantiate(c, yk.IntegratorType.Path(yk.PathParams(max_depth=8)))
    sampler = yk.SamplerType.Stratified((2, 2), True, LAYOUT_SEED)
    old = torch.zeros((32 * 32, 3), dtype=torch.float32, device="cuda:0")
    out = torch.zeros_like(old)
    table = _dev_spheres(moved)
    torch.cuda.synchronize()
    integ.render_tiles_device(b, yk.Camera(sd.camera, fs), sampler, yk.film_tiles(fs), old.data_ptr())
    assert old.any()
    integ.render_tiles_device(b, yk.Camera(sd.camera, fs), sampler, yk.film_tiles(fs), out.data_ptr(), want_stats=False)
    b.edit(spheres=table, lights=[dict(sd.lights[0], L=(1.0, 1.0, 1.0)), sd.lights[1]], background=(0.5, 0.5, 0.5))
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), old.view(torch.int32))
    integ.render_tiles_device(b, yk.Camera(sd.camera, fs), sampler, yk.film_tiles(fs), out.data_ptr())
    assert not torch.equal(out.view(torch.int32), old.view(torch.int32))
    b.close()


# ---- 12. refusals on the device route
def test_bad_device_tables_are_refused_and_the_records_stay(yk, contexts):
    sd = SCENES["glass_balls"]()
    c = contexts()
    s = yk.Scene.from_device(c, sd, _tensors(sd))
    s.edit(spheres=_dev_spheres(ref.moved_spheres(sd.spheres, "scale")))  # the plan exists: a refusal must not touch it either
    before = _snapshot(s)
    moved = ref.moved_spheres(sd.spheres, "rotation")
    for field, at, value in (("object_to_world", 6, np.nan), ("world_to_object", 0, np.inf), ("radius", None, -np.inf), ("radius", None, np.nan)):
        rec = abi.pack_spheres(moved)
        if at is None:
            rec[field][2] = value
        else:
            rec[field][1, at] = value
        with pytest.raises(_ffi.YukiError) as e:
            s.edit(spheres=torch.from_numpy(rec.view(np.uint8).copy()).to("cuda:0"), background=(9.0, 9.0, 9.0))
        assert e.value.status == 1 and str(e.value).endswith("spheres: matrix entry or radius not finite"), str(e.value)
    for material in (-1, len(sd.materials)):
        rec = abi.pack_spheres(moved)
        rec["material"][0] = material
        with pytest.raises(_ffi.YukiError) as e:
            s.edit(spheres=torch.from_numpy(rec.view(np.uint8).copy()).to("cuda:0"))
        assert e.value.status == 1 and str(e.value).endswith("sphere material out of range"), str(e.value)
    good = _dev_spheres(moved)
    for wrong in (good[:-1].contiguous(), good.double(), good.view(torch.int32)[:-1].contiguous(), good.cpu(), good.view(-1, 8).t()):
        with pytest.raises(ValueError):
            s.edit(spheres=wrong)
    host = abi.pack_spheres(moved)
    with pytest.raises(_ffi.YukiError) as e:
        s.edit(spheres=int(host.ctypes.data))
    assert e.value.status == 1 and str(e.value).endswith("spheres is not device memory of this context's device")
    lights = list(sd.lights)
    lights[1] = dict(kind="distant", w=(0.0, -1.0, 0.0), L=(1.0, 1.0, 1.0))
    with pytest.raises(_ffi.YukiError) as e:
        s.edit(spheres=good, lights=lights)
    assert str(e.value).endswith("lights: a light's kind cannot change")
    assert s.edit_info().n_edits == 1
    _same(_snapshot(s), before)
    bits, _ = _render_tile(yk, c, s, sd)
    s.edit(spheres=good.view(torch.float32))  # the same bytes under another element type
    assert s.edit_info().n_edits == 2 and not np.array_equal(_render_tile(yk, c, s, sd)[0], bits)
    s.close()


# ---- 13. surface_motion with previous spheres
def test_motion_on_the_device_equals_the_host_instance(yk, contexts):
    sd = SCENES["glass_balls"]()
    c = contexts()
    prev = sd.spheres
    moved = ref.moved_spheres(sd.spheres, "rotation", amount=0.05)
    moved[1] = dict(moved[1], radius=float(F(0.07)))
    s = yk.Scene(c, sd)
    s.edit(spheres=moved)
    for res in ((37, 23), (32, 32)):
        fs = yk.FilmSettings(res=res, tile_dim=16)
        guides, ids = yk.render_guides_ids(c, s, yk.Camera(sd.camera, fs), fs)
        points = np.ascontiguousarray(sd.points, F)
        dev = yk.surface_motion(s, ids, guides, points, ctx=c, prev_spheres=prev)
        host = yk.surface_motion(s, ids, guides, points, prev_spheres=prev)
        assert same_bits(dev, host)
        want = ref.surface_motion(ids, guides, sd.indices, points, sd.n_triangles, abi.pack_spheres(moved), abi.pack_spheres(prev))
        assert same_bits(dev, want)
        sph = (ids["shape"] >= sd.n_triangles) & (ids["shape"] != abi.SURFACE_NONE)
        assert sph.sum() > 20 and not same_bits(dev["p_prev"][sph], guides["p"][sph])
        plain = yk.surface_motion(s, ids, guides, points, ctx=c)
        assert same_bits(yk.surface_motion(s, ids, guides, points, ctx=c, prev_spheres=None), plain)
        assert same_bits(plain, yk.surface_motion(s, ids, guides, points)) and same_bits(plain["p_prev"][sph], guides["p"][sph])
        # the _device form, on tensors
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")  # noqa: E731
        d_ids, d_guides, d_points, d_prev = t(ids), t(guides), t(points), _dev_spheres(prev)
        d_out = torch.zeros(res[0] * res[1] * 16, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        c.surface_motion_device(s, d_ids.data_ptr(), d_guides.data_ptr(), d_points.data_ptr(), res, d_out.data_ptr(), d_prev_spheres_ptr=d_prev.data_ptr())
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == dev.tobytes()
    s.close()


# ---- 14. the chain, once
def test_the_history_of_a_moved_sphere_lands_where_float64_says(yk, contexts):
    """glass_balls with matte spheres; sphere 0 slides sideways by 0.03 scene diagonals; the history carries the previous
    frame's positions as its colour.

    The motion records of the moved sphere's pixels are held to the float64 statement within the measured tolerance of
    tests/test_scene_edit.py (profiles/scene_edit_tolerances.json).  The carried colour is a bilinear mix of four previous
    positions ON A CURVED SURFACE: it reproduces a point of the sphere to second order only, h^2 / (2 R) with h the pixel
    footprint — at 32 x 32 the sphere (R = 0.082) is seven pixels across, h = 0.023 and that term is 0.003, a tenth of the
    move (0.029) — so it cannot be held to the float32 tolerance.  The test asks what the geometry allows: with the sphere
    motion the median distance between the carried position and the float64 statement is below a quarter of the move,
    without it (prev_spheres=None, the pass as it was) the same pixels are off by more than three quarters of it."""
    sd = scenes.glass_balls()
    sd.spheres = [dict(s, material=m) for s, m in zip(sd.spheres, (0, 2, 3))]  # white, red and green matte
    diag = float(np.linalg.norm(np.asarray(sd.points).max(axis=0) - np.asarray(sd.points).min(axis=0)))
    a = sd.camera
    side = np.cross(np.subtract(a["target"], a["position"]).astype(np.float64), np.array(a["up"], np.float64))
    move = np.eye(4)
    move[:3, 3] = 0.03 * diag * side / np.linalg.norm(side)
    moved = [ref.transformed(sd.spheres[0], move)] + list(sd.spheres[1:])
    c = contexts()
    s = yk.Scene(c, sd)
    fs = yk.FilmSettings(res=(32, 32), tile_dim=32)
    cam = yk.Camera(sd.camera, fs)
    guides_a, _ = yk.render_guides_ids(c, s, cam, fs)
    history = np.zeros(guides_a.shape, abi.HISTORY_DTYPE)
    history["rgb"], history["n"] = guides_a["p"], guides_a["hit"]
    s.edit(spheres=moved)
    guides_b, ids_b = yk.render_guides_ids(c, s, cam, fs)
    points = np.ascontiguousarray(sd.points, F)
    on_sphere = (ids_b["shape"] == sd.n_triangles) & (guides_b["hit"] != 0)
    assert on_sphere.sum() >= 20
    want = ref.sphere_p_prev64(guides_b["p"][on_sphere], abi.pack_spheres(moved), abi.pack_spheres(sd.spheres), np.zeros(int(on_sphere.sum()), np.int64))
    motion = yk.surface_motion(s, ids_b, guides_b, points, ctx=c, prev_spheres=sd.spheres)
    err = float(np.abs(motion["p_prev"][on_sphere].astype(np.float64) - want).max() / diag)
    print(f"motion records of the moved sphere against float64: {err:.3e} scene diagonals, tolerance {motion_tolerance():.3e}")
    assert err <= motion_tolerance()
    params = yk.TemporalParams.for_scene(s)
    distance = {}
    for label, m in (("with", motion), ("without", yk.surface_motion(s, ids_b, guides_b, points, ctx=c, prev_spheres=None))):
        carried = yk.reproject_history_moved(history, guides_a, cam, guides_b, m, params, ctx=c)
        kept = carried["n"][on_sphere] > 0
        d = np.linalg.norm(carried["rgb"][on_sphere].astype(np.float64) - want, axis=1) / (0.03 * diag)
        distance[label] = (float(np.median(d[kept])) if kept.any() else np.inf, int(kept.sum()))
        print(f"carried positions {label} sphere motion: median {distance[label][0]:.3f} of the move over {distance[label][1]} pixels")
    assert distance["with"][1] >= 10 and distance["with"][0] < 0.25
    assert distance["without"][1] == 0 or distance["without"][0] > 0.75
    s.close()


# ---- 15. the library follows the plan
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", ["cornell", "glass_balls"])
def test_a_scene_on_the_device_follows_the_plan(yk, contexts, name, layout):
    sd = SCENES[name]()
    kind = {"host-laid": "HOST_LAID", "device-laid": "DEVICE_LAID"}[layout]
    s = yk.Scene(contexts(**LAYOUTS[layout]), sd)
    assert s.layout_info().layout == (abi.LAYOUT_DEVICE if layout == "device-laid" else abi.LAYOUT_HOST)
    moved = ref.moved_spheres(sd.spheres, "rotation")
    seen = follow_the_edit_rows(s, sd, kind, {"NONE": None, "SPHERES_HOST": moved, "SPHERES_DEVICE": _dev_spheres(moved)})
    assert {r[:4] for r in seen} == {(kind, b, 1, k) for b in ("NONE", "SPHERES_HOST", "SPHERES_DEVICE") for k in (0, 1)}
    points = wobble(sd, 0.02)
    for brings, given in (("POINTS_HOST", points), ("POINTS_DEVICE", torch.from_numpy(points).to("cuda:0")), ("POINTS_HOST", np.ascontiguousarray(sd.points, F))):
        row = row_of(kind, brings, True, False)
        before = s.update_info().n_updates
        s.update(given)
        i = s.update_info()
        assert (i.n_updates, i.route, i.reason) == (before + 1, {"HOST": abi.UPDATE_ROUTE_HOST, "DEVICE": abi.UPDATE_ROUTE_DEVICE}[row.verdict], 0), (kind, brings, i.route, i.reason)
    s.close()
