"""The motion passes on the MI355X (yk_render_guides_ids, yk_surface_motion, yk_history_reproject_moved with a context and
their _device forms): the ids beside the guides are the oracle's and yk_trace_closest's first hits and recombine to the
guides' points bit for bit; the device instances equal the host instances bit for bit on the cases of the CPU suite, on
device pointers at offset addresses between guard words; misaligned and overlapping buffers are refused with nothing
written; the whole sequence of an update (guides + ids, passes, blend, update, guides + ids, motion, reproject-moved, passes,
blend, denoise, tone map) on one torch stream equals the host chain; and the quality conditions hold on films the device
rendered."""
import ctypes as C

import numpy as np
import pytest

import motion_ref as ref
import temporal_ref
from test_gpu_scene_from_device import SCENES as DEVICE_SCENES
from test_gpu_scene_from_device import _tensors
from test_gpu_temporal import GUARD, _between_guards, _payload
from test_motion import MOTIONS, motion_cases, motion_quality_check, moved_variants, quality_setup, scene_views  # noqa: F401
from test_scene_update import wobble
from test_temporal import SEED, camera, params, reproject_cases, same_bits
from yuki_amd import abi, scenes

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def device_views(ctx, yk):
    """name -> (scene data, device scene, camera, film settings, guides, ids) at the scene's own camera."""
    out = {}
    for name, res in ref.SCENES.items():
        sd = scenes.by_name(name)
        fs = yk.FilmSettings(res=res, tile_dim=16)
        sc = yk.Scene(ctx, sd)
        cam = yk.Camera(sd.camera, fs)
        guides, ids = yk.render_guides_ids(ctx, sc, cam, fs)
        guides.setflags(write=False)
        ids.setflags(write=False)
        out[name] = (sd, sc, cam, fs, guides, ids)
    yield out
    for v in out.values():
        v[1].close()


def _recombined(sd, ids):
    """b over the scene's own points in float32, products first, summed left to right."""
    p = np.ascontiguousarray(sd.points, np.float32)
    i = np.asarray(sd.indices).reshape(-1, 3).astype(np.int64)[ids["shape"].astype(np.int64)]
    b = ids["b"]
    s = (p[i[..., 0]] * b[..., 0:1]).astype(np.float32) + (p[i[..., 1]] * b[..., 1:2]).astype(np.float32)
    return (s.astype(np.float32) + (p[i[..., 2]] * b[..., 2:3]).astype(np.float32)).astype(np.float32)


# ------------------------------------------------------------------ ids
@pytest.mark.parametrize("name", list(ref.SCENES))
def test_ids_are_the_first_hits(ctx, yk, oracle, device_views, name):
    sd, sc, cam, fs, guides, ids = device_views[name]
    w, h = fs.res
    nt = sd.n_triangles
    assert same_bits(guides, yk.render_guides(ctx, sc, cam, fs))
    o, d = oracle.camera_rays(cam.matrices, abi.SamplerDesc(abi.SAMPLER_STRATIFIED, 1, 1, 0, 0), (0, 0, w, h), 0)
    osc = oracle.OracleScene(sd)
    want = osc.intersect(o, d)["shape"].reshape(h, w)
    osc.close()
    traced = sc.intersect(o, d)
    shape = np.where(ids["shape"] == abi.SURFACE_NONE, -1, ids["shape"].astype(np.int64))
    assert np.array_equal(shape, want) and np.array_equal(shape, traced["shape"].reshape(h, w))
    hit = shape >= 0
    assert np.array_equal(hit, guides["hit"] != 0) and hit.any()
    tri = hit & (shape < nt)
    assert tri.sum() > 100
    assert same_bits(ids["b"][tri], traced["bary"].reshape(h, w, 3)[tri])
    assert not ids["b"][~tri].view(np.uint32).any()  # a sphere and a miss carry zeros
    if len(sd.spheres):
        assert (hit & ~tri).any()
    assert same_bits(_recombined(sd, ids[tri]), guides["p"][tri])


def test_either_output_alone(ctx, yk, device_views):
    import torch

    sd, sc, cam, fs, guides, ids = device_views["cornell"]
    w, h = fs.res
    n = w * h
    s = torch.cuda.Stream()
    d_g, d_i = _between_guards(torch, 8 * n, 4), _between_guards(torch, 4 * n, 8)
    only_g, only_i = _between_guards(torch, 8 * n, 12), _between_guards(torch, 4 * n, 4)
    torch.cuda.synchronize()
    ctx.render_guides_ids_device(sc, cam, fs.res, d_g.data_ptr() + 16, d_i.data_ptr() + 32, stream=s.cuda_stream)
    ctx.render_guides_ids_device(sc, cam, fs.res, only_g.data_ptr() + 48, None, stream=s.cuda_stream)
    ctx.render_guides_ids_device(sc, cam, fs.res, None, only_i.data_ptr() + 16, stream=s.cuda_stream)
    s.synchronize()
    want_g, want_i = guides.view(np.uint32).reshape(-1), ids.view(np.uint32).reshape(-1)
    assert np.array_equal(_payload(d_g, 4, 8 * n), want_g) and np.array_equal(_payload(d_i, 8, 4 * n), want_i)
    assert np.array_equal(_payload(only_g, 12, 8 * n), want_g) and np.array_equal(_payload(only_i, 4, 4 * n), want_i)
    only_ids = np.zeros((h, w), abi.SURFACE_ID_DTYPE)
    yk.check(yk.lib().yk_render_guides_ids(ctx.h, sc.h, C.byref(cam.matrices), w, h, None, only_ids.ctypes.data), ctx.h)
    assert same_bits(only_ids, ids)
    # refusals: both NULL, misaligned ids or guides, ids inside the guides — nothing is launched
    G, I = d_g.data_ptr() + 16, d_i.data_ptr() + 32
    for g_ptr, i_ptr in [(None, None), (G, I + 4), (G, I + 8), (G + 4, I), (None, I + 12), (G, G + 16), (I + 16 * n - 16, I)]:
        with pytest.raises(yk.YukiError) as e:
            ctx.render_guides_ids_device(sc, cam, fs.res, g_ptr, i_ptr)
        assert e.value.status == 1
    assert yk.lib().yk_render_guides_ids(ctx.h, sc.h, C.byref(cam.matrices), w, h, None, None) == 1
    torch.cuda.synchronize()
    assert np.array_equal(_payload(d_g, 4, 8 * n), want_g) and np.array_equal(_payload(d_i, 8, 4 * n), want_i)


# ------------------------------------------------------------------ motion
@pytest.mark.parametrize("name", list(ref.SCENES))
def test_motion_device_equals_host(ctx, yk, scene_views, device_views, name):
    """The valid-id cases of the CPU matrix (YK_SURFACE_NONE included, no out-of-range shape): the device instance on host
    buffers, and the host instance reading the device scene's indices, against the host instance on the host-only scene."""
    sd, host_scene, views = scene_views[name]
    sc = device_views[name][1]
    for case, ids, g, prev in motion_cases(sd, views, out_of_range=False):
        assert ((ids["shape"] < sd.n_triangles + len(sd.spheres)) | (ids["shape"] == abi.SURFACE_NONE)).all(), case
        want = yk.surface_motion(host_scene, ids, g, prev)
        assert same_bits(yk.surface_motion(sc, ids, g, prev, ctx=ctx), want), (name, case)
        if case.startswith("37x23"):
            assert same_bits(yk.surface_motion(sc, ids, g, prev), want), (name, case)


def test_motion_device_pointers_offsets_and_guard_words(ctx, yk, scene_views, device_views):
    import torch

    s = torch.cuda.Stream()
    for name in ref.SCENES:
        sd, host_scene, views = scene_views[name]
        sc = device_views[name][1]
        nv = np.asarray(sd.points).shape[0]
        for case, ids, g, prev in motion_cases(sd, views, out_of_range=False):
            if not case.startswith(("37x23", "5x70", "1x1-synthetic")):
                continue
            h, w = g.shape
            n = w * h
            d_ids, d_g, d_p = _between_guards(torch, 4 * n, 4, ids), _between_guards(torch, 8 * n, 8, g), _between_guards(torch, 3 * nv, 1, prev)
            d_out = _between_guards(torch, 4 * n, 12)
            torch.cuda.synchronize()
            ctx.surface_motion_device(sc, d_ids.data_ptr() + 16, d_g.data_ptr() + 32, d_p.data_ptr() + 4, (w, h), d_out.data_ptr() + 48, stream=s.cuda_stream)
            s.synchronize()
            assert np.array_equal(_payload(d_out, 12, 4 * n), yk.surface_motion(host_scene, ids, g, prev).view(np.uint32).reshape(-1)), (name, case)
            assert np.array_equal(_payload(d_ids, 4, 4 * n), ids.view(np.uint32).reshape(-1)) and np.array_equal(_payload(d_g, 8, 8 * n), g.view(np.uint32).reshape(-1)), (name, case)
            assert np.array_equal(_payload(d_p, 1, 3 * nv), prev.view(np.uint32).reshape(-1)), (name, case)


@pytest.mark.parametrize("name", list(ref.SCENES))
def test_the_scenes_own_points_give_the_guides_points(ctx, yk, device_views, name):
    sd, sc, cam, fs, guides, ids = device_views[name]
    m = yk.surface_motion(sc, ids, guides, np.ascontiguousarray(sd.points, np.float32), ctx=ctx)
    hit = guides["hit"] != 0
    assert np.array_equal(m["known"] != 0, hit) and np.all(m["known"][hit] == 1.0)
    assert same_bits(m["p_prev"], guides["p"])  # every hit, spheres included; a miss is zero in both
    hist = temporal_ref.make_history(np.random.default_rng(4), *fs.res)
    tp = yk.TemporalParams.for_scene(sc, normal_cos_min=0.9, max_history=32.0)
    assert same_bits(yk.reproject_history_moved(hist, guides, cam, guides, m, tp, ctx=ctx), yk.reproject_history(hist, guides, cam, guides, tp, ctx=ctx))


# ------------------------------------------------------------------ reproject-moved
def test_reproject_moved_device_equals_host(ctx, yk):
    import torch

    s = torch.cuda.Stream()
    p = params(yk)
    for name, hist, pg, pc, g in reproject_cases():
        h, w = g.shape
        n = w * h
        plain = None
        for kind, m in moved_variants(g).items():
            want = yk.reproject_history_moved(hist, pg, pc, g, m, p)
            assert same_bits(yk.reproject_history_moved(hist, pg, pc, g, m, p, ctx=ctx), want), (name, kind)
            if not name.startswith(("37x23", "5x70-translate", "1x1-same", "64x36-dolly-in")):
                continue
            d_hist, d_pg, d_g, d_m = _between_guards(torch, 4 * n, 4, hist), _between_guards(torch, 8 * n, 8, pg), _between_guards(torch, 8 * n, 12, g), _between_guards(torch, 4 * n, 8, m)
            d_out = _between_guards(torch, 4 * n, 4)
            torch.cuda.synchronize()
            ctx.reproject_history_moved_device(d_hist.data_ptr() + 16, d_pg.data_ptr() + 32, pc, d_g.data_ptr() + 48, d_m.data_ptr() + 32, (w, h), p, d_out.data_ptr() + 16, stream=s.cuda_stream)
            s.synchronize()
            assert np.array_equal(_payload(d_out, 4, 4 * n), want.view(np.uint32).reshape(-1)), (name, kind)
            assert np.array_equal(_payload(d_m, 8, 4 * n), m.view(np.uint32).reshape(-1)) and np.array_equal(_payload(d_g, 12, 8 * n), g.view(np.uint32).reshape(-1)), (name, kind)
            if kind == "same":  # the scene stood: the moved instance is the plain one
                plain = _between_guards(torch, 4 * n, 4)
                torch.cuda.synchronize()
                ctx.reproject_history_device(d_hist.data_ptr() + 16, d_pg.data_ptr() + 32, pc, d_g.data_ptr() + 48, (w, h), p, plain.data_ptr() + 16, stream=s.cuda_stream)
                s.synchronize()
                assert np.array_equal(_payload(plain, 4, 4 * n), want.view(np.uint32).reshape(-1)), name


def test_misaligned_or_overlapping_buffers_are_refused(ctx, yk, device_views):
    import torch

    sd, sc = device_views["cornell"][:2]
    w, h = 8, 8
    n = w * h
    nv = np.asarray(sd.points).shape[0]
    fill = lambda k, v: torch.full((k + 8,), v, dtype=torch.float32, device="cuda:0")  # noqa: E731
    hist, pg, g, m = fill(4 * n, 3.0), fill(8 * n, 2.0), fill(8 * n, 2.0), fill(4 * n, 1.0)
    ids = torch.zeros(4 * n + 8, dtype=torch.int32, device="cuda:0")
    pts = fill(max(3 * nv, 4 * n), 0.5)
    rec = torch.full((4 * n + 8,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    p = params(yk)
    cam = camera(yk, temporal_ref.BASE, (w, h))
    H, P, G, M, I, X, R = (t.data_ptr() for t in (hist, pg, g, m, ids, pts, rec))
    bad = [(H + 4, P, G, M, R), (H, P + 8, G, M, R), (H, P, G + 12, M, R)] + [(H, P, G, M + off, R) for off in (4, 8, 12)] + [(H, P, G, M, R + off) for off in (1, 4, 8, 12)]
    bad += [(H, P, G, M, H), (H, P, G, M, M), (H, P, G, M, M + 16), (H, P, G, R + 16 * n - 16, R), (H, P, G, M, G + 32 * n - 16), (H, P, G, None, R)]
    for a, b, c, mm, o in bad:
        with pytest.raises(yk.YukiError) as e:
            ctx.reproject_history_moved_device(a, b, cam, c, mm, (w, h), p, o)
        assert e.value.status == 1
    bad = [(I + off, G, X, R) for off in (4, 8, 12)] + [(I, G + off, X, R) for off in (4, 8, 12)] + [(I, G, X + off, R) for off in (1, 2, 3)] + [(I, G, X, R + off) for off in (1, 4, 8, 12)]
    bad += [(I, G, X, I), (I, G, X, I + 16), (I, G, X, G + 32 * n - 16), (R + 16 * n - 16, G, X, R), (I, G, R + 16 * n - 16, R), (I, G, X, X), (None, G, X, R), (I, None, X, R), (I, G, None, R), (I, G, X, None)]
    for i, gg, x, o in bad:
        with pytest.raises(yk.YukiError) as e:
            ctx.surface_motion_device(sc, i, gg, x, (w, h), o)
        assert e.value.status == 1
    torch.cuda.synchronize()
    assert np.all(rec.cpu().numpy() == GUARD)  # nothing was launched
    assert np.all(hist.cpu().numpy() == 3.0) and np.all(pg.cpu().numpy() == 2.0) and np.all(g.cpu().numpy() == 2.0) and np.all(m.cpu().numpy() == 1.0) and np.all(pts.cpu().numpy() == 0.5)


# ------------------------------------------------------------------ the whole sequence
@pytest.mark.parametrize("name", ["cornell", "city-tiny"])
def test_an_update_on_one_torch_stream(ctx, yk, name):
    """A device-laid scene at 40 x 24.  Guides + ids at the old geometry, two accumulating passes, blend without history;
    Scene.update(wobbled) with a device tensor; guides + ids, motion from the OLD tensor, reproject-moved, two passes, blend,
    denoise (samples NULL), tone map — everything enqueued on one torch stream, one synchronisation at the end.  Equals the
    host chain run on the device-rendered films, guides and ids, bit for bit."""
    import torch

    sd = DEVICE_SCENES[name]()
    res = (40, 24)
    n = res[0] * res[1]
    fs = yk.FilmSettings(res=res, tile_dim=16, accumulate=True)
    arrays = _tensors(sd)
    old_points = arrays["points"]
    new_host = wobble(sd, 0.01)
    new_points = torch.from_numpy(new_host).to("cuda:0")
    sc = yk.Scene.from_device(ctx, sd, arrays)
    tp = yk.TemporalParams.for_scene(sc, normal_cos_min=0.9, max_history=64.0)
    cam = yk.Camera(sd.camera, fs)
    smp = yk.SamplerType.Stratified((2, 2), True, SEED)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    tiles = yk.film_tiles(fs)
    lists = [yk.TileList(ctx, tiles, np.full(len(tiles), k, np.uint16)) for k in range(2)]
    samples = yk.film_samples(fs, tiles, np.full(len(tiles), 2, np.uint32))
    td = yk.film_tile_dim(fs)
    dparams = yk.DenoiseParams.for_scene(sc, iterations=3)
    stream = torch.cuda.Stream()
    z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda:0")  # noqa: E731
    slab = z(lists[0].n_pixels * 3)
    film_a, film_b, guides_a, guides_b, ids_a, ids_b = z(3 * n), z(3 * n), z(8 * n), z(8 * n), z(4 * n), z(4 * n)
    hist_a, motion, carried, hist_b, rgb, clean = z(4 * n), z(4 * n), z(4 * n), z(4 * n), z(3 * n), z(3 * n)
    torch.cuda.synchronize()
    cs = stream.cuda_stream

    def passes(film):
        for tl in lists:
            it.render_tile_list_device(sc, cam, smp, tl, slab.data_ptr(), stream=cs)
            tl.update_film_device(slab.data_ptr(), fs.res, film.data_ptr(), stream=cs, accumulate=True)

    ctx.render_guides_ids_device(sc, cam, res, guides_a.data_ptr(), ids_a.data_ptr(), stream=cs)
    passes(film_a)
    ctx.blend_history_device(film_a.data_ptr(), res, tp, td, samples, None, hist_a.data_ptr(), None, stream=cs)
    sc.update(new_points, stream=cs)
    ctx.render_guides_ids_device(sc, cam, res, guides_b.data_ptr(), ids_b.data_ptr(), stream=cs)
    ctx.surface_motion_device(sc, ids_b.data_ptr(), guides_b.data_ptr(), old_points.data_ptr(), res, motion.data_ptr(), stream=cs)
    ctx.reproject_history_moved_device(hist_a.data_ptr(), guides_a.data_ptr(), cam, guides_b.data_ptr(), motion.data_ptr(), res, tp, carried.data_ptr(), stream=cs)
    passes(film_b)
    ctx.blend_history_device(film_b.data_ptr(), res, tp, td, samples, carried.data_ptr(), hist_b.data_ptr(), rgb.data_ptr(), stream=cs)
    ctx.denoise_device(rgb.data_ptr(), guides_b.data_ptr(), res, dparams, td, None, clean.data_ptr(), stream=cs)
    ctx.tone_map_device(clean.data_ptr(), res, td, yk.ToneMapType.default(), None, clean.data_ptr(), stream=cs)
    stream.synchronize()
    as_film = lambda t: t.cpu().numpy().reshape(res[1], res[0], 3)  # noqa: E731
    as_rec = lambda t, dt: t.cpu().numpy().view(dt).reshape(res[1], res[0])  # noqa: E731
    h_film_a, h_film_b = as_film(film_a), as_film(film_b)
    h_ga, h_gb, h_ib = as_rec(guides_a, abi.GUIDE_DTYPE), as_rec(guides_b, abi.GUIDE_DTYPE), as_rec(ids_b, abi.SURFACE_ID_DTYPE)
    assert np.abs(h_film_a).max() > 0 and np.abs(h_film_b).max() > 0 and not same_bits(h_ga, h_gb)  # the geometry did move
    assert np.array_equal(as_rec(ids_a, abi.SURFACE_ID_DTYPE)["shape"] == abi.SURFACE_NONE, h_ga["hit"] == 0)
    _, want_hist_a = yk.blend_history(h_film_a, tp, tile_dim=td, samples=samples)
    assert same_bits(as_rec(hist_a, abi.HISTORY_DTYPE), want_hist_a)
    host_scene = yk.Scene(None, sd)
    want_motion = yk.surface_motion(host_scene, h_ib, h_gb, np.ascontiguousarray(sd.points, np.float32))
    host_scene.close()
    assert same_bits(as_rec(motion, abi.MOTION_DTYPE), want_motion)
    hits = h_gb["hit"] != 0
    tri = hits & (h_ib["shape"] < sd.n_triangles)
    assert tri.any() and not same_bits(want_motion["p_prev"][tri], h_gb["p"][tri])  # previous positions, not the current ones
    want_carried = yk.reproject_history_moved(want_hist_a, h_ga, cam, h_gb, want_motion, tp)
    assert same_bits(as_rec(carried, abi.HISTORY_DTYPE), want_carried)
    assert (want_carried["n"][hits] > 0).mean() >= 0.5  # the move keeps most of the film
    want_rgb, want_hist_b = yk.blend_history(h_film_b, tp, tile_dim=td, samples=samples, history=want_carried)
    assert same_bits(as_rec(hist_b, abi.HISTORY_DTYPE), want_hist_b) and same_bits(as_film(rgb), want_rgb)
    host_clean = yk.denoise(want_rgb, h_gb, dparams, tile_dim=td, samples=None)
    assert same_bits(as_film(clean), yk.tone_map(host_clean, yk.ToneMapType.default(), td))
    for tl in lists:
        tl.close()
    sc.close()


# ------------------------------------------------------------------ quality
@pytest.fixture(scope="module")
def device_history(ctx, yk):
    """The 64-spp film and the guides of the OLD geometry on the device, rendered once for both motions."""
    q, sd, fs, _ = quality_setup()
    sc = yk.Scene(ctx, sd)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=q["depth"])))
    film = yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(q["history_spp"], SEED ^ 0x777), tiles)[0], fs.res)
    guides = yk.render_guides(ctx, sc, cam, fs)
    sc.close()
    return film, guides


@pytest.mark.parametrize("name", list(MOTIONS))
def test_quality_on_device_films(ctx, yk, device_history, name):
    q, sd, fs, tparams = quality_setup()
    history_film, prev_guides = device_history
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    old = np.ascontiguousarray(sd.points, np.float32)
    new = MOTIONS[name](sd, tparams.plane_tolerance / 0.01)
    sc = yk.Scene(ctx, sd)
    sc.update(new)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=q["depth"])))

    def render(spp, seed):
        return yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(spp, seed), tiles)[0], fs.res)

    noisy, conv = render(q["noisy_spp"], SEED), render(q["converged_spp"], SEED ^ 0x1234567)
    guides, ids = yk.render_guides_ids(ctx, sc, cam, fs)
    motion = yk.surface_motion(sc, ids, guides, old, ctx=ctx)
    sc.close()
    motion_quality_check(yk, q, name, tparams, history_film, prev_guides, cam, guides, motion, noisy, conv, ctx=ctx)
