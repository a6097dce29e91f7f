"""The temporal passes on the MI355X (yk_history_reproject / yk_history_blend with a context and their _device forms): the
device instance equals the host instance bit for bit on every case of the CPU suite; on device pointers at offset
addresses between guard words, and in place; misaligned and overlapping buffers are refused with nothing written; the whole
sequence of a camera move (guides, passes, blend, guides, reproject, passes, blend, denoise, tone map, present) on one torch
stream equals the host chain; and the quality condition holds on films the device rendered."""
import numpy as np
import pytest

import temporal_ref as ref
from test_temporal import COS_MIN, QUALITY, TOL, blend_cases, blend_raw, oracle_views, params, quality_cameras, quality_check, reproject_cases, same_bits  # noqa: F401
from yuki_amd import abi, scenes

pytestmark = pytest.mark.gpu
SEED = 0x73B9642E74AC471C
GUARD = 0x5EADBEEF


@pytest.fixture(scope="module")
def host_reprojected(yk):
    """The host instance on every reproject case, computed once and left unchanged."""
    out = {}
    for name, hist, pg, pc, g in reproject_cases():
        r = yk.reproject_history(hist, pg, pc, g, params(yk))
        r.setflags(write=False)
        out[name] = r
    return out


@pytest.fixture(scope="module")
def host_blended(yk):
    out = {}
    for name, film, td, samples, hist in blend_cases():
        rgb, rec = yk.blend_history(film, params(yk), tile_dim=td, samples=samples, history=hist)
        rgb.setflags(write=False)
        rec.setflags(write=False)
        out[name] = (rgb, rec)
    return out


def test_reproject_device_equals_host_host_buffers(ctx, yk, host_reprojected):
    for name, hist, pg, pc, g in reproject_cases():
        assert same_bits(yk.reproject_history(hist, pg, pc, g, params(yk), ctx=ctx), host_reprojected[name]), name
    name, hist, pg, pc, g = reproject_cases()[ref.SIZES.index((37, 23)) * len(ref.CAMERA_PAIRS) + 1]
    p = params(yk, tol=ref.INF, cos_min=-1.0)
    assert same_bits(yk.reproject_history(hist, pg, pc, g, p, ctx=ctx), yk.reproject_history(hist, pg, pc, g, p)), name


@pytest.mark.parametrize("name", ["cornell", "city-small"])
def test_reproject_device_equals_host_on_oracle_guides(ctx, yk, oracle_views, name):
    ca, ga, cb, gb = oracle_views[name]
    h, w = ga.shape
    hist = ref.make_history(np.random.default_rng(3), w, h)
    tol = 0.01 * float(np.linalg.norm(ga["p"][ga["hit"] != 0].max(0) - ga["p"][ga["hit"] != 0].min(0)))
    for prev_cam, prev_g, cur_g in ((ca, ga, gb), (cb, gb, ga), (ca, ga, ga)):
        got = yk.reproject_history(hist, prev_g, prev_cam, cur_g, params(yk, tol=tol), ctx=ctx)
        assert same_bits(got, yk.reproject_history(hist, prev_g, prev_cam, cur_g, params(yk, tol=tol))), name


def test_blend_device_equals_host_host_buffers(ctx, yk, host_blended):
    p = params(yk)
    for name, film, td, samples, hist in blend_cases():
        want_rgb, want_rec = host_blended[name]
        rgb, rec = yk.blend_history(film, p, tile_dim=td, samples=samples, history=hist, ctx=ctx)
        assert same_bits(rgb, want_rgb) and same_bits(rec, want_rec), name
        only_rgb, _ = blend_raw(yk, film, p, td, samples, hist, want_history=False, ctx=ctx)
        _, only_rec = blend_raw(yk, film, p, td, samples, hist, want_rgb=False, ctx=ctx)
        assert same_bits(only_rgb, want_rgb) and same_bits(only_rec, want_rec), name


def _between_guards(torch, words, lead, data=None):
    """An int32 tensor of `lead` guard words, `words` payload words and 4 guard words; the payload optionally filled."""
    t = torch.full((lead + words + 4,), GUARD, dtype=torch.int32, device="cuda:0")
    if data is not None:
        t[lead : lead + words] = torch.from_numpy(np.ascontiguousarray(data).view(np.int32).reshape(-1).copy()).to("cuda:0")
    return t


def _payload(t, lead, words):
    a = t.cpu().numpy()
    assert np.all(a[:lead] == GUARD) and np.all(a[lead + words :] == GUARD)
    return a[lead : lead + words].view(np.uint32)


def test_device_pointers_offsets_guard_words_and_in_place(ctx, yk, host_reprojected, host_blended):
    """The _device calls on torch buffers and a stream of the caller's: the film at a 4-byte offset, the records and guides
    at 16-byte offsets, every buffer between guard words that stay intact; then blend in place."""
    import torch

    s = torch.cuda.Stream()
    p = params(yk)
    for name, hist, pg, pc, g in reproject_cases():
        if not name.startswith(("37x23", "5x70-translate", "1x1-same", "64x36-dolly-in")):
            continue
        h, w = g.shape
        n = w * h
        d_hist, d_pg, d_g = _between_guards(torch, 4 * n, 4, hist), _between_guards(torch, 8 * n, 8, pg), _between_guards(torch, 8 * n, 12, g)
        d_out = _between_guards(torch, 4 * n, 4)
        torch.cuda.synchronize()
        ctx.reproject_history_device(d_hist.data_ptr() + 16, d_pg.data_ptr() + 32, pc, d_g.data_ptr() + 48, (w, h), p, d_out.data_ptr() + 16, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(_payload(d_out, 4, 4 * n), host_reprojected[name].view(np.uint32).reshape(-1)), name
        assert np.array_equal(_payload(d_hist, 4, 4 * n), hist.view(np.uint32).reshape(-1)), name  # the inputs are only read
        assert np.array_equal(_payload(d_pg, 8, 8 * n), pg.view(np.uint32).reshape(-1)) and np.array_equal(_payload(d_g, 12, 8 * n), g.view(np.uint32).reshape(-1)), name
    for name, film, td, samples, hist in blend_cases():
        if not name.startswith(("37x23", "5x70", "1x1")):
            continue
        h, w = film.shape[:2]
        n = w * h
        want_rgb, want_rec = host_blended[name]
        d_film = _between_guards(torch, 3 * n, 1, film)
        d_hist = None if hist is None else _between_guards(torch, 4 * n, 4, hist)
        d_rec, d_rgb = _between_guards(torch, 4 * n, 8), _between_guards(torch, 3 * n, 3)
        torch.cuda.synchronize()
        hp = None if hist is None else d_hist.data_ptr() + 16
        ctx.blend_history_device(d_film.data_ptr() + 4, (w, h), p, td, samples, hp, d_rec.data_ptr() + 32, d_rgb.data_ptr() + 12, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(_payload(d_rec, 8, 4 * n), want_rec.view(np.uint32).reshape(-1)), name
        assert np.array_equal(_payload(d_rgb, 3, 3 * n), want_rgb.view(np.uint32).reshape(-1)), name
        assert np.array_equal(_payload(d_film, 1, 3 * n), film.view(np.uint32).reshape(-1)), name  # only read
        if hist is None:
            continue
        ctx.blend_history_device(d_film.data_ptr() + 4, (w, h), p, td, samples, hp, hp, d_film.data_ptr() + 4, stream=s.cuda_stream)  # in place
        s.synchronize()
        assert np.array_equal(_payload(d_hist, 4, 4 * n), want_rec.view(np.uint32).reshape(-1)), name
        assert np.array_equal(_payload(d_film, 1, 3 * n), want_rgb.view(np.uint32).reshape(-1)), name


def test_misaligned_or_overlapping_buffers_are_refused(ctx, yk):
    import torch

    w, h = 8, 8
    n = w * h
    film = torch.ones(3 * n + 8, dtype=torch.float32, device="cuda:0")
    hist = torch.full((4 * n + 8,), 3.0, dtype=torch.float32, device="cuda:0")
    pg = torch.full((8 * n + 8,), 2.0, dtype=torch.float32, device="cuda:0")
    g = torch.full((8 * n + 8,), 2.0, dtype=torch.float32, device="cuda:0")
    rec = torch.full((4 * n + 8,), GUARD, dtype=torch.int32, device="cuda:0")
    rgb = torch.full((3 * n + 8,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    p = params(yk)
    cam = yk.Camera(ref.BASE, yk.FilmSettings(res=(w, h), tile_dim=16))
    F, H, P, G, R, C = (t.data_ptr() for t in (film, hist, pg, g, rec, rgb))
    bad = [(H + off, P, G, R) for off in (4, 8, 12)] + [(H, P + off, G, R) for off in (4, 8, 12)] + [(H, P, G + off, R) for off in (4, 8, 12)] + [(H, P, G, R + off) for off in (1, 4, 8, 12)]
    bad += [(H, P, G, H), (H, P, G, H + 16), (H, P, G, P + 32 * n - 16), (H, P, G, G + 32 * n - 16), (R + 16 * n - 16, P, G, R)]
    for a, b, c, o in bad:
        with pytest.raises(yk.YukiError) as e:
            ctx.reproject_history_device(a, b, cam, c, (w, h), p, o)
        assert e.value.status == 1
    bad = [(F + off, H, R, C) for off in (1, 2, 3)] + [(F, H, R, C + off) for off in (1, 2, 3)] + [(F, H + off, R, C) for off in (4, 8, 12)] + [(F, H, R + off, C) for off in (4, 8, 12)]
    bad += [(F, H, None, None), (F, H, H + 16, C), (F, H, R, F + 12), (F, H, F, C), (F, H, R, H), (F, H, R, R + 16 * n - 12)]
    for f, hi, o, r in bad:
        with pytest.raises(yk.YukiError) as e:
            ctx.blend_history_device(f, (w, h), p, 16, None, hi, o, r)
        assert e.value.status == 1
    torch.cuda.synchronize()
    assert np.all(rec.cpu().numpy() == GUARD) and np.all(rgb.cpu().numpy() == GUARD)  # nothing was launched
    assert np.all(film.cpu().numpy() == 1.0) and np.all(hist.cpu().numpy() == 3.0) and np.all(pg.cpu().numpy() == 2.0) and np.all(g.cpu().numpy() == 2.0)


def test_a_camera_move_on_one_torch_stream(ctx, yk):
    """city-small at 64 x 36.  Guides at A, two accumulating passes at A, blend without history; guides at B, reproject, two
    passes at B, blend, denoise (samples NULL), tone map, present — everything enqueued on one torch stream, one
    synchronisation at the end.  Equals the host chain run on the device-rendered films and guides, bit for bit."""
    import torch

    q = QUALITY
    sd = scenes.by_name("city-small")
    res = (64, 36)
    n = res[0] * res[1]
    fs = yk.FilmSettings(res=res, tile_dim=16, accumulate=True)
    sc = yk.Scene(ctx, sd)
    tp = yk.TemporalParams.for_scene(sc, normal_cos_min=q["normal_cos_min"], max_history=q["max_history"])
    cam_a, cam_b = quality_cameras(yk, sd, q, tp.plane_tolerance / 0.01)
    smp = yk.SamplerType.Stratified((2, 2), True, SEED)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    tiles = yk.film_tiles(fs)
    lists = [yk.TileList(ctx, tiles, np.full(len(tiles), k, np.uint16)) for k in range(2)]
    samples = yk.film_samples(fs, tiles, np.full(len(tiles), 2, np.uint32))
    td = yk.film_tile_dim(fs)
    dparams = yk.DenoiseParams.for_scene(sc, iterations=3)
    window = (128, 96)
    stream = torch.cuda.Stream()
    z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda:0")  # noqa: E731
    slab = z(lists[0].n_pixels * 3)
    film_a, film_b, guides_a, guides_b = z(3 * n), z(3 * n), z(8 * n), z(8 * n)
    hist_a, carried, hist_b, rgb, clean = z(4 * n), z(4 * n), z(4 * n), z(3 * n), z(3 * n)
    frame = torch.full((window[0] * window[1],), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    cs = stream.cuda_stream

    def passes(cam, film):
        for tl in lists:
            it.render_tile_list_device(sc, cam, smp, tl, slab.data_ptr(), stream=cs)
            tl.update_film_device(slab.data_ptr(), fs.res, film.data_ptr(), stream=cs, accumulate=True)

    ctx.render_guides_device(sc, cam_a, res, guides_a.data_ptr(), stream=cs)
    passes(cam_a, film_a)
    ctx.blend_history_device(film_a.data_ptr(), res, tp, td, samples, None, hist_a.data_ptr(), None, stream=cs)
    ctx.render_guides_device(sc, cam_b, res, guides_b.data_ptr(), stream=cs)
    ctx.reproject_history_device(hist_a.data_ptr(), guides_a.data_ptr(), cam_a, guides_b.data_ptr(), res, tp, carried.data_ptr(), stream=cs)
    passes(cam_b, film_b)
    ctx.blend_history_device(film_b.data_ptr(), res, tp, td, samples, carried.data_ptr(), hist_b.data_ptr(), rgb.data_ptr(), stream=cs)
    ctx.denoise_device(rgb.data_ptr(), guides_b.data_ptr(), res, dparams, td, None, clean.data_ptr(), stream=cs)
    ctx.tone_map_device(clean.data_ptr(), res, td, yk.ToneMapType.default(), None, clean.data_ptr(), stream=cs)
    ctx.present_device(clean.data_ptr(), res, window, 2, "rgba8", frame.data_ptr(), stream=cs)
    stream.synchronize()
    as_film = lambda t: t.cpu().numpy().reshape(res[1], res[0], 3)  # noqa: E731
    as_guides = lambda t: t.cpu().numpy().view(abi.GUIDE_DTYPE).reshape(res[1], res[0])  # noqa: E731
    as_hist = lambda t: t.cpu().numpy().view(abi.HISTORY_DTYPE).reshape(res[1], res[0])  # noqa: E731
    h_film_a, h_film_b, h_ga, h_gb = as_film(film_a), as_film(film_b), as_guides(guides_a), as_guides(guides_b)
    assert np.abs(h_film_a).max() > 0 and np.abs(h_film_b).max() > 0 and not np.array_equal(h_film_a, h_film_b)
    _, want_hist_a = yk.blend_history(h_film_a, tp, tile_dim=td, samples=samples)
    assert same_bits(as_hist(hist_a), want_hist_a)
    want_carried = yk.reproject_history(want_hist_a, h_ga, cam_a, h_gb, tp)
    assert same_bits(as_hist(carried), want_carried)
    hits = h_gb["hit"] != 0
    assert (want_carried["n"][hits] > 0).mean() >= 0.5  # the move reuses most of the view
    want_rgb, want_hist_b = yk.blend_history(h_film_b, tp, tile_dim=td, samples=samples, history=want_carried)
    assert same_bits(as_hist(hist_b), want_hist_b) and same_bits(as_film(rgb), want_rgb)
    assert np.allclose(want_hist_b["n"][want_carried["n"] > 0], 4.0, rtol=1e-6, atol=0)  # two passes carried over (a bilinear mean of 2s), two new
    host_clean = yk.denoise(want_rgb, h_gb, dparams, tile_dim=td, samples=None)
    host_mapped = yk.tone_map(host_clean, yk.ToneMapType.default(), td)
    assert same_bits(as_film(clean), host_mapped)
    want = yk.present(host_mapped, window)
    got = frame.cpu().numpy().view(np.uint8).reshape(window[1], window[0], 4)
    assert np.array_equal(got, want)
    assert len({tuple(c) for c in got[..., :3].reshape(-1, 3)}) > 100  # a picture, not one colour
    for tl in lists:
        tl.close()
    sc.close()


def test_quality_on_device_films(ctx, yk):
    q = QUALITY
    sd = scenes.by_name(q["scene"])
    fs = yk.FilmSettings(res=q["res"], tile_dim=16)
    sc = yk.Scene(ctx, sd)
    tp = yk.TemporalParams.for_scene(sc, normal_cos_min=q["normal_cos_min"], max_history=q["max_history"])
    cam_a, cam_b = quality_cameras(yk, sd, q, tp.plane_tolerance / 0.01)
    tiles = yk.film_tiles(fs)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=q["depth"])))

    def render(cam, spp, seed):
        return yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(spp, seed), tiles)[0], fs.res)

    history_film = render(cam_a, q["history_spp"], SEED ^ 0x777)
    noisy = render(cam_b, q["noisy_spp"], SEED)
    conv = render(cam_b, q["converged_spp"], SEED ^ 0x1234567)
    quality_check(yk, q, tp, history_film, yk.render_guides(ctx, sc, cam_a, fs), cam_a, yk.render_guides(ctx, sc, cam_b, fs), noisy, conv, ctx=ctx)
    sc.close()
