"""The pixel-mean albedo on the MI355X (yk_albedo_mean with a context, yk_albedo_mean_device, yk_render_albedo_mean and its
_device form): the reduction equals the host instance bit for bit on the device's own ids of the large film, on device
pointers at 16-byte-offset addresses between guard words and a stream of the caller's; the fused route — the large film
traced in bands and never materialised — equals albedo_mean(render_guides_ids at (s*W, s*H)) bit for bit under the default
band, under three bands with a partial last one, under one row per band and when it is called twice; misaligned and
overlapping buffers, a bad s and a resolution that is too large are refused with nothing launched; the chain (passes,
guides + ids, fused mean albedo, demodulated denoise, tone map) on one torch stream equals the host chain; and the quality
condition of the CPU suite holds on films the device rendered.

Films (output res, s): 37 x 23 with 3 is no multiple of the 32 x 8 block; 64 x 36 with 2 is two blocks wide; 33 x 9 with 4
has one lane in its second block column and one row in its second block row; 1 x 1 with 4 is the smallest; 5 x 3 with 8 is
the largest s."""
import numpy as np
import pytest

import albedo_mean_ref as mref
import albedo_ref as ref
from test_albedo import scene_sources
from test_albedo_mean import quality_ratios
from test_denoise import SEED
from test_gpu_temporal import GUARD, _between_guards, _payload
from test_temporal import same_bits
from yuki_amd import abi

pytestmark = pytest.mark.gpu
F = np.float32
CASES = (((37, 23), 3), ((64, 36), 2), ((33, 9), 4), ((1, 1), 4), ((5, 3), 8))
DEFAULT_BAND_ROWS = 0  # the context's "albedo_mean_band_rows": chosen from the scratch budget


def _where(got, want):
    return np.argwhere(got.view(np.uint32).reshape(got.shape + (4,)) != want.view(np.uint32).reshape(got.shape + (4,)))[:4]


def _big(yk, cam, res, s):
    """(the camera of the s-times larger film, its FilmSettings)"""
    fs = yk.supersampled(yk.FilmSettings(res=res, tile_dim=16), s)
    return yk.Camera(cam, fs), fs


@pytest.fixture(scope="module")
def device_views(ctx, yk, tmp_path_factory):
    """name -> (scene data, camera description, device scene, host-only scene, {(res, s): (the device's ids of the large film,
    the host instance's mean of them)}), computed once and left unchanged."""
    out = {}
    for name, (sd, cam) in scene_sources(tmp_path_factory).items():
        sc, host = yk.Scene(ctx, sd), yk.Scene(None, sd)
        views = {}
        for res, s in CASES if name == "textured-city" else CASES[:1]:
            cam_ss, fs_ss = _big(yk, cam, res, s)
            ids = yk.render_guides_ids(ctx, sc, cam_ss, fs_ss)[1]
            want = yk.albedo_mean(host, ids, s)
            ids.setflags(write=False)
            want.setflags(write=False)
            views[(res, s)] = (ids, want)
        out[name] = (sd, cam, sc, host, views)
    yield out
    for v in out.values():
        v[2].close()
        v[3].close()


def _mean_on_device(torch, ctx, sc, ids, res, s, stream):
    """yk_albedo_mean_device on ids at a 16-byte offset between guard words -> the records, guards checked."""
    w, h = res
    n = w * h
    d_ids, d_out = _between_guards(torch, 4 * n * s * s, 4, ids), _between_guards(torch, 4 * n, 12)
    torch.cuda.synchronize()
    ctx.albedo_mean_device(sc, d_ids.data_ptr() + 16, res, s, d_out.data_ptr() + 48, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(_payload(d_ids, 4, 4 * n * s * s), ids.view(np.uint32).reshape(-1))
    return _payload(d_out, 12, 4 * n).view(abi.ALBEDO_DTYPE).reshape(h, w)


def _fused_on_device(torch, ctx, yk, sc, cam, res, s, stream):
    """yk_render_albedo_mean_device into records at a 16-byte offset between guard words, guards checked."""
    w, h = res
    n = w * h
    d_out = _between_guards(torch, 4 * n, 8)
    torch.cuda.synchronize()
    ctx.render_albedo_mean_device(sc, _big(yk, cam, res, s)[0], res, s, d_out.data_ptr() + 32, stream=stream.cuda_stream)
    stream.synchronize()
    return _payload(d_out, 8, 4 * n).view(abi.ALBEDO_DTYPE).reshape(h, w)


# ------------------------------------------------------------------ the reduction
@pytest.mark.parametrize("case", CASES, ids=[f"{r[0]}x{r[1]}-s{s}" for r, s in CASES])
def test_reduction_device_equals_host(ctx, yk, oracle, device_views, case):
    import torch

    res, s = case
    sd, _, sc, host, views = device_views["textured-city"]
    ids, want = views[case]
    stream = torch.cuda.Stream()
    got = _mean_on_device(torch, ctx, sc, ids, res, s, stream)
    assert same_bits(got, want), (case, _where(got, want))
    assert same_bits(yk.albedo_mean(sc, ids, s, ctx=ctx), want), case  # host buffers, the context's stream
    assert same_bits(got, mref.albedo_mean(ids, s, sd, oracle.texture_eval)), case  # independent of the host instance
    assert np.isin(got["known"], (0.0, 1.0)).all()
    if case == CASES[0]:
        assert same_bits(yk.albedo_mean(sc, ids, s), want)  # the host instance reading the device scene's tables
        assert (got["known"] == 1).sum() > 50 and (got["known"] == 0).sum() > 5


def test_reduction_device_equals_host_on_every_kind(ctx, yk, oracle):
    import torch

    sd = ref.kinds_scene()
    sc, host = yk.Scene(ctx, sd), yk.Scene(None, sd)
    rng = np.random.default_rng(20261023)
    stream = torch.cuda.Stream()
    for res, s in CASES:
        ids = ref.kinds_ids(rng, s * res[0], s * res[1], sd)
        want = yk.albedo_mean(host, ids, s)
        got = _mean_on_device(torch, ctx, sc, ids, res, s, stream)
        assert same_bits(got, want), (res, s, _where(got, want))
        assert same_bits(got, mref.albedo_mean(ids, s, sd, oracle.texture_eval)), (res, s)
    ids = ref.kinds_ids(rng, 37, 23, sd)
    assert same_bits(_mean_on_device(torch, ctx, sc, ids, (37, 23), 1, stream), yk.surface_albedo(host, ids))  # s = 1
    sc.close()
    host.close()


# ------------------------------------------------------------------ the fused route
@pytest.mark.parametrize("name", ["textured-city", "textured-cornell", "textured-pbrt"])
def test_fused_route_equals_reduction_of_the_large_film(ctx, yk, device_views, name):
    import torch

    _, cam, sc, _, views = device_views[name]
    stream = torch.cuda.Stream()
    try:
        for (res, s), (_, want) in views.items():  # the default band
            got = _fused_on_device(torch, ctx, yk, sc, cam, res, s, stream)
            assert same_bits(got, want), (name, res, s, _where(got, want))
        res, s = CASES[0]
        want = views[CASES[0]][1]
        for rows in (8, 1, 8):  # 37 x 23: three bands, the last one of 7 rows; 23 bands; three bands again
            ctx.set_option("albedo_mean_band_rows", rows)
            got = _fused_on_device(torch, ctx, yk, sc, cam, res, s, stream)
            assert same_bits(got, want), (name, rows, _where(got, want))
            got = _fused_on_device(torch, ctx, yk, sc, cam, res, s, stream)  # the same call again: the scratch is reused
            assert same_bits(got, want), (name, rows, "second call", _where(got, want))
        fs = yk.FilmSettings(res=res, tile_dim=16)
        assert same_bits(yk.render_albedo_mean(ctx, sc, cam, fs, s=s), want), name  # host array, the context's stream
        ctx.set_option("albedo_mean_band_rows", DEFAULT_BAND_ROWS)
        assert same_bits(yk.render_albedo_mean(ctx, sc, cam, fs, s=s), want), name
    finally:
        ctx.set_option("albedo_mean_band_rows", DEFAULT_BAND_ROWS)


def test_existing_guide_pass_is_untouched_beside_it(ctx, yk, device_views):
    """yk_render_guides_ids before and after a banded call: the same bytes (the band writer is its own kernel)."""
    _, cam, sc, _, views = device_views["textured-city"]
    res, s = CASES[0]
    cam_ss, fs_ss = _big(yk, cam, res, s)
    try:
        ctx.set_option("albedo_mean_band_rows", 8)
        yk.render_albedo_mean(ctx, sc, cam, yk.FilmSettings(res=res, tile_dim=16), s=s)
    finally:
        ctx.set_option("albedo_mean_band_rows", DEFAULT_BAND_ROWS)
    assert same_bits(yk.render_guides_ids(ctx, sc, cam_ss, fs_ss)[1], views[CASES[0]][0])


# ------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_with_nothing_launched(ctx, yk, device_views):
    import torch

    _, cam, sc, _, _ = device_views["textured-city"]
    w, h, s = 8, 8, 2
    n = w * h
    ids = torch.zeros(4 * n * s * s + 8, dtype=torch.int32, device="cuda:0")
    rec = torch.full((4 * n + 8,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    I, R = ids.data_ptr(), rec.data_ptr()
    bad = [(I + off, R, s) for off in (4, 8, 12)] + [(I, R + off, s) for off in (1, 4, 8, 12)]
    bad += [(I, I, s), (I, I + 16 * n * s * s - 16, s), (R + 16 * n - 16, R, 1), (None, R, s), (I, None, s), (I, R, 0), (I, R, 9)]
    for i, o, ss in bad:
        with pytest.raises(yk.YukiError) as e:
            ctx.albedo_mean_device(sc, i, (w, h), ss, o)
        assert e.value.status == 1, (i, o, ss)
    for res, ss in (((32768, 1), 2), ((1, 32768), 2), ((8192, 2), 8), ((0, 4), 2), ((4, 0), 2)):
        with pytest.raises(yk.YukiError) as e:
            ctx.albedo_mean_device(sc, I, res, ss, R)
        assert e.value.status == 1, (res, ss)
    cam_ss = _big(yk, cam, (w, h), s)[0]
    for o, res, ss in [(R + 4, (w, h), s), (R + 8, (w, h), s), (None, (w, h), s), (R, (w, h), 0), (R, (w, h), 9), (R, (32768, 1), 2), (R, (1, 32768), 2), (R, (0, h), s), (R, (w, 0), s)]:
        with pytest.raises(yk.YukiError) as e:
            ctx.render_albedo_mean_device(sc, cam_ss, res, ss, o)
        assert e.value.status == 1, (o, res, ss)
    with pytest.raises(yk.YukiError) as e:
        yk.check(yk.lib().yk_render_albedo_mean_device(ctx.h, sc.h, None, w, h, s, R, None), ctx.h)  # no camera
    assert e.value.status == 1
    host = yk.Scene(None, ref.minimal_scene())  # a scene that is not on the context's device
    for call in (lambda: ctx.albedo_mean_device(host, I, (w, h), s, R), lambda: ctx.render_albedo_mean_device(host, cam_ss, (w, h), s, R)):
        with pytest.raises(yk.YukiError) as e:
            call()
        assert e.value.status == 1
    host.close()
    for key_value in (-1, 65536):
        with pytest.raises(yk.YukiError):
            ctx.set_option("albedo_mean_band_rows", key_value)
    torch.cuda.synchronize()
    assert np.all(rec.cpu().numpy() == GUARD) and not ids.cpu().numpy().any()  # nothing was launched


# ------------------------------------------------------------------ the chain
def test_the_chain_on_one_torch_stream(ctx, yk):
    """Four accumulating passes of textured-city into a 100 x 60 device film, guides + ids, the fused mean albedo (s = 3, in
    bands of 16 rows), the demodulated denoiser under the film's sample table, the tone map — everything enqueued on one
    torch stream, one synchronisation at the end.  Equals the host instances run on copies, bit for bit."""
    import torch

    sd = ref.textured_city()
    res, s = (100, 60), 3
    n = res[0] * res[1]
    fs = yk.FilmSettings(res=res, tile_dim=16, accumulate=True)
    cam = yk.Camera(sd.camera, fs)
    cam_ss, fs_ss = _big(yk, sd.camera, res, s)
    smp = yk.SamplerType.Stratified((2, 2), True, SEED)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    sc = yk.Scene(ctx, sd)
    tiles = yk.film_tiles(fs)
    lists = [yk.TileList(ctx, tiles, np.full(len(tiles), k, np.uint16)) for k in range(4)]
    samples = yk.film_samples(fs, tiles, np.full(len(tiles), 4, np.uint32))
    td = yk.film_tile_dim(fs)
    params = yk.DenoiseParams.for_scene(sc, iterations=4)
    stream = torch.cuda.Stream()
    z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda:0")  # noqa: E731
    slab, film, guides, ids, albedo, clean = z(lists[0].n_pixels * 3), z(3 * n), z(8 * n), z(4 * n), z(4 * n), z(3 * n)
    torch.cuda.synchronize()
    cs = stream.cuda_stream
    try:
        ctx.set_option("albedo_mean_band_rows", 16)
        yk.render_albedo_mean(ctx, sc, sd.camera, yk.FilmSettings(res=(8, 8), tile_dim=16), s=2)  # the scratch exists before the stream-ordered call
        for tl in lists:
            it.render_tile_list_device(sc, cam, smp, tl, slab.data_ptr(), stream=cs)
            tl.update_film_device(slab.data_ptr(), fs.res, film.data_ptr(), stream=cs, accumulate=True)
        ctx.render_guides_ids_device(sc, cam, res, guides.data_ptr(), ids.data_ptr(), stream=cs)
        ctx.render_albedo_mean_device(sc, cam_ss, res, s, albedo.data_ptr(), stream=cs)
        ctx.denoise_device(film.data_ptr(), guides.data_ptr(), res, params, td, samples, clean.data_ptr(), stream=cs, albedo=albedo.data_ptr())
        ctx.tone_map_device(clean.data_ptr(), res, td, yk.ToneMapType.default(), None, clean.data_ptr(), stream=cs)
        stream.synchronize()
    finally:
        ctx.set_option("albedo_mean_band_rows", DEFAULT_BAND_ROWS)
    host_film = film.cpu().numpy().reshape(res[1], res[0], 3)
    host_guides = guides.cpu().numpy().view(abi.GUIDE_DTYPE).reshape(res[1], res[0])
    assert np.abs(host_film).max() > 0 and 0 < (host_guides["hit"] != 0).sum()
    host_scene = yk.Scene(None, sd)
    ids_ss = yk.render_guides_ids(ctx, sc, cam_ss, fs_ss)[1]
    host_albedo = yk.albedo_mean(host_scene, ids_ss, s)
    centre = yk.surface_albedo(host_scene, ids.cpu().numpy().view(abi.SURFACE_ID_DTYPE).reshape(res[1], res[0]))
    host_scene.close()
    assert same_bits(albedo.cpu().numpy().view(abi.ALBEDO_DTYPE).reshape(res[1], res[0]), host_albedo)
    assert mref.differs(host_albedo, centre).mean() > 0.1  # the mean is not the centre record here
    host_clean = yk.denoise(host_film, host_guides, params, tile_dim=td, samples=samples, albedo=host_albedo)
    assert not np.array_equal(host_clean, yk.denoise(host_film, host_guides, params, tile_dim=td, samples=samples, albedo=centre))
    host_mapped = yk.tone_map(host_clean, yk.ToneMapType.default(), td)
    assert np.array_equal(ref.bits(clean.cpu().numpy()), ref.bits(host_mapped).reshape(-1))
    for tl in lists:
        tl.close()
    sc.close()


# ------------------------------------------------------------------ quality
def test_quality_on_device_films(ctx, yk):
    """The conditions of tests/test_albedo_mean.py::test_quality_on_oracle_films, with the same bounds, on films, guides, ids
    and albedo of the device (the mean by the fused route)."""
    q, mq = ref.QUALITY, mref.QUALITY
    sd = ref.textured_city()
    fs = yk.FilmSettings(res=q["res"], tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    sc = yk.Scene(ctx, sd)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=q["depth"])))
    noisy = yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(q["noisy_spp"], SEED), tiles)[0], fs.res)
    conv = yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(q["converged_spp"], SEED ^ 0x1234567), tiles)[0], fs.res)
    guides, ids1 = yk.render_guides_ids(ctx, sc, cam, fs)
    ids = {1: ids1}
    for s in (2, 4):
        cam_ss, fs_ss = _big(yk, sd.camera, q["res"], s)
        ids[s] = yk.render_guides_ids(ctx, sc, cam_ss, fs_ss)[1]
        assert same_bits(yk.render_albedo_mean(ctx, sc, sd.camera, fs, s=s), yk.albedo_mean(sc, ids[s], s, ctx=ctx)), s
    ratios, share, e_centre = quality_ratios(yk, sc, noisy, conv, guides, ids, q, ctx=ctx)
    sc.close()
    print(f"quality: centre {e_centre:.4f}; mean s=2 {ratios[2][0]:.4f} x (masked {ratios[2][1]:.4f} x), s=4 {ratios[4][0]:.4f} x (masked {ratios[4][1]:.4f} x); mask {share:.3f} of the film")
    assert share > mq["mask_min"], share
    for s in (2, 4):
        assert ratios[s][0] <= mq["whole"][s], (s, ratios[s])
        assert ratios[s][1] <= mq["masked"][s], (s, ratios[s])
