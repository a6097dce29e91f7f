"""The albedo passes on the MI355X (yk_surface_albedo and yk_denoise_albedo with a context, and their _device forms): the
device instances equal the host instances bit for bit on the cases of the CPU suite and on the device's own ids, on device
pointers at offset addresses between guard words and a stream of the caller's; the records equal the numpy restatement on
the device's ids; misaligned and overlapping buffers are refused with nothing launched; the chain (passes, guides + ids,
albedo, demodulated denoise, tone map) on one torch stream equals the host chain; and the quality condition holds on films
the device rendered.

Films: 37 x 23 is no multiple of the 32 x 8 block and narrower than the 2 * s halo of step 16, 64 x 36 is wider than that
halo, 100 x 60 carries a sample table, 1 x 1 is the smallest."""
import ctypes as C

import numpy as np
import pytest

import albedo_ref as ref
import denoise_ref
from test_albedo import FILTER_CASES, _params, scene_sources
from test_denoise import SEED, quality_error
from test_gpu_temporal import GUARD, _between_guards, _payload
from test_temporal import same_bits
from yuki_amd import abi

pytestmark = pytest.mark.gpu
F = np.float32
DEFAULT_LDS_MAX_STEP = 2  # the context's "denoise_lds_max_step" 
DEVICE_SIZES = ((37, 23), (48, 48), (64, 36))


@pytest.fixture(scope="module")
def device_views(ctx, yk, tmp_path_factory):
    """name -> (scene data, device scene, host-only scene, {res: ids of render_guides_ids at the scene's camera})."""
    out = {}
    for name, (sd, cam) in scene_sources(tmp_path_factory).items():
        sc = yk.Scene(ctx, sd)
        views = {}
        for res in DEVICE_SIZES:
            fs = yk.FilmSettings(res=res, tile_dim=16)
            ids = yk.render_guides_ids(ctx, sc, yk.Camera(cam, fs), fs)[1]
            ids.setflags(write=False)
            views[res] = ids
        out[name] = (sd, sc, yk.Scene(None, sd), views)
    yield out
    for v in out.values():
        v[1].close()
        v[2].close()


@pytest.fixture(scope="module")
def kinds(ctx, yk):
    """The scene of every material kind, on the device and host-only, with the synthetic ids of the CPU suite."""
    sd = ref.kinds_scene()
    rng = np.random.default_rng(20261020)
    cases = [ref.kinds_ids(rng, w, h, sd) for w, h in ((64, 36), (37, 23), (1, 1))]
    sc, host = yk.Scene(ctx, sd), yk.Scene(None, sd)
    yield sd, sc, host, cases
    sc.close()
    host.close()


def _albedo_on_device(torch, ctx, sc, ids, stream):
    """yk_surface_albedo_device on ids at a 16-byte offset between guard words -> the records, guards checked."""
    h, w = ids.shape
    n = w * h
    d_ids, d_out = _between_guards(torch, 4 * n, 4, ids), _between_guards(torch, 4 * n, 12)
    torch.cuda.synchronize()
    ctx.surface_albedo_device(sc, d_ids.data_ptr() + 16, (w, h), d_out.data_ptr() + 48, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(_payload(d_ids, 4, 4 * n), ids.view(np.uint32).reshape(-1))
    return _payload(d_out, 12, 4 * n).view(abi.ALBEDO_DTYPE).reshape(h, w)


# ------------------------------------------------------------------ yk_surface_albedo
@pytest.mark.parametrize("name", ["textured-city", "textured-cornell", "textured-pbrt"])
def test_albedo_device_equals_host_and_restatement(ctx, yk, oracle, device_views, name):
    import torch

    sd, sc, host, views = device_views[name]
    s = torch.cuda.Stream()
    for res, ids in views.items():
        want = yk.surface_albedo(host, ids)
        got = _albedo_on_device(torch, ctx, sc, ids, s)
        assert same_bits(got, want), (name, res, np.argwhere(got.view(np.uint32).reshape(got.shape + (4,)) != want.view(np.uint32).reshape(got.shape + (4,)))[:4])
        assert same_bits(yk.surface_albedo(sc, ids, ctx=ctx), want), (name, res)  # host buffers, the context's stream
        assert same_bits(got, ref.surface_albedo(ids, sd, oracle.texture_eval)), (name, res)  # independent of the host instance
        assert (got["known"] == 1).sum() > 50 and ((ids["shape"] == abi.SURFACE_NONE) <= (got["known"] == 0)).all()
    ids = views[(37, 23)]
    assert same_bits(yk.surface_albedo(sc, ids), yk.surface_albedo(host, ids))  # the host instance reading the device scene's tables


def test_albedo_device_equals_host_on_every_kind(ctx, yk, oracle, kinds):
    import torch

    sd, sc, host, cases = kinds
    s = torch.cuda.Stream()
    for ids in cases:
        want = yk.surface_albedo(host, ids)
        got = _albedo_on_device(torch, ctx, sc, ids, s)
        assert same_bits(got, want), (ids.shape, np.argwhere(got.view(np.uint32).reshape(got.shape + (4,)) != want.view(np.uint32).reshape(got.shape + (4,)))[:4])
        assert same_bits(got, ref.surface_albedo(ids, sd, oracle.texture_eval)), ids.shape
        assert same_bits(yk.surface_albedo(sc, ids), want), ids.shape
    # a scene whose arrays are as short as they can be: out-of-range ids select the constant record
    small = ref.minimal_scene()
    sc1 = yk.Scene(ctx, small)
    ids = np.zeros((3, 5), abi.SURFACE_ID_DTYPE)
    ids["shape"] = np.array([1, 2, 0xFFFFFFFE, 0x80000000, ref.SURFACE_NONE], np.uint32)[None, :]
    ids["b"] = F(1.0 / 3.0)
    got = _albedo_on_device(torch, ctx, sc1, ids, s)
    assert (got["a"] == 1).all() and not got["known"].any()
    sc1.close()


def test_misaligned_or_overlapping_buffers_are_refused(ctx, yk, kinds):
    import torch

    sc = kinds[1]
    w, h = 8, 8
    n = w * h
    fill = lambda k, v: torch.full((k + 8,), v, dtype=torch.float32, device="cuda:0")  # noqa: E731
    film, guides, albedo = fill(3 * n, 3.0), fill(8 * n, 2.0), fill(4 * n, 1.0)
    ids = torch.zeros(4 * n + 8, dtype=torch.int32, device="cuda:0")
    rec = torch.full((4 * n + 8,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    I, R, Fm, G, A = (t.data_ptr() for t in (ids, rec, film, guides, albedo))
    bad = [(I + off, R) for off in (4, 8, 12)] + [(I, R + off) for off in (1, 4, 8, 12)] + [(I, I), (I, I + 16), (R + 16 * n - 16, R), (None, R), (I, None)]
    for i, o in bad:
        with pytest.raises(yk.YukiError) as e:
            ctx.surface_albedo_device(sc, i, (w, h), o)
        assert e.value.status == 1
    p = yk.DenoiseParams(iterations=2, sigma_plane=0.06)
    bad = [(Fm + 1, G, A, R), (Fm, G + 4, A, R), (Fm, G, A + 4, R), (Fm, G, A + 8, R), (Fm, G, A, R + 2), (Fm, G, A, A), (Fm, G, A, A + 16 * n - 4), (Fm, G, A, G), (Fm, G, A, Fm + 12), (Fm, G, 0, R)]
    for f, g, a, o in bad:
        with pytest.raises(yk.YukiError) as e:
            if a == 0:
                d = p.as_struct()
                yk.check(yk.lib().yk_denoise_albedo_device(ctx.h, C.byref(d), f, g, None, w, h, 16, None, o, None), ctx.h)
            else:
                ctx.denoise_device(f, g, (w, h), p, 16, None, o, albedo=a)
        assert e.value.status == 1
    torch.cuda.synchronize()
    assert np.all(rec.cpu().numpy() == GUARD)  # nothing was launched
    assert np.all(film.cpu().numpy() == 3.0) and np.all(guides.cpu().numpy() == 2.0) and np.all(albedo.cpu().numpy() == 1.0)


# ------------------------------------------------------------------ yk_denoise_albedo
def _device_filter_cases():
    """The CPU suite's cases with iterations 1, 2 and 5, and a 100 x 60 film under a sample table."""
    out = [c for c in FILTER_CASES if c[4] in (1, 2, 5)]
    rng = np.random.default_rng(20261022)
    w, h = 100, 60
    albedo, guides = ref.make_albedo(rng, w, h), denoise_ref.make_guides(rng, w, h)
    with np.errstate(all="ignore"):
        film = (denoise_ref.make_film(rng, w, h) * np.where(np.isfinite(albedo["a"]), albedo["a"], F(1))).astype(np.float32)
    samples = denoise_ref.make_samples(rng, w, h, 16)
    for it in (1, 2, 5):
        out.append((f"100x60-it{it}-samples", film, guides, albedo, it, denoise_ref.SIGMAS, 16, samples))
    return out


@pytest.fixture(scope="module")
def host_filtered(yk):
    """The host instance on every device case, computed once and left unchanged."""
    out = {}
    for name, film, guides, albedo, it, sig, td, samples in _device_filter_cases():
        r = yk.denoise(film, guides, _params(yk, it, sig), tile_dim=td, samples=samples, albedo=albedo)
        r.setflags(write=False)
        out[name] = r
    return out


@pytest.mark.parametrize("lds_max_step", [0, 1, 2])
def test_denoise_albedo_device_equals_host(ctx, yk, host_filtered, lds_max_step):
    import torch

    s = torch.cuda.Stream()
    ctx.set_option("denoise_lds_max_step", lds_max_step)
    try:
        for name, film, guides, albedo, it, sig, td, samples in _device_filter_cases():
            want = host_filtered[name]
            p = _params(yk, it, sig)
            got = yk.denoise(film, guides, p, tile_dim=td, samples=samples, ctx=ctx, albedo=albedo)
            bad = ref.bits(got) != ref.bits(want)
            assert not bad.any(), (name, lds_max_step, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])
            if "-samples" in name and not name.startswith("100x60"):
                continue
            # device pointers: the film at a 4-byte offset, guides and albedo at 16-byte offsets, out of place then in place
            h, w = guides.shape
            n = w * h
            d_film, d_g, d_a = _between_guards(torch, 3 * n, 1, film), _between_guards(torch, 8 * n, 8, guides), _between_guards(torch, 4 * n, 4, albedo)
            d_out = _between_guards(torch, 3 * n, 3)
            torch.cuda.synchronize()
            ctx.denoise_device(d_film.data_ptr() + 4, d_g.data_ptr() + 32, (w, h), p, td, samples, d_out.data_ptr() + 12, stream=s.cuda_stream, albedo=d_a.data_ptr() + 16)
            ctx.denoise_device(d_film.data_ptr() + 4, d_g.data_ptr() + 32, (w, h), p, td, samples, d_film.data_ptr() + 4, stream=s.cuda_stream, albedo=d_a.data_ptr() + 16)
            s.synchronize()
            assert np.array_equal(_payload(d_out, 3, 3 * n), ref.bits(want).reshape(-1)), (name, lds_max_step)
            assert np.array_equal(_payload(d_film, 1, 3 * n), ref.bits(want).reshape(-1)), (name, lds_max_step, "in place")
            assert np.array_equal(_payload(d_g, 8, 8 * n), guides.view(np.uint32).reshape(-1)) and np.array_equal(_payload(d_a, 4, 4 * n), albedo.view(np.uint32).reshape(-1))
    finally:
        ctx.set_option("denoise_lds_max_step", DEFAULT_LDS_MAX_STEP)


def test_zero_iterations_and_plain_denoise_are_untouched(ctx, yk):
    rng = np.random.default_rng(16)
    film, guides, albedo = denoise_ref.make_film(rng, 37, 23), denoise_ref.make_guides(rng, 37, 23), ref.make_albedo(rng, 37, 23)
    samples = denoise_ref.make_samples(rng, 37, 23, 16)
    p0 = yk.DenoiseParams(iterations=0, sigma_plane=0.06)
    assert np.array_equal(ref.bits(yk.denoise(film, guides, p0, ctx=ctx, albedo=albedo)), ref.bits(film))
    assert np.array_equal(ref.bits(yk.denoise(film, guides, p0, samples=samples, ctx=ctx, albedo=albedo)), ref.bits(denoise_ref.normalise(film, 16, samples)))
    ones = np.zeros((23, 37), abi.ALBEDO_DTYPE)
    ones["a"] = 1.0
    p = yk.DenoiseParams(iterations=3, sigma_plane=0.06)
    assert np.array_equal(ref.bits(yk.denoise(film, guides, p, ctx=ctx, albedo=ones)), ref.bits(yk.denoise(film, guides, p, ctx=ctx)))


# ------------------------------------------------------------------ the chain
def test_the_chain_on_one_torch_stream(ctx, yk):
    """Four accumulating passes of textured-city into a 100 x 60 device film, guides + ids, albedo, the demodulated denoiser
    under the film's sample table, the tone map — everything enqueued on one torch stream, one synchronisation at the end.
    Equals the host instances run on copies, bit for bit."""
    import torch

    sd = ref.textured_city()
    res = (100, 60)
    n = res[0] * res[1]
    fs = yk.FilmSettings(res=res, tile_dim=16, accumulate=True)
    cam = yk.Camera(sd.camera, fs)
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
    for tl in lists:
        it.render_tile_list_device(sc, cam, smp, tl, slab.data_ptr(), stream=cs)
        tl.update_film_device(slab.data_ptr(), fs.res, film.data_ptr(), stream=cs, accumulate=True)
    ctx.render_guides_ids_device(sc, cam, res, guides.data_ptr(), ids.data_ptr(), stream=cs)
    ctx.surface_albedo_device(sc, ids.data_ptr(), res, albedo.data_ptr(), stream=cs)
    ctx.denoise_device(film.data_ptr(), guides.data_ptr(), res, params, td, samples, clean.data_ptr(), stream=cs, albedo=albedo.data_ptr())
    ctx.tone_map_device(clean.data_ptr(), res, td, yk.ToneMapType.default(), None, clean.data_ptr(), stream=cs)
    stream.synchronize()
    host_film = film.cpu().numpy().reshape(res[1], res[0], 3)
    host_guides = guides.cpu().numpy().view(abi.GUIDE_DTYPE).reshape(res[1], res[0])
    host_ids = ids.cpu().numpy().view(abi.SURFACE_ID_DTYPE).reshape(res[1], res[0])
    assert np.abs(host_film).max() > 0 and 0 < (host_guides["hit"] != 0).sum()
    host_scene = yk.Scene(None, sd)
    host_albedo = yk.surface_albedo(host_scene, host_ids)
    host_scene.close()
    assert same_bits(albedo.cpu().numpy().view(abi.ALBEDO_DTYPE).reshape(res[1], res[0]), host_albedo)
    assert len({tuple(a) for a in host_albedo["a"][host_albedo["known"] == 1].reshape(-1, 3)}) > 50  # the texture is in view
    host_clean = yk.denoise(host_film, host_guides, params, tile_dim=td, samples=samples, albedo=host_albedo)
    assert not np.array_equal(host_clean, yk.denoise(host_film, host_guides, params, tile_dim=td, samples=samples))
    host_mapped = yk.tone_map(host_clean, yk.ToneMapType.default(), td)
    assert np.array_equal(ref.bits(clean.cpu().numpy()), ref.bits(host_mapped).reshape(-1))
    for tl in lists:
        tl.close()
    sc.close()


# ------------------------------------------------------------------ quality
def test_quality_on_device_films(ctx, yk):
    """The condition of tests/test_albedo.py::test_quality_on_oracle_films on films, guides, ids and albedo of the device.
    Measured: noisy 0.0970, plain 0.0822, demodulated 0.0590, ratio 0.718."""
    q = ref.QUALITY
    sd = ref.textured_city()
    fs = yk.FilmSettings(res=q["res"], tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    sc = yk.Scene(ctx, sd)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=q["depth"])))
    noisy = yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(q["noisy_spp"], SEED), tiles)[0], fs.res)
    conv = yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(q["converged_spp"], SEED ^ 0x1234567), tiles)[0], fs.res)
    guides, ids = yk.render_guides_ids(ctx, sc, cam, fs)
    albedo = yk.surface_albedo(sc, ids, ctx=ctx)
    p = yk.DenoiseParams.for_scene(sc, iterations=q["iterations"], sigma_color=q["sigma_color"], sigma_normal=q["sigma_normal"])
    plain = yk.denoise(noisy, guides, p, ctx=ctx)
    demod = yk.denoise(noisy, guides, p, ctx=ctx, albedo=albedo)
    e_noisy, e_plain, e_demod = quality_error(noisy, conv), quality_error(plain, conv), quality_error(demod, conv)
    print(f"quality: noisy {e_noisy:.4f} plain {e_plain:.4f} demodulated {e_demod:.4f} ratio {e_demod / e_plain:.3f}")
    assert e_demod <= q["bound"] * e_plain, (e_plain, e_demod)
    sc.close()
