"""The denoiser on the MI355X (yk_denoise with a context, yk_denoise_device, yk_render_guides[_device]): the device
instance equals the host instance bit for bit — every film, guide set, parameter set and sample table of the CPU suite,
under both kernel variants — on device pointers with guard words and in place; the guides equal the oracle's first hits
bit for bit; the whole chain (accumulate, guides, denoise, tone map, present) on one torch stream equals the host chain;
and the quality condition holds on films the device rendered."""
import numpy as np
import pytest

import denoise_ref as ref
from test_denoise import CASES, QUALITY, _params, oracle_guides, quality_error
from yuki_amd import abi, scenes

pytestmark = pytest.mark.gpu
SEED = 0x73B9642E74AC471C
GUARD = 0x5EADBEEF
DEFAULT_LDS_MAX_STEP = 2  # the context's "denoise_lds_max_step" 


@pytest.fixture(scope="module")
def host_results(yk):
    """The host instance on every case, computed once and left unchanged."""
    out = {}
    for name, film, guides, it, sig, td, samples in CASES:
        r = yk.denoise(film, guides, _params(yk, it, sig), tile_dim=td, samples=samples)
        r.setflags(write=False)
        out[name] = r
    return out


@pytest.mark.parametrize("lds_max_step", [0, 1, 2])
def test_device_equals_host_host_buffers(ctx, yk, host_results, lds_max_step):
    ctx.set_option("denoise_lds_max_step", lds_max_step)
    try:
        for name, film, guides, it, sig, td, samples in CASES:
            got = yk.denoise(film, guides, _params(yk, it, sig), tile_dim=td, samples=samples, ctx=ctx)
            bad = ref.bits(got) != ref.bits(host_results[name])
            assert not bad.any(), (name, lds_max_step, int(bad.sum()), np.argwhere(bad)[:4])
    finally:
        ctx.set_option("denoise_lds_max_step", DEFAULT_LDS_MAX_STEP)
    with pytest.raises(yk.YukiError):
        ctx.set_option("denoise_lds_max_step", 3)


def _device_case(torch, film, guides):
    big = torch.zeros(film.size + 2, dtype=torch.float32, device="cuda:0")
    big[1:-1] = torch.from_numpy(film.reshape(-1).copy()).to("cuda:0")
    d_guides = torch.from_numpy(np.ascontiguousarray(guides).view(np.float32).reshape(-1).copy()).to("cuda:0")
    return big, d_guides


def test_device_pointers_offset_film_guard_words_and_in_place(ctx, yk, host_results):
    """yk_denoise_device on torch buffers and a stream of the caller's: the film at a 4-byte offset, the output between two
    guard words that stay intact, then the same run in place; the film (out of place) and the guides are only read."""
    import torch

    s = torch.cuda.Stream()
    for name, film, guides, it, sig, td, samples in CASES:
        if not name.startswith(("37x23", "5x3", "130x70-it5", "130x70-it2", "64x36-it1", "1x1-it1")):
            continue
        h, w, _ = film.shape
        big, d_guides = _device_case(torch, film, guides)
        out = torch.full((film.size + 2,), GUARD, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        p = _params(yk, it, sig)
        ctx.denoise_device(big.data_ptr() + 4, d_guides.data_ptr(), (w, h), p, td, samples, out.data_ptr() + 4, stream=s.cuda_stream)
        s.synchronize()
        o = out.cpu().numpy()
        assert o[0] == GUARD and o[-1] == GUARD, name
        want = ref.bits(host_results[name]).reshape(-1)
        assert np.array_equal(o[1:-1].view(np.uint32), want), name
        b = big.cpu().numpy()
        assert np.array_equal(ref.bits(b[1:-1]), ref.bits(film).reshape(-1)) and b[0] == 0 and b[-1] == 0, name  # the film is only read
        ctx.denoise_device(big.data_ptr() + 4, d_guides.data_ptr(), (w, h), p, td, samples, big.data_ptr() + 4, stream=s.cuda_stream)  # in place
        s.synchronize()
        b = big.cpu().numpy()
        assert np.array_equal(ref.bits(b[1:-1]), want) and b[0] == 0 and b[-1] == 0, name
        assert np.array_equal(d_guides.cpu().numpy().view(np.uint32), np.ascontiguousarray(guides).view(np.uint32).reshape(-1)), name


def test_misaligned_or_overlapping_buffers_are_refused(ctx, yk):
    import torch

    w, h = 8, 8
    film = torch.ones(w * h * 3 + 4, dtype=torch.float32, device="cuda:0")
    guides = torch.full((w * h * 8 + 8,), 2.0, dtype=torch.float32, device="cuda:0")
    out = torch.full((w * h * 3 + 4,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    p = yk.DenoiseParams(iterations=2, sigma_plane=0.06)
    bad = [(film.data_ptr() + off, guides.data_ptr(), out.data_ptr()) for off in (1, 2, 3)]
    bad += [(film.data_ptr(), guides.data_ptr(), out.data_ptr() + off) for off in (1, 2, 3)]
    bad += [(film.data_ptr(), guides.data_ptr() + off, out.data_ptr()) for off in (4, 8, 12)]
    bad += [(film.data_ptr(), guides.data_ptr(), guides.data_ptr() + w * h * 32 - 4)]  # the output starts in the last guide record
    bad += [(film.data_ptr(), guides.data_ptr(), film.data_ptr() + 12)]  # overlaps the film without being equal to it
    for f, g, o in bad:
        with pytest.raises(yk.YukiError) as e:
            ctx.denoise_device(f, g, (w, h), p, 16, None, o)
        assert e.value.status == 1
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == GUARD) and np.all(film.cpu().numpy() == 1.0) and np.all(guides.cpu().numpy() == 2.0)  # nothing was launched


@pytest.mark.parametrize("name,res", [("cornell", (48, 48)), ("city-small", (64, 36)), ("glass-balls", (37, 23))])
def test_guides_equal_the_oracle(ctx, yk, oracle, name, res):
    import torch

    sd = scenes.by_name(name)
    fs = yk.FilmSettings(res=res, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    sc = yk.Scene(ctx, sd)
    want = oracle_guides(oracle, oracle.OracleScene(sd), cam, res)
    got = yk.render_guides(ctx, sc, cam, fs)
    assert got.shape == (res[1], res[0]) and got.dtype == abi.GUIDE_DTYPE
    hits = int((want["hit"] != 0).sum())
    assert 0 < hits and (name == "city-small" or hits < want.size)  # cornell and glass-balls look past their geometry
    for k in ("hit", "ns", "p", "t"):
        assert np.array_equal(ref.bits(got[k]), ref.bits(want[k])), (name, k)
    miss = got["hit"] == 0
    assert not got[miss].view(np.uint32).any()  # misses are all-zero records
    # the device-buffer variant on a stream of the caller's, between guard records
    s = torch.cuda.Stream()
    buf = torch.full(((res[0] * res[1] + 2) * 8,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(yk.YukiError) as e:
        ctx.render_guides_device(sc, cam, res, buf.data_ptr() + 36, stream=s.cuda_stream)  # not 16-byte aligned
    assert e.value.status == 1
    torch.cuda.synchronize()
    assert np.all(buf.cpu().numpy() == GUARD)  # nothing was launched
    ctx.render_guides_device(sc, cam, res, buf.data_ptr() + 32, stream=s.cuda_stream)
    s.synchronize()
    b = buf.cpu().numpy()
    assert np.all(b[:8] == GUARD) and np.all(b[-8:] == GUARD)
    assert np.array_equal(b[8:-8].view(np.uint32), got.view(np.uint32).reshape(-1))
    if name == "city-small":  # a film larger than one batch is chunked the way renders are
        ctx.set_option("batch_paths", 1000)
        try:
            again = yk.render_guides(ctx, sc, cam, fs)
        finally:
            ctx.set_option("batch_paths", 128 << 20)
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    sc.close()


def test_whole_chain_on_one_torch_stream(ctx, yk):
    """Four accumulating passes of city-tiny into a device film, its guides, the denoiser under the film's sample table,
    the tone map and present into a 256 x 256 RGBA8 frame — everything enqueued on one torch stream, one synchronisation
    at the end.  Equals the host instances run on copies, bit for bit."""
    import torch

    sd = scenes.by_name("city-tiny")
    fs = yk.FilmSettings(res=(100, 60), tile_dim=16, accumulate=True)
    cam = yk.Camera(sd.camera, fs)
    smp = yk.SamplerType.Stratified((2, 2), True, SEED)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    sc = yk.Scene(ctx, sd)
    tiles = yk.film_tiles(fs)
    lists = [yk.TileList(ctx, tiles, np.full(len(tiles), k, np.uint16)) for k in range(4)]
    samples = yk.film_samples(fs, tiles, np.full(len(tiles), 4, np.uint32))
    td = yk.film_tile_dim(fs)
    params = yk.DenoiseParams.for_scene(sc, iterations=4)
    window = (256, 256)
    stream = torch.cuda.Stream()
    slab = torch.zeros(lists[0].n_pixels * 3, dtype=torch.float32, device="cuda:0")
    film = torch.zeros(60 * 100 * 3, dtype=torch.float32, device="cuda:0")
    guides = torch.zeros(60 * 100 * 8, dtype=torch.float32, device="cuda:0")
    clean = torch.zeros_like(film)
    frame = torch.full((256 * 256,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for tl in lists:
        it.render_tile_list_device(sc, cam, smp, tl, slab.data_ptr(), stream=stream.cuda_stream)
        tl.update_film_device(slab.data_ptr(), fs.res, film.data_ptr(), stream=stream.cuda_stream, accumulate=True)
    ctx.render_guides_device(sc, cam, fs.res, guides.data_ptr(), stream=stream.cuda_stream)
    ctx.denoise_device(film.data_ptr(), guides.data_ptr(), fs.res, params, td, samples, clean.data_ptr(), stream=stream.cuda_stream)
    ctx.tone_map_device(clean.data_ptr(), fs.res, td, yk.ToneMapType.default(), None, clean.data_ptr(), stream=stream.cuda_stream)  # the denoised film is normalised already
    ctx.present_device(clean.data_ptr(), fs.res, window, 2, "rgba8", frame.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    host_film = film.cpu().numpy().reshape(60, 100, 3)
    host_guides = guides.cpu().numpy().view(abi.GUIDE_DTYPE).reshape(60, 100)
    assert np.abs(host_film).max() > 0 and 0 < (host_guides["hit"] != 0).sum()
    assert np.array_equal(host_guides.view(np.uint32), yk.render_guides(ctx, sc, cam, fs).view(np.uint32))
    host_clean = yk.denoise(host_film, host_guides, params, tile_dim=td, samples=samples)
    assert not np.array_equal(host_clean, host_film / 4)  # the filter did something
    host_mapped = yk.tone_map(host_clean, yk.ToneMapType.default(), td)
    assert np.array_equal(ref.bits(clean.cpu().numpy()), ref.bits(host_mapped).reshape(-1))
    want = yk.present(host_mapped, window)
    got = frame.cpu().numpy().view(np.uint8).reshape(256, 256, 4)
    assert np.array_equal(got, want)
    assert len({tuple(c) for c in got[52:205, :, :3].reshape(-1, 3)}) > 100  # a picture, not one colour
    for tl in lists:
        tl.close()
    sc.close()


def test_quality_on_device_films(ctx, yk):
    q = QUALITY
    sd = scenes.by_name(q["scene"])
    fs = yk.FilmSettings(res=q["res"], tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    sc = yk.Scene(ctx, sd)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=q["depth"])))
    noisy = yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(q["noisy_spp"], SEED), tiles)[0], fs.res)
    conv = yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(q["converged_spp"], SEED ^ 0x1234567), tiles)[0], fs.res)
    guides = yk.render_guides(ctx, sc, cam, fs)
    den = yk.denoise(noisy, guides, yk.DenoiseParams(q["iterations"], q["sigma_color"], q["sigma_normal"], q["sigma_plane"]), ctx=ctx)
    e_noisy, e_den = quality_error(noisy, conv), quality_error(den, conv)
    print(f"quality: noisy {e_noisy:.4f} denoised {e_den:.4f} ratio {e_den / e_noisy:.3f}")
    assert e_den <= q["bound"] * e_noisy, (e_noisy, e_den)
    sc.close()
