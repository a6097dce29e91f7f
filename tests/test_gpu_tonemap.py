"""The tone map on the MI355X (yk_tone_map with a context, yk_tone_map_device, yk_film_min_max): the device instance equals the
host instance bit for bit — every kind, in place and out of place, with and without a sample table, vector and scalar
paths — and the device reduction equals the host fold; then whole flows: an interrupted accumulation, a device-resident
film tone-mapped on a torch stream with no synchronisation before the end, and `yuki --out` for BVHIntersections."""
import numpy as np
import pytest

import tonemap_ref as ref
from yuki_amd import scenes

pytestmark = pytest.mark.gpu
SEED = 0x73B9642E74AC471C


def _films():
    rng = np.random.default_rng(20261016)
    return [ref.random_film(rng, h, w) for (h, w) in ((23, 37), (16, 16), (1, 5), (40, 64), (150, 200))]


def _kinds(yk, film, td, rng):
    h, w, _ = film.shape
    n = -(-w // td) * -(-h // td)
    samples = rng.integers(0, 6, size=n).astype(np.uint32)
    out = [(yk.ToneMapType.Raw, None)]
    for e in (0.25, 1.0, 8.0):
        out += [(yk.ToneMapType.Filmic(yk.FilmicParams(e)), None), (yk.ToneMapType.Filmic(yk.FilmicParams(e)), samples)]
    for ch in range(4):
        out += [(yk.ToneMapType.Heatmap(yk.HeatmapParams(None, ch)), None), (yk.ToneMapType.Heatmap(yk.HeatmapParams((-1.0, 50.0), ch)), None)]
    return out


def test_device_equals_host_host_buffers(ctx, yk):
    rng = np.random.default_rng(1)
    for film in _films():
        for td in (16, 5):
            for tm, samples in _kinds(yk, film, td, rng):
                ub_h, ub_d = np.zeros(2, np.float32), np.zeros(2, np.float32)
                want = yk.tone_map(film, tm, td, samples=samples, used_bounds=ub_h)
                got = yk.tone_map(film, tm, td, samples=samples, ctx=ctx, used_bounds=ub_d)
                assert np.array_equal(ref.bits(got), ref.bits(want)), (film.shape, td, tm.kind, tm.channel)
                assert ub_h[0] == ub_d[0] and ub_h[1] == ub_d[1]


def test_device_pointers_in_place_out_of_place_and_unaligned(ctx, yk):
    """yk_tone_map_device on torch buffers: out of place, in place, and at a 4-byte offset (the scalar path)."""
    import torch

    rng = np.random.default_rng(2)
    s = torch.cuda.Stream()
    for film in _films():
        h, w, _ = film.shape
        for tm, samples in _kinds(yk, film, 16, rng):
            want = yk.tone_map(film, tm, 16, samples=samples)
            src = torch.from_numpy(film.reshape(-1)).to("cuda:0")
            dst = torch.empty_like(src)
            ctx.tone_map_device(src.data_ptr(), (w, h), 16, tm, samples, dst.data_ptr(), stream=s.cuda_stream)
            s.synchronize()
            assert np.array_equal(ref.bits(dst.cpu().numpy()), ref.bits(want).reshape(-1))
            ctx.tone_map_device(src.data_ptr(), (w, h), 16, tm, samples, src.data_ptr())  # in place, the context's stream
            torch.cuda.synchronize()
            assert np.array_equal(ref.bits(src.cpu().numpy()), ref.bits(want).reshape(-1))
            big = torch.zeros(film.size + 2, dtype=torch.float32, device="cuda:0")
            big[1:-1] = torch.from_numpy(film.reshape(-1)).to("cuda:0")
            torch.cuda.synchronize()
            ctx.tone_map_device(big.data_ptr() + 4, (w, h), 16, tm, samples, big.data_ptr() + 4, stream=s.cuda_stream)
            s.synchronize()
            b = big.cpu().numpy()
            assert b[0] == 0 and b[-1] == 0  # nothing outside the film touched
            assert np.array_equal(ref.bits(b[1:-1]), ref.bits(want).reshape(-1))


def test_device_min_max_equals_host(ctx, yk):
    for film in _films():
        for ch in range(4):
            assert yk.find_min_max(film, ch, ctx=ctx) == yk.find_min_max(film, ch) == ref.min_max(film, ch)
    nan = np.full((9, 11, 3), np.nan, np.float32)
    assert yk.find_min_max(nan, 0, ctx=ctx) == (np.float32(3.4028235e38), np.float32(-3.4028235e38))


def test_4k_extremes_in_the_last_pixels(ctx, yk):
    """3840 x 2160: the minimum, the maximum and a NaN in the last pixels — a reduction that drops the tail, a block or the
    last partial shows here."""
    rng = np.random.default_rng(4)
    film = rng.uniform(0.0, 10.0, size=(2160, 3840, 3)).astype(np.float32)
    film[-1, -1] = (-7.0, -7.0, -7.0)
    film[-1, -2] = (99.0, 99.0, 99.0)
    film[-1, -3] = (np.nan, np.nan, np.nan)
    for ch in range(4):
        lo, hi = yk.find_min_max(film, ch, ctx=ctx)
        assert (lo, hi) == ref.min_max(film, ch)
    assert yk.find_min_max(film, 0, ctx=ctx) == (-7.0, 99.0)
    for tm in (yk.ToneMapType.Heatmap(yk.HeatmapParams()), yk.ToneMapType.default()):
        ub = np.zeros(2, np.float32)
        got = yk.tone_map(film, tm, 16, ctx=ctx, used_bounds=ub)
        assert np.array_equal(ref.bits(got), ref.bits(yk.tone_map(film, tm, 16)))
        if tm.kind == 2:
            assert tuple(ub) == (-7.0, 99.0)


def test_interrupted_accumulation_filmic(ctx, yk):
    """cfg1's scene (Cornell, Whitted 3) at 200 x 120, tile 16 (200 % 16 = 8): three passes over every tile and a fourth over
    some, as an interrupted accumulation leaves the film.  samples from film_samples; device Filmic == host instance."""
    sd = scenes.by_name("cornell")
    fs = yk.FilmSettings(res=(200, 120), tile_dim=16, accumulate=True)
    cam = yk.Camera(sd.camera, fs)
    smp = yk.SamplerType.Uniform(8, SEED)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Whitted(3))
    sc = yk.Scene(ctx, sd)
    tiles = yk.film_tiles(fs)
    film = np.zeros((120, 200, 3), np.float32)
    counts = np.zeros(len(tiles), np.uint32)
    for k in range(3):
        rgb, _ = it.render_tiles_accumulating(sc, cam, smp, tiles, np.full(len(tiles), k, np.uint16))
        yk.accumulate_tiles(tiles, rgb, film, counts)
    extra = np.zeros(7, np.uint32)
    rgb, _ = it.render_tiles_accumulating(sc, cam, smp, tiles[:7], np.full(7, 3, np.uint16))
    yk.accumulate_tiles(tiles[:7], rgb, film, extra)
    counts[:7] += extra
    samples = yk.film_samples(fs, tiles, counts)
    assert set(np.unique(samples)) == {3, 4}
    td = yk.film_tile_dim(fs)
    want = yk.tone_map(film, yk.ToneMapType.default(), td, samples=samples)
    got = yk.tone_map(film, yk.ToneMapType.default(), td, samples=samples, ctx=ctx)
    assert np.array_equal(ref.bits(got), ref.bits(want))
    assert np.array_equal(ref.bits(want), ref.bits(ref.filmic(film, 1.0, td, samples)))
    sc.close()


def test_device_resident_film_on_a_torch_stream(ctx, yk):
    """Render passes into a device film through tile lists, then tone-map it — all enqueued on one torch stream with no
    synchronisation between producer and tone map; one sync at the end.  Equals the host instance on the downloaded film."""
    import torch

    sd = scenes.by_name("city-tiny")
    fs = yk.FilmSettings(res=(100, 60), tile_dim=16, accumulate=True)
    cam = yk.Camera(sd.camera, fs)
    smp = yk.SamplerType.Stratified((2, 2), True, SEED)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    sc = yk.Scene(ctx, sd)
    tiles = yk.film_tiles(fs)
    lists = [yk.TileList(ctx, tiles, np.full(len(tiles), k, np.uint16)) for k in range(2)] + [yk.TileList(ctx, tiles[::3], np.full(len(tiles[::3]), 2, np.uint16))]
    counts = np.full(len(tiles), 2, np.uint32)
    counts[::3] += 1
    samples = yk.film_samples(fs, tiles, counts)
    td = yk.film_tile_dim(fs)
    stream = torch.cuda.Stream()
    slab = torch.zeros(lists[0].n_pixels * 3, dtype=torch.float32, device="cuda:0")
    film = torch.zeros(60 * 100 * 3, dtype=torch.float32, device="cuda:0")
    filmic = torch.zeros_like(film)
    heat = torch.zeros_like(film)
    torch.cuda.synchronize()
    for tl in lists:
        it.render_tile_list_device(sc, cam, smp, tl, slab.data_ptr(), stream=stream.cuda_stream)
        tl.update_film_device(slab.data_ptr(), fs.res, film.data_ptr(), stream=stream.cuda_stream, accumulate=True)
    ctx.tone_map_device(film.data_ptr(), fs.res, td, yk.ToneMapType.default(), samples, filmic.data_ptr(), stream=stream.cuda_stream)
    ctx.tone_map_device(film.data_ptr(), fs.res, td, yk.ToneMapType.Heatmap(yk.HeatmapParams(None, 3)), None, heat.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    host_film = film.cpu().numpy().reshape(60, 100, 3)
    assert np.abs(host_film).max() > 0
    assert np.array_equal(ref.bits(filmic.cpu().numpy()), ref.bits(yk.tone_map(host_film, yk.ToneMapType.default(), td, samples=samples)).reshape(-1))
    want_heat = yk.tone_map(host_film, yk.ToneMapType.Heatmap(yk.HeatmapParams(None, 3)), td)
    assert np.array_equal(ref.bits(heat.cpu().numpy()), ref.bits(want_heat).reshape(-1))
    for tl in lists:
        tl.close()
    sc.close()


def test_bvh_intersections_write_output_default_heatmap(ctx, yk, tmp_path):
    """BVHIntersections of a small scene -> write_output with the default Heatmap (bounds found on the device): the file
    read back equals the host instance applied to the same film."""
    from test_film import read_exr

    sd = scenes.by_name("city-small")
    fs = yk.FilmSettings(res=(72, 40), tile_dim=16)
    sc = yk.Scene(ctx, sd)
    tiles = yk.film_tiles(fs)
    rgb, _ = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.BVHIntersections).render_tiles(sc, yk.Camera(sd.camera, fs), yk.SamplerType.Uniform(1, SEED), tiles)
    film = yk.update_tiles(tiles, rgb, fs.res)
    tm = yk.ToneMapType.Heatmap(yk.HeatmapParams())
    yk.write_output(tmp_path / "heat.exr", film, tm, settings=fs, ctx=ctx)
    want = yk.tone_map(film, tm, yk.film_tile_dim(fs))
    assert np.array_equal(ref.bits(read_exr(tmp_path / "heat.exr")), ref.bits(want))
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 10
    sc.close()
