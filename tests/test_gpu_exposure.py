"""The exposure meter on the MI355X (yk_film_histogram / yk_exposure_meter with a context, yk_exposure_meter_device,
yk_tone_map_metered_device): the device instance equals the host instance bit for bit — histogram and every field of the
record, vector and scalar paths, with and without a sample table and a window, both settings of "exposure_wave_combine" —
then a film larger than one pass of the grid, the contention films, the metered tone map, and a chain of two frames enqueued
on one torch stream with one synchronisation at the end."""
import dataclasses

import numpy as np
import pytest

import exposure_ref as ref
import tonemap_ref as tmref
from yuki_amd import abi, scenes

pytestmark = pytest.mark.gpu
SEED = 0x73B9642E74AC471C
FIELDS = ("frames", "counted", "skipped", "below", "above")


def _films():
    rng = np.random.default_rng(20261020)
    return [ref.lognormal_film(rng, h, w) for (h, w) in ((23, 37), (16, 16), (5, 1), (1, 1), (150, 200))]


def _same(a, b):
    fb = lambda v: np.array([v], np.float32).view(np.uint32)[0]
    return all(fb(getattr(a, k)) == fb(getattr(b, k)) for k in ("exposure", "log2_adapted", "log2_metered")) and all(getattr(a, k) == getattr(b, k) for k in FIELDS)


def _state_of(words):
    """An ExposureState from eight 32-bit words downloaded from the device."""
    return abi.ExposureState.from_buffer_copy(np.ascontiguousarray(words).tobytes())


def test_device_equals_host_host_buffers(ctx, yk):
    """Films of different sizes one after the other through one context: each gets its own histogram and record — a slot
    left unzeroed between two calls shows here."""
    rng = np.random.default_rng(1)
    for film in _films():
        h, w, _ = film.shape
        for td in (16, 5):
            table = rng.integers(0, 6, size=-(-w // td) * -(-h // td)).astype(np.uint32)
            for samples in (None, table):
                for window in [None] if h * w < 16 else [None, (1, 2, w - 3, h - 1)]:
                    want = yk.film_histogram(film, td, samples=samples, window=window)
                    got = yk.film_histogram(film, td, samples=samples, window=window, ctx=ctx)
                    assert np.array_equal(got[0], want[0]) and got[1] == want[1], (film.shape, td, window)
                    p = yk.ExposureParams(window=window, adapt_up=0.5, adapt_down=0.25)
                    s0 = yk.meter_exposure(film, td, p, samples=samples)
                    d0 = yk.meter_exposure(film, td, p, samples=samples, ctx=ctx)
                    assert _same(d0, s0), (film.shape, td, window)
                    with np.errstate(over="ignore"):
                        bright = (film * np.float32(8.0)).astype(np.float32)
                    assert _same(yk.meter_exposure(bright, td, p, samples=samples, prev=d0, ctx=ctx), yk.meter_exposure(bright, td, p, samples=samples, prev=s0))


def test_device_pointers_offset_guards_and_in_place(ctx, yk):
    """yk_exposure_meter_device on torch buffers: on a stream of the caller's, the film at a 4-byte offset (the scalar path)
    between guard words, the record between guard words and otherwise unwritten before the call; then a second frame whose
    previous record IS the output record."""
    import torch

    rng = np.random.default_rng(2)
    s = torch.cuda.Stream()
    p = yk.ExposureParams(adapt_up=0.5, adapt_down=0.25)
    for film in _films():
        h, w, _ = film.shape
        table = rng.integers(0, 6, size=-(-w // 16) * -(-h // 16)).astype(np.uint32)
        for samples in (None, table):
            for offset in (0, 1):
                big = torch.full((film.size + 5,), 7.0, dtype=torch.float32, device="cuda:0")
                lead = 4 - offset * 3  # offset 0: the film starts 16 bytes in (aligned); offset 1: 4 bytes in
                big[lead : lead + film.size] = torch.from_numpy(film.reshape(-1)).to("cuda:0")
                state = torch.full((10,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
                torch.cuda.synchronize()
                film_ptr, state_ptr = big.data_ptr() + 4 * lead, state.data_ptr() + 4
                ctx.meter_exposure_device(film_ptr, (w, h), 16, p, samples, None, state_ptr, stream=s.cuda_stream)
                s.synchronize()
                words = state.cpu().numpy()
                assert words[0] == 0x5A5A5A5A and words[9] == 0x5A5A5A5A
                want0 = yk.meter_exposure(film, 16, p, samples=samples)
                assert _same(_state_of(words[1:9]), want0), (film.shape, offset)
                darker = (film * np.float32(0.125)).astype(np.float32)
                big[lead : lead + film.size] = torch.from_numpy(darker.reshape(-1)).to("cuda:0")
                torch.cuda.synchronize()
                ctx.meter_exposure_device(film_ptr, (w, h), 16, p, samples, state_ptr, state_ptr, stream=s.cuda_stream)  # in place
                s.synchronize()
                words = state.cpu().numpy()
                assert words[0] == 0x5A5A5A5A and words[9] == 0x5A5A5A5A
                assert _same(_state_of(words[1:9]), yk.meter_exposure(darker, 16, p, samples=samples, prev=want0)), (film.shape, offset)
                guard = big.cpu().numpy()
                assert np.all(guard[:lead] == 7.0) and np.all(guard[lead + film.size :] == 7.0)


def test_film_larger_than_one_pass_extremes_in_the_last_pixels(ctx, yk):
    """2048 x 1100 = 2 252 800 pixels, more than the 2048 x 256 x 4 one pass of the grid covers: a 2^12 pixel, a 2^-12 pixel
    and a NaN in the last three positions — a pass that drops the tail, a block or a stride shows here."""
    rng = np.random.default_rng(4)
    film = np.exp2(rng.uniform(-6.0, 6.0, size=(1100, 2048, 1))).astype(np.float32).repeat(3, axis=2)
    film[-1, -1] = 2.0**12
    film[-1, -2] = 2.0**-12
    film[-1, -3] = np.nan
    want_bins, want_sba = yk.film_histogram(film, 16)
    assert want_sba[0] == 1 and int(want_bins.sum()) == 2048 * 1100 - 1
    for combine in (1, 0):
        ctx.set_option("exposure_wave_combine", combine)
        try:
            got_bins, got_sba = yk.film_histogram(film, 16, ctx=ctx)
            p = yk.ExposureParams(low_cut=0.0, high_cut=0.0)
            got = yk.meter_exposure(film, 16, p, ctx=ctx)
        finally:
            ctx.set_option("exposure_wave_combine", 1)
        assert np.array_equal(got_bins, want_bins) and got_sba == want_sba
        assert _same(got, yk.meter_exposure(film, 16, p))
    top = int(np.flatnonzero(want_bins)[-1])
    assert top == ((int(np.float32(2.0**12).view(np.uint32)) >> 20) - 888) and int(want_bins[top]) == 1


def test_contention_films(ctx, yk):
    """A flat wall (every lane of every wave on one bin), two values by alternate lanes (a lane holds four consecutive
    pixels) and by alternate pixels: exact counts under both settings of "exposure_wave_combine"."""
    h, w = 96, 128
    flat = np.full((h, w, 3), 0.18, np.float32)
    i = np.arange(h * w)
    lanes = np.where((i // 4) % 2 == 0, 0.18, 5.0).astype(np.float32).reshape(h, w, 1).repeat(3, axis=2)
    pixels = np.where(i % 2 == 0, 0.18, 5.0).astype(np.float32).reshape(h, w, 1).repeat(3, axis=2)
    black = np.zeros((h, w, 3), np.float32)  # every lane on the skipped word
    for combine in (1, 0):
        ctx.set_option("exposure_wave_combine", combine)
        try:
            got = [(yk.film_histogram(f, 16, ctx=ctx), yk.meter_exposure(f, 16, ctx=ctx)) for f in (flat, lanes, pixels, black)]
        finally:
            ctx.set_option("exposure_wave_combine", 1)
        for f, ((bins, sba), state) in zip((flat, lanes, pixels, black), got):
            want_bins, want_sba = yk.film_histogram(f, 16)
            assert np.array_equal(bins, want_bins) and sba == want_sba, combine
            assert _same(state, yk.meter_exposure(f, 16)), combine
    assert int(yk.film_histogram(flat, 16, ctx=ctx)[0][107]) == h * w
    assert sorted(int(v) for v in yk.film_histogram(lanes, 16, ctx=ctx)[0] if v) == [h * w // 2, h * w // 2]
    assert yk.film_histogram(black, 16, ctx=ctx)[1] == (h * w, 0, 0)


def test_metered_tone_map(ctx, yk):
    """tone_map_device(exposure_state=) equals the host Filmic at desc.exposure x state.exposure: out of place, in place,
    with and without a sample table, the record produced on the device just before on the same stream."""
    import torch

    rng = np.random.default_rng(6)
    s = torch.cuda.Stream()
    tm = yk.ToneMapType.Filmic(yk.FilmicParams(0.7))
    for film in _films():
        h, w, _ = film.shape
        table = rng.integers(0, 6, size=-(-w // 16) * -(-h // 16)).astype(np.uint32)
        for samples in (None, table):
            state_h = yk.meter_exposure(film, 16, samples=samples)
            want = yk.tone_map(film, tm, 16, samples=samples, exposure_state=state_h)
            src = torch.from_numpy(film.reshape(-1)).to("cuda:0")
            dst = torch.zeros_like(src)
            state = torch.zeros(8, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            ctx.meter_exposure_device(src.data_ptr(), (w, h), 16, None, samples, None, state.data_ptr(), stream=s.cuda_stream)
            ctx.tone_map_device(src.data_ptr(), (w, h), 16, tm, samples, dst.data_ptr(), stream=s.cuda_stream, exposure_state=state.data_ptr())
            ctx.tone_map_device(src.data_ptr(), (w, h), 16, tm, samples, src.data_ptr(), stream=s.cuda_stream, exposure_state=state.data_ptr())  # in place
            s.synchronize()
            assert _same(_state_of(state.cpu().numpy()), state_h)
            assert np.array_equal(tmref.bits(dst.cpu().numpy()), tmref.bits(want).reshape(-1)), film.shape
            assert np.array_equal(tmref.bits(src.cpu().numpy()), tmref.bits(want).reshape(-1)), film.shape
    film = _films()[0]
    src = torch.from_numpy(film.reshape(-1)).to("cuda:0")
    state = torch.zeros(9, dtype=torch.int32, device="cuda:0")
    for bad in (yk.ToneMapType.Heatmap(), yk.ToneMapType.Raw):
        with pytest.raises(yk.YukiError) as e:
            ctx.tone_map_device(src.data_ptr(), (37, 23), 16, bad, None, src.data_ptr(), exposure_state=state.data_ptr())
        assert str(e.value).endswith("yk_tone_map_metered_device: only the Filmic tone map has an exposure")
    with pytest.raises(yk.YukiError) as e:
        ctx.tone_map_device(src.data_ptr(), (37, 23), 16, tm, None, src.data_ptr(), exposure_state=state.data_ptr() + 2)
    assert str(e.value).endswith("yk_tone_map_metered_device: d_state needs 4-byte alignment")


def test_two_frame_chain_on_one_stream(ctx, yk):
    """city-tiny at 100 x 60 under two light levels: render passes -> update_film_device -> meter (previous = the last
    frame's record) -> metered tone map -> present, both frames enqueued on one torch stream, one synchronisation at the
    end.  The records and the window frames equal the host chain's on the downloaded films."""
    import torch

    base = scenes.by_name("city-tiny")

    def lit(scale):
        lights = [dict(l, **{k: tuple(scale * v for v in l[k]) for k in ("L", "I") if k in l}) for l in base.lights]
        return dataclasses.replace(base, lights=lights)

    fs = yk.FilmSettings(res=(100, 60), tile_dim=16, accumulate=True)
    cam = yk.Camera(base.camera, fs)
    smp = yk.SamplerType.Stratified((2, 2), True, SEED)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=4)))
    scs = [yk.Scene(ctx, lit(1.0)), yk.Scene(ctx, lit(0.02))]
    tiles = yk.film_tiles(fs)
    lists = [yk.TileList(ctx, tiles, np.full(len(tiles), k, np.uint16)) for k in range(2)]
    samples = yk.film_samples(fs, tiles, np.full(len(tiles), 2, np.uint32))
    td = yk.film_tile_dim(fs)
    params = yk.ExposureParams(adapt_up=0.5, adapt_down=0.25)
    window = (120, 80)
    stream = torch.cuda.Stream()
    slab = torch.zeros(lists[0].n_pixels * 3, dtype=torch.float32, device="cuda:0")
    films = [torch.zeros(60 * 100 * 3, dtype=torch.float32, device="cuda:0") for _ in scs]
    mapped = torch.zeros_like(films[0])
    states = [torch.zeros(8, dtype=torch.int32, device="cuda:0") for _ in scs]
    frames = [torch.zeros(window[0] * window[1] * 4, dtype=torch.uint8, device="cuda:0") for _ in scs]
    torch.cuda.synchronize()
    for k, sc in enumerate(scs):
        for tl in lists:
            it.render_tile_list_device(sc, cam, smp, tl, slab.data_ptr(), stream=stream.cuda_stream)
            tl.update_film_device(slab.data_ptr(), fs.res, films[k].data_ptr(), stream=stream.cuda_stream, accumulate=True)
        prev = states[k - 1].data_ptr() if k else None
        ctx.meter_exposure_device(films[k].data_ptr(), fs.res, td, params, samples, prev, states[k].data_ptr(), stream=stream.cuda_stream)
        ctx.tone_map_device(films[k].data_ptr(), fs.res, td, yk.ToneMapType.default(), samples, mapped.data_ptr(), stream=stream.cuda_stream, exposure_state=states[k].data_ptr())
        ctx.present_device(mapped.data_ptr(), fs.res, window, abi.PRESENT_ENCODE_SRGB, "rgba8", frames[k].data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    prev = None
    exposures = []
    for k in range(2):
        host_film = films[k].cpu().numpy().reshape(60, 100, 3)
        assert np.abs(host_film).max() > 0
        want = yk.meter_exposure(host_film, td, params, samples=samples, prev=prev)
        assert _same(_state_of(states[k].cpu().numpy()), want), k
        chain = yk.present(yk.tone_map(host_film, yk.ToneMapType.default(), td, samples=samples, exposure_state=want), window, abi.PRESENT_ENCODE_SRGB, "rgba8")
        assert np.array_equal(frames[k].cpu().numpy(), chain.reshape(-1)), k
        prev = want
        exposures.append(want.exposure)
    assert prev.frames == 2 and exposures[1] > exposures[0]  # the darker frame is exposed up, a quarter of the way (adapt_down)
    for tl in lists:
        tl.close()
    for sc in scs:
        sc.close()
