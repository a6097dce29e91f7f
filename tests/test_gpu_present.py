"""The present pass on the MI355X (yk_present with a context, yk_present_device): the device instance equals the host
instance bit for bit — every film, window, encode and format of the CPU suite — on device pointers with guard words, at
sizes with partial blocks, and at the end of the whole chain (render, tone map, overlay, present) on one torch stream."""
import numpy as np
import pytest

import present_ref as ref
from test_present import WINDOWS, films
from yuki_amd import scenes

pytestmark = pytest.mark.gpu
SEED = 0x73B9642E74AC471C
GUARD = 0x5EADBEEF


def _same(got, want):
    if want.dtype == np.uint8:
        return got.dtype == np.uint8 and np.array_equal(got, want)
    return np.array_equal(ref.bits(got), ref.bits(want))


@pytest.mark.parametrize("encode", [0, 1, 2])
def test_device_equals_host_host_buffers(ctx, yk, encode):
    for film in films():
        for window in WINDOWS:
            for fmt in ("rgba8", "rgb32f"):
                want = yk.present(film, window, encode, fmt)
                got = yk.present(film, window, encode, fmt, ctx=ctx)
                assert _same(got, want), (film.shape, window, encode, fmt)
    ramp = np.repeat(np.geomspace(1e-4, 1e4, 4096, dtype=np.float32)[None, :, None], 3, axis=2)  # logf / expf of the encodes on the device
    assert _same(yk.present(ramp, (4096, 1), encode, "rgb32f", ctx=ctx), yk.present(ramp, (4096, 1), encode, "rgb32f"))
    film = films()[0]
    assert _same(yk.present(film, (37, 23), 0, "rgb32f", ctx=ctx), film)  # the identity keeps every bit on the device too


def _frame_words(window, fmt):
    return window[0] * window[1] * (1 if fmt == "rgba8" else 3)


def test_device_pointers_offset_film_and_guard_words(ctx, yk):
    """yk_present_device on torch buffers and a stream of the caller's: the film at a 4-byte offset, the frame between two
    guard words that must stay as they are."""
    import torch

    s = torch.cuda.Stream()
    for film in films():
        h, w, _ = film.shape
        big = torch.zeros(film.size + 2, dtype=torch.float32, device="cuda:0")
        big[1:-1] = torch.from_numpy(film.reshape(-1)).to("cuda:0")
        for window in ((64, 64), (7, 50), (1, 9), (401, 239)):
            for encode, fmt in ((2, "rgba8"), (0, "rgb32f"), (1, "rgb32f")):
                n = _frame_words(window, fmt)
                out = torch.full((n + 2,), GUARD, dtype=torch.int32, device="cuda:0")
                torch.cuda.synchronize()
                ctx.present_device(big.data_ptr() + 4, (w, h), window, encode, fmt, out.data_ptr() + 4, stream=s.cuda_stream)
                s.synchronize()
                o = out.cpu().numpy()
                assert o[0] == GUARD and o[-1] == GUARD, (film.shape, window, fmt)
                want = yk.present(film, window, encode, fmt)
                got = o[1:-1].view(np.uint8).reshape(want.shape) if fmt == "rgba8" else o[1:-1].view(np.float32).reshape(want.shape)
                assert _same(got, want), (film.shape, window, encode, fmt)
        b = big.cpu().numpy()
        assert np.array_equal(ref.bits(b[1:-1]), ref.bits(film).reshape(-1)) and b[0] == 0 and b[-1] == 0  # the film is only read


def test_misaligned_or_overlapping_frame_is_refused(ctx, yk):
    import torch

    from yuki_amd._ffi import YukiError

    film = torch.ones(8 * 8 * 3, dtype=torch.float32, device="cuda:0")
    out = torch.full((16 * 16 + 2,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for off in (1, 2, 3):
        with pytest.raises(YukiError) as e:
            ctx.present_device(film.data_ptr(), (8, 8), (16, 16), 2, "rgba8", out.data_ptr() + off)
        assert e.value.status == 1
    with pytest.raises(YukiError) as e:
        ctx.present_device(film.data_ptr() + 2, (8, 8), (16, 16), 2, "rgba8", out.data_ptr())
    assert e.value.status == 1
    with pytest.raises(YukiError) as e:
        ctx.present_device(film.data_ptr(), (8, 8), (8, 8), 2, "rgba8", film.data_ptr() + 8 * 8 * 12 - 4)  # overlaps the film's last word
    assert e.value.status == 1
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == GUARD)  # nothing was launched
    assert np.all(film.cpu().numpy() == 1.0)


@pytest.fixture(scope="module")
def film_1080p():
    """A saturated film (every value in [0, 1]), made once and left unchanged."""
    film = np.random.default_rng(31).random((1080, 1920, 3), dtype=np.float32)
    film.setflags(write=False)
    return film


@pytest.mark.parametrize(
    "window,cases",
    [
        ((3840, 2160), ((2, "rgba8"),)),  # the whole window, 15 whole blocks a row
        ((2559, 1441), ((2, "rgba8"), (0, "rgb32f"))),  # odd sizes, one clear row above and below, a partial last block in every row
        ((640, 360), ((2, "rgba8"), (1, "rgb32f"))),  # minification: 2 x 2 taps of a 3 x 3 footprint, no mip levels
    ],
)
def test_tails_1080p(ctx, yk, film_1080p, window, cases):
    assert yk.present_target_rect((1920, 1080), window) == {(3840, 2160): (0, 0, 3840, 2160), (2559, 1441): (0, 1, 2559, 1439), (640, 360): (0, 0, 640, 360)}[window]
    for encode, fmt in cases:
        want = yk.present(film_1080p, window, encode, fmt)
        got = yk.present(film_1080p, window, encode, fmt, ctx=ctx)
        assert _same(got, want), (window, encode, fmt)
        assert np.array_equal(got[-1], want[-1]) and got[..., :3].max() > 0


def test_whole_chain_on_one_torch_stream(ctx, yk):
    """Render city-tiny twice into an accumulating device film, tone-map it, draw BVH level 2 on top and present it into a
    256 x 256 RGBA8 frame — everything enqueued on one torch stream, one synchronisation at the end.  Equals the host
    chain on the downloaded film, byte for byte."""
    import torch

    sd = scenes.by_name("city-tiny")
    fs = yk.FilmSettings(res=(100, 60), tile_dim=16, accumulate=True)
    cam = yk.Camera(sd.camera, fs)
    smp = yk.SamplerType.Stratified((2, 2), True, SEED)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    sc = yk.Scene(ctx, sd)
    tiles = yk.film_tiles(fs)
    lists = [yk.TileList(ctx, tiles, np.full(len(tiles), k, np.uint16)) for k in range(2)]
    samples = yk.film_samples(fs, tiles, np.full(len(tiles), 2, np.uint32))
    td = yk.film_tile_dim(fs)
    boxes = sc.node_bounds(2)
    m = yk.overlay_world_to_clip(sd.camera, fs, sc.node_bounds(0)[0])
    window = (256, 256)
    stream = torch.cuda.Stream()
    slab = torch.zeros(lists[0].n_pixels * 3, dtype=torch.float32, device="cuda:0")
    film = torch.zeros(60 * 100 * 3, dtype=torch.float32, device="cuda:0")
    mapped = torch.zeros_like(film)
    d_boxes = torch.from_numpy(np.ascontiguousarray(boxes).reshape(-1).copy()).to("cuda:0")
    frame = torch.full((256 * 256,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for tl in lists:
        it.render_tile_list_device(sc, cam, smp, tl, slab.data_ptr(), stream=stream.cuda_stream)
        tl.update_film_device(slab.data_ptr(), fs.res, film.data_ptr(), stream=stream.cuda_stream, accumulate=True)
    ctx.tone_map_device(film.data_ptr(), fs.res, td, yk.ToneMapType.default(), samples, mapped.data_ptr(), stream=stream.cuda_stream)
    ctx.draw_overlay_device(mapped.data_ptr(), fs.res, m, None, 0, d_boxes.data_ptr(), len(boxes), stream=stream.cuda_stream)
    ctx.present_device(mapped.data_ptr(), fs.res, window, 2, "rgba8", frame.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    host_film = film.cpu().numpy().reshape(60, 100, 3)
    assert np.abs(host_film).max() > 0
    host_mapped = yk.draw_overlay(yk.tone_map(host_film, yk.ToneMapType.default(), td, samples=samples), m, boxes=boxes)
    assert np.array_equal(ref.bits(mapped.cpu().numpy()), ref.bits(host_mapped).reshape(-1))
    want = yk.present(host_mapped, window)
    got = frame.cpu().numpy().view(np.uint8).reshape(256, 256, 4)
    assert np.array_equal(got, want)
    assert yk.present_target_rect(fs.res, window) == (0, 52, 256, 153)
    assert np.all(got[:52, :, :3] == 0) and np.all(got[205:, :, :3] == 0) and np.all(got[..., 3] == 255)  # letterbox above and below
    assert len({tuple(c) for c in got[52:205, :, :3].reshape(-1, 3)}) > 100  # a picture, not one colour
    for tl in lists:
        tl.close()
    sc.close()
