"""The present pass (ScaleOutput::draw, app/renderpasses/scale_output.rs, as an 8-bit window frame) on the host: the target
rectangles of the reference's arithmetic, the library's host instance against an independent numpy float32 restatement
(tests/present_ref.py) bit for bit, the identity, the border fringe, the quantisation, the PNG writer read back two ways,
write_preview and argument errors.  No GPU."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import present_ref as ref
import tonemap_ref
from yuki_amd import abi

F = np.float32
FILM_SIZES = ((23, 37), (3, 5), (1, 1), (120, 200))  # (h, w)
WINDOWS = ((64, 64), (16, 16), (7, 50), (50, 7), (1, 9), (200, 120), (401, 239))  # (W, H)


def films():
    rng = np.random.default_rng(20261018)
    return [tonemap_ref.random_film(rng, h, w) for (h, w) in FILM_SIZES]


# ------------------------------------------------------------------ the target rectangle
RECTS = [
    ((64, 64), (200, 120), (0, 13, 64, 38)),
    ((16, 16), (37, 23), (0, 4, 16, 9)),
    ((7, 50), (37, 23), (0, 23, 7, 4)),
    ((50, 7), (23, 37), (23, 0, 4, 7)),
    ((100, 61), (200, 120), (0, 1, 100, 60)),  # 61 - 60 is odd: the margin is above
    ((1, 1), (1, 1), (0, 0, 1, 1)),
    ((3840, 2160), (1920, 1080), (0, 0, 3840, 2160)),
    ((65535, 65534), (65534, 65533), (0, 0, 65535, 65534)),
    ((1, 9), (100, 1), (0, 5, 1, 0)),  # empty
    ((9, 1), (1, 100), (4, 0, 0, 1)),  # empty
]


@pytest.mark.parametrize("window,film,want", RECTS)
def test_target_rect(yk, window, film, want):
    assert yk.present_target_rect(film, window) == want
    assert ref.target_rect(film, window) == want


def test_empty_rectangle_is_the_clear_colour(yk):
    for window, res in (((1, 9), (100, 1)), ((9, 1), (1, 100))):
        film = np.ones((res[1], res[0], 3), np.float32)
        frame = yk.present(film, window)
        assert frame.shape == (window[1], window[0], 4)
        assert np.array_equal(frame, np.broadcast_to(np.array([0, 0, 0, 255], np.uint8), frame.shape))
        assert np.array_equal(ref.bits(yk.present(film, window, fmt="rgb32f")), np.zeros((window[1], window[0], 3), np.uint32))


# ------------------------------------------------------------------ host instance == restatement
@pytest.mark.parametrize("encode", [0, 1, 2])
def test_host_equals_restatement(yk, encode):
    for film in films():
        for window in WINDOWS:
            got = yk.present(film, window, encode, "rgb32f")
            want = ref.present(film, window, encode, "rgb32f", yk.host_math)
            assert got.shape == want.shape and got.dtype == np.float32
            assert np.array_equal(ref.bits(got), ref.bits(want)), (film.shape, window, encode)
            got8 = yk.present(film, window, encode, "rgba8")
            want8 = ref.present(film, window, encode, "rgba8", yk.host_math)
            assert got8.dtype == np.uint8 and np.array_equal(got8, want8), (film.shape, window, encode)


def test_identity_keeps_every_bit(yk):
    """Window == film, no encode: every weight is zero, so the film's bits come through, NaN payloads and -0 included."""
    for film in films():
        film = film.copy()
        v = film.reshape(-1).view(np.uint32)
        v[:: 7] = 0x7FA12345  # a signalling NaN with a payload
        v[3:: 11] = 0xFFC00001
        v[5:: 13] = 0x80000000  # -0
        h, w, _ = film.shape
        got = yk.present(film, (w, h), 0, "rgb32f")
        assert np.array_equal(ref.bits(got), ref.bits(film))


def test_border_fringe(yk):
    """BorderClamp with the (0, 0, 0) border: a magnified film fades by half a texel at the rectangle's edge."""
    got = yk.present(np.ones((2, 2, 3), np.float32), (4, 4), 0, "rgb32f")
    wgt = np.array([0.75, 1.0, 1.0, 0.75], np.float32)
    want = np.broadcast_to((wgt[:, None] * wgt[None, :])[..., None], (4, 4, 3))
    assert np.array_equal(got, want)
    assert got[0, 0, 0] == F(0.5625) and got[3, 3, 2] == F(0.5625)


def test_integer_magnification_has_exact_weights(yk):
    """Each texel of a 3 x 2 film covers 4 x 4 pixels of a 12 x 8 window: weights are multiples of 1/8, exact."""
    film = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    got = yk.present(film, (12, 8), 0, "rgb32f")
    assert np.array_equal(ref.bits(got), ref.bits(ref.present(film, (12, 8), 0, "rgb32f", yk.host_math)))
    # window column 5: n = (2*5 + 1)*3 - 12 = 21, d = 24 -> tap 0, weight 21/24 for tap 1
    # row 3: n = (2*3 + 1)*2 - 8 = 6, d = 16 -> tap 0, weight 6/16
    top = film[0, 0] * F(1 - 21 / 24) + film[0, 1] * F(21 / 24)
    bot = film[1, 0] * F(1 - 21 / 24) + film[1, 1] * F(21 / 24)
    want = top * F(1 - 6 / 16) + bot * F(6 / 16)
    assert np.array_equal(got[3, 5], want.astype(np.float32))


def test_a_tap_of_weight_zero_is_not_read(yk):
    """A 2 x 2 film whose second column is NaN, magnified 3 times: the centre pixel of a texel has weight zero for its
    neighbour (n = (2*1 + 1)*2 - 6 = 0), so column 1 stays clean although its neighbour tap is NaN."""
    film = np.ones((2, 2, 3), np.float32)
    film[:, 1] = np.nan
    got = yk.present(film, (6, 6), 0, "rgb32f")
    assert np.array_equal(np.isnan(got[..., 0]), np.broadcast_to(np.array([False, False, True, True, True, True]), (6, 6)))
    assert got[1, 1, 0] == 1.0 and got[0, 0, 0] == F(8 / 12) * F(8 / 12)
    assert np.array_equal(ref.bits(got), ref.bits(ref.present(film, (6, 6), 0, "rgb32f", yk.host_math)))


# ------------------------------------------------------------------ the frame buffer
def _one(yk, v, encode):
    return yk.present(np.full((1, 1, 3), v, np.float32), (1, 1), encode, "rgba8")[0, 0]


def test_quantisation(yk):
    for v, want in ((0.0, 0), (1.0, 255), (0.5, 128), (0.2, 51), (0.0031308, 1), (-1.0, 0), (2.0, 255), (np.inf, 255), (np.nan, 0)):
        px = _one(yk, v, 0)
        assert tuple(px) == (want, want, want, 255), (v, px)
    assert tuple(ref.quantise(np.array([0.0, 1.0, 0.5, 0.2, 0.0031308, -1.0, 2.0, np.inf, np.nan], np.float32))) == (0, 255, 128, 51, 1, 0, 255, 255, 0)


def test_srgb_encode_is_monotone_and_anchored(yk):
    x = np.linspace(0.0, 1.0, 4096, dtype=np.float32)
    film = np.repeat(x[None, :, None], 3, axis=2)
    f = yk.present(film, (4096, 1), 2, "rgb32f")[0, :, 0]
    assert f[0] == 0.0 and f[-1] == 1.0 and np.all(np.diff(f) >= 0)
    q = yk.present(film, (4096, 1), 2, "rgba8")[0, :, 0].astype(np.int32)
    assert q[0] == 0 and q[-1] == 255 and np.all(np.diff(q) >= 0) and len(np.unique(q)) == 256
    # against the sRGB transfer function in float64.  The exponent 0.41666 is 6.7e-6 below 1/2.4 and |d/dp x^p| = |x^p ln x|
    # <= 1/(e p) = 0.88, so the curve moves by at most 1.055 * 0.88 * 6.7e-6 = 6.2e-6; float32 rounding adds under 1e-6.
    x64 = x.astype(np.float64)
    exact = np.where(x64 < 0.0031308, 12.92 * x64, 1.055 * x64 ** (1 / 2.4) - 0.055)
    assert np.abs(f - exact).max() < 1e-5
    for v in (-1.0, -np.inf, np.nan, -0.0):
        assert tuple(yk.present(np.full((1, 1, 3), v, np.float32), (1, 1), 2, "rgb32f")[0, 0]) == (0.0, 0.0, 0.0)
    assert tuple(yk.present(np.full((1, 1, 3), np.inf, np.float32), (1, 1), 2, "rgb32f")[0, 0]) == (1.0, 1.0, 1.0)
    # the shader's own curve (gamma 2.2) differs from the back buffer's
    g = yk.present(film, (4096, 1), 1, "rgb32f")[0, :, 0]
    exact = np.where(x64 <= 0.0031308, 12.92 * x64, 1.055 * x64 ** (1 / 2.2) - 0.055)
    assert np.abs(g - exact).max() < 1e-5 and np.abs(g - f).max() > 0.01


# ------------------------------------------------------------------ PNG
def read_png(path):
    """An independent reader: chunk walk with CRC check, zlib.decompress, filter type 0 only."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        (n,) = struct.unpack(">I", data[at : at + 4])
        kind, body = data[at + 4 : at + 8], data[at + 8 : at + 8 + n]
        (crc,) = struct.unpack(">I", data[at + 8 + n : at + 12 + n])
        assert zlib.crc32(kind + body) == crc, kind
        chunks.append((kind, body))
        at += 12 + n
    assert at == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, flt, lace) == (8, 0, 0, 0) and colour in (2, 6)
    ch = 3 if colour == 2 else 4
    raw = zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT"))  # checks the Adler-32
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * ch)
    assert np.all(rows[:, 0] == 0)
    return rows[:, 1:].reshape(h, w, ch)


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("size", [(1, 1), (37, 23), (300, 200)])  # (w, h); the last needs more than one stored block
def test_write_png_reads_back(yk, tmp_path, channels, size):
    from yuki_amd import loaders

    rng = np.random.default_rng(9)
    px = rng.integers(0, 256, size=(size[1], size[0], channels), dtype=np.uint8)
    path = tmp_path / "frame.png"
    yk.write_png(path, px)
    assert np.array_equal(read_png(path), px)
    tex = loaders.load_image_texture(path)  # the library's own decoder: c / 255, alpha dropped
    assert tex.shape == (size[1], size[0], 3)
    assert np.array_equal(np.rint(tex * F(255)).astype(np.uint8), px[..., :3])
    assert np.array_equal(tex, px[..., :3].astype(np.float32) / F(255))


def test_write_preview(yk, tmp_path):
    film = np.abs(tonemap_ref.random_film(np.random.default_rng(5), 27, 48, specials=False))
    fs = yk.FilmSettings(res=(48, 27), tile_dim=16)
    yk.write_preview(tmp_path / "a.png", film, settings=fs)
    mapped = yk.tone_map(film, yk.ToneMapType.default(), yk.film_tile_dim(fs))
    want = yk.present(mapped, (48, 27))
    assert np.array_equal(read_png(tmp_path / "a.png"), want)
    assert len(np.unique(want[..., :3])) > 50 and np.all(want[..., 3] == 255)
    assert np.array_equal(want, ref.present(tonemap_ref.filmic(film, 1.0), (48, 27), 2, "rgba8", yk.host_math))
    yk.write_preview(tmp_path / "b.png", film, yk.ToneMapType.Filmic(yk.FilmicParams(2.0)), settings=fs, window=(100, 100))
    mapped = yk.tone_map(film, yk.ToneMapType.Filmic(yk.FilmicParams(2.0)), 16)
    got = read_png(tmp_path / "b.png")
    assert got.shape == (100, 100, 4) and np.array_equal(got, yk.present(mapped, (100, 100)))
    assert np.array_equal(got[0], np.broadcast_to(np.array([0, 0, 0, 255], np.uint8), (100, 4)))  # the letterbox
    yk.write_preview(tmp_path / "c.png", np.clip(film, 0, 1), yk.ToneMapType.Raw)
    assert np.array_equal(read_png(tmp_path / "c.png"), yk.present(np.clip(film, 0, 1), (48, 27)))


# ------------------------------------------------------------------ argument errors
def test_argument_errors(yk, tmp_path):
    from yuki_amd._ffi import YukiError

    L = yk.lib()
    assert L.yk_sizeof(18) == C.sizeof(abi.PresentDesc) == 12 and L.yk_sizeof(19) == C.sizeof(abi.PresentRect) == 16
    film = np.zeros((4, 4, 3), np.float32)
    out = np.zeros((8, 8, 3), np.float32)
    p, o = film.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    good = abi.PresentDesc(8, 8, 2, 0)
    assert L.yk_present(None, C.byref(good), p, 4, 4, o) == 0
    for d in (abi.PresentDesc(0, 8, 2, 0), abi.PresentDesc(8, 0, 2, 0), abi.PresentDesc(8, 8, 3, 0), abi.PresentDesc(8, 8, 2, 2)):
        assert L.yk_present(None, C.byref(d), p, 4, 4, o) == 1
    assert L.yk_present(None, C.byref(good), None, 4, 4, o) == 1
    assert L.yk_present(None, C.byref(good), p, 4, 4, None) == 1
    assert L.yk_present(None, None, p, 4, 4, o) == 1
    assert L.yk_present(None, C.byref(good), p, 0, 4, o) == 1 and L.yk_present(None, C.byref(good), p, 4, 0, o) == 1
    assert L.yk_present(None, C.byref(good), p, 4, 4, p) == 1  # the output overlaps the film
    assert L.yk_present(None, C.byref(good), p, 4, 4, C.c_void_p(p.value + 4 * 4 * 12 - 4)) == 1
    assert L.yk_present_device(None, C.byref(good), p, 4, 4, o, None) == 1
    r = abi.PresentRect()
    assert L.yk_present_target_rect(0, 4, 8, 8, C.byref(r)) == 1 and L.yk_present_target_rect(4, 4, 8, 0, C.byref(r)) == 1
    assert L.yk_present_target_rect(4, 4, 8, 8, None) == 1
    with pytest.raises(YukiError) as e:
        yk.present(film, (8, 8), encode=3)
    assert e.value.status == 1
    with pytest.raises(ValueError):
        yk.present(film, (8, 8), fmt="bgra8")
    px = np.zeros((2, 2, 4), np.uint8)
    q = px.ctypes.data_as(C.c_void_p)
    assert L.yk_write_png(None, 2, 2, 4, q) == 1 and L.yk_write_png(str(tmp_path / "x.png").encode(), 2, 2, 4, None) == 1
    assert L.yk_write_png(str(tmp_path / "x.png").encode(), 2, 2, 2, q) == 1 and L.yk_write_png(str(tmp_path / "x.png").encode(), 0, 2, 4, q) == 1
    assert L.yk_write_png(str(tmp_path / "no" / "such" / "x.png").encode(), 2, 2, 4, q) == 1
