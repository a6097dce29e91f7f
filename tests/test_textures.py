"""Image textures: ImageTexture::new (PNG decode) and
ImageTexture::evaluate on the device, against the checker's independent restatement.

Parity unpinned: the reference ships no image fixtures and decodes through the `image`
crate (absent from /root/reference); both sides follow the PNG specification and
textures/image_texture.rs.  The tests pin (1) decoded texels == source pixels / 255
(or / 65535) exactly, (2) product decoder == checker decoder bit for bit over colour
types, bit depths, filters, interlacing and deflate block types, (3) device texture
lookup + shading == the oracle's on a textured scene."""
import os

import numpy as np
import pytest

from yuki_amd import abi, loaders
from yuki_amd._ffi import YukiError

import scene_files as sf
from test_loaders import assert_same_camera, assert_same_scene


@pytest.fixture(scope="module")
def oi(oracle):
    from oracle import images

    return images


VARIANTS = [
    dict(),
    dict(alpha=True),
    dict(depth=16),
    dict(depth=16, alpha=True, interlace=True),
    dict(interlace=True),
    dict(level=0),  # stored deflate blocks
    dict(fixed=True),  # fixed Huffman codes
    dict(level=9, filters=(4,)),
    dict(filters=(3, 3, 1)),
    dict(trns=True),
]


@pytest.mark.parametrize("kw", VARIANTS)
@pytest.mark.parametrize("size", [(1, 1), (7, 5), (33, 17)])
def test_png_rgb_decode(tmp_path, oi, kw, size):
    w, h = size
    depth = kw.get("depth", 8)
    src = sf.test_pattern(w, h, depth)
    p = str(tmp_path / "t.png")
    sf.write_png(p, src, **kw)
    got = loaders.load_image_texture(p)
    want = oi.load_png(p)
    assert got.shape == (h, w, 3) and got.dtype == np.float32
    assert got.tobytes() == want.tobytes()
    exact = src.astype(np.float32) / np.float32((1 << depth) - 1)  # image_texture.rs:10-35
    assert got.tobytes() == exact.tobytes()


@pytest.mark.parametrize("depth", [1, 2, 4, 8])
@pytest.mark.parametrize("interlace", [False, True])
def test_png_palette_decode(tmp_path, oi, depth, interlace):
    n = 1 << depth
    rng = np.random.default_rng(depth)
    pal = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    idx = rng.integers(0, n, size=(13, 19)).astype(np.uint8)
    p = str(tmp_path / "p.png")
    sf.write_png(p, idx, depth=depth, palette=pal, interlace=interlace, trns=(depth == 2))
    got = loaders.load_image_texture(p)
    assert got.tobytes() == oi.load_png(p).tobytes()
    assert got.tobytes() == (pal[idx].astype(np.float32) / np.float32(255)).tobytes()


def test_png_large_random_exercises_dynamic_huffman(tmp_path, oi):
    rng = np.random.default_rng(11)
    src = rng.integers(0, 256, size=(96, 128, 3))
    src[20:60] = src[20:21]  # long matches -> length/distance codes with extra bits
    p = str(tmp_path / "r.png")
    sf.write_png(p, src, level=9, filters=(0, 2))
    got = loaders.load_image_texture(p)
    assert got.tobytes() == oi.load_png(p).tobytes()
    assert got.tobytes() == (src.astype(np.float32) / np.float32(255)).tobytes()


# PNG files written by other encoders, kept as data under tests/golden/png/ (tiling_58 is a CC0 texture from sharetextures.com):
# the reference's own 16-bit RGBA normal map as it ships, and crops of its 16-bit grey roughness map and of its 8-bit RGBA
# screenshot, re-encoded by Pillow (adaptive row filters, zlib's dynamic Huffman blocks) to keep the files small.
PNG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png")
REFERENCE_PNGS = [
    "tiling_58_normal-1K.png",  # 1024 x 1024, 16-bit RGBA
    "tiling_58_roughness-crop.png",  # 128 x 128, 16-bit grey
    "screenshot-crop.png",  # 384 x 256, 8-bit RGBA
]


@pytest.mark.parametrize("name", REFERENCE_PNGS)
def test_png_files_the_reference_ships(oi, name):
    """PNG files of the reference's tree (its texture assets and its screenshot: files written by other encoders) through the
    product decoder and through the independent zlib / numpy one: same texels, bit for bit, the first row also against a
    by-hand unfiltering of zlib's output; the 16-bit grey map is refused by both with the reference's own message (a Spectrum
    texture has no Luma arm)."""
    import struct
    import zlib

    path = os.path.join(PNG_DIR, name)
    raw = open(path, "rb").read()
    w, h, depth, ctype = struct.unpack(">IIBB", raw[16:26])
    if ctype in (0, 4):  # Luma / LumaA: `load_image_spectrum_f32` has no arm for them (image_texture.rs:114-141)
        with pytest.raises(YukiError, match="Unsupported image format"):
            loaders.load_image_texture(path)
        with pytest.raises(Exception, match="Unsupported image format"):
            oi.load_png(path)
        return
    got = loaders.load_image_texture(path)
    want = oi.load_png(path)
    assert got.shape == (h, w, 3) and got.tobytes() == want.tobytes()
    # a third reading of the first row: inflate with zlib, undo the row filter by hand (colour types 0 and 6)
    pos, idat = 8, b""
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos : pos + 8])
        if tag == b"IDAT":
            idat += raw[pos + 8 : pos + 8 + n]
        pos += 12 + n
    chans = {0: 1, 6: 4}[ctype]
    bpp = chans * depth // 8
    stride = w * bpp
    data = zlib.decompress(idat)
    assert len(data) == h * (stride + 1)
    f, row = data[0], bytearray(data[1 : 1 + stride])
    assert f in (0, 1, 2, 3, 4)
    if f in (1, 3, 4):  # Sub / Average / Paeth with no row above: left neighbour, half of it, left neighbour
        for i in range(bpp, stride):
            left = row[i - bpp]
            row[i] = (row[i] + (left if f != 3 else left // 2)) & 255
    px = np.frombuffer(bytes(row), dtype=">u2" if depth == 16 else np.uint8).reshape(w, chans).astype(np.float32)
    px = px / np.float32((1 << depth) - 1)
    first = np.repeat(px, 3, axis=1) if chans == 1 else px[:, :3]
    assert got[0].tobytes() == first.tobytes()


def test_png_errors(tmp_path, oi):
    src = sf.test_pattern(9, 6)
    p = str(tmp_path / "g.png")
    sf.write_png(p, src, gray=True)
    with pytest.raises(YukiError) as e:  # Luma8: image_texture.rs:131-135
        loaders.load_image_texture(p)
    assert "Unsupported image format" in str(e.value) and e.value.status == 5
    with pytest.raises(oi.ImageError):
        oi.load_png(p)
    sf.write_png(p, src, gray=True, alpha=True)
    with pytest.raises(YukiError):
        loaders.load_image_texture(p)
    good = str(tmp_path / "ok.png")
    sf.write_png(good, src)
    data = bytearray(open(good, "rb").read())
    for name, mutate in (
        ("crc", lambda d: d.__setitem__(len(d) // 2, d[len(d) // 2] ^ 0x40)),
        ("trunc", lambda d: d.__delitem__(slice(len(d) - 80, len(d)))),
        ("magic", lambda d: d.__setitem__(1, ord("Q"))),
    ):
        d = bytearray(data)
        mutate(d)
        bad = str(tmp_path / f"bad_{name}.png")
        open(bad, "wb").write(d)
        with pytest.raises(YukiError):
            loaders.load_image_texture(bad)
        with pytest.raises(oi.ImageError):
            oi.load_png(bad)
    with pytest.raises(YukiError) as e:
        loaders.load_image_texture(str(tmp_path / "missing.png"))
    assert "Could not open" in str(e.value)


def test_textured_pbrt_scene_loads_identically(tmp_path, oracle):
    from oracle import loaders as ol

    p = sf.write_textured_scene(str(tmp_path))
    got, cam, film = loaders.load_pbrt(p)
    want, wcam, wres = ol.load_pbrt(p)
    assert_same_scene(want, got)
    assert_same_camera(wcam, cam, film, wres)
    assert len(got.textures) == 3 and [t.shape for t in got.textures] == [(23, 37, 3), (16, 16, 3), (11, 13, 3)]
    # `Texture "checks"` is re-declared inside the last block: earlier materials keep the old image
    assert [m.get("tex") for m in got.materials] == [None, 0, 1, 0, 2]
    assert got.materials[2]["c"] != 0.0 and all(got.materials[k]["a"] == (0.0, 0.0, 0.0) for k in (1, 2, 3, 4))


def test_scene_create_validates_texture_index(yk):
    from yuki_amd import scenes

    sd = scenes.by_name("cornell-tris")
    sd.materials[0] = dict(sd.materials[0], tex=3)
    with pytest.raises(YukiError) as e:
        yk.Scene(None, sd)
    assert e.value.status == 1


def test_texture_evaluate(tmp_path, oracle, oi):
    """ImageTexture::evaluate (image_texture.rs:81-111): repeat, flip v, point sample — the C++
    oracle (used by its renderer) against the numpy restatement and hand-checked texels."""
    img = sf.test_pattern(8, 5)
    p = str(tmp_path / "t.png")
    sf.write_png(p, img)
    tex = oi.load_png(p)
    rng = np.random.default_rng(2)
    uv = np.concatenate([
        rng.uniform(-3, 3, size=(500, 2)),
        np.array([[0, 0], [1, 1], [0.999999, 0.999999], [-1e-9, -1e-9], [0.5, 0.5], [np.nan, 0.5], [0.5, np.inf], [-0.0, 2.0], [7.0, -7.0]]),
    ]).astype(np.float32)
    got = oracle.texture_eval(tex, uv)
    want = np.stack([oi.evaluate(tex, u, v) for u, v in uv])
    assert got.tobytes() == want.tobytes()
    # hand-checked: uv (0,0) -> bottom-left texel = last row, first column; (0.999,0.999) -> top-right
    assert oracle.texture_eval(tex, [[0.0, 0.0]])[0].tobytes() == tex[4, 0].tobytes()
    assert oracle.texture_eval(tex, [[0.999, 0.999]])[0].tobytes() == tex[0, 7].tobytes()
    assert oracle.texture_eval(tex, [[1.25, -0.3]])[0].tobytes() == tex[int((1 - 0.7) * 5 - 0.5), int(0.25 * 8 - 0.5)].tobytes()


# ----------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_textured_scene_renders_like_the_oracle(tmp_path, oracle, yk, ctx):
    from oracle import loaders as ol

    p = sf.write_textured_scene(str(tmp_path))
    got_sd, cam_p, film = loaders.load_pbrt(p)
    want_sd, _, _ = ol.load_pbrt(p)
    fs = yk.FilmSettings(res=film.res, tile_dim=film.tile_dim)
    cam = yk.Camera(cam_p, fs)
    tiles = yk.film_tiles(fs)
    osc = oracle.OracleScene(want_sd)
    sc = yk.Scene(ctx, got_sd)
    for sampler, depth in ((yk.SamplerType.Stratified((2, 2), True, 0x73B9642E74AC471C), 5), (yk.SamplerType.Uniform(3, 7), 2)):
        integ = yk.IntegratorType.Path(yk.PathParams(max_depth=depth))
        it = yk.IntegratorType.instantiate(ctx, integ)
        got, stats = it.render_tiles(sc, cam, sampler, tiles)
        want, rays = osc.render_tiles(cam.matrices, sampler, integ, tiles, n_threads=0)
        assert stats.rays == rays
        assert float(np.sqrt(np.mean((got.astype(np.float64) - want) ** 2))) < 1e-4
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the texture is really sampled: the image has structure a constant Kd would not give
    film_img = yk.update_tiles(tiles, got, fs.res)
    assert film_img[40:, :, 0].std() > 0.02
