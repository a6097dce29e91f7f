"""The tone map (app/renderpasses/tonemap.rs, what `yuki --out` writes: app/headless.rs:62-84) on the host: the library's
host instance against an independent numpy float32 restatement (tests/tonemap_ref.py) bit for bit, float64 anchors that
show the restatement itself is right, the reference's two reproduced quirks, find_min_max, the sample table in
FilmTile.index order, argument errors and the EXR that write_output leaves.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import tonemap_ref as ref
from yuki_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _films():
    rng = np.random.default_rng(20261016)
    return [ref.random_film(rng, h, w) for (h, w) in ((23, 37), (16, 16), (1, 5), (40, 64))]


# ------------------------------------------------------------------ host instance == restatement, bit for bit
@pytest.mark.parametrize("exposure", [0.25, 1.0, 8.0])
def test_filmic_host_equals_restatement(yk, exposure):
    rng = np.random.default_rng(7)
    for film in _films():
        h, w, _ = film.shape
        for td in (16, 8, 5):
            got = yk.tone_map(film, yk.ToneMapType.Filmic(yk.FilmicParams(exposure)), td)
            assert np.array_equal(ref.bits(got), ref.bits(ref.filmic(film, exposure, td, None)))
            n = -(-w // td) * -(-h // td)
            samples = rng.integers(0, 6, size=n).astype(np.uint32)  # zeros included: no division there
            got = yk.tone_map(film, yk.ToneMapType.Filmic(yk.FilmicParams(exposure)), td, samples=samples)
            assert np.array_equal(ref.bits(got), ref.bits(ref.filmic(film, exposure, td, samples)))


@pytest.mark.parametrize("channel", [0, 1, 2, 3])
def test_heatmap_host_equals_restatement(yk, channel):
    for film in _films():
        for bounds in ((0.0, 1.0), (-5.0, 100.0), (2.0, 2.0), (-np.inf, 1.0), (1.0, np.inf), (np.nan, 1.0)):
            got = yk.tone_map(film, yk.ToneMapType.Heatmap(yk.HeatmapParams(bounds, channel)), 16)
            assert np.array_equal(ref.bits(got), ref.bits(ref.heatmap(film, bounds[0], bounds[1], channel)))
        used = np.zeros(2, np.float32)
        got = yk.tone_map(film, yk.ToneMapType.Heatmap(yk.HeatmapParams(None, channel)), 16, used_bounds=used)
        lo, hi = ref.min_max(film, channel)
        assert used[0] == lo and used[1] == hi
        assert np.array_equal(ref.bits(got), ref.bits(ref.heatmap(film, lo, hi, channel)))
        # finite films too (bounds found from ordinary values, not from the infinities)
        fin = np.nan_to_num(film, nan=0.0, posinf=1.0, neginf=-1.0)
        lo, hi = ref.min_max(fin, channel)
        got = yk.tone_map(fin, yk.ToneMapType.Heatmap(yk.HeatmapParams(None, channel)), 16)
        assert np.array_equal(ref.bits(got), ref.bits(ref.heatmap(fin, lo, hi, channel)))


def test_raw_copies_the_film(yk):
    for film in _films():
        assert np.array_equal(ref.bits(yk.tone_map(film, yk.ToneMapType.Raw, 16)), ref.bits(film))


def test_default_is_filmic_exposure_one(yk):
    d = yk.ToneMapType.default()
    assert d.kind == abi.TONE_MAP_FILMIC and d.exposure == 1.0
    p = yk.HeatmapParams()
    assert p.bounds is None and p.channel == yk.HeatmapChannel.Red == 0
    assert yk.lib().yk_sizeof(13) == C.sizeof(abi.ToneMapDesc) == 24


# ------------------------------------------------------------------ the reproduced quirks
def test_sample_lookup_uses_floor_tile_count(yk):
    """200 x 150 at tile 16: the table is laid out over the 13-wide ceil grid, the shader indexes with 200 / 16 = 12, so
    pixel (0, 16) reads tile index 1*12 + 0 = 12, not its own index 13."""
    w, h, td = 200, 150, 16
    samples = np.arange(1, 13 * 10 + 1, dtype=np.uint32)  # count of index i = i + 1
    film = np.full((h, w, 3), 0.7, dtype=np.float32)
    got = yk.tone_map(film, yk.ToneMapType.default(), td, samples=samples)
    px = film[16:17, 0:1]
    with_12 = ref.filmic(px, 1.0, td, np.array([13], np.uint32))  # a one-pixel film whose only count is 13
    with_13 = ref.filmic(px, 1.0, td, np.array([14], np.uint32))
    assert np.array_equal(ref.bits(got[16, 0]), ref.bits(with_12[0, 0]))
    assert not np.array_equal(ref.bits(got[16, 0]), ref.bits(with_13[0, 0]))
    assert np.array_equal(ref.bits(got), ref.bits(ref.filmic(film, 1.0, td, samples)))


def test_film_narrower_than_a_tile(yk):
    fs = yk.FilmSettings(res=(10, 40), tile_dim=16)
    assert yk.film_tile_dim(fs) == 10  # Film::tile_dim(): the first spiral tile's width
    assert yk.film_tile_dim(yk.FilmSettings(res=(40, 10), tile_dim=16)) == 16
    assert yk.film_tile_dim(yk.FilmSettings(res=(200, 150), tile_dim=16)) == 16
    film = ref.random_film(np.random.default_rng(3), 40, 10)
    td = yk.film_tile_dim(fs)
    got = yk.tone_map(film, yk.ToneMapType.default(), td)
    assert np.array_equal(ref.bits(got), ref.bits(ref.filmic(film, 1.0, td, None)))
    samples = np.arange(1, 5, dtype=np.uint32)  # ceil(10/10) * ceil(40/10)
    got = yk.tone_map(film, yk.ToneMapType.default(), td, samples=samples)
    assert np.array_equal(ref.bits(got), ref.bits(ref.filmic(film, 1.0, td, samples)))


def test_red_heatmap_maps_luminance_with_red_bounds(yk):
    film = np.zeros((4, 8, 3), np.float32)
    film[..., 0] = np.linspace(0, 10, 32, dtype=np.float32).reshape(4, 8)
    film[..., 1] = np.linspace(3, -2, 32, dtype=np.float32).reshape(4, 8)
    film[..., 2] = 0.5
    lo, hi = yk.find_min_max(film, yk.HeatmapChannel.Red)
    assert (lo, hi) == (0.0, 10.0)  # find_min_max reads red for Red
    used = np.zeros(2, np.float32)
    got = yk.tone_map(film, yk.ToneMapType.Heatmap(yk.HeatmapParams()), 16, used_bounds=used)
    assert tuple(used) == (0.0, 10.0)
    lum = ref.heatmap(film, 0.0, 10.0, 3)
    as_red = film.copy()
    as_red[..., 1] = film[..., 0]
    red = ref.heatmap(as_red, 0.0, 10.0, 1)  # what mapping the red value would give
    assert np.array_equal(ref.bits(got), ref.bits(lum))  # ... but the shader maps luminance
    assert not np.array_equal(ref.bits(got), ref.bits(red))
    assert np.array_equal(ref.bits(got), ref.bits(yk.tone_map(film, yk.ToneMapType.Heatmap(yk.HeatmapParams((0.0, 10.0), 3)), 16)))
    uni = np.full((3, 3, 3), 2.0, np.float32)  # min == max: a uniform film maps to LOW
    out = yk.tone_map(uni, yk.ToneMapType.Heatmap(yk.HeatmapParams()), 16)
    assert np.array_equal(out, np.broadcast_to(np.array([0, 0, 1], np.float32), out.shape))


# ------------------------------------------------------------------ anchors against float64
def _filmic64(film, exposure):
    """The same formulas in float64 (no float32 rounding anywhere)."""
    c = np.asarray(film, np.float64) * exposure
    mi = np.array(ref.M_IN, np.float64)
    mo = np.array(ref.M_OUT, np.float64)
    v = c @ mi.T
    v = (v * (v + 0.0245786) - 0.000090537) / (v * (0.983729 * v + 0.4329510) + 0.238081)
    return np.clip(v @ mo.T, 0.0, 1.0)


def test_filmic_anchors(yk):
    assert np.array_equal(yk.tone_map(np.zeros((1, 1, 3), np.float32), yk.ToneMapType.default(), 16), np.zeros((1, 1, 3), np.float32))
    assert np.array_equal(yk.tone_map(np.full((1, 1, 3), 1e6, np.float32), yk.ToneMapType.default(), 16), np.ones((1, 1, 3), np.float32))
    rng = np.random.default_rng(11)
    for exposure in (0.25, 1.0, 8.0):
        # radiance (non-negative; signed inputs of mixed magnitudes cancel in ACESInputMat, an ill-conditioned sum in any
        # precision), every component below 1e18 after the exposure
        film = np.abs(ref.random_film(rng, 64, 64, specials=False))
        film = film[film.max(axis=-1) < 1e18 / 8][None]
        got = yk.tone_map(film, yk.ToneMapType.Filmic(yk.FilmicParams(exposure)), 16)
        assert np.abs(got.astype(np.float64) - _filmic64(film, exposure)).max() < 2e-6
        assert np.array_equal(ref.bits(got), ref.bits(ref.filmic(film, exposure)))
    # step 5: past ~1.8e19, v*v overflows, a / b = inf / inf = NaN and saturate makes the channel 0, not 1
    with np.errstate(all="ignore"):
        assert abs(float(ref.fit(F(1e19))) - 1.01654) < 1e-5
        assert np.isnan(ref.fit(F(2e19)))
    grey = np.array([[[1e19] * 3, [2e19] * 3, [1e30] * 3, [3e38] * 3]], np.float32)
    got = yk.tone_map(grey, yk.ToneMapType.default(), 16)
    assert np.array_equal(got[0, 0], np.ones(3, np.float32))
    assert np.array_equal(got[0, 1:], np.zeros((3, 3), np.float32))


# ------------------------------------------------------------------ find_min_max
def test_find_min_max(yk):
    film = np.array([[[np.nan, 1, 2], [3, np.nan, -4], [-0.5, 7, np.nan]]], np.float32)
    assert yk.find_min_max(film, 0) == (-0.5, 3.0)
    assert yk.find_min_max(film, 1) == (1.0, 7.0)
    assert yk.find_min_max(film, 2) == (-4.0, 2.0)
    assert yk.find_min_max(film, 3) == ref.min_max(film, 3)
    nan = np.full((5, 7, 3), np.nan, np.float32)
    for ch in range(4):
        assert yk.find_min_max(nan, ch) == (F(3.4028235e38), F(-3.4028235e38))
    for film in _films():
        for ch in range(4):
            assert yk.find_min_max(film, ch) == ref.min_max(film, ch)


# ------------------------------------------------------------------ the sample table
def _generate_tiles_index(res, td):
    """generate_tiles (film.rs:299-331): tile coordinates -> FilmTile.index, row-major over the ceil grid."""
    index, flat = {}, 0
    for j in range(0, res[1], td):
        for i in range(0, res[0], td):
            index[(i // td, j // td)] = flat
            flat += 1
    return index, flat


@pytest.mark.parametrize("res,td", [((200, 150), 16), ((64, 64), 16), ((33, 17), 8), ((100, 40), 32), ((7, 5), 4)])
def test_film_samples_in_tile_index_order(yk, res, td):
    fs = yk.FilmSettings(res=res, tile_dim=td, accumulate=True)
    tiles = yk.film_tiles(fs)
    counts = np.arange(1, len(tiles) + 1, dtype=np.uint32) * 3  # distinct: equal counts would hide the order
    index, n = _generate_tiles_index(res, td)
    want = np.zeros(n, np.uint32)
    for t, c in zip(tiles, counts):
        want[index[(int(t["x0"]) // td, int(t["y0"]) // td)]] += c
    got = yk.film_samples(fs, tiles, counts)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    if len(tiles) > 2:
        assert not np.array_equal(got, counts)  # the spiral is not the index order


# ------------------------------------------------------------------ argument errors
def test_argument_errors(yk):
    from yuki_amd._ffi import YukiError

    film = np.zeros((4, 4, 3), np.float32)
    L = yk.lib()
    out = np.zeros_like(film)
    bad = [abi.ToneMapDesc(3, 1.0, 0, 0, (C.c_float * 2)()), abi.ToneMapDesc(abi.TONE_MAP_HEATMAP, 1.0, 4, 1, (C.c_float * 2)(0, 1))]
    for d in bad:
        with pytest.raises(YukiError) as e:
            yk.tone_map(film, d, 16)
        assert e.value.status == 1
    with pytest.raises(YukiError):
        yk.tone_map(film, yk.ToneMapType.default(), 0)
    with pytest.raises(YukiError):
        yk.tone_map(np.zeros((0, 4, 3), np.float32), yk.ToneMapType.default(), 16)
    with pytest.raises(ValueError):
        yk.tone_map(film, yk.ToneMapType.default(), 16, samples=np.zeros(3, np.uint32))
    d = yk.ToneMapType.default()
    p = film.ctypes.data_as(C.c_void_p)
    assert L.yk_tone_map(None, C.byref(d), None, 4, 4, 16, None, out.ctypes.data_as(C.c_void_p), None) == 1
    assert L.yk_tone_map(None, C.byref(d), p, 4, 4, 16, None, None, None) == 1
    assert L.yk_tone_map(None, None, p, 4, 4, 16, None, out.ctypes.data_as(C.c_void_p), None) == 1
    assert L.yk_tone_map(None, C.byref(d), p, 4, 0, 16, None, out.ctypes.data_as(C.c_void_p), None) == 1
    assert L.yk_tone_map_device(None, C.byref(d), p, 4, 4, 16, None, p, None) == 1
    mm = np.zeros(2, np.float32)
    assert L.yk_film_min_max(None, p, 4, 4, 4, mm.ctypes.data_as(C.c_void_p)) == 1
    assert L.yk_film_min_max(None, None, 4, 4, 0, mm.ctypes.data_as(C.c_void_p)) == 1
    assert L.yk_film_min_max(None, p, 0, 4, 0, mm.ctypes.data_as(C.c_void_p)) == 1


# ------------------------------------------------------------------ write_output (headless.rs:62-84)
def test_write_output_raw_and_filmic(yk, tmp_path):
    from test_film import read_exr

    film = np.abs(ref.random_film(np.random.default_rng(5), 27, 48, specials=False))
    fs = yk.FilmSettings(res=(48, 27), tile_dim=16)
    yk.write_output(tmp_path / "raw.exr", film, yk.ToneMapType.Raw, settings=fs)
    assert np.array_equal(ref.bits(read_exr(tmp_path / "raw.exr")), ref.bits(film))
    yk.write_output(tmp_path / "filmic.exr", film, settings=fs)  # default: Filmic, exposure 1
    assert np.array_equal(ref.bits(read_exr(tmp_path / "filmic.exr")), ref.bits(ref.filmic(film, 1.0)))
    counts = np.arange(1, 13, dtype=np.uint32)
    tiles = yk.film_tiles(fs)
    samples = yk.film_samples(fs, tiles, counts[: len(tiles)])
    yk.write_output(tmp_path / "acc.exr", film, yk.ToneMapType.Filmic(yk.FilmicParams(2.0)), settings=fs, samples=samples)
    assert np.array_equal(ref.bits(read_exr(tmp_path / "acc.exr")), ref.bits(ref.filmic(film, 2.0, 16, samples)))


def test_heatmap_of_the_golden_bvh_intersections_film(yk, tmp_path):
    """The BVHIntersections film of tests/golden (node-test counts) through the default Heatmap, as `yuki --out` with
    that integrator and HeatmapParams::default() writes it."""
    from test_film import read_exr

    g = np.load(os.path.join(ROOT, "tests", "golden", "render_city_small_bvh_intersections.npz"))
    fs = yk.FilmSettings(res=(48, 27), tile_dim=16)
    film = yk.update_tiles(yk.film_tiles(fs), g["rgb"], fs.res)
    lo, hi = ref.min_max(film, 0)
    assert lo < hi
    want = ref.heatmap(film, lo, hi, 0)
    got = yk.tone_map(film, yk.ToneMapType.Heatmap(yk.HeatmapParams()), yk.film_tile_dim(fs))
    assert np.array_equal(ref.bits(got), ref.bits(want))
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 10  # a real gradient, not one colour
    yk.write_output(tmp_path / "heat.exr", film, yk.ToneMapType.Heatmap(yk.HeatmapParams()), settings=fs)
    assert np.array_equal(ref.bits(read_exr(tmp_path / "heat.exr")), ref.bits(want))
