"""The exposure meter's host instance (yk_film_histogram / yk_exposure_meter without a context; the rule of
yuki_amd/csrc/yk_exposure.h) against tests/exposure_ref.py bit for bit, its known answers, the skip set, the percentile
cut, the 2^x polynomial, invariance under scaling, the adaptation, the refusals, and the Python surface around it."""
import ctypes as C

import numpy as np
import pytest

import exposure_ref as ref
import tonemap_ref as tmref
from yuki_amd import abi

LOG2_KEY = float(np.log2(0.18))
CUTS = ((0.05, 0.02), (0.0, 0.0), (0.3, 0.45))


def _ref_desc(p, res):
    d = p.desc(res)
    return ref.Desc(d.low_cut, d.high_cut, d.ev_bias, d.min_ev, d.max_ev, d.adapt_up, d.adapt_down, tuple(d.window))


def _ref_prev(s):
    return None if s is None else ref.State(s.exposure, s.log2_adapted, s.log2_metered, s.frames, s.counted, s.skipped, s.below, s.above)


def _films():
    rng = np.random.default_rng(20261020)
    return [ref.lognormal_film(rng, h, w) for (h, w) in ((23, 37), (16, 16), (5, 1), (1, 1))]


def _windows(h, w):
    return [None] if h * w < 16 else [None, (1, 2, w - 3, h - 1)]


def test_host_equals_the_restatement(yk):
    rng = np.random.default_rng(7)
    for film in _films():
        h, w, _ = film.shape
        for td in (16, 5):
            table = rng.integers(0, 6, size=-(-w // td) * -(-h // td)).astype(np.uint32)
            for samples in (None, table):
                for window in _windows(h, w):
                    bins, sba = yk.film_histogram(film, td, samples=samples, window=window)
                    want_bins, want_sba = ref.histogram(film, td, samples, window)
                    assert [int(v) for v in bins] == want_bins and sba == want_sba, (film.shape, td, window)
                    area = h * w if window is None else (window[2] - window[0]) * (window[3] - window[1])
                    assert sum(want_bins) + sba[0] == area
                    for lo, hi in CUTS:
                        p = yk.ExposureParams(low_cut=lo, high_cut=hi, window=window)
                        got = yk.meter_exposure(film, td, p, samples=samples)
                        assert ref.same_state(got, ref.meter(film, _ref_desc(p, (w, h)), td, samples)), (film.shape, td, window, lo, hi)
                        assert got.counted + got.skipped == area


def test_q_table_and_the_bin_rule():
    assert ref.Q == [int(round(65536 * np.log2(1 + (m + 0.5) / 8))) for m in range(8)]
    just_under_one = np.nextafter(np.float32(1), np.float32(0))
    for value, bin_ in ((0.18, 107), (1.0, 128), (0.5, 120), (2.0**-16, 0), (just_under_one, 127)):
        assert (int(np.float32(value).view(np.uint32)) >> 20) - 888 == bin_
    assert (int(np.float32(1e-9).view(np.uint32)) >> 20) - 888 < 0 and (int(np.float32(1e9).view(np.uint32)) >> 20) - 888 > 255


def test_known_bins_through_the_product(yk):
    """The bins the rule names.  A grey pixel's luminance (0.2126 v + 0.7152 v) + 0.0722 v is v only to a rounding or two,
    which for 0.18, 0.5, 1, 1e-9 and 1e9 stays in the value's bin (the arithmetic is fixed, so that is no accident of a
    platform); 2^-16 and the largest float under 1, where it does not, are fed through green alone."""
    cases = {0.18: (107, 0, 0), 1.0: (128, 0, 0), 0.5: (120, 0, 0), 1e-9: (0, 1, 0), 1e9: (255, 0, 1)}
    for value, (bin_, below, above) in cases.items():
        film = np.full((2, 3, 3), value, np.float32)
        bins, sba = yk.film_histogram(film, 16)
        assert int(bins[bin_]) == 6 and int(bins.sum()) == 6 and sba == (0, 6 * below, 6 * above), value
    # 2^-16 and the largest float under 1 sit on a bin's edge, where the grey's rounding may cross it: feed them through
    # green alone, Y = 0.7152f * g, with g chosen so that the product is the value exactly or the next float inside the bin
    for value, bin_ in ((np.float32(2.0**-16), 0), (np.nextafter(np.float32(1), np.float32(0)), 127)):
        g = np.float32(value / np.float32(0.7152))
        for cand in (g, np.nextafter(g, np.float32(np.inf)), np.nextafter(g, np.float32(0))):
            if np.float32(np.float32(0.7152) * cand) == value:
                g = cand
                break
        else:
            pytest.fail(f"no green value gives luminance {value!r} exactly")
        film = np.zeros((1, 1, 3), np.float32)
        film[0, 0, 1] = g
        bins, sba = yk.film_histogram(film, 16)
        assert int(bins[bin_]) == 1 and sba == (0, 0, 0), value


def test_constant_grey_film_known_answer(yk):
    film = np.full((9, 11, 3), 0.18, np.float32)
    s = yk.meter_exposure(film, 16)
    assert s.counted == 99 and s.skipped == 0 and s.frames == 1
    assert np.float32(s.log2_metered) == np.float32(-162296 / 65536) == np.float32(s.log2_adapted)
    assert ref.bin_value(107) == -162296
    want = 2.0 ** (np.log2(0.18) + 162296 / 65536)
    assert abs(want - 1.00174) < 1e-5
    assert abs(s.exposure / want - 1) <= 1e-5


def test_skip_set(yk):
    vals = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -3.0, 1e-40, 0.25], np.float32)
    film = np.repeat(vals[None, :, None], 3, axis=2)
    bins, sba = yk.film_histogram(film, 16)
    # NaN, +-inf, +-0 and the negative are skipped; the subnormal is counted in bin 0 and `below`; 0.25 in its bin
    assert sba == (6, 1, 0) and int(bins[0]) == 1 and int(bins.sum()) == 2
    assert ([int(v) for v in bins], sba) == ref.histogram(film)
    empty = np.repeat(vals[None, :6, None], 3, axis=2)
    s = yk.meter_exposure(empty, 16)
    assert (s.counted, s.skipped, s.frames) == (0, 6, 0) and s.exposure == 1.0
    assert np.float32(s.log2_adapted) == np.float32(LOG2_KEY) == np.float32(s.log2_metered)
    prev = yk.meter_exposure(np.full((2, 2, 3), 4.0, np.float32), 16)
    t = yk.meter_exposure(empty, 16, prev=prev)
    assert (t.counted, t.skipped, t.frames) == (0, 6, prev.frames)
    assert t.log2_adapted == prev.log2_adapted == t.log2_metered and t.exposure == prev.exposure
    assert ref.same_state(t, ref.meter(empty, ref.Desc(), prev=_ref_prev(prev)))


def test_percentile_cut(yk):
    film = np.full((10, 20, 3), 0.25, np.float32)
    film.reshape(-1, 3)[:10] = 2.0**10  # 5 % of 200 pixels
    grey_bin = int(np.argmax(yk.film_histogram(np.full((1, 1, 3), 0.25, np.float32), 16)[0]))
    cut = yk.meter_exposure(film, 16, yk.ExposureParams(low_cut=0.0, high_cut=0.06))
    assert np.float32(cut.log2_metered) == np.float32(ref.bin_value(grey_bin) / 65536)
    whole = yk.meter_exposure(film, 16, yk.ExposureParams(low_cut=0.0, high_cut=0.0))
    assert whole.log2_metered > cut.log2_metered
    # a boundary inside a bin takes the integer share: 7 samples in one bin and 3 in another, low_cut = 0.25 drops
    # floor(10 * 0.25) = 2 of the 7: (5 v(a) + 3 v(b)) / 8
    two = np.full((1, 10, 3), 0.25, np.float32)
    two[0, 7:] = 8.0
    hi_bin = int(np.argmax(yk.film_histogram(np.full((1, 1, 3), 8.0, np.float32), 16)[0]))
    s = yk.meter_exposure(two, 16, yk.ExposureParams(low_cut=0.25, high_cut=0.0))
    S = 5 * ref.bin_value(grey_bin) + 3 * ref.bin_value(hi_bin)
    assert np.float32(s.log2_metered) == np.float32(np.float64(S) / (8 * 65536.0))


def test_exp2_polynomial(yk):
    """ex_exp2 through the product: an all-skipped film without history gives exposure 2^clamp(ev_bias - ev_bias) = 1, and
    one with a carried state gives 2^(ev_bias - prev.log2_adapted): sweep that over [-24, 24]."""
    x = np.linspace(-24.0, 24.0, 200001).astype(np.float32)
    got = ref.exp2(x)
    err = np.abs(got.astype(np.float64) / np.exp2(x.astype(np.float64)) - 1.0)
    assert err.max() <= 1e-5
    ints = np.arange(-24, 25).astype(np.float32)
    assert np.array_equal(ref.exp2(ints), np.exp2(ints.astype(np.float64)).astype(np.float32))
    # the product's polynomial equals the restatement's on a subset of the sweep (each point is one library call)
    empty = np.zeros((1, 1, 3), np.float32)
    p = yk.ExposureParams(key=1.0, min_ev=-24.0, max_ev=24.0)
    pts = np.concatenate([x[::401], ints])
    for v in pts:
        prev = yk.ExposureState(1.0, -float(v), 0.0, 1, 0, 0, 0, 0)
        s = yk.meter_exposure(empty, 16, p, prev=prev)
        assert np.float32(s.exposure) == ref.exp2(np.array([v], np.float32))[0], v
        assert abs(float(s.exposure) / 2.0 ** float(v) - 1) <= 1e-5


def test_scaling_shifts_the_histogram_and_the_exposure(yk):
    rng = np.random.default_rng(11)
    Y = np.exp2(rng.uniform(-8, 8, size=(24, 31))).astype(np.float32)
    base = np.zeros((24, 31, 3), np.float32)
    base[..., 1] = Y  # green alone: Y' = 0.7152f * g, and a power of two scales it exactly
    p = yk.ExposureParams(low_cut=0.0, high_cut=0.0, min_ev=-20.0, max_ev=20.0)
    bins0, sba0 = yk.film_histogram(base, 16)
    e0 = yk.meter_exposure(base, 16, p).exposure
    assert sba0 == (0, 0, 0)
    for k in range(-6, 7):
        film = (base * np.float32(2.0**k)).astype(np.float32)
        bins, sba = yk.film_histogram(film, 16)
        assert sba == (0, 0, 0) and np.array_equal(np.roll(bins0, 8 * k), bins)
        e = yk.meter_exposure(film, 16, p).exposure
        assert abs(e * 2.0**k / e0 - 1) <= 5e-5, k


def test_adaptation(yk):
    bright = np.full((4, 4, 3), 16.0, np.float32)
    dark = np.full((4, 4, 3), 0.01, np.float32)
    p = yk.ExposureParams(adapt_up=0.25, adapt_down=0.75)
    d = _ref_desc(p, (4, 4))
    got, want = None, None
    for k, film in enumerate((bright, dark, bright, dark, bright)):
        got = yk.meter_exposure(film, 16, p, prev=got)
        want = ref.meter(film, d, prev=want)
        assert ref.same_state(got, want) and got.frames == k + 1
    first = yk.meter_exposure(bright, 16)
    instant = yk.meter_exposure(dark, 16, yk.ExposureParams(adapt_up=1.0, adapt_down=1.0), prev=first)
    assert instant.log2_adapted == instant.log2_metered == yk.meter_exposure(dark, 16).log2_metered
    held = yk.meter_exposure(dark, 16, yk.ExposureParams(adapt_up=0.0, adapt_down=0.0), prev=first)
    assert held.log2_adapted == first.log2_adapted and held.exposure == first.exposure and held.frames == 2
    full = yk.ExposureState(1.0, 0.0, 0.0, 0xFFFFFFFF, 0, 0, 0, 0)
    assert yk.meter_exposure(dark, 16, prev=full).frames == 0xFFFFFFFF
    # the clamp: a very bright film wants far fewer than -2 stops, a very dark one far more than +3
    c = yk.ExposureParams(min_ev=-2.0, max_ev=3.0)
    assert yk.meter_exposure(np.full((2, 2, 3), 1e4, np.float32), 16, c).exposure == 0.25
    assert yk.meter_exposure(np.full((2, 2, 3), 1e-4, np.float32), 16, c).exposure == 8.0


def _raw_meter(yk, desc, film, w, h, td=16, out=True):
    o = abi.ExposureState()
    return yk.lib().yk_exposure_meter(None, C.byref(desc) if desc is not None else None, None if film is None else film.ctypes.data_as(C.c_void_p), w, h, td, None, None, C.byref(o) if out else None)


def test_refusals(yk):
    film = np.ones((4, 6, 3), np.float32)
    bad = [
        (dict(low_cut=0.5, high_cut=0.5), "low_cut + high_cut must be below 65536"),
        (dict(low_cut=0.9, high_cut=0.2), "low_cut + high_cut must be below 65536"),
        (dict(min_ev=-25.0), "needs -24 <= min_ev <= max_ev <= 24"),
        (dict(max_ev=24.5), "needs -24 <= min_ev <= max_ev <= 24"),
        (dict(min_ev=2.0, max_ev=1.0), "needs -24 <= min_ev <= max_ev <= 24"),
        (dict(min_ev=float("nan")), "needs -24 <= min_ev <= max_ev <= 24"),
        (dict(adapt_up=1.5), "adapt_up and adapt_down are rates in [0, 1]"),
        (dict(adapt_down=-0.1), "adapt_up and adapt_down are rates in [0, 1]"),
        (dict(adapt_up=float("nan")), "adapt_up and adapt_down are rates in [0, 1]"),
        (dict(window=(2, 1, 2, 3)), "window needs x0 < x1 <= res_x and y0 < y1 <= res_y"),
        (dict(window=(0, 0, 7, 4)), "window needs x0 < x1 <= res_x and y0 < y1 <= res_y"),
        (dict(window=(0, 3, 6, 5)), "window needs x0 < x1 <= res_x and y0 < y1 <= res_y"),
    ]
    for kw, msg in bad:
        with pytest.raises(yk.YukiError) as e:
            yk.meter_exposure(film, 16, yk.ExposureParams(**kw))
        assert e.value.status == 1 and str(e.value).endswith("yk_exposure_meter: " + msg), (kw, str(e.value))
    for window in ((3, 0, 3, 4), (0, 0, 6, 5)):
        with pytest.raises(yk.YukiError) as e:
            yk.film_histogram(film, 16, window=window)
        assert str(e.value).endswith("yk_film_histogram: window needs x0 < x1 <= res_x and y0 < y1 <= res_y")
    d = yk.ExposureParams().desc((6, 4))
    buf = C.create_string_buffer(256)

    def message():
        yk.lib().yk_last_error(None, buf, 256)
        return buf.value.decode()

    assert _raw_meter(yk, d, film, 0, 4) == 1 and message().startswith("yk_exposure_meter: ")  # the window no longer fits
    assert _raw_meter(yk, d, film, 6, 4, td=0) == 1 and message() == "yk_exposure_meter: tile_dim is 0"
    assert _raw_meter(yk, d, None, 6, 4) == 1 and message() == "yk_exposure_meter: film is NULL"
    assert _raw_meter(yk, d, film, 6, 4, out=False) == 1 and message() == "yk_exposure_meter: out is NULL"
    assert _raw_meter(yk, None, film, 6, 4) == 1 and message() == "yk_exposure_meter: desc is NULL"
    L = yk.lib()
    bins = np.zeros(256, np.uint32)
    fp, bp = film.ctypes.data_as(C.c_void_p), bins.ctypes.data_as(C.c_void_p)
    assert L.yk_film_histogram(None, fp, 0, 4, 16, None, None, bp, None) == 1 and message() == "yk_film_histogram: zero resolution"
    assert L.yk_film_histogram(None, fp, 6, 0, 16, None, None, bp, None) == 1 and message() == "yk_film_histogram: zero resolution"
    assert L.yk_film_histogram(None, fp, 6, 4, 0, None, None, bp, None) == 1 and message() == "yk_film_histogram: tile_dim is 0"
    assert L.yk_film_histogram(None, None, 6, 4, 16, None, None, bp, None) == 1 and message() == "yk_film_histogram: film is NULL"
    assert L.yk_film_histogram(None, fp, 6, 4, 16, None, None, None, None) == 1 and message() == "yk_film_histogram: no output"
    assert L.yk_film_histogram(None, fp, 6, 4, 16, None, None, bp, None) == 0 and int(bins.sum()) == 24


def test_python_surface(yk, tmp_path):
    from test_film import read_exr

    rng = np.random.default_rng(3)
    film = ref.lognormal_film(rng, 20, 28, sigma_stops=3.0, specials=False) * np.float32(40.0)
    state = yk.meter_exposure(film, 16)
    tm = yk.ToneMapType.Filmic(yk.FilmicParams(0.7))
    multiplied = yk.ToneMapType.Filmic(yk.FilmicParams(float(np.float32(0.7) * np.float32(state.exposure))))
    want = yk.tone_map(film, multiplied, 16)
    assert np.array_equal(tmref.bits(yk.tone_map(film, tm, 16, exposure_state=state)), tmref.bits(want))
    assert np.array_equal(tmref.bits(want), tmref.bits(tmref.filmic(film, np.float32(0.7) * np.float32(state.exposure))))
    with pytest.raises(ValueError):
        yk.tone_map(film, yk.ToneMapType.Heatmap(), 16, exposure_state=state)
    # write_output(auto_exposure=True) writes what the host chain gives, the default Filmic at the meter's exposure
    yk.write_output(tmp_path / "auto.exr", film, auto_exposure=True)
    chain = yk.tone_map(film, yk.ToneMapType.default(), 16, exposure_state=state)
    assert np.array_equal(tmref.bits(read_exr(tmp_path / "auto.exr")), tmref.bits(chain))
    params = yk.ExposureParams(compensation=1.0, high_cut=0.1)
    yk.write_output(tmp_path / "auto2.exr", film, tm, auto_exposure=params)
    chain2 = yk.tone_map(film, tm, 16, exposure_state=yk.meter_exposure(film, 16, params))
    assert np.array_equal(tmref.bits(read_exr(tmp_path / "auto2.exr")), tmref.bits(chain2))
    assert not np.array_equal(chain, chain2)
    with pytest.raises(ValueError):
        yk.write_output(tmp_path / "raw.exr", film, yk.ToneMapType.Raw, auto_exposure=True)
    # every old call without the new keywords gives the bytes it gave
    yk.write_output(tmp_path / "old.exr", film)
    assert np.array_equal(tmref.bits(read_exr(tmp_path / "old.exr")), tmref.bits(yk.tone_map(film, yk.ToneMapType.default(), 16)))
    yk.write_preview(tmp_path / "old.png", film)
    yk.write_png(tmp_path / "old_way.png", yk.present(yk.tone_map(film, yk.ToneMapType.default(), 16), (28, 20), abi.PRESENT_ENCODE_SRGB, "rgba8"))
    assert (tmp_path / "old.png").read_bytes() == (tmp_path / "old_way.png").read_bytes()
    yk.write_preview(tmp_path / "auto.png", film, auto_exposure=True)
    yk.write_png(tmp_path / "auto_way.png", yk.present(chain, (28, 20), abi.PRESENT_ENCODE_SRGB, "rgba8"))
    assert (tmp_path / "auto.png").read_bytes() == (tmp_path / "auto_way.png").read_bytes()
    assert (tmp_path / "auto.png").read_bytes() != (tmp_path / "old.png").read_bytes()


def test_same_brightness_under_a_hundredfold_light(yk, tmp_path):
    """A film and the same film a hundred times darker come out of write_preview(auto_exposure=True) at the same
    brightness: the exposures differ by the factor, to the meter's resolution of 0.0875 stop."""
    rng = np.random.default_rng(5)
    film = ref.lognormal_film(rng, 30, 40, sigma_stops=2.0, specials=False) * np.float32(6.0)
    a = yk.meter_exposure(film, 16)
    b = yk.meter_exposure(film * np.float32(0.01), 16)
    assert abs(np.log2(b.exposure / a.exposure) - np.log2(100.0)) <= 2 * 0.0875
    fa = yk.tone_map(film, yk.ToneMapType.default(), 16, exposure_state=a)
    fb = yk.tone_map(film * np.float32(0.01), yk.ToneMapType.default(), 16, exposure_state=b)
    assert abs(float(fa.mean()) / float(fb.mean()) - 1) < 0.15 and 0.05 < float(fa.mean()) < 0.95
    plain = yk.tone_map(film * np.float32(0.01), yk.ToneMapType.default(), 16)
    assert b.exposure > 50.0 * a.exposure and float(plain.mean()) < float(fb.mean())  # the fixed exposure leaves it darker
