"""The variance-guided denoise (yuki_amd/csrc/yk_variance.h: carried luminance moments, the variance image, the à-trous
filter whose colour stop follows it) on the host: the library's host instance against an independent numpy float32
restatement (tests/variance_ref.py, exp from the oracle's libm) bit for bit, the record layout, the reprojection of a
moments buffer through the existing entry point, the exact properties of the rule, the argument errors, the Python layer,
and the quality conditions on oracle-rendered films.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import temporal_ref
import variance_ref as ref
from test_denoise import SEED, _flat_guides, oracle_guides, quality_error
from yuki_amd import _ffi, abi, scenes

F = np.float32
PIC = ref.pictures()
BLEND_CASES, VARIANCE_CASES, FILTER_CASES = ref.blend_cases(PIC), ref.variance_cases(PIC), ref.filter_cases(PIC)
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


def _exp(oracle):
    return lambda x: oracle.libm_array(6, x)


def vparams(yk, it=3, sig=ref.SIGMAS, eps=ref.EPSILON, scale=ref.SCALE):
    return yk.VarianceParams(iterations=it, sigma_variance=sig[0], sigma_normal=sig[1], sigma_plane=sig[2], epsilon=eps, spatial_scale=scale)


def tparams(yk, max_history=ref.MAX_HISTORY):
    return yk.TemporalParams(plane_tolerance=0.05, normal_cos_min=0.9, max_history=max_history)


def same_bits(got, want):
    bad = ref.bits(got) != ref.bits(want)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], np.asarray(got)[bad][:4], np.asarray(want)[bad][:4])


def moments_words(m):
    return np.ascontiguousarray(m).view(np.float32).reshape(m.shape + (4,))


# ------------------------------------------------------------------ layout
def test_record_layout():
    assert abi.MOMENTS_DTYPE.itemsize == 16 and abi.MOMENTS_DTYPE == ref.MOMENTS_DTYPE
    assert [abi.MOMENTS_DTYPE.fields[k][1] for k in ("m1", "m2", "frames", "n")] == [0, 4, 8, 12]
    assert abi.MOMENTS_DTYPE.fields["n"][1] == abi.HISTORY_DTYPE.fields["n"][1] and abi.HISTORY_DTYPE.itemsize == 16
    assert C.sizeof(abi.VarianceDesc) == 24
    assert [getattr(abi.VarianceDesc, k).offset for k in ("iterations", "sigma_variance", "sigma_normal", "sigma_plane", "epsilon", "spatial_scale")] == [0, 4, 8, 12, 16, 20]


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("case", BLEND_CASES, ids=[c[0] for c in BLEND_CASES])
def test_moments_blend_host_equals_restatement(yk, case):
    _, size, td, sk, hist = case
    p = PIC[size]
    samples = None if sk is None else p[sk]
    moments = p["moments"] if hist else None
    got = yk.blend_moments(p["film"], tparams(yk), tile_dim=td, samples=samples, moments=moments)
    want = ref.blend_moments(p["film"], ref.MAX_HISTORY, td, samples, moments)
    same_bits(moments_words(got), moments_words(want))


@pytest.mark.parametrize("case", VARIANCE_CASES, ids=[c[0] for c in VARIANCE_CASES])
def test_variance_host_equals_restatement(yk, oracle, case):
    _, size, mk, alb, td, sk, (sn, sp) = case
    p = PIC[size]
    samples = None if sk is None else p[sk]
    moments = None if mk is None else p[mk]
    albedo = p["albedo"] if alb else None
    got = yk.variance(moments, p["film"], p["guides"], vparams(yk, sig=(4.0, sn, sp)), tile_dim=td, samples=samples, albedo=albedo)
    want = ref.variance(moments, p["film"], p["guides"], sn, sp, ref.SCALE, _exp(oracle), td, samples, albedo)
    assert got.shape == want.shape and got.dtype == np.float32
    same_bits(got, want)
    assert not np.isnan(got).any() and not (got < 0).any()
    if mk == "moments_patch":  # both estimates in one film
        assert (got[30:38, 60:68] != ref.variance(moments, p["film"], p["guides"], sn, sp, 0.0, _exp(oracle))[30:38, 60:68]).any()


@pytest.mark.parametrize("case", FILTER_CASES, ids=[c[0] for c in FILTER_CASES])
def test_filter_host_equals_restatement(yk, oracle, case):
    _, size, it, sig, alb, td, sk = case
    p = PIC[size]
    samples = None if sk is None else p[sk]
    albedo = p["albedo"] if alb else None
    got = yk.denoise(p["film"], p["guides"], vparams(yk, it, sig), tile_dim=td, samples=samples, albedo=albedo, variance=p["variance"])
    want = ref.denoise_variance(p["film"], p["guides"], p["variance"], it, *sig, ref.EPSILON, _exp(oracle), td, samples, albedo)
    assert got.shape == want.shape and got.dtype == np.float32
    same_bits(got, want)


def test_chain_host_equals_restatement(yk, oracle):
    """blend -> blend -> variance -> filter, each step fed with the previous one's output."""
    p = PIC[(37, 23)]
    rng = np.random.default_rng(3)
    film2 = ref.make_film(rng, 37, 23)
    m = yk.blend_moments(p["film"], tparams(yk), samples=p["samples"])
    m = yk.blend_moments(film2, tparams(yk), moments=m)
    w = ref.blend_moments(film2, ref.MAX_HISTORY, moments=ref.blend_moments(p["film"], ref.MAX_HISTORY, 16, p["samples"]))
    same_bits(moments_words(m), moments_words(w))
    assert (m["frames"] == 2).any() and (m["frames"] == 1).any()
    var = yk.variance(m, film2, p["guides"], vparams(yk))
    same_bits(var, ref.variance(w, film2, p["guides"], *ref.SIGMAS[1:], ref.SCALE, _exp(oracle)))
    out = yk.denoise(film2, p["guides"], vparams(yk, 3), variance=var)
    same_bits(out, ref.denoise_variance(film2, p["guides"], var, 3, *ref.SIGMAS, ref.EPSILON, _exp(oracle)))


# ------------------------------------------------------------------ reprojection through the existing entry point
@pytest.mark.parametrize("pair", ["translate", "dolly-in"])
def test_a_moments_buffer_reprojects_through_yk_history_reproject(yk, pair):
    w, h = 37, 23
    rng = np.random.default_rng(12)
    fs = yk.FilmSettings(res=(w, h), tile_dim=16)
    cp, cc = yk.Camera(temporal_ref.CAMERA_PAIRS[pair][0], fs), yk.Camera(temporal_ref.CAMERA_PAIRS[pair][1], fs)
    gp, gc = temporal_ref.plane_guides(cp.matrices, w, h, rng), temporal_ref.plane_guides(cc.matrices, w, h, rng)
    moments = PIC[(w, h)]["moments"]
    got = yk.reproject_history(moments.view(abi.HISTORY_DTYPE), gp, cp, gc, tparams(yk))
    want = ref.reproject_moments(moments, gp, cp.matrices, gc, 0.05, 0.9)
    same_bits(moments_words(got), moments_words(want))
    assert (got["n"] > 0).any() and (got["n"] == 0).any()


# ------------------------------------------------------------------ exact properties
def test_blended_count_equals_history_blend_and_frames_follow_the_clamp(yk):
    rng = np.random.default_rng(13)
    w, h = 37, 23
    film = (F(0.5) + rng.random((h, w, 3), dtype=np.float32)).astype(np.float32)
    samples = np.array([1, 2, 0, 5, 8, 3], np.uint32)  # 3 x 2 tiles
    tp = tparams(yk, max_history=10.0)
    hist, mom = None, None
    for k in range(6):
        _, hist = yk.blend_history(film * F(k + 1), tp, samples=samples, history=hist)
        mom = yk.blend_moments(film * F(k + 1), tp, samples=samples, moments=mom)
        assert np.array_equal(ref.bits(hist["n"]), ref.bits(mom["n"]))
    m = ref.tonemap_ref.sample_counts(h, w, 16, samples)
    live = m > 0
    assert np.all(mom["n"][live] <= 10.0 + m[live]) and np.all(mom["frames"][~live] == 0)
    # unclamped, frames counts the blends; once the clamp bites it grows by less than one a blend
    one = live & (m * 5 <= 10.0)  # the count before the sixth blend was not clamped
    assert one.any() and np.all(mom["frames"][one] == 6)
    clamped = live & (m * 5 > 10.0)
    assert clamped.any() and np.all(mom["frames"][clamped] < 6) and np.all(mom["frames"][clamped] > 1)
    # a clamp alone (no current view): frames scale with the count
    old = np.zeros((h, w), abi.MOMENTS_DTYPE)
    old["m1"], old["m2"], old["frames"], old["n"] = 0.5, 0.3, 8.0, 40.0
    kept = yk.blend_moments(film, tp, samples=np.zeros_like(samples), moments=old)
    assert np.all(kept["n"] == 10.0) and np.all(kept["frames"] == 2.0) and np.all(kept["m1"] == F(0.5))


def test_a_non_finite_pixel_does_not_poison_the_moments(yk):
    w, h = 8, 6
    film = np.full((h, w, 3), 0.5, np.float32)
    tp = tparams(yk)
    m0 = yk.blend_moments(film, tp)
    bad = film.copy()
    bad[2, 3, 1], bad[4, 5, 0], bad[1, 1, 2] = np.nan, np.inf, 1e30
    m1 = yk.blend_moments(bad, tp, moments=m0)
    for y, x in ((2, 3), (4, 5), (1, 1)):
        assert m1[y, x] == m0[y, x]  # the sample was dropped, the moments kept
    assert np.isfinite(moments_words(m1)).all()
    m2 = yk.blend_moments(film, tp, moments=m1)
    assert m2["frames"][2, 3] == 2 and m2["frames"][0, 0] == 3 and np.isfinite(moments_words(m2)).all()
    first = yk.blend_moments(bad, tp)  # no moments to keep: the zero record
    assert not moments_words(first)[2, 3].view(np.uint32).any()


def test_a_constant_film_has_variance_zero_and_comes_back_unchanged(yk):
    w, h = 64, 36
    film = np.full((h, w, 3), 0.375, np.float32)
    guides = _flat_guides(w, h)
    tp = tparams(yk)
    m = None
    for _ in range(3):
        m = yk.blend_moments(film, tp, moments=m)
    for moments in (None, m):
        var = yk.variance(moments, film, guides, vparams(yk))
        assert not ref.bits(var).any()
        out = yk.denoise(film, guides, vparams(yk, 5), variance=var)
        assert np.all(np.abs(out.astype(np.float64) - 0.375) <= 1e-6)
    zeros = np.zeros((h, w, 3), np.float32)
    out = yk.denoise(zeros, ref.make_guides(np.random.default_rng(6), w, h), vparams(yk, 5), variance=yk.variance(None, zeros, guides, vparams(yk)))
    assert not ref.bits(out).any()  # zeros stay zeros


def test_bad_pixels_and_an_infinite_variance_do_not_spread(yk):
    rng = np.random.default_rng(7)
    w, h = 64, 36
    film = rng.random((h, w, 3), dtype=np.float32)
    film[17, 30, 1] = np.inf
    guides = _flat_guides(w, h)
    var = np.full((h, w), 0.05, np.float32)
    out = yk.denoise(film, guides, vparams(yk, 5), variance=var)
    finite = np.isfinite(out)
    assert not finite[17, 30, 1] and finite.sum() == finite.size - 1
    nan_film = film.copy()
    nan_film[17, 30] = np.nan
    out = yk.denoise(nan_film, guides, vparams(yk, 5), variance=var)
    assert np.all(ref.bits(out[17, 30]) == 0x7FC00000) and np.isnan(out).sum() == 3
    v = yk.variance(None, nan_film, guides, vparams(yk))
    assert np.isfinite(v).all() and v[17, 30] == 0
    # an infinite variance opens the colour stop of its own pixel only: two tones, a variance that keeps them apart, one
    # pixel of the dark half with variance +inf next to the edge.  Were +inf to spread, the dark pixels around it would
    # lose their colour stop after an iteration and take the bright half in.
    film = np.full((h, w, 3), 0.2, np.float32)
    film[:, w // 2 :] = 0.8
    film += (rng.random((h, w, 3), dtype=np.float32) - F(0.5)) * F(0.02)
    var = np.full((h, w), 1e-4, np.float32)
    p = vparams(yk, 4, sig=(2.0, 0.3, ref.INF))
    base = yk.denoise(film, guides, p, variance=var)
    var[18, w // 2 - 2] = np.inf
    out = yk.denoise(film, guides, p, variance=var)
    dark = np.ones((h, w), bool)
    dark[:, w // 2 :] = False
    dark[18, w // 2 - 2] = False
    assert out[18, w // 2 - 2].max() > 0.3  # the pixel itself is filtered without a colour stop
    assert out[dark].max() < 0.25 and base[dark].max() < 0.25
    assert np.abs(out[dark] - base[dark]).max() < 0.02


def test_no_leak_across_a_plane_gap(yk):
    w, h, sp = 64, 36, 0.06
    A = np.array([0.7, 0.4, 0.2], np.float32)
    film = np.zeros((h, w, 3), np.float32)
    film[:, : w // 2] = A
    guides = _flat_guides(w, h)
    guides["p"][:, w // 2 :, 2] = F(1e6 * sp)
    var = yk.variance(None, film, guides, vparams(yk))
    # the window does not cross the gap either: 0 on the black side, the rounding of s2 / s0 - mean * mean on the other (a
    # window that took both sides in would measure about 0.05)
    assert not ref.bits(var[:, w // 2 :]).any() and var.max() < 1e-6
    out = yk.denoise(film, guides, vparams(yk, 5, sig=(ref.INF, 0.3, sp)), variance=np.full((h, w), np.inf, np.float32))
    assert not ref.bits(out[:, w // 2 :]).any()
    assert np.all(np.abs(out[:, : w // 2].astype(np.float64) - A) <= 1e-6 * A)


@pytest.mark.parametrize("size", [(37, 23), (64, 36)])
def test_infinite_variance_everywhere_is_denoise_without_a_colour_stop(yk, size):
    """With var = +inf at every pixel g is +inf, the colour term is 0 for every finite luminance difference, and the filter
    is yk_denoise with sigma_color = +inf — on films whose finite values do not make a channel difference overflow where
    the luminance difference does not (yk_variance.h says which): denoise_ref's films hold ordinary values and +-1e30."""
    p = PIC[size]
    inf = np.full(size[::-1], np.inf, np.float32)
    for it in (1, 3, 5):
        got = yk.denoise(p["film"], p["guides"], vparams(yk, it), variance=inf)
        want = yk.denoise(p["film"], p["guides"], yk.DenoiseParams(it, ref.INF, ref.SIGMAS[1], ref.SIGMAS[2]))
        same_bits(got, want)


def test_in_place_equals_out_of_place(yk):
    L = _ffi.lib()
    p = PIC[(37, 23)]
    for it in (0, 1, 3):
        for albedo in (None, p["albedo"]):
            vpar = vparams(yk, it)
            want = yk.denoise(p["film"], p["guides"], vpar, variance=p["variance"], albedo=albedo)
            buf = p["film"].copy()
            d = vpar.as_struct()
            assert L.yk_denoise_variance(None, C.byref(d), vp(buf), vp(p["guides"]), vp(p["variance"]), vp(albedo), 37, 23, 16, None, vp(buf)) == 0
            assert np.array_equal(ref.bits(buf), ref.bits(want))
    tp = tparams(yk).as_struct()
    m = p["moments"].copy()
    want = yk.blend_moments(p["film"], tparams(yk), moments=p["moments"])
    assert L.yk_moments_blend(None, C.byref(tp), vp(p["film"]), 37, 23, 16, None, vp(m), vp(m)) == 0
    assert np.array_equal(moments_words(m).view(np.uint32), moments_words(want).view(np.uint32))


def test_zero_iterations_return_the_normalised_film_bits(yk):
    p = PIC[(37, 23)]
    film = p["film"].copy()
    film.reshape(-1).view(np.uint32)[::7] = 0x7FA12345
    got = yk.denoise(film, p["guides"], vparams(yk, 0), variance=p["variance"], albedo=p["albedo"])
    assert np.array_equal(ref.bits(got), ref.bits(film))
    got = yk.denoise(film, p["guides"], vparams(yk, 0), samples=p["samples"], variance=p["variance"])
    assert np.array_equal(ref.bits(got), ref.bits(ref.denoise_ref.normalise(film, 16, p["samples"])))


# ------------------------------------------------------------------ refusals
def test_every_refusal(yk):
    L = _ffi.lib()
    w, h = 8, 6
    film = np.zeros((h, w, 3), np.float32)
    guides = np.zeros((h, w), abi.GUIDE_DTYPE)
    var = np.zeros((h, w), np.float32)
    albedo = np.zeros((h, w), abi.ALBEDO_DTYPE)
    moments = np.zeros((h, w), abi.MOMENTS_DTYPE)
    out = np.zeros_like(film)
    out_var = np.zeros_like(var)
    out_m = np.zeros_like(moments)
    GOOD = (3, 4.0, 0.3, 0.06, 1e-8, 0.25)

    def filt(desc=GOOD, f=film, g=guides, v=var, a=albedo, rx=w, ry=h, td=16, o=out, null_desc=False):
        d = abi.VarianceDesc(*desc)
        return L.yk_denoise_variance(None, None if null_desc else C.byref(d), vp(f), vp(g), vp(v), vp(a), rx, ry, td, None, vp(o))

    def vari(desc=GOOD, m=moments, f=film, g=guides, a=albedo, rx=w, ry=h, td=16, o=out_var, null_desc=False):
        d = abi.VarianceDesc(*desc)
        return L.yk_variance(None, None if null_desc else C.byref(d), vp(m), vp(f), vp(g), vp(a), rx, ry, td, None, vp(o))

    def blend(desc=(0.05, 0.9, 24.0), f=film, rx=w, ry=h, td=16, m=moments, o=out_m, null_desc=False):
        d = abi.TemporalDesc(*desc)
        return L.yk_moments_blend(None, None if null_desc else C.byref(d), vp(f), rx, ry, td, None, vp(m), vp(o))

    for call in (filt, vari):
        assert call() == 0 and call(a=None) == 0
        assert call(desc=(8, *GOOD[1:])) == 0 and call(desc=(9, *GOOD[1:])) == 1
        for k in (1, 2, 3):
            for bad in (0.0, -1.0, float("nan"), -float("inf")):
                desc = list(GOOD)
                desc[k] = bad
                assert call(desc=tuple(desc)) == 1, (call.__name__, k, bad)
        for k in (4, 5):
            for bad in (-1.0, float("nan"), -float("inf")):
                desc = list(GOOD)
                desc[k] = bad
                assert call(desc=tuple(desc)) == 1, (call.__name__, k, bad)
            desc = list(GOOD)
            desc[k] = 0.0
            assert call(desc=tuple(desc)) == 0
        assert call(null_desc=True) == 1 and call(f=None) == 1 and call(g=None) == 1 and call(o=None) == 1
        assert call(rx=0) == 1 and call(ry=0) == 1 and call(td=0) == 1
    assert filt(v=None) == 1 and vari(m=None) == 0
    assert blend() == 0 and blend(m=None) == 0 and blend(null_desc=True) == 1 and blend(f=None) == 1 and blend(o=None) == 1
    assert blend(rx=0) == 1 and blend(ry=0) == 1 and blend(td=0) == 1
    for desc in ((0.0, 0.9, 24.0), (0.05, 1.5, 24.0), (0.05, 0.9, 0.5), (0.05, 0.9, float("nan")), (float("nan"), 0.9, 24.0)):
        assert blend(desc=desc) == 1, desc
    # overlaps: one buffer, the output starting inside an input's last record; adjacent is fine
    n = w * h
    d = abi.VarianceDesc(*GOOD)
    t = abi.TemporalDesc(0.05, 0.9, 24.0)
    big = np.zeros(n * 32 + n * 16, np.uint8)
    b = big.ctypes.data
    P = C.c_void_p
    for size, args in ((n * 32, lambda i, o: (vp(film), i, vp(var), vp(albedo), o)), (n * 4, lambda i, o: (vp(film), vp(guides), i, vp(albedo), o)), (n * 16, lambda i, o: (vp(film), vp(guides), vp(var), i, o))):
        f, g, v, a, o = args(P(b), P(b + size - 4))
        assert L.yk_denoise_variance(None, C.byref(d), f, g, v, a, w, h, 16, None, o) == 1
        f, g, v, a, o = args(P(b), P(b + size))
        assert L.yk_denoise_variance(None, C.byref(d), f, g, v, a, w, h, 16, None, o) == 0
    assert L.yk_denoise_variance(None, C.byref(d), vp(film), vp(guides), vp(var), None, w, h, 16, None, P(film.ctypes.data + 12)) == 1
    assert L.yk_denoise_variance(None, C.byref(d), vp(film), vp(guides), vp(var), None, w, h, 16, None, vp(film)) == 0  # in place
    for size, args in ((n * 16, lambda i, o: (i, vp(film), vp(guides), vp(albedo), o)), (n * 12, lambda i, o: (vp(moments), i, vp(guides), vp(albedo), o)),
                       (n * 32, lambda i, o: (vp(moments), vp(film), i, vp(albedo), o)), (n * 16, lambda i, o: (vp(moments), vp(film), vp(guides), i, o))):  # fmt: skip
        m, f, g, a, o = args(P(b), P(b + size - 4))
        assert L.yk_variance(None, C.byref(d), m, f, g, a, w, h, 16, None, o) == 1
        m, f, g, a, o = args(P(b), P(b + size))
        assert L.yk_variance(None, C.byref(d), m, f, g, a, w, h, 16, None, o) == 0
    assert L.yk_moments_blend(None, C.byref(t), P(b), w, h, 16, None, None, P(b + n * 12 - 4)) == 1
    assert L.yk_moments_blend(None, C.byref(t), P(b), w, h, 16, None, None, P(b + n * 12 + 4)) == 0
    assert L.yk_moments_blend(None, C.byref(t), vp(film), w, h, 16, None, P(b), P(b + 16)) == 1
    assert L.yk_moments_blend(None, C.byref(t), vp(film), w, h, 16, None, P(b), P(b)) == 0  # in place
    # the _device forms refuse a NULL context
    assert L.yk_moments_blend_device(None, C.byref(t), vp(film), w, h, 16, None, None, vp(out_m), None) == 1
    assert L.yk_variance_device(None, C.byref(d), None, vp(film), vp(guides), None, w, h, 16, None, vp(out_var), None) == 1
    assert L.yk_denoise_variance_device(None, C.byref(d), vp(film), vp(guides), vp(var), None, w, h, 16, None, vp(out), None) == 1


# ------------------------------------------------------------------ the Python layer
def test_python_layer(yk, tmp_path):
    p = yk.VarianceParams()
    assert (p.iterations, p.sigma_variance, p.sigma_normal, p.sigma_plane, p.epsilon, p.spatial_scale) == (5, QUALITY["sigma_variance"], 0.3, None, QUALITY["epsilon"], QUALITY["spatial_scale"])
    assert p.as_struct().sigma_plane == float("inf")

    class FakeScene:
        def info(self):
            i = _ffi.SceneInfo()
            i.bounds_min[:] = (0.0, 0.0, 0.0)
            i.bounds_max[:] = (3.0, 4.0, 12.0)
            return i

    q = yk.VarianceParams.for_scene(FakeScene(), iterations=3)
    assert q.iterations == 3 and abs(q.sigma_plane - 0.13) < 1e-12
    rng = np.random.default_rng(10)
    film = rng.random((23, 37, 3), dtype=np.float32)
    guides = _flat_guides(37, 23)
    vpar = yk.VarianceParams(iterations=2, sigma_plane=0.06)
    var = yk.variance(None, film, guides, vpar)
    a, c = tmp_path / "a.exr", tmp_path / "c.exr"
    yk.write_output(a, film, yk.ToneMapType.Raw)
    yk.write_output(c, film, yk.ToneMapType.Raw, denoise=vpar, guides=guides, variance=var)
    assert a.read_bytes() != c.read_bytes()
    yk.write_preview(tmp_path / "a.png", film)
    yk.write_preview(tmp_path / "c.png", film, denoise=vpar, guides=guides, variance=var)
    assert (tmp_path / "a.png").read_bytes() != (tmp_path / "c.png").read_bytes()
    with pytest.raises(ValueError):
        yk.denoise(film, guides, vpar)  # a VarianceParams without a variance
    with pytest.raises(TypeError):
        yk.denoise(film, guides, yk.DenoiseParams(), variance=var)
    with pytest.raises(ValueError):
        yk.denoise(film, guides, vpar, variance=var[:-1])
    with pytest.raises(ValueError):
        yk.write_output(c, film, variance=var)
    with pytest.raises(TypeError):
        yk.blend_moments(film, vpar)


# ------------------------------------------------------------------ quality on oracle films
# bound: the ratio e_var / e_plain the host instance measures at the defaults on city-small with four frames
# (profiles/variance_quality.json: `measured_ratio`), plus 0.05 for the step from oracle films to device films, rounded up
# to two decimals.
QUALITY = dict(depth=8, frame_spp=4, converged_spp=1024, iterations=3, sigma_variance=3.0, epsilon=1e-8, spatial_scale=1.0, measured_ratio=0.8036, bound=0.86,
               scenes=(("city-small", (64, 36)), ("cornell", (48, 48))))  # fmt: skip


@functools.lru_cache(maxsize=None)
def oracle_frames(name, res, n_frames):
    """(frames of frame_spp each, the converged film, guides, sigma_plane) of a scene, rendered by the oracle."""
    from oracle import binding as oracle
    from yuki_amd import core as yk

    q = QUALITY
    sd = scenes.by_name(name) if name != "cornell" else scenes.cornell()
    fs = yk.FilmSettings(res=res, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    osc = oracle.OracleScene(sd)
    integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, q["depth"], 0, 0.0)
    render = lambda spp, seed: yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, spp, 1, 1, seed), integ, tiles, n_threads=0)[0], fs.res)  # noqa: E731
    frames = [render(q["frame_spp"], SEED + 977 * k) for k in range(n_frames)]
    conv = render(q["converged_spp"], SEED ^ 0x1234567)
    guides = oracle_guides(oracle, osc, cam, fs.res)
    host_scene = yk.Scene(None, sd)
    sigma_plane = yk.DenoiseParams.for_scene(host_scene).sigma_plane
    host_scene.close()
    return frames, conv, guides, sigma_plane


def quality_errors(yk, frames, conv, guides, sigma_plane, n_frames, ctx=None):
    """(e_blended, e_plain, e_var) after n_frames frames folded by blend_history / blend_moments."""
    import test_denoise

    q = QUALITY
    tp = yk.TemporalParams(max_history=64.0)
    hist = mom = rgb = None
    for f in frames[:n_frames]:
        rgb, hist = yk.blend_history(f, tp, history=hist, ctx=ctx)
        mom = yk.blend_moments(f, tp, moments=mom, ctx=ctx)
    tq = test_denoise.QUALITY
    plain = yk.denoise(rgb, guides, yk.DenoiseParams(tq["iterations"], tq["sigma_color"], tq["sigma_normal"], sigma_plane), ctx=ctx)
    vpar = yk.VarianceParams(iterations=q["iterations"], sigma_plane=sigma_plane)
    var = yk.variance(mom, rgb, guides, vpar, ctx=ctx)
    out = yk.denoise(rgb, guides, vpar, variance=var, ctx=ctx)
    return quality_error(rgb, conv), quality_error(plain, conv), quality_error(out, conv)


@pytest.mark.parametrize("name,res", QUALITY["scenes"], ids=[s[0] for s in QUALITY["scenes"]])
def test_quality_four_frames(yk, name, res):
    frames, conv, guides, sp = oracle_frames(name, res, 8)
    e_blend, e_plain, e_var = quality_errors(yk, frames, conv, guides, sp, 4)
    print(f"quality {name} 4 frames: blended {e_blend:.4f} plain {e_plain:.4f} variance-guided {e_var:.4f} ratio {e_var / e_plain:.3f}")
    assert e_var < e_plain and e_var < e_blend, (e_blend, e_plain, e_var)
    if name == "city-small":
        assert QUALITY["bound"] < 1 and e_var <= QUALITY["bound"] * e_plain, (e_plain, e_var)


@pytest.mark.parametrize("name,res", QUALITY["scenes"], ids=[s[0] for s in QUALITY["scenes"]])
def test_quality_eight_frames(yk, name, res):
    frames, conv, guides, sp = oracle_frames(name, res, 8)
    e_blend, e_plain, e_var = quality_errors(yk, frames, conv, guides, sp, 8)
    print(f"quality {name} 8 frames: blended {e_blend:.4f} plain {e_plain:.4f} variance-guided {e_var:.4f}")
    assert e_var < e_blend, (e_blend, e_plain, e_var)


@pytest.mark.parametrize("name,res", QUALITY["scenes"], ids=[s[0] for s in QUALITY["scenes"]])
def test_quality_one_frame_spatial(yk, name, res):
    frames, conv, guides, sp = oracle_frames(name, res, 8)
    e_noisy, e_plain, e_var = quality_errors(yk, frames, conv, guides, sp, 1)
    print(f"quality {name} 1 frame (spatial estimate): noisy {e_noisy:.4f} plain {e_plain:.4f} variance-guided {e_var:.4f} ratio to plain {e_var / e_plain:.3f}")
    assert e_var < e_noisy, (e_noisy, e_var)
