"""The guided upsample (yuki_amd/csrc/yk_upsample.h) on the CPU: yk_upsample without a context against the independent
restatement tests/upsample_ref.py bit for bit, the geometry against exact rationals, what the pass is for (a texture comes
back, nothing bleeds across a silhouette or a crease), its refusals, and its benefit over a bilinear stretch on the
oracle's films."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import albedo_mean_ref as mref
import albedo_ref as aref
import upsample_ref as ref
from test_motion import oracle_view
from test_temporal import same_bits
from yuki_amd import _ffi, abi, scenes

F = np.float32
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
CASES = ref.host_cases()


def _exp(oracle):
    return lambda x: oracle.libm_array(6, x)


def _params(yk, s, sig):
    return yk.UpsampleParams(s=s, sigma_normal=sig[0], sigma_plane=sig[1])


def test_symbols_and_layout(yk):
    L = _ffi.lib()
    assert hasattr(L, "yk_upsample") and hasattr(L, "yk_upsample_device")
    assert C.sizeof(abi.UpsampleDesc) == 12 and abi.UPSAMPLE_MAX_S == abi.ALBEDO_MEAN_MAX_S == ref.MAX_S
    d = yk.UpsampleParams(3, 0.25).as_struct()
    assert (d.s, d.sigma_normal, d.sigma_plane) == (3, 0.25, float("inf"))


# ------------------------------------------------------------------ the host instance against the restatement
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_equals_restatement(yk, oracle, case):
    _, s, sig, td, (low, lg, g, la, a, samples) = case
    got, gw = yk.upsample(low, lg, g, _params(yk, s, sig), tile_dim=td, samples=samples, low_albedo=la, albedo=a, return_weight=True)
    want, ww = ref.upsample(low, lg, g, s, sig[0], sig[1], _exp(oracle), tile_dim=td, samples=samples, low_albedo=la, albedo=a)
    assert got.shape == want.shape == (g.shape[0], g.shape[1], 3) and got.dtype == np.float32
    bad = ref.bits(got) != ref.bits(want)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])
    assert same_bits(gw, ww), np.argwhere(ref.bits(gw) != ref.bits(ww))[:4]
    # without the second output the first is the same
    assert same_bits(got, yk.upsample(low, lg, g, _params(yk, s, sig), tile_dim=td, samples=samples, low_albedo=la, albedo=a))


def test_cases_reach_every_skip_case(oracle):
    """The random records hold what the rule distinguishes: NaN / inf channels, both hit classes against each other, a
    weight that underflows to 0, b == 0 taps, border footprints and pixels where everything is rejected."""
    seen = dict(nonfinite=0, mixed=0, underflow=0, b_zero=0, fallback=0, partial=0)
    for _, s, sig, td, (low, lg, g, la, a, samples) in CASES:
        _, sw = ref.upsample(low, lg, g, s, sig[0], sig[1], _exp(oracle), tile_dim=td, samples=samples, low_albedo=la, albedo=a)
        seen["nonfinite"] += int((~np.isfinite(low)).sum())
        seen["fallback"] += int((sw == 0).sum())
        seen["partial"] += int(((sw > 0) & (sw < F(0.5))).sum())
        Xs, Ys = ref.axis(low.shape[1], s)[0], ref.axis(low.shape[0], s)[0]
        seen["mixed"] += int(((g["hit"] != 0) != (lg["hit"][Ys[:, None], Xs[None, :]] != 0)).sum())
        if s % 2:
            seen["b_zero"] += 1
        if sig[0] == 0.1 and la is None and samples is None:
            # across the crease |dn|^2 = 1.44: e = 144 > 103.97, the weight underflows; the same records without stops keep it
            _, sw_open = ref.upsample(low, lg, g, s, ref.INF, ref.INF, _exp(oracle))
            seen["underflow"] += int(((sw_open > 0) & (sw < sw_open * F(0.75))).sum())
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("planted", ["plus-one", "fallback"])
def test_planted_mistakes_break_the_comparison(yk, oracle, planted, monkeypatch):
    """The comparison can tell: a restatement with one of the rule's choices changed no longer matches."""
    _, s, sig, td, (low, lg, g, la, a, samples) = next(c for c in CASES if c[1] == 3 and c[4][3] is not None)
    kw = dict(tile_dim=td, samples=samples, low_albedo=la, albedo=a)
    if planted == "plus-one":  # a = t + 1 rounded once from the exact rational, not the float sum after the division
        real = ref.axis

        def axis(n_low, s):
            X, x0, _ = real(n_low, s)
            exact = [ref.axis_exact(int(X[k]), k - s * int(X[k]), s)[1] for k in range(s * n_low)]
            return X, x0, np.array([float(v) for v in exact], np.float32)

        monkeypatch.setattr(ref, "axis", axis)
        want, _ = ref.upsample(low, lg, g, s, sig[0], sig[1], _exp(oracle), **kw)
    else:  # the fallback takes the raw film, not c_Q
        want, sw = ref.upsample(low, lg, g, s, sig[0], sig[1], _exp(oracle), **kw)
        Xs, Ys = ref.axis(low.shape[1], s)[0], ref.axis(low.shape[0], s)[0]
        with np.errstate(all="ignore"):
            raw = ref.canon((low[Ys[:, None], Xs[None, :]] * aref.divisor(a["a"])).astype(np.float32))
        want = np.where((sw == 0)[..., None], raw, want)
    got = yk.upsample(low, lg, g, _params(yk, s, sig), **kw)
    assert not same_bits(got, want)


# ------------------------------------------------------------------ geometry
@pytest.mark.parametrize("s", range(1, 9))
def test_geometry_against_exact_rationals(yk, s):
    """(x0, ax) of every i: the restatement's axis against Fractions, and the host instance through a film whose weight
    output is one tap's b — every full pixel a miss, one low pixel Q a miss and the other eight hits, so sw is b of Q where
    Q is in the footprint with b != 0 and 0 elsewhere."""
    lw = lh = 3
    X, x0, a = ref.axis(lw, s)
    want_x0, want_a = [], []
    for x in range(s * lw):
        e0, ea = ref.axis_exact(x // s, x % s, s)
        t = Fraction(2 * (x % s) + 1 - s, 2 * s)
        rounded = F(F(float(t)) + F(1)) if t < 0 else F(float(t))  # the rule: one division, then one sum
        assert abs(Fraction(float(rounded)) - ea) <= Fraction(1, 1 << 24) and 0 <= ea < 1
        if s & (s - 1) == 0:
            assert Fraction(float(rounded)) == ea  # a power of two: every step is exact
        want_x0.append(e0)
        want_a.append(rounded)
    assert list(x0) == want_x0 and list(X) == [x // s for x in range(s * lw)]
    assert same_bits(a, np.array(want_a, np.float32))
    low = np.ones((lh, lw, 3), np.float32)
    g = np.zeros((s * lh, s * lw), abi.GUIDE_DTYPE)
    p = yk.UpsampleParams(s=s)
    for Qy in range(lh):
        for Qx in range(lw):
            lg = ref.plane_guides(lw, lh)
            lg[Qy, Qx] = np.zeros((), abi.GUIDE_DTYPE)
            _, sw = yk.upsample(low, lg, g, p, return_weight=True)
            want = np.zeros((s * lh, s * lw), np.float32)
            for y in range(s * lh):
                for x in range(s * lw):
                    wx = {want_x0[x]: F(1) - want_a[x], want_x0[x] + 1: want_a[x]}.get(Qx, F(0))
                    wy = {want_x0[y]: F(1) - want_a[y], want_x0[y] + 1: want_a[y]}.get(Qy, F(0))
                    want[y, x] = F(wx * wy)
            assert same_bits(sw, want), (s, Qx, Qy)


# ------------------------------------------------------------------ what the pass is for
@pytest.mark.parametrize("s", [2, 3, 4])
def test_texture_recovery(yk, oracle, s):
    """One plane under constant irradiance E: the low film is E x the low mean albedo, and the upsample returns E x the
    FULL albedo within 1e-6 relative (about eight binary32 roundings of 2^-24: 5e-7).  A bilinear stretch of the same film
    misses that by orders of magnitude."""
    lw, lh = 13, 7
    rng = np.random.default_rng(7 + s)
    albedo = np.zeros((s * lh, s * lw), abi.ALBEDO_DTYPE)
    albedo["a"] = (F(abi.ALBEDO_FLOOR) + rng.random((s * lh, s * lw, 3), dtype=np.float32) * F(0.9)).astype(np.float32)
    albedo["known"] = 1.0
    low_albedo = mref.block_mean(albedo, s)
    E = np.array([1.7, 0.9, 0.3], np.float32)
    low = (E * low_albedo["a"]).astype(np.float32)
    want = E.astype(np.float64) * albedo["a"].astype(np.float64)
    lg, g = ref.plane_guides(lw, lh), ref.plane_guides(s * lw, s * lh)
    got, sw = yk.upsample(low, lg, g, yk.UpsampleParams(s=s, sigma_normal=0.3, sigma_plane=0.06), low_albedo=low_albedo, albedo=albedo, return_weight=True)
    e_guided = ref.rel_error(got, want)
    bil, _ = ref.upsample(low, lg, g, s, 0.3, 0.06, _exp(oracle), bilinear=True)
    e_bilinear = ref.rel_error(bil, want)
    print(f"texture recovery s={s}: guided {e_guided:.3e}, bilinear {e_bilinear:.3e}")
    assert (sw > 0).all()
    assert e_guided <= 1e-6, e_guided
    assert not e_bilinear <= 1e-6 and e_bilinear > 1e-2, e_bilinear


def _two_sides(s, lw, lh, kind):
    """A film of two sides whose low colours are far apart (about 1 and about 1000).  kind "sky": an object against the
    sky (hit | miss); "crease": two surfaces whose normals differ by |dn|^2 = 2.  The boundary is no multiple of s at full
    resolution, so full pixels of one side lie in low pixels of the other."""
    rng = np.random.default_rng(11)
    W, H = s * lw, s * lh
    xb = s * (lw // 2) + 1
    side_full = np.broadcast_to(np.arange(W)[None, :] >= xb, (H, W))
    side_low = np.broadcast_to(np.arange(lw)[None, :] >= lw // 2, (lh, lw))

    def guides(side):
        g = np.zeros(side.shape, abi.GUIDE_DTYPE)
        g["ns"] = np.where(side[..., None], np.array([0, 1, 0], np.float32), np.array([1, 0, 0], np.float32))
        g["hit"] = 1.0
        if kind == "sky":
            g[side] = np.zeros((), abi.GUIDE_DTYPE)
        return g

    low = (np.where(side_low[..., None], F(1000), F(1)) * (F(1) + rng.random((lh, lw, 3), dtype=np.float32) * F(0.5))).astype(np.float32)
    return low, guides(side_low), guides(side_full), side_low, side_full


@pytest.mark.parametrize("kind", ["sky", "crease"])
@pytest.mark.parametrize("s", [2, 3])
def test_no_bleeding(yk, oracle, kind, s):
    """A hit next to a miss has w = 0; across the crease e = 2 / 0.1^2 = 200 > 103.97, det_expf underflows and the tap is
    skipped.  So every full pixel is built from taps of its own side only: its bits equal the restatement run on that side
    alone (the other side's low pixels made NaN), and its value lies between that side's extremes."""
    low, lg, g, side_low, side_full = _two_sides(s, 9, 5, kind)
    p = yk.UpsampleParams(s=s, sigma_normal=0.1, sigma_plane=None)
    got, sw = yk.upsample(low, lg, g, p, return_weight=True)
    assert (sw > 0).all()
    for side in (False, True):
        alone = low.copy()
        alone[side_low != side] = np.nan
        want, _ = ref.upsample(alone, lg, g, s, 0.1, ref.INF, _exp(oracle))
        mine = side_full == side
        assert same_bits(got[mine], want[mine]), (kind, s, side)
        own = low[side_low == side]
        assert np.isfinite(got[mine]).all() and got[mine].min() >= own.min() * (1 - 1e-6) and got[mine].max() <= own.max() * (1 + 1e-6)


@pytest.mark.parametrize("s", [1, 2, 3])
def test_nan_pixel_does_not_spread_and_weight_marks_the_fallback(yk, s):
    lw, lh = 6, 5
    rng = np.random.default_rng(3)
    low = rng.random((lh, lw, 3), dtype=np.float32)
    low[2, 3, 1] = np.nan
    lg, g = ref.plane_guides(lw, lh), ref.plane_guides(s * lw, s * lh)
    g[0, 0] = np.zeros((), abi.GUIDE_DTYPE)  # a feature no low ray hit: every tap is of the other class
    got, sw = yk.upsample(low, lg, g, yk.UpsampleParams(s=s), return_weight=True)
    Xs, Ys = np.arange(s * lw) // s, np.arange(s * lh) // s
    own = low[Ys[:, None], Xs[None, :]]
    fell = sw == 0
    assert fell[0, 0] and same_bits(got[fell], own[fell])  # the fallback copies the containing pixel's bits
    nan_px = np.isnan(got).any(-1)
    in_nan_low = (Ys[:, None] == 2) & (Xs[None, :] == 3)
    assert not (nan_px & ~(fell & in_nan_low)).any()
    if s % 2:  # the centre column and row of an odd s have one tap with b != 0: the NaN pixel itself
        assert nan_px[2 * s + s // 2, 3 * s + s // 2]
    else:
        assert not nan_px.any()


# ------------------------------------------------------------------ argument errors and the Python layer
def test_every_refusal(yk):
    L = _ffi.lib()
    lw, lh, s = 4, 3, 2
    n_lo, n = lw * lh, s * s * lw * lh
    low, lg, la = np.zeros((lh, lw, 3), np.float32), np.zeros(n_lo, abi.GUIDE_DTYPE), np.zeros(n_lo, abi.ALBEDO_DTYPE)
    g, a = np.zeros(n, abi.GUIDE_DTYPE), np.zeros(n, abi.ALBEDO_DTYPE)
    out, wt = np.zeros(3 * n, np.float32), np.zeros(n, np.float32)

    def call(d=(s, 0.3, 0.06), low=low, lg=lg, la=la, rx=lw, ry=lh, td=16, g=g, a=a, out=out, wt=wt, desc=True):
        return L.yk_upsample(None, C.byref(abi.UpsampleDesc(*d)) if desc else None, vp(low), vp(lg), vp(la), rx, ry, td, None, vp(g), vp(a), vp(out), vp(wt))

    assert call() == 0 and call(wt=None) == 0 and call(la=None, a=None) == 0
    assert call(desc=False) == 1 and call(low=None) == 1 and call(lg=None) == 1 and call(g=None) == 1 and call(out=None) == 1
    assert call(rx=0) == 1 and call(ry=0) == 1 and call(td=0) == 1
    assert call(d=(0, 0.3, 0.06)) == 1 and call(d=(9, 0.3, 0.06)) == 1 and call(d=(0xFFFFFFFF, 0.3, 0.06)) == 1
    assert call(d=(2, 0.3, 0.06), rx=32768, ry=1) == 1 and call(d=(8, 0.3, 0.06), rx=1, ry=8192) == 1  # before anything is read
    for bad in (0.0, -1.0, float("nan")):
        assert call(d=(s, bad, 0.06)) == 1 and call(d=(s, 0.3, bad)) == 1
    assert call(d=(s, float("inf"), float("inf"))) == 0
    assert call(la=None) == 1 and call(a=None) == 1  # one albedo without the other
    # overlap: an output inside an input, at its end, and just past it; the two outputs
    buf = np.zeros(32 * n + 4 * n + 12 * n + 64, np.uint8)
    base = buf.ctypes.data
    at = lambda off: C.c_void_p(base + off)  # noqa: E731
    d = C.byref(abi.UpsampleDesc(s, 0.3, 0.06))
    two = lambda g_off, out_off, w_off=None: L.yk_upsample(None, d, vp(low), vp(lg), None, lw, lh, 16, None, at(g_off), None, at(out_off), None if w_off is None else at(w_off))  # noqa: E731
    assert two(0, 0) == 1 and two(0, 32 * n - 4) == 1 and two(0, 32 * n) == 0 and two(12 * n - 4, 0) == 1 and two(12 * n, 0) == 0
    assert two(0, 32 * n, 32 * n) == 1 and two(0, 32 * n, 32 * n + 12 * n - 4) == 1 and two(0, 32 * n, 16) == 1 and two(0, 32 * n + 4 * n, 32 * n) == 0
    for name, arr in (("low", low), ("lg", lg), ("la", la), ("a", a)):
        assert call(out=arr.reshape(-1).view(np.float32)) == 1, name
        assert call(wt=arr.reshape(-1).view(np.float32)) == 1, name
    # the device form needs a context
    assert L.yk_upsample_device(None, d, vp(low), vp(lg), None, lw, lh, 16, None, vp(g), None, vp(out), None, None) == 1


def test_python_layer(yk):
    fs = yk.FilmSettings(res=(96, 54), tile_dim=16)
    assert yk.subsampled(fs, 2).res == (48, 27) and yk.subsampled(fs, 1).res == (96, 54)
    assert yk.supersampled(yk.subsampled(fs, 2), 2).res == fs.res
    for bad_s in (4, 5, 0, 9):  # 54 is no multiple of 4; 96 none of 5; outside 1 .. 8
        with pytest.raises(ValueError):
            yk.subsampled(fs, bad_s)
    lw, lh, s = 4, 3, 2
    low, lg, g = np.zeros((lh, lw, 3), np.float32), ref.plane_guides(lw, lh), ref.plane_guides(s * lw, s * lh)
    la, a = np.zeros((lh, lw), abi.ALBEDO_DTYPE), np.zeros((s * lh, s * lw), abi.ALBEDO_DTYPE)
    p = yk.UpsampleParams(s=s)
    assert yk.upsample(low, lg, g, p).shape == (s * lh, s * lw, 3)
    with pytest.raises(ValueError):
        yk.upsample(low, lg, g, p, low_albedo=la)
    with pytest.raises(ValueError):
        yk.upsample(low, lg, g, p, albedo=a)
    with pytest.raises(ValueError):
        yk.upsample(low, lg, lg, p)  # the guides are the full film's
    with pytest.raises(ValueError):
        yk.upsample(low, lg, g, yk.UpsampleParams(s=9))
    with pytest.raises(TypeError):
        yk.upsample(low, lg, g, yk.DenoiseParams())
    with pytest.raises(ValueError):
        yk.upsample(low, lg, g, p, samples=np.zeros(7, np.uint32))
    sd = scenes.by_name("city-tiny")
    scene = yk.Scene(None, sd)
    q, dq = yk.UpsampleParams.for_scene(scene, 4), yk.DenoiseParams.for_scene(scene)
    scene.close()
    assert (q.s, q.sigma_normal, q.sigma_plane) == (4, dq.sigma_normal, dq.sigma_plane)


# ------------------------------------------------------------------ quality
MEAN_S = 4  # the "mean" route: pixel-mean albedo records from the ids of the MEAN_S-times larger film, at both resolutions


def quality_inputs(yk, oracle, sd, res, s, q, mean_s=MEAN_S):
    """The oracle's films: (low noisy, full converged, low guides, full guides, full ids, ids of the mean_s-times larger
    film)."""
    from test_denoise import SEED

    fs = yk.FilmSettings(res=res, tile_dim=16)
    lfs, bfs = yk.subsampled(fs, s), yk.supersampled(fs, mean_s)
    osc = oracle.OracleScene(sd)
    integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, q["depth"], 0, 0.0)
    cam, tiles = yk.Camera(sd.camera, fs), yk.film_tiles(fs)
    lcam, ltiles = yk.Camera(sd.camera, lfs), yk.film_tiles(lfs)
    low = yk.update_tiles(ltiles, osc.render_tiles(lcam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, q["noisy_spp"], 1, 1, SEED), integ, ltiles, n_threads=0)[0], lfs.res)
    conv = yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, q["converged_spp"], 1, 1, SEED ^ 0x1234567), integ, tiles, n_threads=0)[0], fs.res)
    low_guides = oracle_view(oracle, osc, sd, lcam, lfs.res)[0]
    guides, ids = oracle_view(oracle, osc, sd, cam, res)
    ids_big = oracle_view(oracle, osc, sd, yk.Camera(sd.camera, bfs), bfs.res)[1]
    osc.close()
    return low, conv, low_guides, guides, ids, ids_big


def quality_ratios(yk, oracle, scene, low, conv, low_guides, guides, ids, ids_big, s, q, route, ctx=None, mean_s=MEAN_S):
    """The three upsamples of the demodulated-denoised low film against the converged full film: (e_guided, e_geom,
    e_bilinear) on the whole film and on the mask, the mask's share and the guided fallback's share.  route "centre": the
    full albedo is surface_albedo's centre-ray record and the low one its mean over the s x s block; "mean": both are
    pixel means over the MEAN_S-times larger film's ids (factors MEAN_S and s * MEAN_S), the records for texels smaller
    than a pixel.  The mask: the full pixels whose albedo record differs from their containing low pixel's."""
    i = scene.info()
    diag = float(np.linalg.norm(np.array(i.bounds_max[:], np.float64) - np.array(i.bounds_min[:], np.float64)))
    dp = yk.DenoiseParams(q["iterations"], q["sigma_color"], q["sigma_normal"], q["plane_fraction"] * diag)
    up = yk.UpsampleParams(s, q["sigma_normal"], q["plane_fraction"] * diag)
    if route == "centre":
        albedo, low_albedo = yk.surface_albedo(scene, ids, ctx=ctx), yk.albedo_mean(scene, ids, s, ctx=ctx)
    else:
        albedo, low_albedo = yk.albedo_mean(scene, ids_big, mean_s, ctx=ctx), yk.albedo_mean(scene, ids_big, s * mean_s, ctx=ctx)
    clean = yk.denoise(low, low_guides, dp, albedo=low_albedo, ctx=ctx)
    guided, sw = yk.upsample(clean, low_guides, guides, up, low_albedo=low_albedo, albedo=albedo, ctx=ctx, return_weight=True)
    geom = yk.upsample(clean, low_guides, guides, up, ctx=ctx)
    bilinear, _ = ref.upsample(clean, low_guides, guides, s, up.sigma_normal, up.sigma_plane, _exp(oracle), bilinear=True)
    Xs, Ys = ref.axis(low.shape[1], s)[0], ref.axis(low.shape[0], s)[0]
    mask = mref.differs(albedo, low_albedo[Ys[:, None], Xs[None, :]])
    whole = tuple(aref.quality_error(x, conv) for x in (guided, geom, bilinear))
    masked = tuple(aref.quality_error(x, conv, mask) for x in (guided, geom, bilinear)) if mask.any() else (float("nan"),) * 3
    return whole, masked, float(mask.mean()), float((sw == 0).mean())


def check_quality(whole, masked, share, fallback, route, scene="textured-city", key=None):
    q = ref.QUALITY[key or route]
    print(f"quality ({scene}, {route} albedo): guided {whole[0]:.4f}, geom {whole[1]:.4f}, bilinear {whole[2]:.4f}: guided / bilinear {whole[0] / whole[2]:.4f} "
          f"(masked {masked[0] / masked[2]:.4f}); mask {share:.4f} of the film; fallback {fallback:.4f} of the film")
    assert share > q["mask_min"], share
    assert whole[0] / whole[2] <= q["whole"], whole
    assert masked[0] / masked[2] <= q["masked"], masked


@pytest.fixture(scope="module")
def city_films(yk, oracle):
    q = aref.QUALITY
    sd = aref.textured_city()
    return sd, quality_inputs(yk, oracle, sd, q["res"], ref.QUALITY["s"], q)


@pytest.mark.parametrize("route", ["centre", "mean"])
def test_quality_on_oracle_films(yk, oracle, city_films, route):
    """textured-city, full 96 x 54, s = 2: the 4-spp 48 x 27 film, denoised, upsampled three ways, against the 1024-spp full
    film.  The measured values stand beside the bounds in upsample_ref.QUALITY."""
    sd, inputs = city_films
    scene = yk.Scene(None, sd)
    whole, masked, share, fallback = quality_ratios(yk, oracle, scene, *inputs, ref.QUALITY["s"], aref.QUALITY, route)
    scene.close()
    check_quality(whole, masked, share, fallback, route)


def test_quality_where_texels_are_larger_than_a_pixel(yk, oracle):
    """textured-cornell, full 96 x 96, s = 2, the centre ray's albedo and its 2 x 2 mean — the records the pass was first
    described with, on a scene they suit.  The measured values stand beside the bounds in upsample_ref.QUALITY."""
    q, s = aref.QUALITY, ref.QUALITY["s"]
    sd = aref.textured_cornell()
    inputs = quality_inputs(yk, oracle, sd, ref.QUALITY["larger_texels"]["res"], s, q)
    scene = yk.Scene(None, sd)
    whole, masked, share, fallback = quality_ratios(yk, oracle, scene, *inputs, s, q, "centre")
    scene.close()
    check_quality(whole, masked, share, fallback, "centre", scene="textured-cornell", key="larger_texels")


def test_nothing_is_lost_where_there_is_nothing_to_demodulate(yk, oracle):
    """Untextured city-small at 64 x 36: the guided error does not exceed the geometry-only error by more than the measured
    ratio plus 0.01."""
    q, s = aref.QUALITY, ref.QUALITY["s"]
    res, bound = ref.QUALITY["no_gain"]["city-small"]
    sd = scenes.by_name("city-small")
    inputs = quality_inputs(yk, oracle, sd, res, s, q)
    scene = yk.Scene(None, sd)
    whole, masked, share, fallback = quality_ratios(yk, oracle, scene, *inputs, s, q, "centre")
    scene.close()
    print(f"quality (city-small): guided {whole[0]:.4f}, geom {whole[1]:.4f}, bilinear {whole[2]:.4f}; guided / geom {whole[0] / whole[1]:.4f}; fallback {fallback:.4f} of the film")
    assert whole[0] / whole[1] <= bound, whole
