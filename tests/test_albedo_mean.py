"""The pixel-mean albedo (yk_albedo_mean: the mean of the first-hit albedo over an s x s grid of sub-pixel rays, the rule of
include/yuki_hip.h and yuki_amd/csrc/yk_albedo.h) on the host: the library's host instance against an independent numpy
float32 restatement (tests/albedo_mean_ref.py) bit for bit on the oracle's ids and on synthetic ids of every material kind,
the identities of the rule, three planted mistakes the comparison must catch, the argument errors, the Python layer, and
the quality condition on oracle-rendered films: denoise(albedo=mean) against denoise(albedo=centre).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import albedo_mean_ref as mref
import albedo_ref as ref
from test_albedo import scene_sources
from test_denoise import SEED
from test_motion import oracle_view
from test_temporal import camera, same_bits
from yuki_amd import _ffi, abi, scenes

F = np.float32
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


def _where(got, want):
    return np.argwhere(got.view(np.uint32).reshape(got.shape + (4,)) != want.view(np.uint32).reshape(got.shape + (4,)))[:4]


@pytest.fixture(scope="module")
def scene_views(yk, oracle, tmp_path_factory):
    """name -> (scene data, host-only scene, {(output res, s): the oracle's ids of the s-times larger film})."""
    out = {}
    for name, (sd, cam) in scene_sources(tmp_path_factory).items():
        osc = oracle.OracleScene(sd)
        views = {}
        for w, h in mref.SIZES:
            for s in mref.FACTORS:
                big = (s * w, s * h)
                ids = oracle_view(oracle, osc, sd, camera(yk, cam, big), big)[1]
                ids.setflags(write=False)
                views[((w, h), s)] = ids
        osc.close()
        out[name] = (sd, yk.Scene(None, sd), views)
    yield out
    for _, sc, _ in out.values():
        sc.close()


# ------------------------------------------------------------------ the host instance against the restatement
@pytest.mark.parametrize("name", ["textured-city", "textured-cornell", "textured-pbrt"])
def test_mean_host_equals_restatement_on_oracle_ids(yk, oracle, scene_views, name):
    sd, scene, views = scene_views[name]
    mixed = 0
    for ((w, h), s), ids in views.items():
        got = yk.albedo_mean(scene, ids, s)
        want = mref.albedo_mean(ids, s, sd, oracle.texture_eval)
        assert got.shape == want.shape == (h, w) and got.dtype == abi.ALBEDO_DTYPE
        assert same_bits(got, want), (name, (w, h), s, _where(got, want))
        assert np.isin(got["known"], (0.0, 1.0)).all()
        centre = yk.surface_albedo(scene, ids)
        if s == 1:
            assert same_bits(got, centre), (name, (w, h))  # s = 1: yk_surface_albedo's record
        else:
            mixed += int((got["known"] == 1).sum() - (centre.reshape(h, s, w, s)["known"] == 1).all(axis=(1, 3)).sum())
    assert mixed > 0, name  # the views hold pixels whose block is partly known: edges


def test_mean_host_equals_restatement_on_every_kind(yk, oracle):
    """ref.kinds_scene under synthetic ids: every material kind, every out-of-range id case, in every block."""
    sd = ref.kinds_scene()
    scene = yk.Scene(None, sd)
    rng = np.random.default_rng(20261021)
    for w, h in mref.SIZES:
        for s in mref.FACTORS:
            ids = ref.kinds_ids(rng, s * w, s * h, sd)
            got = yk.albedo_mean(scene, ids, s)
            want = mref.albedo_mean(ids, s, sd, oracle.texture_eval)
            assert same_bits(got, want), ((w, h), s, _where(got, want))
            assert np.isin(got["known"], (0.0, 1.0)).all()
    scene.close()


def test_identities(yk, oracle):
    sd = ref.kinds_scene()
    scene = yk.Scene(None, sd)
    rng = np.random.default_rng(7)
    ids = ref.kinds_ids(rng, 37, 23, sd)
    assert same_bits(yk.albedo_mean(scene, ids, 1), yk.surface_albedo(scene, ids))  # s = 1, bit for bit
    nt, ns = sd.n_triangles, len(sd.spheres)
    for s in (2, 3, 4, 8):
        # all-unknown blocks: misses, out-of-range shapes, glass, metal, glossy, a textured sphere -> (1, 1, 1, 0) exactly
        unknown = np.array([ref.SURFACE_NONE, nt + ns, 0xFFFFFFFE, 0x80000000, 12, 14, 16, nt + 1], np.uint32)
        ids = np.zeros((5 * s, 3 * s), abi.SURFACE_ID_DTYPE)
        ids["shape"] = unknown[rng.integers(0, len(unknown), size=ids.shape)]
        ids["b"] = rng.random(ids.shape + (3,), dtype=np.float32)
        got = yk.albedo_mean(scene, ids, s)
        assert same_bits(got["a"], np.ones((5, 3, 3), np.float32)) and not got["known"].view(np.uint32).any(), s
        # one known sub-sample in the last place of one block: known, and the mean is (s*s - 1 + Kd) / (s*s) per channel
        ids["shape"][2 * s - 1, 2 * s - 1] = 6  # material 3: a plain matte, Kd (0.7, 0.01, 0.4)
        got = yk.albedo_mean(scene, ids, s)
        assert got["known"].sum() == 1 and got["known"][1, 1] == 1
        n = F(s * s)
        want = ((n - F(1)) + np.array([0.7, 0.01, 0.4], np.float32)).astype(np.float32) / n
        assert same_bits(got["a"][1, 1], want.astype(np.float32)), (s, got["a"][1, 1], want)
        # a uniform block is its own record: n * Kd / n for a Kd the sum keeps exact (0.25, 0.5, 0.75 of the minimal scene)
    small = yk.Scene(None, ref.minimal_scene())
    for s in (2, 3, 4, 8):
        ids = np.zeros((2 * s, 3 * s), abi.SURFACE_ID_DTYPE)
        ids["b"] = F(1.0 / 3.0)
        got = yk.albedo_mean(small, ids, s)
        assert same_bits(got["a"], np.broadcast_to(np.array([0.25, 0.5, 0.75], np.float32), (2, 3, 3))) and (got["known"] == 1).all()
    small.close()
    scene.close()


# ------------------------------------------------------------------ planted mistakes
@pytest.mark.parametrize("planted", [dict(divide_by=3), dict(i_outer=True), dict(known_from_centre=True)], ids=["divide-by-s", "i-outer", "known-from-centre"])
def test_planted_mistakes_break_the_comparison(yk, oracle, scene_views, planted):
    """Each wrong variant of the restatement differs from the library where the right one equals it (textured-city, 37 x 23,
    s = 3)."""
    sd, scene, views = scene_views["textured-city"]
    ids = views[((37, 23), 3)]
    got = yk.albedo_mean(scene, ids, 3)
    assert same_bits(got, mref.albedo_mean(ids, 3, sd, oracle.texture_eval))
    assert not same_bits(got, mref.albedo_mean(ids, 3, sd, oracle.texture_eval, **planted)), planted


# ------------------------------------------------------------------ argument errors and the Python layer
def test_every_refusal(yk):
    L = _ffi.lib()
    sd = ref.minimal_scene()
    scene = yk.Scene(None, sd)
    w, h, s = 4, 3, 2
    ids = np.zeros((s * h, s * w), abi.SURFACE_ID_DTYPE)
    out = np.zeros((h, w), abi.ALBEDO_DTYPE)
    call = lambda sc=scene.h, i=ids, rx=w, ry=h, ss=s, o=out: L.yk_albedo_mean(None, sc, vp(i), rx, ry, ss, vp(o))  # noqa: E731
    assert call() == 0
    assert call(sc=None) == 1 and call(i=None) == 1 and call(o=None) == 1
    assert call(rx=0) == 1 and call(ry=0) == 1
    big = np.zeros((8 * h, 8 * w), abi.SURFACE_ID_DTYPE)
    assert call(i=big, ss=8) == 0 and call(i=big, ss=0) == 1 and call(i=big, ss=9) == 1 and call(i=big, ss=0xFFFFFFFF) == 1
    # s * res over 65535: refused before anything is read (the arrays are far too short for it)
    assert call(rx=32768, ry=1, ss=2) == 1 and call(rx=1, ry=32768, ss=2) == 1 and call(rx=8192, ry=1, ss=8) == 1
    one = np.zeros((1, 65535), abi.SURFACE_ID_DTYPE)
    assert L.yk_albedo_mean(None, scene.h, vp(one), 65535, 1, 1, vp(np.zeros((1, 65535), abi.ALBEDO_DTYPE))) == 0  # the limit itself
    # overlap: the output inside the ids, at their end, and just past them
    both = np.zeros(16 * (s * s * w * h + w * h), np.uint8)
    base = both.ctypes.data
    n_ids = 16 * s * s * w * h
    assert L.yk_albedo_mean(None, scene.h, C.c_void_p(base), w, h, s, C.c_void_p(base)) == 1
    assert L.yk_albedo_mean(None, scene.h, C.c_void_p(base), w, h, s, C.c_void_p(base + n_ids - 16)) == 1
    assert L.yk_albedo_mean(None, scene.h, C.c_void_p(base), w, h, s, C.c_void_p(base + n_ids)) == 0
    assert L.yk_albedo_mean(None, scene.h, C.c_void_p(base + 16 * w * h - 16), w, h, s, C.c_void_p(base)) == 1
    # the device forms need a context
    cam = camera(yk, sd.camera, (s * w, s * h))
    assert L.yk_albedo_mean_device(None, scene.h, vp(ids), w, h, s, vp(out), None) == 1
    assert L.yk_render_albedo_mean(None, scene.h, C.byref(cam.matrices), w, h, s, vp(out)) == 1
    assert L.yk_render_albedo_mean_device(None, scene.h, C.byref(cam.matrices), w, h, s, vp(out), None) == 1
    # the Python layer
    for bad_s in (0, 9, -1):
        with pytest.raises(ValueError):
            yk.albedo_mean(scene, ids, bad_s)
    with pytest.raises(ValueError):
        yk.albedo_mean(scene, ids, 4)  # 6 x 8 ids are no multiple of 4
    with pytest.raises(ValueError):
        yk.albedo_mean(scene, ids.reshape(-1), 2)
    with pytest.raises(ValueError):
        yk.supersampled(yk.FilmSettings(res=(32768, 4), tile_dim=16), 2)
    assert yk.supersampled(yk.FilmSettings(res=(96, 54), tile_dim=16), 4).res == (384, 216)
    scene.close()


def test_python_layer_consumers_take_the_record(yk, tmp_path):
    """write_output / write_preview / variance take the mean record where they take surface_albedo's."""
    from test_denoise import _flat_guides

    sd = ref.kinds_scene()
    scene = yk.Scene(None, sd)
    rng = np.random.default_rng(17)
    w, h, s = 37, 23, 2
    mean = yk.albedo_mean(scene, ref.kinds_ids(rng, s * w, s * h, sd), s)
    scene.close()
    film = rng.random((h, w, 3), dtype=np.float32)
    guides = _flat_guides(w, h)
    p = yk.DenoiseParams(iterations=2, sigma_plane=0.06)
    a, b = tmp_path / "a.exr", tmp_path / "b.exr"
    yk.write_output(a, film, yk.ToneMapType.Raw, denoise=p, guides=guides)
    yk.write_output(b, film, yk.ToneMapType.Raw, denoise=p, guides=guides, albedo=mean)
    assert a.read_bytes() != b.read_bytes()
    yk.write_preview(tmp_path / "a.png", film, denoise=p, guides=guides)
    yk.write_preview(tmp_path / "b.png", film, denoise=p, guides=guides, albedo=mean)
    assert (tmp_path / "a.png").read_bytes() != (tmp_path / "b.png").read_bytes()
    v = yk.variance(None, film, guides, yk.VarianceParams(), albedo=mean)
    assert v.shape == (h, w) and np.isfinite(v).all()


# ------------------------------------------------------------------ quality
def quality_films(yk, oracle, sd, res, q):
    """(noisy, converged, guides, {s: ids of the s-times larger film}) of the oracle at the scene's camera."""
    fs = yk.FilmSettings(res=res, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    osc = oracle.OracleScene(sd)
    integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, q["depth"], 0, 0.0)
    noisy = yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, q["noisy_spp"], 1, 1, SEED), integ, tiles, n_threads=0)[0], fs.res)
    conv = yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, q["converged_spp"], 1, 1, SEED ^ 0x1234567), integ, tiles, n_threads=0)[0], fs.res)
    guides, ids1 = oracle_view(oracle, osc, sd, cam, fs.res)
    ids = {1: ids1}
    for s in (2, 4):
        big = (s * res[0], s * res[1])
        ids[s] = oracle_view(oracle, osc, sd, camera(yk, sd.camera, big), big)[1]
    osc.close()
    return noisy, conv, guides, ids


def quality_ratios(yk, scene, noisy, conv, guides, ids, q, ctx=None):
    """denoise(albedo=mean_s) against denoise(albedo=centre): {s: (whole-film ratio, masked ratio)}, the mask's share of the
    film, and the centre error.  The mask: the pixels whose s = 4 mean differs from the centre record."""
    i = scene.info()
    diag = float(np.linalg.norm(np.array(i.bounds_max[:], np.float64) - np.array(i.bounds_min[:], np.float64)))
    p = yk.DenoiseParams(q["iterations"], q["sigma_color"], q["sigma_normal"], q["plane_fraction"] * diag)
    centre = yk.surface_albedo(scene, ids[1], ctx=ctx)
    mean = {s: yk.albedo_mean(scene, ids[s], s, ctx=ctx) for s in (2, 4)}
    mask = mref.differs(mean[4], centre)
    d_centre = yk.denoise(noisy, guides, p, albedo=centre, ctx=ctx)
    e_centre = ref.quality_error(d_centre, conv)
    m_centre = ref.quality_error(d_centre, conv, mask) if mask.any() else float("nan")
    out = {}
    for s in (2, 4):
        d = yk.denoise(noisy, guides, p, albedo=mean[s], ctx=ctx)
        out[s] = (ref.quality_error(d, conv) / e_centre, ref.quality_error(d, conv, mask) / m_centre if mask.any() else float("nan"))
    return out, float(mask.mean()), e_centre


def test_quality_on_oracle_films(yk, oracle):
    """textured-city at 96 x 54, Path depth 8, Uniform 4 spp against 1024 spp, 4 iterations at the library's default sigmas:
    the error of denoise(albedo=mean) against the error of denoise(albedo=centre), on the whole film and on the pixels
    whose s = 4 mean differs from the centre record by more than 0.02 in some channel.  The measured values stand beside
    the bounds in albedo_mean_ref.QUALITY."""
    q, mq = ref.QUALITY, mref.QUALITY
    sd = ref.textured_city()
    noisy, conv, guides, ids = quality_films(yk, oracle, sd, q["res"], q)
    scene = yk.Scene(None, sd)
    ratios, share, e_centre = quality_ratios(yk, scene, noisy, conv, guides, ids, q)
    scene.close()
    print(f"quality: centre {e_centre:.4f}; mean s=2 {ratios[2][0]:.4f} x (masked {ratios[2][1]:.4f} x), s=4 {ratios[4][0]:.4f} x (masked {ratios[4][1]:.4f} x); mask {share:.3f} of the film")
    assert share > mq["mask_min"], share
    for s in (2, 4):
        assert ratios[s][0] <= mq["whole"][s], (s, ratios[s])
        assert ratios[s][1] <= mq["masked"][s], (s, ratios[s])


@pytest.mark.parametrize("name", ["textured-cornell", "city-small"])
def test_nothing_is_lost_where_there_is_nothing_to_gain(yk, oracle, name):
    """Textured-cornell at 48 x 48 (texels far larger than a pixel) and untextured city-small at 64 x 36: the mean-albedo
    error does not exceed the centre-albedo error by more than the measured ratio plus 0.01."""
    q = ref.QUALITY
    res, bound = mref.QUALITY["no_gain"][name]
    sd = ref.textured_cornell() if name == "textured-cornell" else scenes.by_name(name)
    noisy, conv, guides, ids = quality_films(yk, oracle, sd, res, q)
    scene = yk.Scene(None, sd)
    ratios, share, e_centre = quality_ratios(yk, scene, noisy, conv, guides, ids, q)
    scene.close()
    print(f"quality ({name}): centre {e_centre:.4f}; mean s=2 {ratios[2][0]:.4f} x, s=4 {ratios[4][0]:.4f} x; mask {share:.3f} of the film")
    for s in (2, 4):
        assert ratios[s][0] <= bound, (name, s, ratios[s])
