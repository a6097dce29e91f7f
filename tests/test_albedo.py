"""The albedo passes (yuki_amd/csrc/yk_albedo.h: the first-hit albedo of every pixel from its surface id, and the à-trous
filter on radiance / albedo) on the host: the library's host instance against an independent numpy float32 restatement
(tests/albedo_ref.py) bit for bit, the exact properties of the rule, the argument errors, the Python layer, and the quality
condition on oracle-rendered films of a textured scene.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import albedo_ref as ref
import denoise_ref
import scene_files
from test_denoise import SEED, _flat_guides, oracle_guides, quality_error
from test_motion import oracle_view
from test_temporal import camera, same_bits
from yuki_amd import _ffi, abi, loaders

F = np.float32
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
FILTER_CASES = ref.filter_cases()


def _params(yk, it, sig):
    return yk.DenoiseParams(iterations=it, sigma_color=sig[0], sigma_normal=sig[1], sigma_plane=sig[2])


def _exp(oracle):
    return lambda x: oracle.libm_array(6, x)


def test_record_layout():
    assert abi.ALBEDO_DTYPE.itemsize == 16 and abi.ALBEDO_DTYPE == ref.ALBEDO_DTYPE
    assert [abi.ALBEDO_DTYPE.fields[k][1] for k in ("a", "known")] == [0, 12]
    assert np.array([abi.ALBEDO_FLOOR], np.float32).view(np.uint32)[0] == 0x3C800000 == np.array([ref.FLOOR]).view(np.uint32)[0]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yuki_hip.h")).read()
    assert "#define YK_ALBEDO_FLOOR 0.015625f" in hdr


# ------------------------------------------------------------------ yk_surface_albedo
def scene_sources(tmp_path_factory):
    """name -> (scene data, camera description): the three scenes of the issue."""
    sd_city, sd_cornell = ref.textured_city(), ref.textured_cornell()
    pbrt = scene_files.write_textured_scene(str(tmp_path_factory.mktemp("albedo_textured")))
    sd_pbrt, cam_p, _ = loaders.load_pbrt(pbrt)
    return {"textured-city": (sd_city, sd_city.camera), "textured-cornell": (sd_cornell, sd_cornell.camera), "textured-pbrt": (sd_pbrt, cam_p)}


@pytest.fixture(scope="module")
def scene_views(yk, oracle, tmp_path_factory):
    """name -> (scene data, host-only scene, the oracle's ids at the scene's camera on every film size)."""
    out = {}
    for name, (sd, cam) in scene_sources(tmp_path_factory).items():
        osc = oracle.OracleScene(sd)
        views = {res: oracle_view(oracle, osc, sd, camera(yk, cam, res), res)[1] for res in ref.SIZES}
        osc.close()
        out[name] = (sd, yk.Scene(None, sd), views)
    yield out
    for _, s, _ in out.values():
        s.close()


@pytest.mark.parametrize("name", ["textured-city", "textured-cornell", "textured-pbrt"])
def test_albedo_host_equals_restatement_on_oracle_ids(yk, oracle, scene_views, name):
    sd, scene, views = scene_views[name]
    for res, ids in views.items():
        got = yk.surface_albedo(scene, ids)
        want = ref.surface_albedo(ids, sd, oracle.texture_eval)
        assert got.shape == want.shape == (res[1], res[0]) and got.dtype == abi.ALBEDO_DTYPE
        assert same_bits(got, want), (name, res, np.argwhere(got.view(np.uint32).reshape(got.shape + (4,)) != want.view(np.uint32).reshape(got.shape + (4,)))[:4])
        assert np.isin(got["known"], (0.0, 1.0)).all() and (got["a"][got["known"] == 0] == 1).all()
        # the view shows the texture: known texels that are no material's Kd
        kds = {tuple(np.asarray(m.get("a", (0, 0, 0)), np.float32)) for m in sd.materials}
        texels = [tuple(a) for a in got["a"][got["known"] == 1].reshape(-1, 3) if tuple(a) not in kds]
        assert len(set(texels)) >= 3, (name, res)


def test_albedo_host_equals_restatement_on_every_kind(yk, oracle):
    sd = ref.kinds_scene()
    scene = yk.Scene(None, sd)
    rng = np.random.default_rng(20261020)
    nt, ns = sd.n_triangles, len(sd.spheres)
    seen = set()
    for w, h in ((64, 36), (37, 23), (1, 1)):
        ids = ref.kinds_ids(rng, w, h, sd)
        got = yk.surface_albedo(scene, ids)
        want = ref.surface_albedo(ids, sd, oracle.texture_eval)
        assert same_bits(got, want), (w, h, np.argwhere(got.view(np.uint32).reshape(got.shape + (4,)) != want.view(np.uint32).reshape(got.shape + (4,)))[:4])
        shape = ids["shape"].astype(np.int64)
        seen |= {"none"} if (ids["shape"] == ref.SURFACE_NONE).any() else set()
        seen |= {"range"} if ((shape >= nt + ns) & (ids["shape"] != ref.SURFACE_NONE)).any() else set()
        seen |= {f"mat{m}" for m in np.unique(np.asarray(sd.tri_material)[shape[shape < nt]])}
        seen |= {f"sph{k}" for k in np.unique(shape[(shape >= nt) & (shape < nt + ns)] - nt)}
    assert seen == {"none", "range"} | {f"mat{m}" for m in range(10)} | {f"sph{k}" for k in range(4)}, seen
    # by hand: corners of the uv quad, the 1 x 1 texture, the default uvs, the kinds that are not demodulated
    ids = np.zeros((1, 8), abi.SURFACE_ID_DTYPE)
    ids["shape"][0] = [0, 4, 2, 12, 14, 16, nt + 1, nt + 3]
    ids["b"][0] = [(1, 0, 0), (0.25, 0.5, 0.25), (0, 0, 1), (0.2, 0.3, 0.5), (0.2, 0.3, 0.5), (0.2, 0.3, 0.5), (0, 0, 0), (0, 0, 0)]
    got = yk.surface_albedo(scene, ids)[0]
    assert same_bits(got["a"][0], sd.textures[0][8, 0]) and got["known"][0] == 1  # uv (0, 0): the bottom-left texel, v flipped
    assert same_bits(got["a"][1], sd.textures[2][0, 0]) and got["known"][1] == 1
    assert same_bits(got["a"][2], oracle.texture_eval(sd.textures[1], np.array([[1.0, 1.0]], np.float32))[0])  # mesh 1 has no uvs: (1, 1) at vertex 2
    for k in (3, 4, 5, 6):
        assert (got["a"][k] == 1).all() and got["known"][k] == 0, k  # glass, metal, glossy, a textured sphere
    assert not got["a"][7].view(np.uint32).any() and got["known"][7] == 1  # a black matte sphere: Kd = 0 as bits
    scene.close()


def test_out_of_range_ids_are_never_followed(yk):
    """Shapes n_shapes, n_shapes + 1, 0xfffffffe and 0x80000000 on a scene whose arrays are as short as they can be."""
    sd = ref.minimal_scene()
    scene = yk.Scene(None, sd)
    ids = np.zeros((3, 5), abi.SURFACE_ID_DTYPE)
    ids["shape"] = np.array([1, 2, 0xFFFFFFFE, 0x80000000, ref.SURFACE_NONE], np.uint32)[None, :]
    ids["b"] = F(1.0 / 3.0)
    got = yk.surface_albedo(scene, ids)
    assert (got["a"] == 1).all() and not got["known"].any()
    ids["shape"] = 0
    got = yk.surface_albedo(scene, ids)
    assert same_bits(got["a"], np.broadcast_to(np.array([0.25, 0.5, 0.75], np.float32), (3, 5, 3))) and (got["known"] == 1).all()
    scene.close()


# ------------------------------------------------------------------ yk_denoise_albedo
@pytest.mark.parametrize("case", FILTER_CASES, ids=[c[0] for c in FILTER_CASES])
def test_denoise_albedo_host_equals_restatement(yk, oracle, case):
    _, film, guides, albedo, it, sig, td, samples = case
    got = yk.denoise(film, guides, _params(yk, it, sig), tile_dim=td, samples=samples, albedo=albedo)
    want = ref.denoise_albedo(film, guides, albedo, it, *sig, exp=_exp(oracle), tile_dim=td, samples=samples)
    assert got.shape == want.shape and got.dtype == np.float32
    bad = ref.bits(got) != ref.bits(want)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])


def test_special_values_are_all_met():
    """The cases above hold every special albedo value and NaN, +-inf and 1e30 film pixels."""
    a = np.concatenate([c[3]["a"].reshape(-1) for c in FILTER_CASES])
    for v in ref.SPECIAL_ALBEDO:
        assert (ref.bits(a) == ref.bits(np.array([v], np.float32))[0]).any(), v
    f = np.concatenate([c[1].reshape(-1) for c in FILTER_CASES])
    assert np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any() and (np.abs(f[np.isfinite(f)]) >= 1e28).any()
    assert np.array_equal(ref.divisor(np.array([0.0, -0.0, 0.015624999, 0.015625, 1.0, 3.5, np.nan, np.inf, -np.inf], np.float32)),
                          np.array([0.015625, 0.015625, 0.015625, 0.015625, 1.0, 3.5, 1.0, 1.0, 1.0], np.float32))


_ONES_CASES = denoise_ref.cases()


@pytest.mark.parametrize("case", _ONES_CASES, ids=[c[0] for c in _ONES_CASES])
def test_an_albedo_of_ones_is_plain_denoise(yk, case):
    _, film, guides, it, sig, td, samples = case
    ones = np.zeros(guides.shape, abi.ALBEDO_DTYPE)
    ones["a"] = 1.0
    got = yk.denoise(film, guides, _params(yk, it, sig), tile_dim=td, samples=samples, albedo=ones)
    assert np.array_equal(ref.bits(got), ref.bits(yk.denoise(film, guides, _params(yk, it, sig), tile_dim=td, samples=samples)))


def test_a_film_equal_to_its_albedo_comes_back(yk):
    """radiance / albedo is 1 everywhere, a filter of ones gives ones, times the albedo: the film, bit for bit — while the
    plain filter blurs the texture."""
    rng = np.random.default_rng(12)
    w, h = 64, 36
    albedo = np.zeros((h, w), abi.ALBEDO_DTYPE)
    albedo["a"] = (ref.FLOOR + (1 - ref.FLOOR) * rng.random((h, w, 3))).astype(np.float32)
    albedo["known"] = 1.0
    film = albedo["a"].copy()
    p = yk.DenoiseParams(iterations=5, sigma_color=float("inf"), sigma_normal=0.3, sigma_plane=0.06)
    guides = _flat_guides(w, h)
    assert np.array_equal(ref.bits(yk.denoise(film, guides, p, albedo=albedo)), ref.bits(film))
    assert not np.array_equal(ref.bits(yk.denoise(film, guides, p)), ref.bits(film))


def test_zeros_infinities_and_nans(yk):
    rng = np.random.default_rng(13)
    w, h = 64, 36
    albedo = ref.make_albedo(rng, w, h)
    guides = denoise_ref.make_guides(rng, w, h)
    p = yk.DenoiseParams(iterations=5, sigma_plane=0.06)
    assert not ref.bits(yk.denoise(np.zeros((h, w, 3), np.float32), guides, p, albedo=albedo)).any()  # a film of zeros stays zeros
    film = rng.random((h, w, 3), dtype=np.float32)
    film[17, 30, 1] = np.inf
    out = yk.denoise(film, _flat_guides(w, h), p, albedo=albedo)
    finite = np.isfinite(out)
    assert not finite[17, 30, 1] and finite.sum() == finite.size - 1  # an infinite pixel stays and does not spread
    film[17, 30] = np.nan
    out = yk.denoise(film, _flat_guides(w, h), p, albedo=albedo)
    assert np.all(ref.bits(out[17, 30]) == 0x7FC00000) and np.isnan(out).sum() == 3  # a NaN centre stays NaN, canonical
    # iterations = 0: the normalised film as bits, no division and no product
    film.reshape(-1).view(np.uint32)[::7] = 0x7FA12345
    samples = denoise_ref.make_samples(rng, w, h, 16)
    p0 = yk.DenoiseParams(iterations=0, sigma_plane=0.06)
    assert np.array_equal(ref.bits(yk.denoise(film, guides, p0, albedo=albedo)), ref.bits(film))
    assert np.array_equal(ref.bits(yk.denoise(film, guides, p0, samples=samples, albedo=albedo)), ref.bits(denoise_ref.normalise(film, 16, samples)))


def test_in_place_equals_out_of_place(yk):
    L = _ffi.lib()
    rng = np.random.default_rng(14)
    film, guides, albedo = denoise_ref.make_film(rng, 37, 23), denoise_ref.make_guides(rng, 37, 23), ref.make_albedo(rng, 37, 23)
    for it in (0, 1, 3):
        p = yk.DenoiseParams(iterations=it, sigma_plane=0.06)
        want = yk.denoise(film, guides, p, albedo=albedo)
        buf = film.copy()
        d = p.as_struct()
        assert L.yk_denoise_albedo(None, C.byref(d), vp(buf), vp(guides), vp(albedo), 37, 23, 16, None, vp(buf)) == 0
        assert np.array_equal(ref.bits(buf), ref.bits(want))


def test_every_refusal(yk, tmp_path):
    L = _ffi.lib()
    w, h = 8, 6
    film = np.zeros((h, w, 3), np.float32)
    guides = np.zeros((h, w), abi.GUIDE_DTYPE)
    albedo = np.zeros((h, w), abi.ALBEDO_DTYPE)
    out = np.zeros_like(film)

    def call(desc=None, f=film, g=guides, a=albedo, rx=w, ry=h, td=16, o=out, null_desc=False):
        d = abi.DenoiseDesc(3, 4.0, 0.3, 0.06) if desc is None else abi.DenoiseDesc(*desc)
        return L.yk_denoise_albedo(None, None if null_desc else C.byref(d), vp(f), vp(g), vp(a), rx, ry, td, None, vp(o))

    assert call() == 0
    assert call(desc=(8, 4.0, 0.3, 0.06)) == 0 and call(desc=(9, 4.0, 0.3, 0.06)) == 1
    for k in range(3):
        for bad in (0.0, -1.0, float("nan"), -float("inf")):
            sig = [4.0, 0.3, 0.06]
            sig[k] = bad
            assert call(desc=(3, *sig)) == 1, (k, bad)
    assert call(null_desc=True) == 1 and call(f=None) == 1 and call(g=None) == 1 and call(o=None) == 1 and call(a=None) == 1
    assert call(rx=0) == 1 and call(ry=0) == 1 and call(td=0) == 1
    d = abi.DenoiseDesc(3, 4.0, 0.3, 0.06)
    both = np.zeros(w * h * 32 + w * h * 12, np.uint8)  # the guides overlap the output
    base = both.ctypes.data
    assert L.yk_denoise_albedo(None, C.byref(d), vp(film), C.c_void_p(base), vp(albedo), w, h, 16, None, C.c_void_p(base + w * h * 32 - 4)) == 1
    assert L.yk_denoise_albedo(None, C.byref(d), vp(film), C.c_void_p(base), vp(albedo), w, h, 16, None, C.c_void_p(base + w * h * 32)) == 0
    both = np.zeros(w * h * 16 + w * h * 12, np.uint8)  # the albedo overlaps the output
    base = both.ctypes.data
    assert L.yk_denoise_albedo(None, C.byref(d), vp(film), vp(guides), C.c_void_p(base), w, h, 16, None, C.c_void_p(base + w * h * 16 - 4)) == 1
    assert L.yk_denoise_albedo(None, C.byref(d), vp(film), vp(guides), C.c_void_p(base), w, h, 16, None, C.c_void_p(base + w * h * 16)) == 0
    assert L.yk_denoise_albedo(None, C.byref(d), vp(film), vp(guides), vp(albedo), w, h, 16, None, C.c_void_p(film.ctypes.data + 12)) == 1
    assert L.yk_denoise_albedo(None, C.byref(d), vp(film), vp(guides), vp(albedo), w, h, 16, None, vp(film)) == 0  # in place
    # yk_surface_albedo
    sd = ref.minimal_scene()
    scene = yk.Scene(None, sd)
    ids = np.zeros((h, w), abi.SURFACE_ID_DTYPE)
    rec = np.zeros((h, w), abi.ALBEDO_DTYPE)
    assert L.yk_surface_albedo(None, scene.h, vp(ids), w, h, vp(rec)) == 0
    assert L.yk_surface_albedo(None, None, vp(ids), w, h, vp(rec)) == 1 and L.yk_surface_albedo(None, scene.h, None, w, h, vp(rec)) == 1
    assert L.yk_surface_albedo(None, scene.h, vp(ids), w, h, None) == 1 and L.yk_surface_albedo(None, scene.h, vp(ids), 0, h, vp(rec)) == 1
    assert L.yk_surface_albedo(None, scene.h, vp(ids), w, 0, vp(rec)) == 1 and L.yk_surface_albedo(None, scene.h, vp(ids), w, h, vp(ids)) == 1
    assert L.yk_surface_albedo_device(None, scene.h, vp(ids), w, h, vp(rec), None) == 1  # no context
    assert L.yk_denoise_albedo_device(None, C.byref(d), vp(film), vp(guides), vp(albedo), w, h, 16, None, vp(out), None) == 1
    # the Python layer
    with pytest.raises(_ffi.YukiError) as e:
        yk.denoise(film, guides, yk.DenoiseParams(iterations=9), albedo=albedo)
    assert e.value.status == 1
    with pytest.raises(ValueError):
        yk.denoise(film, guides, yk.DenoiseParams(), albedo=albedo[:-1])
    with pytest.raises(ValueError):
        yk.surface_albedo(scene, ids.reshape(-1))
    with pytest.raises(ValueError):
        yk.write_output(tmp_path / "x.exr", film, albedo=albedo)  # albedo without denoise and guides
    with pytest.raises(ValueError):
        yk.write_preview(tmp_path / "x.png", film, albedo=albedo)
    with pytest.raises(ValueError):
        yk.write_output(tmp_path / "x.exr", film, denoise=yk.DenoiseParams(), albedo=albedo)  # ... without guides
    scene.close()


def test_python_layer(yk, tmp_path):
    """write_output / write_preview: the defaults leave the files as they were, albedo changes the denoised ones."""
    rng = np.random.default_rng(15)
    albedo = ref.make_albedo(rng, 37, 23)
    film = (rng.random((23, 37, 3), dtype=np.float32) * ref.divisor(albedo["a"])).astype(np.float32)
    guides = _flat_guides(37, 23)
    p = yk.DenoiseParams(iterations=2, sigma_plane=0.06)
    a, b, c, d = (tmp_path / n for n in ("a.exr", "b.exr", "c.exr", "d.exr"))
    yk.write_output(a, film, yk.ToneMapType.Raw)
    yk.write_output(b, film, yk.ToneMapType.Raw, albedo=None)
    yk.write_output(c, film, yk.ToneMapType.Raw, denoise=p, guides=guides)
    yk.write_output(d, film, yk.ToneMapType.Raw, denoise=p, guides=guides, albedo=albedo)
    assert a.read_bytes() == b.read_bytes() and len({a.read_bytes(), c.read_bytes(), d.read_bytes()}) == 3
    yk.write_preview(tmp_path / "c.png", film, denoise=p, guides=guides)
    yk.write_preview(tmp_path / "d.png", film, denoise=p, guides=guides, albedo=albedo)
    assert (tmp_path / "c.png").read_bytes() != (tmp_path / "d.png").read_bytes()


# ------------------------------------------------------------------ quality
def test_quality_on_oracle_films(yk, oracle):
    """textured-city at 96 x 54, Path depth 8, Uniform 4 spp against 1024 spp, 4 iterations at the library's default sigmas:
    the demodulated filter's error is at most 0.8 of the plain filter's.  Measured: noisy 0.0970, plain 0.0822, demodulated 0.0597,
    ratio 0.726 (on the textured pixels alone: noisy 0.0690, plain 0.0881 — worse than it went in — and 0.0502, ratio 0.570)."""
    q = ref.QUALITY
    sd = ref.textured_city()
    fs = yk.FilmSettings(res=q["res"], tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    osc = oracle.OracleScene(sd)
    integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, q["depth"], 0, 0.0)
    noisy = yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, q["noisy_spp"], 1, 1, SEED), integ, tiles, n_threads=0)[0], fs.res)
    conv = yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, q["converged_spp"], 1, 1, SEED ^ 0x1234567), integ, tiles, n_threads=0)[0], fs.res)
    guides, ids = oracle_view(oracle, osc, sd, cam, fs.res)
    assert same_bits(guides, oracle_guides(oracle, osc, cam, fs.res))
    scene = yk.Scene(None, sd)
    albedo = yk.surface_albedo(scene, ids)
    i = scene.info()
    diag = float(np.linalg.norm(np.array(i.bounds_max[:], np.float64) - np.array(i.bounds_min[:], np.float64)))
    p = yk.DenoiseParams(q["iterations"], q["sigma_color"], q["sigma_normal"], q["plane_fraction"] * diag)
    plain = yk.denoise(noisy, guides, p)
    demod = yk.denoise(noisy, guides, p, albedo=albedo)
    ground = len(sd.materials) - 2
    textured = (albedo["known"] == 1) & (ids["shape"] < sd.n_triangles) & (np.asarray(sd.tri_material)[np.minimum(ids["shape"], sd.n_triangles - 1)] == ground)
    assert textured.mean() > 0.2
    e_noisy, e_plain, e_demod = quality_error(noisy, conv), quality_error(plain, conv), quality_error(demod, conv)
    t_noisy, t_plain, t_demod = (ref.quality_error(x, conv, textured) for x in (noisy, plain, demod))
    print(f"quality: noisy {e_noisy:.4f} plain {e_plain:.4f} demodulated {e_demod:.4f} ratio {e_demod / e_plain:.3f}; "
          f"textured pixels: noisy {t_noisy:.4f} plain {t_plain:.4f} demodulated {t_demod:.4f} ratio {t_demod / t_plain:.3f}")
    assert e_demod <= q["bound"] * e_plain, (e_plain, e_demod)
    scene.close()
    osc.close()
