"""The temporal passes (yuki_amd/csrc/yk_temporal.h: reproject the previous view's history through both views' guides,
blend the current film into it) on the host: the library's host instance against an independent numpy float32
restatement (tests/temporal_ref.py) bit for bit, the exact properties of the rule, the argument errors, the Python layer,
and the quality condition on oracle-rendered films.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import temporal_ref as ref
from test_denoise import oracle_guides, quality_error
from yuki_amd import _ffi, abi, scenes

F = np.float32
SEED = 0x73B9642E74AC471C
TOL, COS_MIN, MAX_HISTORY = 0.05, 0.9, 32.0  # the matrix's parameters: plane_tolerance in the units of ref.plane_guides
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


def params(yk, tol=TOL, cos_min=COS_MIN, max_history=MAX_HISTORY):
    return yk.TemporalParams(plane_tolerance=tol, normal_cos_min=cos_min, max_history=max_history)


def camera(yk, cam, res):
    return yk.Camera(cam, yk.FilmSettings(res=res, tile_dim=16))


@functools.lru_cache(maxsize=None)
def reproject_cases():
    """(name, history, previous guides, previous camera, guides): every film size under every camera pair, on two planes
    seen from both cameras; the histories carry NaN, +-inf, -0, 1e30 and counts of 0, -3, NaN, +inf."""
    from yuki_amd import core as yk

    rng = np.random.default_rng(20261019)
    out = []
    for w, h in ref.SIZES:
        for name, (prev, cur) in ref.CAMERA_PAIRS.items():
            cp, cc = camera(yk, prev, (w, h)), camera(yk, cur, (w, h))
            out.append((f"{w}x{h}-{name}", ref.make_history(rng, w, h), ref.plane_guides(cp.matrices, w, h, rng), cp, ref.plane_guides(cc.matrices, w, h, rng)))
    return out


@functools.lru_cache(maxsize=None)
def blend_cases():
    """(name, film, tile_dim, samples, history): every film size with and without a sample table (tile_dim 16, and 7 on
    sizes that are no multiple of it; the tables hold zeros) and with and without a history."""
    rng = np.random.default_rng(20261020)
    out = []
    for w, h in ref.SIZES:
        film = ref.denoise_ref.make_film(rng, w, h)
        film.reshape(-1).view(np.uint32)[::11] = 0x7FA12345  # a signalling NaN with a payload: only copied without a table
        hist = ref.make_history(rng, w, h)
        for td in (None, 16, 7):
            samples = None if td is None else ref.make_samples(rng, w, h, td)
            if samples is not None and w * h > 1:
                samples[0] = 0
            for hs in (None, hist):
                out.append((f"{w}x{h}-td{td}-{'hist' if hs is not None else 'nohist'}", film, td or 16, samples, hs))
    return out


def blend_raw(yk, film, p, td, samples, history, want_history=True, want_rgb=True, ctx=None):
    """yk_history_blend with either output NULL: (rgb or None, history or None)."""
    h, w = film.shape[:2]
    d = p.as_struct()
    rgb = np.zeros_like(film) if want_rgb else None
    rec = np.zeros((h, w), abi.HISTORY_DTYPE) if want_history else None
    c = ctx.h if ctx else None
    yk.check(_ffi.lib().yk_history_blend(c, C.byref(d), vp(film), w, h, td, vp(samples), vp(history), vp(rec), vp(rgb)), c)
    return rgb, rec


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_record_layout():
    assert abi.HISTORY_DTYPE.itemsize == 16 and abi.HISTORY_DTYPE == ref.HISTORY_DTYPE
    assert [abi.HISTORY_DTYPE.fields[k][1] for k in ("rgb", "n")] == [0, 12]
    assert C.sizeof(abi.TemporalDesc) == 12


def test_reproject_host_equals_restatement(yk):
    taken = 0
    for name, hist, pg, pc, g in reproject_cases():
        got = yk.reproject_history(hist, pg, pc, g, params(yk))
        want = ref.reproject(hist, pg, pc.matrices, g, TOL, COS_MIN)
        assert got.shape == want.shape and got.dtype == abi.HISTORY_DTYPE
        assert same_bits(got, want), (name, np.argwhere(got.view(np.uint32).reshape(got.shape + (4,)) != want.view(np.uint32).reshape(got.shape + (4,)))[:4])
        frac = float((got["n"] > 0).mean())
        if name.endswith("about-face"):
            assert frac == 0.0, name
        if name in ("64x36-same", "64x36-translate", "64x36-dolly-in", "64x36-dolly-out", "64x36-rotate"):
            assert frac > 0.2, (name, frac)  # the matrix is not a matrix of zeros
            taken += 1
    assert taken == 5
    # the plane test switched off, the normal test at its loosest
    name, hist, pg, pc, g = reproject_cases()[ref.SIZES.index((37, 23)) * len(ref.CAMERA_PAIRS) + 1]
    got = yk.reproject_history(hist, pg, pc, g, params(yk, tol=ref.INF, cos_min=-1.0))
    assert same_bits(got, ref.reproject(hist, pg, pc.matrices, g, ref.INF, -1.0)), name


@pytest.fixture(scope="module")
def oracle_views(yk, oracle):
    """The oracle's guides of cornell and city-small at the scene's camera and at one moved sideways."""
    out = {}
    for name, res, shift in (("cornell", (37, 23), (0.03, 0.01, 0.0)), ("city-small", (64, 36), (0.4, 0.05, -0.3))):
        sd = scenes.by_name(name)
        osc = oracle.OracleScene(sd)
        a = dict(sd.camera)
        b = dict(a, position=tuple(np.add(a["position"], shift)), target=tuple(np.add(a["target"], shift)))
        ca, cb = camera(yk, a, res), camera(yk, b, res)
        out[name] = (ca, oracle_guides(oracle, osc, ca, res), cb, oracle_guides(oracle, osc, cb, res))
        osc.close()
    return out


@pytest.mark.parametrize("name", ["cornell", "city-small"])
def test_reproject_host_equals_restatement_on_oracle_guides(yk, oracle_views, name):
    ca, ga, cb, gb = oracle_views[name]
    h, w = ga.shape
    hist = ref.make_history(np.random.default_rng(3), w, h)
    tol = 0.01 * float(np.linalg.norm(ga["p"][ga["hit"] != 0].max(0) - ga["p"][ga["hit"] != 0].min(0)))
    for prev_cam, prev_g, cur_g in ((ca, ga, gb), (cb, gb, ga), (ca, ga, ga)):
        got = yk.reproject_history(hist, prev_g, prev_cam, cur_g, params(yk, tol=tol))
        assert same_bits(got, ref.reproject(hist, prev_g, prev_cam.matrices, cur_g, tol, COS_MIN)), name
        assert (got["n"] > 0).mean() > 0.3, name


def test_blend_host_equals_restatement(yk):
    p = params(yk)
    for name, film, td, samples, hist in blend_cases():
        want_rgb, want_rec = ref.blend(film, MAX_HISTORY, td, samples, hist)
        rgb, rec = yk.blend_history(film, p, tile_dim=td, samples=samples, history=hist)
        assert same_bits(rgb, want_rgb) and same_bits(rec, want_rec), name
        only_rgb, none = blend_raw(yk, film, p, td, samples, hist, want_history=False)
        assert none is None and same_bits(only_rgb, want_rgb), name
        none, only_rec = blend_raw(yk, film, p, td, samples, hist, want_rgb=False)
        assert none is None and same_bits(only_rec, want_rec), name


# ------------------------------------------------------------------ exact properties
def _case(name):
    return next(c for c in reproject_cases() if c[0] == name)


def test_no_previous_hits_no_history(yk):
    _, hist, pg, pc, g = _case("37x23-translate")
    assert not yk.reproject_history(hist, np.zeros_like(pg), pc, g, params(yk)).view(np.uint32).any()


def test_empty_history_stays_empty(yk):
    _, hist, pg, pc, g = _case("37x23-translate")
    empty = hist.copy()
    empty["n"] = 0.0
    assert not yk.reproject_history(empty, pg, pc, g, params(yk)).view(np.uint32).any()


def test_a_camera_turned_right_round_sees_nothing_of_before(yk):
    _, hist, pg, pc, g = _case("64x36-about-face")
    hist = hist.copy()
    hist["n"] = 8.0
    assert (g["hit"] != 0).any()
    assert not yk.reproject_history(hist, pg, pc, g, params(yk)).view(np.uint32).any()


def _clean_view(yk, w=64, h=36):
    cp, cc = camera(yk, ref.BASE, (w, h)), camera(yk, ref.CAMERA_PAIRS["translate"][1], (w, h))
    hist = np.zeros((h, w), abi.HISTORY_DTYPE)
    hist["rgb"] = np.random.default_rng(11).random((h, w, 3), dtype=np.float32)
    hist["n"] = 16.0
    return hist, ref.plane_guides(cp.matrices, w, h), cp, ref.plane_guides(cc.matrices, w, h)


def test_bad_pixels_do_not_spread(yk):
    hist, pg, pc, g = _clean_view(yk)
    hist["rgb"][17, 30] = np.nan
    hist["rgb"][12, 20, 1] = np.inf
    out = yk.reproject_history(hist, pg, pc, g, params(yk))
    assert np.isfinite(out["rgb"]).all() and np.isfinite(out["n"]).all() and (out["n"] >= 0).all()
    assert (out["n"] > 0).mean() > 0.5


def test_nothing_crosses_a_plane_gap(yk):
    hist, pg, pc, g = _clean_view(yk)
    assert (yk.reproject_history(hist, pg, pc, g, params(yk))["n"] > 0).mean() > 0.5
    far = pg.copy()
    far["p"][..., 1] += F(1e6 * TOL) * far["ns"][..., 1]  # the previous view's floor, 1e6 tolerances below the current one's
    far["p"][..., 2] += F(1e6 * TOL) * far["ns"][..., 2]
    assert not yk.reproject_history(hist, far, pc, g, params(yk)).view(np.uint32).any()


def test_normals_must_agree(yk):
    hist, pg, pc, g = _clean_view(yk)
    tilted = pg.copy()  # the previous view's normals lean 0.1 towards x: every dot product is about 0.995
    tilted["ns"][..., 0] += F(0.1)
    tilted["ns"] /= np.sqrt((tilted["ns"] * tilted["ns"]).sum(-1, keepdims=True)).astype(np.float32)
    tilted["ns"][pg["hit"] == 0] = 0.0
    assert (yk.reproject_history(hist, tilted, pc, g, params(yk, cos_min=0.99))["n"] > 0).mean() > 0.5
    assert not yk.reproject_history(hist, tilted, pc, g, params(yk, cos_min=1.0)).view(np.uint32).any()


def test_blend_without_history_or_table_returns_the_film(yk):
    film = blend_cases()[0 + 6 * 3][1]  # 37x23
    rgb, rec = yk.blend_history(film, params(yk))
    assert same_bits(rgb, film) and same_bits(rec["rgb"], film) and np.all(rec["n"] == 1.0)


def test_blend_with_no_samples_returns_the_clamped_history(yk):
    rng = np.random.default_rng(13)
    w, h = 37, 23
    film = rng.random((h, w, 3), dtype=np.float32)
    hist = np.zeros((h, w), abi.HISTORY_DTYPE)
    hist["rgb"] = rng.random((h, w, 3), dtype=np.float32)
    hist["n"] = rng.integers(1, 100, size=(h, w)).astype(np.float32)
    rgb, rec = yk.blend_history(film, params(yk), tile_dim=16, samples=np.zeros(6, np.uint32), history=hist)
    assert same_bits(rgb, hist["rgb"]) and same_bits(rec["rgb"], hist["rgb"])
    assert (hist["n"] > MAX_HISTORY).any() and np.array_equal(rec["n"], np.minimum(hist["n"], F(MAX_HISTORY)))


def test_blend_bounds_the_count(yk):
    for name, film, td, samples, hist in blend_cases():
        _, rec = yk.blend_history(film, params(yk), tile_dim=td, samples=samples, history=hist)
        m = np.ones(film.shape[:2], np.float32) if samples is None else ref.tonemap_ref.sample_counts(film.shape[0], film.shape[1], td, samples)
        assert np.all(rec["n"] <= F(MAX_HISTORY) + m), name


def test_zeros_stay_zeros(yk):
    film = np.zeros((23, 37, 3), np.float32)
    hist = np.zeros((23, 37), abi.HISTORY_DTYPE)
    rgb, rec = yk.blend_history(film, params(yk), history=hist)
    assert not rgb.view(np.uint32).any() and not rec["rgb"].view(np.uint32).any() and np.all(rec["n"] == 1.0)
    hist["n"] = 5.0
    rgb, rec = yk.blend_history(film, params(yk), history=hist)
    assert not rgb.view(np.uint32).any() and np.all(rec["n"] == 6.0)


def test_blend_in_place_equals_out_of_place(yk):
    L = _ffi.lib()
    p = params(yk)
    for name, film, td, samples, hist in blend_cases():
        if hist is None or not name.startswith(("37x23", "5x70")):
            continue
        want_rgb, want_rec = yk.blend_history(film, p, tile_dim=td, samples=samples, history=hist)
        f, r = film.copy(), hist.copy()
        d = p.as_struct()
        assert L.yk_history_blend(None, C.byref(d), vp(f), film.shape[1], film.shape[0], td, vp(samples), vp(r), vp(r), vp(f)) == 0
        assert same_bits(f, want_rgb) and same_bits(r, want_rec), name


def test_every_refusal(yk):
    L = _ffi.lib()
    w, h = 8, 6
    n = w * h
    cam = camera(yk, ref.BASE, (w, h)).matrices
    hist, out = np.zeros((h, w), abi.HISTORY_DTYPE), np.zeros((h, w), abi.HISTORY_DTYPE)
    pg, g = np.zeros((h, w), abi.GUIDE_DTYPE), np.zeros((h, w), abi.GUIDE_DTYPE)
    film, rgb = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
    good = (0.05, 0.9, 32.0)
    bad_descs = [(v, 0.9, 32.0) for v in (0.0, -1.0, float("nan"), -float("inf"))]
    bad_descs += [(0.05, v, 32.0) for v in (-1.5, 1.5, float("nan"), float("inf"))]
    bad_descs += [(0.05, 0.9, v) for v in (0.5, 0.0, -1.0, float("nan"))]
    ptr = lambda a: a if isinstance(a, (int, type(None))) else a.ctypes.data  # noqa: E731
    cv = lambda a: None if ptr(a) is None else C.c_void_p(ptr(a))  # noqa: E731

    def rep(desc=good, hi=hist, p=pg, c=cam, gg=g, rx=w, ry=h, o=out, null_desc=False):
        d = abi.TemporalDesc(*desc)
        return L.yk_history_reproject(None, None if null_desc else C.byref(d), cv(hi), cv(p), None if c is None else C.byref(c), cv(gg), rx, ry, cv(o))

    def bl(desc=good, f=film, rx=w, ry=h, td=16, hi=hist, o=out, r=rgb, null_desc=False):
        d = abi.TemporalDesc(*desc)
        return L.yk_history_blend(None, None if null_desc else C.byref(d), cv(f), rx, ry, td, None, cv(hi), cv(o), cv(r))

    assert rep() == 0 and bl() == 0
    assert rep(desc=(float("inf"), -1.0, 1.0)) == 0 and rep(desc=(0.05, 1.0, float("inf"))) == 0  # the ends of the ranges
    for d in bad_descs:
        assert rep(desc=d) == 1 and bl(desc=d) == 1, d
    assert rep(null_desc=True) == 1 and rep(hi=None) == 1 and rep(p=None) == 1 and rep(c=None) == 1 and rep(gg=None) == 1 and rep(o=None) == 1
    assert rep(rx=0) == 1 and rep(ry=0) == 1
    # a reproject output that overlaps any input: it starts in the input's last record / the input starts in its last record
    assert rep(o=hist) == 1 and rep(o=hist.ctypes.data + 16) == 1
    big = np.zeros(n * 32 + n * 16 + 16, np.uint8)
    base = (big.ctypes.data + 15) & ~15
    assert rep(p=base, o=base + n * 32 - 16) == 1 and rep(p=base, o=base + n * 32) == 0
    assert rep(gg=base, o=base + n * 32 - 16) == 1 and rep(gg=base + n * 16 - 16, o=base) == 1 and rep(gg=base + n * 16, o=base) == 0
    assert bl(null_desc=True) == 1 and bl(f=None) == 1 and bl(rx=0) == 1 and bl(ry=0) == 1 and bl(td=0) == 1
    assert bl(o=None, r=None) == 1 and bl(o=None) == 0 and bl(r=None) == 0 and bl(hi=None) == 0
    assert bl(o=hist, r=film) == 0  # in place: each output equal to its own counterpart
    assert bl(o=hist.ctypes.data + 16) == 1 and bl(r=film.ctypes.data + 12) == 1  # overlapping without being equal
    assert bl(o=film) == 1 and bl(r=hist) == 1  # the other one's input
    assert bl(o=base, r=base + n * 16 - 12) == 1 and bl(o=base, r=base + n * 16) == 0  # the two outputs
    with pytest.raises(_ffi.YukiError) as e:
        yk.blend_history(film, yk.TemporalParams(max_history=0.0))
    assert e.value.status == 1
    with pytest.raises(ValueError):
        yk.reproject_history(hist[:-1], pg, camera(yk, ref.BASE, (w, h)), g, params(yk))
    with pytest.raises(ValueError):
        yk.blend_history(film, params(yk), tile_dim=16, samples=np.zeros(5, np.uint32))
    with pytest.raises(TypeError):
        yk.blend_history(film, yk.DenoiseParams())


def test_python_layer(yk):
    p = yk.TemporalParams()
    assert (p.plane_tolerance, p.normal_cos_min, p.max_history) == (None, 0.9, 64.0)
    assert p.as_struct().plane_tolerance == float("inf")

    class FakeScene:
        def info(self):
            i = _ffi.SceneInfo()
            i.bounds_min[:] = (0.0, 0.0, 0.0)
            i.bounds_max[:] = (3.0, 4.0, 12.0)
            return i

    q = yk.TemporalParams.for_scene(FakeScene(), max_history=16.0)
    assert q.max_history == 16.0 and abs(q.plane_tolerance - 0.13) < 1e-12
    # a round trip: blend, stand still, reproject with the same camera, blend again: two films of weight 1 average
    hist0, pg, pc, g = _clean_view(yk)
    a = np.where(pg["hit"][..., None] != 0, F(0.25), F(0)).astype(np.float32) * np.ones(3, np.float32)
    b = np.where(pg["hit"][..., None] != 0, F(0.75), F(0)).astype(np.float32) * np.ones(3, np.float32)
    rgb0, rec0 = yk.blend_history(a, params(yk))
    carried = yk.reproject_history(rec0, pg, pc, pg, params(yk))
    hit = pg["hit"] != 0
    assert same_bits(carried[hit], rec0[hit]) and not carried[~hit].view(np.uint32).any()  # the same view: every hit keeps its record
    rgb1, rec1 = yk.blend_history(b, params(yk), history=carried)
    assert np.all(rgb1[hit] == F(0.5)) and np.all(rec1["n"][hit] == 2.0) and np.all(rec1["n"][~hit] == 1.0)
    assert rgb1.dtype == np.float32 and rec1.dtype == abi.HISTORY_DTYPE and rec1.shape == (36, 64)


# ------------------------------------------------------------------ quality
QUALITY = dict(scene="city-small", res=(64, 36), depth=8, history_spp=64, noisy_spp=4, converged_spp=1024, move=0.01, normal_cos_min=0.9, max_history=64.0, coverage=0.5, bound=0.666)  # bound: the midpoint of 1 and the ratio 0.332 the host instance measures on these films (coverage 0.980)


def quality_cameras(yk, sd, q, diag):
    """Camera A = the scene's own; B = A moved sideways (along forward x up) by q["move"] x the scene diagonal."""
    a = dict(sd.camera)
    fwd = np.subtract(a["target"], a["position"]).astype(np.float64)
    side = np.cross(fwd, np.array(a["up"], np.float64))
    side *= q["move"] * diag / np.linalg.norm(side)
    b = dict(a, position=tuple(np.add(a["position"], side)), target=tuple(np.add(a["target"], side)))
    return camera(yk, a, q["res"]), camera(yk, b, q["res"])


def quality_check(yk, q, tparams, history_film, guides_a, cam_a, guides_b, noisy, conv, ctx=None):
    """The condition both suites assert: coverage of B's hits, and the blended film's error against the 4-spp film's."""
    h, w = noisy.shape[:2]
    hist = np.zeros((h, w), abi.HISTORY_DTYPE)
    hist["rgb"] = history_film
    hist["n"] = float(q["history_spp"])
    carried = yk.reproject_history(hist, guides_a, cam_a, guides_b, tparams, ctx=ctx)
    hits = guides_b["hit"] != 0
    coverage = float((carried["n"][hits] > 0).mean())
    # the 4-spp film as the accumulating film it is: the sum of 4 passes under a table of 4s (x 4 and / 4 are exact)
    td = 16
    samples = np.full((-(-w // td)) * (-(-h // td)), q["noisy_spp"], np.uint32)
    blended, _ = yk.blend_history(noisy * F(q["noisy_spp"]), tparams, tile_dim=td, samples=samples, history=carried, ctx=ctx)
    e_noisy, e_blend = quality_error(noisy, conv), quality_error(blended, conv)
    print(f"temporal quality: coverage {coverage:.3f} noisy {e_noisy:.4f} blended {e_blend:.4f} ratio {e_blend / e_noisy:.3f}")
    assert hits.any() and coverage >= q["coverage"], coverage
    assert e_blend < e_noisy, (e_noisy, e_blend)  # the hard condition
    assert e_blend <= q["bound"] * e_noisy, (e_noisy, e_blend)


def test_quality_on_oracle_films(yk, oracle):
    q = QUALITY
    sd = scenes.by_name(q["scene"])
    fs = yk.FilmSettings(res=q["res"], tile_dim=16)
    host_scene = yk.Scene(None, sd)
    tparams = yk.TemporalParams.for_scene(host_scene, normal_cos_min=q["normal_cos_min"], max_history=q["max_history"])
    cam_a, cam_b = quality_cameras(yk, sd, q, tparams.plane_tolerance / 0.01)
    tiles = yk.film_tiles(fs)
    osc = oracle.OracleScene(sd)
    integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, q["depth"], 0, 0.0)

    def render(cam, spp, seed):
        return yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, spp, 1, 1, seed), integ, tiles, n_threads=0)[0], fs.res)

    history_film = render(cam_a, q["history_spp"], SEED ^ 0x777)
    noisy = render(cam_b, q["noisy_spp"], SEED)
    conv = render(cam_b, q["converged_spp"], SEED ^ 0x1234567)
    quality_check(yk, q, tparams, history_film, oracle_guides(oracle, osc, cam_a, fs.res), cam_a, oracle_guides(oracle, osc, cam_b, fs.res), noisy, conv)
