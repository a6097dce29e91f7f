"""The motion passes (yuki_amd/csrc/yk_motion.h: a surface id and the previous vertex array give the previous position of a
pixel's surface point; yk_temporal.h: the reprojection that takes it) on the host: the library's host instance against an
independent numpy float32 restatement (tests/motion_ref.py) bit for bit, the exact properties of the rule, the argument
errors, the Python layer, and the quality conditions on oracle-rendered films of geometry that moved.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import motion_ref as ref
import temporal_ref
from test_denoise import quality_error
from test_scene_update import moved_scene, wobble
from test_temporal import COS_MIN, QUALITY, SEED, TOL, camera, params, reproject_cases, same_bits
from yuki_amd import _ffi, abi, scenes

F = np.float32
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


def test_record_layout():
    assert abi.SURFACE_ID_DTYPE.itemsize == 16 and abi.SURFACE_ID_DTYPE == ref.SURFACE_ID_DTYPE
    assert [abi.SURFACE_ID_DTYPE.fields[k][1] for k in ("shape", "b")] == [0, 4]
    assert abi.MOTION_DTYPE.itemsize == 16 and abi.MOTION_DTYPE == ref.MOTION_DTYPE
    assert [abi.MOTION_DTYPE.fields[k][1] for k in ("p_prev", "known")] == [0, 12]
    assert abi.SURFACE_NONE == ref.SURFACE_NONE == 0xFFFFFFFF


# ------------------------------------------------------------------ yk_surface_motion
def oracle_view(oracle, osc, sd, cam, res):
    """(guides, ids) of the oracle's first hits through the pixel centres: the shapes are OracleScene.intersect's, the
    barycentrics solved from its p."""
    o, d = oracle.camera_rays(cam.matrices, abi.SamplerDesc(abi.SAMPLER_STRATIFIED, 1, 1, 0, 0), (0, 0, res[0], res[1]), 0)
    r = osc.intersect(o, d)
    hit = r["shape"] >= 0
    g = np.zeros(res[0] * res[1], ref.GUIDE_DTYPE)
    g["hit"] = hit.astype(np.float32)
    g["ns"] = np.where(hit[:, None], r["ns"], F(0))
    g["p"] = np.where(hit[:, None], r["p"], F(0))
    g["t"] = np.where(hit, r["t"], F(0))
    ids = ref.solved_ids(r["shape"], r["p"], hit, sd.points, sd.indices, sd.n_triangles)
    return g.reshape(res[1], res[0]), ids.reshape(res[1], res[0])


@pytest.fixture(scope="module")
def scene_views(yk, oracle):
    """name -> (scene data, host-only scene, the oracle's guides and ids at the scene's camera on every film size)."""
    out = {}
    for name in ref.SCENES:
        sd = scenes.by_name(name)
        osc = oracle.OracleScene(sd)
        views = {res: oracle_view(oracle, osc, sd, camera(yk, sd.camera, res), res) for res in temporal_ref.SIZES}
        osc.close()
        out[name] = (sd, yk.Scene(None, sd), views)
    yield out
    for _, s, _ in out.values():
        s.close()


def motion_cases(sd, views, out_of_range=True):
    """(name, ids, guides, previous points): the oracle's ids on every film size under the scene's own and under wobbled
    points, and synthetic ids of every kind under points that hold NaN, +-inf and 1e30."""
    rng = np.random.default_rng(20261021)
    own = np.ascontiguousarray(sd.points, dtype=np.float32)
    for (w, h), (g, ids) in views.items():
        yield f"{w}x{h}-own", ids, g, own
        yield f"{w}x{h}-wobbled", ids, g, wobble(sd, 0.02)
        sids, sg = ref.synthetic_ids(rng, w, h, sd.n_triangles, len(sd.spheres), out_of_range)
        yield f"{w}x{h}-synthetic", sids, sg, ref.rough_points(rng, own)


@pytest.mark.parametrize("name", list(ref.SCENES))
def test_motion_host_equals_restatement(yk, scene_views, name):
    sd, scene, views = scene_views[name]
    nt, ns = sd.n_triangles, len(sd.spheres)
    kinds = np.zeros(4, np.int64)
    for case, ids, g, prev in motion_cases(sd, views):
        got = yk.surface_motion(scene, ids, g, prev)
        want = ref.surface_motion(ids, g, sd.indices, prev, nt, ns)
        assert got.shape == want.shape and got.dtype == abi.MOTION_DTYPE
        assert same_bits(got, want), (name, case, np.argwhere(got.view(np.uint32).reshape(got.shape + (4,)) != want.view(np.uint32).reshape(got.shape + (4,)))[:4])
        assert np.isin(got["known"], (0.0, 1.0)).all() and not got["p_prev"][got["known"] == 0].view(np.uint32).any(), case
        if case.endswith("own"):  # the solved barycentrics give the oracle's p back to rounding
            tri = (got["known"] == 1) & (ids["shape"] < nt)
            if tri.any():
                scale = np.abs(np.asarray(sd.points)).max()
                assert np.abs(got["p_prev"][tri].astype(np.float64) - g["p"][tri]).max() <= 1e-5 * scale, case
            sph = (got["known"] == 1) & (ids["shape"] >= nt)
            assert same_bits(got["p_prev"][sph], g["p"][sph]), case
        if case.endswith("synthetic"):
            live = (ids["shape"] != ref.SURFACE_NONE) & (g["hit"] != 0)
            kinds += [int((~live).sum()), int((live & (ids["shape"] >= nt + ns)).sum()), int((live & (ids["shape"] >= nt) & (ids["shape"] < nt + ns)).sum()), int((live & (ids["shape"] < nt)).sum())]
    assert kinds[0] > 0 and kinds[1] > 0 and kinds[3] > 0 and (kinds[2] > 0) == (ns > 0), kinds  # every case of the rule was met


def test_out_of_range_shapes_are_never_followed(yk, scene_views):
    """Shapes n_shapes, n_shapes + 1 and 0xfffffffe with hits under them: zero records, whatever the barycentrics."""
    sd, scene, _ = scene_views["cornell"]
    n = sd.n_triangles + len(sd.spheres)
    ids = np.zeros((3, 4), abi.SURFACE_ID_DTYPE)
    ids["shape"] = np.array([n, n + 1, 0xFFFFFFFE, 0x80000000], np.uint32)[None, :]
    ids["b"] = F(1.0 / 3.0)
    g = np.zeros((3, 4), abi.GUIDE_DTYPE)
    g["hit"], g["p"] = 1.0, 7.0
    assert not yk.surface_motion(scene, ids, g, np.ascontiguousarray(sd.points, np.float32)).view(np.uint32).any()


# ------------------------------------------------------------------ yk_history_reproject_moved
def moved_variants(g):
    """name -> the motion records of one case: the current positions themselves, the same with known = 0 on a checkerboard,
    and positions shifted by a constant."""
    h, w = g.shape
    m = np.zeros((h, w), abi.MOTION_DTYPE)
    m["p_prev"], m["known"] = g["p"], g["hit"]
    board = m.copy()
    y, x = np.mgrid[0:h, 0:w]
    board["known"][(x + y) % 2 == 1] = 0.0
    shifted = m.copy()
    shifted["p_prev"] = (m["p_prev"] + np.array([0.11, 0.0, -0.07], np.float32)).astype(np.float32)
    return {"same": m, "checkerboard": board, "shifted": shifted}


def test_reproject_moved_host_equals_restatement(yk):
    taken = 0
    for name, hist, pg, pc, g in reproject_cases():
        plain = yk.reproject_history(hist, pg, pc, g, params(yk))
        for kind, m in moved_variants(g).items():
            got = yk.reproject_history_moved(hist, pg, pc, g, m, params(yk))
            want = ref.reproject_moved(hist, pg, pc.matrices, g, m, TOL, COS_MIN)
            assert got.shape == want.shape and got.dtype == abi.HISTORY_DTYPE
            assert same_bits(got, want), (name, kind)
            if kind == "same":
                assert same_bits(got, plain), name  # motion = (guides.p, hit): yk_history_reproject itself
            if kind == "checkerboard":
                assert not got[m["known"] == 0].view(np.uint32).any() and same_bits(got[m["known"] != 0], plain[m["known"] != 0]), name
            if kind == "shifted" and name in ("64x36-same", "64x36-translate", "64x36-dolly-out"):
                assert (got["n"] > 0).mean() > 0.1 and not same_bits(got, plain), name  # the shift slides along the floor: taps are taken, other ones
                taken += 1
    assert taken == 3


def _case(name):
    return next(c for c in reproject_cases() if c[0] == name)


def test_nothing_known_nothing_carried(yk):
    _, hist, pg, pc, g = _case("37x23-translate")
    m = moved_variants(g)["same"]
    m["known"] = 0.0
    assert not yk.reproject_history_moved(hist, pg, pc, g, m, params(yk)).view(np.uint32).any()


def test_a_nan_position_is_a_zero_record_and_touches_no_other(yk):
    _, hist, pg, pc, g = _case("64x36-translate")
    m = moved_variants(g)["same"]
    base = yk.reproject_history_moved(hist, pg, pc, g, m, params(yk))
    spots = [(y, x) for y, x in zip(*np.nonzero(base["n"] > 0))][:: max(1, int((base["n"] > 0).sum()) // 7)][:7]
    assert len(spots) >= 5
    bad = m.copy()
    for k, (y, x) in enumerate(spots):
        bad["p_prev"][y, x, k % 3] = np.nan
    got = yk.reproject_history_moved(hist, pg, pc, g, bad, params(yk))
    touched = np.zeros(g.shape, bool)
    for y, x in spots:
        touched[y, x] = True
    assert not got[touched].view(np.uint32).any() and same_bits(got[~touched], base[~touched])


def test_non_finite_previous_points_never_reach_the_history(yk, scene_views):
    """Motion from vertex arrays that hold NaN, +-inf and 1e30, carried through reproject-moved at every tolerance setting: no
    record of the result is non-finite."""
    sd, scene, views = scene_views["city-small"]
    g, ids = views[(64, 36)]
    cam = camera(yk, sd.camera, (64, 36))
    rng = np.random.default_rng(5)
    prev = ref.rough_points(rng, np.ascontiguousarray(sd.points, np.float32))
    m = yk.surface_motion(scene, ids, g, prev)
    assert (~np.isfinite(m["p_prev"])).any() and np.isfinite(m["p_prev"]).all(-1).mean() > 0.5
    hist = np.zeros(g.shape, abi.HISTORY_DTYPE)
    hist["rgb"] = rng.random(g.shape + (3,), dtype=np.float32)
    hist["n"] = 16.0
    for p in (params(yk, tol=1.0), params(yk, tol=temporal_ref.INF, cos_min=-1.0)):
        out = yk.reproject_history_moved(hist, g, cam, g, m, p)
        assert np.isfinite(out["rgb"]).all() and np.isfinite(out["n"]).all() and (out["n"] >= 0).all()
        assert (out["n"] > 0).mean() > 0.2


# ------------------------------------------------------------------ refusals
def test_every_refusal(yk, scene_views):
    L = _ffi.lib()
    sd, scene, _ = scene_views["cornell"]
    w, h = 8, 6
    n = w * h
    cam = camera(yk, temporal_ref.BASE, (w, h)).matrices
    ids, g, pg = np.zeros((h, w), abi.SURFACE_ID_DTYPE), np.zeros((h, w), abi.GUIDE_DTYPE), np.zeros((h, w), abi.GUIDE_DTYPE)
    m, hist, out = np.zeros((h, w), abi.MOTION_DTYPE), np.zeros((h, w), abi.HISTORY_DTYPE), np.zeros((h, w), abi.HISTORY_DTYPE)
    pts = np.ascontiguousarray(sd.points, np.float32)
    ptr = lambda a: a if isinstance(a, (int, type(None))) else a.ctypes.data  # noqa: E731
    cv = lambda a: None if ptr(a) is None else C.c_void_p(ptr(a))  # noqa: E731

    def mo(s=scene.h, i=ids, gg=g, p=pts, rx=w, ry=h, o=m):
        return L.yk_surface_motion(None, s, cv(i), cv(gg), cv(p), rx, ry, cv(o))

    def rep(desc=(0.05, 0.9, 32.0), hi=hist, p=pg, c=cam, gg=g, mm=m, rx=w, ry=h, o=out, null_desc=False):
        d = abi.TemporalDesc(*desc)
        return L.yk_history_reproject_moved(None, None if null_desc else C.byref(d), cv(hi), cv(p), None if c is None else C.byref(c), cv(gg), cv(mm), rx, ry, cv(o))

    assert mo() == 0 and rep() == 0
    assert mo(s=None) == 1 and mo(i=None) == 1 and mo(gg=None) == 1 and mo(p=None) == 1 and mo(o=None) == 1 and mo(rx=0) == 1 and mo(ry=0) == 1
    # a motion output that overlaps an input: it starts in the input's last record / the input starts in its last record
    assert mo(o=ids) == 1 and mo(o=ids.ctypes.data + 16 * n - 16) == 1 and mo(i=m.ctypes.data + 16 * n - 16) == 1
    big = np.zeros(n * 32 + n * 16 + 32, np.uint8)
    base = (big.ctypes.data + 15) & ~15
    assert mo(gg=base, o=base + n * 32 - 16) == 1 and mo(gg=base, o=base + n * 32) == 0 and mo(gg=base + n * 16, o=base) == 0 and mo(gg=base + n * 16 - 16, o=base) == 1
    own = np.zeros(pts.size + 4 * n + 8, np.float32)  # the previous points, then room for the records
    assert mo(p=own, o=own.ctypes.data + 12 * pts.shape[0] - 4) == 1 and mo(p=own, o=own.ctypes.data + 12 * pts.shape[0]) == 0
    assert rep(null_desc=True) == 1 and rep(hi=None) == 1 and rep(p=None) == 1 and rep(c=None) == 1 and rep(gg=None) == 1 and rep(mm=None) == 1 and rep(o=None) == 1
    assert rep(rx=0) == 1 and rep(ry=0) == 1
    for d in ((0.0, 0.9, 32.0), (float("nan"), 0.9, 32.0), (0.05, 1.5, 32.0), (0.05, 0.9, 0.5)):
        assert rep(desc=d) == 1, d
    assert rep(o=hist) == 1 and rep(o=m) == 1 and rep(o=m.ctypes.data + 16 * n - 16) == 1 and rep(mm=out.ctypes.data + 16 * n - 16) == 1
    assert rep(p=base, o=base + n * 32 - 16) == 1 and rep(gg=base, o=base + n * 32 - 16) == 1 and rep(mm=base, o=base + n * 16) == 0
    # the guide pass has no host instance: without a context it is refused whatever else it is given (with one: tests/test_gpu_motion.py)
    assert L.yk_render_guides_ids(None, scene.h, C.byref(cam), w, h, None, None) == 1
    assert L.yk_render_guides_ids_device(None, scene.h, C.byref(cam), w, h, None, None, None) == 1


# ------------------------------------------------------------------ the Python layer
def test_python_layer(yk, scene_views):
    sd, scene, views = scene_views["cornell"]
    g, ids = views[(37, 23)]
    pts = np.ascontiguousarray(sd.points, np.float32)
    m = yk.surface_motion(scene, ids, g, pts)
    assert m.dtype == abi.MOTION_DTYPE and m.shape == g.shape
    assert same_bits(m, yk.surface_motion(scene, ids.reshape(-1), g, pts.reshape(-1)))  # flat ids and flat points are taken
    with pytest.raises(ValueError):
        yk.surface_motion(scene, ids, g, pts[:-1])
    with pytest.raises(ValueError):
        yk.surface_motion(scene, ids, g, pts.astype(np.float64))
    with pytest.raises(ValueError):
        yk.surface_motion(scene, ids[:-1], g, pts)
    with pytest.raises(ValueError):
        yk.surface_motion(scene, ids, g.reshape(-1), pts)
    cam = camera(yk, sd.camera, (37, 23))
    hist = temporal_ref.make_history(np.random.default_rng(2), 37, 23)
    with pytest.raises(ValueError):
        yk.reproject_history_moved(hist, g, cam, g, m[:-1], params(yk))
    with pytest.raises(TypeError):
        yk.reproject_history_moved(hist, g, cam, g, m, yk.DenoiseParams())
    # the geometry stood still: carried through the motion records = carried plainly, to the rounding of the solved ids
    tol = 0.01 * float(np.linalg.norm(pts.max(0) - pts.min(0)))
    a = yk.reproject_history_moved(hist, g, cam, g, m, params(yk, tol=tol))
    b = yk.reproject_history(hist, g, cam, g, params(yk, tol=tol))
    assert a.dtype == abi.HISTORY_DTYPE and ((a["n"] > 0) == (b["n"] > 0)).mean() > 0.98 and (a["n"] > 0).mean() > 0.3


# ------------------------------------------------------------------ quality
# Geometry that moves under a camera that stands, on test_temporal.QUALITY's films.  Measured on oracle films with the
# host instance (coverage, blended / noisy, plain-reprojected blended / noisy):
#   slide  (every unlit vertex + 0.03 x diagonal sideways)   0.938  0.389  1.030   (plain coverage 0.162)
#   wobble (test_scene_update.wobble(sd, 0.01))              0.953  0.475  0.675   (plain coverage 0.821)
# and on device-rendered films with the device instances (tests/test_gpu_motion.py): slide 0.939  0.385  1.030, wobble
# 0.953  0.475  0.675.  The slide's bound 0.666 is test_temporal.QUALITY's, the still-geometry case's.
MOTIONS = {"slide": lambda sd, diag: ref.slid_points(sd, 0.03, diag), "wobble": lambda sd, diag: wobble(sd, 0.01)}


def motion_quality_check(yk, q, name, tparams, history_film, prev_guides, cam, guides, motion, noisy, conv, ctx=None):
    """The conditions both suites assert on one motion: coverage of the moved scene's hits, the blended film against the
    4-spp film, against what plain reprojection gives on the same films, and (slide) against the still-geometry bound."""
    h, w = noisy.shape[:2]
    hist = np.zeros((h, w), abi.HISTORY_DTYPE)
    hist["rgb"] = history_film
    hist["n"] = float(q["history_spp"])
    carried = yk.reproject_history_moved(hist, prev_guides, cam, guides, motion, tparams, ctx=ctx)
    plain = yk.reproject_history(hist, prev_guides, cam, guides, tparams, ctx=ctx)
    hits = guides["hit"] != 0
    coverage, plain_coverage = float((carried["n"][hits] > 0).mean()), float((plain["n"][hits] > 0).mean())
    td = 16
    samples = np.full((-(-w // td)) * (-(-h // td)), q["noisy_spp"], np.uint32)
    film = noisy * F(q["noisy_spp"])
    blended, _ = yk.blend_history(film, tparams, tile_dim=td, samples=samples, history=carried, ctx=ctx)
    plain_blended, _ = yk.blend_history(film, tparams, tile_dim=td, samples=samples, history=plain, ctx=ctx)
    e_noisy, e_blend, e_plain = quality_error(noisy, conv), quality_error(blended, conv), quality_error(plain_blended, conv)
    print(f"motion quality {name}: coverage {coverage:.3f} (plain {plain_coverage:.3f}) noisy {e_noisy:.4f} blended {e_blend:.4f} ratio {e_blend / e_noisy:.3f} plain ratio {e_plain / e_noisy:.3f}")
    assert hits.any() and coverage >= q["coverage"], coverage
    assert e_blend < e_noisy, (e_noisy, e_blend)
    assert e_blend < e_plain, (e_plain, e_blend)
    if name == "slide":
        assert e_blend <= q["bound"] * e_noisy, (e_noisy, e_blend)


@functools.lru_cache(maxsize=None)
def quality_setup():
    from yuki_amd import core as yk

    q = QUALITY
    sd = scenes.by_name(q["scene"])
    host_scene = yk.Scene(None, sd)
    tparams = yk.TemporalParams.for_scene(host_scene, normal_cos_min=q["normal_cos_min"], max_history=q["max_history"])
    host_scene.close()
    return q, sd, yk.FilmSettings(res=q["res"], tile_dim=16), tparams


@pytest.fixture(scope="module")
def oracle_history(yk, oracle):
    """The 64-spp film and the guides of the OLD geometry, rendered once for both motions."""
    q, sd, fs, _ = quality_setup()
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    osc = oracle.OracleScene(sd)
    integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, q["depth"], 0, 0.0)
    film = yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, q["history_spp"], 1, 1, SEED ^ 0x777), integ, tiles, n_threads=0)[0], fs.res)
    guides, _ = oracle_view(oracle, osc, sd, cam, fs.res)
    osc.close()
    return film, guides


@pytest.mark.parametrize("name", list(MOTIONS))
def test_quality_on_oracle_films(yk, oracle, oracle_history, name):
    q, sd, fs, tparams = quality_setup()
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    history_film, prev_guides = oracle_history
    old = np.ascontiguousarray(sd.points, np.float32)
    new = MOTIONS[name](sd, tparams.plane_tolerance / 0.01)
    moved = moved_scene(sd, new)
    osc = oracle.OracleScene(moved)
    integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, q["depth"], 0, 0.0)

    def render(spp, seed):
        return yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, spp, 1, 1, seed), integ, tiles, n_threads=0)[0], fs.res)

    noisy, conv = render(q["noisy_spp"], SEED), render(q["converged_spp"], SEED ^ 0x1234567)
    guides, ids = oracle_view(oracle, osc, moved, cam, fs.res)
    osc.close()
    scene = yk.Scene(None, sd)
    scene.update(new)  # the library's own sequence: update, then motion from the array the scene had before
    motion = yk.surface_motion(scene, ids, guides, old)
    scene.close()
    motion_quality_check(yk, q, name, tparams, history_film, prev_guides, cam, guides, motion, noisy, conv)
