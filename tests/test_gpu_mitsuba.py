"""Mitsuba files on the device: file -> yk_load_mitsuba -> yk_scene_create -> render, against the oracle's render of what
tests/mitsuba_ref.py read from the same file, bit for bit.  Every mesh of such a scene is mirrored (scale(-1, 1, 1) * transform,
scene/mitsuba/shape.rs:78-79), so Triangle::intersect flips the geometric normal and then faces it forward to the shading
normal (shapes/triangle.rs:187-224) on every hit — here at BASELINE size and on every traversal path."""
import copy

import numpy as np
import pytest

from yuki_amd import loaders

import mitsuba_files as mf

pytestmark = pytest.mark.gpu
SEED = 0x73B9642E74AC471C


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def mr(oracle):
    import mitsuba_ref

    return mitsuba_ref


# ----------------------------------------------------------------------------- cfg2 as a Mitsuba file
def test_cfg2_mitsuba_file_renders_like_the_oracle(tmp_path, mr, oracle, yk, ctx):
    """BASELINE configs[1]'s mesh (69,312 triangles in one mirrored PLY, `twosided` diffuse, the point light of Scene::ply as
    an emitter), Path 8, Uniform 16 spp, 1920 x 1080: the first 48 spiral tiles, ray counts included.  The faces are written
    with reversed winding (tests/mitsuba_files.py): with the generator's winding the mirrored mesh is inside out and, lit by a
    point light alone, renders black on both sides — equal, and empty."""
    from yuki_amd import scenes

    p, _, info = mf.write_scene_as_mitsuba(scenes.by_name("cfg2"), str(tmp_path), twosided=True, reverse_winding=True)
    assert info == dict(ply_files=1, shapes=1, lights=1)
    got_sd, cam_p, film = loaders.load_mitsuba(p)
    want_sd, _, _ = mr.load_mitsuba(p)
    assert got_sd.n_triangles == 69312 and got_sd.meshes == [(False, False, True)] and film.res == (1920, 1080)
    fs = yk.FilmSettings(res=film.res, tile_dim=film.tile_dim)
    cam = yk.Camera(cam_p, fs)
    tiles = yk.film_tiles(fs)[:48]
    sampler = yk.SamplerType.Uniform(16, SEED)
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=8))
    sc = yk.Scene(ctx, got_sd)
    got, stats = yk.IntegratorType.instantiate(ctx, integ).render_tiles(sc, cam, sampler, tiles)
    sc.close()
    want, rays = oracle.OracleScene(want_sd).render_tiles(cam.matrices, sampler, integ, tiles, n_threads=0)
    assert stats.rays == rays and np.array_equal(_bits(got), _bits(want)) and got.max() > 0.05


# ----------------------------------------------------------------------------- cfg3's city as a Mitsuba file
@pytest.fixture(scope="module")
def cfg3_mitsuba(tmp_path_factory, cfg3_scene, mr, oracle, yk):
    """The city written once (802 mirrored PLY files, matte and glass only, two point lights, a spot light under a rotating
    transform, constant background), loaded by both loaders, and rendered once by the oracle: the first 24 spiral tiles."""
    d = str(tmp_path_factory.mktemp("cfg3_mitsuba_gpu"))
    spot = dict(kind="spot", cutoff=50.0, beam=35.0, I=(500.0, 480.0, 450.0), transform='<rotate x="1" angle="80"/><rotate y="1" angle="30"/><translate value="-20 2.9 10"/>')
    p, _, info = mf.write_scene_as_mitsuba(cfg3_scene, d, extra_lights=[spot], reverse_winding=True)
    assert info == dict(ply_files=802, shapes=802, lights=3)
    got_sd, cam_p, film = loaders.load_mitsuba(p)
    want_sd, _, _ = mr.load_mitsuba(p)
    assert got_sd.n_triangles == 1024012 and all(m[2] for m in got_sd.meshes) and any(m[0] for m in got_sd.meshes)
    assert np.array_equal(got_sd.points, cfg3_scene.points) and np.array_equal(got_sd.indices, cfg3_scene.indices[:, [0, 2, 1]]) and film.res == (1920, 1080)
    fs = yk.FilmSettings(res=film.res, tile_dim=film.tile_dim)
    cam = yk.Camera(cam_p, fs)
    tiles = yk.film_tiles(fs)[:24]
    sampler = yk.SamplerType.Stratified((8, 8), True, SEED)
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=8))
    osc = oracle.OracleScene(want_sd)
    want, rays = osc.render_tiles(cam.matrices, sampler, integ, tiles, n_threads=0)
    osc.close()
    return dict(sd=got_sd, cam=cam, tiles=tiles, sampler=sampler, integ=integ, want=want, rays=rays)


@pytest.mark.parametrize("wide_bvh,packet_bounces", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_cfg3_mitsuba_file_renders_like_the_oracle(cfg3_mitsuba, yk, wide_bvh, packet_bounces):
    """Path 8, Stratified 8 x 8, 1920 x 1080, first 24 spiral tiles, on both node layouts and with the wave-packet kernels off
    and on for the first bounce: mirrored meshes have not met those paths at this size."""
    c = cfg3_mitsuba
    ctx = yk.Context(0, wide_bvh=wide_bvh, packet_bounces=packet_bounces)
    try:
        sc = yk.Scene(ctx, c["sd"])
        got, stats = yk.IntegratorType.instantiate(ctx, c["integ"]).render_tiles(sc, c["cam"], c["sampler"], c["tiles"])
        sc.close()
    finally:
        ctx.close()
    assert stats.rays == c["rays"] and np.array_equal(_bits(got), _bits(c["want"])) and got.mean() > 0.01


# ----------------------------------------------------------------------------- the hand-written scene
@pytest.fixture(scope="module")
def hand(tmp_path_factory, mr, yk):
    p = mf.write_hand_scene(str(tmp_path_factory.mktemp("hand")))
    got_sd, cam_p, film = loaders.load_mitsuba(p)
    want_sd, _, _ = mr.load_mitsuba(p)
    fs = yk.FilmSettings(res=film.res, tile_dim=film.tile_dim)
    return dict(sd=got_sd, want_sd=want_sd, cam=yk.Camera(cam_p, fs), tiles=yk.film_tiles(fs))


def test_handedness_is_live(hand, oracle, yk, ctx):
    """GeometryNormals and ShadingNormals equal the oracle's and differ from the render of the same description with every
    swaps_handedness cleared: a loader that forgets the mirror's flag cannot pass."""
    sampler = yk.SamplerType.Uniform(1, SEED)
    unflagged = copy.copy(hand["sd"])
    unflagged.meshes = [(n, uv, False) for n, uv, _ in hand["sd"].meshes]
    osc = oracle.OracleScene(hand["want_sd"])
    sc, sc_unflagged = yk.Scene(ctx, hand["sd"]), yk.Scene(ctx, unflagged)
    for integ in (yk.IntegratorType.GeometryNormals, yk.IntegratorType.ShadingNormals):
        it = yk.IntegratorType.instantiate(ctx, integ)
        got, stats = it.render_tiles(sc, hand["cam"], sampler, hand["tiles"])
        want, rays = osc.render_tiles(hand["cam"].matrices, sampler, integ, hand["tiles"], n_threads=0)
        assert stats.rays == rays and np.array_equal(_bits(got), _bits(want))
        other, _ = it.render_tiles(sc_unflagged, hand["cam"], sampler, hand["tiles"])
        assert np.mean(np.any(_bits(got) != _bits(other), axis=-1)) > 0.2  # the meshes cover a good part of the frame
    sc.close()
    sc_unflagged.close()
    osc.close()


@pytest.mark.parametrize("depth", [1, 5])
def test_whitted_on_the_hand_written_scene(hand, oracle, yk, ctx, depth):
    """Glass (two dielectrics) and a spot light behind a mirroring light_to_world."""
    sampler = yk.SamplerType.Stratified((2, 2), True, SEED)
    integ = yk.IntegratorType.Whitted(depth)
    sc = yk.Scene(ctx, hand["sd"])
    got, stats = yk.IntegratorType.instantiate(ctx, integ).render_tiles(sc, hand["cam"], sampler, hand["tiles"])
    sc.close()
    osc = oracle.OracleScene(hand["want_sd"])
    want, rays = osc.render_tiles(hand["cam"].matrices, sampler, integ, hand["tiles"], n_threads=0)
    osc.close()
    assert stats.rays == rays and np.array_equal(_bits(got), _bits(want)) and got.mean() > 0.01


def test_li_debug_on_the_hand_written_scene(hand, oracle, yk, ctx):
    """yk_li_debug equals yk_li and the oracle's li on the camera rays of the whole 96 x 64 frame, segment counts included."""
    sampler = yk.SamplerType.Uniform(2, SEED)
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=6))
    tile = (0, 0, 96, 64)
    xy = np.stack(np.meshgrid(np.arange(96), np.arange(64), indexing="xy"), axis=-1).reshape(-1, 2).astype(np.uint16)
    o, d = yk.camera_rays(ctx, hand["cam"], sampler, tile, 1)
    si = np.full(len(o), 1, dtype=np.uint32)
    sc = yk.Scene(ctx, hand["sd"])
    it = yk.IntegratorType.instantiate(ctx, integ)
    li, counts, _ = it.li_debug(sc, sampler, o, d, xy, si)
    li2 = it.li(sc, sampler, o, d, xy, si)
    sc.close()
    osc = oracle.OracleScene(hand["want_sd"])
    want, want_counts = osc.li(sampler, integ, o, d, xy, si)
    osc.close()
    assert np.array_equal(_bits(li), _bits(li2)) and np.array_equal(_bits(li), _bits(want))
    assert np.array_equal(counts, np.asarray(want_counts, dtype=np.uint32)) and li.mean() > 0.01
