"""The staging boundaries of k_shade (yk_shade_queue.h) at the smallest sizes that reach them, bit for bit against the oracle.

A block of 256 threads stages up to 335 surviving paths and 768 shadow rays in LDS.  With up to three lights (256 x nl <= 768)
and one shadow queue the flush decisions are taken once per iteration; with more lights, or when the shadow rays are split
into an area and a delta queue, light by light, with a flush whenever the class of the light changes.  Up to four lights
share one verdict word per path, five or more have a byte each.

Integrator.li gives bounce 0 a queue of exactly n paths: one thread, one path short of a block, a block, one path into the
second iteration, the survivor staging (335) and one more, more than one block, and more blocks than a window.  yk_li
reports no ray count for the Path integrator (the wavefront keeps none per sample), so these cases compare the radiance;
the film renders compare the ray count too."""
import copy

import numpy as np
import pytest

from yuki_amd import abi, scenes

pytestmark = pytest.mark.gpu
SEED = 0x73B9642E74AC471C
RES = (64, 48)
SIZES = [1, 255, 256, 257, 335, 336, 769, 2049]
N_MAX = max(SIZES)
OFFSET = np.array([0.35, -0.4, 0.25], dtype=np.float32)  # a copied light is its source moved by a multiple of this


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _moved(light, k):
    m = copy.deepcopy(light)
    for key, sign in (("l2w", 1.0), ("l2w_inv", -1.0)):
        if key in m:
            m[key] = m[key].copy()
            m[key][:3, 3] += np.float32(sign * k) * OFFSET
    return m


def _with_lights(n_rect, n_point):
    """city-tiny (every material kind; one rectangular and two point lights) with n_rect rectangular lights followed by
    n_point point lights: its own, cut, or extended with moved copies (a copied rectangle has no triangles: it lights the
    scene and is not seen)."""
    sd = copy.copy(scenes.by_name("city-tiny"))
    rect = [l for l in sd.lights if l["kind"] == "rect"]
    point = [l for l in sd.lights if l["kind"] == "point"]
    assert len(rect) == 1 and len(point) == 2 and sd.lights[0]["kind"] == "rect"  # the area light keeps index 0: tri_area_light names it
    rect = rect + [_moved(rect[0], k) for k in range(1, n_rect)]
    point = (point + [_moved(point[0], k) for k in range(1, n_point)])[:n_point]
    sd.lights = rect[:n_rect] + point
    return sd


def _li_lights(nl):
    return _with_lights(1, nl - 1)


@pytest.fixture(scope="module")
def li_rays(yk, oracle):
    """N_MAX camera rays of a RES film, spread over the whole image (5 and 64 x 48 have no common factor), their pixels,
    and per light count the scene data and the oracle's radiance of every ray (computed once, read-only)."""
    sd = scenes.by_name("city-tiny")
    fs = yk.FilmSettings(res=RES, tile_dim=64)
    cam = yk.Camera(sd.camera, fs)
    sampler = yk.SamplerType.Stratified((1, 1), True, SEED)
    o, d = oracle.camera_rays(cam.matrices, sampler, (0, 0, RES[0], RES[1]), 0)
    pick = (np.arange(N_MAX) * 5) % (RES[0] * RES[1])
    assert len(np.unique(pick)) == N_MAX
    xy = np.stack([pick % RES[0], pick // RES[0]], axis=-1).astype(np.uint16)
    o, d = np.ascontiguousarray(o[pick]), np.ascontiguousarray(d[pick])
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=5))
    want = {}
    for nl in (1, 2, 3, 4, 5):
        sdl = _li_lights(nl)
        osc = oracle.OracleScene(sdl)
        li, _ = osc.li(sampler, integ, o, d, xy, np.zeros(N_MAX, dtype=np.uint32))
        osc.close()
        li.setflags(write=False)
        want[nl] = (sdl, li)
    return sampler, integ, o, d, xy, want


@pytest.fixture(scope="module", params=[0, 1], ids=["unsorted", "sorted"])
def reorder_ctx(yk, request):
    c = yk.Context(0, shade_reorder=request.param)
    yield c
    c.close()


@pytest.mark.parametrize("nl", [1, 2, 3, 4, 5])
def test_li_queue_lengths(yk, reorder_ctx, li_rays, nl):
    """Bounce 0's queue is exactly n paths long; depth 5.  nl <= 3: once-per-iteration decisions (3 fills the shadow staging
    exactly); 4: light by light with word verdicts; 5: light by light with byte verdicts."""
    sampler, integ, o, d, xy, want = li_rays
    sdl, li_want = want[nl]
    sc = yk.Scene(reorder_ctx, sdl)
    it = yk.IntegratorType.instantiate(reorder_ctx, integ)
    try:
        assert li_want.max() > 0
        for n in SIZES:
            got = it.li(sc, sampler, o[:n], d[:n], xy[:n], np.zeros(n, dtype=np.uint32), dimension=2)
            mism = int((_bits(got) != _bits(li_want[:n])).sum())
            assert mism == 0, f"n={n}, {nl} lights: {mism} of {got.size} channel values differ from the oracle bit pattern"
    finally:
        sc.close()


@pytest.mark.parametrize("n_rect,n_point", [(1, 2), (2, 3)])
def test_film_with_split_shadow_queues(yk, oracle, n_rect, n_point):
    """packet_shadow_bounces = 8: the shadow rays of every bounce are split into the area and the delta queue, and the
    staging is flushed when the class of the light changes — below (3) and above (5) four lights."""
    sd = _with_lights(n_rect, n_point)
    fs = yk.FilmSettings(res=RES, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    sampler = yk.SamplerType.Stratified((2, 2), True, SEED)
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=4))
    c = yk.Context(0, packet_shadow_bounces=8)
    try:
        sc = yk.Scene(c, sd)
        got, stats = yk.IntegratorType.instantiate(c, integ).render_tiles(sc, cam, sampler, tiles)
        sc.close()
    finally:
        c.close()
    osc = oracle.OracleScene(sd)
    want, rays = osc.render_tiles(cam.matrices, sampler, integ, tiles, n_threads=0)
    osc.close()
    assert stats.rays == rays
    assert want.max() > 0
    assert np.array_equal(_bits(got), _bits(want))


def test_guides_with_and_without_ids(ctx, yk):
    """One guide kernel, two instantiations: the guide records of yk_render_guides and yk_render_guides_ids compare byte for
    byte, as the latter's contract says.  The Cornell box: triangles, the sphere, and pixels that miss."""
    sd = scenes.by_name("cornell")
    fs = yk.FilmSettings(res=RES, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    sc = yk.Scene(ctx, sd)
    try:
        plain = yk.render_guides(ctx, sc, cam, fs)
        guides, ids = yk.render_guides_ids(ctx, sc, cam, fs)
    finally:
        sc.close()
    assert plain.tobytes() == guides.tobytes()
    assert plain["hit"].any() and not plain["hit"].all()  # hits and misses, both written by the plain instantiation
    assert np.array_equal(ids["shape"] == abi.SURFACE_NONE, plain["hit"] == 0)
