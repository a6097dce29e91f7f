"""Work the path kernels leave out because no result reads it, against the oracle bit for bit:

  * the sampler draw of a light that ignores its sample (point, spot, distant) is skipped — sampler_skip_2d keeps the state,
    and the state after it feeds the next light and the BSDF sample, so the place of the rectangular light among the others
    matters: first, between and last, and light sets without one.  Path (k_shade), Whitted (k_whitted) and yk_li_debug
    (k_path_debug) each have the light loop;
  * a regression test of the benchmark's route (a prepared tile list, k_raygen followed by the packet kernel on the camera
    bounce) at a size where the last packet of 64 is partly empty, with the ray and shadow-ray counts, and the same frame with
    packet_bounces = 0.  A flavour of the packet kernel that generated its camera rays itself was measured and not kept
    (DESIGN.md §9): of this change the frame runs the light loop of k_shade and k_accumulate's skip, nothing else;
  * k_accumulate leaves the sample slot alone when a vertex adds +-0: a scene where nearly every vertex after the camera's
    is fully shadowed, and one where next to none is."""
import copy

import numpy as np
import pytest

from yuki_amd import abi, scenes

pytestmark = pytest.mark.gpu
SEED = 0x73B9642E74AC471C
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _translation(p):
    m = np.eye(4, dtype=F)
    m[:3, 3] = p
    inv = np.eye(4, dtype=F)
    inv[:3, 3] = [-F(v) for v in p]
    return m, inv


def _samplers(yk):
    return (yk.SamplerType.Stratified((2, 2), True, SEED), yk.SamplerType.Stratified((2, 2), False, SEED), yk.SamplerType.Uniform(4, SEED))


# ------------------------------------------------------------------ light sets
def _point(p, i):
    return dict(kind="point", l2w=_translation(p)[0], I=i)


def _light_set(name):
    """The Cornell box (triangles only) under `name`'s lights; the box's own rectangular light keeps its quad, at whatever
    index the set gives it."""
    s = scenes.cornell_triangles_only()
    rect = s.lights[0]
    p1 = _point((0.15, 0.45, -0.20), (0.30, 0.25, 0.20))
    p2 = _point((0.42, 0.30, -0.40), (0.15, 0.20, 0.30))
    l2w, inv = _translation((0.278, 0.50, -0.45))
    spot = dict(kind="spot", l2w=l2w, l2w_inv=inv, I=(0.5, 0.5, 0.4), total_width=70.0, falloff_start=30.0)  # looks along +z, at the camera's side of the floor
    distant = dict(kind="distant", w=(0.15, 0.25, 1.0), L=(0.6, 0.6, 0.7))  # comes in through the open front
    s.lights = {
        "points": [p1, p2],
        "point-spot-distant": [p1, spot, distant],
        "rect-first": [rect, p1, p2],
        "rect-between": [p1, rect, p2],
        "rect-last": [p1, p2, rect],
    }[name]
    kinds = [l["kind"] for l in s.lights]
    s.tri_area_light = np.where(s.tri_area_light >= 0, kinds.index("rect") if "rect" in kinds else -1, -1).astype(np.int32)
    s.background = (0.02, 0.03, 0.05)
    s.name = "cornell-" + name
    return s


LIGHT_SETS = ["points", "point-spot-distant", "rect-first", "rect-between", "rect-last"]


@pytest.fixture(scope="module", params=LIGHT_SETS)
def lit(request, ctx, yk, oracle):
    """One light set: the scene on the device and in the oracle, shared by the three integrator tests."""
    sd = _light_set(request.param)
    sc = yk.Scene(ctx, sd)
    osc = oracle.OracleScene(sd)
    yield sd, sc, osc
    sc.close()
    osc.close()


def _render(ctx, yk, sd, sc, osc, sampler, integ, res=(32, 32)):
    fs = yk.FilmSettings(res=res, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    got, stats = yk.IntegratorType.instantiate(ctx, integ).render_tiles(sc, cam, sampler, tiles)
    want, rays, ostats = osc.render_tiles(cam.matrices, sampler, integ, tiles, n_threads=0, want_stats=True)
    return got, stats, want, rays, ostats


def test_path_under_every_light_set(ctx, yk, lit):
    sd, sc, osc = lit
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=4))
    for sampler in _samplers(yk):
        got, stats, want, rays, ostats = _render(ctx, yk, sd, sc, osc, sampler, integ)
        assert stats.rays == rays and stats.shadow_rays == ostats.shadow_rays
        assert want.max() > 0 and np.isfinite(want).all()
        assert np.array_equal(_bits(got), _bits(want)), sd.name


def test_whitted_under_every_light_set(ctx, yk, lit):
    sd, sc, osc = lit
    integ = yk.IntegratorType.Whitted(3)
    for sampler in _samplers(yk):
        got, stats, want, rays, _ = _render(ctx, yk, sd, sc, osc, sampler, integ)
        assert stats.rays == rays
        assert want.max() > 0 and np.isfinite(want).all()
        assert np.array_equal(_bits(got), _bits(want)), sd.name


def test_li_debug_under_every_light_set(ctx, yk, lit):
    """yk_li_debug on 64 camera rays: k_path_debug takes vertex_light as k_shade does."""
    sd, sc, osc = lit
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=4))
    it = yk.IntegratorType.instantiate(ctx, integ)
    fs = yk.FilmSettings(res=(32, 32), tile_dim=32)
    cam = yk.Camera(sd.camera, fs)
    tile = (12, 14, 20, 22)
    xy = np.stack(np.meshgrid(np.arange(tile[0], tile[2]), np.arange(tile[1], tile[3]), indexing="xy"), axis=-1).reshape(-1, 2).astype(np.uint16)
    for sampler in _samplers(yk):
        k = 2
        o, d = yk.camera_rays(ctx, cam, sampler, tile, k)
        assert len(o) == 64
        si = np.full(len(o), k, dtype=np.uint32)
        li, counts, _ = it.li_debug(sc, sampler, o, d, xy, si)
        want, want_counts = osc.li(sampler, integ, o, d, xy, si)
        assert np.array_equal(_bits(li), _bits(want)), sd.name
        assert np.array_equal(counts, np.asarray(want_counts, dtype=np.uint32))
        assert np.array_equal(_bits(it.li(sc, sampler, o, d, xy, si)), _bits(want))


# ------------------------------------------------------------------ camera rays of the packet route
@pytest.mark.parametrize("strata", [(8, 8), (3, 3)])
def test_tile_list_frame_of_70_by_3(ctx, yk, oracle, strata):
    """70 x 3 pixels through a prepared tile list, the route of the benchmark's frame: k_raygen, then the packet kernel traces
    the camera bounce (the existing kernels: the packet flavour that made its own camera rays was not kept, so this is a
    regression test of the route under the changed light loop and accumulate).  8 x 8 strata fill 210 packets of 64 samples;
    3 x 3 leave the last of 30 partly empty (1890 samples, 34 in the last).  Film, rays and shadow rays against the oracle; the
    same frame with the per-lane kernel on the camera bounce is the same film."""
    import torch

    sd = scenes.by_name("city-small")
    fs = yk.FilmSettings(res=(70, 3), tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    sampler = yk.SamplerType.Stratified(strata, True, SEED)
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=4))
    osc = oracle.OracleScene(sd)
    want, rays, ostats = osc.render_tiles(cam.matrices, sampler, integ, tiles, n_threads=0, want_stats=True)
    osc.close()
    assert want.max() > 0
    films = []
    for c in (ctx, yk.Context(0, packet_bounces=0)):
        sc = yk.Scene(c, sd)
        tl = yk.TileList(c, tiles)
        out = torch.zeros(tl.n_pixels * 3, dtype=torch.float32, device="cuda:0")
        st = yk.IntegratorType.instantiate(c, integ).render_tile_list_device(sc, cam, sampler, tl, out.data_ptr(), want_stats=True)
        torch.cuda.synchronize()
        films.append(out.cpu().numpy().reshape(-1, 3))
        assert st.samples == 70 * 3 * strata[0] * strata[1]
        assert st.rays == rays and st.shadow_rays == ostats.shadow_rays
        tl.close()
        sc.close()
        if c is not ctx:
            c.close()
    assert np.array_equal(_bits(films[0]), _bits(want))
    assert np.array_equal(_bits(films[1]), _bits(films[0]))


# ------------------------------------------------------------------ vertices that add nothing
def _walls_only():
    """The Cornell box without the tall box: from a light in the middle of the room every wall point is seen."""
    s = scenes.cornell_triangles_only()
    keep = s.tri_mesh != s.tri_mesh.max()  # the tall box is the last mesh
    s.indices, s.tri_mesh, s.tri_material, s.tri_area_light = s.indices[keep], s.tri_mesh[keep], s.tri_material[keep], np.full(int(keep.sum()), -1, dtype=np.int32)
    return s


@pytest.mark.parametrize("where", ["behind-the-wall", "mid-room"])
def test_vertices_that_add_nothing(ctx, yk, oracle, where):
    """One point light.  Behind the back wall: every shadow ray of the room is blocked (or f is black), there is no emitter,
    so after the camera's vertex only the rays that leave through the open front add anything — k_accumulate skips the slot
    on nearly every lane, beside lanes that do not.  In the middle of the empty room: every wall point sees the light, and next
    to no vertex is skipped."""
    sd = _walls_only() if where == "mid-room" else copy.copy(scenes.cornell_triangles_only())
    sd.tri_area_light = np.full_like(sd.tri_area_light, -1)
    sd.lights = [_point((0.278, 0.273, -0.9) if where == "behind-the-wall" else (0.278, 0.273, -0.28), (0.4, 0.4, 0.4))]
    sd.background = (0.3, 0.35, 0.4)
    sc = yk.Scene(ctx, sd)
    osc = oracle.OracleScene(sd)
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=4))
    for sampler in (yk.SamplerType.Stratified((2, 2), True, SEED), yk.SamplerType.Uniform(4, SEED)):
        got, stats, want, rays, ostats = _render(ctx, yk, sd, sc, osc, sampler, integ)
        assert stats.rays == rays and stats.shadow_rays == ostats.shadow_rays
        assert want.max() > 0 and np.isfinite(want).all()
        assert np.array_equal(_bits(got), _bits(want)), where
    sc.close()
    osc.close()
