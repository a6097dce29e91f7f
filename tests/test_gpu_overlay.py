"""The overlays on the MI355X (yk_overlay_draw with a context, yk_overlay_draw_device): the device instance equals the host
instance bit for bit — every film and primitive set of tests/test_overlay.py, both work splits of the box kernel, the
launch's block and grid-stride edges, a 4K film, 200,000 contending boxes — and whole flows on one torch stream."""
import faulthandler

import numpy as np
import pytest

import overlay_ref as ref
from yuki_amd import scenes

pytestmark = pytest.mark.gpu
SEED = 0x73B9642E74AC471C
M = ref.simple_matrix()
BOXES_PER_BLOCK, LINES_PER_BLOCK, MAX_BLOCKS = 16, 4, 2048  # yk_overlay.hip: OV_BOXES_PER_BLOCK, OV_BLOCK / 64, OV_MAX_BLOCKS


@pytest.fixture(autouse=True)
def _time_limit():
    """Each test's GPU work runs under its own limit: a hang ends the process instead of the session waiting on it."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _same(a, b):
    return np.array_equal(ref.bits(a), ref.bits(b))


def test_device_equals_host_on_every_film_and_set(ctx, yk):
    for h, w in ref.FILMS:
        rng = np.random.default_rng(300 + w)
        film = ref.random_film(rng, h, w)
        few = ref.random_lines(rng, 40)
        for name, lines in ref.line_sets(w, h, rng).items():
            assert _same(yk.draw_overlay(film, M, lines=lines, ctx=ctx), yk.draw_overlay(film, M, lines=lines)), (h, w, name)
        for name, boxes in ref.box_sets(rng).items():
            assert _same(yk.draw_overlay(film, M, boxes=boxes, ctx=ctx), yk.draw_overlay(film, M, boxes=boxes)), (h, w, name)
            assert _same(yk.draw_overlay(film, M, lines=few, boxes=boxes, ctx=ctx), yk.draw_overlay(film, M, lines=few, boxes=boxes)), (h, w, name, "both")


def test_both_box_work_splits_equal_host(ctx, yk):
    """Every edge drawn by its own lane (threshold above any edge), every edge by the whole wave (threshold 1), and the
    default: the same film."""
    rng = np.random.default_rng(11)
    film = ref.random_film(rng, 150, 200)
    boxes = np.concatenate([ref.random_boxes(rng, 500), ref.random_boxes(rng, 40, size=9.0)])
    want = yk.draw_overlay(film, M, boxes=boxes)
    try:
        for coop_min in (1, 7, 65536, 32):
            ctx.set_option("overlay_coop_min", coop_min)
            assert _same(yk.draw_overlay(film, M, boxes=boxes, ctx=ctx), want), coop_min
    finally:
        ctx.set_option("overlay_coop_min", 32)


def test_counts_at_the_launch_edges(ctx, yk):
    rng = np.random.default_rng(12)
    film = ref.random_film(rng, 40, 64)
    lines = ref.random_lines(rng, LINES_PER_BLOCK * MAX_BLOCKS + 1)
    for n in (1, 3, 4, 5, 63, 64, 65, 5000, LINES_PER_BLOCK * MAX_BLOCKS - 1, LINES_PER_BLOCK * MAX_BLOCKS, LINES_PER_BLOCK * MAX_BLOCKS + 1):
        assert _same(yk.draw_overlay(film, M, lines=lines[:n], ctx=ctx), yk.draw_overlay(film, M, lines=lines[:n])), n
    edge = BOXES_PER_BLOCK * MAX_BLOCKS
    boxes = ref.random_boxes(rng, 2 * edge + 1, size=0.3)
    for n in (3, 4, 5, 15, 16, 17, 63, 64, 65, edge - 1, edge, edge + 1, 2 * edge + 1):
        assert _same(yk.draw_overlay(film, M, boxes=boxes[:n], ctx=ctx), yk.draw_overlay(film, M, boxes=boxes[:n])), n


def test_4k_long_lines_and_a_film_filling_box(ctx, yk):
    """3840 x 2160: four corner-to-corner lines and one box whose edges run along the film's border and through its middle —
    a per-lane loop bound or a wave split that is wrong shows on segments thousands of pixels long."""
    w, h = 3840, 2160
    tw = lambda x, y, z=2.0: ref.to_world(x, y, z, w, h)  # noqa: E731
    lines = ref.make_lines([tw(0, 0), tw(w, 0), tw(0.5, 0.5), tw(0, h / 2)], [tw(w, h), tw(0, h), tw(w - 0.5, h - 0.5), tw(w, h / 2 + 1)])
    lo, hi = tw(0.25, h - 0.25), tw(w - 0.25, 0.25)  # the near face (z = 2) along the border, the far face (z = 3) at 2/3 of it
    boxes = np.array([[(lo[0], lo[1], 2.0), (hi[0], hi[1], 3.0)]], np.float32)
    film = np.zeros((h, w, 3), np.float32)
    want = yk.draw_overlay(film, M, lines=lines, boxes=boxes)
    got = yk.draw_overlay(film, M, lines=lines, boxes=boxes, ctx=ctx)
    assert _same(got, want)
    touched = ref.bits(want).any(axis=2)
    assert touched.sum() > 4 * 3000 and touched[:, :8].any() and touched[:, -8:].any() and touched[:8].any() and touched[-8:].any()


def test_200000_tiny_boxes_contend(ctx, yk):
    rng = np.random.default_rng(13)
    film = ref.random_film(rng, 150, 200)
    boxes = ref.random_boxes(rng, 200000, size=0.15)
    want = yk.draw_overlay(film, M, boxes=boxes)
    assert _same(yk.draw_overlay(film, M, boxes=boxes, ctx=ctx), want)
    assert (ref.bits(want) != ref.bits(film)).any(axis=2).mean() > 0.9  # nearly every pixel fought over


def _upload(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(-1).copy()).to("cuda:0")


def test_device_pointers_stream_in_place_offset_and_composition(ctx, yk):
    """yk_overlay_draw_device on torch buffers: on a torch stream, on the context's stream, at a 4-byte offset between
    guards, and two calls on one stream, the second over the first."""
    import torch

    rng = np.random.default_rng(14)
    s = torch.cuda.Stream()
    for h, w in ((23, 37), (150, 200)):
        film = ref.random_film(rng, h, w)
        lines, boxes = ref.random_lines(rng, 70), ref.random_boxes(rng, 33)
        lines2, boxes2 = ref.random_lines(rng, 9), ref.random_boxes(rng, 5, size=6.0)
        want = yk.draw_overlay(film, M, lines=lines, boxes=boxes)
        d_lines, d_boxes, d_lines2, d_boxes2 = _upload(torch, lines), _upload(torch, boxes), _upload(torch, lines2), _upload(torch, boxes2)
        d_film = _upload(torch, film)
        big = torch.full((film.size + 5,), 7.5, dtype=torch.float32, device="cuda:0")
        big[1:-4] = d_film
        d_two = d_film.clone()
        torch.cuda.synchronize()
        ctx.draw_overlay_device(d_film.data_ptr(), (w, h), M, d_lines.data_ptr(), len(lines), d_boxes.data_ptr(), len(boxes), stream=s.cuda_stream)
        s.synchronize()
        assert _same(d_film.cpu().numpy(), want.reshape(-1))
        ctx.draw_overlay_device(big.data_ptr() + 4, (w, h), M, d_lines.data_ptr(), len(lines), d_boxes.data_ptr(), len(boxes))  # the context's stream
        torch.cuda.synchronize()
        b = big.cpu().numpy()
        assert b[0] == 7.5 and (b[-4:] == 7.5).all()
        assert _same(b[1:-4], want.reshape(-1))
        # two calls on one stream, no synchronisation between them; boxes only, then lines only
        ctx.draw_overlay_device(d_two.data_ptr(), (w, h), M, None, 0, d_boxes.data_ptr(), len(boxes), stream=s.cuda_stream)
        ctx.draw_overlay_device(d_two.data_ptr(), (w, h), M, d_lines2.data_ptr(), len(lines2), d_boxes2.data_ptr(), len(boxes2), stream=s.cuda_stream)
        s.synchronize()
        first = yk.draw_overlay(film, M, boxes=boxes)
        second = yk.draw_overlay(first, M, lines=lines2, boxes=boxes2)
        assert _same(d_two.cpu().numpy(), second.reshape(-1))
        assert not _same(first, second)


def _debug_rays(yk, ctx, sc, sd, fs, cam, smp, integ, pixel):
    x, y = pixel
    o, d = yk.camera_rays(ctx, cam, smp, (x, y, x + 1, y + 1), 0)
    it = yk.IntegratorType.instantiate(ctx, integ)
    _, _, rays = it.li_debug(sc, smp, o, d, np.array([[x, y]], np.uint16), np.zeros(1, np.uint32))
    return rays[0]


def test_whole_flow_on_one_torch_stream(ctx, yk):
    """Render city-tiny into a device film, tone-map it, draw a debug sample's rays and BVH level 4 on top — everything
    enqueued on one torch stream, one synchronisation at the end.  Equals the host chain on the downloaded film."""
    import torch

    sd = scenes.by_name("city-tiny")
    fs = yk.FilmSettings(res=(100, 60), tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    smp = yk.SamplerType.Uniform(1, SEED)
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=5))
    it = yk.IntegratorType.instantiate(ctx, integ)
    sc = yk.Scene(ctx, sd)
    rays = _debug_rays(yk, ctx, sc, sd, fs, cam, smp, integ, (50, 40))
    assert len(rays) >= 2
    lines = yk.overlay_ray_lines(rays)
    boxes = sc.node_bounds(4)
    m = yk.overlay_world_to_clip(sd.camera, fs, sc.node_bounds(0)[0])
    tiles = yk.film_tiles(fs)
    tl = yk.TileList(ctx, tiles)
    td = yk.film_tile_dim(fs)
    stream = torch.cuda.Stream()
    slab = torch.zeros(tl.n_pixels * 3, dtype=torch.float32, device="cuda:0")
    film = torch.zeros(60 * 100 * 3, dtype=torch.float32, device="cuda:0")
    mapped = torch.zeros_like(film)
    shown = torch.zeros_like(film)
    d_lines, d_boxes = _upload(torch, lines), _upload(torch, boxes)
    torch.cuda.synchronize()
    it.render_tile_list_device(sc, cam, smp, tl, slab.data_ptr(), stream=stream.cuda_stream)
    tl.update_film_device(slab.data_ptr(), fs.res, film.data_ptr(), stream=stream.cuda_stream)
    ctx.tone_map_device(film.data_ptr(), fs.res, td, yk.ToneMapType.default(), None, mapped.data_ptr(), stream=stream.cuda_stream)
    with torch.cuda.stream(stream):
        shown.copy_(mapped)
    ctx.draw_overlay_device(shown.data_ptr(), fs.res, m, d_lines.data_ptr(), len(lines), None, 0, stream=stream.cuda_stream)
    ctx.draw_overlay_device(shown.data_ptr(), fs.res, m, None, 0, d_boxes.data_ptr(), len(boxes), stream=stream.cuda_stream)
    stream.synchronize()
    host_mapped = mapped.cpu().numpy().reshape(60, 100, 3)
    assert _same(host_mapped, yk.tone_map(film.cpu().numpy().reshape(60, 100, 3), yk.ToneMapType.default(), td))
    want = yk.draw_overlay(yk.draw_overlay(host_mapped, m, lines=lines), m, boxes=boxes)
    got = shown.cpu().numpy().reshape(60, 100, 3)
    assert _same(got, want)
    assert _same(want, yk.draw_visualizations(host_mapped, sc, sd.camera, fs, rays=rays, bvh_level=4))
    colours = {tuple(c) for c in got.reshape(-1, 3)}
    assert (1.0, 0.0, 0.0) in colours and (0.0, 1.0, 0.0) in colours  # both box colours
    ray_colours = {tuple(c) for c in lines["rgb"]} - {(1.0, 0.0, 0.0), (0.0, 1.0, 0.0)}
    assert ray_colours & colours  # at least one ray colour that no box has
    tl.close()
    sc.close()


def test_draw_visualizations_device_equals_host(ctx, yk):
    sd = scenes.by_name("city-tiny")
    fs = yk.FilmSettings(res=(200, 150), tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    smp = yk.SamplerType.Uniform(1, SEED)
    sc = yk.Scene(ctx, sd)
    rays = _debug_rays(yk, ctx, sc, sd, fs, cam, smp, yk.IntegratorType.Path(yk.PathParams(max_depth=4)), (100, 100))
    film = ref.random_film(np.random.default_rng(15), 150, 200)
    for level in (None, -1, 0, 3, 7):
        want = yk.draw_visualizations(film, sc, sd.camera, fs, rays=rays, bvh_level=level)
        assert _same(yk.draw_visualizations(film, sc, sd.camera, fs, rays=rays, bvh_level=level, ctx=ctx), want), level
        assert not _same(want, film)
    assert _same(yk.draw_visualizations(film, sc, sd.camera, fs), film)
    sc.close()
