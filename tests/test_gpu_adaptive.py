"""Adaptive sampling on the MI355X (csrc/yk_adaptive.hip, the pixel-list route of csrc/yk_render.cpp): the device instance
of select / accumulate / resolve equals the host instance bit for bit on every case of the CPU suite, through host buffers
and on device pointers at offset addresses between guard words on a caller's stream; bad arguments are refused with nothing
launched; a pixel-list render equals the accumulating tile render — the oracle's and the device's own — entry by entry and
pass by pass; the fused fold equals render-then-accumulate; render_adaptive equals the same loop run with host instances over
oracle passes, continues where it stopped, and meets the quality conditions of the CPU suite; and the chain adaptive render
-> resolve -> variance-guided denoise -> tone map on one torch stream equals the host chain."""
import numpy as np
import pytest

import adaptive_ref as ref
from test_adaptive import QUALITY, SEED, adaptive_loop, fold_cases, params, quality_bound, same_bits, select_cases
from test_gpu_temporal import GUARD, _between_guards, _payload
from yuki_amd import abi, scenes

pytestmark = pytest.mark.gpu
F = np.float32


# ------------------------------------------------------------------ device equals host
def test_select_device_equals_host_host_buffers(ctx, yk):
    for name, stats, kw in select_cases():
        xy, sample = yk.adaptive_select(stats, params(yk, **kw), ctx=ctx)
        want_xy, want_sample = yk.adaptive_select(stats, params(yk, **kw))
        assert same_bits(xy, want_xy) and same_bits(sample, want_sample), name


def test_accumulate_and_resolve_device_equal_host_host_buffers(ctx, yk):
    for name, xy, passes, film, stats in fold_cases():
        got_f, got_s, want_f, want_s = film.copy(), stats.copy(), film.copy(), stats.copy()
        yk.adaptive_accumulate(xy, passes, got_f, got_s, ctx=ctx)
        yk.adaptive_accumulate(xy, passes, want_f, want_s)
        assert same_bits(got_f, want_f) and same_bits(got_s, want_s), name
        film2 = film.copy()
        film2[0, 0], film2[-1, -1] = ref.CANON, ref.INF
        for a, b in zip(yk.adaptive_resolve(film2, stats, ctx=ctx), yk.adaptive_resolve(film2, stats)):
            assert same_bits(a, b), name


def test_device_pointers_offsets_guard_words_and_a_callers_stream(ctx, yk):
    """select_device into a PixelList, accumulate_device and resolve_device on torch buffers at offset addresses (the film
    and the passes at 4 bytes, the statistics at 16) between guard words that stay intact, on a stream of the caller's."""
    import torch

    s = torch.cuda.Stream()
    cs = s.cuda_stream
    for name, stats, kw in select_cases():
        if not name.startswith(("5x3", "37x23", "130x70")) and name != "528x528-dilate1":
            continue
        h, w = stats.shape
        n = w * h
        d_stats = _between_guards(torch, 4 * n, 4, stats)
        pl = yk.PixelList(ctx, (w, h))
        torch.cuda.synchronize()
        count = ctx.adaptive_select_device(d_stats.data_ptr() + 16, (w, h), params(yk, **kw), pl, stream=cs)
        xy, sample = pl.read()
        want_xy, want_sample = yk.adaptive_select(stats, params(yk, **kw))
        assert count == len(want_xy) and same_bits(xy, want_xy) and same_bits(sample, want_sample), name
        assert np.array_equal(_payload(d_stats, 4, 4 * n), stats.view(np.uint32).reshape(-1)), name  # only read
        pl.close()
    for name, xy, passes, film, stats in fold_cases():
        h, w = stats.shape
        n = w * h
        pl = yk.PixelList(ctx, (w, h))
        pl.set(xy, np.zeros(len(xy), np.uint32), passes=3)
        d_film, d_stats, d_passes = _between_guards(torch, 3 * n, 1, film), _between_guards(torch, 4 * n, 8, stats), _between_guards(torch, passes.size, 3, passes)
        d_rgb, d_var = _between_guards(torch, 3 * n, 5), _between_guards(torch, n, 7)
        torch.cuda.synchronize()
        ctx.adaptive_accumulate_device(pl, d_passes.data_ptr() + 12, 3, (w, h), d_film.data_ptr() + 4, d_stats.data_ptr() + 32, stream=cs)
        ctx.adaptive_resolve_device(d_film.data_ptr() + 4, d_stats.data_ptr() + 32, (w, h), d_rgb.data_ptr() + 20, d_var.data_ptr() + 28, stream=cs)
        s.synchronize()
        want_f, want_s = film.copy(), stats.copy()
        yk.adaptive_accumulate(xy, passes, want_f, want_s)
        want_rgb, want_var = yk.adaptive_resolve(want_f, want_s)
        assert np.array_equal(_payload(d_film, 1, 3 * n), want_f.view(np.uint32).reshape(-1)), name
        assert np.array_equal(_payload(d_stats, 8, 4 * n), want_s.view(np.uint32).reshape(-1)), name
        assert np.array_equal(_payload(d_passes, 3, passes.size), passes.view(np.uint32).reshape(-1)), name  # only read
        assert np.array_equal(_payload(d_rgb, 5, 3 * n), want_rgb.view(np.uint32).reshape(-1)), name
        assert np.array_equal(_payload(d_var, 7, n), want_var.view(np.uint32).reshape(-1)), name
        only_var = _between_guards(torch, n, 2)
        ctx.adaptive_resolve_device(d_film.data_ptr() + 4, d_stats.data_ptr() + 32, (w, h), None, only_var.data_ptr() + 8, stream=cs)
        s.synchronize()
        assert np.array_equal(_payload(only_var, 2, n), want_var.view(np.uint32).reshape(-1)), name
        pl.close()


def test_bad_arguments_are_refused_with_nothing_launched(ctx, yk):
    import torch

    w, h = 8, 8
    n = w * h
    fill = lambda k, v: torch.full((k + 8,), v, dtype=torch.float32, device="cuda:0")  # noqa: E731
    film, passes, out = fill(3 * n, 3.0), fill(3 * 3 * n, 2.0), fill(3 * n, 5.0)
    stats = torch.full((4 * n + 8,), 7, dtype=torch.int32, device="cuda:0")
    var = torch.full((n + 8,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    Fm, P, O, S, V = (t.data_ptr() for t in (film, passes, out, stats, var))
    pl, other = yk.PixelList(ctx, (w, h)), yk.PixelList(ctx, (h + 1, w))
    all_xy = np.array([x | (y << 16) for y in range(h) for x in range(w)], dtype=np.uint32)
    pl.set(all_xy, np.zeros(n, np.uint32), passes=3)
    other.set(all_xy[:4], np.zeros(4, np.uint32), passes=3)
    p = params(yk)
    status = []

    def refused(call, *args, **kw):
        with pytest.raises(yk.YukiError) as e:
            call(*args, **kw)
        status.append(e.value.status)

    for st, lst in ((S + 4, pl), (S + 8, pl), (None, pl), (S, other)):
        refused(ctx.adaptive_select_device, st, (w, h), p, lst)
    refused(ctx.adaptive_select_device, S, (w, h), params(yk, min_samples=1), pl)
    assert pl.read()[0].tolist() == all_xy.tolist()  # a refused selection leaves the list as it was
    # accumulate: (list, passes, n_passes, film, stats)
    for lst, ps, k, f, st in ((pl, P + 2, 3, Fm, S), (pl, P, 3, Fm + 1, S), (pl, P, 3, Fm, S + 4), (pl, P, 3, Fm, S + 8), (pl, P, 0, Fm, S), (pl, P, 4, Fm, S), (other, P, 3, Fm, S), (pl, None, 3, Fm, S),
                              (pl, P, 3, None, S), (pl, P, 3, Fm, None), (pl, P, 3, Fm, Fm + 16), (pl, P, 3, P + 12, S), (pl, P, 3, Fm, P + 36 * n - 16)):  # fmt: skip
        refused(ctx.adaptive_accumulate_device, lst, ps, k, (w, h), f, st)
    # resolve: (film, stats, rgb, variance)
    for f, st, o, v in ((Fm + 2, S, O, V), (Fm, S + 8, O, V), (Fm, S, O + 1, V), (Fm, S, O, V + 2), (Fm, S, None, None), (None, S, O, V), (Fm, None, O, V), (Fm, S, Fm, V), (Fm, S, O, S + 16), (Fm, S, O, O + 4),
                        (Fm, S, O, Fm + 12 * n - 4)):  # fmt: skip
        refused(ctx.adaptive_resolve_device, f, st, (w, h), o, v)
    # host entries are checked before they are uploaded
    for xy, smp, k in (([w], [0], 1), ([h << 16], [0], 1), ([3, 3], [0, 0], 1), ([0], [(1 << 24) - 2], 3), ([0], [0], 0), ([0], [0], 0x10000)):
        refused(pl.set, np.array(xy, np.uint32), np.array(smp, np.uint32), passes=k)
    assert pl.read()[0].tolist() == all_xy.tolist()
    assert set(status) == {1}
    torch.cuda.synchronize()
    assert np.all(var.cpu().numpy() == GUARD) and np.all(stats.cpu().numpy() == 7)  # nothing was launched
    for t, val in ((film, 3.0), (passes, 2.0), (out, 5.0)):
        assert np.all(t.cpu().numpy() == val)
    pl.close()
    other.close()


# ------------------------------------------------------------------ a list render equals the accumulating render
RES = (48, 27)
LIST_SIZES = (1, 63, 64, 65, 257, 1296)


def _render_setup(yk, which, res=RES):
    if which == "cornell-whitted":
        sd, sampler, integ = scenes.cornell(), yk.SamplerType.Uniform(16, SEED), yk.IntegratorType.Whitted(3)
    else:
        sd = scenes.by_name("city-tiny")
        sampler = yk.SamplerType.Uniform(16, SEED) if which == "city-tiny-uniform" else yk.SamplerType.Stratified((4, 4), True, SEED)
        integ = yk.IntegratorType.Path(yk.PathParams(max_depth=8))
    fs = yk.FilmSettings(res=res, tile_dim=16)
    return sd, sampler, integ, yk.Camera(sd.camera, fs)


_reference = {}


def reference_passes(yk, oracle, ctx, which, res=RES):
    """(16, h * w, 3): pass s of the whole film, row-major — the oracle's render_tiles_accumulating over the film's tiles,
    which the device's own yk_render_tiles_accumulating must equal first.  Rendered once per setup and left unchanged."""
    if (which, res) not in _reference:
        sd, sampler, integ, cam = _render_setup(yk, which, res)
        tiles = yk.film_tiles(yk.FilmSettings(res=res, tile_dim=16))
        osc = oracle.OracleScene(sd)
        want = np.stack([osc.render_tiles_accumulating(cam.matrices, sampler, integ, tiles, np.full(len(tiles), s), n_threads=0)[0] for s in range(16)])
        sc = yk.Scene(ctx, sd)
        got, _ = yk.IntegratorType.instantiate(ctx, integ).render_tiles_accumulating(sc, cam, sampler, tiles, np.zeros(len(tiles)), n_passes=16)
        sc.close()
        assert same_bits(got, want), which
        want = np.stack([yk.update_tiles(tiles, w, res).reshape(-1, 3) for w in want])
        want.setflags(write=False)
        _reference[which, res] = want
    return _reference[which, res]


def _lists(rng, n_passes, res, sizes):
    """One (xy, sample) per list size: distinct pixels in a shuffled order, sample indices mixed over what 16 allow."""
    out = []
    for n in sizes:
        pix = rng.permutation(res[0] * res[1])[:n]
        xy = ((pix % res[0]) | ((pix // res[0]) << 16)).astype(np.uint32)
        out.append((xy, rng.integers(0, 16 - n_passes + 1, size=n).astype(np.uint32)))
    return out


def _check_list_renders(yk, c, sc, which, want, n_passes, seed, res=RES, sizes=LIST_SIZES):
    import torch

    sd, sampler, integ, cam = _render_setup(yk, which, res)
    it = yk.IntegratorType.instantiate(c, integ)
    pl = yk.PixelList(c, res)
    for xy, sample in _lists(np.random.default_rng(seed), n_passes, res, sizes):
        n = len(xy)
        pl.set(xy, sample, passes=n_passes)
        d_out = _between_guards(torch, n_passes * n * 3, 1)
        torch.cuda.synchronize()
        stats = it.render_pixel_list_device(sc, cam, sampler, pl, n_passes, d_out.data_ptr() + 4, want_stats=True)
        got = _payload(d_out, 1, n_passes * n * 3).view(F).reshape(n_passes, n, 3)
        pix = (xy >> 16).astype(np.int64) * res[0] + (xy & 0xFFFF)
        for k in range(n_passes):
            assert same_bits(got[k], want[sample + k, pix]), (which, n, k)
        assert stats.samples == n * n_passes
    pl.close()
    return stats


@pytest.mark.parametrize("which", ["city-tiny-uniform", "city-tiny-stratified", "cornell-whitted"])
def test_list_render_equals_the_accumulating_render(ctx, yk, oracle, which):
    want = reference_passes(yk, oracle, ctx, which)
    sc = yk.Scene(ctx, _render_setup(yk, which)[0])
    for n_passes in (1, 3):
        _check_list_renders(yk, ctx, sc, which, want, n_passes, 40 + n_passes)
    sc.close()


@pytest.mark.parametrize("option", [dict(batch_paths=64), dict(packet_bounces=0)], ids=["batch_paths-64", "packet_bounces-0"])
def test_list_render_under_other_plans(ctx, yk, oracle, option):
    """Many batches that alternate between both work sets; no packet kernel."""
    which = "city-tiny-uniform"
    want = reference_passes(yk, oracle, ctx, which)
    c = yk.Context(0, **option)
    sc = yk.Scene(c, _render_setup(yk, which)[0])
    stats = _check_list_renders(yk, c, sc, which, want, 3, 77)
    assert stats.batches == (-(-1296 * 3 // 64) if "batch_paths" in option else 1)
    sc.close()
    c.close()


def test_list_render_in_two_chunks(ctx, yk, oracle):
    """The smallest "sample_buf_cap" (1 MiB) holds 16384 pixels of 4 passes: at 192 x 108 a list of 16385 entries is cut into
    chunks of 16384 and 1, the whole film into 16384 and 4352."""
    which, res = "city-tiny-uniform", (192, 108)
    want = reference_passes(yk, oracle, ctx, which, res)
    c = yk.Context(0, sample_buf_cap=1 << 20)
    sc = yk.Scene(c, _render_setup(yk, which, res)[0])
    _check_list_renders(yk, c, sc, which, want, 4, 78, res, (16385, res[0] * res[1]))
    sc.close()
    c.close()


def test_list_beyond_the_sampler_is_refused_and_an_empty_list_launches_nothing(ctx, yk):
    import torch

    sd, sampler, integ, cam = _render_setup(yk, "city-tiny-stratified")
    sc = yk.Scene(ctx, sd)
    it = yk.IntegratorType.instantiate(ctx, integ)
    pl = yk.PixelList(ctx, RES)
    d_out = torch.full((3 * 4 * 3 + 8,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pl.set(np.array([5, 6, 7], np.uint32), np.array([0, 14, 3], np.uint32), passes=3)  # 14 + 3 = 17 > 16
    for n_passes in (3, 1):
        with pytest.raises(yk.YukiError, match="beyond the sampler's samples per pixel") as e:
            it.render_pixel_list_device(sc, cam, sampler, pl, n_passes, d_out.data_ptr())
        assert e.value.status == 1
    pl.set(np.array([5, 6, 7], np.uint32), np.array([0, 13, 3], np.uint32), passes=3)
    with pytest.raises(yk.YukiError, match="bad number of passes"):
        it.render_pixel_list_device(sc, cam, sampler, pl, 4, d_out.data_ptr())
    with pytest.raises(yk.YukiError):
        it.render_pixel_list_device(sc, cam, sampler, pl, 3, None)
    pl.set(np.zeros(0, np.uint32), np.zeros(0, np.uint32), passes=3)
    stats = it.render_pixel_list_device(sc, cam, sampler, pl, 3, d_out.data_ptr(), want_stats=True)
    assert stats.samples == 0 and stats.rays == 0 and stats.batches == 0
    torch.cuda.synchronize()
    assert np.all(d_out.cpu().numpy() == GUARD)
    pl.close()
    sc.close()


# ------------------------------------------------------------------ the fused route and the driver
ADAPT = dict(min_samples=4, round_passes=4, max_rounds=3)


def _adaptive_setup(yk, ctx, spp=32):
    sd = scenes.by_name("city-tiny")
    fs = yk.FilmSettings(res=RES, tile_dim=16)
    return sd, fs, yk.Camera(sd.camera, fs), yk.SamplerType.Uniform(spp, SEED), yk.IntegratorType.Path(yk.PathParams(max_depth=8))


def _host(film_sum, stats):
    return film_sum.cpu().numpy(), stats.cpu().numpy().view(abi.PIXEL_STATS_DTYPE).reshape(stats.shape[0], stats.shape[1])


def test_fused_route_equals_render_then_accumulate(ctx, yk):
    import torch

    sd, fs, cam, sampler, integ = _adaptive_setup(yk, ctx)
    sc = yk.Scene(ctx, sd)
    it = yk.IntegratorType.instantiate(ctx, integ)
    p = yk.AdaptiveParams.for_sampler(sampler, **ADAPT)
    p.max_rounds = 1
    w, h = RES
    f_film = f_stats = None
    film = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    stats = torch.zeros((h, w, 4), dtype=torch.int32, device="cuda:0")
    pl = yk.PixelList(ctx, RES)
    for rnd in range(3):  # cleared: every pixel; then two rounds of sparse lists
        f_film, f_stats, info = it.render_adaptive(sc, cam, sampler, fs, p, f_film, f_stats)
        n = ctx.adaptive_select_device(stats.data_ptr(), RES, p, pl)
        assert info.rounds == 1 and info.first_pixels == info.last_pixels == n and (rnd > 0 or n == w * h)
        slab = torch.zeros(p.round_passes * n * 3, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        it.render_pixel_list_device(sc, cam, sampler, pl, p.round_passes, slab.data_ptr())
        ctx.adaptive_accumulate_device(pl, slab.data_ptr(), p.round_passes, RES, film.data_ptr(), stats.data_ptr())
        torch.cuda.synchronize()
        for a, b in zip(_host(f_film, f_stats), _host(film, stats)):
            assert same_bits(a, b), rnd
    assert 0 < n < w * h  # the later rounds were sparse
    pl.close()
    sc.close()


def test_render_adaptive_equals_the_host_loop_over_oracle_passes(ctx, yk, oracle):
    """Uniform 32, min 4, round 4, three rounds: film sums, statistics and every round's list equal the loop of
    tests/test_adaptive.py run with host instances over the oracle's accumulating passes; a second call with a larger
    max_samples continues, and equals one longer run; info.samples is the sum of drawn."""
    sd, fs, cam, sampler, integ = _adaptive_setup(yk, ctx)
    w, h = RES
    film_tile = np.array([(0, 0, w, h)], dtype=abi.TILE_DTYPE)
    osc = oracle.OracleScene(sd)
    passes = np.stack([osc.render_tiles_accumulating(cam.matrices, sampler, integ, film_tile, [s], n_threads=0)[0] for s in range(32)])
    sc = yk.Scene(ctx, sd)
    it = yk.IntegratorType.instantiate(ctx, integ)
    p = yk.AdaptiveParams.for_sampler(sampler, **ADAPT)
    p.max_samples = 16
    host_lists = []
    want_f, want_s, rounds = adaptive_loop(yk, passes, RES, p, lists=host_lists)
    assert rounds == 3 and len(host_lists) == 4 and 0 < len(host_lists[2][0]) < w * h
    film, stats, info = it.render_adaptive(sc, cam, sampler, fs, p)
    got_f, got_s = _host(film, stats)
    assert same_bits(got_f, want_f) and same_bits(got_s, want_s)
    assert (info.rounds, info.converged, info.first_pixels, info.last_pixels) == (3, 0, w * h, len(host_lists[2][0]))
    assert info.samples == int(got_s["drawn"].sum()) and info.rays > info.samples
    # round by round: the device's lists are the host's
    one = yk.AdaptiveParams.for_sampler(sampler, **ADAPT)
    one.max_samples, one.max_rounds = 16, 1
    pl = yk.PixelList(ctx, RES)
    f2 = s2 = None
    for rnd in range(3):
        if rnd:
            assert ctx.adaptive_select_device(s2.data_ptr(), RES, one, pl) == len(host_lists[rnd][0])
            xy, sample = pl.read()
            assert same_bits(xy, host_lists[rnd][0]) and same_bits(sample, host_lists[rnd][1]), rnd
        f2, s2, _ = it.render_adaptive(sc, cam, sampler, fs, one, f2, s2)
    for a, b in zip(_host(f2, s2), (want_f, want_s)):
        assert same_bits(a, b)
    # a larger cap continues, and equals one longer run
    more = yk.AdaptiveParams.for_sampler(sampler, min_samples=4, round_passes=4)
    film, stats, info2 = it.render_adaptive(sc, cam, sampler, fs, more, film, stats)
    long_f, long_s, long_info = it.render_adaptive(sc, cam, sampler, fs, more)
    for a, b in zip(_host(film, stats), _host(long_f, long_s)):
        assert same_bits(a, b)
    host_f, host_s, host_rounds = adaptive_loop(yk, passes, RES, more)
    assert same_bits(_host(long_f, long_s)[0], host_f) and same_bits(_host(long_f, long_s)[1], host_s)
    assert info2.converged == 1 and long_info.converged == 1 and long_info.rounds == host_rounds and info.samples + info2.samples == long_info.samples == int(host_s["drawn"].sum())
    with pytest.raises(yk.YukiError):  # more than the sampler has
        it.render_adaptive(sc, cam, sampler, fs, yk.AdaptiveParams(max_samples=33, **ADAPT))
    pl.close()
    sc.close()


def test_quality_on_device_films(ctx, yk):
    """The conditions of tests/test_adaptive.py, with render_adaptive at the defaults against the device's own uniform passes."""
    from test_denoise import quality_error

    q = QUALITY
    sd = scenes.by_name(q["scene"])
    w, h = q["res"]
    fs = yk.FilmSettings(res=q["res"], tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    sc = yk.Scene(ctx, sd)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=q["depth"])))
    sampler = yk.SamplerType.Uniform(q["spp"], SEED)
    tiles = yk.film_tiles(fs)
    conv = yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(q["converged_spp"], SEED ^ 0x1234567), tiles)[0], fs.res)
    p = yk.AdaptiveParams.for_sampler(sampler)
    film, stats, info = it.render_adaptive(sc, cam, sampler, fs, p)
    film, stats = _host(film, stats)
    rgb, _ = yk.adaptive_resolve(film, stats, ctx=ctx)
    k = -(-int(info.samples) // (w * h))
    uniform, _ = it.render_tiles_accumulating(sc, cam, sampler, np.array([(0, 0, w, h)], dtype=abi.TILE_DTYPE), [0], n_passes=k)
    uniform = uniform.astype(np.float64).sum(0).reshape(h, w, 3) / k
    e_ad, e_un, bound = quality_error(rgb, conv), quality_error(uniform, conv), quality_bound()
    print(f"adaptive quality on the device: {info.rounds} rounds, mean spp {info.samples / (w * h):.1f}, adaptive {e_ad:.4f} uniform at {k} spp {e_un:.4f} ratio {e_ad / e_un:.3f} bound {bound}")
    assert info.converged == 1 and info.samples == int(stats["drawn"].sum()) and k < q["spp"]
    assert e_ad < e_un, (e_ad, e_un)
    assert bound < 1 and e_ad <= bound * e_un, (e_ad, e_un, bound)
    sc.close()


# ------------------------------------------------------------------ the chain
def test_the_chain_on_one_torch_stream(ctx, yk):
    """Guides, render_adaptive, resolve, the variance-guided denoise with the resolved variance, the tone map — handed to
    one torch stream, one synchronisation at the end.  Equals the host instances run on the device's film sums, statistics
    and guides, bit for bit."""
    import torch

    sd, fs, cam, sampler, integ = _adaptive_setup(yk, ctx)
    w, h = RES
    n = w * h
    sc = yk.Scene(ctx, sd)
    it = yk.IntegratorType.instantiate(ctx, integ)
    p = yk.AdaptiveParams.for_sampler(sampler, min_samples=4, round_passes=4, max_rounds=4)
    vpar = yk.VarianceParams.for_scene(sc, iterations=3)
    td = yk.film_tile_dim(fs)
    stream = torch.cuda.Stream()
    z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda:0")  # noqa: E731
    guides, rgb, var, clean = z(8 * n), z(3 * n), z(n), z(3 * n)
    film = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    stats = torch.zeros((h, w, 4), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    cs = stream.cuda_stream
    ctx.render_guides_device(sc, cam, RES, guides.data_ptr(), stream=cs)
    _, _, info = it.render_adaptive(sc, cam, sampler, fs, p, film, stats, stream=cs)
    ctx.adaptive_resolve_device(film.data_ptr(), stats.data_ptr(), RES, rgb.data_ptr(), var.data_ptr(), stream=cs)
    ctx.denoise_variance_device(rgb.data_ptr(), guides.data_ptr(), var.data_ptr(), RES, vpar, td, None, clean.data_ptr(), stream=cs)
    ctx.tone_map_device(clean.data_ptr(), RES, td, yk.ToneMapType.default(), None, clean.data_ptr(), stream=cs)
    stream.synchronize()
    assert info.rounds == 4 and 0 < info.last_pixels < n
    h_film, h_stats = _host(film, stats)
    hg = guides.cpu().numpy().view(abi.GUIDE_DTYPE).reshape(h, w)
    h_rgb, h_var = yk.adaptive_resolve(h_film, h_stats)
    assert same_bits(rgb.cpu().numpy(), h_rgb.reshape(-1)) and same_bits(var.cpu().numpy(), h_var.reshape(-1))
    assert np.isfinite(h_var).all() and h_var.max() > 0  # every pixel has its min_samples: the estimate is everywhere
    want = yk.tone_map(yk.denoise(h_rgb, hg, vpar, variance=h_var), yk.ToneMapType.default(), td)
    assert same_bits(clean.cpu().numpy(), want.reshape(-1))
    sc.close()
