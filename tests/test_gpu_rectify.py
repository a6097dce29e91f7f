"""History rectification on the MI355X (yk_history_rectify with a context and yk_history_rectify_device): the device
instance equals the host instance bit for bit on the whole matrix of the CPU suite; on device pointers at 16-byte offsets
between guard words, and in place; misaligned and overlapping buffers are refused with nothing launched; reproject,
rectify, blend and moments blend on one torch stream equal the host chain; and the lighting-change quality conditions hold
on films the device rendered."""
import numpy as np
import pytest

import rectify_ref as ref
from test_gpu_temporal import GUARD, _between_guards, _payload
from test_rectify import QUALITY, QUALITY_CASES, TABLE, matrix, quality_chains, quality_films, relit, report, rp, run, same_records
from test_temporal import params as tparams_of
from test_temporal import quality_cameras, reproject_cases, same_bits
from yuki_amd import abi, scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_rectified(yk):
    """The host instance on the whole matrix, computed once and left unchanged."""
    out = {}
    for case, radius, with_m in matrix():
        got = run(yk, case, radius, with_m)
        for a in got if with_m else (got,):
            a.setflags(write=False)
        out[(case[0], radius, with_m)] = got
    return out


def test_device_equals_host_host_buffers(ctx, yk, host_rectified):
    for case, radius, with_m in matrix():
        assert same_records(run(yk, case, radius, with_m, ctx=ctx), host_rectified[(case[0], radius, with_m)]), (case[0], radius, with_m)
    case = next(c for c in ref.cases() if c[0] == "37x23-td7")
    for gamma in (0.0, 0.25, float("inf")):
        assert same_records(run(yk, case, 2, True, gamma, ctx=ctx), run(yk, case, 2, True, gamma)), gamma


def test_a_film_without_histories_is_copied(ctx, yk):
    """No lane of any block has a history: the blocks return before they stage anything, and every record is copied."""
    name, film, td, samples, hist, mom = next(c for c in ref.cases() if c[0] == "64x36-tdNone")
    empty = hist.copy()
    empty["n"] = np.where(np.arange(empty.size).reshape(empty.shape) % 3 == 0, np.float32(np.nan), np.float32(-1.0))
    out, out_m = yk.rectify_history(empty, film, rp(yk), tile_dim=td, samples=samples, moments=mom, ctx=ctx)
    assert same_bits(out, empty) and same_bits(out_m, mom)


def test_device_pointers_offsets_guard_words_and_in_place(ctx, yk, host_rectified):
    """The _device call on torch buffers and a stream of the caller's: the film at a 4-byte offset, the records at 16-byte
    offsets, every buffer between guard words that stay intact; then in place."""
    import torch

    s = torch.cuda.Stream()
    for case, radius, with_m in matrix():
        name, film, td, samples, hist, mom = case
        if not name.startswith(("37x23", "33x9", "1x1", "64x36-td16")):
            continue
        h, w = film.shape[:2]
        n = w * h
        want = host_rectified[(name, radius, with_m)]
        want_h, want_m = want if with_m else (want, None)
        d_film, d_hist, d_mom = _between_guards(torch, 3 * n, 1, film), _between_guards(torch, 4 * n, 4, hist), _between_guards(torch, 4 * n, 8, mom)
        d_out, d_out_m = _between_guards(torch, 4 * n, 12), _between_guards(torch, 4 * n, 4)
        torch.cuda.synchronize()
        fp, hp, mp = d_film.data_ptr() + 4, d_hist.data_ptr() + 16, d_mom.data_ptr() + 32
        op, omp = d_out.data_ptr() + 48, d_out_m.data_ptr() + 16
        ctx.rectify_history_device(fp, (w, h), rp(yk, radius), td, samples, hp, op, stream=s.cuda_stream, moments=mp if with_m else None, out_moments=omp if with_m else None)
        s.synchronize()
        assert np.array_equal(_payload(d_out, 12, 4 * n), want_h.view(np.uint32).reshape(-1)), (name, radius, with_m)
        if with_m:
            assert np.array_equal(_payload(d_out_m, 4, 4 * n), want_m.view(np.uint32).reshape(-1)), (name, radius)
        else:
            assert np.all(d_out_m.cpu().numpy() == GUARD)
        # the inputs are only read
        assert np.array_equal(_payload(d_film, 1, 3 * n), film.view(np.uint32).reshape(-1))
        assert np.array_equal(_payload(d_hist, 4, 4 * n), hist.view(np.uint32).reshape(-1)) and np.array_equal(_payload(d_mom, 8, 4 * n), mom.view(np.uint32).reshape(-1))
        ctx.rectify_history_device(fp, (w, h), rp(yk, radius), td, samples, hp, hp, stream=s.cuda_stream, moments=mp if with_m else None, out_moments=mp if with_m else None)  # in place
        s.synchronize()
        assert np.array_equal(_payload(d_hist, 4, 4 * n), want_h.view(np.uint32).reshape(-1)), (name, radius, with_m)
        assert np.array_equal(_payload(d_mom, 8, 4 * n), (want_m if with_m else mom).view(np.uint32).reshape(-1)), (name, radius)


def test_misaligned_or_overlapping_buffers_are_refused(ctx, yk):
    import torch

    w, h = 8, 8
    n = w * h
    film = torch.ones(3 * n + 8, dtype=torch.float32, device="cuda:0")
    hist = torch.full((4 * n + 8,), 3.0, dtype=torch.float32, device="cuda:0")
    mom = torch.full((4 * n + 8,), 2.0, dtype=torch.float32, device="cuda:0")
    out = torch.full((4 * n + 8,), GUARD, dtype=torch.int32, device="cuda:0")
    out_m = torch.full((4 * n + 8,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    F, H, M, O, OM = (t.data_ptr() for t in (film, hist, mom, out, out_m))
    bad = [(F + off, H, M, O, OM) for off in (1, 2, 3)]
    bad += [(F, H + off, M, O, OM) for off in (4, 8, 12)] + [(F, H, M + off, O, OM) for off in (4, 8, 12)]
    bad += [(F, H, M, O + off, OM) for off in (1, 4, 8, 12)] + [(F, H, M, O, OM + off) for off in (1, 4, 8, 12)]
    bad += [(F, H, M, H + 16, OM), (F, H, M, O, M + 16), (F, H, M, M, OM), (F, H, M, O, H), (F, H, M, O, O), (F, H, M, O, O + 16 * n - 16), (F, H, M, F, OM), (F, H, M, O, F)]
    bad += [(F, H, M, O, None), (F, H, None, O, OM), (F, None, M, O, OM), (None, H, M, O, OM), (F, H, M, None, OM)]
    for f, hi, m, o, om in bad:
        with pytest.raises(yk.YukiError) as e:
            ctx.rectify_history_device(f, (w, h), rp(yk), 16, None, hi, o, moments=m, out_moments=om)
        assert e.value.status == 1
    for desc in ((0, 1.0), (4, 1.0), (2, float("nan")), (2, -0.5)):
        with pytest.raises(yk.YukiError) as e:
            ctx.rectify_history_device(F, (w, h), yk.RectifyParams(*desc), 16, None, H, O, moments=M, out_moments=OM)
        assert e.value.status == 1
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == GUARD) and np.all(out_m.cpu().numpy() == GUARD)  # nothing was launched
    assert np.all(film.cpu().numpy() == 1.0) and np.all(hist.cpu().numpy() == 3.0) and np.all(mom.cpu().numpy() == 2.0)


def test_the_chain_on_one_torch_stream(ctx, yk):
    """Reproject the history and the moments, rectify both in place, blend the history, blend the moments: five calls on
    one torch stream and one synchronisation, equal to the host chain bit for bit."""
    import torch

    stream = torch.cuda.Stream()
    cs = stream.cuda_stream
    tp = tparams_of(yk)
    rng = np.random.default_rng(7)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(-1).copy()).to("cuda:0")  # noqa: E731
    for name, hist, pg, pc, g in reproject_cases():
        if name not in ("37x23-translate", "64x36-dolly-in", "33x9-same"):
            continue
        h, w = g.shape
        n = w * h
        film = (ref.denoise_ref.make_film(rng, w, h) * np.float32(3)).astype(np.float32)
        samples = ref.temporal_ref.make_samples(rng, w, h, 16)
        mom = ref.make_moments(rng, w, h, hist)
        z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda:0")  # noqa: E731
        d_hist, d_mom, d_pg, d_g, d_film = up(hist), up(mom), up(pg), up(g), up(film)
        carried, carried_m, out_h, out_m, rgb = z(4 * n), z(4 * n), z(4 * n), z(4 * n), z(3 * n)
        torch.cuda.synchronize()
        ctx.reproject_history_device(d_hist.data_ptr(), d_pg.data_ptr(), pc, d_g.data_ptr(), (w, h), tp, carried.data_ptr(), stream=cs)
        ctx.reproject_history_device(d_mom.data_ptr(), d_pg.data_ptr(), pc, d_g.data_ptr(), (w, h), tp, carried_m.data_ptr(), stream=cs)
        ctx.rectify_history_device(d_film.data_ptr(), (w, h), rp(yk), 16, samples, carried.data_ptr(), carried.data_ptr(), stream=cs, moments=carried_m.data_ptr(), out_moments=carried_m.data_ptr())
        ctx.blend_history_device(d_film.data_ptr(), (w, h), tp, 16, samples, carried.data_ptr(), out_h.data_ptr(), rgb.data_ptr(), stream=cs)
        ctx.blend_moments_device(d_film.data_ptr(), (w, h), tp, 16, samples, carried_m.data_ptr(), out_m.data_ptr(), stream=cs)
        stream.synchronize()
        want_c = yk.reproject_history(hist, pg, pc, g, tp)
        want_cm = yk.reproject_history(mom.view(abi.HISTORY_DTYPE), pg, pc, g, tp).view(abi.MOMENTS_DTYPE)
        want_c, want_cm = yk.rectify_history(want_c, film, rp(yk), tile_dim=16, samples=samples, moments=want_cm)
        want_rgb, want_h = yk.blend_history(film, tp, tile_dim=16, samples=samples, history=want_c)
        want_m = yk.blend_moments(film, tp, tile_dim=16, samples=samples, moments=want_cm)
        rec = lambda t, dt: t.cpu().numpy().view(dt).reshape(h, w)  # noqa: E731
        assert same_bits(rec(carried, abi.HISTORY_DTYPE), want_c) and same_bits(rec(carried_m, abi.MOMENTS_DTYPE), want_cm), name
        assert same_bits(rec(out_h, abi.HISTORY_DTYPE), want_h) and same_bits(rec(out_m, abi.MOMENTS_DTYPE), want_m), name
        assert same_bits(rgb.cpu().numpy().reshape(h, w, 3), want_rgb), name


def test_quality_after_a_lighting_change_on_device_films(ctx, yk):
    """The cornell-lighting case of the CPU suite on films and guides the device rendered, every pass on the device: after 4
    frames the rectified chain beats both keeping the history and throwing it away."""
    q, name = QUALITY, "cornell-lighting"
    case = dict(QUALITY_CASES[name])
    sd = scenes.by_name(case["scene"])
    fs = yk.FilmSettings(res=case["res"], tile_dim=16)
    sc_before, sc_after = yk.Scene(ctx, sd), yk.Scene(ctx, relit(case["scene"]))
    tp = yk.TemporalParams.for_scene(sc_before, normal_cos_min=q["normal_cos_min"], max_history=q["max_history"])
    case["cams"] = quality_cameras(yk, sd, case, tp.plane_tolerance / 0.01)
    tiles = yk.film_tiles(fs)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=q["depth"])))

    def renderer(sc):
        return lambda cam, spp, seed: yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(spp, seed), tiles)[0], fs.res)

    films = quality_films(yk, case, renderer(sc_before), renderer(sc_after), lambda cam: yk.render_guides(ctx, sc_after, cam, fs))
    e = quality_chains(yk, tp, films, False, yk.RectifyParams(**TABLE), ctx=ctx)
    report(name + " (device)", e)
    i4 = q["frames"].index(4)
    assert e["rectified"][i4] < e["plain"][i4], e
    assert e["rectified"][i4] < e["restart"][i4], e
    sc_before.close()
    sc_after.close()
