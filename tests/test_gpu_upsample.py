"""The guided upsample on the device (yuki_amd/csrc/yk_upsample.hip): k_upsample against the host instance bit for bit — the
host instance is pinned against the independent restatement by tests/test_upsample.py — on device pointers between guard
words and on a stream of the caller's, its refusals with nothing launched, the whole low-resolution chain on one torch
stream, and the CPU suite's quality conditions on films the device rendered."""
import numpy as np
import pytest

import albedo_ref as aref
import upsample_ref as ref
from test_denoise import SEED
from test_gpu_temporal import GUARD, _between_guards, _payload
from test_temporal import same_bits
from test_upsample import CASES as HOST_CASES
from test_upsample import MEAN_S, check_quality, quality_ratios
from yuki_amd import abi

pytestmark = pytest.mark.gpu
F = np.float32
# (low res, s): full 74 x 46 is no multiple of the 32 x 8 block | b == 0 taps, one lane in a last block column | exactly two
# blocks wide | the widest LDS window | a small film | the smallest film at the largest s
CASES = (((37, 23), 2), ((33, 9), 3), ((32, 18), 2), ((37, 23), 1), ((5, 3), 4), ((1, 1), 8))
SIG = (0.3, 0.06)


def _device_inputs():
    """(name, s, sigmas, tile_dim, inputs): every CASE with and without albedo, one of them with a sample table."""
    rng = np.random.default_rng(20261021)
    out = []
    for (lw, lh), s in CASES:
        for with_albedo in (False, True):
            td = 16 if ((lw, lh), s, with_albedo) == ((37, 23), 2, True) else None
            out.append((f"{lw}x{lh}-s{s}{'-albedo' if with_albedo else ''}{'-samples' if td else ''}", s, SIG, td or 16, ref.make_case(rng, lw, lh, s, with_albedo, td)))
    return out


DEVICE_CASES = _device_inputs()


def _on_device(torch, ctx, yk, stream, s, sig, td, low, lg, g, la, a, samples):
    """yk_upsample_device on buffers at 16-byte offsets (the RGB film at a 4-byte one) between guard words -> (rgb words,
    weight words); the inputs are checked to be only read."""
    lh, lw = low.shape[:2]
    n_lo, n = lw * lh, s * s * lw * lh
    d_low, d_lg, d_g = _between_guards(torch, 3 * n_lo, 1, low), _between_guards(torch, 8 * n_lo, 4, lg), _between_guards(torch, 8 * n, 8, g)
    d_la = None if la is None else _between_guards(torch, 4 * n_lo, 12, la)
    d_a = None if a is None else _between_guards(torch, 4 * n, 4, a)
    d_out, d_w = _between_guards(torch, 3 * n, 3), _between_guards(torch, n, 5)
    torch.cuda.synchronize()
    ctx.upsample_device(d_low.data_ptr() + 4, d_lg.data_ptr() + 16, (lw, lh), d_g.data_ptr() + 32, yk.UpsampleParams(s, *sig), td, samples, d_out.data_ptr() + 12, stream=stream.cuda_stream,
                        low_albedo=None if la is None else d_la.data_ptr() + 48, albedo=None if a is None else d_a.data_ptr() + 16, d_out_weight_ptr=d_w.data_ptr() + 20)
    stream.synchronize()
    assert np.array_equal(_payload(d_low, 1, 3 * n_lo), low.view(np.uint32).reshape(-1)) and np.array_equal(_payload(d_lg, 4, 8 * n_lo), lg.view(np.uint32).reshape(-1))
    assert np.array_equal(_payload(d_g, 8, 8 * n), g.view(np.uint32).reshape(-1))
    if la is not None:
        assert np.array_equal(_payload(d_la, 12, 4 * n_lo), la.view(np.uint32).reshape(-1)) and np.array_equal(_payload(d_a, 4, 4 * n), a.view(np.uint32).reshape(-1))
    return _payload(d_out, 3, 3 * n), _payload(d_w, 5, n)


@pytest.mark.parametrize("case", DEVICE_CASES + [c for c in HOST_CASES if c[1] in (3, 8) or "37x23-s2-albedo-samples" == c[0]], ids=lambda c: c[0])
def test_device_equals_host(ctx, yk, case):
    """Both outputs, on device pointers at offsets between guard words, on a torch stream; then through the host-array entry
    point with a context, with and without the weight output."""
    import torch

    _, s, sig, td, (low, lg, g, la, a, samples) = case
    p = yk.UpsampleParams(s, *sig)
    want, want_w = yk.upsample(low, lg, g, p, tile_dim=td, samples=samples, low_albedo=la, albedo=a, return_weight=True)
    got, got_w = _on_device(torch, ctx, yk, torch.cuda.Stream(), s, sig, td, low, lg, g, la, a, samples)
    bad = got != want.view(np.uint32).reshape(-1)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4] // 3)
    assert np.array_equal(got_w, want_w.view(np.uint32).reshape(-1))
    staged, staged_w = yk.upsample(low, lg, g, p, tile_dim=td, samples=samples, low_albedo=la, albedo=a, return_weight=True, ctx=ctx)
    assert same_bits(staged, want) and same_bits(staged_w, want_w)
    assert same_bits(yk.upsample(low, lg, g, p, tile_dim=td, samples=samples, low_albedo=la, albedo=a, ctx=ctx), want)


def test_bad_arguments_are_refused_with_nothing_launched(ctx, yk):
    import torch

    lw, lh, s = 8, 4, 2
    n_lo, n = lw * lh, s * s * lw * lh
    ones = lambda k, v: torch.full((k + 8,), v, dtype=torch.float32, device="cuda:0")  # noqa: E731
    low, lg, la, g, a = ones(3 * n_lo, 1.0), ones(8 * n_lo, 2.0), ones(4 * n_lo, 3.0), ones(8 * n, 4.0), ones(4 * n, 5.0)
    out = torch.full((3 * n + 8,), GUARD, dtype=torch.int32, device="cuda:0")
    wt = torch.full((n + 8,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    L, LG, LA, G, A, O, W = (t.data_ptr() for t in (low, lg, la, g, a, out, wt))
    p = yk.UpsampleParams(s, 0.3, 0.06)

    def call(low=L, lg=LG, la=LA, g=G, a=A, o=O, w=W, res=(lw, lh), td=16, p=p):
        ctx.upsample_device(low, lg, res, g, p, td, None, o, low_albedo=la, albedo=a, d_out_weight_ptr=w)

    bad = [dict(low=None), dict(lg=None), dict(g=None), dict(o=None), dict(la=None), dict(a=None)]  # required pointers; one albedo without the other
    bad += [dict(res=(0, lh)), dict(res=(lw, 0)), dict(td=0), dict(res=(32768, 1)), dict(res=(1, 32768))]
    bad += [dict(p=yk.UpsampleParams(s, v, 0.06)) for v in (0.0, -1.0, float("nan"))] + [dict(p=yk.UpsampleParams(s, 0.3, v)) for v in (0.0, -1.0, float("nan"))]
    bad += [dict(low=L + off) for off in (1, 2, 3)] + [dict(o=O + off) for off in (1, 2, 3)] + [dict(w=W + off) for off in (1, 2, 3)]
    bad += [dict(lg=LG + off) for off in (4, 8, 12)] + [dict(la=LA + off) for off in (4, 8, 12)] + [dict(g=G + off) for off in (4, 8, 12)] + [dict(a=A + off) for off in (4, 8, 12)]
    bad += [dict(o=L), dict(o=LG), dict(o=LA + 16 * n_lo - 4), dict(o=G + 32 * n - 4), dict(o=A), dict(w=L), dict(w=LG + 16), dict(w=LA), dict(w=G), dict(w=A + 16 * n - 4)]
    bad += [dict(w=O), dict(w=O + 12 * n - 4), dict(o=W + 4 * n - 4)]
    for kw in bad:
        with pytest.raises(yk.YukiError) as e:
            call(**kw)
        assert e.value.status == 1, kw
    for bad_s in (0, 9):  # past the Python layer, which refuses them itself
        with pytest.raises(yk.YukiError) as e:
            d = abi.UpsampleDesc(bad_s, 0.3, 0.06)
            yk.check(yk.lib().yk_upsample_device(ctx.h, d, L, LG, LA, lw, lh, 16, None, G, A, O, W, None), ctx.h)
        assert e.value.status == 1
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == GUARD) and np.all(wt.cpu().numpy() == GUARD)  # nothing was launched
    for t, v in ((low, 1.0), (lg, 2.0), (la, 3.0), (g, 4.0), (a, 5.0)):
        assert np.all(t.cpu().numpy() == v)
    call()  # the same arguments, all good: it runs
    torch.cuda.synchronize()
    assert not np.any(out.cpu().numpy()[: 3 * n] == GUARD)


# ------------------------------------------------------------------ the chain
def test_the_chain_on_one_torch_stream(ctx, yk):
    """Four accumulating passes of textured-city into a 50 x 30 device film, its guides, the guides and ids of the 100 x 60
    film, the full albedo, the low mean albedo (s = 2), the demodulated denoiser on the low film under its sample table, the
    upsample, the tone map — everything enqueued on one torch stream, one synchronisation at the end.  Equals the host
    instances run on copies, bit for bit."""
    import torch

    sd = aref.textured_city()
    res, s = (100, 60), 2
    fs = yk.FilmSettings(res=res, tile_dim=16)
    lfs = yk.subsampled(fs, s)
    lfs.accumulate = True
    lres = lfs.res
    n, n_lo = res[0] * res[1], lres[0] * lres[1]
    cam, lcam = yk.Camera(sd.camera, fs), yk.Camera(sd.camera, lfs)
    smp = yk.SamplerType.Stratified((2, 2), True, SEED)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    sc = yk.Scene(ctx, sd)
    tiles = yk.film_tiles(lfs)
    lists = [yk.TileList(ctx, tiles, np.full(len(tiles), k, np.uint16)) for k in range(4)]
    samples = yk.film_samples(lfs, tiles, np.full(len(tiles), 4, np.uint32))
    td = yk.film_tile_dim(lfs)
    dp = yk.DenoiseParams.for_scene(sc, iterations=4)
    up = yk.UpsampleParams.for_scene(sc, s)
    stream = torch.cuda.Stream()
    z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda:0")  # noqa: E731
    slab, film, low_guides, guides, ids = z(lists[0].n_pixels * 3), z(3 * n_lo), z(8 * n_lo), z(8 * n), z(4 * n)
    albedo, low_albedo, clean, full, weight = z(4 * n), z(4 * n_lo), z(3 * n_lo), z(3 * n), z(n)
    torch.cuda.synchronize()
    cs = stream.cuda_stream
    for tl in lists:
        it.render_tile_list_device(sc, lcam, smp, tl, slab.data_ptr(), stream=cs)
        tl.update_film_device(slab.data_ptr(), lres, film.data_ptr(), stream=cs, accumulate=True)
    ctx.render_guides_device(sc, lcam, lres, low_guides.data_ptr(), stream=cs)
    ctx.render_guides_ids_device(sc, cam, res, guides.data_ptr(), ids.data_ptr(), stream=cs)
    ctx.surface_albedo_device(sc, ids.data_ptr(), res, albedo.data_ptr(), stream=cs)
    ctx.albedo_mean_device(sc, ids.data_ptr(), lres, s, low_albedo.data_ptr(), stream=cs)
    ctx.denoise_device(film.data_ptr(), low_guides.data_ptr(), lres, dp, td, samples, clean.data_ptr(), stream=cs, albedo=low_albedo.data_ptr())
    ctx.upsample_device(clean.data_ptr(), low_guides.data_ptr(), lres, guides.data_ptr(), up, td, None, full.data_ptr(), stream=cs, low_albedo=low_albedo.data_ptr(), albedo=albedo.data_ptr(),
                        d_out_weight_ptr=weight.data_ptr())
    ctx.tone_map_device(full.data_ptr(), res, td, yk.ToneMapType.default(), None, full.data_ptr(), stream=cs)
    stream.synchronize()
    host_film = film.cpu().numpy().reshape(lres[1], lres[0], 3)
    host_lg = low_guides.cpu().numpy().view(abi.GUIDE_DTYPE).reshape(lres[1], lres[0])
    host_g = guides.cpu().numpy().view(abi.GUIDE_DTYPE).reshape(res[1], res[0])
    host_ids = ids.cpu().numpy().view(abi.SURFACE_ID_DTYPE).reshape(res[1], res[0])
    assert np.abs(host_film).max() > 0 and (host_g["hit"] != 0).sum() > 0 and (host_lg["hit"] != 0).sum() > 0
    host_scene = yk.Scene(None, sd)
    host_albedo, host_low_albedo = yk.surface_albedo(host_scene, host_ids), yk.albedo_mean(host_scene, host_ids, s)
    host_scene.close()
    assert same_bits(albedo.cpu().numpy().view(abi.ALBEDO_DTYPE).reshape(res[1], res[0]), host_albedo)
    assert same_bits(low_albedo.cpu().numpy().view(abi.ALBEDO_DTYPE).reshape(lres[1], lres[0]), host_low_albedo)
    host_clean = yk.denoise(host_film, host_lg, dp, tile_dim=td, samples=samples, albedo=host_low_albedo)
    assert same_bits(clean.cpu().numpy().reshape(host_clean.shape), host_clean)
    host_full, host_w = yk.upsample(host_clean, host_lg, host_g, up, tile_dim=td, low_albedo=host_low_albedo, albedo=host_albedo, return_weight=True)
    assert same_bits(weight.cpu().numpy().reshape(host_w.shape), host_w) and (host_w > 0).mean() > 0.9
    assert not np.array_equal(host_full, yk.upsample(host_clean, host_lg, host_g, up, tile_dim=td))  # the albedo does something here
    host_mapped = yk.tone_map(host_full, yk.ToneMapType.default(), td)
    assert np.array_equal(ref.bits(full.cpu().numpy()), ref.bits(host_mapped).reshape(-1))
    for tl in lists:
        tl.close()
    sc.close()


# ------------------------------------------------------------------ quality
@pytest.fixture(scope="module")
def device_city_films(ctx, yk):
    """test_upsample.quality_inputs with the device as the renderer."""
    q, s = aref.QUALITY, ref.QUALITY["s"]
    sd = aref.textured_city()
    fs = yk.FilmSettings(res=q["res"], tile_dim=16)
    lfs, bfs = yk.subsampled(fs, s), yk.supersampled(fs, MEAN_S)
    cam, lcam = yk.Camera(sd.camera, fs), yk.Camera(sd.camera, lfs)
    tiles, ltiles = yk.film_tiles(fs), yk.film_tiles(lfs)
    sc = yk.Scene(ctx, sd)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=q["depth"])))
    low = yk.update_tiles(ltiles, it.render_tiles(sc, lcam, yk.SamplerType.Uniform(q["noisy_spp"], SEED), ltiles)[0], lfs.res)
    conv = yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(q["converged_spp"], SEED ^ 0x1234567), tiles)[0], fs.res)
    low_guides = yk.render_guides(ctx, sc, lcam, lfs)
    guides, ids = yk.render_guides_ids(ctx, sc, cam, fs)
    ids_big = yk.render_guides_ids(ctx, sc, yk.Camera(sd.camera, bfs), bfs)[1]
    yield sc, (low, conv, low_guides, guides, ids, ids_big)
    sc.close()


@pytest.mark.parametrize("route", ["centre", "mean"])
def test_quality_on_device_films(ctx, yk, oracle, device_city_films, route):
    """The conditions of tests/test_upsample.py::test_quality_on_oracle_films, with the same bounds, on films, guides, ids,
    albedo, denoise and upsample of the device."""
    sc, inputs = device_city_films
    whole, masked, share, fallback = quality_ratios(yk, oracle, sc, *inputs, ref.QUALITY["s"], aref.QUALITY, route, ctx=ctx)
    check_quality(whole, masked, share, fallback, route)
