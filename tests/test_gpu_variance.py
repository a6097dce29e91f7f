"""The variance-guided denoise on the MI355X (yk_moments_blend, yk_variance and yk_denoise_variance with a context, and their
_device forms): the device instances equal the host instances bit for bit on every case of the CPU suite under
"denoise_lds_max_step" 0, 1 and 2, on device pointers at offset addresses between guard words and a stream of the caller's,
out of place and in place; misaligned and overlapping buffers are refused with nothing launched; the whole chain
(accumulate, guides, reproject, blend, moments blend, variance, filter, tone map, present) on one torch stream equals the
host chain; and the quality conditions hold on films the device rendered.

Films: 37 x 23 and 5 x 3 put every halo across a film edge, 130 x 70 at iteration 4 (step 16) reaches across blocks on both
axes, and the 130 x 70 moments whose frames are >= 2 everywhere but in one 8 x 8 patch take k_variance's block-uniform
window decision both ways."""
import ctypes as C

import numpy as np
import pytest

import temporal_ref
import variance_ref as ref
from test_denoise import SEED, quality_error
from test_gpu_temporal import GUARD, _between_guards, _payload
from test_variance import BLEND_CASES, FILTER_CASES, PIC, QUALITY, VARIANCE_CASES, moments_words, same_bits, tparams, vparams
from yuki_amd import abi

pytestmark = pytest.mark.gpu
F = np.float32
DEFAULT_LDS_MAX_STEP = 2  # the context's "denoise_lds_max_step" 


def _filter_args(yk, case):
    _, size, it, sig, alb, td, sk = case
    p = PIC[size]
    return p, vparams(yk, it, sig), (p["albedo"] if alb else None), td, (None if sk is None else p[sk])


def _variance_args(yk, case):
    _, size, mk, alb, td, sk, (sn, sp) = case
    p = PIC[size]
    return p, vparams(yk, sig=(4.0, sn, sp)), (None if mk is None else p[mk]), (p["albedo"] if alb else None), td, (None if sk is None else p[sk])


@pytest.fixture(scope="module")
def host_results(yk):
    """The host instance on every case, computed once and left unchanged."""
    out = {}
    for case in BLEND_CASES:
        _, size, td, sk, hist = case
        p = PIC[size]
        out["blend", case[0]] = yk.blend_moments(p["film"], tparams(yk), tile_dim=td, samples=None if sk is None else p[sk], moments=p["moments"] if hist else None)
    for case in VARIANCE_CASES:
        p, vpar, moments, albedo, td, samples = _variance_args(yk, case)
        out["variance", case[0]] = yk.variance(moments, p["film"], p["guides"], vpar, tile_dim=td, samples=samples, albedo=albedo)
    for case in FILTER_CASES:
        p, vpar, albedo, td, samples = _filter_args(yk, case)
        out["filter", case[0]] = yk.denoise(p["film"], p["guides"], vpar, tile_dim=td, samples=samples, albedo=albedo, variance=p["variance"])
    for v in out.values():
        v.setflags(write=False)
    return out


# ------------------------------------------------------------------ device equals host, through host buffers
def test_moments_blend_device_equals_host(ctx, yk, host_results):
    for case in BLEND_CASES:
        _, size, td, sk, hist = case
        p = PIC[size]
        got = yk.blend_moments(p["film"], tparams(yk), tile_dim=td, samples=None if sk is None else p[sk], moments=p["moments"] if hist else None, ctx=ctx)
        same_bits(moments_words(got), moments_words(host_results["blend", case[0]]))


def test_variance_device_equals_host(ctx, yk, host_results):
    for case in VARIANCE_CASES:
        p, vpar, moments, albedo, td, samples = _variance_args(yk, case)
        got = yk.variance(moments, p["film"], p["guides"], vpar, tile_dim=td, samples=samples, albedo=albedo, ctx=ctx)
        bad = ref.bits(got) != ref.bits(host_results["variance", case[0]])
        assert not bad.any(), (case[0], int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], host_results["variance", case[0]][bad][:4])


@pytest.mark.parametrize("lds_max_step", [0, 1, 2])
def test_filter_device_equals_host(ctx, yk, host_results, lds_max_step):
    ctx.set_option("denoise_lds_max_step", lds_max_step)
    try:
        for case in FILTER_CASES:
            p, vpar, albedo, td, samples = _filter_args(yk, case)
            got = yk.denoise(p["film"], p["guides"], vpar, tile_dim=td, samples=samples, albedo=albedo, variance=p["variance"], ctx=ctx)
            want = host_results["filter", case[0]]
            bad = ref.bits(got) != ref.bits(want)
            assert not bad.any(), (case[0], lds_max_step, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])
    finally:
        ctx.set_option("denoise_lds_max_step", DEFAULT_LDS_MAX_STEP)


# ------------------------------------------------------------------ device pointers, offsets, guard words, in place
POINTER_SIZES = ((5, 3), (37, 23), (130, 70))


def test_device_pointers_offsets_guard_words_and_in_place(ctx, yk, host_results):
    """The _device calls on torch buffers and a stream of the caller's: the film and the variance at 4-byte offsets, the
    records at 16-byte offsets, every buffer between guard words that stay intact; the filter and the blend once more in
    place; the inputs are only read."""
    import torch

    s = torch.cuda.Stream()
    cs = s.cuda_stream
    for w, h in POINTER_SIZES:
        p = PIC[(w, h)]
        n = w * h
        res = (w, h)
        d_film, d_g, d_a = _between_guards(torch, 3 * n, 1, p["film"]), _between_guards(torch, 8 * n, 8, p["guides"]), _between_guards(torch, 4 * n, 4, p["albedo"])
        d_m, d_v = _between_guards(torch, 4 * n, 4, p["moments"]), _between_guards(torch, n, 3, p["variance"])
        d_om, d_ov, d_out = _between_guards(torch, 4 * n, 12), _between_guards(torch, n, 1), _between_guards(torch, 3 * n, 3)
        torch.cuda.synchronize()
        film, g, a, m, v = d_film.data_ptr() + 4, d_g.data_ptr() + 32, d_a.data_ptr() + 16, d_m.data_ptr() + 16, d_v.data_ptr() + 12
        ctx.blend_moments_device(film, res, tparams(yk), 16, p["samples"], m, d_om.data_ptr() + 48, stream=cs)
        ctx.variance_device(m, film, g, res, vparams(yk), 16, None, d_ov.data_ptr() + 4, stream=cs, albedo=a)
        ctx.denoise_variance_device(film, g, v, res, vparams(yk, 3), 16, None, d_out.data_ptr() + 12, stream=cs, albedo=a)
        s.synchronize()
        same_bits(_payload(d_om, 12, 4 * n).view(np.float32), moments_words(host_results["blend", f"{w}x{h}-moments-samples"]).reshape(-1))
        same_bits(_payload(d_ov, 1, n).view(np.float32), host_results["variance", f"{w}x{h}-moments-albedo"].reshape(-1))
        want = yk.denoise(p["film"], p["guides"], vparams(yk, 3), albedo=p["albedo"], variance=p["variance"])
        same_bits(_payload(d_out, 3, 3 * n).view(np.float32), want.reshape(-1))
        for t, lead, data in ((d_film, 1, p["film"]), (d_g, 8, p["guides"]), (d_a, 4, p["albedo"]), (d_m, 4, p["moments"]), (d_v, 3, p["variance"])):
            assert np.array_equal(_payload(t, lead, data.nbytes // 4), np.ascontiguousarray(data).view(np.uint32).reshape(-1))  # only read
        # in place: the moments into themselves, the filter into the film
        ctx.blend_moments_device(film, res, tparams(yk), 16, p["samples"], m, m, stream=cs)
        ctx.denoise_variance_device(film, g, v, res, vparams(yk, 3), 16, None, film, stream=cs, albedo=a)
        s.synchronize()
        same_bits(_payload(d_m, 4, 4 * n).view(np.float32), moments_words(host_results["blend", f"{w}x{h}-moments-samples"]).reshape(-1))
        same_bits(_payload(d_film, 1, 3 * n).view(np.float32), want.reshape(-1))


@pytest.mark.parametrize("size", [(37, 23), (1, 1)], ids=["37x23", "1x1"])
def test_every_moments_instance_writes_its_records_only(ctx, yk, host_results, size):
    """The four instances of the shared record blend that carry the moments rule — {table, no table} x {moments, none} —
    through blend_moments_device: the records equal the host instance's bit for bit, and neither the film nor an
    RGB-sized buffer of guard words — the history blend's instances have an RGB output, these have none — is written."""
    import torch

    s = torch.cuda.Stream()
    w, h = size
    n = w * h
    p = PIC[size]
    d_film, d_m = _between_guards(torch, 3 * n, 1, p["film"]), _between_guards(torch, 4 * n, 4, p["moments"])
    d_rgb = _between_guards(torch, 3 * n, 3)
    for name, case_size, td, sk, hist in BLEND_CASES:
        if case_size != size:
            continue
        d_om = _between_guards(torch, 4 * n, 8)
        torch.cuda.synchronize()
        ctx.blend_moments_device(d_film.data_ptr() + 4, size, tparams(yk), td, None if sk is None else p[sk], d_m.data_ptr() + 16 if hist else None, d_om.data_ptr() + 32, stream=s.cuda_stream)
        s.synchronize()
        same_bits(_payload(d_om, 8, 4 * n).view(np.float32), moments_words(host_results["blend", name]).reshape(-1))
        assert np.array_equal(_payload(d_film, 1, 3 * n), p["film"].view(np.uint32).reshape(-1)), name  # only read
        assert np.array_equal(_payload(d_m, 4, 4 * n), np.ascontiguousarray(p["moments"]).view(np.uint32).reshape(-1)), name
        assert np.all(d_rgb.cpu().numpy() == GUARD), name


def test_misaligned_or_overlapping_buffers_are_refused(ctx, yk):
    import torch

    w, h = 8, 8
    n = w * h
    fill = lambda k, v: torch.full((k + 8,), v, dtype=torch.float32, device="cuda:0")  # noqa: E731
    film, guides, albedo, moments, var = fill(3 * n, 3.0), fill(8 * n, 2.0), fill(4 * n, 1.0), fill(4 * n, 4.0), fill(n, 0.5)
    rec = torch.full((4 * n + 8,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    Fm, G, A, M, V, R = (t.data_ptr() for t in (film, guides, albedo, moments, var, rec))
    tp, vpar = tparams(yk), vparams(yk, 2)
    status = []

    def refused(call, *args, **kw):
        with pytest.raises(yk.YukiError) as e:
            call(*args, **kw)
        status.append(e.value.status)

    # moments blend: (film, moments, out)
    for f, m, o in ((Fm + 1, M, R), (Fm, M + 4, R), (Fm, M + 8, R), (Fm, M, R + 4), (Fm, M, R + 8), (Fm, M, M + 16), (Fm, M, Fm), (Fm, M, Fm + 12 * n - 4), (None, M, R), (Fm, M, None)):
        refused(ctx.blend_moments_device, f, (w, h), tp, 16, None, m, o)
    # variance: (moments, film, guides, albedo, out)
    for m, f, g, a, o in ((M + 4, Fm, G, A, R), (M, Fm + 2, G, A, R), (M, Fm, G + 4, A, R), (M, Fm, G + 8, A, R), (M, Fm, G, A + 4, R), (M, Fm, G, A, R + 1), (M, Fm, G, A, R + 2),
                          (M, Fm, G, A, M), (M, Fm, G, A, Fm + 8), (M, Fm, G, A, G + 32 * n - 4), (M, Fm, G, A, A + 4), (M, None, G, A, R), (M, Fm, None, A, R), (M, Fm, G, A, None)):  # fmt: skip
        refused(ctx.variance_device, m, f, g, (w, h), vpar, 16, None, o, albedo=a)
    # filter: (film, guides, variance, albedo, out)
    for f, g, v, a, o in ((Fm + 1, G, V, A, R), (Fm, G + 4, V, A, R), (Fm, G, V + 2, A, R), (Fm, G, V, A + 8, R), (Fm, G, V, A, R + 2), (Fm, G, V, A, A), (Fm, G, V, A, A + 16 * n - 4),
                          (Fm, G, V, A, G), (Fm, G, V, A, V), (Fm, G, V, A, V + 4 * n - 4), (Fm, G, V, A, Fm + 12), (Fm, G, None, A, R), (None, G, V, A, R), (Fm, None, V, A, R)):  # fmt: skip
        refused(ctx.denoise_variance_device, f, g, v, (w, h), vpar, 16, None, o, albedo=a)
    refused(ctx.denoise_variance_device, Fm, G, V, (w, h), vparams(yk, 9), 16, None, R)
    assert set(status) == {1}
    torch.cuda.synchronize()
    assert np.all(rec.cpu().numpy() == GUARD)  # nothing was launched
    for t, val in ((film, 3.0), (guides, 2.0), (albedo, 1.0), (moments, 4.0), (var, 0.5)):
        assert np.all(t.cpu().numpy() == val)


# ------------------------------------------------------------------ the chain
def test_the_chain_on_one_torch_stream(ctx, yk):
    """Three frames of city-small at 100 x 60, each rendered into a cleared device film (four accumulating passes); guides
    once; before the third frame the camera moves: history and moments go through reproject_history_device.  Every frame:
    blend, moments blend, variance, filter, tone map, present — everything enqueued on one torch stream, one
    synchronisation at the end.  Equals the host instances run on copies of the device's films and guides, bit for bit."""
    import torch

    from yuki_amd import scenes

    sd = scenes.by_name("city-small")
    res = (100, 60)
    window = (160, 90)
    n = res[0] * res[1]
    fs = yk.FilmSettings(res=res, tile_dim=16, accumulate=True)
    cam_a = yk.Camera(sd.camera, fs)
    moved = dict(sd.camera)
    moved["position"] = tuple(np.asarray(sd.camera["position"], np.float64) + np.array([0.3, 0.05, 0.0]))
    cam_b = yk.Camera(moved, fs)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=5)))
    sc = yk.Scene(ctx, sd)
    tiles = yk.film_tiles(fs)
    lists = [yk.TileList(ctx, tiles, np.full(len(tiles), k, np.uint16)) for k in range(4)]
    samples = yk.film_samples(fs, tiles, np.full(len(tiles), 4, np.uint32))
    td = yk.film_tile_dim(fs)
    tp = yk.TemporalParams.for_scene(sc, max_history=32.0)
    vpar = yk.VarianceParams.for_scene(sc, iterations=4)
    stream = torch.cuda.Stream()
    z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda:0")  # noqa: E731
    slab = z(lists[0].n_pixels * 3)
    films = [z(3 * n) for _ in range(3)]
    guides = [z(8 * n), z(8 * n)]
    hist, mom, hist_r, mom_r, rgb, var, clean = z(4 * n), z(4 * n), z(4 * n), z(4 * n), z(3 * n), z(n), z(3 * n)
    frames_out = [torch.zeros(window[0] * window[1], dtype=torch.int32, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()
    cs = stream.cuda_stream
    ctx.render_guides_device(sc, cam_a, res, guides[0].data_ptr(), stream=cs)
    ctx.render_guides_device(sc, cam_b, res, guides[1].data_ptr(), stream=cs)
    for k in range(3):
        cam, g = (cam_a, guides[0]) if k < 2 else (cam_b, guides[1])
        smp = yk.SamplerType.Stratified((2, 2), True, SEED + k)
        for tl in lists:
            it.render_tile_list_device(sc, cam, smp, tl, slab.data_ptr(), stream=cs)
            tl.update_film_device(slab.data_ptr(), fs.res, films[k].data_ptr(), stream=cs, accumulate=True)
        h_in, m_in = (None, None) if k == 0 else (hist.data_ptr(), mom.data_ptr())
        if k == 2:
            ctx.reproject_history_device(hist.data_ptr(), guides[0].data_ptr(), cam_a, g.data_ptr(), res, tp, hist_r.data_ptr(), stream=cs)
            ctx.reproject_history_device(mom.data_ptr(), guides[0].data_ptr(), cam_a, g.data_ptr(), res, tp, mom_r.data_ptr(), stream=cs)
            h_in, m_in = hist_r.data_ptr(), mom_r.data_ptr()
        ctx.blend_history_device(films[k].data_ptr(), res, tp, td, samples, h_in, hist.data_ptr(), rgb.data_ptr(), stream=cs)
        ctx.blend_moments_device(films[k].data_ptr(), res, tp, td, samples, m_in, mom.data_ptr(), stream=cs)
        ctx.variance_device(mom.data_ptr(), rgb.data_ptr(), g.data_ptr(), res, vpar, td, None, var.data_ptr(), stream=cs)
        ctx.denoise_variance_device(rgb.data_ptr(), g.data_ptr(), var.data_ptr(), res, vpar, td, None, clean.data_ptr(), stream=cs)
        ctx.tone_map_device(clean.data_ptr(), res, td, yk.ToneMapType.default(), None, clean.data_ptr(), stream=cs)
        ctx.present_device(clean.data_ptr(), res, window, 2, "rgba8", frames_out[k].data_ptr(), stream=cs)
    stream.synchronize()
    hg = [g.cpu().numpy().view(abi.GUIDE_DTYPE).reshape(res[1], res[0]) for g in guides]
    h_hist = h_mom = None
    temporal_frames = []
    for k in range(3):
        film = films[k].cpu().numpy().reshape(res[1], res[0], 3)
        assert np.abs(film).max() > 0
        g = hg[0] if k < 2 else hg[1]
        if k == 2:
            h_hist = yk.reproject_history(h_hist, hg[0], cam_a, g, tp)
            h_mom = yk.reproject_history(h_mom.view(abi.HISTORY_DTYPE), hg[0], cam_a, g, tp).view(abi.MOMENTS_DTYPE)
            assert (h_mom["n"] > 0).sum() > n // 2 and (h_mom["n"] == 0).any()  # carried, with disocclusions
        h_rgb, h_hist = yk.blend_history(film, tp, tile_dim=td, samples=samples, history=h_hist)
        h_mom = yk.blend_moments(film, tp, tile_dim=td, samples=samples, moments=h_mom)
        h_var = yk.variance(h_mom, h_rgb, g, vpar)
        temporal_frames.append(int((h_mom["frames"] >= 2).sum()))
        h_clean = yk.denoise(h_rgb, g, vpar, variance=h_var)
        h_mapped = yk.tone_map(h_clean, yk.ToneMapType.default(), td)
        want = yk.present(h_mapped, window, 2, "rgba8")
        assert np.array_equal(frames_out[k].cpu().numpy().view(np.uint8).reshape(window[1], window[0], 4), want), k
    same_bits(mom.cpu().numpy(), moments_words(h_mom).reshape(-1))
    same_bits(var.cpu().numpy(), h_var.reshape(-1))
    assert temporal_frames[0] == 0 and temporal_frames[1] > n // 2 and 0 < temporal_frames[2] < n  # both estimates were used
    for tl in lists:
        tl.close()
    sc.close()


# ------------------------------------------------------------------ quality
@pytest.mark.parametrize("name,res", QUALITY["scenes"], ids=[s[0] for s in QUALITY["scenes"]])
def test_quality_on_device_films(ctx, yk, name, res):
    """The conditions of tests/test_variance.py on films and guides the device rendered, filtered on the device."""
    from test_variance import quality_errors
    from yuki_amd import scenes

    q = QUALITY
    sd = scenes.cornell() if name == "cornell" else scenes.by_name(name)
    fs = yk.FilmSettings(res=res, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    sc = yk.Scene(ctx, sd)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=q["depth"])))
    render = lambda spp, seed: yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(spp, seed), tiles)[0], fs.res)  # noqa: E731
    frames = [render(q["frame_spp"], SEED + 977 * k) for k in range(8)]
    conv = render(q["converged_spp"], SEED ^ 0x1234567)
    guides = yk.render_guides(ctx, sc, cam, fs)
    sp = yk.DenoiseParams.for_scene(sc).sigma_plane
    e_noisy, e_plain1, e_var1 = quality_errors(yk, frames, conv, guides, sp, 1, ctx=ctx)
    e_blend4, e_plain4, e_var4 = quality_errors(yk, frames, conv, guides, sp, 4, ctx=ctx)
    e_blend8, e_plain8, e_var8 = quality_errors(yk, frames, conv, guides, sp, 8, ctx=ctx)
    print(f"quality {name}: 1 frame noisy {e_noisy:.4f} plain {e_plain1:.4f} variance-guided {e_var1:.4f} ratio to plain {e_var1 / e_plain1:.3f}")
    print(f"quality {name}: 4 frames blended {e_blend4:.4f} plain {e_plain4:.4f} variance-guided {e_var4:.4f} ratio {e_var4 / e_plain4:.3f}")
    print(f"quality {name}: 8 frames blended {e_blend8:.4f} plain {e_plain8:.4f} variance-guided {e_var8:.4f}")
    assert e_var1 < e_noisy, (e_noisy, e_var1)
    assert e_var4 < e_plain4 and e_var4 < e_blend4, (e_blend4, e_plain4, e_var4)
    if name == "city-small":
        assert e_var4 <= q["bound"] * e_plain4, (e_plain4, e_var4)
    assert e_var8 < e_blend8, (e_blend8, e_plain8, e_var8)
    sc.close()
