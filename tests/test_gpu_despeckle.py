"""The despeckle pass on the MI355X (yk_despeckle with a context and yk_despeckle_device): the device instance equals the
host instance bit for bit on the whole matrix of the CPU suite — films, masks and counts; on device pointers at 16-byte
offsets (the film at a 4-byte one) between guard words on a caller's torch stream, the inputs only read; misaligned and
overlapping buffers are refused with nothing launched; with and without mask and counts the film is the same; despeckle,
rectify, blend and moments blend on one torch stream equal the host chain; and the 8-frame quality condition holds on
frames the device rendered."""
import numpy as np
import pytest

import despeckle_ref as ref
import rectify_ref
from test_despeckle import MEAN_BOUNDS, QUALITY, SEED, dp, mean_errors, run
from test_gpu_temporal import GUARD, _between_guards, _payload
from test_temporal import same_bits
from yuki_amd import abi, scenes

pytestmark = pytest.mark.gpu
GUARD_BYTE = 0xA5
key = lambda row: (row[0][0],) + row[1:]  # noqa: E731


@pytest.fixture(scope="module")
def host_despeckled(yk):
    """The host instance on the whole matrix, computed once and left unchanged."""
    out = {}
    for row in ref.matrix():
        film, mask, counts = run(yk, row)
        film.setflags(write=False)
        mask.setflags(write=False)
        out[key(row)] = (film, mask, counts)
    return out


def test_device_equals_host_host_buffers(ctx, yk, host_despeckled):
    for row in ref.matrix():
        film, mask, counts = run(yk, row, ctx=ctx)
        w_film, w_mask, w_counts = host_despeckled[key(row)]
        assert same_bits(film, w_film) and np.array_equal(mask, w_mask) and counts == w_counts, key(row)
    name, film, td, samples = next(c for c in ref.cases() if c[0] == "65x17-td7")
    for gain, floor in ((0.0, 0.0), (1.5, 0.0), (1.0, 1.0), (4.0, 0.5)):
        p = dp(yk, 2, 2, gain, floor=floor, repair=True)
        got, want = yk.despeckle(film, p, tile_dim=td, samples=samples, ctx=ctx, return_mask=True), yk.despeckle(film, p, tile_dim=td, samples=samples, return_mask=True)
        assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (gain, floor)


def _mask_between_guards(torch, n):
    return torch.full((16 + n + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda:0")


def _mask_payload(t, n):
    a = t.cpu().numpy()
    assert np.all(a[:16] == GUARD_BYTE) and np.all(a[16 + n :] == GUARD_BYTE)
    return a[16 : 16 + n]


def test_device_pointers_offsets_and_guard_words(ctx, yk, host_despeckled):
    """The _device call on torch buffers and a stream of the caller's: the film at a 4-byte offset, the output and the
    mask at 16-byte offsets, the counts at a 4-byte one (16 + 4), every buffer between guard words that stay intact; the film
    is only read; and without mask and counts the film is the same."""
    import torch

    s = torch.cuda.Stream()
    for row in ref.matrix():
        (name, film, td, samples), radius, rank, repair, gain, min_taps, floor = row
        if not name.startswith(("37x23", "65x17", "1x1", "2x1-td16", "64x36-td16")) or gain == ref.INF or rank == 3:
            continue
        h, w = film.shape[:2]
        n = w * h
        w_film, w_mask, w_counts = host_despeckled[key(row)]
        p = dp(yk, radius, rank, gain, min_taps=min_taps, floor=floor, repair=repair)
        d_film, d_out, d_bare = _between_guards(torch, 3 * n, 1, film), _between_guards(torch, 3 * n, 4), _between_guards(torch, 3 * n, 8)
        d_mask, d_counts = _mask_between_guards(torch, n), _between_guards(torch, 2, 5)
        torch.cuda.synchronize()
        fp = d_film.data_ptr() + 4
        ctx.despeckle_device(fp, (w, h), p, td, samples, d_out.data_ptr() + 16, stream=s.cuda_stream, mask=d_mask.data_ptr() + 16, counts=d_counts.data_ptr() + 20)
        ctx.despeckle_device(fp, (w, h), p, td, samples, d_bare.data_ptr() + 32, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(_payload(d_out, 4, 3 * n), w_film.view(np.uint32).reshape(-1)), key(row)
        assert np.array_equal(_payload(d_bare, 8, 3 * n), w_film.view(np.uint32).reshape(-1)), key(row)
        assert np.array_equal(_mask_payload(d_mask, n), w_mask.reshape(-1)), key(row)
        assert tuple(int(v) for v in _payload(d_counts, 5, 2)) == w_counts, key(row)
        assert np.array_equal(_payload(d_film, 1, 3 * n), film.view(np.uint32).reshape(-1))  # the input is only read


def test_tensors_are_taken_as_they_are(ctx, yk):
    import torch

    name, film, td, samples = next(c for c in ref.cases() if c[0] == "64x36-tdNone")
    h, w = film.shape[:2]
    d_film = torch.from_numpy(film).to("cuda:0")
    d_out, d_mask, d_counts = torch.zeros_like(d_film), torch.zeros((h, w), dtype=torch.uint8, device="cuda:0"), torch.full((2,), 77, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.despeckle_device(d_film, (w, h), dp(yk, 1, 1, 2.0), td, samples, d_out, mask=d_mask, counts=d_counts)
    torch.cuda.synchronize()  # the context's own stream is a stream of the same device
    want = yk.despeckle(film, dp(yk, 1, 1, 2.0), return_mask=True)
    assert same_bits(d_out.cpu().numpy(), want[0]) and np.array_equal(d_mask.cpu().numpy(), want[1]) and tuple(d_counts.cpu().numpy().tolist()) == want[2]


def test_misaligned_or_overlapping_buffers_are_refused(ctx, yk):
    import torch

    w, h = 8, 8
    n = w * h
    film = torch.ones(3 * n + 8, dtype=torch.float32, device="cuda:0")
    out = torch.full((3 * n + 8,), GUARD, dtype=torch.int32, device="cuda:0")
    mask = torch.full((n + 16,), GUARD_BYTE, dtype=torch.uint8, device="cuda:0")
    counts = torch.full((4,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    F, O, M, C = (t.data_ptr() for t in (film, out, mask, counts))
    bad = [(F + off, O, M, C) for off in (1, 2, 3)] + [(F, O + off, M, C) for off in (1, 2, 3)] + [(F, O, M, C + off) for off in (1, 2, 3)]
    bad += [(F, F, M, C), (F, F + 4, M, C), (F, F + 12 * n - 4, M, C), (F + 12, F, M, C)]  # the output on the film: never in place
    bad += [(F, O, F, C), (F, O, O + 12 * n - 1, C), (F, O, M, F + 4), (F, O, M, O + 12 * n - 4), (F, O, M, M), (F, O, C, C), (F, O, M, M + n - 4)]
    bad += [(None, O, M, C), (F, None, M, C)]
    for f, o, m, c in bad:
        with pytest.raises(yk.YukiError) as e:
            ctx.despeckle_device(f, (w, h), dp(yk), 16, None, o, mask=m, counts=c)
        assert e.value.status == 1, (f, o, m, c)
    for desc in (dict(radius=0), dict(radius=3), dict(rank=0), dict(rank=5, min_taps=5), dict(rank=2, min_taps=1), dict(gain=float("nan")), dict(gain=-0.5), dict(floor=float("inf")), dict(floor=-1.0)):
        with pytest.raises(yk.YukiError) as e:
            ctx.despeckle_device(F, (w, h), yk.DespeckleParams(**desc), 16, None, O, mask=M, counts=C)
        assert e.value.status == 1, desc
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == GUARD) and np.all(mask.cpu().numpy() == GUARD_BYTE) and np.all(counts.cpu().numpy() == GUARD)  # nothing was launched
    assert np.all(film.cpu().numpy() == 1.0)


def test_the_chain_on_one_torch_stream(ctx, yk):
    """Despeckle the frame, rectify the history and the moments in place against the despeckled film, blend the history,
    blend the moments: four calls on one torch stream and one synchronisation, equal to the host chain bit for bit."""
    import torch

    stream = torch.cuda.Stream()
    cs = stream.cuda_stream
    tp, rp, p = yk.TemporalParams(max_history=32.0), yk.RectifyParams(radius=2, gamma=1.0), dp(yk, 1, 2, 1.5, repair=True)
    rng = np.random.default_rng(7)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(-1).copy()).to("cuda:0")  # noqa: E731
    z = lambda k: torch.zeros(k, dtype=torch.float32, device="cuda:0")  # noqa: E731
    for w, h in ((37, 23), (65, 17), (259, 131)):
        n = w * h
        with np.errstate(all="ignore"):
            film = (ref.make_film(rng, w, h) * np.float32(3)).astype(np.float32)
        samples = rectify_ref.temporal_ref.make_samples(rng, w, h, 16)
        hist = rectify_ref.temporal_ref.make_history(rng, w, h)
        mom = rectify_ref.make_moments(rng, w, h, hist)
        d_film, d_hist, d_mom = up(film), up(hist), up(mom)
        clean, out_h, out_m, rgb = z(3 * n), z(4 * n), z(4 * n), z(3 * n)
        torch.cuda.synchronize()
        ctx.despeckle_device(d_film, (w, h), p, 16, samples, clean, stream=cs)
        ctx.rectify_history_device(clean.data_ptr(), (w, h), rp, 16, samples, d_hist.data_ptr(), d_hist.data_ptr(), stream=cs, moments=d_mom.data_ptr(), out_moments=d_mom.data_ptr())
        ctx.blend_history_device(clean.data_ptr(), (w, h), tp, 16, samples, d_hist.data_ptr(), out_h.data_ptr(), rgb.data_ptr(), stream=cs)
        ctx.blend_moments_device(clean.data_ptr(), (w, h), tp, 16, samples, d_mom.data_ptr(), out_m.data_ptr(), stream=cs)
        stream.synchronize()
        want_clean = yk.despeckle(film, p, tile_dim=16, samples=samples)
        want_c, want_cm = yk.rectify_history(hist, want_clean, rp, tile_dim=16, samples=samples, moments=mom)
        want_rgb, want_h = yk.blend_history(want_clean, tp, tile_dim=16, samples=samples, history=want_c)
        want_m = yk.blend_moments(want_clean, tp, tile_dim=16, samples=samples, moments=want_cm)
        rec = lambda t, dt: t.cpu().numpy().view(dt).reshape(h, w)  # noqa: E731
        assert same_bits(clean.cpu().numpy().reshape(h, w, 3), want_clean) and not same_bits(want_clean, film), (w, h)
        assert same_bits(rec(d_hist, abi.HISTORY_DTYPE), want_c) and same_bits(rec(d_mom, abi.MOMENTS_DTYPE), want_cm), (w, h)
        assert same_bits(rec(out_h, abi.HISTORY_DTYPE), want_h) and same_bits(rec(out_m, abi.MOMENTS_DTYPE), want_m), (w, h)
        assert same_bits(rgb.cpu().numpy().reshape(h, w, 3), want_rgb), (w, h)


def test_quality_on_device_rendered_frames(ctx, yk):
    """cornell 48 x 48 at 4 spp from the device: every frame despeckled on the device equals the host instance on the same
    film, and the despeckled 8-frame mean beats the raw one by the CPU suite's bound."""
    q, name = QUALITY, "cornell"
    sd = scenes.by_name(name)
    fs = yk.FilmSettings(res=(48, 48), tile_dim=16)
    sc = yk.Scene(ctx, sd)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=q["depth"])))
    render = lambda spp, seed: yk.update_tiles(tiles, it.render_tiles(sc, cam, yk.SamplerType.Uniform(spp, seed), tiles)[0], fs.res)  # noqa: E731
    frames = [render(q["noisy_spp"], SEED + 977 * k) for k in range(1, q["frames"] + 1)]
    conv = render(q["converged_spp"], SEED ^ 0x1234567)
    p = yk.DespeckleParams()
    for f in frames:
        got, want = yk.despeckle(f, p, ctx=ctx, return_mask=True), yk.despeckle(f, p, return_mask=True)
        assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] and got[2][0] > 0
    e_raw, e_des, n_clamped, kept = mean_errors(yk, frames, conv, p, ctx=ctx)
    print(f"despeckle quality {name} (device): raw {e_raw:.4f} despeckled {e_des:.4f} ratio {e_des / e_raw:.4f} bound {MEAN_BOUNDS[name]}; {n_clamped:.1f} pixels clamped, {kept:.3f} of the luminance kept per frame")
    assert e_des < e_raw and e_des <= MEAN_BOUNDS[name] * e_raw, (e_raw, e_des)
    sc.close()
