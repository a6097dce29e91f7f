"""The despeckle pass (yuki_amd/csrc/yk_despeckle.h: a film pixel far brighter than its neighbourhood is scaled down to a
rank-conditioned bound, before anything else reads the film) on the host: the library's host instance against an independent
numpy float32 restatement (tests/despeckle_ref.py) bit for bit, the exact properties of the rule, the argument errors, the
Python layer, the quality conditions on oracle-rendered films, and the rule's stand-alone program under the host
sanitizers.  No GPU."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import despeckle_ref as ref
from test_denoise import oracle_guides, quality_error
from test_temporal import same_bits
from yuki_amd import _ffi, abi, scenes

F = np.float32
SEED = 0x73B9642E74AC471C
INF = float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dp(yk, radius=1, rank=1, gain=2.0, **kw):  # the matrix's parameters, not the defaults
    return yk.DespeckleParams(radius=radius, rank=rank, gain=gain, **kw)


def run(yk, row, ctx=None):
    """One row of ref.matrix() through the library -> (film, mask, counts)."""
    (name, film, td, samples), radius, rank, repair, gain, min_taps, floor = row
    return yk.despeckle(film, dp(yk, radius, rank, gain, min_taps=min_taps, floor=floor, repair=repair), tile_dim=td, samples=samples, ctx=ctx, return_mask=True)


def want(row):
    (name, film, td, samples), radius, rank, repair, gain, min_taps, floor = row
    return ref.despeckle(film, radius, rank, gain, min_taps, floor, repair, td, samples)


def check_matrix(yk, ctx=None):
    """Every row against the restatement: films, masks and counts; the matrix exercises every way out of the rule."""
    clamped = passed = repaired = 0
    for row in ref.matrix():
        got, mask, counts = run(yk, row, ctx)
        w_film, w_mask, w_counts = want(row)
        assert same_bits(got, w_film), (row[0][0],) + row[1:]
        assert np.array_equal(mask, w_mask) and counts == w_counts, (row[0][0],) + row[1:]
        clamped += counts[0]
        repaired += counts[1]
        passed += mask.size - counts[0] - counts[1]
    assert clamped > 1000 and passed > 1000 and repaired > 100, (clamped, passed, repaired)


def test_descriptor_layout():
    assert C.sizeof(abi.DespeckleDesc) == 24
    assert [getattr(abi.DespeckleDesc, k).offset for k in ("radius", "rank", "min_taps", "flags", "gain", "floor")] == [0, 4, 8, 12, 16, 20]
    assert (abi.DESPECKLE_REPAIR, abi.DESPECKLE_UNTOUCHED, abi.DESPECKLE_CLAMPED, abi.DESPECKLE_REPAIRED) == (1, ref.UNTOUCHED, ref.CLAMPED, ref.REPAIRED)


def test_host_equals_restatement(yk):
    check_matrix(yk)


def test_an_infinite_gain_is_the_identity(yk):
    for name, film, td, samples in ref.cases():
        for radius in ref.RADII:
            for rank in ref.RANKS:
                got, mask, counts = yk.despeckle(film, dp(yk, radius, rank, INF, min_taps=rank, floor=0.0), tile_dim=td, samples=samples, return_mask=True)
                assert same_bits(got, film) and not mask.any() and counts == (0, 0), (name, radius, rank)


def test_a_constant_film_is_untouched(yk):
    film = np.empty((9, 33, 3), np.float32)
    film[...] = (0.3, 0.7, 0.1)
    for radius in ref.RADII:
        for rank in ref.RANKS:
            for gain in (1.0, 1.5, 4.0):
                got, mask, counts = yk.despeckle(film, dp(yk, radius, rank, gain, min_taps=rank), return_mask=True)
                assert same_bits(got, film) and counts == (0, 0)


def test_one_bright_pixel_comes_out_at_the_gain(yk):
    w, h = 37, 23
    base = np.array((0.3, 0.7, 0.1), np.float32)
    film = np.empty((h, w, 3), np.float32)
    film[...] = base
    film[11, 17] = (90.0, 30.0, 60.0)
    lum = ref.luminance(film)
    for radius in ref.RADII:
        for gain in (1.0, 2.0, 3.0):
            got, mask, counts = yk.despeckle(film, dp(yk, radius, 1, gain), return_mask=True)
            others = np.ones((h, w), bool)
            others[11, 17] = False
            assert same_bits(got[others], film[others]) and counts == (1, 0) and mask[11, 17] == 1 and not mask[others].any()
            s = F(F(gain) * lum[0, 0]) / lum[11, 17]
            assert same_bits(got[11, 17], film[11, 17] * F(s))
            assert abs(float(ref.luminance(got[11, 17])) - gain * float(lum[0, 0])) < 1e-5  # gain x the constant's luminance
            assert np.allclose(got[11, 17] / got[11, 17].sum(), film[11, 17] / film[11, 17].sum(), rtol=1e-6)  # the chromaticity
    # rank 2 looks past ONE bright neighbour, not past two
    film[11, 18] = (90.0, 30.0, 60.0)
    assert yk.despeckle(film, dp(yk, 1, 1, 2.0), return_mask=True)[2] == (0, 0)
    assert yk.despeckle(film, dp(yk, 1, 2, 2.0), return_mask=True)[2] == (2, 0)


def test_a_negative_zero_gain_or_floor_is_a_zero(yk):
    """gain = -0 and floor = -0 pass the descriptor check (-0 >= 0) and are taken as +0: the same bits as with +0, which are
    the restatement's, and a clamped positive channel comes out +0, never -0."""
    for name, film, td, samples in ref.cases():
        if not name.startswith(("37x23", "65x17")):
            continue
        for gain, floor in ((-0.0, -0.0), (-0.0, 0.25), (2.0, -0.0)):
            got = yk.despeckle(film, dp(yk, 1, 1, gain, floor=floor), tile_dim=td, samples=samples, return_mask=True)
            pos = yk.despeckle(film, dp(yk, 1, 1, abs(gain), floor=abs(floor)), tile_dim=td, samples=samples, return_mask=True)
            w_film, w_mask, w_counts = ref.despeckle(film, 1, 1, gain, 3, floor, False, td, samples)
            assert same_bits(got[0], pos[0]) and same_bits(got[0], w_film) and np.array_equal(got[1], w_mask) and got[2] == pos[2] == w_counts and got[2][0] > 0
            if gain == 0.0 and floor == 0.0:
                hit = (got[1] == 1)[..., None] & (film > 0)
                assert hit.any() and not np.signbit(got[0][hit]).any() and np.all(got[0][hit] == 0)


def test_a_pixel_below_the_floor_is_never_clamped(yk):
    name, film, td, samples = next(c for c in ref.cases() if c[0] == "37x23-tdNone")
    lum = ref.luminance(film)
    for floor in (0.5, 2.0, 1e6):
        got, mask, _ = yk.despeckle(film, dp(yk, 1, 1, 1.0, floor=floor), return_mask=True)
        assert not (mask[lum <= F(floor)] == 1).any()
        if floor < 1e6:
            assert (mask == 1).any()
        with np.errstate(all="ignore"):
            out_l = ref.luminance(got)[mask == 1]
        assert np.all(out_l >= F(floor) * F(1 - 1e-4))  # nothing is pushed under the floor either (up to the rounding of three products)


def test_a_bad_pixel_only_leaves_the_windows_and_repair_gives_the_mean(yk):
    rng = np.random.default_rng(2)
    w, h, td = 37, 23, 1
    film = np.abs(0.5 + 0.2 * rng.standard_normal((h, w, 3))).astype(np.float32)
    samples = np.ones(w * h, np.uint32)  # tile_dim 1: a count per pixel
    bad = [(11, 17), (0, 0), (22, 36), (5, 6), (5, 8)]
    p = dp(yk, 2, 2, 1.0)
    for poison in (np.nan, np.inf, -np.inf):
        f, s = film.copy(), samples.copy()
        for k, (y, x) in enumerate(bad):
            f[y, x, k % 3] = poison
            s[y * w + x] = 0
        got = yk.despeckle(f, p, tile_dim=td, samples=samples)
        gone = yk.despeckle(film, p, tile_dim=td, samples=s)  # the same windows without those taps
        rest = np.ones((h, w), bool)
        for y, x in bad:
            rest[y, x] = False
            assert same_bits(got[y, x], f[y, x])  # without repair a pixel that is not finite keeps its bits
        assert same_bits(got[rest], gone[rest])
        fixed, mask, counts = yk.despeckle(f, dp(yk, 2, 2, 1.0, repair=True), tile_dim=td, samples=samples, return_mask=True)
        assert counts[1] == len(bad) and same_bits(fixed[rest], got[rest]) and np.isfinite(fixed).all()
        for y, x in bad:
            assert mask[y, x] == 2
            acc, k = np.zeros(3, np.float32), 0
            for qy in range(max(0, y - 2), min(h, y + 3)):
                for qx in range(max(0, x - 2), min(w, x + 3)):
                    if (qy, qx) != (y, x) and np.isfinite(f[qy, qx]).all():
                        acc = (acc + f[qy, qx]).astype(np.float32)
                        k += 1
            assert same_bits(fixed[y, x], (acc / F(k)).astype(np.float32) * F(1))


def test_a_pixel_without_samples_and_one_pixel_pass_through(yk):
    w, h, td = 33, 9, 16
    film = np.full((h, w, 3), 0.25, np.float32)
    film[3, 5] = film[4, 20] = 1e4
    samples = np.array([4, 0, 4], np.uint32)  # the middle tile (x 16 .. 31) has no samples
    got, mask, counts = yk.despeckle(film, dp(yk), tile_dim=td, samples=samples, return_mask=True)
    assert mask[3, 5] == 1 and mask[4, 20] == 0 and counts == (1, 0) and same_bits(got[:, 16:32], film[:, 16:32])
    one = np.full((1, 1, 3), 9.0, np.float32)
    for radius in ref.RADII:
        assert same_bits(yk.despeckle(one, dp(yk, radius, 1, 0.0, min_taps=1, repair=True)), one)


def test_mask_and_counts_agree_with_the_films(yk):
    for row in ref.matrix():
        if not row[0][0].startswith(("37x23", "65x17")) or row[4] == INF:
            continue
        film = row[0][1]
        got, mask, counts = run(yk, row)
        changed = (got.view(np.uint32) != film.view(np.uint32)).any(-1)
        assert not changed[mask == 0].any() and changed[mask == 2].all()
        assert counts == (int((mask == 1).sum()), int((mask == 2).sum())) and set(np.unique(mask)) <= {0, 1, 2}
        assert same_bits(yk.despeckle(film, dp(yk, row[1], row[2], row[4], min_taps=row[5], floor=row[6], repair=row[3]), tile_dim=row[0][2], samples=row[0][3]), got)  # with and without mask


def test_every_refusal(yk):
    L = _ffi.lib()
    w, h = 8, 6
    n = w * h
    film, out = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
    mask, counts = np.zeros((h, w), np.uint8), np.zeros(2, np.uint32)
    ptr = lambda a: a if isinstance(a, (int, type(None))) else a.ctypes.data  # noqa: E731
    cv = lambda a: None if ptr(a) is None else C.c_void_p(ptr(a))  # noqa: E731
    good = (1, 1, 3, 0, 2.0, 0.0)

    def ds(desc=good, f=film, rx=w, ry=h, td=16, o=out, m=mask, c=counts, null_desc=False):
        d = abi.DespeckleDesc(*desc)
        return L.yk_despeckle(None, None if null_desc else C.byref(d), cv(f), rx, ry, td, None, cv(o), cv(m), cv(c))

    assert ds() == 0 and ds(m=None) == 0 and ds(c=None) == 0 and ds(m=None, c=None) == 0
    for d in ((1, 1, 1, 0, 0.0, 0.0), (2, 4, 4, 1, INF, 3e38), (2, 4, 0xFFFFFFFF, 1, 1.0, 0.0)):  # the ends of the ranges
        assert ds(desc=d) == 0, d
    bad = [(0, 1, 3, 0, 2.0, 0.0), (3, 1, 3, 0, 2.0, 0.0), (0xFFFFFFFF, 1, 3, 0, 2.0, 0.0)]  # radius
    bad += [(1, 0, 3, 0, 2.0, 0.0), (1, 5, 5, 0, 2.0, 0.0), (1, 0xFFFFFFFF, 0xFFFFFFFF, 0, 2.0, 0.0)]  # rank
    bad += [(1, 2, 1, 0, 2.0, 0.0), (1, 1, 0, 0, 2.0, 0.0), (2, 4, 3, 0, 2.0, 0.0)]  # min_taps < rank
    bad += [(1, 1, 3, 2, 2.0, 0.0), (1, 1, 3, 3, 2.0, 0.0), (1, 1, 3, 0x80000000, 2.0, 0.0)]  # an unknown flag
    bad += [(1, 1, 3, 0, float("nan"), 0.0), (1, 1, 3, 0, -1.0, 0.0), (1, 1, 3, 0, -INF, 0.0), (1, 1, 3, 0, -1e-30, 0.0)]  # gain
    bad += [(1, 1, 3, 0, 2.0, float("nan")), (1, 1, 3, 0, 2.0, -1.0), (1, 1, 3, 0, 2.0, INF), (1, 1, 3, 0, 2.0, -1e-30)]  # floor
    for d in bad:
        assert ds(desc=d) == 1, d
    assert ds(null_desc=True) == 1 and ds(f=None) == 1 and ds(o=None) == 1
    assert ds(rx=0) == 1 and ds(ry=0) == 1 and ds(td=0) == 1
    assert ds(o=film) == 1  # not in place: a pixel reads its neighbours' input
    assert ds(m=film) == 1 and ds(m=out) == 1 and ds(c=film) == 1 and ds(c=out) == 1 and ds(c=mask) == 1 and ds(m=counts) == 1
    big = np.zeros(3 * n * 12 + 64, np.uint8)
    base = (big.ctypes.data + 15) & ~15
    assert ds(f=base, o=base + n * 12 - 4) == 1 and ds(f=base, o=base + n * 12) == 0  # the film's last float
    assert ds(f=base + n * 12 - 4, o=base) == 1 and ds(f=base + 4, o=base) == 1
    assert ds(f=base, o=base + n * 12, m=base + 2 * n * 12 - 1) == 1 and ds(f=base, o=base + n * 12, m=base + 2 * n * 12) == 0  # the output's last byte
    assert ds(f=base, o=base + n * 12, m=base + 2 * n * 12, c=base + 2 * n * 12 + n - 1) == 1  # the mask's last byte
    assert ds(f=base, o=base + n * 12, m=base + 2 * n * 12, c=base + 2 * n * 12 + n) == 0
    assert ds(f=base, o=base + n * 12, c=base + n * 12 - 7) == 1 and ds(f=base + 16, o=base + 16 + n * 12, c=base + 9) == 1  # the counts' eight bytes
    assert not out.view(np.uint32).any() and not mask.any()  # a zero film gives zeros: nothing above wrote anything else
    with pytest.raises(_ffi.YukiError) as e:
        yk.despeckle(film, yk.DespeckleParams(radius=3))
    assert e.value.status == 1
    with pytest.raises(_ffi.YukiError):
        yk.despeckle(film, yk.DespeckleParams(rank=4, min_taps=3))
    with pytest.raises(ValueError):
        yk.despeckle(film[..., :2], dp(yk))
    with pytest.raises(ValueError):
        yk.despeckle(film, dp(yk), tile_dim=16, samples=np.zeros(5, np.uint32))
    with pytest.raises(TypeError):
        yk.despeckle(film, yk.RectifyParams())


def test_python_layer(yk, tmp_path):
    p = yk.DespeckleParams()
    assert (p.radius, p.rank, p.gain, p.min_taps, p.floor, p.repair) == (DEFAULTS["radius"], DEFAULTS["rank"], DEFAULTS["gain"], 3, 0.0, False)
    d = yk.DespeckleParams(radius=2, rank=4, gain=INF, min_taps=7, floor=0.5, repair=True).as_struct()
    assert (d.radius, d.rank, d.min_taps, d.flags, d.gain, d.floor) == (2, 4, 7, abi.DESPECKLE_REPAIR, INF, 0.5)
    # the intended use: a firefly in front of the blend is gone from what the blend keeps
    rng = np.random.default_rng(3)
    w, h = 37, 23
    film = np.abs(0.2 + 0.02 * rng.standard_normal((h, w, 3))).astype(np.float32)
    film[7, 9] = 500.0
    p = dp(yk, 1, 1, 2.0)  # clamps the firefly alone on this film: the noise is a tenth of the signal
    out = yk.despeckle(film, p)
    assert out.dtype == np.float32 and out.shape == film.shape and out[7, 9].max() < 1.0 and same_bits(np.delete(out.reshape(-1, 3), 7 * w + 9, 0), np.delete(film.reshape(-1, 3), 7 * w + 9, 0))
    full = yk.despeckle(film, p, return_mask=True)
    assert isinstance(full, tuple) and same_bits(full[0], out) and full[1].dtype == np.uint8 and full[1].shape == (h, w) and full[2] == (1, 0)
    # a film of sums with its table comes out as a film of sums
    td = 16
    samples = np.full((-(-w // td)) * (-(-h // td)), 4, np.uint32)
    sums = yk.despeckle(film * F(4), p, tile_dim=td, samples=samples)
    assert np.allclose(sums, out * F(4), rtol=1e-6)
    # write_output / write_preview: None leaves every byte as it was, a DespeckleParams changes them
    a, b, c = tmp_path / "a.exr", tmp_path / "b.exr", tmp_path / "c.exr"
    yk.write_output(a, film, yk.ToneMapType.Raw)
    yk.write_output(b, film, yk.ToneMapType.Raw, despeckle=None)
    yk.write_output(c, film, yk.ToneMapType.Raw, despeckle=p)
    assert a.read_bytes() == b.read_bytes() != c.read_bytes()
    yk.write_output(tmp_path / "o.exr", out, yk.ToneMapType.Raw)
    assert (tmp_path / "o.exr").read_bytes() == c.read_bytes()  # it is the despeckled film that was written
    yk.write_output(tmp_path / "d.exr", film)
    yk.write_output(tmp_path / "e.exr", film, despeckle=None)
    yk.write_output(tmp_path / "f.exr", film, despeckle=p)
    assert (tmp_path / "d.exr").read_bytes() == (tmp_path / "e.exr").read_bytes() != (tmp_path / "f.exr").read_bytes()
    yk.write_preview(tmp_path / "a.png", film)
    yk.write_preview(tmp_path / "b.png", film, despeckle=None)
    yk.write_preview(tmp_path / "c.png", film, despeckle=p)
    assert (tmp_path / "a.png").read_bytes() == (tmp_path / "b.png").read_bytes() != (tmp_path / "c.png").read_bytes()
    with pytest.raises(TypeError):
        yk.write_output(c, film, despeckle=yk.RectifyParams())


def test_rule_program_under_the_host_sanitizers(tmp_path):
    """tests/cpp/despeckle_rule.cpp, a program of its own over the rule's header, compiled for the host with
    AddressSanitizer and UBSan (host code only: each sanitizer option goes to the host compilation alone) and run as that
    program."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "despeckle_rule"
    csrc = os.path.join(ROOT, "yuki_amd", "csrc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I", csrc]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "cpp", "despeckle_rule.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "bad = 0" in r.stdout.splitlines()[-1] and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-2000:])


# ------------------------------------------------------------------ quality
# Per scene: frames k = 1 .. 8 of 4 spp (Path depth 8, Uniform, seeds SEED + 977 k) and a 1024-spp film (seed SEED ^ 0x1234567)
# from the oracle, as tests/test_denoise.py and tests/test_rectify.py render theirs.  The error is quality_error against the
# 1024-spp film.  "raw": the mean of the eight frames; "despeckled": the mean of the eight frames, each despeckled.  The
# conditions are asserted at the defaults the sweep chose (tools/despeckle_quality.py, profiles/despeckle_quality.json);
# every bound is the midpoint of 1 and the ratio e_despeckled / e_raw the host instance measured, written beside it.
DEFAULTS = dict(radius=2, rank=3, gain=1.5)
QUALITY = dict(depth=8, noisy_spp=4, converged_spp=1024, frames=8, denoise_frames=3, iterations=3, sigma_color=4.0, sigma_normal=0.3, sigma_plane=0.06)
QUALITY_SCENES = {"cornell": (48, 48), "city-small": (64, 36), "glass-balls": (48, 48)}
# scene -> bound: measured 0.92048 (0.09924 / 0.10781), 0.91687 (0.03588 / 0.03914) and 0.92346 (0.11521 / 0.12476) at DEFAULTS
# (profiles/despeckle_quality.json, "chosen_ratio" and "chosen_bound")
MEAN_BOUNDS = {"cornell": 0.9602, "city-small": 0.9584, "glass-balls": 0.9617}


@functools.lru_cache(maxsize=None)
def oracle_films(name):
    """(frames, converged film, guides) of one scene, rendered by the oracle once."""
    from oracle import binding as oracle
    from yuki_amd import core as yk

    q = QUALITY
    sd = scenes.by_name(name)
    fs = yk.FilmSettings(res=QUALITY_SCENES[name], tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    osc = oracle.OracleScene(sd)
    integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, q["depth"], 0, 0.0)
    render = lambda spp, seed: yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, spp, 1, 1, seed), integ, tiles, n_threads=0)[0], fs.res)  # noqa: E731
    frames = [render(q["noisy_spp"], SEED + 977 * k) for k in range(1, q["frames"] + 1)]
    return frames, render(q["converged_spp"], SEED ^ 0x1234567), oracle_guides(oracle, osc, cam, fs.res)


def mean_errors(yk, frames, conv, params, ctx=None):
    """(e_raw, e_despeckled, clamped pixels per frame, luminance kept per frame) of the mean of the frames."""
    out, n_clamped, kept = [], [], []
    for f in frames:
        g, _, counts = yk.despeckle(f, params, ctx=ctx, return_mask=True)
        out.append(g)
        n_clamped.append(counts[0])
        kept.append(float(ref.luminance(g).astype(np.float64).sum() / ref.luminance(f).astype(np.float64).sum()))
    raw = np.mean(np.asarray(frames, np.float64), axis=0)
    des = np.mean(np.asarray(out, np.float64), axis=0)
    return quality_error(raw, conv), quality_error(des, conv), float(np.mean(n_clamped)), float(np.mean(kept))


def denoised_errors(yk, frames, conv, guides, params):
    """The worst of the first three frames by e_despeckled-then-denoised / e_denoised -> (e_denoised, e_both, ratio)."""
    q = QUALITY
    den = yk.DenoiseParams(q["iterations"], q["sigma_color"], q["sigma_normal"], q["sigma_plane"])
    worst = None
    for f in frames[: q["denoise_frames"]]:
        e_plain = quality_error(yk.denoise(f, guides, den), conv)
        e_both = quality_error(yk.denoise(yk.despeckle(f, params), guides, den), conv)
        if worst is None or e_both / e_plain > worst[2]:
            worst = (e_plain, e_both, e_both / e_plain)
    return worst


def bias(yk, conv, params):
    """What the pass does to the 1024-spp film itself: (pixels clamped, luminance kept, quality_error against the film)."""
    g, _, counts = yk.despeckle(conv, params, return_mask=True)
    return counts[0], float(ref.luminance(g).astype(np.float64).sum() / ref.luminance(conv).astype(np.float64).sum()), quality_error(g, conv)


@pytest.mark.parametrize("name", list(QUALITY_SCENES))
def test_quality_of_the_despeckled_mean(yk, oracle, name):
    frames, conv, _ = oracle_films(name)
    e_raw, e_des, n_clamped, kept = mean_errors(yk, frames, conv, yk.DespeckleParams())
    print(f"despeckle quality {name}: raw {e_raw:.4f} despeckled {e_des:.4f} ratio {e_des / e_raw:.4f} bound {MEAN_BOUNDS[name]}; {n_clamped:.1f} pixels clamped and {kept:.3f} of the luminance kept per 4-spp frame")
    n, k, e = bias(yk, conv, yk.DespeckleParams())
    print(f"despeckle bias {name} (printed, not asserted): on the 1024-spp film {n} pixels clamped, {k:.3f} of the luminance kept, error against the film {e:.4f}")
    assert e_des < e_raw, (e_raw, e_des)
    assert e_des <= MEAN_BOUNDS[name] * e_raw, (e_raw, e_des)


def test_quality_of_one_denoised_frame(yk, oracle):
    frames, conv, guides = oracle_films("city-small")
    e_plain, e_both, ratio = denoised_errors(yk, frames, conv, guides, yk.DespeckleParams())
    print(f"despeckle quality city-small, one denoised frame, worst of three seeds: denoised {e_plain:.4f} despeckled then denoised {e_both:.4f} ratio {ratio:.4f}")
    assert ratio <= 1.0, (e_plain, e_both)
