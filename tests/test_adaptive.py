"""Adaptive sampling, host instance (yk_adaptive_select / _accumulate / _resolve without a context, csrc/yk_adaptive.h)
against the independent numpy restatement of tests/adaptive_ref.py, bit for bit and in the rule's order; the special
cases of the rule one by one; the refusals; and the quality condition on oracle films: on city-small the adaptive loop
beats uniform passes at equal total samples by the bound profiles/adaptive_quality.json records."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import adaptive_ref as ref
from yuki_amd import abi, scenes

F = np.float32
SEED = 0x73B9642E74AC471C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE = dict(min_samples=16, max_samples=128, round_passes=16, dilate=True, threshold=0.1, epsilon=0.01)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def params(yk, **kw):
    r = dict(RULE)
    r.update(kw)
    return yk.AdaptiveParams(**r)


def ref_select(stats, **kw):
    r = dict(RULE)
    r.update(kw)
    return ref.select(stats, r["min_samples"], r["max_samples"], r["round_passes"], r["dilate"], r["threshold"], r["epsilon"])


def converged(w, h, n=RULE["min_samples"]):
    """Statistics no pixel of which wants anything: n samples that all agreed."""
    s = np.zeros((h, w), dtype=ref.STATS)
    s["n"] = s["drawn"] = n
    s["mean"] = F(1)
    return s


@functools.lru_cache(maxsize=None)
def select_cases():
    """(name, stats, rule overrides): sprinkled statistics on every size with dilate 0 and 1, all selected, none selected."""
    out = []
    for k, (w, h) in enumerate(ref.SIZES):
        s = ref.sprinkled_stats(np.random.default_rng(1000 + k), w, h, RULE["min_samples"], RULE["max_samples"], RULE["round_passes"])
        s.setflags(write=False)
        for dilate in (False, True):
            out.append((f"{w}x{h}-dilate{int(dilate)}", s, dict(dilate=dilate)))
        out.append((f"{w}x{h}-cleared", np.zeros((h, w), dtype=ref.STATS), {}))
        out.append((f"{w}x{h}-converged", converged(w, h), {}))
        capped = np.zeros((h, w), dtype=ref.STATS)  # every pixel wants (n = 0) and none is eligible
        capped["drawn"] = RULE["max_samples"]
        out.append((f"{w}x{h}-at-the-cap", capped, {}))
    return out


@functools.lru_cache(maxsize=None)
def fold_cases():
    """(name, xy, passes (3, n, 3), film_sum, stats): a sprinkled film, a selected list, passes with non-finite values."""
    out = []
    for k, (w, h) in enumerate(ref.SIZES[:3]):
        rng = np.random.default_rng(2000 + k)
        stats = ref.sprinkled_stats(rng, w, h, RULE["min_samples"], RULE["max_samples"], RULE["round_passes"])
        film = (rng.uniform(0.0, 3.0, size=(h, w, 3)) * np.maximum(stats["n"], 1)[..., None]).astype(F)
        xy, _ = ref_select(stats)
        assert len(xy) > 0
        passes = rng.uniform(0.0, 2.0, size=(3, len(xy), 3)).astype(F)
        for v in (ref.CANON, ref.INF, -ref.INF, F(1e30)):
            passes[rng.random(passes.shape) < 0.02] = v
        for a in (xy, passes, film, stats):
            a.setflags(write=False)
        out.append((f"{w}x{h}", xy, passes, film, stats))
    return out


# ------------------------------------------------------------------ select
def test_select_host_equals_restatement(yk):
    seen_some = seen_all = seen_none = False
    for name, stats, kw in select_cases():
        xy, sample = yk.adaptive_select(stats, params(yk, **kw))
        want_xy, want_sample = ref_select(stats, **kw)
        assert same_bits(xy, want_xy) and same_bits(sample, want_sample), name
        seen_all |= len(xy) == stats.size
        seen_none |= len(xy) == 0
        seen_some |= 0 < len(xy) < stats.size
    assert seen_some and seen_all and seen_none


def test_select_order_is_tiles_then_rows(yk):
    """On a cleared 37 x 23 film everything is selected: the list IS the order of the rule."""
    w, h = 37, 23
    xy, sample = yk.adaptive_select(np.zeros((h, w), dtype=ref.STATS), params(yk))
    want = [x | (y << 16) for ty in range(0, h, 16) for tx in range(0, w, 16) for y in range(ty, min(h, ty + 16)) for x in range(tx, min(w, tx + 16))]
    assert xy.tolist() == want and not sample.any()


@pytest.mark.parametrize("size", [(37, 23), (16, 16), (5, 3)])
def test_lone_wanting_pixel_selects_its_in_film_neighbours(yk, size):
    w, h = size
    spots = {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2), (w // 2, h // 2), (min(15, w - 1), min(15, h - 1)), (min(16, w - 1), min(16, h - 1))}
    for px, py in sorted(spots):
        s = converged(w, h)
        s["n"][py, px] = 0
        s["drawn"][py, px] = 0
        got = set(yk.adaptive_select(s, params(yk))[0].tolist())
        want = {x | (y << 16) for y in range(max(0, py - 1), min(h, py + 2)) for x in range(max(0, px - 1), min(w, px + 2))}
        assert got == want, (px, py)
        assert yk.adaptive_select(s, params(yk, dilate=False))[0].tolist() == [px | (py << 16)]
        # a neighbour's want counts although that neighbour is not eligible itself
        s["drawn"][py, px] = RULE["max_samples"]
        assert set(yk.adaptive_select(s, params(yk))[0].tolist()) == want - {px | (py << 16)}, (px, py)


def test_wants_threshold_edge_and_nan(yk):
    """m2 just above / at the right-hand side; a NaN on either side compares false; n < min_samples always wants."""
    s = converged(4, 1, n=20)
    p = RULE
    thr2 = F(p["threshold"]) * F(p["threshold"])
    rhs = (thr2 * ((F(20) - F(1)) * F(20))) * ((F(1) + F(p["epsilon"])) * (F(1) + F(p["epsilon"])))
    s["m2"] = [rhs, np.nextafter(rhs, ref.INF), ref.CANON, rhs]
    s["mean"][0, 3] = ref.CANON
    assert yk.adaptive_select(s, params(yk, dilate=False))[0].tolist() == [1]
    s["n"][0, 2] = p["min_samples"] - 1
    assert yk.adaptive_select(s, params(yk, dilate=False))[0].tolist() == [1, 2]


# ------------------------------------------------------------------ fold
def test_fold_host_equals_restatement(yk):
    for name, xy, passes, film, stats in fold_cases():
        got_f, got_s = film.copy(), stats.copy()
        yk.adaptive_accumulate(xy, passes, got_f, got_s)
        want_f, want_s = ref.fold(xy, passes, film, stats)
        assert same_bits(got_f, want_f) and same_bits(got_s, want_s), name
        untouched = np.ones(stats.shape, dtype=bool)
        untouched[xy >> 16, xy & 0xFFFF] = False
        assert same_bits(got_f[untouched], film[untouched]) and same_bits(got_s[untouched], stats[untouched]), name


def test_fold_three_passes_equal_three_folds_of_one(yk):
    for name, xy, passes, film, stats in fold_cases():
        a_f, a_s = film.copy(), stats.copy()
        yk.adaptive_accumulate(xy, passes, a_f, a_s)
        b_f, b_s = film.copy(), stats.copy()
        for k in range(3):
            yk.adaptive_accumulate(xy, passes[k : k + 1], b_f, b_s)
        assert same_bits(a_f, b_f) and same_bits(a_s, b_s), name


def test_fold_non_finite_samples_only_advance_drawn(yk):
    w, h = 5, 3
    rng = np.random.default_rng(7)
    film = rng.uniform(1.0, 9.0, size=(h, w, 3)).astype(F)
    stats = converged(w, h, n=9)
    stats["m2"] = F(0.25)
    xy = np.array([x | (y << 16) for y in range(h) for x in range(w)], dtype=np.uint32)
    bad = [ref.CANON, ref.INF, -ref.INF, F(1e30), F(-1e30)]  # 1e30: finite, but the square of its luminance is not
    passes = np.full((len(bad) * 3, len(xy), 3), F(0.5))
    for k, v in enumerate(bad):
        for ch in range(3):
            passes[3 * k + ch, :, ch] = v
    f, s = film.copy(), stats.copy()
    yk.adaptive_accumulate(xy, passes, f, s)
    assert same_bits(f, film) and same_bits(s["mean"], stats["mean"]) and same_bits(s["m2"], stats["m2"]) and same_bits(s["n"], stats["n"])
    assert np.all(s["drawn"] == stats["drawn"] + len(passes))


def test_fold_is_welford_in_sample_order(yk):
    rng = np.random.default_rng(11)
    passes = rng.uniform(0.0, 4.0, size=(24, 1, 3)).astype(F)
    f, s = np.zeros((1, 1, 3), dtype=F), np.zeros((1, 1), dtype=ref.STATS)
    yk.adaptive_accumulate(np.zeros(1, dtype=np.uint32), passes, f, s)
    mean, m2 = ref.welford(ref.luminance(passes[:, 0, :]))
    assert same_bits(s["mean"][0, 0], mean) and same_bits(s["m2"][0, 0], m2) and s["n"][0, 0] == 24 and s["drawn"][0, 0] == 24
    want = np.zeros(3, dtype=F)
    for c in passes[:, 0, :]:
        want = want + c
    assert same_bits(f[0, 0], want)
    assert abs(float(m2) / 23 - float(np.var(ref.luminance(passes[:, 0, :]).astype(np.float64), ddof=1))) < 1e-5  # it IS the sample variance


# ------------------------------------------------------------------ resolve
def test_resolve_host_equals_restatement(yk):
    for name, xy, passes, film, stats in fold_cases():
        film2 = film.copy()
        film2[0, 0] = ref.CANON
        film2[-1, -1] = ref.INF
        rgb, var = yk.adaptive_resolve(film2, stats)
        want_rgb, want_var = ref.resolve(film2, stats)
        assert same_bits(rgb, want_rgb) and same_bits(var, want_var), name
        assert not np.isnan(var).any() and (var >= 0).all()
        assert np.all(var[stats["n"] < 2] == ref.INF) and not rgb[stats["n"] == 0].any()


def test_resolved_variance_feeds_the_variance_guided_denoise(yk):
    """adaptive_resolve's variance is the image denoise(..., variance=) takes: +inf (n < 2) switches that pixel's colour stop off."""
    w, h = 16, 12
    rng = np.random.default_rng(5)
    stats = converged(w, h, n=8)
    stats["m2"] = rng.uniform(0.0, 0.5, size=(h, w)).astype(F)
    stats["n"][3, 4] = 1
    film = (rng.uniform(0.2, 0.8, size=(h, w, 3)) * stats["n"][..., None]).astype(F)
    rgb, var = yk.adaptive_resolve(film, stats)
    guides = np.zeros((h, w), dtype=abi.GUIDE_DTYPE)
    out = yk.denoise(rgb, guides, yk.VarianceParams(iterations=2), variance=var)
    assert out.shape == rgb.shape and np.isfinite(out).all() and var[3, 4] == ref.INF


# ------------------------------------------------------------------ refusals
BAD_DESCS = [dict(min_samples=1), dict(min_samples=0), dict(max_samples=15), dict(max_samples=(1 << 24) + 1), dict(round_passes=0), dict(round_passes=0x10000), dict(dilate=2),
             dict(threshold=0.0), dict(threshold=-0.1), dict(threshold=float("nan")), dict(epsilon=-1e-3), dict(epsilon=float("nan"))]  # fmt: skip


@pytest.mark.parametrize("bad", BAD_DESCS, ids=[f"{k}={v}" for d in BAD_DESCS for k, v in d.items()])
def test_descriptor_refusals(yk, bad):
    with pytest.raises(yk.YukiError) as e:
        yk.adaptive_select(np.zeros((3, 5), dtype=ref.STATS), params(yk, **bad))
    assert e.value.status == 1


def test_descriptor_limits_are_accepted(yk):
    s = np.zeros((3, 5), dtype=ref.STATS)
    for ok in (dict(min_samples=2, max_samples=2), dict(max_samples=1 << 24), dict(round_passes=0xFFFF), dict(epsilon=0.0), dict(threshold=float("inf"))):
        yk.adaptive_select(s, params(yk, **ok))


def test_argument_refusals(yk):
    L = yk.lib()
    w, h = 5, 3
    film, stats = np.zeros((h, w, 3), dtype=F), np.zeros((h, w), dtype=ref.STATS)
    one = np.zeros((1, 1, 3), dtype=F)
    for xy in ([5], [3 << 16], [0xFFFF_FFFF]):  # outside the film
        with pytest.raises(yk.YukiError):
            yk.adaptive_accumulate(np.array(xy, dtype=np.uint32), one, film, stats)
    with pytest.raises(yk.YukiError):  # a pixel twice
        yk.adaptive_accumulate(np.array([1, 2, 1], dtype=np.uint32), np.zeros((1, 3, 3), dtype=F), film, stats)
    assert not film.any() and not stats["drawn"].any()
    d = params(yk).as_struct()
    n = C.c_uint32(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.yk_adaptive_select(None, None, vp(stats), w, h, None, None, C.byref(n)) == 1
    assert L.yk_adaptive_select(None, C.byref(d), None, w, h, None, None, C.byref(n)) == 1
    assert L.yk_adaptive_select(None, C.byref(d), vp(stats), 0, h, None, None, C.byref(n)) == 1
    assert L.yk_adaptive_select(None, C.byref(d), vp(stats), w, h, None, None, None) == 1
    assert L.yk_adaptive_select(None, C.byref(d), vp(stats), w, h, None, None, C.byref(n)) == 0 and n.value == w * h  # counting alone is served
    xy = np.zeros(1, dtype=np.uint32)
    assert L.yk_adaptive_accumulate(None, vp(xy), 1, vp(one), 0, w, h, vp(film), vp(stats)) == 1  # no passes
    assert L.yk_adaptive_accumulate(None, vp(xy), 1, None, 1, w, h, vp(film), vp(stats)) == 1
    both = np.zeros(w * h * 7, dtype=F)  # film and statistics that share bytes
    assert L.yk_adaptive_accumulate(None, vp(xy), 1, vp(one), 1, w, h, vp(both), vp(both[w * h :])) == 1
    assert L.yk_adaptive_resolve(None, vp(film), vp(stats), w, h, None, None) == 1  # nothing asked for
    assert L.yk_adaptive_resolve(None, vp(film), vp(stats), w, h, vp(film), None) == 1  # the output is the input
    out = np.zeros(w * h * 4, dtype=F)
    assert L.yk_adaptive_resolve(None, vp(film), vp(stats), w, h, vp(out), vp(out[w * h * 2 :])) == 1  # the two outputs overlap
    assert L.yk_adaptive_resolve(None, vp(film), vp(stats), w, h, vp(out), vp(out[w * h * 3 :])) == 0
    assert L.yk_pixel_list_create(None, w, h, C.byref(C.c_void_p())) == 1 and L.yk_pixel_list_set(None, None, None, 0, 1) == 1
    assert L.yk_render_adaptive_device(None, None, None, None, None, C.byref(d), w, h, None, None, None, None, None, None) == 1


def test_params_for_sampler(yk):
    p = yk.AdaptiveParams.for_sampler(yk.SamplerType.Stratified((4, 4)))
    assert p.max_samples == 16 and yk.AdaptiveParams.for_sampler(yk.SamplerType.Uniform(128)).max_samples == 128
    with pytest.raises(ValueError):
        yk.AdaptiveParams().as_struct()
    assert C.sizeof(abi.AdaptiveDesc) == 28 and abi.PIXEL_STATS_DTYPE.itemsize == 16 and C.sizeof(abi.AdaptiveInfo) == 40


# ------------------------------------------------------------------ quality on oracle films (city-small only)
QUALITY = dict(scene="city-small", res=(64, 36), depth=8, spp=128, converged_spp=1024)


def quality_bound():
    with open(os.path.join(ROOT, "profiles", "adaptive_quality.json")) as f:
        return float(json.load(f)["bound"])


@functools.lru_cache(maxsize=None)
def oracle_passes():
    """(passes (spp, h * w, 3): accumulating pass k of the whole film as one tile, row-major; the 1024-spp film), by the oracle."""
    from oracle import binding as oracle
    from yuki_amd import core as yk

    q = QUALITY
    sd = scenes.by_name(q["scene"])
    fs = yk.FilmSettings(res=q["res"], tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    osc = oracle.OracleScene(sd)
    integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, q["depth"], 0, 0.0)
    smp = abi.SamplerDesc(abi.SAMPLER_UNIFORM, q["spp"], 1, 1, SEED)
    film = np.array([(0, 0, q["res"][0], q["res"][1])], dtype=abi.TILE_DTYPE)
    passes = np.stack([osc.render_tiles_accumulating(cam.matrices, smp, integ, film, [k], n_threads=0)[0] for k in range(q["spp"])])
    tiles = yk.film_tiles(fs)
    conv = yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, q["converged_spp"], 1, 1, SEED ^ 0x1234567), integ, tiles, n_threads=0)[0], fs.res)
    passes.setflags(write=False)
    return passes, conv


def adaptive_loop(yk, passes, res, p, ctx=None, lists=None):
    """The driver's loop with the entry points of `ctx` (None: the host instance) over passes rendered beforehand:
    passes[k][y * w + x] is sample k of the pixel.  -> (film_sum, stats, rounds)."""
    w, h = res
    film, stats = np.zeros((h, w, 3), dtype=F), np.zeros((h, w), dtype=ref.STATS)
    rounds = 0
    while True:
        xy, sample = yk.adaptive_select(stats, p, ctx=ctx)
        if lists is not None:
            lists.append((xy, sample))
        if len(xy) == 0 or (p.max_rounds and rounds == p.max_rounds):
            return film, stats, rounds
        pix = (xy >> 16).astype(np.int64) * w + (xy & 0xFFFF)
        got = np.stack([passes[sample + k, pix] for k in range(p.round_passes)])
        yk.adaptive_accumulate(xy, got, film, stats, ctx=ctx)
        rounds += 1


def quality_check(yk, passes, conv, p, ctx=None):
    """(e_adaptive, e_uniform at ceil(mean spp), mean spp, rounds, fraction of pixels at the cap)"""
    from test_denoise import quality_error

    w, h = QUALITY["res"]
    film, stats, rounds = adaptive_loop(yk, passes, (w, h), p, ctx=ctx)
    rgb, _ = yk.adaptive_resolve(film, stats, ctx=ctx)
    total = int(stats["drawn"].sum())
    k = -(-total // (w * h))
    uniform = passes[:k].astype(np.float64).sum(0).reshape(h, w, 3) / k
    return quality_error(rgb, conv), quality_error(uniform, conv), total / (w * h), rounds, float((stats["drawn"] >= p.max_samples).mean())


def test_quality_on_oracle_films(yk):
    passes, conv = oracle_passes()
    p = yk.AdaptiveParams.for_sampler(yk.SamplerType.Uniform(QUALITY["spp"]))
    e_ad, e_un, mean_spp, rounds, capped = quality_check(yk, passes, conv, p)
    bound = quality_bound()
    print(f"adaptive quality: {rounds} rounds, mean spp {mean_spp:.1f}, {100 * capped:.0f} % at the cap, adaptive {e_ad:.4f} uniform {e_un:.4f} ratio {e_ad / e_un:.3f} bound {bound}")
    assert mean_spp < QUALITY["spp"]
    assert e_ad < e_un, (e_ad, e_un)
    assert bound < 1 and e_ad <= bound * e_un, (e_ad, e_un, bound)
