"""An independent numpy float32 restatement of the despeckle pass, written from the statement of the rule in
include/yuki_hip.h (not from yuki_amd/csrc/yk_despeckle.h): one operation per statement, a whole film per step, the
rank-th largest luminance by a sort.  It never calls the product: the sample-table index rule, the normalisation and the
canonical NaN come from the other restatements (tonemap_ref, denoise_ref).  Shared by tests/test_despeckle.py (host
instance) and tests/test_gpu_despeckle.py (device instance), which also take their films from here."""
import functools

import numpy as np

import denoise_ref
import tonemap_ref
from denoise_ref import bits, canon

F = np.float32
INF = float("inf")
SIZES = ((1, 1), (2, 1), (5, 70), (33, 9), (37, 23), (64, 36), (65, 17))  # (w, h); 65 x 17 crosses a 32 x 8 block with its halo
RADII = (1, 2)
RANKS = (1, 2, 3, 4)
GAINS = (1.0, 2.0, INF)
UNTOUCHED, CLAMPED, REPAIRED = 0, 1, 2


def luminance(c):
    with np.errstate(all="ignore"):
        pr, pg, pb = F(0.2126) * c[..., 0], F(0.7152) * c[..., 1], F(0.0722) * c[..., 2]
        return canon(((pr + pg).astype(np.float32) + pb).astype(np.float32))


def _neighbours(a, r, fill):
    """The (2r + 1)^2 - 1 shifted copies of `a` (h, w, ...) around each pixel, without the pixel, in row-major order;
    outside the film: `fill`."""
    h, w = a.shape[:2]
    pad = np.full((h + 2 * r, w + 2 * r) + a.shape[2:], fill, a.dtype)
    pad[r : r + h, r : r + w] = a
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx or dy:
                yield pad[r + dy : r + dy + h, r + dx : r + dx + w]


def despeckle(film, radius, rank, gain, min_taps=3, floor=0.0, repair=False, tile_dim=16, samples=None):
    """(h, w, 3) film -> (film, (h, w) uint8 mask, (clamped, repaired)); bit patterns of copied values are kept."""
    with np.errstate(all="ignore"):
        film = np.ascontiguousarray(film, np.float32)
        h, w = film.shape[:2]
        if samples is None:
            m = np.ones((h, w), np.float32)
            c = film.copy()
        else:
            m = tonemap_ref.sample_counts(h, w, tile_dim, samples)
            c = denoise_ref.normalise(film, tile_dim, samples)
        finite = np.isfinite(c).all(-1)
        ok = (m != F(0)) & finite
        lum = luminance(c)
        c_taps = list(_neighbours(c, radius, F(0)))
        ok_taps = list(_neighbours(ok, radius, False))
        l_taps = list(_neighbours(lum, radius, F(0)))
        S = np.zeros((h, w, 3), np.float32)
        k = np.zeros((h, w), np.int64)
        for cq, take in zip(c_taps, ok_taps):
            S = np.where(take[..., None], (S + cq).astype(np.float32), S)
            k = k + take
        ranked = np.sort(np.stack([np.where(take, lq, F(-np.inf)) for lq, take in zip(l_taps, ok_taps)]), axis=0)[::-1]
        v = ranked[rank - 1] if rank <= len(l_taps) else np.full((h, w), F(-np.inf))
        v = np.where(v > F(0), v, F(0)).astype(np.float32)
        gain, floor = F(gain) + F(0), F(floor) + F(0)  # a -0 is taken as +0
        bound = (gain * v).astype(np.float32)
        bound = np.where(bound < floor, floor, bound).astype(np.float32)
        live = (m != F(0)) & (k >= max(min_taps, rank)) & ~np.isnan(bound)

        clamp = live & finite & (lum > bound)
        s = (bound / np.where(clamp, lum, F(1))).astype(np.float32)
        clamped = (film * s[..., None]).astype(np.float32)
        fix = live & ~finite & bool(repair)
        mean = canon((S / np.maximum(k, 1).astype(np.float32)[..., None]).astype(np.float32))
        if samples is not None:
            mean = canon((mean * m[..., None]).astype(np.float32))

        out = film.copy()
        ob = out.view(np.uint32)
        ob[clamp] = bits(clamped)[clamp]
        ob[fix] = bits(mean)[fix]
        mask = np.zeros((h, w), np.uint8)
        mask[clamp] = CLAMPED
        mask[fix] = REPAIRED
        assert np.all((s[clamp] >= 0) & (s[clamp] < 1))
        return out, mask, (int(clamp.sum()), int(fix.sum()))


# ------------------------------------------------------------------ the films of both suites
def make_film(rng, w, h):
    """A noisy positive two-tone picture with fireflies, and with NaN, +-inf, -0, negative channels, 1e30 and 3e38 (finite
    as it stands, +inf once a film of sums has multiplied it by 4) sprinkled in."""
    y, x = np.mgrid[0:h, 0:w]
    base = np.where((x * 2 > w)[..., None], F(0.8), F(0.3)) + F(0.1) * np.sin(y / F(3.0))[..., None].astype(np.float32)
    film = np.abs(base + rng.standard_normal((h, w, 3)).astype(np.float32) * F(0.2)).astype(np.float32)
    fly = rng.random((h, w)) < 0.03
    film[fly] = (film[fly] * rng.uniform(5, 200, size=(int(fly.sum()), 1))).astype(np.float32)
    pool = np.array([np.nan, np.inf, -np.inf, -0.0, 1e30, 3e38, 0.0], dtype=np.float32)
    pick = rng.random((h, w, 3)) < 0.02
    film[pick] = pool[rng.integers(0, len(pool), size=int(pick.sum()))]
    neg = rng.random((h, w, 3)) < 0.03
    film[neg] = -np.abs(film[neg])
    dark = rng.random((h, w)) < 0.01  # a neighbourhood's darkest: all three channels negative
    film[dark] = -np.abs(np.where(np.isfinite(film[dark]), film[dark], F(1)))
    return film


@functools.lru_cache(maxsize=None)
def cases():
    """(name, film, tile_dim, samples): every size without a table, with one of tile_dim 16, and with one of tile_dim 7;
    the tables hold zeros.  Every film also holds signalling NaNs with a payload."""
    rng = np.random.default_rng(20261021)
    out = []
    for w, h in SIZES:
        film = make_film(rng, w, h)
        for td in (None, 16, 7):
            samples = None if td is None else denoise_ref.make_samples(rng, w, h, td)
            if samples is not None and len(samples) > 1:
                samples[0] = 0
            with np.errstate(all="ignore"):
                f = film.copy() if samples is None else (film * F(4)).astype(np.float32)  # with a table: a film of sums
            f.reshape(-1).view(np.uint32)[::29] = 0x7FA12345
            out.append((f"{w}x{h}-td{td}", f, td or 16, samples))
    return out


def matrix():
    """(case, radius, rank, repair, gain, min_taps, floor): what both suites walk.  min_taps is the default 3 (raised to the
    rank) without repair and the rank itself with it; the floor is 0 except under tile_dim 7."""
    for case in cases():
        for radius in RADII:
            for rank in RANKS:
                for repair in (False, True):
                    for gain in GAINS:
                        yield case, radius, rank, repair, gain, (rank if repair else max(3, rank)), (0.25 if case[0].endswith("td7") else 0.0)
