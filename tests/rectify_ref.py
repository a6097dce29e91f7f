"""An independent numpy float32 restatement of history rectification (the rule of yuki_amd/csrc/yk_rectify.h, written from
its statement in include/yuki_hip.h), one operation per statement, a whole film per step.  It never calls the product: the
sample-table index rule, the normalisation and the canonical NaN come from the other restatements (tonemap_ref,
denoise_ref).  Shared by tests/test_rectify.py (host instance) and tests/test_gpu_rectify.py (device instance), which also
take their films, histories and moments from here."""
import functools

import numpy as np

import denoise_ref
import temporal_ref
import tonemap_ref
from denoise_ref import bits, canon

F = np.float32
HISTORY_DTYPE = temporal_ref.HISTORY_DTYPE
MOMENTS_DTYPE = np.dtype([("m1", "<f4"), ("m2", "<f4"), ("frames", "<f4"), ("n", "<f4")])
SIZES = temporal_ref.SIZES
RADII = (1, 2, 3)


def _windows(a, r, fill):
    """The (2r + 1)^2 shifted copies of `a` (h, w, ...) in tap order (dy outer, dx inner); outside the film: `fill`."""
    h, w = a.shape[:2]
    pad = np.full((h + 2 * r, w + 2 * r) + a.shape[2:], fill, a.dtype)
    pad[r : r + h, r : r + w] = a
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            yield pad[r + dy : r + dy + h, r + dx : r + dx + w]


def present(rec4):
    """A record (h, w, 4) is present: n > 0 (a NaN is not) and the three other fields finite."""
    return (rec4[..., 3] > F(0)) & np.isfinite(rec4[..., :3]).all(-1)


def rectify(history, film, radius, gamma, tile_dim=16, samples=None, moments=None):
    """(h, w) HISTORY_DTYPE, (h, w, 3) film -> the rectified history, or (history, moments) with (h, w) MOMENTS_DTYPE
    moments; bit patterns of copied values are kept."""
    out, out_m, _, _ = _rectify(history, film, radius, gamma, tile_dim, samples, moments)
    return out if moments is None else (out, out_m)


def factors(history, film, radius, gamma, tile_dim=16, samples=None):
    """(clipped (h, w) bool, f (h, w) float32): which pixels the rule clips and by what factor it scales their count."""
    _, _, clipped, f = _rectify(history, film, radius, gamma, tile_dim, samples, None)
    return clipped, f


def _rectify(history, film, radius, gamma, tile_dim, samples, moments):
    with np.errstate(all="ignore"):
        film = np.asarray(film, np.float32)
        h, w = film.shape[:2]
        if samples is None:
            m = np.ones((h, w), np.float32)
            c = film.copy()
        else:
            m = tonemap_ref.sample_counts(h, w, tile_dim, samples)
            c = denoise_ref.normalise(film, tile_dim, samples)
        ok = (m != F(0)) & np.isfinite(c).all(-1)
        c_taps = list(_windows(c, radius, F(0)))
        ok_taps = list(_windows(ok, radius, False))
        S = np.zeros((h, w, 3), np.float32)
        k = np.zeros((h, w), np.int64)
        for cq, take in zip(c_taps, ok_taps):
            S = np.where(take[..., None], (S + cq).astype(np.float32), S)
            k = k + take
        kf = np.maximum(k, 1).astype(np.float32)[..., None]
        mu = (S / kf).astype(np.float32)
        V = np.zeros((h, w, 3), np.float32)
        for cq, take in zip(c_taps, ok_taps):
            d = (cq - mu).astype(np.float32)
            dd = (d * d).astype(np.float32)
            V = np.where(take[..., None], (V + dd).astype(np.float32), V)
        var = (V / kf).astype(np.float32)
        sigma = np.sqrt(var).astype(np.float32)
        e = (F(gamma) * sigma).astype(np.float32)
        lo = (mu - e).astype(np.float32)
        hi = (mu + e).astype(np.float32)

        rec = np.zeros((h, w, 4), np.float32)
        rec.view(np.uint32)[..., :3] = bits(history["rgb"])
        rec.view(np.uint32)[..., 3] = bits(history["n"])
        hr, hn = rec[..., :3], rec[..., 3]
        live = present(rec) & (k >= 2) & np.isfinite(mu).all(-1) & np.isfinite(e).all(-1)
        below, above = hr < lo, hr > hi
        out_of_box = below | above
        clipped = live & out_of_box.any(-1)
        moved = np.where(below, lo, np.where(above, hi, hr))
        dist = np.abs((hr - mu).astype(np.float32))
        fc = np.where(out_of_box, (e / dist).astype(np.float32), F(1))
        f = np.ones((h, w), np.float32)
        for ch in range(3):
            f = np.where(fc[..., ch] < f, fc[..., ch], f)
        n1 = canon(hn * f)

        out = rec.copy()
        ob = out.view(np.uint32)
        ob[..., :3][clipped] = bits(moved)[clipped]
        ob[..., 3][clipped] = bits(n1)[clipped]
        o = np.zeros((h, w), HISTORY_DTYPE)
        o["rgb"] = out[..., :3]
        o["n"] = out[..., 3]
        assert np.array_equal(bits(o["rgb"]), ob[..., :3])  # the structured copy kept every payload

        om = None
        if moments is not None:
            mr = np.zeros((h, w, 4), np.float32)
            for j, name in enumerate(("m1", "m2", "frames", "n")):
                mr.view(np.uint32)[..., j] = bits(moments[name])
            touch = clipped & present(mr)
            mo = mr.copy()
            mb = mo.view(np.uint32)
            mb[..., 2][touch] = bits(canon(mr[..., 2] * f))[touch]
            mb[..., 3][touch] = bits(n1)[touch]
            om = np.zeros((h, w), MOMENTS_DTYPE)
            for j, name in enumerate(("m1", "m2", "frames", "n")):
                om[name] = mo[..., j]
        return o, om, clipped, np.where(clipped, f, F(1)).astype(np.float32)


# ------------------------------------------------------------------ the films, histories and moments of both suites
def make_moments(rng, w, h, history):
    """Moments beside `history`: the same counts on most pixels (as the blends keep them), plus absent and odd records."""
    m = np.zeros((h, w), MOMENTS_DTYPE)
    m["m1"] = rng.random((h, w)).astype(np.float32)
    m["m2"] = (m["m1"] * m["m1"] + rng.random((h, w)).astype(np.float32) * F(0.1)).astype(np.float32)
    m["frames"] = rng.integers(1, 20, size=(h, w)).astype(np.float32)
    m["n"] = history["n"]
    pool = np.array([np.nan, np.inf, -np.inf, -0.0, 1e30, 0.0], np.float32)
    for name in ("m1", "m2", "frames", "n"):
        pick = rng.random((h, w)) < 0.05
        m[name][pick] = pool[rng.integers(0, len(pool), size=int(pick.sum()))]
    return m


@functools.lru_cache(maxsize=None)
def cases():
    """(name, film, tile_dim, samples, history, moments): every film size with and without a sample table (tile_dim 16, and
    7 on sizes that are no multiple of it; the tables hold zeros).  Films and histories carry NaN, +-inf, -0 and 1e30, the
    counts 0, -3, NaN and +inf (temporal_ref.make_history); the film also holds a signalling NaN with a payload."""
    rng = np.random.default_rng(20261021)
    out = []
    for w, h in SIZES:
        film = denoise_ref.make_film(rng, w, h)
        hist = temporal_ref.make_history(rng, w, h)
        hist["rgb"].reshape(-1).view(np.uint32)[5::31] = 0x7FA54321  # absent records with a payload: copied as they are
        mom = make_moments(rng, w, h, hist)
        for td in (None, 16, 7):
            samples = None if td is None else temporal_ref.make_samples(rng, w, h, td)
            if samples is not None and w * h > 1:
                samples[0] = 0
            # with a table the film is a film of sums: scale it so that the normalised film stays near the histories
            f = film.copy() if samples is None else (film * F(4)).astype(np.float32)
            f.reshape(-1).view(np.uint32)[::29] = 0x7FA12345
            out.append((f"{w}x{h}-td{td}", f, td or 16, samples, hist, mom))
    return out
