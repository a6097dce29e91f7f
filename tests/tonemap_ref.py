"""An independent numpy float32 restatement of the tone map (app/renderpasses/tonemap.rs; the rules of
yuki_amd/csrc/yk_tonemap.h), one operation per statement.  It never calls the product.  Shared by
tests/test_tonemap.py (host instance) and tests/test_gpu_tonemap.py (device instance)."""
import numpy as np

F = np.float32
FLT_MAX = F(3.4028235e38)

M_IN = [(F(0.59719), F(0.35458), F(0.04823)), (F(0.07600), F(0.90834), F(0.01566)), (F(0.02840), F(0.13383), F(0.83777))]
M_OUT = [(F(1.60475), F(-0.53108), F(-0.07367)), (F(-0.10208), F(1.10813), F(-0.00605)), (F(-0.00327), F(-0.07276), F(1.07602))]


def saturate(x):
    inner = np.where(x < F(1), x, F(1))
    return np.where(x > F(0), inner, F(0)).astype(np.float32)


def luminance(r, g, b):
    a = F(0.2126) * r
    c = F(0.7152) * g
    s = a + c
    d = F(0.0722) * b
    return s + d


def fit(v):
    t = v + F(0.0245786)
    a = v * t
    a = a - F(0.000090537)
    u = F(0.983729) * v
    u = u + F(0.4329510)
    b = v * u
    b = b + F(0.238081)
    return a / b


def row(m, r, g, b):
    x = m[0] * r
    y = m[1] * g
    s = x + y
    z = m[2] * b
    return s + z


def sample_counts(h, w, tile_dim, samples):
    """(float)samples[flat] per pixel, flat = (y / td) * (w / td, floor) + x / td."""
    y, x = np.mgrid[0:h, 0:w]
    flat = (y // tile_dim) * (w // tile_dim) + x // tile_dim
    return np.asarray(samples, dtype=np.uint32)[flat].astype(np.float32)


def filmic(film, exposure=1.0, tile_dim=16, samples=None):
    with np.errstate(all="ignore"):
        film = np.asarray(film, dtype=np.float32)
        r, g, b = film[..., 0], film[..., 1], film[..., 2]
        if samples is not None:
            n = sample_counts(film.shape[0], film.shape[1], tile_dim, samples)
            pos = n > F(0)
            safe = np.where(pos, n, F(1))
            r = np.where(pos, r / safe, r)
            g = np.where(pos, g / safe, g)
            b = np.where(pos, b / safe, b)
        e = F(exposure)
        r = r * e
        g = g * e
        b = b * e
        i = [fit(row(m, r, g, b)) for m in M_IN]
        o = [saturate(row(m, i[0], i[1], i[2])) for m in M_OUT]
        return np.stack(o, axis=-1).astype(np.float32)


def heat_value(film, channel):
    """texel[channel] for 1 / 2, luminance for 0 AND 3 (the shader's `channel > 0 && channel < 3`)."""
    if channel in (1, 2):
        return film[..., channel]
    return luminance(film[..., 0], film[..., 1], film[..., 2])


def mix(x, y, a):
    w = F(1) - a
    p = x * w
    q = y * a
    return p + q


def heatmap(film, lo, hi, channel=0):
    with np.errstate(all="ignore"):
        film = np.asarray(film, dtype=np.float32)
        v = heat_value(film, channel)
        num = v - F(lo)
        den = F(hi) - F(lo)
        s = num / den
        s2x = s * F(2)
        s1 = saturate(s2x)
        s2 = saturate(s2x - F(1))
        low, mid, high = (F(0), F(0), F(1)), (F(0), F(1), F(0)), (F(1), F(0), F(0))
        out = [mix(mix(low[k], mid[k], s1), high[k], s2) for k in range(3)]
        return np.stack(out, axis=-1).astype(np.float32)


def min_max(film, channel):
    """find_min_max: the fold from (f32::MAX, f32::MIN) skipping NaN pixels (min / max are exact: the fold's value)."""
    with np.errstate(all="ignore"):
        film = np.asarray(film, dtype=np.float32)
        v = luminance(film[..., 0], film[..., 1], film[..., 2]) if channel == 3 else film[..., channel]
        v = v[~np.isnan(v)]
        lo, hi = FLT_MAX, -FLT_MAX
        if v.size:
            lo = min(lo, F(v.min()))
            hi = max(hi, F(v.max()))
        return F(lo), F(hi)


def random_film(rng, h, w, specials=True):
    """Signed values over many magnitudes; with `specials`, also +-0, subnormals, huge values, +-inf and NaN."""
    mag = np.float32(10.0) ** rng.uniform(-6, 6, size=(h, w, 3)).astype(np.float32)
    film = (rng.standard_normal((h, w, 3)).astype(np.float32) * mag).astype(np.float32)
    if specials:
        pool = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45, 1e18, 1e19, 2e19, 3e38, -3e38, np.inf, -np.inf, np.nan, 1.0, -1.0], dtype=np.float32)
        pick = rng.random((h, w, 3)) < 0.15
        film[pick] = pool[rng.integers(0, len(pool), size=int(pick.sum()))]
    return film


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
