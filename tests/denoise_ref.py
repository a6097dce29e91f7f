"""An independent numpy float32 restatement of the denoiser (the rules of yuki_amd/csrc/yk_denoise.h), one operation per
statement, a whole film per tap.  It never calls the product; `exp` is handed in (the oracle's libm_array).  Shared by
tests/test_denoise.py (host instance) and tests/test_gpu_denoise.py (device instance), which also take their films,
guides and parameter sets from here."""
import numpy as np

import tonemap_ref

F = np.float32
K = (F(0.375), F(0.25), F(0.0625))  # k[|offset|] = 3/8, 1/4, 1/16
GUIDE_DTYPE = np.dtype([("ns", "<f4", 3), ("hit", "<f4"), ("p", "<f4", 3), ("t", "<f4")])
QNAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def canon(a):
    """A NaN an operation produced is 0x7fc00000."""
    a = np.asarray(a, dtype=np.float32).copy()
    a.view(np.uint32)[np.isnan(a)] = 0x7FC00000
    return a


def dot(ax, ay, az, bx, by, bz):
    """The library's dot: ((0 + x*x') + y*y') + z*z'."""
    s = F(0) + ax * bx
    s = s + ay * by
    return s + az * bz


def normalise(film, tile_dim, samples):
    """Each channel divided by (float)samples[flat] where that count is > 0; everything else keeps its bits."""
    film = np.asarray(film, dtype=np.float32)
    if samples is None:
        return film.copy()
    n = tonemap_ref.sample_counts(film.shape[0], film.shape[1], tile_dim, samples)
    pos = n > F(0)
    safe = np.where(pos, n, F(1))[..., None]
    out = film.copy()
    with np.errstate(all="ignore"):
        q = canon(film / safe)
    m = np.broadcast_to(pos[..., None], film.shape)
    out.view(np.uint32)[m] = q.view(np.uint32)[m]
    return out


def _window(n, off):
    """The pixels P of an axis of length n whose tap P + off lies inside: (start, stop), possibly empty."""
    return max(0, -off), min(n, n - off)


def iteration(c, guides, i, sigma_color, sigma_normal, sigma_plane, exp):
    h, w = c.shape[0], c.shape[1]
    s = 1 << i
    sc = F(sigma_color) / F(1 << i)
    den_c = sc * sc
    den_n = F(sigma_normal) * F(sigma_normal)
    den_p = F(sigma_plane) * F(sigma_plane)
    ns, hit, p = guides["ns"], guides["hit"] != F(0), guides["p"]
    acc = np.zeros((h, w, 3), np.float32)
    wsum = np.zeros((h, w), np.float32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            y0, y1 = _window(h, s * dy)
            x0, x1 = _window(w, s * dx)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
            hk = K[abs(dx)] * K[abs(dy)]
            cq = c[Q]
            if dx == 0 and dy == 0:
                wt = np.full(cq.shape[:2], hk, np.float32)
                take = np.ones(cq.shape[:2], bool)
            else:
                d = c[P] - cq
                rr = d[..., 0] * d[..., 0]
                gg = d[..., 1] * d[..., 1]
                bb = d[..., 2] * d[..., 2]
                a_c = ((rr + gg) + bb) / den_c
                n = ns[P] - ns[Q]
                a_n = dot(n[..., 0], n[..., 1], n[..., 2], n[..., 0], n[..., 1], n[..., 2]) / den_n
                v = p[Q] - p[P]
                dist = dot(ns[P][..., 0], ns[P][..., 1], ns[P][..., 2], v[..., 0], v[..., 1], v[..., 2])
                a_p = (dist * dist) / den_p
                both = hit[P] & hit[Q]
                a_n = np.where(both, a_n, F(0))
                a_p = np.where(both, a_p, F(0))
                e = (a_c + a_n) + a_p
                x = exp((-e).astype(np.float32)).reshape(e.shape)
                wt = (hk * x).astype(np.float32)
                wt = np.where(hit[P] != hit[Q], F(0), wt)
                take = ~((wt == F(0)) | np.isnan(wt))
            prod = wt[..., None] * cq
            acc[P] = np.where(take[..., None], acc[P] + prod, acc[P])
            wsum[P] = np.where(take, wsum[P] + wt, wsum[P])
    return canon(acc / wsum[..., None])


def denoise(film, guides, iterations, sigma_color, sigma_normal, sigma_plane, exp, tile_dim=16, samples=None):
    """(h, w, 3) float32 film, (h, w) GUIDE_DTYPE guides -> the denoised film."""
    with np.errstate(all="ignore"):
        c = normalise(film, tile_dim, samples)
        for i in range(iterations):
            c = iteration(c, guides, i, sigma_color, sigma_normal, sigma_plane, exp)
        return c


# ------------------------------------------------------------------ the films, guides and parameter sets of both suites
SIZES = ((1, 1), (5, 3), (37, 23), (64, 36), (130, 70))  # (w, h)
ITERATIONS = (0, 1, 3, 5, 8)
SIGMAS = (4.0, 0.3, 0.06)  # colour, normal, plane
INF = float("inf")


def make_film(rng, w, h):
    """A noisy two-tone picture with NaN, +-inf, -0 and 1e30 pixels sprinkled in."""
    y, x = np.mgrid[0:h, 0:w]
    base = np.where((x * 2 > w)[..., None], F(0.8), F(0.2)) + F(0.1) * np.sin(y / F(3.0))[..., None].astype(np.float32)
    film = (base + rng.standard_normal((h, w, 3)).astype(np.float32) * F(0.25)).astype(np.float32)
    pool = np.array([np.nan, np.inf, -np.inf, -0.0, 1e30, -1e30, 0.0], dtype=np.float32)
    pick = rng.random((h, w, 3)) < 0.03
    film[pick] = pool[rng.integers(0, len(pool), size=int(pick.sum()))]
    return film


def make_guides(rng, w, h):
    """Two planes that meet in a crease, a slanted floor strip, and miss regions (a corner block and scattered pixels)."""
    y, x = np.mgrid[0:h, 0:w]
    g = np.zeros((h, w), GUIDE_DTYPE)
    left = x * 2 <= w
    n = np.where(left[..., None], np.array([0.6, 0.0, 0.8], np.float32), np.array([-0.6, 0.0, 0.8], np.float32)).astype(np.float32)
    n = n + rng.standard_normal((h, w, 3)).astype(np.float32) * F(0.02)
    n = n / np.sqrt((n * n).sum(-1, keepdims=True)).astype(np.float32)
    px = (x / F(16.0)).astype(np.float32)
    py = (y / F(16.0)).astype(np.float32)
    pz = (np.abs(x - w / 2.0) * 0.045).astype(np.float32) + rng.standard_normal((h, w)).astype(np.float32) * F(0.002)
    hit = np.ones((h, w), bool)
    hit[: max(h // 4, 1) - (1 if h == 1 else 0), (3 * w) // 4 :] = False
    hit &= rng.random((h, w)) > 0.05
    g["ns"] = np.where(hit[..., None], n, F(0))
    g["hit"] = hit.astype(np.float32)
    g["p"] = np.where(hit[..., None], np.stack([px, py, pz], -1), F(0))
    g["t"] = np.where(hit, F(3.0) + pz, F(0))
    return g


def make_samples(rng, w, h, tile_dim):
    n = (-(-w // tile_dim)) * (-(-h // tile_dim))
    t = rng.integers(1, 9, size=n).astype(np.uint32)
    t[rng.random(n) < 0.2] = 0  # a tile no pass has reached yet: its pixels keep their bits
    return t


def cases():
    """(name, film, guides, iterations, (sigma_color, sigma_normal, sigma_plane), tile_dim, samples): every film size under
    every iteration count, a sample table with tile_dim 16 on a resolution that is no multiple of 16, each sigma at +inf."""
    rng = np.random.default_rng(20261018)
    out = []
    pictures = {}
    for w, h in SIZES:
        pictures[(w, h)] = (make_film(rng, w, h), make_guides(rng, w, h))
        for it in ITERATIONS:
            out.append((f"{w}x{h}-it{it}", *pictures[(w, h)], it, SIGMAS, 16, None))
    film, guides = pictures[(37, 23)]
    for it in (0, 1, 3):
        out.append((f"37x23-it{it}-samples", film, guides, it, SIGMAS, 16, make_samples(rng, 37, 23, 16)))
    film, guides = pictures[(130, 70)]
    out.append(("130x70-it2-samples-td7", film, guides, 2, SIGMAS, 7, make_samples(rng, 130, 70, 7)))
    film, guides = pictures[(64, 36)]
    for k in range(3):
        sig = tuple(INF if j == k else v for j, v in enumerate(SIGMAS))
        out.append((f"64x36-it3-inf{k}", film, guides, 3, sig, 16, None))
    out.append(("64x36-it3-allinf", film, guides, 3, (INF, INF, INF), 16, None))
    return out
