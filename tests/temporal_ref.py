"""An independent numpy float32 restatement of the temporal passes (reproject and blend; the rule of
yuki_amd/csrc/yk_temporal.h), one operation per statement, a whole film per step.  It never calls the product: the point
transform, the dot product, the sample-table index rule and the canonical NaN are restated here or taken from the other
restatements (denoise_ref, tonemap_ref).  Shared by tests/test_temporal.py (host instance) and tests/test_gpu_temporal.py
(device instance), which also take their cameras, guides, histories and films from here."""
import numpy as np

import denoise_ref
import tonemap_ref
from denoise_ref import GUIDE_DTYPE, bits, canon, dot  # noqa: F401

F = np.float32
HISTORY_DTYPE = np.dtype([("rgb", "<f4", 3), ("n", "<f4")])
INF = float("inf")


def xf_point(m, x, y, z):
    """Transform::point (math/transform.rs): row sums left to right, the divide by w only where w != 1.  Returns (x, y, z, w)."""
    m = np.asarray(m, np.float32).reshape(16)

    def row(k):
        s = m[4 * k] * x
        s = s + m[4 * k + 1] * y
        s = s + m[4 * k + 2] * z
        return s + m[4 * k + 3]

    xp, yp, zp, wp = row(0), row(1), row(2), row(3)
    one = wp == F(1)
    safe = np.where(one, F(1), wp)
    return np.where(one, xp, xp / safe), np.where(one, yp, yp / safe), np.where(one, zp, zp / safe), wp


def reproject(history, prev_guides, prev_camera, guides, plane_tolerance, normal_cos_min):
    """(h, w) HISTORY_DTYPE, (h, w) GUIDE_DTYPE, a camera with camera_to_world_inv / raster_to_camera_inv (16 floats each),
    (h, w) GUIDE_DTYPE -> (h, w) HISTORY_DTYPE."""
    with np.errstate(all="ignore"):
        h, w = guides.shape
        tol, cmin = F(plane_tolerance), F(normal_cos_min)
        ns, p = guides["ns"], guides["p"]
        live = guides["hit"] != F(0)
        cx, cy, cz, _ = xf_point(np.array(prev_camera.camera_to_world_inv[:], np.float32), p[..., 0], p[..., 1], p[..., 2])
        rx, ry, _, wr = xf_point(np.array(prev_camera.raster_to_camera_inv[:], np.float32), cx, cy, cz)
        live &= wr > F(0)  # false for NaN
        fx = (rx - F(0.5)).astype(np.float32)
        fy = (ry - F(0.5)).astype(np.float32)
        live &= (fx >= F(-1)) & (fx < F(w)) & (fy >= F(-1)) & (fy < F(h))
        fx = np.where(live, fx, F(0))
        fy = np.where(live, fy, F(0))
        flx, fly = np.floor(fx), np.floor(fy)
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        ax, ay = (fx - flx).astype(np.float32), (fy - fly).astype(np.float32)
        wx = ((F(1) - ax).astype(np.float32), ax)
        wy = ((F(1) - ay).astype(np.float32), ay)
        acc = np.zeros((h, w, 4), np.float32)
        sw = np.zeros((h, w), np.float32)
        hq_all = np.concatenate([history["rgb"], history["n"][..., None]], -1).astype(np.float32)
        for k in range(4):
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            inside = (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
            sx, sy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            b = (wx[k & 1] * wy[k >> 1]).astype(np.float32)
            hq = hq_all[sy, sx]
            gq = prev_guides[sy, sx]
            take = live & inside & (b != F(0)) & (gq["hit"] != F(0)) & (hq[..., 3] > F(0)) & np.isfinite(hq[..., :3]).all(-1)
            v = gq["p"] - p
            d = dot(ns[..., 0], ns[..., 1], ns[..., 2], v[..., 0], v[..., 1], v[..., 2])
            take &= np.abs(d) <= tol
            cs = dot(ns[..., 0], ns[..., 1], ns[..., 2], gq["ns"][..., 0], gq["ns"][..., 1], gq["ns"][..., 2])
            take &= cs >= cmin
            prod = (b[..., None] * hq).astype(np.float32)
            acc = np.where(take[..., None], acc + prod, acc)
            sw = np.where(take, sw + b, sw)
        some = sw != F(0)
        q = canon(acc / np.where(some, sw, F(1))[..., None])
        out = np.zeros((h, w), HISTORY_DTYPE)
        out["rgb"] = np.where(some[..., None], q[..., :3], F(0))
        out["n"] = np.where(some, q[..., 3], F(0))
        return out


def blend(film, max_history, tile_dim=16, samples=None, history=None):
    """(h, w, 3) film -> (rgb (h, w, 3), history (h, w) HISTORY_DTYPE); bit patterns of copied values are kept."""
    with np.errstate(all="ignore"):
        film = np.asarray(film, np.float32)
        h, w = film.shape[:2]
        if samples is None:
            m = np.ones((h, w), np.float32)
            c = film.copy()
        else:
            m = tonemap_ref.sample_counts(h, w, tile_dim, samples)
            c = denoise_ref.normalise(film, tile_dim, samples)
        cur = m != F(0)
        out = np.zeros((h, w, 4), np.float32)
        ob = out.view(np.uint32)
        if history is None:
            hist = np.zeros((h, w), bool)
            n = np.zeros((h, w), np.float32)
            hr = np.zeros((h, w, 3), np.float32)
        else:
            hr = np.ascontiguousarray(history["rgb"], np.float32)
            hn = np.ascontiguousarray(history["n"], np.float32)
            n = np.where(hn > F(max_history), F(max_history), hn).astype(np.float32)
            hist = (n > F(0)) & np.isfinite(hr).all(-1)
        only_c = cur & ~hist
        ob[..., :3][only_c] = bits(c)[only_c]
        ob[..., 3][only_c] = bits(m)[only_c]
        only_h = hist & ~cur
        ob[..., :3][only_h] = bits(hr)[only_h]
        ob[..., 3][only_h] = bits(n)[only_h]
        both = hist & cur
        t = (n + m).astype(np.float32)
        nh = (n[..., None] * hr).astype(np.float32)
        mc = (m[..., None] * c).astype(np.float32)
        s = (nh + mc).astype(np.float32)
        q = canon(s / np.where(both, t, F(1))[..., None])
        ob[..., :3][both] = bits(q)[both]
        ob[..., 3][both] = bits(t)[both]
        rec = np.zeros((h, w), HISTORY_DTYPE)
        rec["rgb"] = out[..., :3]
        rec["n"] = out[..., 3]
        return out[..., :3].copy(), rec


# ------------------------------------------------------------------ the cameras, guides, histories and films of both suites
SIZES = ((1, 1), (5, 70), (33, 9), (37, 23), (64, 36))  # (w, h): none a multiple of the 32 x 8 block
BASE = dict(position=(0.3, 1.6, 4.0), target=(0.0, 0.6, 0.0), up=(0, 1, 0), fov_axis=0, fov_degrees=50.0)


def _moved(**kw):
    c = dict(BASE)
    c.update(kw)
    return c


# name -> (previous camera, current camera)
CAMERA_PAIRS = {
    "same": (BASE, BASE),
    "translate": (BASE, _moved(position=(0.42, 1.63, 4.0), target=(0.12, 0.63, 0.0))),
    "rotate": (BASE, _moved(target=(1.6, 0.6, 0.0))),  # part of the view leaves the film
    "dolly-in": (BASE, _moved(position=(0.15, 1.1, 2.0))),  # magnification: neighbouring pixels share taps
    "dolly-out": (BASE, _moved(position=(0.45, 2.1, 6.0))),
    "about-face": (_moved(target=(0.6, 2.6, 8.0)), BASE),  # the previous camera looked the other way: every point behind it
}


def plane_guides(cam, w, h, rng=None):
    """First hits of the pixel-centre rays of `cam` (matrices) on a floor y = 0 and a wall z = -1.5; what lies further than
    30 units is a miss.  With rng: scattered misses and slightly perturbed normals."""
    with np.errstate(all="ignore"):
        y, x = np.mgrid[0:h, 0:w]
        r2c = np.array(cam.raster_to_camera[:], np.float32)
        c2w = np.array(cam.camera_to_world[:], np.float32).reshape(4, 4)
        px, py, pz, _ = xf_point(r2c, (x + 0.5).astype(np.float32), (y + 0.5).astype(np.float32), np.zeros((h, w), np.float32))
        d = np.stack([px, py, pz], -1).astype(np.float64)
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        d = d @ c2w[:3, :3].astype(np.float64).T
        o = c2w[:3, 3].astype(np.float64)
        t_floor = np.where(d[..., 1] < 0, -o[1] / d[..., 1], np.inf)
        t_wall = np.where(d[..., 2] < 0, (-1.5 - o[2]) / d[..., 2], np.inf)
        t = np.minimum(t_floor, t_wall)
        hit = np.isfinite(t) & (t < 30.0)
        if rng is not None:
            hit &= rng.random((h, w)) > 0.04
        n = np.where((t_floor <= t_wall)[..., None], np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]))
        if rng is not None:
            n = n + rng.standard_normal((h, w, 3)) * 0.01
            n /= np.linalg.norm(n, axis=-1, keepdims=True)
        p = o + np.where(hit, t, 0.0)[..., None] * d
        g = np.zeros((h, w), GUIDE_DTYPE)
        g["hit"] = hit.astype(np.float32)
        g["ns"] = np.where(hit[..., None], n, 0.0).astype(np.float32)
        g["p"] = np.where(hit[..., None], p, 0.0).astype(np.float32)
        g["t"] = np.where(hit, t, 0.0).astype(np.float32)
        return g


def make_history(rng, w, h):
    """Ordinary means and counts plus NaN, +-inf, -0 and 1e30 channels, and counts of 0, -3, NaN and +inf."""
    rec = np.zeros((h, w), HISTORY_DTYPE)
    rec["rgb"] = denoise_ref.make_film(rng, w, h)
    n = rng.integers(1, 100, size=(h, w)).astype(np.float32)
    pool = np.array([0.0, -3.0, np.nan, np.inf, -0.0, 0.5], np.float32)
    pick = rng.random((h, w)) < 0.08
    n[pick] = pool[rng.integers(0, len(pool), size=int(pick.sum()))]
    rec["n"] = n
    return rec


def make_samples(rng, w, h, tile_dim):
    return denoise_ref.make_samples(rng, w, h, tile_dim)
