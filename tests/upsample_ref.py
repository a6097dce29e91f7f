"""An independent numpy float32 restatement of the guided upsample (the rule stated in include/yuki_hip.h, "guided
upsampling", and in the header comment of yuki_amd/csrc/yk_upsample.h), one operation per statement, a whole film per tap.
It never calls the product; `exp` is handed in (the oracle's libm_array).  It carries its own plain-bilinear upsample: the
same footprint with the weights b alone on the film as it is, which is what a bilinear stretch of the small film does.
Shared by tests/test_upsample.py (host instance) and tests/test_gpu_upsample.py (device instance), which also take their
inputs and the QUALITY dictionary from here."""
from fractions import Fraction

import numpy as np

import albedo_ref
import denoise_ref
from denoise_ref import GUIDE_DTYPE, bits, canon, dot  # noqa: F401

F = np.float32
INF = float("inf")
ALBEDO_DTYPE = albedo_ref.ALBEDO_DTYPE
MAX_S = 8
FACTORS = (1, 2, 3, 4, 8)

# The quality films are albedo_ref.QUALITY's scene (textured-city, full 96 x 54, Path depth 8, Uniform 4 spp against the
# 1024-spp FULL film), s = 2, low 48 x 27.  The low film goes through the demodulated denoiser (QUALITY's iterations and
# sigmas, the low albedo) and then through each of the three upsamples; the error is the RMSE of x / (1 + x).  The mask:
# the full pixels whose albedo record differs (by more than albedo_mean_ref.MASK_THRESHOLD in some channel) from their
# containing low pixel's record; its share must stay above half the share measured.
# At 96 x 54 the ground's texels are SMALLER than a full pixel (the scene albedo_mean_ref.QUALITY was chosen for), so the
# record of one ray through a pixel centre is not the albedo of what the film averaged — at either resolution.  Two routes:
#   mean    both records are pixel means over the ids of the 4-times larger film (factor 4 for the full film, 8 for the low
#           one): the records the project prescribes where texels are smaller than a pixel.  The bounds are the midpoint of
#           1 and the ratio the host instance measures on the oracle's films (the convention of test_temporal.QUALITY).
#   centre  the full record is the centre ray's and the low one its s x s mean.  Measured: NO gain over the bilinear stretch
#           (the aliasing of the point-sampled texture costs what the demodulation wins), so a midpoint of 1 and the
#           measured ratio on the whole film would be a bound the measurement itself misses; that bound is the no-gain
#           convention instead, the measured ratio + 0.01: the route must not get worse.  On the mask the measured ratio is
#           under 1 and carries the midpoint bound.
# `larger_texels`: the centre route where it is at home — textured-cornell at 96 x 96, whose texels are far larger than a
# pixel (low 48 x 48) — under the midpoint convention.  There the gain comes from the guides: the albedo adds nothing
# (guided / geometry only measured 1.0072).
QUALITY = dict(
    s=2,
    # e_guided / e_bilinear measured 0.9045 (guided 0.0658, geometry only 0.0751, bilinear 0.0728), on the mask 0.8245;
    # the mask is 0.5394 of the film; the fallback ran on no pixel
    mean=dict(whole=0.9523, masked=0.9123, mask_min=0.2697),
    # measured 1.0020 (guided 0.0732, geometry only 0.0753, bilinear 0.0730), on the mask 0.9995; mask 0.4373 of the film
    centre=dict(whole=1.0120, masked=0.99975, mask_min=0.2186),
    # measured 0.9574 (guided 0.1128, geometry only 0.1120, bilinear 0.1178), on the mask 0.9297; mask 0.1332 of the film
    larger_texels=dict(res=(96, 96), whole=0.9787, masked=0.9649, mask_min=0.0666),
    # nothing to demodulate: e_guided / e_geom, the measured ratio + 0.01.  city-small at 64 x 36 measured 0.9984 (guided
    # 0.0681, geometry only 0.0682) — and the bilinear stretch 0.0560: on a film this small, without a texture, the
    # antialiased blend of four taps is closer to the converged film than the guided pass's hard silhouettes.
    no_gain={"city-small": ((64, 36), 1.0084)},
)


def axis(n_low, s):
    """Every full coordinate x of an axis of n_low low pixels -> (X, x0, a): the containing low pixel, the first tap and
    the weight of the second."""
    x = np.arange(s * n_low)
    X = x // s
    i = x - s * X
    t = (2 * i + 1 - s).astype(np.float32) / F(2 * s)
    before = t < F(0)
    x0 = np.where(before, X - 1, X)
    a = np.where(before, (t + F(1)).astype(np.float32), t).astype(np.float32)
    return X, x0, a


def axis_exact(X, i, s):
    """(x0, a) of full pixel s*X + i as exact rationals."""
    t = Fraction(2 * i + 1 - s, 2 * s)
    return (X - 1, t + 1) if t < 0 else (X, t)


def low_colours(low_film, tile_dim, samples, low_albedo):
    """c_Q of every low pixel: normalised by the low table, then divided by the divisor of the low albedo."""
    c = denoise_ref.normalise(low_film, tile_dim, samples)
    if low_albedo is not None:
        with np.errstate(all="ignore"):
            c = canon((c / albedo_ref.divisor(low_albedo["a"])).astype(np.float32))
    return c


def upsample(low_film, low_guides, guides, s, sigma_normal, sigma_plane, exp, tile_dim=16, samples=None, low_albedo=None, albedo=None, bilinear=False):
    """(lh, lw, 3) low film, (lh, lw) low guides, (s*lh, s*lw) guides -> ((s*lh, s*lw, 3) film, (s*lh, s*lw) weight sums).
    bilinear: the weights are b alone and only taps outside the film or with b == 0 are skipped."""
    low_film = np.asarray(low_film, np.float32)
    lh, lw = low_film.shape[:2]
    Xs, x0, ax = axis(lw, s)
    Ys, y0, ay = axis(lh, s)
    den_n = F(sigma_normal) * F(sigma_normal)
    den_p = F(sigma_plane) * F(sigma_plane)
    with np.errstate(all="ignore"):
        c = low_colours(low_film, tile_dim, samples, low_albedo)
        nsP, hp, pP = guides["ns"], guides["hit"] != F(0), guides["p"]
        acc = np.zeros((s * lh, s * lw, 3), np.float32)
        sw = np.zeros((s * lh, s * lw), np.float32)
        for k in range(4):
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            bx = ax if k & 1 else (F(1) - ax).astype(np.float32)
            by = ay if k >> 1 else (F(1) - ay).astype(np.float32)
            b = (bx[None, :] * by[:, None]).astype(np.float32)
            inside = ((qx >= 0) & (qx < lw))[None, :] & ((qy >= 0) & (qy < lh))[:, None]
            cy, cx = np.clip(qy, 0, lh - 1)[:, None], np.clip(qx, 0, lw - 1)[None, :]
            cq, gq = c[cy, cx], low_guides[cy, cx]
            if bilinear:
                w = b
                take = inside & (b != F(0))
            else:
                hq = gq["hit"] != F(0)
                n = nsP - gq["ns"]
                a_n = dot(n[..., 0], n[..., 1], n[..., 2], n[..., 0], n[..., 1], n[..., 2]) / den_n
                v = gq["p"] - pP
                d = dot(nsP[..., 0], nsP[..., 1], nsP[..., 2], v[..., 0], v[..., 1], v[..., 2])
                a_p = (d * d) / den_p
                e = (a_n + a_p).astype(np.float32)
                x = exp((-e).astype(np.float32)).reshape(e.shape)
                w = np.where(hp, (b * x).astype(np.float32), b)
                finite = np.isfinite(cq).all(-1)
                take = inside & (b != F(0)) & (hp == hq) & finite & ~((w == F(0)) | np.isnan(w))
            prod = (w[..., None] * cq).astype(np.float32)
            acc = np.where(take[..., None], acc + prod, acc)
            sw = np.where(take, sw + w, sw)
        out = c[Ys[:, None], Xs[None, :]].copy()  # the containing low pixel, as bits
        q = canon(acc / sw[..., None])
        m = np.broadcast_to((sw != F(0))[..., None], out.shape)
        out.view(np.uint32)[m] = q.view(np.uint32)[m]
        if albedo is not None:
            out = canon((out * albedo_ref.divisor(albedo["a"])).astype(np.float32))
    return out, sw


# ------------------------------------------------------------------ the random records of both suites
def make_case(rng, lw, lh, s, with_albedo, tile_dim=None):
    """Random records that reach every skip case: a low film with NaN / +-inf channels, guides of two planes with a crease
    and miss regions at both resolutions (the low ones sampled from the full ones, then some flipped to the other hit
    class), albedos with every special value, optionally a low sample table with zero counts."""
    W, H = s * lw, s * lh
    low = denoise_ref.make_film(rng, lw, lh)
    guides = denoise_ref.make_guides(rng, W, H)
    low_guides = np.ascontiguousarray(guides[s // 2 :: s, s // 2 :: s]).copy()
    low_guides["p"] += np.where(low_guides["hit"][..., None] != 0, rng.standard_normal((lh, lw, 3)).astype(np.float32) * F(0.003), F(0))
    flip = rng.random((lh, lw)) < 0.08
    other = denoise_ref.make_guides(rng, lw, lh)
    other["hit"] = 1.0 - low_guides["hit"]
    other["ns"] = np.where(other["hit"][..., None] != 0, np.array([0.0, 0.0, 1.0], np.float32), F(0))
    other["p"] = np.where(other["hit"][..., None] != 0, other["p"], F(0))
    low_guides[flip] = other[flip]
    low_albedo = albedo_ref.make_albedo(rng, lw, lh) if with_albedo else None
    albedo = albedo_ref.make_albedo(rng, W, H) if with_albedo else None
    samples = denoise_ref.make_samples(rng, lw, lh, tile_dim) if tile_dim else None
    return low, low_guides, guides, low_albedo, albedo, samples


SIGMAS = ((0.3, 0.06), (0.1, 0.02), (INF, INF))  # (normal, plane): the denoiser's, a pair that underflows across the crease, both stops off
HOST_SIZES = {1: (37, 23), 2: (37, 23), 3: (33, 9), 4: (12, 7), 8: (5, 3)}  # low (w, h) per factor on the host


def host_cases():
    """(name, s, (sigma_normal, sigma_plane), tile_dim, inputs): every factor with and without albedo, with and without a
    sample table on a low film that is no multiple of tile_dim."""
    rng = np.random.default_rng(20261020)
    out = []
    for s in FACTORS:
        lw, lh = HOST_SIZES[s]
        for with_albedo in (False, True):
            for td in (None, 16 if lw > 16 else 4):
                sig = SIGMAS[len(out) % len(SIGMAS)]
                out.append((f"{lw}x{lh}-s{s}{'-albedo' if with_albedo else ''}{'-samples' if td else ''}", s, sig, td or 16, make_case(rng, lw, lh, s, with_albedo, td)))
    return out


def plane_guides(w, h):
    """One plane: n = (0, 0, 1), p.z = 0 — both stops are exactly 0 between any two pixels."""
    g = np.zeros((h, w), GUIDE_DTYPE)
    g["ns"] = np.array([0.0, 0.0, 1.0], np.float32)
    g["hit"] = 1.0
    y, x = np.mgrid[0:h, 0:w]
    g["p"] = np.stack([(x + F(0.5)) / F(w), (y + F(0.5)) / F(h), np.zeros((h, w))], -1).astype(np.float32)
    g["t"] = 1.0
    return g


def rel_error(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))
