"""An independent numpy float32 restatement of the pixel-mean albedo (the rule stated in include/yuki_hip.h, "Pixel mean"),
one operation per statement, a whole film per step.  It never calls the product: the per-sub-sample record is
albedo_ref.surface_albedo on the large film's ids, then the sequential block sum and one division.  Shared by
tests/test_albedo_mean.py (host instance) and tests/test_gpu_albedo_mean.py (device instance).

The keyword arguments plant the mistakes the bit-exact tests must catch; the defaults are the rule."""
import numpy as np

import albedo_ref
from albedo_ref import ALBEDO_DTYPE, canon

F = np.float32
SIZES = ((37, 23), (12, 7), (1, 1))  # (w, h) of the OUTPUT films on the host
FACTORS = (1, 2, 3, 4)
MASK_THRESHOLD = 0.02  # a pixel "differs" where any channel of the s = 4 mean is further than this from the centre record
# The quality films are albedo_ref.QUALITY's (textured-city, 96 x 54, Path depth 8, Uniform 4 spp against 1024 spp, 4
# iterations at the default sigmas).  The yardstick is denoise(albedo=centre record).  Every bound is the midpoint of 1 and
# the ratio the host instance measures on the oracle's films (the convention of test_temporal.QUALITY), the measured value
# beside it; `no_gain` are the scenes with nothing to gain: the measured ratio and a margin of 0.01 over it.
QUALITY = dict(
    whole={2: 0.9639, 4: 0.9542},  # measured 0.9277 (s = 2) and 0.9083 (s = 4) of the centre record's error 0.0597
    masked={2: 0.9140, 4: 0.8904},  # measured 0.8280 (s = 2) and 0.7808 (s = 4) on the masked pixels
    mask_min=0.2,  # a fifth of the film; measured 0.341
    # measured: textured-cornell 1.0007 (s = 2) and 1.0014 (s = 4), city-small 1.0011 and 1.0002; the larger one + 0.01
    no_gain={"textured-cornell": ((48, 48), 1.0114), "city-small": ((64, 36), 1.0111)},
)


def block_mean(rec, s, divide_by=None, i_outer=False, known_from_centre=False):
    """(s*h, s*w) ALBEDO_DTYPE records of the large film -> (h, w): the rule's mean."""
    s = int(s)
    hh, ww = rec.shape
    assert hh % s == 0 and ww % s == 0
    h, w = hh // s, ww // s
    if s == 1:
        return rec.copy()  # copied: no operation touches the bits
    a = np.ascontiguousarray(rec["a"]).reshape(h, s, w, s, 3)  # [y, j, x, i, channel]
    k = np.ascontiguousarray(rec["known"]).reshape(h, s, w, s)
    order = [(j, i) for i in range(s) for j in range(s)] if i_outer else [(j, i) for j in range(s) for i in range(s)]
    with np.errstate(all="ignore"):
        total = None
        for j, i in order:
            v = a[:, j, :, i, :]
            total = v.copy() if total is None else (total + v).astype(np.float32)
        n = F(s * s if divide_by is None else divide_by)
        q = canon((total / n).astype(np.float32))
    out = np.zeros((h, w), ALBEDO_DTYPE)
    out["a"] = q
    known = k[:, s // 2, :, s // 2] != 0 if known_from_centre else (k != 0).any(axis=(1, 3))
    out["known"] = np.where(known, F(1), F(0))
    return out


def albedo_mean(ids_ss, s, sd, texture_eval, **planted):
    """(s*h, s*w) SURFACE_ID_DTYPE of the large film and the scene data -> (h, w) ALBEDO_DTYPE."""
    return block_mean(albedo_ref.surface_albedo(ids_ss, sd, texture_eval), s, **planted)


def differs(mean, centre, threshold=MASK_THRESHOLD):
    """The pixels whose mean record is further than `threshold` from the centre record in some channel."""
    with np.errstate(all="ignore"):
        return (np.abs(mean["a"].astype(np.float64) - centre["a"].astype(np.float64)) > threshold).any(-1)
