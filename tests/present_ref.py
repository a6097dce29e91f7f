"""An independent numpy float32 restatement of the present pass (ScaleOutput::draw, app/renderpasses/scale_output.rs, as
an 8-bit window frame), one operation per statement.  Written from the rule's statement (include/yuki_hip.h) and the
reference's lines, with the texture coordinate in plain 64-bit integers; it never calls the product's present.  pow goes
through `host_math` functions 3 (logf) and 30 (expf), which tests/test_oracle_libm.py pins.  Shared by
tests/test_present.py (host instance) and tests/test_gpu_present.py (device instance)."""
import numpy as np

F = np.float32
QNAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def target_rect(res, window):
    """scale_output.rs:64-84 in u32 arithmetic: (x0, y0, width, height), top-down, unclipped."""
    w, h = int(res[0]), int(res[1])
    W, H = int(window[0]), int(window[1])
    frame_aspect = F(W) / F(H)
    texture_aspect = F(w) / F(h)
    if frame_aspect < texture_aspect:
        sh = (W * h) // w
        bottom = max(H - sh, 0) // 2 + sh  # from the window's lower edge; the quad's height is -sh
        return 0, H - bottom, W, sh
    sw = (H * w) // h
    left = max(W - sw, 0) // 2
    return left, 0, sw, H  # bottom = H, height = -H


def axis(n_out, x0, extent, texels):
    """Per output pixel: inside the rectangle?, the first tap, the neighbour's weight."""
    k = np.arange(n_out, dtype=np.int64) - x0
    inside = (k >= 0) & (k < extent)
    if extent == 0:
        return inside, np.zeros(n_out, np.int64), np.zeros(n_out, np.float32)
    n = (2 * k + 1) * texels - extent
    d = 2 * extent
    i0 = n // d  # floor
    r = n - i0 * d
    a = r.astype(np.float32) / F(d)
    return inside, i0, a.astype(np.float32)


def taps(film, jj, ii):
    """film[jj, ii] with BorderClamp: (0, 0, 0) outside."""
    h, w, _ = film.shape
    ok = (jj[:, None] >= 0) & (jj[:, None] < h) & (ii[None, :] >= 0) & (ii[None, :] < w)
    t = film[np.clip(jj, 0, h - 1)[:, None], np.clip(ii, 0, w - 1)[None, :]]
    return np.where(ok[..., None], t, F(0)).astype(np.float32)


def canon(v):
    """A NaN that an operation produced is the quiet NaN 0x7fc00000."""
    return np.where(np.isnan(v), QNAN, v).astype(np.float32)


def mix(x, y, a):
    w = F(1) - a
    p = x * w
    q = y * a
    s = canon(p + q)
    return np.where(a == F(0), x, s).astype(np.float32)


def sample(film, window):
    """(inside mask (H, W), filtered colour (H, W, 3)): horizontal mixes first, then the vertical one."""
    film = np.asarray(film, dtype=np.float32)
    h, w, _ = film.shape
    W, H = window
    x0, y0, width, height = target_rect((w, h), window)
    in_x, i0, a = axis(W, x0, width, w)
    in_y, j0, b = axis(H, y0, height, h)
    a3, b3 = a[None, :, None], b[:, None, None]
    with np.errstate(all="ignore"):
        top = mix(taps(film, j0, i0), taps(film, j0, i0 + 1), a3)
        bottom = mix(taps(film, j0 + 1, i0), taps(film, j0 + 1, i0 + 1), a3)
        out = mix(top, bottom, b3)
    return in_y[:, None] & in_x[None, :], out


def _pow(x, y, host_math):
    l = host_math(3, x)
    e = (F(y) * l).astype(np.float32)
    return host_math(30, e)


def encode(x, kind, host_math):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        if kind == 0:
            return x
        if kind == 1:  # linearToSRGB (scale_output.rs:154-158), gamma = 2.2
            p = _pow(x, F(1) / F(2.2), host_math)
            hi = F(1.055) * p
            hi = hi - F(0.055)
            lo = F(12.92) * x
            return np.where(np.isnan(x), QNAN, np.where(x <= F(0.0031308), lo, hi)).astype(np.float32)
        assert kind == 2  # the OpenGL sRGB conversion of a back buffer
        p = _pow(x, F(0.41666), host_math)
        hi = F(1.055) * p
        hi = hi - F(0.055)
        lo = F(12.92) * x
        out = np.where(x < F(1), hi, F(1))
        out = np.where(x < F(0.0031308), lo, out)
        return np.where(x > F(0), out, F(0)).astype(np.float32)  # x <= 0 and NaN


def saturate(x):
    inner = np.where(x < F(1), x, F(1))
    return np.where(x > F(0), inner, F(0)).astype(np.float32)


def quantise(x):
    with np.errstate(all="ignore"):
        s = saturate(np.asarray(x, dtype=np.float32)) * F(255)
        s = s + F(0.5)
        return s.astype(np.uint8)  # truncation of a value in [0.5, 255.5]


def present(film, window, kind, fmt, host_math):
    """fmt "rgb32f": (H, W, 3) float32, 0 outside the rectangle; "rgba8": (H, W, 4) uint8, (0, 0, 0, 255) outside."""
    inside, colour = sample(film, window)
    colour = encode(colour, kind, host_math)
    if fmt == "rgb32f":
        return np.where(inside[..., None], colour, F(0)).astype(np.float32)
    W, H = window
    out = np.zeros((H, W, 4), dtype=np.uint8)
    out[..., 3] = 255
    out[..., :3] = np.where(inside[..., None], quantise(colour), 0)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
