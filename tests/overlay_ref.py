"""An independent numpy float32 restatement of the overlay passes (app/renderpasses/ray_visualization.rs,
bvh_visualization.rs; BoundingVolumeHierarchy::node_bounds, bvh.rs:121-157) and of the line rule of
yuki_amd/csrc/yk_overlay.h, one operation per statement.  It never calls the product.  Shared by tests/test_overlay.py
(host instance) and tests/test_gpu_overlay.py (device instance)."""
from collections import deque

import numpy as np

F = np.float32
FLT_MAX = F(3.4028235e38)

RAY_COLOURS = {0: (1.0, 1.0, 1.0), 1: (1.0, 0.0, 0.0), 2: (0.0, 1.0, 0.0), 3: (0.0, 0.0, 1.0), 4: (1.0, 1.0, 0.0)}
LINE_DTYPE = np.dtype([("p0", "<f4", 3), ("p1", "<f4", 3), ("rgb", "<f4", 3)])
# bvh_visualization.rs:41-67
CORNER_FROM_MAX = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 4), (1, 5), (2, 6), (3, 7), (4, 5), (5, 6), (6, 7), (7, 4)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# --------------------------------------------------------------------------- node_bounds
def node_bounds(nodes, target_level):
    """bvh.rs:121-157 over the exported nodes (abi.BVH_NODE_DTYPE: bmin, bmax, a = second child, is_leaf)."""
    out = []

    def box(i):
        return np.stack([nodes["bmin"][i], nodes["bmax"][i]])

    if target_level <= 0:
        out.append(box(0))
    queue = deque([(0, 1)])
    while queue:
        index, level = queue.popleft()
        if target_level >= 0 and level > target_level:
            break
        if not nodes["is_leaf"][index]:
            second = int(nodes["a"][index])
            if target_level < 0 or level == target_level:
                out.append(box(index + 1))
                out.append(box(second))
            queue.append((index + 1, level + 1))
            queue.append((second, level + 1))
    return np.array(out, dtype=np.float32).reshape(-1, 2, 3)


def tree_depth(nodes):
    """The number of levels: 1 for a root that is a leaf."""
    depth, stack = 0, [(0, 1)]
    while stack:
        i, lv = stack.pop()
        depth = max(depth, lv)
        if not nodes["is_leaf"][i]:
            stack += [(i + 1, lv + 1), (int(nodes["a"][i]), lv + 1)]
    return depth


# --------------------------------------------------------------------------- world_to_clip
def mat_mul(a, b):
    """matrix.rs:289-301: ((a0*b0 + a1*b1) + a2*b2) + a3*b3."""
    r = np.zeros((4, 4), np.float32)
    for row in range(4):
        for col in range(4):
            s = a[row, 0] * b[0, col]
            s = s + a[row, 1] * b[1, col]
            s = s + a[row, 2] * b[2, col]
            s = s + a[row, 3] * b[3, col]
            r[row, col] = s
    return r


def world_to_clip(world_to_camera, position, fov_axis, fov_degrees, res, bounds, tan):
    """ray_visualization.rs:87-157.  world_to_camera: look_at's matrix (4, 4); bounds (p_min, p_max); tan: f32 -> f32."""
    with np.errstate(all="ignore"):
        p0, p1 = np.asarray(bounds, np.float32).reshape(2, 3)
        pos = np.asarray(position, np.float32)
        pts = [p0, (p0[0], p0[1], p1[2]), (p0[0], p1[1], p0[2]), (p0[0], p1[1], p1[2]), (p1[0], p0[1], p0[2]), (p1[0], p0[1], p1[2]), (p1[0], p1[1], p0[2]), p1]
        zf = F(0)
        for p in pts:
            d = np.asarray(p, np.float32) - pos
            sq = F(0) + d[0] * d[0]
            sq = sq + d[1] * d[1]
            sq = sq + d[2] * d[2]
            ln = F(np.sqrt(np.float64(sq)))
            zf = ln if (ln > zf or zf != zf) else zf
        zn = zf * F(1e-5)
        half = F(fov_degrees) * F(0.5)
        rad = half * (F(np.pi) / F(180.0))
        t = F(tan(rad))
        rx, ry = F(res[0]), F(res[1])
        if fov_axis == 0:
            ar = ry / rx
            xf = F(1) / t
            yf = F(1) / (t * ar)
        else:
            ar = rx / ry
            xf = F(1) / (t * ar)
            yf = F(1) / t
        c2c = np.zeros((4, 4), np.float32)
        c2c[0, 0] = xf
        c2c[1, 1] = yf
        c2c[2, 2] = (zf + zn) / (zf - zn)
        c2c[2, 3] = -((F(2.0) * zf) * zn) / (zf - zn)
        c2c[3, 2] = F(1)
        flip = np.eye(4, dtype=np.float32)
        flip[1, 1] = F(-1)
        return mat_mul(flip, mat_mul(c2c, np.asarray(world_to_camera, np.float32).reshape(4, 4)))


# --------------------------------------------------------------------------- line lists
def ray_lines(rays):
    """ray_visualization.rs:28-56 for records with fields o, d, t_max, ray_type."""
    out = np.zeros(len(rays), LINE_DTYPE)
    with np.errstate(all="ignore"):
        for i, r in enumerate(rays):
            out["p0"][i] = r["o"]
            s = r["d"] * r["t_max"]
            out["p1"][i] = r["o"] + s
            out["rgb"][i] = RAY_COLOURS[int(r["ray_type"])]
    return out


# --------------------------------------------------------------------------- the rule of yk_overlay.h
def clip_points(m, p):
    """Step 1 for points (n, 3): (n, 4)."""
    m = np.asarray(m, np.float32).reshape(4, 4)
    p = np.asarray(p, np.float32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.zeros((len(p), 4), np.float32)
    with np.errstate(all="ignore"):
        for i in range(4):
            a = m[i, 0] * x
            b = m[i, 1] * y
            s = a + b
            c = m[i, 2] * z
            s = s + c
            out[:, i] = s + m[i, 3]
    return out


def box_segments(m, boxes):
    """The 12 edges of every box in the reference's order, as clip-space ends, and their colours."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 2, 3)
    n = len(boxes)
    corners = np.zeros((n, 8, 3), np.float32)
    for j, sel in enumerate(CORNER_FROM_MAX):
        for axis in range(3):
            corners[:, j, axis] = boxes[:, sel[axis], axis]
    clip = clip_points(m, corners.reshape(-1, 3)).reshape(n, 8, 4)
    c0 = np.stack([clip[:, i0] for i0, _ in EDGES], axis=1).reshape(-1, 4)
    c1 = np.stack([clip[:, i1] for _, i1 in EDGES], axis=1).reshape(-1, 4)
    rgb = np.zeros((n, 12, 3), np.float32)
    rgb[0::2, :, 0] = 1.0
    rgb[1::2, :, 1] = 1.0
    return c0, c1, rgb.reshape(-1, 3)


def _window(v, w, res):
    n = v / w
    n = n * F(0.5)
    n = n + F(0.5)
    return n * F(res)


def _first_center(v, res):
    """The smallest integer k in [0, res] with k + 0.5 >= v."""
    k = np.zeros(v.shape, np.int64)
    k[v >= F(res)] = res
    mid = (v > F(0.5)) & (v < F(res))
    fl = np.floor(v[mid])
    k[mid] = fl.astype(np.int64) + ((fl + F(0.5)) < v[mid])
    return k


def spans(c0, c1, res_x, res_y):
    """Steps 2-5 for clip-space ends (n, 4): a dict of per-segment arrays; `ok` marks the segments that draw."""
    with np.errstate(all="ignore"):
        c0 = np.array(c0, np.float32).reshape(-1, 4)
        c1 = np.array(c1, np.float32).reshape(-1, 4)
        n = len(c0)
        ok = np.all(np.abs(c0) <= FLT_MAX, axis=1) & np.all(np.abs(c1) <= FLT_MAX, axis=1)  # 2
        less = np.zeros(n, bool)  # 2a: c1 < c0, component by component
        decided = np.zeros(n, bool)
        for i in range(4):
            ne = (c1[:, i] != c0[:, i]) & ~decided
            less[ne] = c1[ne, i] < c0[ne, i]
            decided |= ne
        c0[less], c1[less] = c1[less].copy(), c0[less].copy()
        t0 = np.zeros(n, np.float32)  # 3
        t1 = np.ones(n, np.float32)
        for i, sign in ((0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)):
            d0 = c0[:, 3] + c0[:, i] if sign > 0 else c0[:, 3] - c0[:, i]
            d1 = c1[:, 3] + c1[:, i] if sign > 0 else c1[:, 3] - c1[:, i]
            n0, n1 = d0 < 0, d1 < 0
            ok &= ~(n0 & n1)
            den = d0 - d1
            t = d0 / den
            up = n0 & ~n1 & (t > t0)
            t0 = np.where(up, t, t0)
            dn = n1 & ~n0 & (t < t1)
            t1 = np.where(dn, t, t1)
        ok &= ~(t0 > t1)
        d = c1 - c0
        e0 = np.where((t0 != 0)[:, None], c0 + d * t0[:, None], c0)
        e1 = np.where((t1 != 1)[:, None], c0 + d * t1[:, None], c1)
        x0, y0 = _window(e0[:, 0], e0[:, 3], res_x), _window(e0[:, 1], e0[:, 3], res_y)  # 4
        x1, y1 = _window(e1[:, 0], e1[:, 3], res_x), _window(e1[:, 1], e1[:, 3], res_y)
        for v in (x0, y0, x1, y1):
            ok &= np.abs(v) <= FLT_MAX  # 4a
        dx, dy = x1 - x0, y1 - y0  # 5
        x_major = np.abs(dx) >= np.abs(dy)
        a, b = np.where(x_major, x0, y0), np.where(x_major, x1, y1)
        m_a, m_b = np.where(x_major, y0, x0), np.where(x_major, y1, x1)
        swap = a > b
        a, b = np.where(swap, b, a), np.where(swap, a, b)
        m_a, m_b = np.where(swap, m_b, m_a), np.where(swap, m_a, m_b)
        ok &= a < b
        k_lo = np.zeros(n, np.int64)
        k_hi = np.zeros(n, np.int64)
        for major, res in ((True, res_x), (False, res_y)):
            sel = ok & (x_major == major)
            k_lo[sel] = _first_center(a[sel], res)
            k_hi[sel] = _first_center(b[sel], res)
        slope = (m_b - m_a) / (b - a)
        ok &= k_lo < k_hi
        return dict(ok=ok, x_major=x_major, k_lo=k_lo, k_hi=k_hi, a=a, m_a=m_a, slope=slope)


def segment_pixels(s, i, res_x, res_y):
    """Step 6 for segment i of spans(): (x, y) index arrays."""
    with np.errstate(all="ignore"):
        k = np.arange(s["k_lo"][i], s["k_hi"][i], dtype=np.int64)
        c = k.astype(np.float32) + F(0.5)
        u = c - s["a"][i]
        v = u * s["slope"][i]
        m = s["m_a"][i] + v
        res_minor = res_y if s["x_major"][i] else res_x
        keep = (m >= 0) & (m < F(res_minor))
        j = np.floor(m[keep]).astype(np.int64)
        k = k[keep]
        return (k, j) if s["x_major"][i] else (j, k)


def draw(film, m, lines=None, boxes=None):
    """Step 7: a copy of the (h, w, 3) film with the lines, then the boxes drawn one after the other."""
    out = np.array(film, dtype=np.float32, copy=True)
    h, w = out.shape[0], out.shape[1]
    flat = out.reshape(h * w, 3).view(np.uint32)
    batches = []
    if lines is not None and len(lines):
        lines = np.asarray(lines, LINE_DTYPE)
        batches.append((clip_points(m, lines["p0"]), clip_points(m, lines["p1"]), lines["rgb"]))
    if boxes is not None and len(boxes):
        batches.append(box_segments(m, boxes))
    for c0, c1, rgb in batches:
        s = spans(c0, c1, w, h)
        colour = bits(rgb).reshape(-1, 3)
        for i in np.nonzero(s["ok"])[0]:
            x, y = segment_pixels(s, i, w, h)
            flat[y * w + x] = colour[i]
    return out


def covered(m, lines, res_x, res_y):
    """The set of pixels (x, y) the lines cover."""
    film = draw(np.zeros((res_y, res_x, 3), np.float32), m, lines=lines)
    ys, xs = np.nonzero(bits(film).any(axis=2))
    return set(zip(xs.tolist(), ys.tolist()))


# --------------------------------------------------------------------------- inputs
def random_film(rng, h, w):
    film = rng.uniform(0.0, 1.0, size=(h, w, 3)).astype(np.float32)
    # payload NaNs, infinities and negative zero: untouched pixels must keep their bits
    v = film.reshape(-1).view(np.uint32)
    idx = rng.choice(v.size, size=max(1, v.size // 50), replace=False)
    v[idx] = rng.choice(np.array([0x7FC01234, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x7F800001], np.uint32), size=idx.size)
    return film


def make_lines(p0, p1, rgb=None, rng=None):
    p0 = np.asarray(p0, np.float32).reshape(-1, 3)
    out = np.zeros(len(p0), LINE_DTYPE)
    out["p0"] = p0
    out["p1"] = np.asarray(p1, np.float32).reshape(-1, 3)
    if rgb is None:
        rgb = (rng or np.random.default_rng(5)).uniform(0.05, 1.0, size=(len(p0), 3))
    out["rgb"] = rgb
    return out


def simple_matrix():
    """A perspective world_to_clip for hand-made geometry: camera at the origin looking down +z, w = z, x and y in
    [-w, w] visible, near 0.1, far 100, y flipped as the reference's matrix is."""
    zn, zf = 0.1, 100.0
    return np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, (zf + zn) / (zf - zn), -(2 * zf * zn) / (zf - zn)], [0, 0, 1, 0]], np.float32)


def to_world(xw, yw, z, res_x, res_y):
    """The world point that simple_matrix() puts at window (xw, yw) and depth z (up to float32 rounding)."""
    return ((xw / res_x - 0.5) * 4.0 * (z / 2.0), -(yw / res_y - 0.5) * 4.0 * (z / 2.0), z)


FILMS = ((23, 37), (40, 64), (5, 1), (1, 5), (150, 200))  # (h, w)


def line_sets(w, h, rng):
    """Named line lists for a w x h film under simple_matrix()."""

    def seg(a, b, z0=2.0, z1=2.0):
        return to_world(a[0], a[1], z0, w, h), to_world(b[0], b[1], z1, w, h)

    def lines(segs):
        return make_lines([s[0] for s in segs], [s[1] for s in segs], rng=rng)

    d = min(w, h)
    inf, nan = np.inf, np.nan
    sets = {
        "empty": make_lines(np.zeros((0, 3)), np.zeros((0, 3)), rng=rng),
        "horizontal": lines([seg((0, 3.5), (w, 3.5)), seg((1.25, 0.0), (w - 0.75, 0.0)), seg((0.5, h / 2), (w - 0.5, h / 2)), seg((w, 1.0), (0, 1.0))]),
        "vertical": lines([seg((3.5, 0), (3.5, h)), seg((0.0, 0.25), (0.0, h - 0.25)), seg((w / 2, 0.5), (w / 2, h - 0.5)), seg((1.0, h), (1.0, 0))]),
        "diagonal": lines([seg((0, 0), (d, d)), seg((0, d), (d, 0)), seg((0.5, 0), (d, d - 0.5)), seg((0, 0.5), (d - 0.5, d))]),
        "centres": lines([seg((0.5, 0.5), (w - 0.5, h - 0.5)), seg((w - 0.5, 0.5), (0.5, h - 0.5)), seg((0.5, 0.5), (1.5, 0.5))]),
        "corners": lines([seg((0, 0), (w, h)), seg((w, 0), (0, h)), seg((1, 1), (w, h / 2)), seg((0, 0), (1, 1))]),
        "zero length": lines([seg((2.5, 0.5), (2.5, 0.5)), seg((0, 0), (0, 0))]),
        "outside": lines([seg((w + 3, 1), (w + 9, h)), seg((-5, -5), (-1, -9)), seg((1, h + 2), (w, h + 7))]),
        "planes": make_lines(
            [(0, 0, 2), (0, 0, 2), (0, 0, 2), (0, 0, 2), (0.01, 0.02, 0.05), (0.5, -0.5, 50), (-9, 0.3, 3), (0.2, 7, 1)],
            [(-6, 0.3, 2), (6, -0.2, 2), (0.1, 6, 2), (-0.3, -6, 2), (0.2, 0.1, 1), (-3, 2, 200), (9, -0.4, 3), (-0.1, -7, 1.5)],
            rng=rng,
        ),
        "behind": make_lines([(0, 0, -1), (0.3, 0.2, -2), (1, 1, 0)], [(1, 1, -3), (-0.5, 0.4, 4), (0.5, -0.5, 3)], rng=rng),
        "non-finite": make_lines([(0, 0, 2), (nan, 0, 2), (0, 0, 2), (0.1, 0.1, 1)], [(inf, 0, 2), (1, 1, 2), (0, -inf, inf), (0.2, 0.2, 3.0e38)], rng=rng),
        "random": random_lines(rng, 300),
    }
    if (w, h) == (64, 40):
        sets["random 5000"] = random_lines(rng, 5000)
    return sets


def random_lines(rng, n):
    p = rng.uniform(-6.0, 6.0, size=(2, n, 3))
    p[:, :, 2] = rng.uniform(-1.0, 8.0, size=(2, n))
    return make_lines(p[0], p[1], rng=rng)


def random_boxes(rng, n, size=1.5):
    lo = rng.uniform(-6.0, 6.0, size=(n, 3))
    lo[:, 2] = rng.uniform(-1.0, 8.0, size=n)
    hi = lo + rng.uniform(0.0, size, size=(n, 3))
    return np.stack([lo, hi], axis=1).astype(np.float32)


def box_sets(rng):
    return {
        "one": random_boxes(rng, 1),
        "two": random_boxes(rng, 2),
        "random 1000": random_boxes(rng, 1000),
        "around the camera": np.array([[(-1, -1, -1), (1, 1, 1)], [(-0.5, -2, -3), (2, 0.5, 4)]], np.float32),
        "flat": np.array([[(-1, -1, 3), (1, 1, 3)], [(0.5, -1, 2), (0.5, 1, 4)], [(0, 0, 2), (0, 0, 2)]], np.float32),
    }
