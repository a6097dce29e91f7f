"""An independent numpy float32 restatement of the adaptive-sampling rule, written from the comment in
include/yuki_hip.h ("adaptive sampling"), not from the C++: select with the order of its list, the fold and the resolve.
numpy's float32 array operations are separate IEEE-754 operations (no fusing), which is the rule's arithmetic; a NaN an
operation produces is made the canonical 0x7fc00000 here as there.  Also the sprinkled statistics the CPU and GPU suites
share."""
import numpy as np

F = np.float32
STATS = np.dtype([("mean", "<f4"), ("m2", "<f4"), ("n", "<u4"), ("drawn", "<u4")])
TILE = 16
INF = F(np.inf)
CANON = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]
SIZES = [(5, 3), (37, 23), (130, 70), (528, 528)]  # one clipped tile; 3 x 2 tiles, both edges clipped; 9 x 5; 1089 tiles: the tile-count scan crosses its 1024-entry block


def canon(v):
    v = np.array(v, dtype=F, copy=True)
    v[np.isnan(v)] = CANON
    return v


def luminance(c):
    with np.errstate(all="ignore"):
        pr, pg, pb = F(0.2126) * c[..., 0], F(0.7152) * c[..., 1], F(0.0722) * c[..., 2]
        return canon((pr + pg) + pb)


def wants(stats, min_samples, threshold, epsilon):
    with np.errstate(all="ignore"):
        thr2 = F(threshold) * F(threshold)
        nf = stats["n"].astype(F)
        rhs = (thr2 * ((nf - F(1)) * nf)) * ((stats["mean"] + F(epsilon)) * (stats["mean"] + F(epsilon)))
        return (stats["n"] < min_samples) | (stats["m2"] > rhs)


def select(stats, min_samples, max_samples, round_passes, dilate, threshold, epsilon):
    """-> (xy, sample): uint32 arrays in the rule's order."""
    h, w = stats.shape
    wnt = wants(stats, min_samples, threshold, epsilon)
    eligible = stats["drawn"].astype(np.int64) + int(round_passes) <= int(max_samples)
    near = np.zeros((h, w), dtype=bool)
    if dilate:
        pad = np.zeros((h + 2, w + 2), dtype=bool)
        pad[1:-1, 1:-1] = wnt
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if (dy, dx) != (1, 1):
                    near |= pad[dy : dy + h, dx : dx + w]
    sel = eligible & (wnt | near)
    xs, ys = [], []
    for ty in range(0, h, TILE):
        for tx in range(0, w, TILE):
            yy, xx = np.nonzero(sel[ty : ty + TILE, tx : tx + TILE])  # row-major inside the tile
            xs.append(xx + tx)
            ys.append(yy + ty)
    x = np.concatenate(xs).astype(np.uint32)
    y = np.concatenate(ys).astype(np.uint32)
    return x | (y << np.uint32(16)), stats["drawn"][y, x].astype(np.uint32)


def fold(xy, passes, film_sum, stats):
    """passes (n_passes, n, 3) folded in pass order into copies of film_sum (h, w, 3) and stats (h, w); -> (film_sum, stats)."""
    film_sum, stats = film_sum.copy(), stats.copy()
    x, y = (xy & 0xFFFF).astype(np.int64), (xy >> 16).astype(np.int64)
    assert len(set(zip(x.tolist(), y.tolist()))) == len(xy)
    f = film_sum[y, x]
    mean, m2, n, drawn = stats["mean"][y, x], stats["m2"][y, x], stats["n"][y, x], stats["drawn"][y, x]
    with np.errstate(all="ignore"):
        for c in np.asarray(passes, dtype=F):
            drawn = drawn + np.uint32(1)
            l = luminance(c)
            ok = np.isfinite(canon(l * l))
            f = np.where(ok[:, None], canon(f + c), f)
            n2 = n + np.uint32(1)
            d = l - mean
            mean2 = canon(mean + d / n2.astype(F))
            m22 = canon(m2 + d * (l - mean2))
            mean, m2, n = np.where(ok, mean2, mean), np.where(ok, m22, m2), np.where(ok, n2, n)
    film_sum[y, x] = f
    stats["mean"][y, x], stats["m2"][y, x], stats["n"][y, x], stats["drawn"][y, x] = mean, m2, n, drawn
    return film_sum, stats


def resolve(film_sum, stats):
    """-> (rgb (h, w, 3), variance (h, w))."""
    with np.errstate(all="ignore"):
        nf = stats["n"].astype(F)
        rgb = np.where((stats["n"] > 0)[..., None], canon(film_sum / nf[..., None]), F(0)).astype(F)
        v = canon(stats["m2"] / ((nf - F(1)) * nf))
        v = np.where(v >= 0, v, F(0))  # NaN or negative
        var = np.where(stats["n"] >= 2, v, INF).astype(F)
    return rgb, var


def welford(ls):
    """(mean, m2) of a sequence of float32 luminances, one scalar operation after the other."""
    mean, m2 = F(0), F(0)
    for k, l in enumerate(ls):
        d = F(l) - mean
        mean = F(mean + F(d / F(k + 1)))
        m2 = F(m2 + F(d * F(F(l) - mean)))
    return mean, m2


def sprinkled_stats(rng, w, h, min_samples, max_samples, round_passes):
    """Plausible statistics around the threshold with every special value of the rule sprinkled in."""
    n = rng.integers(min_samples, max_samples + 1, size=(h, w)).astype(np.uint32)
    s = np.zeros((h, w), dtype=STATS)
    s["n"] = n
    s["drawn"] = np.minimum(n + rng.integers(0, 3, size=(h, w)).astype(np.uint32), max_samples)
    s["mean"] = rng.uniform(0.0, 2.0, size=(h, w)).astype(F)
    nf = n.astype(np.float64)
    s["m2"] = (rng.uniform(0.0, 2.5, size=(h, w)) * 0.01 * nf * (nf - 1) * (s["mean"].astype(np.float64) + 0.01) ** 2).astype(F)  # 0 .. 2.5 x the threshold at 0.1
    pick = lambda k: rng.random((h, w)) < k  # noqa: E731
    for v in (0, 1, min_samples - 1, min_samples):
        s["n"][pick(0.04)] = v
    for v in (max_samples, max_samples - round_passes, max_samples - round_passes + 1, 0):
        s["drawn"][pick(0.04)] = v
    for v in (F(0), INF, CANON, -INF):
        s["m2"][pick(0.03)] = v
    for v in (F(-0.0), F(1e30), CANON, INF):
        s["mean"][pick(0.03)] = v
    return s
