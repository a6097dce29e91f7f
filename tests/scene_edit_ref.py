"""The rules of an edit in place (yk_scene_apply_edit) and of the sphere case of the motion pass (yuki_amd/csrc/yk_motion.h)
restated in numpy, one float32 operation per statement; it never calls the product.  Also the moved sphere tables both
suites use, and the float64 statement of a sphere point's previous position."""
import copy

import numpy as np

import motion_ref
from denoise_ref import bits, canon

F = np.float32
BIG = np.finfo(np.float32).max
# transform.rs:194-206: the corners of a box in the order Transform * Bounds3 visits them
CORNERS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))


def xf_point(m, p):
    """&Transform * Point3 (transform.rs:128-142) in float32: m is (..., 16) or (16,), p is (..., 3).  Each row is
    m0 * x + m1 * y + m2 * z + m3, products first, summed left to right; divided by w unless w == 1."""
    m = np.asarray(m, F)
    p = np.asarray(p, F)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        rows = []
        for r in range(4):
            t0 = (m[..., 4 * r] * x).astype(F)
            t1 = (m[..., 4 * r + 1] * y).astype(F)
            t2 = (m[..., 4 * r + 2] * z).astype(F)
            s = (t0 + t1).astype(F)
            s = (s + t2).astype(F)
            rows.append((s + m[..., 4 * r + 3]).astype(F))
        out = np.stack(rows[:3], axis=-1).astype(F)
        w = rows[3]
        div = (out / w[..., None]).astype(F)
        return np.where((w == F(1))[..., None], out, div).astype(F)


def _rmin(a, b):
    """yk_math.h rmin(a, b): b where a is NaN, a where b is NaN, else b only where it is smaller (a tie keeps a)."""
    return np.where(a != a, b, np.where(b != b, a, np.where(b < a, b, a))).astype(F)


def _rmax(a, b):
    return np.where(a != a, b, np.where(b != b, a, np.where(b > a, b, a))).astype(F)


def sphere_bounds(spheres):
    """(n, 6) float32: Sphere::world_bound of every sphere of a SceneData list — the box [-r, r]^3, its eight corners
    through object_to_world in CORNERS' order, folded with rmin / rmax from +-f32::MAX."""
    out = np.zeros((len(spheres), 6), F)
    for k, s in enumerate(spheres):
        m = np.asarray(s["o2w"], F).reshape(16)
        r = F(s["radius"])
        lo, hi = np.full(3, BIG, F), np.full(3, -BIG, F)
        for c in CORNERS:
            q = xf_point(m, np.array([r if c[0] else -r, r if c[1] else -r, r if c[2] else -r], F))
            lo, hi = _rmin(lo, q), _rmax(hi, q)
        out[k, :3], out[k, 3:] = lo, hi
    return out


def surface_motion(ids, guides, indices, prev_points, n_triangles, current, prev):
    """motion_ref.surface_motion with the sphere case of a previous sphere table: `current` and `prev` are (n_spheres,)
    records with object_to_world, world_to_object and radius (abi.SPHERE_DTYPE).  Sphere k: q = xf_point(w2o_current, p),
    q * (r_prev / r_current) unless the radii have equal bits, p_prev = xf_point(o2w_prev, q), canonical."""
    n_spheres = len(current)
    if n_triangles:
        out = motion_ref.surface_motion(ids, guides, indices, prev_points, n_triangles, n_spheres)
    else:
        out = motion_ref.surface_motion(ids, guides, np.zeros((0, 3), np.uint32), np.zeros((0, 3), F), 0, n_spheres)
    if not n_spheres:
        return out
    with np.errstate(all="ignore"):
        shape = ids["shape"].astype(np.int64)
        sph = (ids["shape"] != np.uint32(motion_ref.SURFACE_NONE)) & (guides["hit"] != F(0)) & (shape >= n_triangles) & (shape < n_triangles + n_spheres)
        k = np.where(sph, shape - n_triangles, 0)
        q = xf_point(np.asarray(current["world_to_object"], F)[k], guides["p"])
        r, rp = np.asarray(current["radius"], F)[k], np.asarray(prev["radius"], F)[k]
        f = (rp / r).astype(F)
        scaled = (q * f[..., None]).astype(F)
        q = np.where((bits(r) != bits(rp))[..., None], scaled, q).astype(F)
        p = canon(xf_point(np.asarray(prev["object_to_world"], F)[k], q))
        pb = out["p_prev"].view(np.uint32)
        pb[sph] = bits(np.ascontiguousarray(p))[sph]
    return out


def sphere_p_prev64(p, current, prev, k):
    """The float64 statement: the point p (n, 3) on sphere k of the current table, where it stood under the previous one.
    The matrices are taken as given (float32 values, exact in float64); the inverse is the table's own world_to_object."""
    w2o = np.asarray(current["world_to_object"], np.float64)[k].reshape(-1, 4, 4)
    o2w = np.asarray(prev["object_to_world"], np.float64)[k].reshape(-1, 4, 4)
    ph = np.concatenate([np.asarray(p, np.float64), np.ones((len(p), 1))], axis=1)
    q = np.einsum("nij,nj->ni", w2o, ph)
    q = q[:, :3] / q[:, 3:4]
    q = q * (np.asarray(prev["radius"], np.float64)[k] / np.asarray(current["radius"], np.float64)[k])[:, None]
    r = np.einsum("nij,nj->ni", o2w, np.concatenate([q, np.ones((len(p), 1))], axis=1))
    return r[:, :3] / r[:, 3:4]


# ------------------------------------------------------------------ moved sphere tables
def _rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.eye(4)
    r[:3, :3] = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    return r


def transformed(sphere, m64, radius=None):
    """The SceneData sphere with `m64` (4 x 4, float64) applied after its object_to_world; world_to_object is the float64
    inverse of the ROUNDED object_to_world, rounded."""
    out = copy.copy(sphere)
    o2w = (np.asarray(m64, np.float64) @ np.asarray(sphere["o2w"], np.float64).reshape(4, 4)).astype(F)
    out["o2w"] = o2w
    out["w2o"] = np.linalg.inv(o2w.astype(np.float64)).astype(F)
    if radius is not None:
        out["radius"] = float(F(radius))
    return out


def _about(centre, m):
    t, ti = np.eye(4), np.eye(4)
    t[:3, 3], ti[:3, 3] = centre, -np.asarray(centre)
    return t @ m @ ti


MOVES = ("translation", "rotation", "scale", "mirror")


def moved_spheres(spheres, move, amount=0.03):
    """Every sphere of the list moved: a translation of `amount`, a rotation about a tilted axis through a point beside the
    sphere, a non-uniform scale about its centre, or a mirrored transform (x -> -x about its centre) with a translation."""
    out = []
    for k, s in enumerate(spheres):
        c = np.asarray(s["o2w"], np.float64).reshape(4, 4)[:3, 3]
        if move == "translation":
            m = np.eye(4)
            m[:3, 3] = amount * np.array([1.0, 0.37 * (k + 1), -0.61])
        elif move == "rotation":
            m = _about(c + amount * np.array([0.5, 0.25, 1.0]), _rotation((0.3, 1.0, 0.45), 0.4 + 0.1 * k))
        elif move == "scale":
            m = _about(c, np.diag([1.3, 0.7 + 0.05 * k, 1.1, 1.0]))
        elif move == "mirror":
            m = _about(c, np.diag([-1.0, 1.0, 1.0, 1.0]))
            m[:3, 3] += amount * np.array([0.2, 0.1, 0.3])
        else:
            raise ValueError(move)
        out.append(transformed(s, m))
    return out
