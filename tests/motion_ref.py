"""An independent numpy float32 restatement of the motion passes (the rule of yuki_amd/csrc/yk_motion.h and of
tp_reproject_moved_pixel in yk_temporal.h), one operation per statement, a whole film per step.  It never calls the product.
The tap rule of the reprojection is unchanged, so it is temporal_ref's.  Shared by tests/test_motion.py (host instance) and
tests/test_gpu_motion.py (device instance), which also take their ids, vertex arrays and moved scenes from here."""
import numpy as np

import temporal_ref
from denoise_ref import GUIDE_DTYPE, bits, canon  # noqa: F401
from temporal_ref import HISTORY_DTYPE  # noqa: F401

F = np.float32
SURFACE_NONE = 0xFFFFFFFF
SURFACE_ID_DTYPE = np.dtype([("shape", "<u4"), ("b", "<f4", 3)])
MOTION_DTYPE = np.dtype([("p_prev", "<f4", 3), ("known", "<f4")])


def surface_motion(ids, guides, indices, prev_points, n_triangles, n_spheres):
    """(h, w) SURFACE_ID_DTYPE, (h, w) GUIDE_DTYPE, the scene's (n_triangles, 3) indices, the previous (n_vertices, 3)
    float32 points -> (h, w) MOTION_DTYPE."""
    with np.errstate(all="ignore"):
        shape = ids["shape"].astype(np.int64)
        live = (ids["shape"] != np.uint32(SURFACE_NONE)) & (guides["hit"] != F(0)) & (shape < n_triangles + n_spheres)
        tri = live & (shape < n_triangles)
        out = np.zeros(ids.shape, MOTION_DTYPE)
        pb = out["p_prev"].view(np.uint32)  # written as bits: copied values keep theirs
        sphere = live & ~tri
        pb[sphere] = bits(np.ascontiguousarray(guides["p"]))[sphere]
        if n_triangles:
            prev = np.asarray(prev_points, np.float32).reshape(-1, 3)
            idx = np.asarray(indices).reshape(-1, 3).astype(np.int64)[np.where(tri, shape, 0)]
            b = ids["b"]
            t0 = (prev[idx[..., 0]] * b[..., 0:1]).astype(np.float32)
            t1 = (prev[idx[..., 1]] * b[..., 1:2]).astype(np.float32)
            t2 = (prev[idx[..., 2]] * b[..., 2:3]).astype(np.float32)
            s = (t0 + t1).astype(np.float32)
            q = canon((s + t2).astype(np.float32))
            pb[tri] = bits(np.ascontiguousarray(q))[tri]
        out["known"] = np.where(live, F(1), F(0))
        return out


def reproject_moved(history, prev_guides, prev_camera, guides, motion, plane_tolerance, normal_cos_min):
    """temporal_ref.reproject with the pixel's point replaced by motion.p_prev and a pixel without a previous position
    treated as a miss; the normal and the hit flag stay the current guide's."""
    g = np.array(guides, GUIDE_DTYPE, copy=True)
    g["p"] = motion["p_prev"]
    g["hit"] = np.where(motion["known"] == F(0), F(0), guides["hit"])
    return temporal_ref.reproject(history, prev_guides, prev_camera, g, plane_tolerance, normal_cos_min)


# ------------------------------------------------------------------ ids, vertex arrays and moved scenes of both suites
SCENES = {"cornell": (37, 23), "city-small": (64, 36)}  # name -> (w, h) of its film in the scene tests


def solved_ids(shape, p, hit, points, indices, n_triangles):
    """Surface ids from first-hit shapes (int, -1 on a miss) and points: a triangle's barycentrics solved in float64 from p
    (least squares over the triangle's plane) and rounded; a sphere and a miss carry zeros.  They only have to be the same
    numbers on both sides of a comparison."""
    shape = np.asarray(shape).reshape(-1).astype(np.int64)
    p = np.asarray(p, np.float64).reshape(-1, 3)
    hit = np.asarray(hit).reshape(-1) != 0
    ids = np.zeros(shape.size, SURFACE_ID_DTYPE)
    ids["shape"] = np.where(hit & (shape >= 0), shape, SURFACE_NONE).astype(np.uint32)
    tri = hit & (shape >= 0) & (shape < n_triangles)
    if tri.any():
        v = np.asarray(points, np.float64).reshape(-1, 3)[np.asarray(indices).reshape(-1, 3).astype(np.int64)[shape[tri]]]  # (k, 3 vertices, 3)
        e1, e2, ep = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], p[tri] - v[:, 0]
        d11, d12, d22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
        r1, r2 = (ep * e1).sum(-1), (ep * e2).sum(-1)
        det = d11 * d22 - d12 * d12
        b1 = (r1 * d22 - r2 * d12) / det
        b2 = (r2 * d11 - r1 * d12) / det
        ids["b"][tri] = np.stack([1.0 - b1 - b2, b1, b2], -1).astype(np.float32)
    return ids


def synthetic_ids(rng, w, h, n_triangles, n_spheres, out_of_range=True):
    """Ids of every kind over a film: triangles, spheres, misses, and — with out_of_range — shapes n_shapes, n_shapes + 1 and
    0xfffffffe; barycentrics ordinary, NaN, +-inf, -0 and 1e30.  The matching guides: hits with random points, scattered
    misses (also under ids that are not misses)."""
    n_shapes = n_triangles + n_spheres
    ids = np.zeros((h, w), SURFACE_ID_DTYPE)
    ids["shape"] = rng.integers(0, max(n_shapes, 1), size=(h, w)).astype(np.uint32)
    b = rng.random((h, w, 3), dtype=np.float32)
    b /= b.sum(-1, keepdims=True)
    pool = np.array([np.nan, np.inf, -np.inf, -0.0, 1e30], np.float32)
    pick = rng.random((h, w, 3)) < 0.1
    b[pick] = pool[rng.integers(0, len(pool), size=int(pick.sum()))]
    ids["b"] = b
    special = [SURFACE_NONE] + ([n_shapes, n_shapes + 1, 0xFFFFFFFE] if out_of_range else [])
    if n_spheres:
        special += [n_triangles, n_shapes - 1]
    if n_triangles:
        special += [0, n_triangles - 1]
    pick = rng.random((h, w)) < (0.3 if w * h > 1 else 0.0)
    ids["shape"][pick] = np.array(special, np.uint32)[rng.integers(0, len(special), size=int(pick.sum()))]
    g = np.zeros((h, w), GUIDE_DTYPE)
    g["hit"] = (rng.random((h, w)) > 0.1).astype(np.float32)
    g["ns"] = rng.standard_normal((h, w, 3)).astype(np.float32)
    g["p"] = rng.standard_normal((h, w, 3)).astype(np.float32)
    g["p"].reshape(-1).view(np.uint32)[::17] = 0x7FA12345  # a signalling NaN with a payload: a sphere's p is only copied
    g["t"] = rng.random((h, w), dtype=np.float32)
    return ids, g


def rough_points(rng, points):
    """The previous vertex array of the synthetic cases: the scene's points shifted a little, with NaN, +-inf and 1e30
    scattered through them."""
    p = (np.asarray(points, np.float32) + rng.standard_normal(np.shape(points)).astype(np.float32) * F(0.05)).astype(np.float32)
    flat = p.reshape(-1)
    pool = np.array([np.nan, np.inf, -np.inf, 1e30], np.float32)
    pick = rng.random(flat.size) < 0.02
    flat[pick] = pool[rng.integers(0, len(pool), size=int(pick.sum()))]
    return p


def unlit_vertices(sd):
    """A mask of the vertices that belong to no triangle carrying an area light (an update does not move a light's record)."""
    al = np.asarray(sd.tri_area_light) if sd.tri_area_light is not None else np.zeros(0, np.int32)
    lit = np.unique(np.asarray(sd.indices)[np.nonzero(al >= 0)[0]].reshape(-1)).astype(np.int64)
    keep = np.ones(np.asarray(sd.points).shape[0], bool)
    keep[lit] = False
    return keep


def slid_points(sd, fraction, diag):
    """Quality case (a): every vertex that is on no area-light triangle moved by fraction x diag along the camera's side vector
    (forward x up)."""
    a = sd.camera
    fwd = np.subtract(a["target"], a["position"]).astype(np.float64)
    side = np.cross(fwd, np.array(a["up"], np.float64))
    side *= fraction * diag / np.linalg.norm(side)
    p = np.ascontiguousarray(sd.points, dtype=np.float32).copy()
    keep = unlit_vertices(sd)
    p[keep] = (p[keep] + side.astype(np.float32)).astype(np.float32)
    return p
