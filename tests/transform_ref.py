"""The rule of yk_scene_transform restated in numpy; written from the specification in include/yuki_hip.h, it never calls
the product.  Arithmetic is float32 with one operation a statement (numpy rounds every binary operation on float32 arrays
to float32: nothing is fused), the tree cost is float64.

Records are abi.MESH_TRANSFORM_DTYPE: rest_to_world and world_to_rest, row-major, one per mesh.  A vertex belongs to the one
mesh whose triangles index it (none: it keeps its rest bits).  A record whose rest_to_world equals the identity entry by
entry (== : -0 counts as 0) gives the rest pose's bits; any other gives Transform * Point3 (with the w == 1 test and the
division) and Transform * Normal (the inverse, transposed through the accesses, not renormalised), and flips the mesh's
swaps_handedness flag when the upper 3 x 3 determinant of rest_to_world is negative."""
import numpy as np

F = np.float32
NO_MESH = 0xFFFFFFFF
MESH_SWAPS = 4  # YK_MESH_SWAPS


def vertex_mesh_table(indices, tri_mesh, n_vertices):
    """-> (lo, hi) uint32 per vertex: the smallest and the largest mesh of the triangles that index it, (NO_MESH, 0) where
    none does.  lo != hi (and lo != NO_MESH) says the vertex is shared by two meshes."""
    idx = np.asarray(indices).reshape(-1, 3).astype(np.int64)
    tm = np.zeros(len(idx), np.uint32) if tri_mesh is None else np.asarray(tri_mesh).astype(np.uint32)
    lo, hi = np.full(n_vertices, NO_MESH, np.uint32), np.zeros(n_vertices, np.uint32)
    for k in range(3):
        np.minimum.at(lo, idx[:, k], tm)
        np.maximum.at(hi, idx[:, k], tm)
    return lo, hi


def shared_vertices(lo, hi):
    return (lo != NO_MESH) & (lo != hi)


def is_identity(m):
    return bool(np.all(np.asarray(m, dtype=F).reshape(16) == np.eye(4, dtype=F).reshape(16)))


def xf_point(m, p):
    """Transform * Point3 (math/transform.rs): m is 16 floats row-major, p is (n, 3) float32."""
    m = np.asarray(m, dtype=F).reshape(16)
    x, y, z = p[:, 0].astype(F), p[:, 1].astype(F), p[:, 2].astype(F)
    rows = []
    for r in range(4):
        a = m[4 * r] * x
        b = m[4 * r + 1] * y
        c = m[4 * r + 2] * z
        s = a + b
        s = s + c
        s = s + m[4 * r + 3]
        rows.append(s.astype(F))
    xp, yp, zp, wp = rows
    out = np.stack([xp, yp, zp], axis=1).astype(F)
    div = wp != F(1.0)
    with np.errstate(all="ignore"):
        out[div] = (out[div] / wp[div][:, None]).astype(F)
    return out


def xf_normal(mi, n):
    """Transform * Normal: the INVERSE matrix mi, transposed through the accesses; not renormalised."""
    mi = np.asarray(mi, dtype=F).reshape(16)
    x, y, z = n[:, 0].astype(F), n[:, 1].astype(F), n[:, 2].astype(F)
    cols = []
    for c in range(3):
        a = mi[c] * x
        b = mi[4 + c] * y
        d = mi[8 + c] * z
        s = a + b
        s = s + d
        cols.append(s.astype(F))
    return np.stack(cols, axis=1).astype(F)


def swaps_handedness(m):
    m = np.asarray(m, dtype=F).reshape(16)
    a = m[5] * m[10]
    b = m[6] * m[9]
    c = m[4] * m[10]
    d = m[6] * m[8]
    e = m[4] * m[9]
    f = m[5] * m[8]
    t0 = m[0] * F(a - b)
    t1 = m[1] * F(c - d)
    t2 = m[2] * F(e - f)
    det = F(F(t0 - t1) + t2)
    return bool(det < F(0.0))


def transform(sd, records):
    """The scene data's rest pose under `records` -> (points, normals or None, flipped), flipped: a bool per mesh."""
    rest = np.ascontiguousarray(sd.points, dtype=F)
    lo, _ = vertex_mesh_table(sd.indices, sd.tri_mesh, len(rest))
    points = rest.copy()
    normals = None if sd.normals is None else np.ascontiguousarray(sd.normals, dtype=F).copy()
    flipped = np.zeros(len(records), bool)
    with np.errstate(all="ignore"):
        for m, rec in enumerate(records):
            if is_identity(rec["rest_to_world"]):
                continue
            flipped[m] = swaps_handedness(rec["rest_to_world"])
            mine = np.nonzero(lo == m)[0]
            if len(mine):
                points[mine] = xf_point(rec["rest_to_world"], rest[mine])
                if normals is not None:
                    normals[mine] = xf_normal(rec["world_to_rest"], np.ascontiguousarray(sd.normals, dtype=F)[mine])
    return points, normals, flipped


def flipped_meshes(sd, flipped):
    """sd.meshes with swaps_handedness flipped where `flipped` says so."""
    return [(hn, hu, bool(sw) != bool(f)) for (hn, hu, sw), f in zip(sd.meshes, flipped)]


def tree_cost(nodes):
    """( sum over interior nodes of A + sum over leaves of A * count ) / A(root) in float64, summed in node order;
    A = 2 (dx dy + dy dz + dz dx) of the float box converted to double; 0 when A(root) is not > 0."""
    lo = np.asarray(nodes["bmin"], dtype=np.float64)
    hi = np.asarray(nodes["bmax"], dtype=np.float64)
    d = hi - lo
    area = 2.0 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0])
    interior, leaf = 0.0, 0.0
    for i in range(len(nodes)):
        if nodes["is_leaf"][i]:
            leaf += float(area[i]) * float(nodes["count"][i])
        else:
            interior += float(area[i])
    return (interior + leaf) / float(area[0]) if area[0] > 0.0 else 0.0


def cost_bound(n_nodes, value):
    """|device - host| <= n_nodes * 2^-51 * host: equal non-negative terms, two sums in different orders and a division."""
    return n_nodes * 2.0 ** -51 * value
