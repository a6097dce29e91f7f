"""Traversal against geometry (no GPU): the oracle's BoundingVolumeHierarchy::intersect / any_intersect
(bvh.rs:160-302) against the float64 brute force of tests/trace_ref.py, and the host BVH (yk_scene_export_bvh)
against the primitives it bounds.  Every other traversal test compares two restatements of the same tree;
these compare the tree walk with plain geometry, so a bound or a leaf range wrong on both sides is caught.

The ray sets are shared with tests/test_gpu_trace_kernels.py."""
import os
import sys

import numpy as np
import pytest

import trace_ref
from yuki_amd import abi, scenes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

F = np.float32
SEED = 0x5EED7


# ------------------------------------------------------------------ scenes
def _single_triangle():
    base = scenes.by_name("city-tiny")
    return scenes.SceneData(points=base.points[:3].copy(), indices=np.array([[0, 1, 2]], dtype=np.uint32), tri_mesh=np.zeros(1, np.uint32),
                            tri_material=np.zeros(1, np.int32), tri_area_light=np.full(1, -1, np.int32), meshes=[(False, False, False)],
                            materials=base.materials[:1], lights=base.lights, camera=dict(position=(1.5, 2.0, 3.0), target=(0.5, 0.0, 0.2), up=(0, 1, 0), fov_axis=abi.FOV_X, fov_degrees=60.0),
                            name="single-triangle")


def _duplicated_triangles():
    s = _single_triangle()
    s.indices = np.array([[0, 1, 2]] * 7, dtype=np.uint32)
    s.tri_mesh, s.tri_material, s.tri_area_light = np.zeros(7, np.uint32), np.zeros(7, np.int32), np.full(7, -1, np.int32)
    s.name = "duplicated-triangles"
    return s


def _glass_balls_transformed():
    """glass-balls with its spheres rotated and scaled non-uniformly: world bounds and the w2o ray
    transform away from pure translations (sphere.rs:38-39,121-123)."""
    s = scenes.by_name("glass-balls")
    out = []
    for k, sph in enumerate(s.spheres):
        a = 0.4 + 0.7 * k
        c, sn = np.cos(a), np.sin(a)
        rot = np.array([[c, -sn, 0, 0], [sn, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]) @ np.array([[1, 0, 0, 0], [0, c, -sn, 0], [0, sn, c, 0], [0, 0, 0, 1]])
        m = np.asarray(sph["o2w"], dtype=np.float64) @ rot @ np.diag([1.0 + 0.3 * k, 0.6, 1.4 - 0.2 * k, 1.0])
        out.append(dict(sph, o2w=m.astype(F), w2o=np.linalg.inv(m).astype(F)))
    s.spheres = out
    s.name = "glass-balls-xf"
    return s


def scene_by_name(name):
    if name == "single-triangle":
        return _single_triangle()
    if name == "duplicated-triangles":
        return _duplicated_triangles()
    if name == "glass-balls-xf":
        return _glass_balls_transformed()
    if name.startswith("fuzz-"):
        import parity_fuzz

        return parity_fuzz.random_scene(int(name.split("-")[1]))
    return scenes.by_name(name)


# scenes whose ties between different surfaces at one distance are part of the scene, so fewer rays are robust:
# Cornell's ceiling is four overlapping coplanar quads around the light hole (scene/mod.rs); deep-chain's planes
# x = 3^-k lie closer together than f32 rounding of t for large k
MIN_ROBUST = {"cornell": 0.85, "cornell-tris": 0.85, "glass-balls": 0.85, "glass-balls-xf": 0.85, "deep-chain-60": 0.7}
SCENES = ["cornell", "cornell-tris", "glass-balls", "glass-balls-xf", "city-small", "cfg2", "deep-chain-60", "single-triangle", "duplicated-triangles", "fuzz-1", "fuzz-2", "fuzz-3"]


# ------------------------------------------------------------------ ray sets
def random_rays(sd, n, seed):
    """Origins in the scene's box grown by 30 % on every side, towards points inside it; 5 % axis-aligned,
    5 % with one zero component (as tests/test_gpu_stages.py)."""
    rng = np.random.default_rng(seed)
    lo, hi = sd.points.min(axis=0), sd.points.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3)
    o = (lo - 0.3 * ext + rng.uniform(0, 1, (n, 3)) * 1.6 * ext).astype(F)
    tgt = (lo + rng.uniform(0, 1, (n, 3)) * ext).astype(F)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    k = n // 20
    d[:k] = 0
    d[np.arange(k), rng.integers(0, 3, k)] = rng.choice([-1.0, 1.0], k)
    d[k : 2 * k, rng.integers(0, 3)] = 0
    d[~d.any(axis=1)] = (1.0, 0.0, 0.0)
    return o, d.astype(F)


def camera_rays(oracle, sd, res, sample_index, seed=SEED):
    """Camera::ray for every pixel of a res film at one sample index (the oracle's camera, camera.rs:105-114)."""
    from yuki_amd import core as yk

    cam = yk.Camera(sd.camera, yk.FilmSettings(res=res))
    s = yk.SamplerType.Stratified((8, 8), True, seed)
    return oracle.camera_rays(cam.matrices, s, (0, 0, res[0], res[1]), sample_index)


def pixel_bundles(oracle, sd, res, pixels):
    """The 64 camera samples of each pixel in `pixels` (flat indices of a res film), pixel-major: one
    pixel per 64-ray packet, as the render's camera bounce forms them."""
    per = [camera_rays(oracle, sd, res, i) for i in range(64)]
    o = np.stack([p[0][pixels] for p in per], axis=1).reshape(-1, 3)
    d = np.stack([p[1][pixels] for p in per], axis=1).reshape(-1, 3)
    return o, d


def centroid_rays(sd, n, seed):
    """From random origins around the scene towards random triangle centroids (hits by construction)."""
    rng = np.random.default_rng(seed)
    lo, hi = sd.points.min(axis=0), sd.points.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3)
    tri = rng.integers(0, sd.n_triangles, n)
    c = sd.points[sd.indices[tri]].astype(np.float64).mean(axis=1)
    o = (lo - 0.3 * ext + rng.uniform(0, 1, (n, 3)) * 1.6 * ext).astype(F)
    d = (c - o).astype(F)
    d[~d.any(axis=1)] = (1.0, 0.0, 0.0)
    return o, d


def shadow_segments(sd, n, seed):
    """Segments from random points in the scene's box to random points on area-light triangles, as
    Path's light sampling makes them: unnormalised d, t_max = 1 - 1e-4 (short of the light) or 2 (through it),
    area_light the target's light (the right one) or another value (-1 or a different light).
    -> (o, d, t_max, right_light, wrong_light) or None without area lights."""
    lit = np.nonzero(np.asarray(sd.tri_area_light) >= 0)[0]
    if len(lit) == 0:
        return None
    rng = np.random.default_rng(seed)
    lo, hi = sd.points.min(axis=0), sd.points.max(axis=0)
    o = (lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)).astype(F)
    tri = lit[rng.integers(0, len(lit), n)]
    b = rng.dirichlet((1.0, 1.0, 1.0), n)
    p = np.einsum("ij,ijk->ik", b, sd.points[sd.indices[tri]].astype(np.float64))
    d = (p - o).astype(F)
    d[~d.any(axis=1)] = (1.0, 0.0, 0.0)
    t_max = np.where(rng.random(n) < 0.5, F(1.0 - 1e-4), F(2.0)).astype(F)
    right = np.asarray(sd.tri_area_light)[tri].astype(np.int32)
    wrong = np.where(rng.random(n) < 0.5, -1, (right + 1) % max(1, len(sd.lights))).astype(np.int32)
    return o, d, t_max, right, wrong


def ray_sets(oracle, sd, name, scale=1.0):
    """-> list of (label, o, d, t_max or None) closest-hit sets, and (label, o, d, t_max, area_light) any-hit sets."""
    n = max(64, int(2000 * scale))
    closest, anyhit = [], []
    o, d = random_rays(sd, n, SEED)
    closest.append(("random", o, d, None))
    if sd.camera is not None:
        co, cd = camera_rays(oracle, sd, (40, 30), 5)
        sel = np.random.default_rng(SEED).permutation(len(co))[: max(64, int(1200 * scale))]
        closest.append(("camera", co[sel], cd[sel], None))
    co, cd = centroid_rays(sd, n // 2, SEED + 1)
    closest.append(("centroid", co, cd, None))
    diag = float(np.linalg.norm(sd.points.max(axis=0) - sd.points.min(axis=0)))
    tm = np.random.default_rng(SEED + 2).uniform(0.0, 1.5 * diag, n).astype(F)
    closest.append(("finite t_max", o, d, tm))
    rng = np.random.default_rng(SEED + 3)
    al = rng.integers(-1, max(1, len(sd.lights)), n).astype(np.int32)
    anyhit.append(("random", o, d, tm, al))
    seg = shadow_segments(sd, n // 2, SEED + 4)
    if seg is not None:
        so, sdir, stm, right, wrong = seg
        anyhit.append(("shadow, right light", so, sdir, stm, right))
        anyhit.append(("shadow, wrong light", so, sdir, stm, wrong))
    return closest, anyhit


def canon_shape(ref, shape):
    shape = np.asarray(shape)
    return np.where(shape >= 0, ref.canon[np.maximum(shape, 0)], -1)


def check_closest(ref, label, o, d, t_max, shape, t):
    """Asserts a traversal's (shape, t) against the f64 reference on its robust rays; -> (robust, robust hit) masks."""
    r = ref.closest(o, d, t_max)
    rob, hit = r["robust"], r["shape"] >= 0
    got = canon_shape(ref, shape)
    bad = rob & (got != r["shape"])
    assert not bad.any(), (label, "shape", int(bad.sum()), np.nonzero(bad)[0][:5], got[bad][:5], r["shape"][bad][:5])
    if t is not None:
        # the nearest hit's distance, where it is well defined (ties of coplanar surfaces included)
        sel = r["robust_t"]
        err = np.abs(np.asarray(t, np.float64)[sel] - r["t"][sel])
        tol = np.maximum(1e-5 * r["t"][sel], r["dt"][sel])
        assert (err <= tol).all(), (label, "t", int((err > tol).sum()), float((err / r["t"][sel]).max()))
        # ... and the traversal's own shape lies on it
        ts = ref.t_of(o[sel], d[sel], np.asarray(shape)[sel])
        err = np.abs(ts - r["t"][sel])
        assert (err <= tol).all(), (label, "shape not on the first surface", int((~(err <= tol)).sum()))
    return rob, rob & hit


def check_any(ref, label, o, d, t_max, al, hit):
    r = ref.any(o, d, t_max, al)
    bad = r["robust"] & (np.asarray(hit).astype(bool) != r["hit"])
    assert not bad.any(), (label, "any", int(bad.sum()), np.nonzero(bad)[0][:5])
    return r["robust"]


# ------------------------------------------------------------------ oracle against the f64 reference
@pytest.mark.parametrize("name", SCENES)
def test_oracle_traversal_matches_f64_brute_force(oracle, name):
    sd = scene_by_name(name)
    ref = trace_ref.TraceRef(sd)
    osc = oracle.OracleScene(sd)
    closest, anyhit = ray_sets(oracle, sd, name, scale=0.5 if name == "cfg2" else 1.0)
    rob, rhit = [], []
    for label, o, d, tm in closest:
        w = osc.intersect(o, d, tm)
        a, b = check_closest(ref, label, o, d, tm, w["shape"], w["t"])
        if label == "centroid":
            assert b.mean() > 0.5, (label, float(b.mean()))  # aimed at centroids: robust hits by construction
        rob.append(a)
        rhit.append(b)
    arob = []
    for label, o, d, tm, al in anyhit:
        arob.append(check_any(ref, label, o, d, tm, al, osc.any_intersect(o, d, tm, al)))
    rob, rhit, arob = np.concatenate(rob), np.concatenate(rhit), np.concatenate(arob)
    print(f"{name}: {len(rob)} closest-hit rays, {rob.mean():.3f} robust, {rhit.mean():.3f} robust hits; {len(arob)} any-hit rays, {arob.mean():.3f} robust")
    assert rob.mean() >= MIN_ROBUST.get(name, 0.9), (name, float(rob.mean()))
    assert rhit.mean() >= 0.3, (name, float(rhit.mean()))
    assert arob.mean() >= MIN_ROBUST.get(name, 0.9), (name, float(arob.mean()))


def coplanar_rays(n, seed):
    """Random origins around the coplanar-slabs scene towards random points of its box: every direction-sign
    group, not camera rays."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-2.5, 2.5, (n, 3)).astype(F)
    d = (rng.uniform(-1.5, 1.5, (n, 3)) - o).astype(F)
    return o, d


def test_oracle_coplanar_slabs_hits_the_first_plane(oracle):
    """Three slabs of overlapping coplanar triangles: which triangle wins a tie is rounding, so the shape is
    not asserted; the distance is: the oracle's t and its triangle lie on the first plane the ray meets."""
    sd = scenes.by_name("coplanar-slabs")
    ref = trace_ref.TraceRef(sd)
    o, d = coplanar_rays(6000, SEED)
    w = oracle.OracleScene(sd).intersect(o, d)
    r = ref.closest(o, d)
    sel = r["robust_t"]
    assert sel.mean() > 0.2, float(sel.mean())
    err = np.abs(w["t"][sel].astype(np.float64) - r["t"][sel])
    tol = np.maximum(1e-5 * r["t"][sel], r["dt"][sel])
    assert (err <= tol).all()
    ts = ref.t_of(o[sel], d[sel], w["shape"][sel])
    assert (np.abs(ts - r["t"][sel]) <= tol).all()
    assert (w["shape"][r["robust"] & (r["shape"] < 0)] == -1).all()
    print(f"coplanar-slabs: {sel.mean():.3f} of the rays with a well-defined first plane, {(r['robust'] & (r['shape'] < 0)).mean():.3f} robust misses")


# ------------------------------------------------------------------ BVH invariants against the geometry
def _shape_bounds(sd):
    """f64 world bounds: triangles (triangle.rs:229-235, exact), spheres (sphere.rs:121-123: o2w of the
    object box, its 8 corners)."""
    p = sd.points[sd.indices].astype(np.float64)
    lo, hi = [p.min(axis=1)], [p.max(axis=1)]
    for s in sd.spheres:
        r = float(np.float32(s["radius"]))
        corners = np.array([[x, y, z, 1.0] for x in (-r, r) for y in (-r, r) for z in (-r, r)])
        w = corners @ np.asarray(s["o2w"], dtype=np.float64).reshape(4, 4).T
        w = w[:, :3] / w[:, 3:]
        lo.append(w.min(axis=0)[None])
        hi.append(w.max(axis=0)[None])
    return np.concatenate(lo), np.concatenate(hi)


@pytest.mark.parametrize("name", ["cornell", "glass-balls", "glass-balls-xf"])
@pytest.mark.parametrize("method", [abi.SPLIT_SAH, abi.SPLIT_MIDDLE, abi.SPLIT_EQUAL_COUNTS])
@pytest.mark.parametrize("max_shapes", [1, 4])
def test_bvh_bounds_its_geometry(yk, name, method, max_shapes):
    sd = scene_by_name(name)
    sd.split_method, sd.max_shapes_in_node = method, max_shapes
    hs = yk.Scene(None, sd)
    nodes, order = hs.export_bvh()
    n_shapes = sd.n_triangles + len(sd.spheres)
    assert sorted(order.tolist()) == list(range(n_shapes))
    slo, shi = _shape_bounds(sd)
    bmin, bmax = nodes["bmin"].astype(np.float64), nodes["bmax"].astype(np.float64)
    seen = np.zeros(n_shapes, dtype=np.int64)
    visited = np.zeros(len(nodes), dtype=np.int64)
    depth = 0
    stack = [(0, 1)]
    while stack:
        i, lvl = stack.pop()
        visited[i] += 1
        depth = max(depth, lvl)
        nd = nodes[i]
        if nd["is_leaf"]:
            a, c = int(nd["a"]), int(nd["count"])
            assert 1 <= c and a + c <= n_shapes
            src = order[a : a + c]
            seen[src] += 1
            tri = src[src < sd.n_triangles]
            sph = src[src >= sd.n_triangles]
            # triangles: f32 vertices, so the node's f32 bounds must hold them exactly
            assert (bmin[i] <= slo[tri]).all() and (bmax[i] >= shi[tri]).all(), (i, "triangle outside its leaf")
            # spheres: the f32 transform of the object box rounds; 1e-6 relative slack
            slack = 1e-6 * np.maximum(1.0, np.abs(np.concatenate([slo[sph], shi[sph]])).max(initial=1.0))
            assert (bmin[i] <= slo[sph] + slack).all() and (bmax[i] >= shi[sph] - slack).all(), (i, "sphere outside its leaf")
        else:
            for ch in (i + 1, int(nd["a"])):
                assert (bmin[ch] >= bmin[i]).all() and (bmax[ch] <= bmax[i]).all(), (i, ch, "child outside its parent")
                stack.append((ch, lvl + 1))
    assert (visited == 1).all(), "every node is reached exactly once"
    assert (seen == 1).all(), "the leaves partition the shapes"
    assert hs.info().tree_depth == depth
