"""Integrator::li_debug (yk_li_debug, k_path_debug) and the ShadingUVs integrator on the device.

li_debug's radiance is pinned to yk_li and the oracle bit for bit, and its ray records are checked bounce by bounce
against independent geometry: Scene.intersect's hits, a float32 restatement of the root box's slab test
(bounds.rs:176-206), spawn_ray / spawn_ray_to (interaction.rs:27-59) and the point lights' positions."""
import os
import sys

import numpy as np
import pytest

from yuki_amd import abi, scenes
from yuki_amd._ffi import YukiError

pytestmark = pytest.mark.gpu
SEED = 0x5EED
F = np.float32
DIRECT, REFLECTION, REFRACTION, NORMAL, SHADOW = range(5)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    return bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _matte_box_with_light_behind_wall():
    """Cornell (triangles, glass box turned matte) with a point light behind the back wall: the wall's visible face gets a
    non-black li from it while f is black (wi lies below the surface), so path.rs:103-113 records a shadow ray it never traces."""
    s = scenes.cornell_triangles_only()
    s.materials = [m if m["kind"] != abi.MAT_GLASS else dict(kind=abi.MAT_MATTE, a=(0.5, 0.5, 0.5), c=0.0) for m in s.materials]
    l2w = np.eye(4, dtype=F)
    l2w[:3, 3] = (0.278, 0.273, -0.9)
    s.lights = list(s.lights) + [dict(kind="point", l2w=l2w, I=(0.4, 0.4, 0.4))]
    s.name = "cornell-light-behind-wall"
    return s


def _camera_samples(yk, ctx, sd, sampler, tile, ks):
    fs = yk.FilmSettings(res=(64, 64), tile_dim=64)
    cam = yk.Camera(sd.camera, fs)
    x0, y0, x1, y1 = tile
    xy = np.stack(np.meshgrid(np.arange(x0, x1), np.arange(y0, y1), indexing="xy"), axis=-1).reshape(-1, 2).astype(np.uint16)
    os_, ds, pix, si = [], [], [], []
    for k in ks:
        o, d = yk.camera_rays(ctx, cam, sampler, tile, k)
        os_.append(o)
        ds.append(d)
        pix.append(xy)
        si.append(np.full(len(o), k, dtype=np.uint32))
    return cam, np.concatenate(os_), np.concatenate(ds), np.concatenate(pix), np.concatenate(si)


def _tools():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import parity_fuzz
    import stage_fuzz

    return parity_fuzz, stage_fuzz


# ------------------------------------------------------------------ 1. li and counts
@pytest.mark.parametrize("name", ["city-tiny", "cornell", "glass-balls", "light-behind-wall"])
def test_li_debug_equals_li_and_the_oracle(ctx, yk, oracle, name):
    sd = _matte_box_with_light_behind_wall() if name == "light-behind-wall" else scenes.by_name(name)
    sc = yk.Scene(ctx, sd)
    osc = oracle.OracleScene(sd)
    for sampler in (yk.SamplerType.Uniform(3, SEED), yk.SamplerType.Stratified((2, 2), True, SEED)):
        _, o, d, pix, si = _camera_samples(yk, ctx, sd, sampler, (16, 16, 40, 40), (0, 2))
        integ = yk.IntegratorType.Path(yk.PathParams(max_depth=6))
        it = yk.IntegratorType.instantiate(ctx, integ)
        li, counts, rays = it.li_debug(sc, sampler, o, d, pix, si)
        assert _same(li, it.li(sc, sampler, o, d, pix, si))
        want, want_counts = osc.li(sampler, integ, o, d, pix, si)
        assert _same(li, want)
        assert np.array_equal(counts, np.asarray(want_counts, dtype=np.uint32))
        segs = np.array([int(np.isin(r["ray_type"], (DIRECT, REFLECTION, REFRACTION)).sum()) for r in rays])
        assert np.array_equal(segs, counts)
    sc.close()


@pytest.mark.parametrize("seed", [3, 8, 13])
def test_li_debug_on_random_scenes_matches_the_oracle(oracle, yk, seed):
    """The inputs of test_li_on_random_rays_matches_the_oracle: random scenes and rays, both samplers, a random dimension."""
    parity_fuzz, stage_fuzz = _tools()
    ctx = parity_fuzz.variant_context(seed)
    sd = parity_fuzz.random_scene(seed)
    r = np.random.default_rng(seed ^ 0x11)
    o, d = stage_fuzz.rays_for(sd, r, n=600)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    smp = yk.SamplerType.Uniform(5, SEED) if seed % 2 else yk.SamplerType.Stratified((2, 3), True, SEED)
    pix = r.integers(0, 300, (len(o), 2)).astype(np.uint16)
    si = r.integers(0, yk.samples_per_pixel(smp), len(o)).astype(np.uint32)
    dim = int(r.integers(0, 7))
    sc = yk.Scene(ctx, sd)
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=int(r.integers(1, 8)), indirect_clamp=None if seed % 3 else 0.5))
    it = yk.IntegratorType.instantiate(ctx, integ)
    li, counts, _ = it.li_debug(sc, smp, o, d, pix, si, dimension=dim)
    assert _same(li, it.li(sc, smp, o, d, pix, si, dimension=dim))
    want, want_counts = oracle.OracleScene(sd).li(smp, integ, o, d, pix, si, dimension=dim)
    assert _same(li, want)
    assert np.array_equal(counts, np.asarray(want_counts, dtype=np.uint32))
    sc.close()


# ------------------------------------------------------------------ 2. one tile against the render
def test_li_debug_sums_to_the_rendered_tile(ctx, yk):
    sd = scenes.by_name("cornell")
    sc = yk.Scene(ctx, sd)
    sampler = yk.SamplerType.Stratified((2, 2), True, SEED)
    spp = 4
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=5))
    it = yk.IntegratorType.instantiate(ctx, integ)
    tile = (8, 16, 40, 48)
    cam, o, d, pix, si = _camera_samples(yk, ctx, sd, sampler, tile, range(spp))
    li, counts, _ = it.li_debug(sc, sampler, o, d, pix, si)
    n = 32 * 32
    acc = np.zeros((n, 3), dtype=np.float32)
    for k in range(spp):  # integrators/mod.rs:172-175: the samples in order, then / spp, in f32
        acc = (acc + li[k * n:(k + 1) * n]).astype(np.float32)
    acc = (acc / np.float32(spp)).astype(np.float32)
    px, rays = it.render(sc, cam, sampler, tile)
    assert _same(acc, px)
    assert int(counts.sum()) == rays
    sc.close()


# ------------------------------------------------------------------ 3. record structure
def _min_len(sc):
    info = sc.info()
    lo = np.array(info.bounds_min, dtype=np.float32)
    hi = np.array(info.bounds_max, dtype=np.float32)
    dd = (hi - lo).astype(np.float32)
    i = 0 if (dd[0] > dd[1] and dd[0] > dd[2]) else (1 if dd[1] > dd[2] else 2)  # Bounds3::maximum_extent
    return np.float32(np.float32(hi[i] - lo[i]) / np.float32(10.0)), lo, hi


def _root_exit(lo, hi, o, d, miss_len):
    """Bounds3::intersections (bounds.rs:176-206) in float32 with a ray t_max of inf; f32::min / max drop a NaN (np.fmin / fmax)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (np.float32(1.0) / d).astype(np.float32)
        t0 = ((lo - o) * inv).astype(np.float32)
        t1 = ((hi - o) * inv).astype(np.float32)
    n, f = np.fmin(t0, t1), np.fmax(t0, t1)
    tmin = np.fmax(np.fmax(n[0], np.fmax(n[1], n[2])), np.float32(0))
    tmax = np.fmin(np.fmin(f[0], np.fmin(f[1], f[2])), np.float32(np.inf))
    return np.float32(tmax) if tmin <= tmax else miss_len


def _spawn(p, n, d):
    off = (n * np.float32(0.001)).astype(np.float32)
    dot = np.float32(np.float32(np.float32(d[0] * n[0]) + np.float32(d[1] * n[1])) + np.float32(d[2] * n[2]))
    return (p + off).astype(np.float32) if dot > 0 else (p - off).astype(np.float32)


def _point_lights(sd):
    return [np.asarray(l["l2w"], dtype=np.float32)[:3, 3] for l in sd.lights if l["kind"] == "point"]


@pytest.mark.parametrize("name", ["cornell", "glass-balls", "light-behind-wall"])
def test_li_debug_records_follow_the_path(ctx, yk, name):
    sd = _matte_box_with_light_behind_wall() if name == "light-behind-wall" else scenes.by_name(name)
    sc = yk.Scene(ctx, sd)
    sampler = yk.SamplerType.Stratified((2, 2), True, SEED)
    _, o, d, pix, si = _camera_samples(yk, ctx, sd, sampler, (8, 8, 56, 56), (1,))
    max_depth = 6
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.Path(yk.PathParams(max_depth=max_depth)))
    li, counts, rays = it.li_debug(sc, sampler, o, d, pix, si)
    min_len, lo, hi = _min_len(sc)
    lights = _point_lights(sd)
    n_lights = len(sd.lights)
    assert all(len(r) <= max_depth * (2 + n_lights) for r in rays)
    # every traced segment of every sample, intersected once in a batch
    seg_o, seg_d, where = [], [], []
    for i, r in enumerate(rays):
        assert len(r) >= 1 and r["ray_type"][0] == DIRECT
        assert _same(r["o"][0], o[i]) and _same(r["d"][0], d[i])
        for j in np.nonzero(np.isin(r["ray_type"], (DIRECT, REFLECTION, REFRACTION)))[0]:
            seg_o.append(r["o"][j])
            seg_d.append(r["d"][j])
            where.append((i, j))
    hit = sc.intersect(np.array(seg_o), np.array(seg_d))
    types_seen = set()
    black_f = 0
    for k, (i, j) in enumerate(where):
        r = rays[i]
        rec = r[j]
        types_seen.add(int(rec["ray_type"]))
        if hit["shape"][k] < 0:
            want_t = np.float32(np.inf) if rec["ray_type"] == DIRECT else _root_exit(lo, hi, rec["o"], rec["d"], min_len)
            assert _same(rec["t_max"], want_t), (name, i, j)
            assert j == len(r) - 1  # a miss ends the path
            continue
        assert _same(rec["t_max"], hit["t"][k]), (name, i, j)
        nrm = r[j + 1]
        assert nrm["ray_type"] == NORMAL and _same(nrm["t_max"], min_len)
        p_ray = rec["o"].astype(np.float64) + hit["t"][k] * rec["d"].astype(np.float64)
        assert np.abs(nrm["o"] - p_ray).max() <= 1e-4 * (1.0 + np.abs(p_ray).max()), (name, i, j)
        assert abs(np.linalg.norm(nrm["d"].astype(np.float64)) - 1.0) < 1e-5
        q = j + 2
        shadows = 0
        while q < len(r) and r[q]["ray_type"] == SHADOW:
            s = r[q]
            types_seen.add(SHADOW)
            shadows += 1
            p, n = nrm["o"], nrm["d"]
            off = (n * np.float32(0.001)).astype(np.float32)
            assert _same(s["o"], (p + off).astype(np.float32)) or _same(s["o"], (p - off).astype(np.float32))
            assert _same(s["t_max"], np.float32(0.9999))
            for lp in lights:  # VisibilityTester::ray towards a point light: d = p1 - o exactly
                if _same(s["d"], (lp - s["o"]).astype(np.float32)):
                    assert _same(s["o"], _spawn(p, n, (lp - p).astype(np.float32)))
                    # all-matte scene: f is black when wi and wo lie on opposite sides of the geometric normal
                    if name == "light-behind-wall" and np.dot(s["d"].astype(np.float64), n) * np.dot(-rec["d"].astype(np.float64), n) < 0:
                        black_f += 1
            q += 1
        assert shadows <= n_lights
        types_seen.add(NORMAL)
        if q < len(r):  # the next segment leaves the vertex: Interaction::spawn_ray(wi)
            nxt = r[q]
            assert nxt["ray_type"] in (REFLECTION, REFRACTION)
            assert _same(nxt["o"], _spawn(nrm["o"], nrm["d"], nxt["d"])), (name, i, q)
    if name == "cornell":
        assert types_seen == {DIRECT, REFLECTION, REFRACTION, NORMAL, SHADOW}
    if name == "light-behind-wall":
        assert black_f > 0  # recorded though f is black and nothing was traced
    sc.close()


# ------------------------------------------------------------------ 4. capacity and errors
def test_li_debug_capacity_and_errors(ctx, yk):
    sd = scenes.by_name("glass-balls")
    sc = yk.Scene(ctx, sd)
    sampler = yk.SamplerType.Uniform(2, SEED)
    _, o, d, pix, si = _camera_samples(yk, ctx, sd, sampler, (20, 20, 36, 36), (0, 1))
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=7))
    it = yk.IntegratorType.instantiate(ctx, integ)
    full = 7 * (2 + len(sd.lights))
    li, counts, recs, n_rays = it.li_debug_records(sc, sampler, o, d, pix, si, 2, full)
    assert n_rays.max() <= full and n_rays.max() > 3
    li3, counts3, recs3, n_rays3 = it.li_debug_records(sc, sampler, o, d, pix, si, 2, 3)
    assert np.array_equal(n_rays3, n_rays) and np.array_equal(counts3, counts) and _same(li3, li)
    for i in range(len(o)):
        k = min(3, int(n_rays[i]))
        assert recs3[i, :k].tobytes() == recs[i, :k].tobytes()
        assert not recs3[i, k:].tobytes().strip(b"\0")
    li0, _, _, n_rays0 = it.li_debug_records(sc, sampler, o, d, pix, si, 2, 0)
    assert np.array_equal(n_rays0, n_rays) and _same(li0, li)
    for other in (yk.IntegratorType.Whitted(3), yk.IntegratorType.BVHIntersections, yk.IntegratorType.GeometryNormals, yk.IntegratorType.ShadingNormals,
                  yk.IntegratorType.ShadingUVs):
        with pytest.raises(YukiError) as e:
            yk.IntegratorType.instantiate(ctx, other).li_debug(sc, sampler, o, d, pix, si)
        assert e.value.status == 5  # YK_ERR_UNSUPPORTED: the trait's default in the reference
    with pytest.raises(YukiError) as e:
        it.li_debug_records(sc, sampler, o, d, pix, si, 2, (1 << 24) // len(o) + 1)
    assert e.value.status == 1  # n * ray_cap above YK_LI_DEBUG_MAX_RECORDS
    sc.close()
    deep = yk.Scene(ctx, scenes.deep_chain())
    with pytest.raises(YukiError) as e:
        it.li_debug(deep, sampler, np.array([[-1.0, 0.0, 0.0]], F), np.array([[1.0, 0.0, 0.0]], F), np.zeros((1, 2), np.uint16), np.zeros(1, np.uint32))
    assert e.value.status == 8  # YK_ERR_STACK_OVERFLOW
    deep.close()


# ------------------------------------------------------------------ 5. ShadingUVs
def _uv_render(yk, ctx, sd, res=64):
    fs = yk.FilmSettings(res=(res, res), tile_dim=res)
    cam = yk.Camera(sd.camera, fs)
    sampler = yk.SamplerType.Uniform(1, SEED)
    sc = yk.Scene(ctx, sd)
    it = yk.IntegratorType.instantiate(ctx, yk.IntegratorType.ShadingUVs)
    tiles = yk.film_tiles(fs)
    img, stats = it.render_tiles(sc, cam, sampler, tiles)
    assert stats.rays == res * res  # one ray per sample, as the other debug integrators
    o, d = yk.camera_rays(ctx, cam, sampler, (0, 0, res, res), 0)
    return sc, cam, sampler, tiles, it, img, o, d


@pytest.mark.parametrize("name", ["cornell-tris", "city-tiny"])
def test_shading_uvs_on_triangles(ctx, yk, name):
    """uv_hit = uv0 * b0 + uv1 * b1 + uv2 * b2 (triangle.rs:142-176), default uvs (0,0) (1,0) (1,1) where a mesh has none."""
    sd = scenes.by_name(name)
    sc, cam, sampler, tiles, it, img, o, d = _uv_render(yk, ctx, sd)
    hit = sc.intersect(o, d)
    want = np.zeros_like(img)
    for i in range(len(o)):
        s = int(hit["shape"][i])
        if s < 0:
            continue
        tri = sd.indices[s]
        if sd.meshes[int(sd.tri_mesh[s])][1]:
            uv = np.asarray(sd.uvs, dtype=np.float32)[tri]
        else:
            uv = np.array([[0, 0], [1, 0], [1, 1]], dtype=np.float32)
        b = hit["bary"][i].astype(np.float32)
        for c in range(2):
            want[i, c] = np.float32(np.float32(np.float32(uv[0, c] * b[0]) + np.float32(uv[1, c] * b[1])) + np.float32(uv[2, c] * b[2]))
    assert _same(img, want)
    # the same image through the accumulating film, the combiner and the combiner's accumulating path
    acc, _ = it.render_tiles_accumulating(sc, cam, sampler, tiles, np.zeros(len(tiles), dtype=np.uint16))
    assert _same(acc, img)
    comb = yk.Combiner([ctx])
    t = tiles[0]
    px, _ = comb.render(it, sc, cam, sampler, (t["x0"], t["y0"], t["x1"], t["y1"]))
    assert _same(px, img)
    comb.close()
    sc.close()


def test_shading_uvs_on_spheres(ctx, yk):
    """Sphere uv, sphere.rs:88-101: phi / phi_max and (theta - theta_min) / (theta_max - theta_min), in float64 from the hit t."""
    sd = scenes.by_name("glass-balls")
    sc, _, _, _, _, img, o, d = _uv_render(yk, ctx, sd)
    hit = sc.intersect(o, d)
    nt = sd.n_triangles
    checked = 0
    for i in np.nonzero(hit["shape"] >= nt)[0]:
        sp = sd.spheres[int(hit["shape"][i]) - nt]
        w2o = np.asarray(sp["w2o"], dtype=np.float64).reshape(4, 4)
        r = float(sp["radius"])
        p = w2o[:3, :3] @ (o[i].astype(np.float64) + float(hit["t"][i]) * d[i].astype(np.float64)) + w2o[:3, 3]
        p *= r / np.linalg.norm(p)
        if p[0] == 0 and p[1] == 0:
            p[0] = 1e-5 * r
        phi = np.arctan2(p[1], p[0])
        if phi < 0:
            phi += 2 * np.pi
        z = np.clip(p[2] / r, -1, 1)
        u, v = phi / (2 * np.pi), (np.arccos(z) - np.pi) / (0 - np.pi)
        # float32 inputs: near the axis (u) and the poles (v) the angles amplify their rounding
        tol_u = 2e-6 * max(1.0, 0.05 * r / max(np.hypot(p[0], p[1]), 1e-12))
        tol_v = 2e-6 * max(1.0, 0.05 / max(np.sqrt(max(1 - z * z, 0.0)), 1e-12))
        du = abs(img[i, 0] - u)
        assert min(du, 1 - du) <= tol_u, (i, img[i, 0], u)
        assert abs(img[i, 1] - v) <= tol_v, (i, img[i, 1], v)
        assert img[i, 2] == 0
        checked += 1
    assert checked > 50
    assert (img[hit["shape"] < 0] == 0).all()  # a miss is black, not the background
    sc.close()
