"""Light work the light loops leave out because it changes no bit of the film (context option "nee_skip", a bit mask):

  2  a shadow ray whose contribution is +-0 in every component is reported but neither staged nor traced.

(Bit 1 — no light sampling at a vertex whose material takes no light — was built, passed these tests under masks 0 to 3, and
was not kept: it did not pay on the flagship frame, DESIGN.md §9.  The option now accepts 0 and 2.)

Under either mask (0 = every ray) the film is the oracle's bit for bit and `rays` / `shadow_rays` are the oracle's: the
reported shadow-ray count has to include the rays that were not traced, over blocks, bounces and batches.  The scenes hold
every material kind (glass, a black matte and a matte whose texture is black in places among them) under every place of the
rectangular light among two point lights.  Path (k_shade), Whitted (k_whitted) and yk_li_debug (k_path_debug) each have the
light loop.  The oracle records no ray lists: yk_li_debug's lists under mask 2 are held against those of mask 0, which
tests/test_gpu_li_debug.py checks against independent geometry."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from yuki_amd import abi, scenes

pytestmark = pytest.mark.gpu
SEED = 0x73B9642E74AC471C
F = np.float32
MASKS = (0, 2)
RES = (64, 36)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _samplers(yk):
    return (yk.SamplerType.Stratified((2, 2), True, SEED), yk.SamplerType.Stratified((2, 2), False, SEED), yk.SamplerType.Uniform(4, SEED))


def _translation(p):
    m = np.eye(4, dtype=F)
    m[:3, 3] = p
    inv = np.eye(4, dtype=F)
    inv[:3, 3] = [-F(v) for v in p]
    return m, inv


@pytest.fixture(scope="module")
def nctx(yk):
    """A context of this module's own: the tests change its "nee_skip"."""
    c = yk.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ scenes
LIGHT_ORDERS = ["rect-first", "rect-middle", "rect-last", "rect-alone"]


def mixed_scene(order="rect-first"):
    """A 4 x 3 city (972 triangles) whose twelve instances are given every material kind on purpose: Lambert, Oren-Nayar,
    metal, glossy, glass and a black matte; the ground carries a checker texture with black squares (a matte that is black in
    places).  Every second instance has shading normals.  The rectangular light stands at `order`'s place among the two
    point lights."""
    s = scenes.city((4, 3), 1, 1, "mixed")
    n_inst = 12
    col = (0.7, 0.5, 0.3)
    kinds = [
        dict(kind=abi.MAT_MATTE, a=col, c=0.0),
        dict(kind=abi.MAT_GLASS, a=(1, 1, 1), b=(1, 1, 1), c=1.5),
        dict(kind=abi.MAT_MATTE, a=(0, 0, 0), c=0.0),
        dict(kind=abi.MAT_MATTE, a=col, c=float(np.float32(np.deg2rad(20.0)))),
        dict(kind=abi.MAT_METAL, a=(0.27105, 0.67693, 1.31640), b=(3.60920, 2.62480, 2.29210), c=0.12, remap=True),
        dict(kind=abi.MAT_GLOSSY, a=col, c=0.3, remap=False),
    ]
    s.materials = [dict(kinds[k % len(kinds)]) for k in range(n_inst)] + list(s.materials[n_inst:])
    ground = n_inst
    s.materials[ground] = dict(kind=abi.MAT_MATTE, a=(0.55, 0.55, 0.55), c=0.0, tex=0)
    checker = np.zeros((8, 8, 3), dtype=F)
    checker[::2, ::2] = (0.6, 0.5, 0.4)
    checker[1::2, 1::2] = (0.3, 0.5, 0.7)
    s.textures = [checker]
    rect, p1, p2 = s.lights
    s.lights = {"rect-first": [rect, p1, p2], "rect-middle": [p1, rect, p2], "rect-last": [p1, p2, rect], "rect-alone": [rect]}[order]
    s.tri_area_light = np.where(s.tri_area_light >= 0, [l["kind"] for l in s.lights].index("rect"), -1).astype(np.int32)
    s.name = "city-4x3-every-kind-" + order
    return s


def _quad(p0, p1, p2, p3):
    return np.array([p0, p1, p2, p3], dtype=F), np.array([(0, 1, 2), (0, 2, 3)], dtype=np.uint32)


def zero_scene():
    """Shadow rays that add exactly zero although f is not black, by construction:

      * a matte floor (y = 0) whose per-vertex normals are tilted 53 degrees towards +x, lit by a point light that grazes it
        from -x: above the geometric surface like the camera (f is not black), behind the shading normal (the clamp is 0);
      * two upright matte quads at z = -1 with opposite windings, camera and point light on their +z side: one of them is
        seen and lit from the back (geometric = shading normal points away from both: f not black, the clamp 0);
      * two glass spheres, a point light in the centre of one of them (f of glass is black: no ray, beside rays that add zero);
      * the other upright quad and an Oren-Nayar quad behind the gap between the two, so that ordinary contributions exist too."""
    tilt = np.array((0.8, 0.6, 0.0), dtype=F)
    parts = [
        (_quad((-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2)), 0, tilt),
        (_quad((-1.6, 0.0, -1.0), (-0.2, 0.0, -1.0), (-0.2, 1.2, -1.0), (-1.6, 1.2, -1.0)), 1, None),
        (_quad((0.2, 0.0, -1.0), (0.2, 1.2, -1.0), (1.6, 1.2, -1.0), (1.6, 0.0, -1.0)), 1, None),
        (_quad((-0.6, 0.0, -1.6), (0.6, 0.0, -1.6), (0.6, 1.6, -1.6), (-0.6, 1.6, -1.6)), 2, None),
    ]
    pts, nrm, idx, tmesh, tmat, meshes = [], [], [], [], [], []
    base = 0
    for k, ((p, f), mat, n) in enumerate(parts):
        pts.append(p)
        nrm.append(np.tile(n, (4, 1)) if n is not None else np.zeros((4, 3), dtype=F))
        idx.append(f + np.uint32(base))
        tmesh += [k] * 2
        tmat += [mat] * 2
        meshes.append((n is not None, False, False))
        base += 4
    GLASS = 3
    materials = [
        dict(kind=abi.MAT_MATTE, a=(0.6, 0.6, 0.6), c=0.0),
        dict(kind=abi.MAT_MATTE, a=(0.7, 0.4, 0.3), c=0.0),
        dict(kind=abi.MAT_MATTE, a=(0.3, 0.6, 0.4), c=float(np.float32(np.deg2rad(20.0)))),
        dict(kind=abi.MAT_GLASS, a=(1, 1, 1), b=(1, 1, 1), c=1.5),
    ]
    spheres = []
    for c, r in (((0.9, 0.45, 0.4), 0.4), ((-0.9, 0.35, 0.6), 0.3)):
        o2w, w2o = _translation(c)
        spheres.append(dict(o2w=o2w, w2o=w2o, radius=r, material=GLASS))
    lights = [
        dict(kind="point", l2w=_translation((-3.0, 0.3, 0.0))[0], I=(6.0, 5.0, 4.0)),  # grazes the floor from -x
        dict(kind="point", l2w=_translation((0.9, 0.45, 0.4))[0], I=(1.0, 1.2, 1.5)),  # inside the first glass sphere
    ]
    return scenes.SceneData(
        points=np.concatenate(pts), normals=np.concatenate(nrm).astype(F), indices=np.concatenate(idx), tri_mesh=np.asarray(tmesh, dtype=np.uint32),
        tri_material=np.asarray(tmat, dtype=np.int32), tri_area_light=np.full(len(tmat), -1, dtype=np.int32), meshes=meshes, materials=materials, lights=lights,
        spheres=spheres, background=(0.05, 0.06, 0.08), split_method=abi.SPLIT_SAH, max_shapes_in_node=1,
        camera=dict(position=(0.0, 1.6, 3.2), target=(0.0, 0.4, -0.6), up=(0, 1, 0), fov_axis=abi.FOV_X, fov_degrees=55.0), name="zero-contributions")


def certain_zero_rays(sd, osc, o, d):
    """Counted on the host from the oracle's hits of the camera rays (o, d): (vertex, point light) pairs of a matte surface
    where the light and the viewer lie on the same side of the geometric normal (f is not black) and the light lies at least a
    degree behind the shading normal (the clamp of ns . l is 0): rays path.rs:113 traces for a contribution of exactly zero."""
    hit = osc.intersect(o, d)
    tri = hit["shape"]
    on_tri = (tri >= 0) & (tri < sd.n_triangles)
    matte = np.zeros(len(tri), dtype=bool)
    mk = np.array([m["kind"] == abi.MAT_MATTE and max(m["a"]) > 0 for m in sd.materials])
    matte[on_tri] = mk[sd.tri_material[tri[on_tri]]]
    n, ns, p = hit["n"].astype(np.float64), hit["ns"].astype(np.float64), hit["p"].astype(np.float64)
    wo = -np.asarray(d, dtype=np.float64)
    total = 0
    for l in sd.lights:
        if l["kind"] != "point":
            continue
        wi = np.asarray(l["l2w"], dtype=np.float64)[:3, 3] - p
        wi /= np.linalg.norm(wi, axis=1, keepdims=True)
        same_side = (wi * n).sum(1) * (wo * n).sum(1) > 1e-6
        behind = (ns * wi).sum(1) < -np.sin(np.deg2rad(1.0))
        total += int((matte & same_side & behind).sum())
    return total


def _frame(yk, sd):
    fs = yk.FilmSettings(res=RES, tile_dim=16)
    return yk.Camera(sd.camera, fs), yk.film_tiles(fs)


def _check_frame_under_every_mask(yk, nctx, oracle, sd, integ, masks=MASKS, shadow=True):
    """Film, rays and shadow rays of `sd` against the oracle, for the three samplers under every mask; the oracle renders once
    per sampler."""
    sc = yk.Scene(nctx, sd)
    osc = oracle.OracleScene(sd)
    cam, tiles = _frame(yk, sd)
    it = yk.IntegratorType.instantiate(nctx, integ)
    try:
        for sampler in _samplers(yk):
            want, rays, ostats = osc.render_tiles(cam.matrices, sampler, integ, tiles, n_threads=0, want_stats=True)
            assert want.max() > 0 and np.isfinite(want).all()
            for mask in masks:
                nctx.set_option("nee_skip", mask)
                got, stats = it.render_tiles(sc, cam, sampler, tiles)
                assert stats.rays == rays, (sd.name, mask)
                if shadow:
                    assert stats.shadow_rays == ostats.shadow_rays, (sd.name, mask)
                assert np.array_equal(_bits(got), _bits(want)), (sd.name, mask)
    finally:
        nctx.set_option("nee_skip", 2)
        sc.close()
        osc.close()


# ------------------------------------------------------------------ every material kind, every light order
@pytest.mark.parametrize("order", LIGHT_ORDERS)
def test_every_material_kind_under_every_light_order(nctx, yk, oracle, order):
    _check_frame_under_every_mask(yk, nctx, oracle, mixed_scene(order), yk.IntegratorType.Path(yk.PathParams(max_depth=8)))


def test_option_range(nctx, yk):
    from yuki_amd._ffi import YukiError

    for bad in (-1, 1, 3, 4):  # bit 1 was not kept
        with pytest.raises(YukiError):
            nctx.set_option("nee_skip", bad)
    nctx.set_option("nee_skip", 2)


# ------------------------------------------------------------------ zero contributions
def test_zero_contributions_keep_film_and_counts(nctx, yk, oracle):
    sd = zero_scene()
    osc = oracle.OracleScene(sd)
    cam, _ = _frame(yk, sd)
    o, d = oracle.camera_rays(cam.matrices, _samplers(yk)[0], (0, 0, RES[0], RES[1]), 0)
    assert certain_zero_rays(sd, osc, o, d) > 100  # the scene has what it was built for, before any device work
    osc.close()
    _check_frame_under_every_mask(yk, nctx, oracle, sd, yk.IntegratorType.Path(yk.PathParams(max_depth=8)))


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
from yuki_amd import core as yk
import test_gpu_nee_skip as T
sd = T.zero_scene()
cam, tiles = T._frame(yk, sd)
sampler = T._samplers(yk)[0]
integ = yk.IntegratorType.Path(yk.PathParams(max_depth=8))
for mask in (0, 2):
    ctx = yk.Context(0, nee_skip=mask, time_kernels=2)
    sc = yk.Scene(ctx, sd)
    print("mask %d" % mask, file=sys.stderr, flush=True)
    got, stats = yk.IntegratorType.instantiate(ctx, integ).render_tiles(sc, cam, sampler, tiles)
    print("shadow_rays %d" % stats.shadow_rays, file=sys.stderr, flush=True)
    sc.close()
    ctx.close()
"""


def test_zero_contributions_are_not_traced():
    """YK_DEBUG_BOUNCES=1 prints, per bounce, the shadow rays traced (the any-hit queues' lengths) and reported (what the bounce
    added to the render's count).  A fresh child process (the variable is read by the library): under mask 0 the two are equal
    on every bounce, under mask 2 fewer are traced than reported, and the reported totals are the same and are `shadow_rays`."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, YK_DEBUG_BOUNCES="1")
    env.pop("YK_NEE_SKIP", None)
    out = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(here), here], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    per_mask, mask = {}, None
    for line in out.stderr.splitlines():
        m = re.match(r"mask (\d+)", line)
        if m:
            mask = int(m.group(1))
            per_mask[mask] = dict(traced=[], reported=[], shadow_rays=None)
        m = re.match(r"bounce \d+: shadow rays traced / reported (\d+) / (\d+)", line)
        if m:
            per_mask[mask]["traced"].append(int(m.group(1)))
            per_mask[mask]["reported"].append(int(m.group(2)))
        m = re.match(r"shadow_rays (\d+)", line)
        if m:
            per_mask[mask]["shadow_rays"] = int(m.group(1))
    assert set(per_mask) == {0, 2}, out.stderr
    for mask, r in per_mask.items():
        assert len(r["traced"]) == 8 and sum(r["reported"]) == r["shadow_rays"], (mask, r)
    assert per_mask[0]["traced"] == per_mask[0]["reported"]
    assert per_mask[2]["reported"] == per_mask[0]["reported"]
    assert all(t <= r for t, r in zip(per_mask[2]["traced"], per_mask[2]["reported"]))
    assert per_mask[2]["traced"][0] < per_mask[2]["reported"][0]  # the camera bounce: certain_zero_rays counted them on the host
    assert sum(per_mask[2]["traced"]) < sum(per_mask[2]["reported"])


# ------------------------------------------------------------------ several batches
@pytest.mark.parametrize("which", ["mixed", "zero"])
def test_frame_cut_into_batches(yk, oracle, which):
    """batch_paths = 1000: the 9216 samples of the frame take ten batches, the last one of 216 paths; inside a batch the
    later bounces' queues end in partly empty windows.  The reported count is summed over blocks, bounces and batches."""
    sd = mixed_scene("rect-middle") if which == "mixed" else zero_scene()
    c = yk.Context(0, batch_paths=1000)
    try:
        _check_frame_under_every_mask(yk, c, oracle, sd, yk.IntegratorType.Path(yk.PathParams(max_depth=8)))
    finally:
        c.close()


# ------------------------------------------------------------------ Whitted and li_debug
def test_whitted_glass_balls(nctx, yk, oracle):
    """k_whitted's light loop takes the same gate; its shadow-ray count stays what mask 0 reports."""
    sd = scenes.glass_balls()
    integ = yk.IntegratorType.Whitted(5)
    _check_frame_under_every_mask(yk, nctx, oracle, sd, integ, shadow=False)
    sc = yk.Scene(nctx, sd)
    cam, tiles = _frame(yk, sd)
    it = yk.IntegratorType.instantiate(nctx, integ)
    counts = []
    for mask in MASKS:
        nctx.set_option("nee_skip", mask)
        counts.append(it.render_tiles(sc, cam, _samplers(yk)[0], tiles)[1].shadow_rays)
    nctx.set_option("nee_skip", 2)
    sc.close()
    assert counts[0] > 0 and counts == [counts[0]] * len(MASKS)


def test_whitted_zero_contributions(nctx, yk, oracle):
    _check_frame_under_every_mask(yk, nctx, oracle, zero_scene(), yk.IntegratorType.Whitted(4), shadow=False)


@pytest.mark.parametrize("which", ["mixed", "zero"])
def test_li_debug_records_under_every_mask(nctx, yk, oracle, which):
    """yk_li_debug (k_path_debug reports the ray that is not traced): radiance and closest-hit counts against the oracle, the
    ray lists (origins, directions, t_max, types, order) against mask 0's."""
    sd = mixed_scene("rect-middle") if which == "mixed" else zero_scene()
    sc = yk.Scene(nctx, sd)
    osc = oracle.OracleScene(sd)
    integ = yk.IntegratorType.Path(yk.PathParams(max_depth=8))
    it = yk.IntegratorType.instantiate(nctx, integ)
    fs = yk.FilmSettings(res=RES, tile_dim=64)
    cam = yk.Camera(sd.camera, fs)
    tile = (20, 12, 36, 28)
    xy = np.stack(np.meshgrid(np.arange(tile[0], tile[2]), np.arange(tile[1], tile[3]), indexing="xy"), axis=-1).reshape(-1, 2).astype(np.uint16)
    try:
        for sampler in _samplers(yk):
            k = 1
            o, d = yk.camera_rays(nctx, cam, sampler, tile, k)
            si = np.full(len(o), k, dtype=np.uint32)
            want, want_counts = osc.li(sampler, integ, o, d, xy, si)
            base = None
            for mask in MASKS:
                nctx.set_option("nee_skip", mask)
                li, counts, rays = it.li_debug(sc, sampler, o, d, xy, si)
                assert np.array_equal(_bits(li), _bits(want)), (sd.name, mask)
                assert np.array_equal(counts, np.asarray(want_counts, dtype=np.uint32))
                assert np.array_equal(_bits(it.li(sc, sampler, o, d, xy, si)), _bits(want)), (sd.name, mask)
                if base is None:
                    base = rays
                    assert any((r["ray_type"] == 4).any() for r in rays)  # RayType::Shadow
                else:
                    assert len(rays) == len(base)
                    assert all(a.tobytes() == b.tobytes() for a, b in zip(rays, base)), (sd.name, mask)
    finally:
        nctx.set_option("nee_skip", 2)
        sc.close()
        osc.close()
