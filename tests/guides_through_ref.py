"""Guides through glass (yuki_amd/csrc/yk_guides_through.h), restated independently of the library: the surfaces come from
OracleScene.surface and the lobes' directions from orc_bsdf_sample (u0 = 0.75 draws the transmission lobe of glass,
u0 = 0.25 the reflection lobe — Bsdf::sample_f picks lobe floor(2 u0)); the spawn rule, the running T and the branch
decisions are numpy float32 here.  Also the test scenes: a closed glass slab in front of a two-part wall, and its variants."""
import ctypes as C

import numpy as np

from yuki_amd import abi, scenes

F = np.float32
SF = abi.SURFACE_FIELDS
MAX = abi.GUIDES_THROUGH_MAX

# what happened to the ray at interface k of a pixel (branch[:, k]); 0 = the pixel had ended before
NONE, TRANSMIT, TIR_REFLECT, KT0_REFLECT, STOP, FINAL, MISS, CUT = range(8)
BRANCH_NAMES = ["none", "transmit", "tir-reflect", "kt0-reflect", "stop", "final", "miss", "cut"]


def _material_desc(m):
    d = abi.MaterialDesc()
    d.kind = m["kind"]
    d.a = abi.f3(m.get("a", (0, 0, 0)))
    d.b = abi.f3(m.get("b", (0, 0, 0)))
    d.c = float(m.get("c", 0.0))
    d.flags = 1 if m.get("remap", False) else 0
    return d


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _lobe_wi(oracle, md, rec, wo, u0):
    """wi of Bsdf::sample_f(wo, (u0, 0)) at the surface record, or None when the sample is empty (pdf 0)."""
    u = np.array([u0, 0.0], F)
    out = np.zeros(8, F)
    ng, ns, dpdu = (np.ascontiguousarray(rec[SF[k]], F) for k in ("n", "ns", "dpdus"))
    oracle.lib().orc_bsdf_sample(C.byref(md), _vp(ng), _vp(ns), _vp(dpdu), _vp(wo), _vp(u), _vp(out))
    if out[6] == 0.0 or int(out[7]) == 0:
        return None
    return out[0:3].copy()


def _dot(a, b):
    """V3 . V3 in binary32, products summed left to right."""
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def spawn_origin(p, n, d):
    """Interaction::spawn_ray (interaction.rs:27-40): p +- n * 0.001, the sign of d . n."""
    off = (n * F(0.001)).astype(F)
    return (p + off).astype(F) if _dot(d, n) > F(0) else (p - off).astype(F)


def camera_rays(oracle, cam, res):
    return oracle.camera_rays(cam.matrices, abi.SamplerDesc(abi.SAMPLER_STRATIFIED, 1, 1, 0, 0), (0, 0, res[0], res[1]), 0)


def guides_through(oracle, osc, sd, cam, res, max_through, want_segments=False):
    """-> (guides (h, w) GUIDE_DTYPE, ids (h, w) SURFACE_ID_DTYPE, through (h, w) uint32, branch (h, w, MAX + 1) uint8).
    want_segments: also the list of (pixel indices, o, d, surface records) of every pass, for the device-only tie."""
    w, h = res
    n = w * h
    o, d = camera_rays(oracle, cam, res)
    guides = np.zeros(n, abi.GUIDE_DTYPE)
    ids = np.zeros(n, abi.SURFACE_ID_DTYPE)
    ids["shape"] = abi.SURFACE_NONE
    through = np.zeros(n, np.uint32)
    branch = np.zeros((n, MAX + 1), np.uint8)
    mats = [_material_desc(m) for m in sd.materials]
    pix = np.arange(n)
    T = np.zeros(n, F)
    segments = []
    for k in range(max_through + 1):
        if len(pix) == 0:
            break
        rec = osc.surface(o, d)
        if want_segments:
            segments.append((pix.copy(), o.copy(), d.copy(), rec.copy()))
        nxt_pix, nxt_o, nxt_d, nxt_T = [], [], [], []
        for j, px in enumerate(pix):
            r = rec[j]
            through[px] = k
            if r[SF["hit"]] == 0.0:
                branch[px, k] = MISS
                continue
            Tk = r[SF["t"]] if k == 0 else F(T[j] + r[SF["t"]])
            m = sd.materials[int(r[SF["material"]])]
            step = FINAL
            wi = None
            if m["kind"] == abi.MAT_GLASS:
                if k == max_through:
                    step = CUT
                else:
                    wo = (-d[j]).astype(F)
                    kr0 = all(F(v) == F(0) for v in m.get("a", (0, 0, 0)))
                    kt0 = all(F(v) == F(0) for v in m.get("b", (0, 0, 0)))
                    md = mats[int(r[SF["material"]])]
                    step = STOP
                    if not kt0:
                        wi = _lobe_wi(oracle, md, r, wo, 0.75)
                        if wi is not None:
                            step = TRANSMIT
                    if wi is None and not kr0:
                        wi = _lobe_wi(oracle, md, r, wo, 0.25)
                        if wi is not None:
                            step = KT0_REFLECT if kt0 else TIR_REFLECT
            branch[px, k] = step
            if wi is not None:
                nxt_pix.append(px)
                nxt_o.append(spawn_origin(r[SF["p"]], r[SF["n"]], wi))
                nxt_d.append(wi)
                nxt_T.append(Tk)
                continue
            guides["ns"][px] = r[SF["ns"]]
            guides["hit"][px] = 1.0
            guides["p"][px] = r[SF["p"]]
            guides["t"][px] = Tk
            ids["shape"][px] = int(r[SF["shape"]])
            ids["b"][px] = r[SF["b"]]
        pix = np.asarray(nxt_pix, np.int64)
        o = np.asarray(nxt_o, F).reshape(-1, 3)
        d = np.asarray(nxt_d, F).reshape(-1, 3)
        T = np.asarray(nxt_T, F)
    out = (guides.reshape(h, w), ids.reshape(h, w), through.reshape(h, w), branch.reshape(h, w, MAX + 1))
    return out + (segments,) if want_segments else out


def branch_counts(branch):
    """{name: pixels in which the branch occurs at some interface}."""
    return {BRANCH_NAMES[c]: int((branch == c).any(axis=-1).sum()) for c in range(1, 8)}


def crossed_histogram(through, guides):
    """pixels by interfaces crossed, 0 .. MAX (the issue's table)."""
    return np.bincount(through.reshape(-1), minlength=MAX + 1).tolist()


# ------------------------------------------------------------------ the slab scenes
# World: y up, the camera on the +z side looking towards -z.  A wall at z = WALL_Z whose left half (x < 0) is a plain
# matte and whose right half is an image-textured matte; a floor; one downward rectangular light with its emitter quad; in
# front of the wall the glass, by variant.  Lengths in metres.
WALL_Z, FLOOR_Y = -2.5, -1.5
SLAB = dict(x=(-0.8, 0.8), y=(-0.6, 0.6), z=(-1.0, -0.8), eta=1.5)  # front face z = -0.8 (towards the camera), back face z = -1.0
SLAB2_Z = (-1.5, -1.3)
CAMERA = dict(position=(0.9, 0.35, 1.0), target=(0.0, 0.0, -1.5), up=(0, 1, 0), fov_axis=abi.FOV_X, fov_degrees=50.0)
VARIANTS = ("slab", "mirror", "black", "prism", "two")
RES = (37, 23)


def _checker(w=16, h=16):
    y, x = np.mgrid[0:h, 0:w]
    t = np.zeros((h, w, 3), F)
    on = ((x // 2 + y // 2) % 2) == 0
    t[on] = (0.85, 0.8, 0.2)
    t[~on] = (0.1, 0.25, 0.7)
    return t


def _box(x, y, z):
    """A closed box, 12 triangles, outward normals (counter-clockwise seen from outside)."""
    p = np.array([(x[i], y[j], z[k]) for i in (0, 1) for j in (0, 1) for k in (0, 1)], F)  # index = 4 i + 2 j + k
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # -x +x -y +y -z +z
    idx = []
    for a, b, c, e in quads:
        idx += [(a, b, c), (a, c, e)]
    return p, np.asarray(idx, np.uint32)


def _prism(x, y, z):
    """A right-angle prism: cross-section in the xz plane with the right angle at (x1, z1); legs along the front face
    z = z1 (x0 .. x1) and the side face x = x1 (z0 .. z1); the hypotenuse from (x0, z1) to (x1, z0).  A ray that enters
    the front face straight meets the hypotenuse at 45 degrees, beyond the critical angle of eta 1.5 (41.8 degrees)."""
    a, b, c = (x[0], z[1]), (x[1], z[1]), (x[1], z[0])
    p = np.array([(q[0], yy, q[1]) for yy in y for q in (a, b, c)], F)  # 0..2 bottom, 3..5 top
    idx = [(0, 2, 1), (3, 4, 5), (0, 4, 3), (0, 1, 4), (1, 5, 4), (1, 2, 5), (2, 3, 5), (2, 0, 3)]  # outward normals
    return p, np.asarray(idx, np.uint32)


def slab_scene(variant="slab"):
    assert variant in VARIANTS
    glass = dict(kind=abi.MAT_GLASS, a=(1, 1, 1), b=(1, 1, 1), c=SLAB["eta"])
    if variant == "mirror":
        glass["b"] = (0, 0, 0)
    if variant == "black":
        glass["a"] = glass["b"] = (0, 0, 0)
    WALL_L, WALL_R, WHITE, EMIT, GLASS = range(5)
    materials = [
        dict(kind=abi.MAT_MATTE, a=(0.7, 0.3, 0.2), c=0.0),
        dict(kind=abi.MAT_MATTE, a=(0.5, 0.5, 0.5), c=0.0, tex=0),
        dict(kind=abi.MAT_MATTE, a=(0.7, 0.7, 0.7), c=0.0),
        dict(kind=abi.MAT_MATTE, a=(0, 0, 0), c=0.0),
        glass,
    ]
    z = F(WALL_Z)
    meshes = []  # (points, indices, uvs or None, material, area light)
    meshes.append((np.array([(-3, -1.5, z), (0, -1.5, z), (0, 2, z), (-3, 2, z)], F), np.array([(0, 1, 2), (0, 2, 3)], np.uint32), None, WALL_L, -1))
    meshes.append((np.array([(0, -1.5, z), (3, -1.5, z), (3, 2, z), (0, 2, z)], F), np.array([(0, 1, 2), (0, 2, 3)], np.uint32), np.array([(0, 0), (2, 0), (2, 2), (0, 2)], F), WALL_R, -1))
    fy = F(FLOOR_Y)
    meshes.append((np.array([(-3, fy, z), (3, fy, z), (3, fy, 2), (-3, fy, 2)], F), np.array([(0, 2, 1), (0, 3, 2)], np.uint32), None, WHITE, -1))
    ly = F(1.9)
    meshes.append((np.array([(-0.5, ly, -1.0), (0.5, ly, -1.0), (0.5, ly, 0.0), (-0.5, ly, 0.0)], F), np.array([(0, 1, 2), (0, 2, 3)], np.uint32), None, EMIT, 0))
    if variant == "prism":
        meshes.append(_prism((-0.6, 0.6), SLAB["y"], (-2.0, -0.8)) + (None, GLASS, -1))
    else:
        meshes.append(_box(SLAB["x"], SLAB["y"], SLAB["z"]) + (None, GLASS, -1))
    if variant == "two":
        meshes.append(_box(SLAB["x"], SLAB["y"], SLAB2_Z) + (None, GLASS, -1))
    pts, uvs, idx, tmesh, tmat, tal, flags = [], [], [], [], [], [], []
    base = 0
    for mi, (p, ind, uv, mat, al) in enumerate(meshes):
        pts.append(np.asarray(p, F))
        uvs.append(np.asarray(uv, F) if uv is not None else np.zeros((len(p), 2), F))
        idx.append(ind + np.uint32(base))
        tmesh += [mi] * len(ind)
        tmat += [mat] * len(ind)
        tal += [al] * len(ind)
        flags.append((False, uv is not None, False))
        base += len(p)
    size = F(1.0)
    radiance = F(6.0)
    l2w, l2w_inv = scenes._translation((0.0, float(ly), -0.5))
    return scenes.SceneData(
        points=np.concatenate(pts),
        uvs=np.concatenate(uvs),
        indices=np.concatenate(idx),
        tri_mesh=np.asarray(tmesh, np.uint32),
        tri_material=np.asarray(tmat, np.int32),
        tri_area_light=np.asarray(tal, np.int32),
        meshes=flags,
        materials=materials,
        lights=[dict(kind="rect", l2w=l2w, l2w_inv=l2w_inv, L=(radiance,) * 3, size=(size, size))],
        background=(0.05, 0.06, 0.08),
        split_method=abi.SPLIT_SAH,
        max_shapes_in_node=1,
        camera=dict(CAMERA),
        name="glass-" + variant,
        textures=[_checker()],
    )


# ------------------------------------------------------------------ float64 optics of the slab
def slab_optics(o, d):
    """The closed form for a ray that enters the slab's front face and leaves through its back face, in float64, with the
    renderer's two 1e-3 spawn offsets along the face normals: -> dict(ok, d_out, p_wall, T).  ok is False where the ray
    misses the front face, would leave through a side face, or is totally reflected (impossible from outside)."""
    o = np.asarray(o, np.float64)
    d = np.asarray(d, np.float64)
    zf, zb, zw = SLAB["z"][1], SLAB["z"][0], WALL_Z
    eta = 1.0 / SLAB["eta"]
    n = np.array([0.0, 0.0, 1.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (zf - o[:, 2]) / d[:, 2]
        p1 = o + t1[:, None] * d
        dl = np.linalg.norm(d, axis=1)
        u = d / dl[:, None]
        cos_i = -u[:, 2]
        sin2_t = eta * eta * (1.0 - cos_i * cos_i)
        cos_t = np.sqrt(1.0 - sin2_t)
        # Snell, in the renderer's scaling: wt = eta * (-wo) + (eta cos_i - cos_t) n with wo = -d (d's length kept)
        d2 = eta * d + (eta * cos_i * dl - cos_t * dl)[:, None] * n
        o2 = p1 - 1e-3 * n
        t2 = (zb - o2[:, 2]) / d2[:, 2]
        p2 = o2 + t2[:, None] * d2
        dl2 = np.linalg.norm(d2, axis=1)
        u2 = d2 / dl2[:, None]
        cos_i2 = -u2[:, 2]
        eta2 = SLAB["eta"]
        sin2_t2 = eta2 * eta2 * (1.0 - cos_i2 * cos_i2)
        cos_t2 = np.sqrt(1.0 - sin2_t2)
        d3 = eta2 * d2 + (eta2 * cos_i2 * dl2 - cos_t2 * dl2)[:, None] * n
        o3 = p2 - 1e-3 * n
        t3 = (zw - o3[:, 2]) / d3[:, 2]
        p3 = o3 + t3[:, None] * d3
    inside = lambda p: (p[:, 0] > SLAB["x"][0]) & (p[:, 0] < SLAB["x"][1]) & (p[:, 1] > SLAB["y"][0]) & (p[:, 1] < SLAB["y"][1])  # noqa: E731
    ok = (d[:, 2] < 0) & (t1 > 0) & inside(p1) & inside(p2) & (sin2_t2 < 1.0) & (np.abs(p3[:, 0]) < 3.0) & (p3[:, 1] > FLOOR_Y) & (p3[:, 1] < 2.0)
    return dict(ok=ok, d_out=d3, p_wall=p3, T=t1 + t2 + t3, d_in=d)


# ------------------------------------------------------------------ the restatement against the closed form
# The test's camera is CAMERA; the tolerances are measured under these (tools/guides_through_tolerances.py), whose rays
# are other rays: positions and targets moved by decimetres.
CALIBRATION_CAMERAS = tuple(dict(CAMERA, position=p, target=t) for p, t in (((0.5, 0.1, 1.3), (0.1, 0.05, -1.5)), ((1.2, 0.5, 0.8), (-0.1, -0.1, -1.5)), ((-0.7, 0.25, 1.1), (0.05, 0.0, -1.5))))
OPTICS_RES = (64, 36)
OPTICS_FIGURES = ("dir_abs", "p_abs", "T_rel")


def slab_score(yk, oracle, camera, res=OPTICS_RES):
    """The restatement on the slab scene under `camera` against slab_optics: over the pixels whose path is front face ->
    back face -> wall, dir_abs = the largest component difference between the last segment's direction and the camera
    ray's (exit parallel to entry), p_abs = the largest component difference of the guide's p from the closed-form point
    on the wall, T_rel = the largest relative difference of the guide's t from the summed segment lengths; `excluded` =
    the share of those pixels the closed form's own predicates leave out, `compared` their number."""
    sd = slab_scene("slab")
    sd.camera = dict(camera)
    fs = yk.FilmSettings(res=res, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    osc = oracle.OracleScene(sd)
    guides, ids, through, branch, seg = guides_through(oracle, osc, sd, cam, res, 4, want_segments=True)
    osc.close()
    n = res[0] * res[1]
    g = guides.reshape(n)
    br = branch.reshape(n, MAX + 1)
    o0, d0 = seg[0][1], seg[0][2]
    path = (br[:, 0] == TRANSMIT) & (br[:, 1] == TRANSMIT) & (br[:, 2] == FINAL)
    zf, zb = SLAB["z"][1], SLAB["z"][0]
    p_first = np.full((n, 3), np.nan)
    p_first[seg[0][0]] = seg[0][3][:, SF["p"]]
    p_second = np.full((n, 3), np.nan)
    p_second[seg[1][0]] = seg[1][3][:, SF["p"]]
    d_last = np.full((n, 3), np.nan)
    d_last[seg[2][0]] = seg[2][2]
    with np.errstate(invalid="ignore"):
        path &= (np.abs(p_first[:, 2] - zf) < 1e-5) & (np.abs(p_second[:, 2] - zb) < 1e-5) & (np.abs(g["p"][:, 2] - WALL_Z) < 1e-5)
    opt = slab_optics(o0, d0)
    use = path & opt["ok"]
    assert use.sum() > 0.2 * n, int(use.sum())
    d64 = d0.astype(np.float64)
    return dict(
        dir_abs=float(np.abs(d_last[use] - d64[use]).max()),
        p_abs=float(np.abs(g["p"][use].astype(np.float64) - opt["p_wall"][use]).max()),
        T_rel=float((np.abs(g["t"][use].astype(np.float64) - opt["T"][use]) / opt["T"][use]).max()),
        excluded=float((path & ~opt["ok"]).sum() / max(1, path.sum())),
        compared=int(use.sum()),
    )


# ------------------------------------------------------------------ the quality condition
QUALITY_SCENES = {"glass-slab": (64, 36), "cornell": (48, 48)}
QUALITY = dict(depth=8, noisy_spp=4, converged_spp=1024, max_through=4, converged_seed=0x73B9642E74AC471C ^ 0x1234567)
QUALITY_TEST_SEED = 0x73B9642E74AC471C
QUALITY_CALIBRATION_SEEDS = (0x1D872B41A3C5E697, 0x2545F4914F6CDD1D, 0x9E3779B97F4A7C15)
_CONVERGED = {}


def masked_error(x, ref_film, mask):
    """test_denoise.quality_error (RMSE over all channels of x / (1 + x), float64) over the pixels of `mask`."""
    a = np.asarray(x, np.float64)[mask]
    b = np.asarray(ref_film, np.float64)[mask]
    d = a / (1.0 + a) - b / (1.0 + b)
    return float(np.sqrt(np.mean(d * d)))


def quality_inputs(yk, oracle, name):
    """Everything about a quality scene that does not depend on the noisy film's seed, computed once: the converged film,
    the first-hit and the through guides, ids and albedos, the mask `through >= 1 and hit`."""
    if name in _CONVERGED:
        return _CONVERGED[name]
    from test_denoise import oracle_guides

    res = QUALITY_SCENES[name]
    sd = slab_scene("slab") if name == "glass-slab" else scenes.by_name(name)
    fs = yk.FilmSettings(res=res, tile_dim=16)
    cam = yk.Camera(sd.camera, fs)
    tiles = yk.film_tiles(fs)
    osc = oracle.OracleScene(sd)
    integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, QUALITY["depth"], 0, 0.0)
    conv = yk.update_tiles(tiles, osc.render_tiles(cam.matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, QUALITY["converged_spp"], 1, 1, QUALITY["converged_seed"]), integ, tiles, n_threads=0)[0], fs.res)
    first = oracle_guides(oracle, osc, cam, res)
    guides, ids, through, _ = guides_through(oracle, osc, sd, cam, res, QUALITY["max_through"])
    _, first_ids, _, _ = guides_through(oracle, osc, sd, cam, res, 0)
    host_scene = yk.Scene(None, sd)
    q = dict(sd=sd, fs=fs, cam=cam, tiles=tiles, osc=osc, integ=integ, conv=conv, first=first, guides=guides, through=through, mask=(through >= 1) & (guides["hit"] != 0),
             albedo=yk.surface_albedo(host_scene, ids), first_albedo=yk.surface_albedo(host_scene, first_ids))
    host_scene.close()
    _CONVERGED[name] = q
    return q


def quality_figures(yk, oracle, name, seed):
    """{figure: value} for the noisy film of sampler seed `seed`: the masked errors of the host denoiser (default
    DenoiseParams) under first-hit and under through guides, their ratio, the whole-film ratio, and — with albedo — the
    same for denoise(albedo=) under each pass's own albedo."""
    q = quality_inputs(yk, oracle, name)
    noisy = yk.update_tiles(q["tiles"], q["osc"].render_tiles(q["cam"].matrices, abi.SamplerDesc(abi.SAMPLER_UNIFORM, QUALITY["noisy_spp"], 1, 1, seed), q["integ"], q["tiles"], n_threads=0)[0], q["fs"].res)
    p = yk.DenoiseParams()
    every = np.ones(q["mask"].shape, bool)
    out = dict(masked_pixels=int(q["mask"].sum()), noisy=masked_error(noisy, q["conv"], q["mask"]))
    for tag, kw_first, kw_through in (("", {}, {}), ("albedo_", dict(albedo=q["first_albedo"]), dict(albedo=q["albedo"]))):
        a = yk.denoise(noisy, q["first"], p, **kw_first)
        b = yk.denoise(noisy, q["guides"], p, **kw_through)
        out[tag + "first"] = masked_error(a, q["conv"], q["mask"])
        out[tag + "through"] = masked_error(b, q["conv"], q["mask"])
        out[tag + "ratio"] = out[tag + "through"] / out[tag + "first"]
        out[tag + "film_ratio"] = masked_error(b, q["conv"], every) / masked_error(a, q["conv"], every)
    return out
