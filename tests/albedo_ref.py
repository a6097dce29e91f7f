"""An independent numpy float32 restatement of the albedo passes (the rule of yuki_amd/csrc/yk_albedo.h), one operation per
statement, a whole film per step.  It never calls the product: the texel lookup is handed in (the oracle's texture_eval),
as is exp (the oracle's libm_array) for the filter, which is denoise_ref's.  Shared by tests/test_albedo.py (host instance)
and tests/test_gpu_albedo.py (device instance), which also take their scenes, ids, albedo records and films from here."""
import numpy as np

import denoise_ref
from denoise_ref import GUIDE_DTYPE, bits, canon  # noqa: F401
from motion_ref import SURFACE_ID_DTYPE, SURFACE_NONE, synthetic_ids  # noqa: F401

F = np.float32
ALBEDO_DTYPE = np.dtype([("a", "<f4", 3), ("known", "<f4")])
FLOOR = F(0.015625)
MAT_MATTE = 0  # YK_MAT_MATTE
SIZES = ((37, 23), (64, 36))  # (w, h) of the scene films on the host; the device suite adds 48 x 48
QUALITY = dict(res=(96, 54), depth=8, noisy_spp=4, converged_spp=1024, iterations=4, sigma_color=4.0, sigma_normal=0.3, plane_fraction=0.01, bound=0.8)


# ------------------------------------------------------------------ yk_surface_albedo
def surface_albedo(ids, sd, texture_eval):
    """(h, w) SURFACE_ID_DTYPE and the scene data the scene was made from -> (h, w) ALBEDO_DTYPE."""
    with np.errstate(all="ignore"):
        nt, ns, nm = int(sd.n_triangles), len(sd.spheres), len(sd.materials)
        shape = ids["shape"].astype(np.int64)
        live = (ids["shape"] != np.uint32(SURFACE_NONE)) & (shape < nt + ns)
        tri = live & (shape < nt)
        sph = live & ~tri
        mat = np.full(ids.shape, -1, np.int64)
        if nt:
            mat[tri] = np.asarray(sd.tri_material, np.int64)[shape[tri]]
        if ns:
            mat[sph] = np.array([s["material"] for s in sd.spheres], np.int64)[shape[sph] - nt]
        m_ok = live & (mat >= 0) & (mat < nm)
        m = np.where(m_ok, mat, 0)
        matte = np.array([mm["kind"] == MAT_MATTE for mm in sd.materials], bool)[m] & m_ok
        tex = np.array([mm["tex"] if (mm.get("tex") is not None and mm["kind"] == MAT_MATTE) else -1 for mm in sd.materials], np.int64)[m]
        kd = np.array([np.asarray(mm.get("a", (0, 0, 0)), np.float32) for mm in sd.materials], np.float32).reshape(-1, 3)[m]
        out = np.zeros(ids.shape, ALBEDO_DTYPE)
        out["a"] = F(1)
        ab = out["a"].view(np.uint32)  # written as bits: copied values keep theirs
        plain = matte & (tex < 0)
        ab[plain] = bits(np.ascontiguousarray(kd))[plain]
        textured = matte & (tex >= 0) & (tex < len(sd.textures)) & tri
        if textured.any():
            t = np.where(textured, shape, 0)
            idx = np.asarray(sd.indices).reshape(-1, 3).astype(np.int64)[t]  # (h, w, 3)
            has_uv = np.array([bool(mm[1]) for mm in sd.meshes], bool)[np.asarray(sd.tri_mesh, np.int64)[t]]
            default = np.broadcast_to(np.array([[0, 0], [1, 0], [1, 1]], np.float32), ids.shape + (3, 2))
            own = np.asarray(sd.uvs, np.float32).reshape(-1, 2)[idx] if sd.uvs is not None else default
            uv = np.where(has_uv[..., None, None], own, default).astype(np.float32)  # (h, w, vertex, component)
            b = ids["b"]
            p0 = (uv[..., 0, :] * b[..., 0:1]).astype(np.float32)
            p1 = (uv[..., 1, :] * b[..., 1:2]).astype(np.float32)
            p2 = (uv[..., 2, :] * b[..., 2:3]).astype(np.float32)
            s = (p0 + p1).astype(np.float32)
            st = (s + p2).astype(np.float32)
            for k, image in enumerate(sd.textures):
                pick = textured & (tex == k)
                if pick.any():
                    texel = texture_eval(image, np.ascontiguousarray(st[pick]))
                    ab[pick] = bits(np.ascontiguousarray(texel))
        out["known"] = np.where(plain | textured, F(1), F(0))
        return out


# ------------------------------------------------------------------ yk_denoise_albedo
def divisor(a):
    a = np.asarray(a, np.float32)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(a), np.where(a >= FLOOR, a, FLOOR), F(1)).astype(np.float32)


def denoise_albedo(film, guides, albedo, iterations, sigma_color, sigma_normal, sigma_plane, exp, tile_dim=16, samples=None):
    """denoise_ref.denoise with the division before the first iteration and the product after the last."""
    with np.errstate(all="ignore"):
        c = denoise_ref.normalise(film, tile_dim, samples)
        if iterations == 0:
            return c
        d = divisor(albedo["a"])
        c = canon((c / d).astype(np.float32))
        for i in range(iterations):
            c = denoise_ref.iteration(c, guides, i, sigma_color, sigma_normal, sigma_plane, exp)
        return canon((c * d).astype(np.float32))


# ------------------------------------------------------------------ the scenes of both suites
def textured_city():
    """city-small with its ground material (the second to last, Kd 0.55) replaced by a matte with a 16 x 16 random texture.
    The box mesh has uvs."""
    from yuki_amd import abi, scenes

    sd = scenes.by_name("city-small")
    ground = len(sd.materials) - 2
    assert tuple(sd.materials[ground]["a"]) == (0.55, 0.55, 0.55)
    sd.materials[ground] = dict(kind=abi.MAT_MATTE, a=(0.55, 0.55, 0.55), c=0.0, tex=0)
    sd.textures = [(0.1 + 0.8 * np.random.default_rng(3).random((16, 16, 3))).astype(np.float32)]
    return sd


def textured_cornell():
    """Cornell with material 1 (the back wall, which has uvs) textured by a 7 x 5 texture; the copper sphere and the glass
    box stay."""
    from yuki_amd import abi, scenes

    sd = scenes.cornell()
    sd.materials[1] = dict(kind=abi.MAT_MATTE, a=sd.materials[1]["a"], c=0.0, tex=0)
    sd.textures = [(0.05 + 0.9 * np.random.default_rng(4).random((5, 7, 3))).astype(np.float32)]
    return sd


def _translation(v):
    m, mi = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    m[:3, 3] = v
    mi[:3, 3] = -np.asarray(v, np.float32)
    return m, mi


def kinds_scene():
    """Every case of the rule in one small scene: ten quads (two triangles each) side by side, one material each, the even
    meshes with uvs and the odd ones without; four spheres.  Materials: 0 textured matte (17 x 9), 1 textured matte on a
    mesh without uvs (the default uvs), 2 textured matte (1 x 1), 3 plain matte, 4 Oren-Nayar matte, 5 black matte, 6 glass,
    7 metal, 8 glossy, 9 textured matte whose uvs lie outside [0, 1).  Spheres: plain matte, textured matte, metal, black."""
    from yuki_amd import abi, scenes

    rng = np.random.default_rng(11)
    textures = [rng.random((9, 17, 3)).astype(np.float32), rng.random((4, 3, 3)).astype(np.float32), np.array([[[0.25, 0.5, 0.75]]], np.float32)]
    textures[0][2, 3] = (0.0, -0.0, 1e-3)  # texels below the floor are the albedo all the same
    M, G, T, Y = abi.MAT_MATTE, abi.MAT_GLASS, abi.MAT_METAL, abi.MAT_GLOSSY
    materials = [
        dict(kind=M, a=(0.1, 0.2, 0.3), c=0.0, tex=0),
        dict(kind=M, a=(0.1, 0.2, 0.3), c=0.0, tex=1),
        dict(kind=M, a=(0.1, 0.2, 0.3), c=0.0, tex=2),
        dict(kind=M, a=(0.7, 0.01, 0.4), c=0.0),
        dict(kind=M, a=(0.3, 0.6, 0.9), c=0.35),
        dict(kind=M, a=(0, 0, 0), c=0.0),
        dict(kind=G, a=(1, 1, 1), b=(1, 1, 1), c=1.5),
        dict(kind=T, a=(0.27105, 0.67693, 1.31640), b=(3.60920, 2.62480, 2.29210), c=0.1, remap=True),
        dict(kind=Y, a=(0.5, 0.4, 0.3), c=0.3, remap=False),
        dict(kind=M, a=(0.1, 0.2, 0.3), c=0.0, tex=0),
    ]
    pts, uvs, idx, tmesh, tmat, meshes = [], [], [], [], [], []
    for k in range(10):
        x = F(k)
        pts += [(x, 0, 0), (x + F(1), 0, 0), (x + F(1), 1, 0), (x, 1, 0)]
        quad_uv = [(0, 0), (1, 0), (1, 1), (0, 1)] if k != 9 else [(-1.5, -0.25), (2.0, 0.0), (3.75, 1.0), (0.0, 2.5)]
        uvs += quad_uv if k % 2 == 0 or k == 9 else [(0.3, 0.3)] * 4  # a mesh without uvs: what stands here is not read
        idx += [(4 * k, 4 * k + 1, 4 * k + 2), (4 * k, 4 * k + 2, 4 * k + 3)]
        tmesh += [k, k]
        tmat += [k, k]
        meshes.append((False, k % 2 == 0 or k == 9, False))
    spheres = []
    for k, m in enumerate((3, 0, 7, 5)):
        o2w, w2o = _translation((F(2 * k + 1), F(2.0), F(0.0)))
        spheres.append(dict(o2w=o2w, w2o=w2o, radius=0.5, material=m))
    l2w, _ = _translation((5.0, 1.0, 4.0))
    return scenes.SceneData(
        points=np.array(pts, np.float32), uvs=np.array(uvs, np.float32), indices=np.array(idx, np.uint32), tri_mesh=np.array(tmesh, np.uint32),
        tri_material=np.array(tmat, np.int32), tri_area_light=np.full(20, -1, np.int32), meshes=meshes, materials=materials,
        lights=[dict(kind="point", l2w=l2w, I=(30.0, 30.0, 30.0))], spheres=spheres, textures=textures, split_method=abi.SPLIT_MIDDLE,
        camera=dict(position=(5.0, 1.2, 9.0), target=(5.0, 1.0, 0.0), up=(0, 1, 0), fov_axis=abi.FOV_X, fov_degrees=60.0), name="albedo-kinds",
    )  # fmt: skip


def minimal_scene():
    """Arrays as short as they can be: one triangle, one material, one mesh, no uvs, no spheres, no textures."""
    from yuki_amd import abi, scenes

    l2w, _ = _translation((0.0, 0.0, 2.0))
    return scenes.SceneData(
        points=np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.float32), indices=np.array([(0, 1, 2)], np.uint32), tri_mesh=np.zeros(1, np.uint32),
        tri_material=np.zeros(1, np.int32), tri_area_light=np.full(1, -1, np.int32), meshes=[(False, False, False)],
        materials=[dict(kind=abi.MAT_MATTE, a=(0.25, 0.5, 0.75), c=0.0)], lights=[dict(kind="point", l2w=l2w, I=(1.0, 1.0, 1.0))],
        camera=dict(position=(0.3, 0.3, 2.0), target=(0.3, 0.3, 0.0), up=(0, 1, 0), fov_axis=abi.FOV_X, fov_degrees=40.0), name="albedo-minimal",
    )  # fmt: skip


def kinds_ids(rng, w, h, sd):
    """synthetic_ids (every kind of shape index, rough barycentrics) with a third of the film's barycentrics replaced by
    ones that put uv at exactly 0 and 1 (the triangle's corners) and by ordinary interior points."""
    ids, _ = synthetic_ids(rng, w, h, sd.n_triangles, len(sd.spheres), True)
    corners = np.eye(3, dtype=np.float32)
    pick = rng.random((h, w)) < 0.15
    ids["b"][pick] = corners[rng.integers(0, 3, size=int(pick.sum()))]
    pick = rng.random((h, w)) < 0.3
    b = rng.random((int(pick.sum()), 3), dtype=np.float32)
    ids["b"][pick] = b / b.sum(-1, keepdims=True)
    return ids


# ------------------------------------------------------------------ the films and albedo records of the filter tests
SPECIAL_ALBEDO = np.array([0.0, -0.0, 0.015624999, 0.015625, 1.0, 3.5, np.nan, np.inf, -np.inf, -2.0, 1e-30], np.float32)
FILTER_SIZES = ((1, 1), (37, 23), (64, 36))
FILTER_ITERATIONS = (0, 1, 2, 5)


def make_albedo(rng, w, h):
    """A blocky texture in [0.05, 0.95] with the special channel values scattered through it."""
    y, x = np.mgrid[0:h, 0:w]
    table = (0.05 + 0.9 * rng.random((8, 8, 3))).astype(np.float32)
    a = table[(y // 3) % 8, (x // 3) % 8].copy()
    pick = rng.random((h, w, 3)) < 0.08
    a[pick] = SPECIAL_ALBEDO[rng.integers(0, len(SPECIAL_ALBEDO), size=int(pick.sum()))]
    out = np.zeros((h, w), ALBEDO_DTYPE)
    out["a"] = a
    out["known"] = (rng.random((h, w)) > 0.2).astype(np.float32)  # not read by the filter
    if w * h == 1:
        out["a"] = np.array([0.5, 0.0, np.nan], np.float32)
    return out


def filter_cases():
    """(name, film, guides, albedo, iterations, sigmas, tile_dim, samples): denoise_ref's films (NaN, +-inf, 1e30 pixels)
    times a texture, under albedo records that hold every special value, with and without a sample table."""
    rng = np.random.default_rng(20261019)
    out = []
    for w, h in FILTER_SIZES:
        albedo = make_albedo(rng, w, h)
        guides = denoise_ref.make_guides(rng, w, h)
        with np.errstate(all="ignore"):
            film = (denoise_ref.make_film(rng, w, h) * np.where(np.isfinite(albedo["a"]), albedo["a"], F(1))).astype(np.float32)
        samples = denoise_ref.make_samples(rng, w, h, 16)
        for it in FILTER_ITERATIONS:
            out.append((f"{w}x{h}-it{it}", film, guides, albedo, it, denoise_ref.SIGMAS, 16, None))
            out.append((f"{w}x{h}-it{it}-samples", film, guides, albedo, it, denoise_ref.SIGMAS, 16, samples))
    return out


def quality_error(x, ref_film, mask=None):
    """tests/test_denoise.py::quality_error (RMSE over all channels of x / (1 + x), float64), optionally over a pixel mask."""
    a = np.asarray(x, np.float64)
    b = np.asarray(ref_film, np.float64)
    d = a / (1.0 + a) - b / (1.0 + b)
    if mask is not None:
        d = d[mask]
    return float(np.sqrt(np.mean(d * d)))
