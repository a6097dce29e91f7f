"""The cases that pin shading to tests/physics_ref.py: seeded inputs, the two back ends that answer them (the CPU oracle
and the device) and the scoring of an answer against the float64 physics.

Test infrastructure only.  tests/test_physics.py (oracle), tests/test_gpu_physics.py (device) and
tools/physics_tolerances.py (calibration) all go through `run_case`, so they ask the same question of the same inputs and
differ only in the back end and the seed set.  A score is a dict of named figures:

  *_rel, *_abs, *_pos   worst error of one output over the compared rows; the tolerance comes from profiles/physics_tolerances.json
  *_mismatch            rows whose zero / no-sample / flag pattern differs from the float64 prediction; must be 0
  excluded, compared    shares of the batch left out by a predicate on the INPUTS, and compared with a non-zero value

How errors are measured is fixed here, before anything is calibrated:
  relative figures are max_c |got - ref| / max_c |ref| per row (RGB) or |got - ref| / |ref| (scalars);
  `_pos` figures are |got - ref| / max(1, |p|, |p1|): positions and position differences carry the rounding of the
  coordinates they were formed from, not of their own length;
  where an output is ill-conditioned in an input the error is multiplied by that input's conditioning factor (stated at
  the place) instead of excluding rows, because the lights' test points are drawn down to 1e-3 from the light.
"""
import ctypes as C
import functools
import json
import os

import numpy as np

import physics_ref as P
from yuki_amd import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOLERANCES = os.path.join(ROOT, "profiles", "physics_tolerances.json")
MARGIN = 4.0
FLOOR = 2.0**-23  # one f32 ulp: a figure that calibrates to exactly 0 still admits the last bit
N_STAGE = 4000
MAX_EXCLUDED, MIN_COMPARED = 0.05, 0.40
COS_CUT = 0.01

# test seeds and the disjoint calibration seeds (tools/physics_tolerances.py)
BSDF_SEED, BSDF_CALIBRATION = 7100, (9100, 9200, 9300, 9400)
LIGHT_SEEDS = {"point": 1, "spot": 2, "distant": 3, "rect": 4}  # tests/test_gpu_stages.py::test_light_sample_li_bit_exact's
LIGHT_CALIBRATION = (9500, 9600, 9700)
LI_SEED, LI_CALIBRATION = 7300, (9800, 9900)
MC_SEED = 0x5EED0F1E


def material_name(m):
    """A name that says what the material is, from its content (so the order of a list of materials does not matter)."""
    c, remap = float(m.get("c", 0.0)), "remap-" if m.get("remap") else ""
    if m["kind"] == abi.MAT_MATTE:
        return "black" if not any(m["a"]) else ("lambert" if c == 0.0 else f"oren-nayar-{c:g}")
    if m["kind"] == abi.MAT_GLASS:
        return f"glass-{c:.4g}" if c != 1.0 else "glass-1.0"
    if m["kind"] == abi.MAT_METAL:
        return f"copper-{remap}{c:g}" if abs(m["a"][0] - 0.27105) < 1e-6 else f"metal-{remap}{c:g}"
    return f"glossy-{remap}{c:g}"


def stage_materials():
    """The eight of tests/test_gpu_stages.py plus the edges: strong Oren-Nayar, the alpha clamp and alpha 1, an index-matched
    and a water pane."""
    from test_gpu_stages import MATERIALS

    out = {material_name(m): m for m in MATERIALS}
    assert len(out) == len(MATERIALS) == 8, sorted(out)
    metal = dict(kind=abi.MAT_METAL, a=(0.2, 0.9, 1.1), b=(3.9, 2.4, 2.2), remap=False)
    out["oren-nayar-1.0"] = dict(kind=abi.MAT_MATTE, a=(0.7, 0.5, 0.3), c=1.0)
    out["metal-0.001"] = dict(metal, c=0.001)
    out["metal-1.0"] = dict(metal, c=1.0)
    out["glass-1.0"] = dict(kind=abi.MAT_GLASS, a=(1, 1, 1), b=(0.9, 0.95, 1.0), c=1.0)
    out["glass-1.33"] = dict(kind=abi.MAT_GLASS, a=(1, 1, 1), b=(0.9, 0.95, 1.0), c=1.33)
    return out


EXTRA_MATERIALS = {"metal-0.0001": dict(kind=abi.MAT_METAL, a=(0.2, 0.9, 1.1), b=(3.9, 2.4, 2.2), c=0.0001, remap=False)}  # ledger only


def material(name):
    return EXTRA_MATERIALS[name] if name in EXTRA_MATERIALS else stage_materials()[name]


def mat_desc(m):
    d = abi.MaterialDesc()
    d.kind = m["kind"]
    d.a = abi.f3(m.get("a", (0, 0, 0)))
    d.b = abi.f3(m.get("b", (0, 0, 0)))
    d.c = m.get("c", 0.0)
    d.flags = 1 if m.get("remap") else 0
    return d


# ----------------------------------------------------------------------------- back ends
def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class OracleBackend:
    name = "oracle"

    def __init__(self, oracle):
        self.o = oracle
        self.factory = oracle.LightFactory

    def bsdf_eval(self, md, ng, ns, dpdu, wo, wi):
        L, n = self.o.lib(), len(wo)
        out = np.zeros((n, 3), dtype=np.float32)
        for i in range(n):
            L.orc_bsdf_eval(C.byref(md), _vp(ng[i : i + 1]), _vp(ns[i : i + 1]), _vp(dpdu[i : i + 1]), _vp(wo[i : i + 1]), _vp(wi[i : i + 1]), _vp(out[i : i + 1]))
        return out

    def bsdf_sample(self, md, ng, ns, dpdu, wo, u):
        L, n = self.o.lib(), len(wo)
        out = np.zeros((n, 8), dtype=np.float32)
        for i in range(n):
            L.orc_bsdf_sample(C.byref(md), _vp(ng[i : i + 1]), _vp(ns[i : i + 1]), _vp(dpdu[i : i + 1]), _vp(wo[i : i + 1]), _vp(u[i : i + 1]), _vp(out[i : i + 1]))
        return out

    def light_sample(self, desc, index, p, ng, u):
        out = np.zeros((len(p), 18), dtype=np.float32)
        self.o.lib().orc_light_sample(C.byref(desc), index, len(p), _vp(p), _vp(ng), _vp(u), _vp(out))
        return out

    def li(self, sd, sampler, integ, o, d, pix, si, dimension=2):
        sc = self.o.OracleScene(sd)
        try:
            return sc.li(sampler, integ, o, d, pix, si, dimension)[0]
        finally:
            sc.close()


class DeviceBackend:
    name = "device"

    def __init__(self, yk, ctx):
        self.yk, self.ctx = yk, ctx
        self.factory = yk.LightFactory

    def bsdf_eval(self, md, ng, ns, dpdu, wo, wi):
        return self.yk.bsdf_eval(self.ctx, md, ng, ns, dpdu, wo, wi)

    def bsdf_sample(self, md, ng, ns, dpdu, wo, u):
        return self.yk.bsdf_sample(self.ctx, md, ng, ns, dpdu, wo, u)

    def light_sample(self, desc, index, p, ng, u):
        return self.yk.light_sample(self.ctx, desc, index, p, ng, u)

    def li(self, sd, sampler, integ, o, d, pix, si, dimension=2):
        sc = self.yk.Scene(self.ctx, sd)
        try:
            return self.yk.IntegratorType.instantiate(self.ctx, integ).li(sc, sampler, o, d, pix, si, dimension)
        finally:
            sc.close()


# ----------------------------------------------------------------------------- figures
def _worst(err, mask):
    return float(err[mask].max()) if mask.any() else 0.0


def _rgb_rel(got, ref):
    with np.errstate(all="ignore"):
        return np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)


def _rel(got, ref):
    with np.errstate(all="ignore"):
        return np.abs(got - ref) / np.abs(ref)


def _vec_abs(got, ref):
    return np.linalg.norm(got - ref, axis=1)


# ----------------------------------------------------------------------------- BSDF stage
def bsdf_inputs(seed, tilted, n=N_STAGE):
    """Unit ns, dpdu perpendicular to it (an orthonormal frame), uniform wo and wi, u in [0,1)^2; ng = ns, or ns tilted by
    up to 0.1 so that the geometric-normal reflect / transmit filter of BSDF::f separates from the shading hemisphere."""
    rng = np.random.default_rng(seed)

    def unit(k):
        v = rng.normal(size=(k, 3))
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

    ns = unit(n)
    tilt = unit(n)
    dpdu = np.cross(ns, unit(n)).astype(np.float32)
    wo, wi = unit(n), unit(n)
    u = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    u = np.minimum(u, np.float32(1.0 - 2.0**-24))
    if tilted:
        ng = (ns + np.float32(0.1) * tilt).astype(np.float32)
        ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    else:
        ng = ns.copy()
    return dict(ng=ng, ns=ns, dpdu=dpdu, wo=wo, wi=wi, u=u)


def answer_bsdf(be, m, inp):
    md = mat_desc(m)
    return dict(f=be.bsdf_eval(md, inp["ng"], inp["ns"], inp["dpdu"], inp["wo"], inp["wi"]),
                s=be.bsdf_sample(md, inp["ng"], inp["ns"], inp["dpdu"], inp["wo"], inp["u"]))


def score_bsdf(m, inp, ans):
    """Bsdf::f and Bsdf::sample_f of one material against the physics.

    Excluded, by predicates on the inputs alone: min(|cos theta_o|, |cos theta_i|) < 0.01 against the shading normal (1/cos
    terms), |w . ng| < 1e-6 (the side test's f32 dot product decides it either way), and for sampling u0 > 0.99 (half-vector
    tan^2 = a^2 u0/(1-u0)), a disk sample within 1e-6 of the rim, a predicted wi within 0.01 of the horizon or wo.wh within
    1e-4 of 0, and |sin theta_t - 1| < 1e-5 at the edge of total internal reflection.

    The sampled f is compared with the lobe's own value at the RETURNED wi (pbrt-v3 §14.1.6 BSDF::Sample_f re-evaluates
    through the geometric filter only when several lobes match, and so does the reference); glass f is compared as
    |f - f_ref| * |cos theta_i|, i.e. as an absolute error of R*F or T*(1 - F).

    Conditioning factor (inputs only) of the sampled f and pdf of a microfacet lobe: both carry D(wh) at the sampled half
    vector, and ln D moves by 2 / (alpha^2 + tan^2 theta_h) per unit of tan^2 theta_h, which f32 forms as (1 - cos^2) / cos^2
    with a rounding of its own size near the normal.  Their relative errors are therefore multiplied by one over that
    condition number, min(1, (alpha^2 + tan^2 theta_h) / 2) at the half vector predicted from u: at the alpha clamp, where D
    alone is off by up to 22 % in f32, a pdf without its 1 / (4 wo.wh) still fails by three orders of magnitude, where the
    unscaled figure would have needed a tolerance of 0.9."""
    g = {k: P.f64(v) for k, v in inp.items()}
    n = len(g["wo"])
    fr = P.frame(g["ns"], g["dpdu"])
    wo_l, wi_l = P.to_local(g["wo"], fr), P.to_local(g["wi"], fr)
    got_f, got_s = P.f64(ans["f"]), P.f64(ans["s"])
    out = {}

    # ---- f
    side_band = (np.abs(P.dot(g["wo"], g["ng"])) < 1e-6) | (np.abs(P.dot(g["wi"], g["ng"])) < 1e-6)
    ex = (np.minimum(np.abs(wo_l[:, 2]), np.abs(wi_l[:, 2])) < COS_CUT) | side_band
    ref_f, _ = P.bsdf_f(m, g["ng"], g["ns"], g["dpdu"], g["wo"], g["wi"])
    nz_ref, nz_got = ref_f.max(axis=1) > 0, np.abs(got_f).max(axis=1) > 0
    out["f_zero_mismatch"] = int(((nz_ref != nz_got) & ~ex).sum())
    cmp_ = ~ex & nz_ref & nz_got
    out["f_rel"] = _worst(_rgb_rel(got_f, ref_f), cmp_)
    out["f_excluded"] = float(ex.mean())
    out["f_compared"] = float(cmp_.mean())

    # ---- sample_f
    wi_got_w = got_s[:, 0:3]
    wi_got = P.to_local(wi_got_w, fr)
    valid_got = got_s[:, 7] != 0
    kind = m["kind"]
    ex_s = np.abs(wo_l[:, 2]) < COS_CUT
    if kind == abi.MAT_GLASS:
        r = P.glass_sample(m, wo_l, g["u"])
        ex_s = ex_s | (np.abs(r["sin_t"] - 1.0) < 1e-5)
        valid_ref = ~r["none"]
        both = valid_ref & valid_got & ~ex_s
        out["s_valid_mismatch"] = int(((valid_ref != valid_got) & ~ex_s).sum())
        out["s_type_mismatch"] = int(((got_s[:, 7] != r["type"]) & ~ex_s).sum())
        out["s_pdf_abs"] = _worst(np.abs(got_s[:, 6] - r["pdf"]), ~ex_s)
        out["s_wi_abs"] = _worst(_vec_abs(wi_got_w, P.to_world(r["wi"], fr)), both)
        out["s_fresnel_abs"] = _worst(np.abs(got_s[:, 3:6] - r["f"]).max(axis=1) * np.abs(r["wi"][:, 2]), both)
        out["s_compared"] = float(both.mean())
    else:
        has_lobe = kind != abi.MAT_MATTE or bool(np.asarray(m["a"], dtype=np.float32).any())
        w_d = np.ones(n)
        if not has_lobe:
            wi_ref, valid_ref = np.zeros((n, 3)), np.zeros(n, dtype=bool)
        elif kind == abi.MAT_MATTE:
            wi_ref = P.cosine_hemisphere_sample(wo_l, g["u"])
            valid_ref = np.ones(n, dtype=bool)
            ex_s = ex_s | (np.abs(2.0 * g["u"] - 1.0).max(axis=1) > 1.0 - 1e-6) | (np.abs(wi_ref[:, 2]) < COS_CUT)
        else:
            alpha = P.material_alpha(m)
            wh = P.tr_sample_wh(wo_l, g["u"], alpha)
            wi_ref = P.mirror(wo_l, wh)
            woh = P.dot(wo_l, wh)
            w_d = np.minimum(1.0, 0.5 * (alpha * alpha + (1.0 - wh[:, 2] ** 2) / wh[:, 2] ** 2))
            valid_ref = (woh >= 0) & (wo_l[:, 2] * wi_ref[:, 2] > 0)
            ex_s = ex_s | (g["u"][:, 0] > 0.99) | (np.abs(wi_ref[:, 2]) < COS_CUT) | (np.abs(woh) < 1e-4)
        both = valid_ref & valid_got & ~ex_s
        out["s_valid_mismatch"] = int(((valid_ref != valid_got) & ~ex_s).sum())
        want_type = np.where(valid_ref, P.lobe_type(m), 0)
        out["s_type_mismatch"] = int(((got_s[:, 7] != want_type) & ~ex_s).sum())
        # a "no sample" is all zeros
        out["s_none_nonzero"] = int((np.abs(got_s[~valid_got & ~ex_s]).max(initial=0.0)) != 0)
        out["s_wi_abs"] = _worst(_vec_abs(wi_got_w, P.to_world(wi_ref, fr)), both)
        if has_lobe:
            with np.errstate(all="ignore"):
                f_at = P.lobe_f_local(m, wo_l, wi_got)
                pdf_at = P.lobe_pdf_local(m, wo_l, wi_got)
            out["s_f_rel"] = _worst(_rgb_rel(got_s[:, 3:6], f_at) * w_d, both)
            out["s_pdf_rel"] = _worst(_rel(got_s[:, 6], pdf_at) * w_d, both)
        out["s_compared"] = float(both.mean())
    out["s_unit_abs"] = _worst(np.abs(np.linalg.norm(wi_got_w, axis=1) - 1.0), valid_got)
    out["s_excluded"] = float(ex_s.mean())
    return out


# ----------------------------------------------------------------------------- light stage
def _rigid(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    t = rng.uniform(-4, 4, 3)
    m = np.eye(4)
    m[:3, :3] = q
    m[:3, 3] = t
    return m.astype(np.float32), np.linalg.inv(m).astype(np.float32)


def light_inputs(kind, seed, n=N_STAGE, trials=6):
    """The draws of tests/test_gpu_stages.py::test_light_sample_li_bit_exact (same generator, same order), keeping each light's
    parameters: 6 random lights, 4000 points each at 1e-3 .. 1e3 from the light's origin."""
    rng = np.random.default_rng(seed)
    out = []
    for trial in range(trials):
        l2w, l2w_inv = _rigid(rng)
        if kind == "point":
            light = dict(kind=P.POINT, l2w=l2w, I=rng.uniform(0.1, 50, 3))
        elif kind == "spot":
            total = rng.uniform(10, 80)
            light = dict(kind=P.SPOT, l2w=l2w, l2w_inv=l2w_inv, I=rng.uniform(0.1, 50, 3), total=total, falloff=rng.uniform(1, total))
        elif kind == "rect":
            light = dict(kind=P.RECT, l2w=l2w, l2w_inv=l2w_inv, L=rng.uniform(0.1, 20, 3), size=rng.uniform(0.05, 3, 2))
        else:
            w = rng.normal(size=3)
            light = dict(kind=P.DISTANT, l2w=l2w, w=w / np.linalg.norm(w), L=rng.uniform(0.1, 5, 3))
        scale = 10.0 ** rng.uniform(-3, 3, (n, 1))
        p = (l2w[:3, 3] + rng.normal(size=(n, 3)) * scale).astype(np.float32)
        ng = rng.normal(size=(n, 3))
        ng = (ng / np.linalg.norm(ng, axis=1, keepdims=True)).astype(np.float32)
        u = rng.uniform(0, 1, (n, 2)).astype(np.float32)
        out.append(dict(light=light, index=trial, p=p, ng=ng, u=u))
    return out


def light_desc(light, factory):
    d = abi.LightDesc()
    k = light["kind"]
    if k == P.POINT:
        factory.make_point_light(light["l2w"], light["I"], d)
    elif k == P.SPOT:
        factory.make_spot_light(light["l2w"], light["l2w_inv"], light["I"], light["total"], light["falloff"], d)
    elif k == P.RECT:
        factory.make_rect_light(light["l2w"], light["l2w_inv"], light["L"], light["size"], d)
    else:
        d.kind = abi.LIGHT_DISTANT
        d.p = abi.f3(light["w"])
        d.i = abi.f3(light["L"])
    return d


def answer_light(be, batch):
    return [be.light_sample(light_desc(b["light"], be.factory), b["index"], b["p"], b["ng"], b["u"]) for b in batch]


def score_light(batch, answers):
    """Light::sample_li's 18 outputs (l, Li, pdf, has-visibility, area-light id, p1, shadow ray o and d) over a batch of lights.

    Conditioning factors (inputs only).  Spot: Li is measured against the unattenuated I/d^2 and times (cos falloff_start -
    cos total_width), because the falloff's delta divides by that width.  Rectangular: the light's plane is placed by f32
    matrices, an error of position that a point at distance d sees as direction error ~1/d and, through the cosine, as
    relative pdf error ~1/h (h its height over the plane): l is measured times min(1, d), the pdf times min(1, |h|).
    Excluded: |cos - cos total_width| < 1e-6 (spot: in or out of the cone), |h| < 1e-5 (rectangular: front or back)."""
    fig = dict(l_abs=0.0, li_rel=0.0, pdf_rel=0.0, p1_pos=0.0, ray_o_pos=0.0, ray_d_pos=0.0, flag_mismatch=0, li_zero_mismatch=0)
    excluded = compared = total = 0
    for b, got in zip(batch, answers):
        light, got = b["light"], P.f64(got)
        p = P.f64(b["p"])
        r = P.light_sample(light, b["index"], p, b["ng"], b["u"])
        n = len(p)
        ex = np.zeros(n, dtype=bool)
        w_l = w_pdf = np.ones(n)
        li_scale = np.abs(r["li"]).max(axis=1)
        if light["kind"] == P.SPOT:
            ct, cf = np.cos(np.radians(light["total"])), np.cos(np.radians(light["falloff"]))
            ex = np.abs(r["cos_spot"] - ct) < 1e-6
            inten = P.f64(np.asarray(light["I"], dtype=np.float32)).max()
            li_scale = inten / (r["dist"] ** 2) / (cf - ct)
        elif light["kind"] == P.RECT:
            h = r["cos_light"] * r["dist"]
            ex = np.abs(h) < 1e-5
            w_l, w_pdf = np.minimum(1.0, r["dist"]), np.minimum(1.0, np.abs(h))
            li_scale = np.full(n, P.f64(np.asarray(light["L"], dtype=np.float32)).max())
        keep = ~ex
        nz_ref, nz_got = r["li"].max(axis=1) > 0, got[:, 3:6].max(axis=1) > 0
        fig["li_zero_mismatch"] += int(((nz_ref != nz_got) & keep).sum())
        fig["flag_mismatch"] += int((((got[:, 7] != r["has_vis"]) | (got[:, 8] != r["area_light"])) & keep).sum())
        fig["l_abs"] = max(fig["l_abs"], _worst(_vec_abs(got[:, 0:3], r["l"]) * w_l, keep))
        fig["li_rel"] = max(fig["li_rel"], _worst(np.abs(got[:, 3:6] - r["li"]).max(axis=1) / li_scale, keep))
        fig["pdf_rel"] = max(fig["pdf_rel"], _worst(_rel(got[:, 6], r["pdf"]) * w_pdf, keep))
        pos = np.maximum(1.0, np.maximum(np.linalg.norm(p, axis=1), np.linalg.norm(r["p1"], axis=1)))
        fig["p1_pos"] = max(fig["p1_pos"], _worst(_vec_abs(got[:, 9:12], r["p1"]) / pos, keep))
        fig["ray_o_pos"] = max(fig["ray_o_pos"], _worst(_vec_abs(got[:, 12:15], r["ray_o"]) / pos, keep))
        fig["ray_d_pos"] = max(fig["ray_d_pos"], _worst(_vec_abs(got[:, 15:18], r["ray_d"]) / pos, keep))
        excluded += int(ex.sum())
        compared += int((keep & nz_ref).sum())
        total += n
    fig["excluded"] = excluded / total
    fig["compared"] = compared / total
    return fig


# ----------------------------------------------------------------------------- estimator: the one-quad floor
FLOOR_HALF = 5.0
BACKGROUND = (1.0, 0.8, 0.6)
UP = np.array([0.0, 1.0, 0.0])


def _quad(y, half, up):
    """Two triangles at height y whose geometric normal (counter-clockwise front, as Triangle::intersect's cross product
    gives it) points to +y when `up`."""
    pts = np.array([(-half, y, -half), (half, y, -half), (half, y, half), (-half, y, half)], dtype=np.float32)
    idx = np.array([(0, 2, 1), (0, 3, 2)] if up else [(0, 1, 2), (0, 2, 3)], dtype=np.uint32)
    return pts, idx


def floor_scene(m, lights=(), background=(0, 0, 0), emitter=None):
    """One 10 x 10 floor quad at y = 0, normal +y.  `emitter` = (y, half): a second, downward-facing quad bound to light 0
    (the CPU-only ledger case of emission seen through a pane)."""
    pts, idx = _quad(0.0, FLOOR_HALF, True)
    mats = [m]
    tri_mat, tri_al, meshes = [0, 0], [-1, -1], [(False, False, False)]
    tri_mesh = [0, 0]
    if emitter is not None:
        p2, i2 = _quad(emitter[0], emitter[1], False)
        idx = np.concatenate([idx, i2 + np.uint32(len(pts))])
        pts = np.concatenate([pts, p2])
        mats = mats + [dict(kind=abi.MAT_MATTE, a=(0, 0, 0), c=0.0)]
        tri_mat += [1, 1]
        tri_al += [0, 0]
        tri_mesh += [1, 1]
        meshes.append((False, False, False))
    return scenes.SceneData(
        points=pts, indices=idx, tri_mesh=np.asarray(tri_mesh, dtype=np.uint32), tri_material=np.asarray(tri_mat, dtype=np.int32),
        tri_area_light=np.asarray(tri_al, dtype=np.int32), meshes=meshes, materials=mats, lights=list(lights), background=tuple(background),
        name="physics-floor",
    )


def _sampler(n, seed=MC_SEED):
    return abi.SamplerDesc(abi.SAMPLER_UNIFORM, int(n), 1, 1, seed)


def _path(depth):
    return abi.IntegratorDesc(abi.INTEGRATOR_PATH, depth, 0, 0.0)


def _translate(v):
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = v
    mi = np.eye(4, dtype=np.float32)
    mi[:3, 3] = -np.asarray(v, dtype=np.float32)
    return m, mi


def _aim(pos, direction):
    """Rigid light-to-world matrix that puts local +z (a spot light's axis) along `direction` at `pos`."""
    z = np.asarray(direction, dtype=np.float64)
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0] if abs(z[2]) < 0.9 else [1.0, 0.0, 0.0], z)
    x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, pos
    return m.astype(np.float32), np.linalg.inv(m).astype(np.float32)


def direct_lights():
    """name -> (scene light dict, physics light dict) for the depth-1 cases."""
    pm, _ = _translate((1.0, 3.0, -0.5))
    sm, smi = _aim((-1.0, 4.0, 1.0), (0.2, -1.0, 0.1))
    w = np.array([0.3, 1.0, 0.2])
    w = (w / np.linalg.norm(w)).astype(np.float32)
    return {
        "point": (dict(kind="point", l2w=pm, I=(20.0, 15.0, 10.0)), dict(kind=P.POINT, l2w=pm, I=(20.0, 15.0, 10.0))),
        "spot": (dict(kind="spot", l2w=sm, l2w_inv=smi, I=(40.0, 30.0, 20.0), total_width=40.0, falloff_start=25.0),
                 dict(kind=P.SPOT, l2w=sm, I=(40.0, 30.0, 20.0), total=40.0, falloff=25.0)),
        "distant": (dict(kind="distant", w=w, L=(2.0, 1.5, 1.0)), dict(kind=P.DISTANT, l2w=np.eye(4), w=w, L=(2.0, 1.5, 1.0))),
    }


DIRECT_MATERIALS = {"lambert": dict(kind=abi.MAT_MATTE, a=(0.7, 0.5, 0.3), c=0.0), "oren-nayar": dict(kind=abi.MAT_MATTE, a=(0.7, 0.5, 0.3), c=0.349)}


def direct_rays(seed, n=2000):
    """Rays from above onto random floor points within [-4, 4]^2, at up to ~84 degrees from the normal."""
    rng = np.random.default_rng(seed)
    hit = np.stack([rng.uniform(-4, 4, n), np.zeros(n), rng.uniform(-4, 4, n)], axis=-1)
    cos = rng.uniform(0.1, 1.0, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    s = np.sqrt(1 - cos * cos)
    back = np.stack([s * np.cos(phi), cos, s * np.sin(phi)], axis=-1)
    o = (hit + back * rng.uniform(1.0, 6.0, (n, 1))).astype(np.float32)
    d = hit - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return o, d


def _floor_hit(o, d):
    o, d = P.f64(o), P.f64(d)
    t = -o[:, 1] / d[:, 1]
    return o + t[:, None] * d


def _floor_f(m, wo, wi):
    n = len(wo)
    up = np.broadcast_to(UP, (n, 3))
    return P.bsdf_f(m, up, up, np.broadcast_to(np.array([1.0, 0.0, 0.0]), (n, 3)), wo, wi)[0]


def run_direct(be, mat, light, seed):
    """Path::li at depth 1: one hit, one light, no occluder — Li_o = f(wo, l) Li max(0, n.l) / pdf per ray (pbrt-v3 §14.3
    EstimateDirect for a delta light).  Excluded: the spot cone's edge (|cos - cos total_width| < 1e-6)."""
    m = DIRECT_MATERIALS[mat]
    sl, pl = direct_lights()[light]
    o, d = direct_rays(seed)
    n = len(o)
    got = P.f64(be.li(floor_scene(m, [sl]), _sampler(1), _path(1), o, d, np.zeros((n, 2), np.uint16), np.zeros(n, np.uint32)))
    p = _floor_hit(o, d)
    up = np.broadcast_to(UP, (n, 3))
    r = P.light_sample(pl, 0, p, up, np.zeros((n, 2)))
    ref = _floor_f(m, -P.f64(d), r["l"]) * r["li"] * np.clip(r["l"] @ UP, 0.0, None)[:, None] / r["pdf"][:, None]
    ex = np.zeros(n, dtype=bool)
    scale = np.abs(ref).max(axis=1)
    if light == "spot":  # measured against the unattenuated value: the falloff's relative error is unbounded at the cone's edge
        ex = np.abs(r["cos_spot"] - np.cos(np.radians(pl["total"]))) < 1e-6
        full = P.light_sample(dict(pl, kind=P.POINT), 0, p, up, np.zeros((n, 2)))
        scale = (_floor_f(m, -P.f64(d), r["l"]) * full["li"] * np.clip(r["l"] @ UP, 0.0, None)[:, None]).max(axis=1)
    nz_ref, nz_got = ref.max(axis=1) > 0, got.max(axis=1) > 0
    cmp_ = ~ex & nz_ref & nz_got
    with np.errstate(all="ignore"):
        err = np.abs(got - ref).max(axis=1) / scale
    return dict(li_rel=_worst(err, cmp_), li_zero_mismatch=int(((nz_ref != nz_got) & ~ex).sum()), excluded=float(ex.mean()), compared=float(cmp_.mean()))


# ---- Monte-Carlo cases: N sample indices of one pixel, Uniform sampler, the same ray
def _ray_at(angle_deg, hit=(0.0, 0.0, 0.0), from_below=False):
    a = np.radians(angle_deg)
    d = np.array([np.sin(a), np.cos(a) if from_below else -np.cos(a), 0.0])
    o = np.asarray(hit, dtype=np.float64) - 3.0 * d
    return o.astype(np.float32), d.astype(np.float32)


def li_samples(be, sd, depth, o, d, n, dimension=2, seed=MC_SEED):
    """li of one ray for sample indices 0 .. n-1 of pixel (3, 5)."""
    oo = np.broadcast_to(o, (n, 3)).copy()
    dd = np.broadcast_to(d, (n, 3)).copy()
    pix = np.broadcast_to(np.array([3, 5], dtype=np.uint16), (n, 2)).copy()
    return P.f64(be.li(sd, _sampler(n, seed), _path(depth), oo, dd, pix, np.arange(n, dtype=np.uint32), dimension))


def mc_figures(samples, truth):
    """Mean of the brightest channel of `truth` against it: (z, relative standard error, mean, truth)."""
    c = int(np.argmax(truth))
    x = samples[:, c]
    se = x.std(ddof=1) / np.sqrt(len(x))
    return dict(z=float((x.mean() - truth[c]) / se) if se > 0 else (0.0 if x.mean() == truth[c] else np.inf), rel_se=float(se / truth[c]), mean=float(x.mean()), truth=float(truth[c]))


FURNACE_MATERIALS = {
    "oren-nayar": dict(kind=abi.MAT_MATTE, a=(0.7, 0.5, 0.3), c=0.349),
    "metal-0.2": dict(kind=abi.MAT_METAL, a=(0.2, 0.9, 1.1), b=(3.9, 2.4, 2.2), c=0.2, remap=False),
    "copper": dict(kind=abi.MAT_METAL, a=(0.27105, 0.67693, 1.31640), b=(3.60920, 2.62480, 2.29210), c=0.01, remap=True),
    "glossy-0.3": dict(kind=abi.MAT_GLOSSY, a=(0.8, 0.6, 0.2), c=0.3, remap=False),
    "glass": dict(kind=abi.MAT_GLASS, a=(1, 1, 1), b=(1, 1, 1), c=1.5),
}
FURNACE_ANGLES = (10, 45, 75)
RECT_POINTS = ((0.5, 0.0, -0.3), (2.0, 0.0, 1.0), (-3.0, 0.0, 0.5), (0.0, 0.0, -2.5))
RECT = dict(pos=(0.5, 2.0, -0.3), size=(1.5, 1.0), L=(5.0, 4.0, 3.0))
LIGHT_BELOW = dict(kind="point", l2w=_translate((0.5, -2.0, 0.25))[0], I=(30.0, 30.0, 30.0))


def mc_cases():
    """name -> spec of every Monte-Carlo case (furnace, furnace with a light below the floor, rectangular light)."""
    out = {}
    for mat in FURNACE_MATERIALS:
        for a in FURNACE_ANGLES:
            out[f"furnace/{mat}/{a}"] = dict(kind="furnace", mat=mat, angle=a, below=False)
    for mat in FURNACE_MATERIALS:  # quirk 4: the whole furnace again with a point light below the floor
        for a in FURNACE_ANGLES:
            out[f"furnace-light-below/{mat}/{a}"] = dict(kind="furnace", mat=mat, angle=a, below=True)
    for k in range(len(RECT_POINTS)):
        out[f"rect/{k}"] = dict(kind="rect", point=k)
    return out


@functools.lru_cache(maxsize=None)
def _albedo(mat, angle, mutation, off):
    return P.directional_albedo(FURNACE_MATERIALS[mat], np.cos(np.radians(angle)))


def mc_truth(spec):
    """The float64 expectation of a Monte-Carlo case's li (RGB)."""
    if spec["kind"] == "furnace":
        if spec["mat"] == "glass":  # R = T = 1: F B + (1 - F) B
            return P.f64(BACKGROUND)
        return P.f64(BACKGROUND) * _albedo(spec["mat"], spec["angle"], P._MUTATION, tuple(sorted(P._OFF)))
    # Lambert floor under the rectangular light: Kd/pi * L * E(polygon of unit radiance)
    cx, cy, cz = RECT["pos"]
    hx, hz = RECT["size"][0] / 2, RECT["size"][1] / 2
    verts = [(cx - hx, cy, cz - hz), (cx + hx, cy, cz - hz), (cx + hx, cy, cz + hz), (cx - hx, cy, cz + hz)]
    e = P.polygon_irradiance(RECT_POINTS[spec["point"]], UP, verts)
    return P.lambert_f(DIRECT_MATERIALS["lambert"]["a"]) * P.f64(RECT["L"]) * e


def mc_samples(be, spec, n):
    if spec["kind"] == "furnace":
        o, d = _ray_at(spec["angle"])
        sd = floor_scene(FURNACE_MATERIALS[spec["mat"]], [LIGHT_BELOW] if spec["below"] else [], BACKGROUND)
        return li_samples(be, sd, 2, o, d, n)
    m, mi = _translate(RECT["pos"])
    sd = floor_scene(DIRECT_MATERIALS["lambert"], [dict(kind="rect", l2w=m, l2w_inv=mi, L=RECT["L"], size=RECT["size"])])
    hit = np.asarray(RECT_POINTS[spec["point"]])
    d = np.array([0.3, -1.0, 0.1])
    d /= np.linalg.norm(d)
    return li_samples(be, sd, 1, (hit - 2.0 * d).astype(np.float32), d.astype(np.float32), n)


def run_furnace_exact(be, mat, seed=MC_SEED):
    """Depth 2 over one floor under a uniform background B, no lights: a Lambert floor returns Kd * B on every sample (f cos /
    pdf = Kd exactly for cosine sampling), a black one 0."""
    m = dict(kind=abi.MAT_MATTE, a=(0.7, 0.5, 0.3) if mat == "lambert" else (0, 0, 0), c=0.0)
    worst = 0.0
    for a in FURNACE_ANGLES:
        o, d = _ray_at(a)
        got = li_samples(be, floor_scene(m, [], BACKGROUND), 2, o, d, 256, seed=seed)
        ref = P.f64(np.asarray(m["a"], dtype=np.float32)) * P.f64(BACKGROUND)
        if mat == "lambert":
            worst = max(worst, float((np.abs(got - ref) / ref).max()))
        else:
            worst = max(worst, float(np.abs(got).max()))
    return dict(li_rel=worst) if mat == "lambert" else dict(li_abs=worst)


def run_dimension_shift(be):
    """Quirk 4 per sample: a point light below the floor contributes nothing and consumes two dimensions, so every sample
    equals the light-less scene's started two dimensions later, and not the light-less scene's at the same dimension.
    -> (mismatches against the expectation, rows where the two light-less runs differ)."""
    o, d = _ray_at(45)
    m = FURNACE_MATERIALS["metal-0.2"]
    with_light = li_samples(be, floor_scene(m, [LIGHT_BELOW], BACKGROUND), 2, o, d, 256)
    bare = floor_scene(m, [], BACKGROUND)
    same_dim = li_samples(be, bare, 2, o, d, 256, dimension=2)
    shifted = li_samples(be, bare, 2, o, d, 256, dimension=4)
    want = shifted if P._on("nee_consumes_dimensions") else same_dim
    return dict(shift_mismatch=int((with_light != want).any(axis=1).sum()), shift_rows_differing=int((same_dim != shifted).any(axis=1).sum()))


def run_emitter_through_pane(be):
    """Quirk 2 per sample: an index-matched pane (eta 1, R = T = 1) under a downward-facing emitter, seen from below.  A
    sample that picks transmission carries beta = T (1 - F) / 0.5 = 2 and finds Le after a specular bounce: the reference adds
    beta^2 Le = 4 Le, a path tracer beta Le = 2 Le; a sample that picks reflection has F = 0 and ends black."""
    le = (3.0, 2.0, 1.0)
    m, mi = _translate((0.0, 2.0, 0.0))
    pane = dict(kind=abi.MAT_GLASS, a=(1, 1, 1), b=(1, 1, 1), c=1.0)
    sd = floor_scene(pane, [dict(kind="rect", l2w=m, l2w_inv=mi, L=le, size=(2.0, 2.0))], (0, 0, 0), emitter=(2.0, 1.0))
    o, d = _ray_at(10, from_below=True)
    got = li_samples(be, sd, 3, o, d, 256)
    lit = got.max(axis=1) > 0
    beta = 2.0
    want = P.f64(le) * (beta * beta if P._on("emission_beta_squared") else beta)
    return dict(emission_rel=_worst(_rgb_rel(got, np.broadcast_to(want, got.shape)), lit), lit_share=float(lit.mean()))


# ----------------------------------------------------------------------------- one entry point per deterministic case
def deterministic_cases():
    """id -> (kind, arguments, test seed, calibration seeds) of every deterministic case the tests run."""
    out = {}
    for name in stage_materials():
        for tilted in (False, True):
            out[f"bsdf/{name}/{'tilted' if tilted else 'ortho'}"] = ("bsdf", (name, tilted), BSDF_SEED + (1 if tilted else 0), BSDF_CALIBRATION)
    for kind in LIGHT_SEEDS:
        out[f"light/{kind}"] = ("light", (kind,), LIGHT_SEEDS[kind], LIGHT_CALIBRATION)
    for mat in DIRECT_MATERIALS:
        for light in direct_lights():
            out[f"direct/{mat}/{light}"] = ("direct", (mat, light), LI_SEED, LI_CALIBRATION)
    for mat in ("lambert", "black"):
        out[f"furnace-exact/{mat}"] = ("furnace-exact", (mat,), MC_SEED, (MC_SEED + 1, MC_SEED + 2))
    return out


_ANSWERS = {}


def run_case(be, case_id, seed=None, cache=True):
    """Score of one deterministic case on one back end; `seed` None = the test seed.  Stage answers are cached per (back end,
    case, seed), so re-scoring under `P.textbook` / `P.mutated` costs no second run."""
    kind, args, test_seed, _ = all_cases()[case_id]
    seed = test_seed if seed is None else seed
    key = (be.name, case_id, seed)
    if kind == "bsdf":
        name, tilted = args
        m = material(name)
        inp = bsdf_inputs(seed, tilted)
        if not cache or key not in _ANSWERS:
            _ANSWERS[key] = answer_bsdf(be, m, inp)
        return score_bsdf(m, inp, _ANSWERS[key])
    if kind == "light":
        batch = light_inputs(args[0], seed)
        if not cache or key not in _ANSWERS:
            _ANSWERS[key] = answer_light(be, batch)
        return score_light(batch, _ANSWERS[key])
    if kind == "direct":
        return run_direct(be, args[0], args[1], seed)
    return run_furnace_exact(be, args[0], seed)


def all_cases():
    out = deterministic_cases()
    out["bsdf/metal-0.0001/ortho"] = ("bsdf", ("metal-0.0001", False), BSDF_SEED, BSDF_CALIBRATION)  # the alpha clamp's ledger case
    return out


# ----------------------------------------------------------------------------- tolerances
@functools.lru_cache(maxsize=1)
def tolerances():
    with open(TOLERANCES) as fh:
        return json.load(fh)


def is_toleranced(figure):
    return figure.endswith(("_rel", "_abs", "_pos"))


def tolerance(case_id, figure):
    return tolerances()["rows"][f"{case_id}:{figure}"]["tolerance"]


def adopt(worst):
    return max(MARGIN * worst, FLOOR)


def check_score(case_id, score):
    """The assertions every deterministic case makes of its score; returns the list of failures (empty = pass)."""
    bad = []
    for k, v in score.items():
        if is_toleranced(k):
            if not v <= tolerance(case_id, k):
                bad.append(f"{case_id}:{k} = {v:.3e} > {tolerance(case_id, k):.3e}")
        elif k.endswith(("_mismatch", "_nonzero")):
            if v != 0:
                bad.append(f"{case_id}:{k} = {v}")
        elif k.endswith("excluded"):
            if not v <= MAX_EXCLUDED:
                bad.append(f"{case_id}:{k} = {v:.3f} > {MAX_EXCLUDED}")
    return bad


Z_MAX = 4.0


def _show(case_id, score):
    print(case_id, {k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in score.items()})


def check_deterministic(be, case_id):
    """What a test of one deterministic case asserts, on either back end."""
    score = run_case(be, case_id)
    _show(case_id, score)
    assert check_score(case_id, score) == []
    if case_id.startswith("bsdf/"):
        m = material(case_id.split("/")[1])
        has_lobe = m["kind"] in (abi.MAT_METAL, abi.MAT_GLOSSY) or (m["kind"] == abi.MAT_MATTE and any(m["a"]))
        if has_lobe:  # same-hemisphere pairs are half of a batch; at least 40 % of the batch carries a compared, non-zero f
            assert score["f_compared"] >= MIN_COMPARED
        if m["kind"] != abi.MAT_MATTE or any(m["a"]):
            assert score["s_compared"] >= MIN_COMPARED
    elif "compared" in score:
        assert score["compared"] > 0.1


def check_monte_carlo(be, name):
    """What a test of one Monte-Carlo case asserts: |mean - truth| within 4 standard errors at the recorded N."""
    spec = mc_cases()[name]
    rec = tolerances()["monte_carlo"][name]
    fig = mc_figures(mc_samples(be, spec, rec["n"]), mc_truth(spec))
    print(name, "N", rec["n"], fig)
    assert fig["rel_se"] <= 0.01 or rec["n"] == 65536
    assert abs(fig["z"]) <= Z_MAX
