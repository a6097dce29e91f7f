"""The cases that pin shading to tests/physics_ref.py: seeded inputs, the two back ends that answer them (the CPU oracle
and the device) and the scoring of an answer against the float64 physics.

Test infrastructure only.  tests/test_physics.py (oracle), tests/test_gpu_physics.py (device) and
tools/physics_tolerances.py (calibration) all go through `run_case`, so they ask the same question of the same inputs and
differ only in the back end and the seed set.  A score is a dict of named figures:

  *_rel, *_abs, *_pos   worst error of one output over the compared rows; the tolerance comes from profiles/physics_tolerances.json
  *_mismatch            rows whose zero / no-sample / flag / cell / ray-count pattern differs from the float64 prediction; must be 0
  *_z                   |z| of observed counts against their float64 probabilities; at most Z_MAX, like every statistical bound
  excluded, compared    shares of the batch left out by a predicate on the INPUTS, and compared with a non-zero value
  *_rows                how many compared rows took one branch of the code under test; the case built for a branch asserts it has rows

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
Z_MAX = 4.0
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

    def camera_rays(self, cam, res, sampler, tile, sample_index):
        return self.o.camera_rays(self.o.make_camera(cam, res), sampler, tile, sample_index)

    def sampler_sequence(self, sampler, px, py, sample_index, dims):
        dims = np.ascontiguousarray(dims, dtype=np.uint8)
        out = np.zeros((len(dims), 2), dtype=np.float32)
        self.o.lib().orc_sampler_sequence(C.byref(sampler), px, py, sample_index, _vp(dims), len(dims), _vp(out))
        return out

    def li(self, sd, sampler, integ, o, d, pix, si, dimension=2):
        sc = self.o.OracleScene(sd)
        try:
            return sc.li(sampler, integ, o, d, pix, si, dimension)[0]
        finally:
            sc.close()

    def surface(self, sd, o, d, route=0):
        """orc_surface: the oracle has one way to the surface, `route` is ignored."""
        sc = self.o.OracleScene(sd)
        try:
            return sc.surface(o, d)
        finally:
            sc.close()

    def li_counts(self, sd, sampler, integ, o, d, pix, si, dimension=2):
        """(li, closest-hit rays per sample)"""
        sc = self.o.OracleScene(sd)
        try:
            li, rays = sc.li(sampler, integ, o, d, pix, si, dimension)
            return li, rays.astype(np.int64)
        finally:
            sc.close()


class NullBackend:
    """Answers nothing but zeros: what is left of a score is what the float64 reference alone decides — the excluded share."""

    name = "null"

    def surface(self, sd, o, d, route=0):
        return np.zeros((len(o), abi.SURFACE_FLOATS), dtype=np.float32)

    def li(self, sd, sampler, integ, o, d, pix, si, dimension=2):
        return np.zeros((len(o), 3), dtype=np.float32)


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

    def camera_rays(self, cam, res, sampler, tile, sample_index):
        return self.yk.camera_rays(self.ctx, self.yk.Camera(cam, self.yk.FilmSettings(res=tuple(res))), sampler, tile, sample_index)

    def sampler_sequence(self, sampler, px, py, sample_index, dims):
        return self.yk.sampler_sequence(self.ctx, sampler, px, py, sample_index, dims)

    def li(self, sd, sampler, integ, o, d, pix, si, dimension=2):
        sc = self.yk.Scene(self.ctx, sd)
        try:
            return self.yk.IntegratorType.instantiate(self.ctx, integ).li(sc, sampler, o, d, pix, si, dimension)
        finally:
            sc.close()

    def surface(self, sd, o, d, route=0):
        sc = self.yk.Scene(self.ctx, sd)
        try:
            return self.yk.surface(self.ctx, sc, o, d, route)
        finally:
            sc.close()

    def li_counts(self, sd, sampler, integ, o, d, pix, si, dimension=2):
        """(li, closest-hit rays per sample).  li is yk_li's; so are Whitted's counts.  The wavefront that serves Path keeps no
        per-sample count, so a Path integrator's are yk_li_debug's (the per-sample kernel, without records)."""
        sc = self.yk.Scene(self.ctx, sd)
        try:
            integrator = self.yk.IntegratorType.instantiate(self.ctx, integ)
            if integ.kind != abi.INTEGRATOR_PATH:
                li, counts = integrator.li(sc, sampler, o, d, pix, si, dimension, ray_counts=True)
                return li, counts.astype(np.int64)
            li = integrator.li(sc, sampler, o, d, pix, si, dimension)
            return li, integrator.li_debug_records(sc, sampler, o, d, pix, si, dimension, 0)[1].astype(np.int64)
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
    out["floor-under-pane"] = dict(kind="floor-under-pane")  # diffuse and specular vertices mixed, max_depth 64
    return out


UNDER_PANE = dict(rho=(0.5, 0.4, 0.3), eta=1.5, gap=0.01, thick=0.01, half=100.0, depth=64)


def under_pane_bias():
    """Upper bound, relative to the truth's brightest channel, on what separates the expectation of the floor-under-pane case
    from P.floor_under_pane's infinite plates and unbounded depth.
    Depth: P.floor_under_pane(max_depth=64) is the truncated expectation itself.
    Width: a path reaches the plates' edge only if one of its first n crossings of the gap runs at least half / (2 n) sideways (the
    other half of the width is left to the travel inside the pane, under 64 * thick); a cosine-distributed direction does so with
    probability 1 / (1 + (half / (2 n gap))^2); the n-th crossing carries at most rho_max^floor(n / 2) of the radiance (one floor vertex
    per two crossings; the pane's vertices have expected weight 1 in total); and what the path then finds differs from what it
    should by at most the background."""
    u = UNDER_PANE
    rho = P.f64(np.asarray(u["rho"], dtype=np.float32))
    full, cut = P.floor_under_pane(rho, u["eta"]), P.floor_under_pane(rho, u["eta"], u["depth"])
    c = int(np.argmax(full * P.f64(BACKGROUND)))
    depth_bias = abs(full[c] - cut[c]) / full[c]
    width_bias = sum(rho.max() ** (n // 2) * min(1.0, n / (1.0 + (u["half"] / (2.0 * n * u["gap"])) ** 2)) for n in range(1, u["depth"] + 1)) / full[c]
    return float(depth_bias + width_bias)


@functools.lru_cache(maxsize=None)
def _albedo(mat, angle, mutation, off):
    return P.directional_albedo(FURNACE_MATERIALS[mat], np.cos(np.radians(angle)))


def mc_truth(spec):
    """The float64 expectation of a Monte-Carlo case's li (RGB)."""
    if spec["kind"] == "floor-under-pane":
        return P.f64(BACKGROUND) * P.floor_under_pane(np.asarray(UNDER_PANE["rho"], dtype=np.float32), UNDER_PANE["eta"])
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
    if spec["kind"] == "floor-under-pane":  # the ray starts in the gap and hits the floor first
        u = UNDER_PANE
        sd = pane_scene([(u["gap"], u["gap"] + u["thick"])], GLASSES["clear"], dict(kind=abi.MAT_MATTE, a=u["rho"], c=0.0), half=u["half"])
        d = np.array([0.3, -1.0, 0.1])
        d /= np.linalg.norm(d)
        return li_samples(be, sd, u["depth"], np.array([0.0, 0.5 * u["gap"], 0.0], dtype=np.float32), d.astype(np.float32), n)
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


# ----------------------------------------------------------------------------- camera stage
CAMERA_RESOLUTIONS = ((1, 1), (17, 9), (9, 17), (1920, 1080), (4096, 2160))
CAMERA_SEED, CAMERA_CALIBRATION = 7400, (9150, 9250, 9350)
SAMPLER_SEED = 0x73B9642E74AC471C  # tests/test_gpu_stages.py's


def camera_specs():
    """name -> (fov axis, fov degrees, pose): 1, 90 and 170 degrees along either axis from a camera near the origin, one camera
    1e4 away from it and one looking straight down with up = +z."""
    out = {}
    for axis, a in ((P.FOV_X, "x"), (P.FOV_Y, "y")):
        for fov in (1, 90, 170):
            out[f"camera/{a}{fov}"] = (axis, float(fov), "near")
    out["camera/far"] = (P.FOV_X, 60.0, "far")
    out["camera/down"] = (P.FOV_Y, 60.0, "down")
    return out


def camera_pose(spec, rng):
    axis, fov, pose = spec
    v = rng.normal(size=3)
    v /= np.linalg.norm(v)
    if abs(v[1]) > 0.9:  # not along the up vector
        v = np.array([v[1], v[0], v[2]])
    up = (0.0, 1.0, 0.0)
    pos = rng.uniform(-10, 10, 3)
    if pose == "far":
        pos = rng.uniform(0.5, 2.0, 3) * 1e4 * rng.choice([-1.0, 1.0], 3)
    if pose == "down":
        v, up = np.array([0.0, -1.0, 0.0]), (0.0, 0.0, 1.0)
    pos = pos.astype(np.float32)
    target = (pos + (v * rng.uniform(1, 20)).astype(np.float32)).astype(np.float32)
    return dict(position=tuple(float(x) for x in pos), target=tuple(float(x) for x in target), up=up, fov_axis=axis, fov_degrees=fov)


def camera_tiles(res, rng):
    """A 1 x 1, a 5 x 3 (15 lanes) and a 16 x 16 tile at random places and the film's clipped corner tile, each clipped to the film."""
    rx, ry = res
    out = []
    for w, h in ((1, 1), (5, 3), (16, 16)):
        x0, y0 = int(rng.integers(0, max(1, rx - w + 1))), int(rng.integers(0, max(1, ry - h + 1)))
        out.append((x0, y0, min(rx, x0 + w), min(ry, y0 + h)))
    out.append((((rx - 1) // 16) * 16, ((ry - 1) // 16) * 16, rx, ry))
    return sorted(set(out))


def _tile_pixels(tile):
    x0, y0, x1, y1 = tile
    xs, ys = np.meshgrid(np.arange(x0, x1), np.arange(y0, y1))  # row by row, as the tile's rays are stored
    return np.stack([xs.ravel(), ys.ravel()], axis=-1).astype(np.float64)


def _stratified(nx, ny, jitter, seed=SAMPLER_SEED):
    return abi.SamplerDesc(abi.SAMPLER_STRATIFIED, nx, ny, 1 if jitter else 0, seed)


def run_camera(be, name, seed):
    """yk_camera_init + yk_camera_rays (oracle: Camera::new + Camera::ray) against the float64 pinhole camera, over the five
    resolutions.  The sampler is Stratified (1, 1) without jitter, so the film point is the pixel's centre exactly.  Figures: origin
    against the position (relative to |position|), angle between the direction and float64's, | |d| - 1 |, the angle between the ray
    through the film's centre and normalize(target - position) (resolutions with a centre pixel: both extents odd), and the angle
    between the film's two edges on the fov axis, found from the first and last pixel of the middle row or column, against the fov."""
    spec = camera_specs()[name]
    rng = np.random.default_rng(seed)
    cam = camera_pose(spec, rng)
    s11 = _stratified(1, 1, False)
    pos = P.f64(cam["position"])
    fig = dict(o_rel=0.0, d_angle_abs=0.0, d_unit_abs=0.0, centre_angle_abs=0.0, fov_abs=0.0)
    for res in CAMERA_RESOLUTIONS:
        for tile in camera_tiles(res, rng):
            o, d = (P.f64(a) for a in be.camera_rays(cam, res, s11, tile, 0))
            ref_o, ref_d = P.camera_ray(cam, res, _tile_pixels(tile) + 0.5)
            assert o.shape == ref_o.shape
            fig["o_rel"] = max(fig["o_rel"], float(np.linalg.norm(o - ref_o, axis=1).max() / np.linalg.norm(pos)))
            fig["d_angle_abs"] = max(fig["d_angle_abs"], float(P.angle_between(d, ref_d).max()))
            fig["d_unit_abs"] = max(fig["d_unit_abs"], float(np.abs(np.linalg.norm(d, axis=1) - 1.0).max()))
        rx, ry = res
        if rx % 2 and ry % 2:
            _, d = be.camera_rays(cam, res, s11, (rx // 2, ry // 2, rx // 2 + 1, ry // 2 + 1), 0)
            fig["centre_angle_abs"] = max(fig["centre_angle_abs"], float(P.angle_between(d[0], P.camera_basis(cam)[2])))
        n_axis = rx if cam["fov_axis"] == P.FOV_X else ry
        if n_axis > 1:
            ends = [(0, ry // 2), (rx - 1, ry // 2)] if cam["fov_axis"] == P.FOV_X else [(rx // 2, 0), (rx // 2, ry - 1)]
            d0, d1 = (be.camera_rays(cam, res, s11, (x, y, x + 1, y + 1), 0)[1][0] for x, y in ends)
            fig["fov_abs"] = max(fig["fov_abs"], float(abs(P.camera_fov_from_rays(cam, res, d0, d1) - np.radians(cam["fov_degrees"]))))
    return fig


JITTER_RES, JITTER_GRID = (96, 54), (4, 4)


def run_camera_jitter(be, seed):
    """k_raygen's own use of the sampler: Stratified (4, 4) with jitter, every sample index over one 16 x 16 tile.  Each ray is
    projected back to the raster in float64; the offset from its pixel's corner must lie in the unit square (`film_inside_abs`: how
    far outside it lies, a toleranced figure because the projection carries the ray's f32 rounding) and, for a 4 x 4 grid of the
    tile's pixels, equal the first 2-D draw the sampler stage gives for that pixel and sample index (`film_offset_abs`, in pixels)."""
    rng = np.random.default_rng(seed)
    cam = camera_pose((P.FOV_X, 60.0, "near"), rng)
    s = _stratified(*JITTER_GRID, True, SAMPLER_SEED + (seed - CAMERA_SEED))
    x0, y0 = int(rng.integers(0, JITTER_RES[0] - 15)), int(rng.integers(0, JITTER_RES[1] - 15))
    tile = (x0, y0, x0 + 16, y0 + 16)
    pix = _tile_pixels(tile)
    picked = [k for k in range(256) if (k % 16) % 5 == 0 and (k // 16) % 5 == 0]
    fig = dict(film_inside_abs=0.0, film_offset_abs=0.0)
    for idx in range(JITTER_GRID[0] * JITTER_GRID[1]):
        _, d = be.camera_rays(cam, JITTER_RES, s, tile, idx)
        off = P.camera_raster(cam, JITTER_RES, d) - pix
        fig["film_inside_abs"] = max(fig["film_inside_abs"], float(np.maximum(-off, off - 1.0).max(initial=0.0)))
        for k in picked:
            u = P.f64(be.sampler_sequence(s, int(pix[k, 0]), int(pix[k, 1]), idx, [2]))[0]
            fig["film_offset_abs"] = max(fig["film_offset_abs"], float(np.abs(off[k] - u).max()))
    fig["film_inside_abs"] = max(fig["film_inside_abs"], 0.0)
    return fig


# ----------------------------------------------------------------------------- sampler stage: structure, no oracle needed
SQUARE_GRIDS = ((1, 1), (2, 2), (3, 3), (5, 5), (8, 8))  # spp 1, 4, 9, 25, 64: the odd ones walk the permutation's cycles
RECT_GRIDS = ((4, 2), (2, 4), (5, 3), (1, 7))
SAMPLER_PIXEL = (3, 5)


def _draws(be, s, pixel, spp, dims):
    """(spp, len(dims), 2): the draws `dims` of every sample index of one pixel."""
    return np.stack([be.sampler_sequence(s, pixel[0], pixel[1], idx, dims) for idx in range(spp)])


def _multiset_difference(a, b):
    from collections import Counter

    ca, cb = Counter(a), Counter(b)
    return sum(((ca - cb) + (cb - ca)).values())


def run_strata_1d(be, seed):
    """Stratified get_1d for a fixed pixel at dimensions 0, 1 and 2 over the spp sample indices: floor(u spp) is a permutation of
    0 .. spp-1 — and the very one Kensler's algorithm gives in Python integers for the hashed (pixel, dimension, seed); every
    value lies in [0,1); without jitter u is (k + 1/2) / spp rounded to f32 exactly."""
    from test_oracle_sampler import stratum_py

    fig = dict(perm_mismatch=0, stratum_mismatch=0, range_mismatch=0, centre_mismatch=0)
    for n, _ in SQUARE_GRIDS:
        spp = n * n
        want = np.array([[stratum_py(*SAMPLER_PIXEL, dim, seed, idx, spp) for dim in range(3)] for idx in range(spp)])
        for jitter in (False, True):
            u = _draws(be, _stratified(n, n, jitter, seed), SAMPLER_PIXEL, spp, [1, 1, 1])[:, :, 0]
            k = np.floor(P.f64(u) * spp).astype(np.int64)
            fig["perm_mismatch"] += sum(sorted(k[:, dim]) != list(range(spp)) for dim in range(3))
            fig["stratum_mismatch"] += int((k != want).sum())
            fig["range_mismatch"] += int(((u < 0) | (u >= 1)).sum())
            if not jitter:
                fig["centre_mismatch"] += int((u != ((want.astype(np.float32) + np.float32(0.5)) / np.float32(spp))).sum())
    return fig


def run_strata_2d(be, seed, grids):
    """Stratified get_2d at dimensions 0 and 2 of a fixed pixel over the spp sample indices: the multiset of cells floor(u (nx, ny))
    is the one the float64-free rule gives for strata 0 .. spp-1 — for nx = ny every cell exactly once."""
    fig = dict(cells_mismatch=0, beyond_unit=0)
    for nx, ny in grids:
        spp = nx * ny
        cx, cy = P.strata_cell(np.arange(spp), nx, ny)
        want = sorted(zip(cx.tolist(), cy.tolist()))
        if nx == ny and P._on("strata_row_divides_by_ny") and P._MUTATION is None:
            assert want == [(x, y) for x in range(nx) for y in range(ny)]
        for jitter in (False, True):
            u = P.f64(_draws(be, _stratified(nx, ny, jitter, seed), SAMPLER_PIXEL, spp, [2, 2]))
            for k in range(2):
                got = sorted(zip(np.floor(u[:, k, 0] * nx).astype(int).tolist(), np.floor(u[:, k, 1] * ny).astype(int).tolist()))
                fig["cells_mismatch"] += _multiset_difference(got, want)
            fig["beyond_unit"] += int((u >= 1).sum())
    return fig


PERMUTATION_GRID = (3, 3)
PERMUTATION_PIXELS = [(x, y) for y in (0, 40, 1033, 65534) for x in (0, 17, 1918, 65534)]


def run_permutations(be, seed):
    """Decorrelation: over 16 pixels, how many use different permutations at dimensions 0 and 1, and how many use a different
    one from their right-hand neighbour at dimension 0 — the counts Kensler's algorithm gives in Python integers (at least one each)."""
    from test_oracle_sampler import stratum_py

    spp = PERMUTATION_GRID[0] * PERMUTATION_GRID[1]
    s = _stratified(*PERMUTATION_GRID, False, seed)

    def device(px, py):
        u = _draws(be, s, (px, py), spp, [1, 1])[:, :, 0]
        return np.floor(P.f64(u) * spp).astype(int)

    def python(px, py):
        return np.array([[stratum_py(px, py, dim, seed, idx, spp) for dim in range(2)] for idx in range(spp)])

    counts = {}
    for name, perm in (("got", device), ("want", python)):
        dims = neighbours = 0
        for px, py in PERMUTATION_PIXELS:
            here, right = perm(px, py), perm(px + 1, py)
            dims += int((here[:, 0] != here[:, 1]).any())
            neighbours += int((here[:, 0] != right[:, 0]).any())
        counts[name] = (dims, neighbours)
    assert min(counts["want"]) >= 1, counts
    return dict(dims_count_mismatch=abs(counts["got"][0] - counts["want"][0]), neighbours_count_mismatch=abs(counts["got"][1] - counts["want"][1]),
                differing_dims=counts["got"][0], differing_neighbours=counts["got"][1])


SEEK_DRAWS, SEEK_TAIL, SEEK_INDEX = 32768, 8, 2


def run_uniform(be, seed):
    """The uniform sampler from ONE call of 32,768 + 8 two-dimensional draws at sample index 2: every value is k 2^-24 in [0,1); mean
    and variance of the first 4096 values lie within 4 standard errors of 1/2 and 1/12; and the last 8 draws are the first 8 of sample
    index 3, because the stream position is index * 65536 + dimension (the ledger's `uniform_streams_overlap`; switched off, the
    expectation is that no draw repeats)."""
    s = abi.SamplerDesc(abi.SAMPLER_UNIFORM, 16, 1, 1, seed)
    u = be.sampler_sequence(s, *SAMPLER_PIXEL, SEEK_INDEX, np.full(SEEK_DRAWS + SEEK_TAIL, 2, dtype=np.uint8))
    nxt = be.sampler_sequence(s, *SAMPLER_PIXEL, SEEK_INDEX + 1, np.full(SEEK_TAIL, 2, dtype=np.uint8))
    k = P.f64(u) * 2.0**24
    z_mean, z_var = P.uniform_moments_z(u[:2048])
    same = (u[SEEK_DRAWS:] == nxt).all(axis=1)
    return dict(grid_mismatch=int(((k != np.floor(k)) | (u < 0) | (u >= 1)).sum()), moments_mismatch=int(abs(z_mean) > Z_MAX) + int(abs(z_var) > Z_MAX),
                seek_mismatch=int((~same).sum() if P._on("uniform_streams_overlap") else same.sum()), z_mean=z_mean, z_var=z_var)


# ----------------------------------------------------------------------------- Whitted over a stack of panes
PANE_HALF = 50.0
PANE_THICK, PANE_GAP, FLOOR_GAP = 0.2, 0.02, 0.5
GLASSES = {
    "clear": dict(kind=abi.MAT_GLASS, a=(1, 1, 1), b=(1, 1, 1), c=1.5),
    "tinted": dict(kind=abi.MAT_GLASS, a=(0.9, 0.6, 0.3), b=(0.4, 0.7, 0.95), c=1.5),
}
PANE_FLOOR = dict(kind=abi.MAT_MATTE, a=(0.7, 0.5, 0.3), c=0.0)
PANE_LIGHT = dict(pos=(0.3, 0.25, -0.2), I=(2.0, 1.5, 1.0))  # between the lowest pane and the floor: shadow rays stop at glass
WHITTED_DEPTHS = (1, 2, 3, 8, 16)
WHITTED_ANGLES = (0.0, 40.0, 75.0, 89.0)
WHITTED_SEED, WHITTED_CALIBRATION = 7500, (9550, 9650)


def pane_heights(k, first=FLOOR_GAP):
    """[(y_bottom, y_top)] of k panes stacked over the floor, lowest first."""
    return [(first + j * (PANE_THICK + PANE_GAP), first + j * (PANE_THICK + PANE_GAP) + PANE_THICK) for j in range(k)]


def pane_scene(panes, glass, floor=None, lights=(), background=BACKGROUND, half=PANE_HALF):
    """Horizontal glass panes, each two quads with outward normals, over an optional matte floor at y = 0."""
    quads = [] if floor is None else [(0.0, True, 0)]
    for lo, hi in panes:
        quads += [(lo, False, 1), (hi, True, 1)]
    pts, idx, tri_mat = [], [], []
    for y, up, mat in quads:
        p, i = _quad(np.float32(y), half, up)
        idx.append(i + np.uint32(4 * len(pts)))
        pts.append(p)
        tri_mat += [mat, mat]
    n = len(quads)
    return scenes.SceneData(
        points=np.concatenate(pts), indices=np.concatenate(idx), tri_mesh=np.repeat(np.arange(n, dtype=np.uint32), 2), tri_material=np.asarray(tri_mat, dtype=np.int32),
        tri_area_light=np.full(2 * n, -1, dtype=np.int32), meshes=[(False, False, False)] * n, materials=[floor or PANE_FLOOR, glass], lights=list(lights),
        background=tuple(background), name="physics-panes",
    )


def _whitted(depth):
    return abi.IntegratorDesc(abi.INTEGRATOR_WHITTED, depth, 0, 0.0)


def _heading_rays(rng, angle_deg, n, y, spread=5.0):
    """n rays from height y going down at `angle_deg` to the vertical, at random headings from random places within +-spread."""
    a = np.radians(angle_deg)
    phi = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.sin(a) * np.cos(phi), np.full(n, -np.cos(a)), np.sin(a) * np.sin(phi)], axis=-1).astype(np.float32)
    o = np.stack([rng.uniform(-spread, spread, n), np.full(n, y), rng.uniform(-spread, spread, n)], axis=-1).astype(np.float32)
    return o, d


def _whitted_reference(panes, glass, depth, o, d, inside):
    """li and ray count of every ray by P.whitted_stack; the rays of one call share their angle to the vertical."""
    o64, d64 = P.f64(o), P.normalize(d)
    cos_start = float(np.mean(-d64[:, 1]))
    assert np.abs(-d64[:, 1] - cos_start).max() < 1e-6
    bg, floor, rays, reach = P.whitted_stack(panes, float(np.float32(glass["c"])), np.asarray(glass["a"], dtype=np.float32), np.asarray(glass["b"], dtype=np.float32),
                                             cos_start, float(o64[0, 1]), inside, depth)
    assert reach + np.abs(o64[:, [0, 2]]).max() < PANE_HALF - 1.0, reach  # no ray leaves the panes sideways
    li = np.broadcast_to(bg * P.f64(BACKGROUND), (len(o), 3)).copy()
    h = d64[:, [0, 2]]
    norm = np.linalg.norm(h, axis=1, keepdims=True)
    h = np.divide(h, norm, out=np.zeros_like(h), where=norm > 0)
    pm, _ = _translate(PANE_LIGHT["pos"])
    light = dict(kind=P.POINT, l2w=pm, I=PANE_LIGHT["I"])
    up = np.broadcast_to(UP, (len(o), 3))
    for w, s in floor:
        p = np.stack([o64[:, 0] + s * h[:, 0], np.zeros(len(o)), o64[:, 2] + s * h[:, 1]], axis=-1)
        r = P.light_sample(light, 0, p, up, np.zeros((len(o), 2)))
        li += w[None, :] * P.lambert_f(np.asarray(PANE_FLOOR["a"], dtype=np.float32))[None, :] * r["li"] * np.clip(r["l"] @ UP, 0.0, None)[:, None]
    return li, rays


def run_whitted(be, k, glass_name, depth, seed, tir=False):
    """Whitted::li over k panes, a matte floor and a point light under the lowest pane, against P.whitted_stack: li per ray
    (relative to the ray's brightest channel) and the number of closest-hit rays, exactly (where the back end reports one).
    64 rays per incidence, 0, 40, 75 and 89 degrees: 256 rays, four waves, over three panes; 16 per incidence, one wave, over one.
    `tir`: 64 rays that start inside the lowest pane at 60 degrees to the normal and are totally reflected at both faces: only the
    reflection child exists, li = 0 and max_depth rays are traced.  `tir` = an angle: 64 rays that start inside the lowest pane at
    that angle and leave it: the one place where a factor on transmission alone does not cancel between entering and leaving."""
    rng = np.random.default_rng(seed)
    glass = GLASSES[glass_name]
    panes = pane_heights(k)
    pm, _ = _translate(PANE_LIGHT["pos"])
    sd = pane_scene(panes, glass, PANE_FLOOR, [dict(kind="point", l2w=pm, I=PANE_LIGHT["I"])])
    if tir:
        groups = [_heading_rays(rng, 60.0 if tir is True else float(tir), 64, panes[0][0] + 0.5 * PANE_THICK)]
    else:
        groups = [_heading_rays(rng, a, 64 if k > 1 else 16, panes[-1][1] + 0.05) for a in WHITTED_ANGLES]
    o, d = np.concatenate([g[0] for g in groups]), np.concatenate([g[1] for g in groups])
    n = len(o)
    key = (be.name, "whitted", k, glass_name, depth, tir, seed)
    if key not in _ANSWERS:
        _ANSWERS[key] = be.li_counts(sd, _sampler(1), _whitted(depth), o, d, np.zeros((n, 2), np.uint16), np.zeros(n, np.uint32))
    got, counts = _ANSWERS[key]
    got = P.f64(got)
    ref, want = [], []
    for go, gd in groups:
        li, rays = _whitted_reference(panes, glass, depth, go, gd, bool(tir))
        ref.append(li)
        want.append(np.full(len(go), rays))
    ref, want = np.concatenate(ref), np.concatenate(want)
    out = {}
    if tir is True:
        out["li_abs"] = float(np.abs(got).max())
        assert not ref.any() and (want == depth).all()
    else:  # at max_depth 1 every ray ends on glass and li is 0: nothing to compare but the zeros
        nz_ref, nz_got = ref.max(axis=1) > 0, got.max(axis=1) > 0
        out["li_rel"] = _worst(_rgb_rel(got, ref), nz_ref & nz_got)
        out["li_zero_mismatch"] = int((nz_ref != nz_got).sum())
    if counts is not None:
        out["rays_mismatch"] = int((counts != want).sum())
    out["rays_per_sample"] = int(want.max())
    return out


# ----------------------------------------------------------------------------- deep paths: the roulette
RR_DEPTH, RR_N = 24, 65536
RR_ALBEDOS = {"warm": (0.8, 0.5, 0.3), "green": (0.5, 0.97, 0.2)}  # `green` reaches the 0.05 floor; `warm` is the ledger's case: green is not its largest
RR_MIN_EXPECTED = 20
SLAB_DEPTH, SLAB_N, SLAB_MIN_EXPECTED = 12, 65536, 30


def _count_z(observed, expected_p, n, min_expected):
    """Largest |z| of the classes whose expected count is at least min_expected, the others pooled into one class that is tested
    too; a pooled class of probability 0 that has members gives inf."""
    keys = sorted(set(observed) | set(expected_p))
    big = [k for k in keys if n * expected_p.get(k, 0.0) >= min_expected]
    rest_p = sum(expected_p.get(k, 0.0) for k in keys if k not in big)
    rest_obs = sum(observed.get(k, 0) for k in keys if k not in big)
    worst = 0.0
    for obs, p in [(observed.get(k, 0), expected_p[k]) for k in big] + [(rest_obs, rest_p)]:
        var = n * p * (1.0 - p)
        z = (obs - n * p) / np.sqrt(var) if var > 0 else (0.0 if obs == n * p else np.inf)
        worst = max(worst, abs(z))
    return float(worst)


def sphere_scene(material, center, radius, linear=np.eye(3), lights=(), background=(0, 0, 0)):
    """One sphere whose object-to-world transform is `linear` followed by a translation to `center`."""
    o2w = np.eye(4)
    o2w[:3, :3], o2w[:3, 3] = linear, center
    o2w = o2w.astype(np.float32)
    w2o = np.linalg.inv(o2w.astype(np.float64)).astype(np.float32)
    z = np.zeros(0, dtype=np.int32)
    return scenes.SceneData(
        points=np.zeros((0, 3), dtype=np.float32), indices=np.zeros((0, 3), dtype=np.uint32), tri_mesh=z.astype(np.uint32), tri_material=z, tri_area_light=z, meshes=[],
        materials=[material], lights=list(lights), spheres=[dict(o2w=o2w, w2o=w2o, radius=radius, material=0)], background=tuple(background), name="physics-sphere",
    )


def run_rr_lengths(be, albedo, seed):
    """Path lengths inside a closed Lambert sphere without a light: li is exactly 0, every ray count is one the roulette allows,
    and the counts follow P.rr_length_distribution (classes of expected count >= 20, the rest pooled) — `length_z`, a |z| held to
    Z_MAX like every statistical figure.  65,536 rays from one point in uniform directions, Uniform sampler, max_depth 24."""
    rng = np.random.default_rng(seed & 0xFFFF)
    rho = RR_ALBEDOS[albedo]
    sd = sphere_scene(dict(kind=abi.MAT_MATTE, a=rho, c=0.0), (1.0, -0.5, 0.7), 2.0)
    v = rng.normal(size=(RR_N, 3))
    d = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    o = np.broadcast_to(np.array([1.3, -0.2, 0.4], dtype=np.float32), d.shape).copy()
    key = (be.name, "rr", albedo, seed)
    if key not in _ANSWERS:
        pix = np.stack([np.arange(RR_N) % 256, np.arange(RR_N) // 256], axis=-1).astype(np.uint16)
        _ANSWERS[key] = be.li_counts(sd, _sampler(1, seed), _path(RR_DEPTH), o, d, pix, np.zeros(RR_N, np.uint32))
    li, counts = _ANSWERS[key]
    want = P.rr_length_distribution(rho, RR_DEPTH)
    vals, freq = np.unique(counts, return_counts=True)
    observed = dict(zip(vals.tolist(), freq.tolist()))
    return dict(li_abs=float(np.abs(li).max()), impossible_mismatch=int(sum(f for v, f in observed.items() if v not in want)),
                length_z=_count_z(observed, want, RR_N, RR_MIN_EXPECTED), longest=int(vals.max()))


def run_slab_classes(be, angle, seed):
    """Per-sample radiance of a path through one clear pane under a uniform background, no lights, max_depth 12: li / B of every
    sample is one of the finitely many values of P.slab_path_classes (`class_abs`: the distance to the nearest, worst channel),
    the classes' counts follow their probabilities (`class_z`; expected count >= 30, the rest pooled), and `class_gap` is the
    smallest distance between two members, which check_deterministic holds above 100 x the tolerance of class_abs."""
    sd = pane_scene([(-PANE_THICK, 0.0)], GLASSES["clear"], None)
    o, d = _ray_at(angle)
    key = (be.name, "slab", angle, seed)
    if key not in _ANSWERS:
        half = SLAB_N // 2  # two pixels x 32,768 sample indices: the samples per pixel are a u16 (integrators/mod.rs:139)
        pix = np.repeat(np.array([[3, 5], [4, 5]], dtype=np.uint16), half, axis=0)
        si = np.tile(np.arange(half, dtype=np.uint32), 2)
        _ANSWERS[key] = P.f64(be.li(sd, _sampler(half, seed), _path(SLAB_DEPTH), np.broadcast_to(o, (SLAB_N, 3)).copy(), np.broadcast_to(d, (SLAB_N, 3)).copy(), pix, si))
    x = _ANSWERS[key] / P.f64(BACKGROUND)[None, :]
    members = P.slab_path_classes(float(-P.normalize(d)[1]), 1.5, SLAB_DEPTH)
    values = np.array([m[0] for m in members])
    nearest = np.abs(x[:, :1] - values[None, :]).argmin(axis=1)
    vals, freq = np.unique(nearest, return_counts=True)
    return dict(class_abs=float(np.abs(x - values[nearest][:, None]).max()), class_z=_count_z(dict(zip(vals.tolist(), freq.tolist())), {k: m[1] for k, m in enumerate(members)}, SLAB_N, SLAB_MIN_EXPECTED),
                class_gap=float(np.diff(values).min()), classes=len(members), mean=float(x[:, 0].mean()))


CLAMP = 2.5


def run_clamp(be, seed):
    """`indirect_clamp` below the emitter's brightest channel, on run_emitter_through_pane's scene: every transmitted sample is
    P.clamped_emission(2, Le, c) exactly, the others black."""
    le = (3.0, 2.0, 1.0)
    m, mi = _translate((0.0, 2.0, 0.0))
    pane = dict(kind=abi.MAT_GLASS, a=(1, 1, 1), b=(1, 1, 1), c=1.0)
    sd = floor_scene(pane, [dict(kind="rect", l2w=m, l2w_inv=mi, L=le, size=(2.0, 2.0))], (0, 0, 0), emitter=(2.0, 1.0))
    o, d = _ray_at(10, from_below=True)
    n = 256
    integ = abi.IntegratorDesc(abi.INTEGRATOR_PATH, 3, 1, CLAMP)
    pix = np.broadcast_to(np.array([3, 5], dtype=np.uint16), (n, 2)).copy()
    got = P.f64(be.li(sd, _sampler(n, seed), integ, np.broadcast_to(o, (n, 3)).copy(), np.broadcast_to(d, (n, 3)).copy(), pix, np.arange(n, dtype=np.uint32)))
    lit = got.max(axis=1) > 0
    want = P.clamped_emission(2.0, le, CLAMP)
    return dict(emission_rel=_worst(_rgb_rel(got, np.broadcast_to(want, got.shape)), lit), lit_share_mismatch=int(not 0.3 < lit.mean() < 0.7))


# ----------------------------------------------------------------------------- the sphere's wo
def run_sphere_wo(be, seed):
    """Path::li at depth 1 on a Lambert sphere rotated 90 degrees about x under a point light, rays from outside: the ledger's
    `sphere_wo_transformed_again` — the lobe sees M wo, so a point is lit where (M wo).n and l.n have the same sign (and l.n > 0:
    the sphere shadows itself), with kd/pi I (n.l)/d^2 there.  Excluded: |(M wo).n| or |wo.n| or |l.n| below 1e-3, where f32 decides the side."""
    rng = np.random.default_rng(seed)
    n = 2000
    rot = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    c, radius, kd = np.array([0.5, 1.0, -0.25]), 1.0, (0.7, 0.5, 0.3)
    lp, inten = (3.0, 3.0, 1.0), (20.0, 15.0, 10.0)
    pm, _ = _translate(lp)
    sd = sphere_scene(dict(kind=abi.MAT_MATTE, a=kd, c=0.0), c, radius, rot, [dict(kind="point", l2w=pm, I=inten)])
    v = rng.normal(size=(n, 3))
    o = (c + 4.0 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    t = rng.normal(size=(n, 3))
    aim = c + 0.8 * radius * rng.uniform(0, 1, (n, 1)) ** (1 / 3) * t / np.linalg.norm(t, axis=1, keepdims=True)
    d = aim - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    got = P.f64(be.li(sd, _sampler(1), _path(1), o, d, np.zeros((n, 2), np.uint16), np.zeros(n, np.uint32)))
    o64, d64 = P.f64(o), P.normalize(d)
    oc = o64 - c
    b = P.dot(oc, d64)
    t_hit = -b - np.sqrt(b * b - (P.dot(oc, oc) - radius * radius))  # the nearer root: the rays start outside
    p = o64 + t_hit[:, None] * d64
    nrm = (p - c) / radius
    wo = -d64
    seen = wo @ rot.T if P._on("sphere_wo_transformed_again") else wo
    r = P.light_sample(dict(kind=P.POINT, l2w=pm, I=inten), 0, p, nrm, np.zeros((n, 2)))
    ln = P.dot(r["l"], nrm)
    lit = (ln > 0) & (P.dot(seen, nrm) > 0)
    ref = np.where(lit[:, None], P.lambert_f(np.asarray(kd, dtype=np.float32))[None, :] * r["li"] * np.clip(ln, 0.0, None)[:, None], 0.0)
    ex = (np.abs(P.dot(wo @ rot.T, nrm)) < 1e-3) | (np.abs(P.dot(wo, nrm)) < 1e-3) | (np.abs(ln) < 1e-3)
    nz_ref, nz_got = ref.max(axis=1) > 0, got.max(axis=1) > 0
    cmp_ = ~ex & nz_ref & nz_got
    return dict(li_rel=_worst(_rgb_rel(got, ref), cmp_), li_zero_mismatch=int(((nz_ref != nz_got) & ~ex).sum()), excluded=float(ex.mean()), compared=float(cmp_.mean()),
                dark_where_textbook_is_lit=float(((ln > 0) & ~lit & ~ex).mean()))


# ----------------------------------------------------------------------------- the surface stage
SURFACE_SEED, SURFACE_CALIBRATION = 7600, (9050, 9060, 9070)
SURFACE_CASES = ("plain", "uvs", "normals", "mixed-meshes", "degenerate", "sphere-rigid", "sphere-scaled", "sphere-mirrored", "sphere-inside", "sphere-poles")
EDGE_CUT, DISC_CUT, AXIS_SCALE = 1e-4, 1e-4, 0.05
SF = abi.SURFACE_FIELDS
ONE_TEXEL = np.full((1, 1, 3), 0.5, dtype=np.float32)  # any image texture makes both back ends compute a sphere's uv


def _unit(rng, k):
    v = rng.normal(size=(k, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _random_triangles(rng, k, spread=3.0):
    """k triangles with sides of about 1 to 3 and no angle below 20 degrees, anywhere within +-spread: (3k, 3) f32 points."""
    out = []
    while len(out) < k:
        c = rng.uniform(-spread, spread, 3)
        p = c + rng.normal(size=(3, 3)) * rng.uniform(0.6, 1.4)
        e = [p[(i + 1) % 3] - p[i] for i in range(3)]
        cos = [np.dot(-e[i - 1], e[i]) / (np.linalg.norm(e[i - 1]) * np.linalg.norm(e[i])) for i in range(3)]
        if max(cos) <= np.cos(np.radians(20.0)):
            out.append(p)
    return np.concatenate(out).astype(np.float32)


def _random_uvs(rng, pts, mirrored):
    """Per-vertex uvs in [-2.3, 3.1] with |uv_det| >= 0.05 |duv02| |duv12|; triangle k's winding is mirrored (uv_det < 0) where mirrored[k]."""
    k = len(pts) // 3
    uv = np.zeros((3 * k, 2), dtype=np.float32)
    for t in range(k):
        while True:
            q = rng.uniform(-2.3, 3.1, (3, 2)).astype(np.float32).astype(np.float64)
            a, b = q[0] - q[2], q[1] - q[2]
            det = a[0] * b[1] - a[1] * b[0]
            if abs(det) >= 0.05 * np.linalg.norm(a) * np.linalg.norm(b) and (det < 0) == bool(mirrored[t]):
                uv[3 * t : 3 * t + 3] = q
                break
    return uv


def _tilted_normals(rng, pts, far_side):
    """Per-vertex normals up to 40 degrees from the face normal normalize((p0 - p2) x (p1 - p2)), lengths 0.3 .. 3; on the far side
    of it where far_side[k]."""
    p = pts.astype(np.float64).reshape(-1, 3, 3)
    face = np.cross(p[:, 0] - p[:, 2], p[:, 1] - p[:, 2])
    face /= np.linalg.norm(face, axis=1, keepdims=True)
    face = np.where(np.asarray(far_side, dtype=bool)[:, None], -face, face)
    out = np.zeros((len(p), 3, 3))
    for v in range(3):
        side = np.cross(face, _unit(rng, len(p)))
        side /= np.linalg.norm(side, axis=1, keepdims=True)
        a = np.radians(rng.uniform(0.0, 40.0, (len(p), 1)))
        out[:, v] = (np.cos(a) * face + np.sin(a) * side) * rng.uniform(0.3, 3.0, (len(p), 1))
    return out.reshape(-1, 3).astype(np.float32)


LAMBERT = dict(kind=abi.MAT_MATTE, a=(0.7, 0.5, 0.3), c=0.0)


def _mesh_scene(pts, meshes, tri_mesh, normals=None, uvs=None, tri_material=None, tri_area_light=None, materials=None, lights=(), order=None, name="physics-surface"):
    k = len(pts) // 3
    return scenes.SceneData(
        points=pts, indices=np.arange(3 * k, dtype=np.uint32).reshape(k, 3), tri_mesh=np.asarray(tri_mesh, dtype=np.uint32),
        tri_material=np.zeros(k, dtype=np.int32) if tri_material is None else np.asarray(tri_material, dtype=np.int32),
        tri_area_light=np.full(k, -1, dtype=np.int32) if tri_area_light is None else np.asarray(tri_area_light, dtype=np.int32), meshes=list(meshes),
        materials=[LAMBERT] if materials is None else materials, lights=list(lights), normals=normals, uvs=uvs, max_shapes_in_node=2, shape_order=order, name=name,
    )


def _aimed_rays(rng, targets, n=N_STAGE, reach=(1.0, 6.0)):
    """n rays towards random members of `targets` (points on the primitives) from random directions, i.e. from both sides, from
    origins at most 10 from the world's origin."""
    hit = targets[rng.integers(0, len(targets), n)]
    o = hit + _unit(rng, n) * rng.uniform(reach[0], reach[1], (n, 1))
    o *= np.minimum(1.0, 9.9 / np.linalg.norm(o, axis=1, keepdims=True))
    o = o.astype(np.float32)
    d = hit - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _points_on(rng, pts, per=64):
    p = pts.astype(np.float64).reshape(-1, 3, 3)
    w = rng.dirichlet((1.0, 1.0, 1.0), (len(p), per))
    return np.einsum("kjv,kvc->kjc", w, p).reshape(-1, 3)


SPHERE_SCALE = (1.0, 0.5, 2.0)


def _sphere_transform(rng, kind):
    """object_to_world of the sphere cases: rotation and translation; then with scale (1, 0.5, 2); then with a reflection besides.
    `poles`: a quarter turn, the same scale and a translation in eighths, so that the object z-axis is reached exactly in f32."""
    if kind == "poles":
        rot = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
        lin, c = rot @ np.diag(SPHERE_SCALE), np.round(rng.uniform(-2, 2, 3) * 8) / 8
    else:
        rot = _rigid(rng)[0][:3, :3].astype(np.float64)
        c = rng.uniform(-2, 2, 3)
        lin = rot if kind == "rigid" else rot @ np.diag(SPHERE_SCALE)
        if kind == "mirrored":
            lin = lin @ np.diag([1.0, -1.0, 1.0])
    return lin, c


def surface_inputs(name, seed):
    """(SceneData, ray origins, ray directions) of one surface case; everything follows from the seed."""
    rng = np.random.default_rng([seed, SURFACE_CASES.index(name)])
    if name.startswith("sphere-"):
        kind = name.split("-")[1]
        lin, c = _sphere_transform(rng, {"inside": "scaled"}.get(kind, kind))
        radius = 1.5
        sd = sphere_scene(dict(LAMBERT, tex=0), c, radius, lin)
        sd.textures = [ONE_TEXEL]
        n = N_STAGE
        if kind == "poles":
            sign = rng.choice([-1.0, 1.0], (n, 1))
            tilt = np.radians(rng.uniform(0, 1e-3 * 180 / np.pi, (n, 1)))
            tilt[:64] = 0.0
            phi = rng.uniform(0, 2 * np.pi, (n, 1))
            axis_dir = np.concatenate([np.sin(tilt) * np.cos(phi), np.sin(tilt) * np.sin(phi), np.cos(tilt)], axis=1) * sign
            dist = np.where(np.arange(n)[:, None] < 64, 8.0 * rng.integers(1, 4, (n, 1)), rng.uniform(4.0, 8.0, (n, 1)))
            o = (c + (axis_dir * dist) @ lin.T).astype(np.float32)  # object space: on the axis, scaled by dist
            d = -(axis_dir @ lin.T)
            d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
            return sd, o, d
        target = c + (_unit(rng, n) * radius * rng.uniform(0, 1, (n, 1)) ** (1 / 3) * 0.98) @ lin.T
        if kind == "inside":
            o = (c + (_unit(rng, n) * radius * 0.9 * rng.uniform(0, 1, (n, 1)) ** (1 / 3)) @ lin.T).astype(np.float32)
            d = _unit(rng, n).astype(np.float32)
            return sd, o, d
        o = target + _unit(rng, n) * rng.uniform(4.5, 7.5, (n, 1))
        o = o.astype(np.float32)
        d = target - o
        return sd, o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    if name == "degenerate":
        # eighths, so that every difference of coordinates is exact in f32.  Mesh 0: uvs whose three values are equal (and swaps_handedness
        # without normals, the one place where a triangle's flag decides the side of n); mesh 1: flagged
        # as having normals, all zero; mesh 2: a triangle in the xy-plane with p1 - p0 along x and no uvs, so dpdu = p1 - p0 = (2, 0, 0),
        # whose vertex normals are that very vector
        pts = (np.round(_random_triangles(rng, 16).astype(np.float64) * 8) / 8).astype(np.float32)
        z = float(np.round(rng.uniform(-3, 3) * 8) / 8)
        x, y = (float(v) for v in np.round(rng.uniform(-2, 2, 2) * 8) / 8)
        pts = np.concatenate([pts, np.array([(x, y, z), (x + 2, y, z), (x + 0.5, y + 1.5, z)], dtype=np.float32)])
        k = 17
        tri_mesh = [0] * 8 + [1] * 8 + [2]
        uvs = np.repeat(rng.uniform(-2.3, 3.1, (k, 2)), 3, axis=0).astype(np.float32)
        normals = np.zeros((3 * k, 3), dtype=np.float32)
        normals[48:51] = (2.0, 0.0, 0.0)
        sd = _mesh_scene(pts, [(False, True, True), (True, False, False), (True, False, False)], tri_mesh, normals=normals, uvs=uvs, order=rng.permutation(k).astype(np.uint32))
        targets = np.concatenate([_points_on(rng, pts[:48]), np.repeat(_points_on(rng, pts[48:]), 12, axis=0)])
        o, d = _aimed_rays(rng, targets)
        return sd, o, d
    if name == "mixed-meshes":
        k = 64
        pts = _random_triangles(rng, k)
        tri_mesh = np.repeat(np.arange(4), 16)
        meshes = [(False, False, False), (False, True, False), (True, True, False), (True, True, True)]
        uvs = _random_uvs(rng, pts, rng.integers(0, 2, k))
        normals = _tilted_normals(rng, pts, rng.integers(0, 4, k) == 0)
        materials = [dict(kind=abi.MAT_MATTE, a=(0.2 + 0.01 * m, 0.5, 0.3), c=0.0) for m in range(70)]
        tri_material = rng.permutation(70)[:k]
        tri_material[:3] = (69, 64, 63)
        tri_al = np.full(k, -1)
        lit = rng.choice(k, 2, replace=False)
        tri_al[lit] = (0, 1)
        lm, lmi = _translate((0.0, 6.0, 0.0))
        lights = [dict(kind="rect", l2w=lm, l2w_inv=lmi, L=(1.0, 1.0, 1.0), size=(1.0, 1.0))] * 2
        perm = rng.permutation(k)  # the meshes' triangles interleave in source order
        idx = np.arange(3 * k).reshape(k, 3)[perm]
        sd = _mesh_scene(pts, meshes, tri_mesh[perm], normals=normals, uvs=uvs, tri_material=tri_material[perm], tri_area_light=tri_al[perm], materials=materials,
                         lights=lights, order=rng.permutation(k).astype(np.uint32))
        sd.indices = idx.astype(np.uint32)
        o, d = _aimed_rays(rng, _points_on(rng, pts))
        return sd, o, d
    k = 64
    pts = _random_triangles(rng, k)
    uvs = _random_uvs(rng, pts, np.arange(k) % 2) if name == "uvs" else None
    normals = _tilted_normals(rng, pts, np.arange(k) % 4 == 0) if name == "normals" else None
    sd = _mesh_scene(pts, [(name == "normals", name == "uvs", False)], np.zeros(k), normals=normals, uvs=uvs, order=rng.permutation(k).astype(np.uint32))
    o, d = _aimed_rays(rng, _points_on(rng, pts))
    return sd, o, d


def scene_arrays(sd, points=None, normals=None):
    """The f32 arrays of a SceneData as tests/physics_ref.py's surface functions take them."""
    flags = np.asarray(sd.meshes, dtype=bool).reshape(-1, 3)[np.asarray(sd.tri_mesh, dtype=np.int64)] if len(sd.indices) else np.zeros((0, 3), dtype=bool)
    return dict(points=sd.points if points is None else points, indices=sd.indices, tri_flags=flags, normals=sd.normals if normals is None else normals, uvs=sd.uvs,
                spheres=[(s["o2w"], s["w2o"], s["radius"]) for s in sd.spheres])


def surface_reference(sd, o, d, points=None, normals=None):
    """P.surface plus what the scene description itself says of the hit shape: material and area light."""
    r = P.surface(scene_arrays(sd, points, normals), o, d)
    nt = sd.n_triangles
    shape = r["shape"]
    tri = np.clip(shape, 0, max(nt - 1, 0))
    mat = np.asarray(sd.tri_material, dtype=np.int64)[tri] if nt else np.zeros(len(shape), dtype=np.int64)
    al = np.asarray(sd.tri_area_light, dtype=np.int64)[tri] if nt else np.full(len(shape), -1)
    for k, s in enumerate(sd.spheres):
        mat = np.where(shape == nt + k, int(s["material"]), mat)
        al = np.where(shape == nt + k, -1, al)
    r["material"], r["area_light"] = np.where(r["hit"], mat, 0), np.where(r["hit"], al, 0)
    return r


def surface_excluded(r, d):
    """Rows left out, by the float64 reference alone: grazing rays, hits at a triangle's edge, rays that graze a sphere, and shading
    normals in the plane of their triangle (where f32 decides the side of n) unless the case is about that very branch."""
    d = P.f64(d)
    graze = np.abs(P.dot(d, r["face"])) < COS_CUT
    edge = ~r["is_sphere"] & (r["edge"] < EDGE_CUT)
    disc = r["is_sphere"] & (r["disc"] < DISC_CUT)
    flat = ~r["tangent_along_ns"] & (np.abs(P.dot(r["ns"], r["face"])) < COS_CUT * np.linalg.norm(r["ns"], axis=1))
    return r["hit"] & (graze | edge | disc | flat)


def score_surface(sd, o, d, got, points=None, normals=None):
    """One yk_surface / orc_surface answer against the float64 surface.

    Conditioning factors (reference only), on sphere rows.  Pole: a sphere's u and tangent turn by 1 / sin theta per unit of
    rounding in the object-space point, and v by the same through the arc cosine, so their errors are multiplied by
    min(1, sin theta / 0.05), the factor tests/test_gpu_li_debug.py::test_shading_uvs_on_spheres divides its tolerance by; so are
    those of n and ns, because Sphere::intersect forms the normal as dpdu x dpdv with dpdv.z = -r sin(acos(z / r)) (sphere.rs:88-104,
    as pbrt-v3 §3.2.3 does), which carries the same arc cosine: unscaled, n is off by 1.4e-3 at 1e-3 rad from a pole.  Grazing: the
    hit distance solves a quadratic whose root moves by 1 / sqrt(disc / b^2) per unit of rounding in the ray, and with it the point and
    all that is read off it, so every position-dependent error of a sphere row is multiplied by sqrt(disc / b^2) (<= 1; rows below
    1e-4 are excluded outright).  u is compared around the seam.
    On every row t's relative error is multiplied by min(1, t / max(1, |p|, |o|)): a hit distance carries the rounding of the coordinates
    it is a difference of, so a ray that starts next to a surface has an absolute error of that size in however short a t.
    The tangent is compared as a unit vector: a mesh without normals and a sphere report dpdu itself, the BSDF frame normalises it.
    Rows whose tangent the geometry leaves open (equal uvs; dpdu along ns) are held to what holds in any frame instead: s.ns = 0 and,
    with vertex normals, |s| = 1 — for every triangle row; a vanished interpolated normal must give ns = n (`ns_n_abs`: the frame is
    rebuilt from s x t, so to rounding)."""
    r = surface_reference(sd, o, d, points, normals)
    got = P.f64(got)
    ex = surface_excluded(r, d)
    keep = r["hit"] & ~ex
    hit_got = got[:, SF["hit"]] != 0
    both = keep & hit_got
    out = dict(hit_mismatch=int(((hit_got != r["hit"]) & ~ex).sum()), shape_mismatch=int(((got[:, SF["shape"]] != r["shape"]) & ~ex).sum()))
    both &= got[:, SF["shape"]] == r["shape"]
    out["material_mismatch"] = int((got[both, SF["material"]] != r["material"][both]).sum())
    out["light_mismatch"] = int((got[both, SF["area_light"]] != r["area_light"][both]).sum())
    out["side_mismatch"] = int((P.dot(got[:, SF["n"]], r["n"]) <= 0)[both].sum())
    out["nan_mismatch"] = int((~np.isfinite(got)).any(axis=1).sum())
    scale = np.maximum(1.0, np.maximum(np.linalg.norm(r["p"], axis=1), np.linalg.norm(P.f64(o), axis=1)))
    graze = np.where(r["is_sphere"], np.sqrt(np.clip(r["disc"], 0.0, 1.0)), 1.0)
    cond = np.minimum(1.0, r["axis"] / AXIS_SCALE) * graze
    out["t_rel"] = _worst(_rel(got[:, SF["t"]], r["t"]) * graze * np.minimum(1.0, r["t"] / scale), both)
    out["p_pos"] = _worst(_vec_abs(got[:, SF["p"]], r["p"]) / scale * graze, both)
    out["origin_pos"] = _worst(_vec_abs(got[:, SF["origin"]], r["origin"]) / scale * graze, both)
    out["n_abs"] = _worst(_vec_abs(got[:, SF["n"]], r["n"]) * cond, both)
    out["ns_abs"] = _worst(_vec_abs(got[:, SF["ns"]], r["ns"]) * cond, both)
    out["ns_n_abs"] = _worst(_vec_abs(got[:, SF["ns"]], got[:, SF["n"]]), both & r["ns_zero"])
    out["wo_abs"] = _worst(_vec_abs(got[:, SF["wo"]], r["wo"]), both)
    s_got = got[:, SF["dpdus"]]
    with np.errstate(all="ignore"):
        s_unit = s_got / np.linalg.norm(s_got, axis=1, keepdims=True)
    open_frame = r["uv_degenerate"] | r["tangent_along_ns"] | r["ns_zero"]
    out["s_abs"] = _worst(_vec_abs(s_unit, r["s"]) * cond, both & ~open_frame)
    tri = both & ~r["is_sphere"]
    out["s_perp_abs"] = _worst(np.abs(P.dot(s_unit, got[:, SF["ns"]])), tri)
    out["s_unit_abs"] = _worst(np.abs(np.linalg.norm(s_got, axis=1) - 1.0), tri & r["has_normals"])
    uv_got = np.stack([got[:, SF["u"]], got[:, SF["v"]]], axis=-1)
    duv = np.abs(uv_got - r["uv"])
    duv[:, 0] = np.where(r["is_sphere"], np.minimum(duv[:, 0], 1.0 - duv[:, 0]), duv[:, 0])
    out["uv_abs"] = _worst(np.linalg.norm(duv, axis=1) * cond / np.maximum(1.0, np.linalg.norm(r["uv"], axis=1)), both)
    out["excluded"] = float(ex.mean())
    out["compared"] = float(both.mean())
    back = P.dot(P.f64(d), r["face"]) > 0
    flags = np.asarray(scene_arrays(sd)["tri_flags"], dtype=bool)
    tri_of = np.clip(r["shape"], 0, max(sd.n_triangles - 1, 0))
    is_tri = both & ~r["is_sphere"]
    uv3 = None if sd.uvs is None else P.f64(sd.uvs)[np.asarray(sd.indices, dtype=np.int64)[tri_of]] if sd.n_triangles else None
    out.update(
        back_rows=int((both & back).sum()), sphere_rows=int((both & r["is_sphere"]).sum()), inside_rows=int((both & r["inside"]).sum()),
        nudge_rows=int((both & r["is_sphere"] & (r["axis"] == 0)).sum()), near_pole_rows=int((both & r["is_sphere"] & (r["axis"] < AXIS_SCALE)).sum()),
        uv_degenerate_rows=int((both & r["uv_degenerate"]).sum()), ns_zero_rows=int((both & r["ns_zero"]).sum()), tangent_along_ns_rows=int((both & r["tangent_along_ns"]).sum()),
        flipped_rows=int((is_tri & (P.dot(r["n"], r["face"]) < 0)).sum()), normals_rows=int((is_tri & r["has_normals"]).sum()),
        light_rows=int((both & (r["area_light"] >= 0)).sum()), material_high_rows=int((both & (r["material"] >= 64)).sum()),
        swaps_rows=int((is_tri & flags[tri_of, 2]).sum()) if sd.n_triangles else 0,
        default_uv_rows=int((is_tri & ~flags[tri_of, 1]).sum()) if sd.n_triangles else 0,
        uv_mirrored_rows=0 if uv3 is None else int((is_tri & flags[tri_of, 1] & (np.linalg.det(np.stack([uv3[:, 0] - uv3[:, 2], uv3[:, 1] - uv3[:, 2]], axis=1)) < 0)).sum()),
    )
    return out


SURFACE_BRANCH = {  # the rows each case was built for: every named count must be > 0 (tests/test_physics.py)
    "plain": ("back_rows", "default_uv_rows"), "uvs": ("uv_mirrored_rows", "back_rows"), "normals": ("flipped_rows", "normals_rows"),
    "mixed-meshes": ("light_rows", "material_high_rows", "swaps_rows", "default_uv_rows", "normals_rows", "uv_mirrored_rows"),
    "degenerate": ("uv_degenerate_rows", "ns_zero_rows", "tangent_along_ns_rows", "swaps_rows"), "sphere-rigid": ("sphere_rows",), "sphere-scaled": ("sphere_rows",),
    "sphere-mirrored": ("sphere_rows",), "sphere-inside": ("inside_rows",), "sphere-poles": ("nudge_rows", "near_pole_rows"),
}


def surface_stage_cases():
    """The cases that pin the surface stage and the estimator above it."""
    return [c for c in deterministic_cases() if c.startswith(("surface/", "direct-smooth/", "direct-textured/"))]


def excluded_share(case_id, seed):
    """The share of a case's batch that the float64 predicates leave out, with no back end at all."""
    return run_case(NullBackend(), case_id, seed, cache=False)["excluded"]


def run_surface(be, name, seed, route=0, cache=True):
    sd, o, d = surface_inputs(name, seed)
    key = (be.name, "surface", name, seed, route)
    if not cache or key not in _ANSWERS:
        _ANSWERS[key] = be.surface(sd, o, d, route)
    return score_surface(sd, o, d, _ANSWERS[key])


# ----------------------------------------------------------------------------- the surface under the estimator
TEXTURE_SIZES = ((7, 5), (1, 1), (16, 3))  # width x height
TEXEL_CUT = 1e-4  # texels: far wider than the uv_abs tolerance times 16 texels
POINT_LIGHT = dict(pos=(1.0, 3.0, -0.5), I=(20.0, 15.0, 10.0))


@functools.lru_cache(maxsize=None)
def texture_pattern(w, h):
    """A w x h PNG, written by scene_files.write_png and read back by the product's ImageTexture::new: (h, w, 3) f32 texels, pixel / 255.
    Horizontally and vertically adjacent texels differ by at least 26 / 255 > 0.1 in red."""
    import tempfile

    import scene_files
    from yuki_amd import loaders

    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([40 + 26 * ((x + 3 * y) % 7), 230 - 26 * ((2 * x + y) % 5), 70 + 13 * ((x + y) % 3)], axis=-1).astype(np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, f"pattern-{w}x{h}.png")
        scene_files.write_png(path, img)
        tex = loaders.load_image_texture(path)
    assert tex.shape == (h, w, 3) and np.array_equal(tex, img.astype(np.float32) / np.float32(255))
    return tex


def _point_light():
    pm, _ = _translate(POINT_LIGHT["pos"])
    return dict(kind="point", l2w=pm, I=POINT_LIGHT["I"]), dict(kind=P.POINT, l2w=pm, I=POINT_LIGHT["I"])


def _lambert_direct(be, sd, o, d, kd, lit_rule, ex):
    """Path::li at depth 1 under the point light against kd / pi * I * clamp(ns.l) / d^2 where `lit_rule(r, light sample)` holds, 0
    elsewhere; r is the float64 surface of the scene."""
    n = len(o)
    got = P.f64(be.li(sd, _sampler(1), _path(1), o, d, np.zeros((n, 2), np.uint16), np.zeros(n, np.uint32)))
    r = surface_reference(sd, o, d)
    ls = P.light_sample(_point_light()[1], 0, r["p"], r["n"], np.zeros((n, 2)))
    lit = r["hit"] & lit_rule(r, ls)
    ref = np.where(lit[:, None], kd(r) / np.pi * ls["li"] * np.clip(P.dot(r["ns"], ls["l"]), 0.0, 1.0)[:, None], 0.0)
    ex = ex(r, ls) | surface_excluded(r, d)
    nz_ref, nz_got = ref.max(axis=1) > 0, got.max(axis=1) > 0
    cmp_ = ~ex & nz_ref & nz_got
    # measured against the value without its cosine, whose relative error is unbounded at the terminator; a sphere row times its
    # grazing factor (score_surface)
    full = (kd(r) / np.pi * ls["li"]).max(axis=1)
    graze = np.where(r["is_sphere"], np.sqrt(np.clip(r["disc"], 0.0, 1.0)), 1.0)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref).max(axis=1) / full * graze
    return dict(li_rel=_worst(err, cmp_), li_zero_mismatch=int(((nz_ref != nz_got) & ~ex).sum()), excluded=float(ex.mean()), compared=float(cmp_.mean()),
                dark_rows=int((~nz_ref & ~ex).sum()))


def _merge(scores):
    out = {}
    for sc in scores:
        for k, v in sc.items():
            out[k] = v + out.get(k, 0) if k.endswith(("_mismatch", "_rows")) else max(v, out.get(k, 0.0)) if k != "compared" else min(v, out.get(k, 1.0))
    return out


def _same_side(r, ls):
    """BSDF::f's filter (pbrt-v3 §9.1): reflection counts where wo and wi lie on one side of the GEOMETRIC normal."""
    return P.dot(r["wo"], r["n"]) * P.dot(ls["l"], r["n"]) > 0


def _side_band(r, ls):
    return (np.abs(P.dot(r["wo"], r["n"])) < 1e-3) | (np.abs(P.dot(ls["l"], r["n"])) < 1e-3) | (np.abs(P.dot(ls["l"], r["ns"])) < 1e-3)


def run_direct_textured(be, which, seed):
    """A matte surface whose kd is an image texture, at depth 1 under a point light: kd is the texel the float64 uv selects (repeat,
    v flipped, point sampled, the ledger's index rule).  `quad`: the floor with vertex uvs in [-2.3, 3.1], once per texture of 7 x 5,
    1 x 1 and 16 x 3 texels (PNG files, decoded by the product's loader).  `sphere`: the scaled sphere with the 7 x 5.
    Excluded: a float64 uv within 1e-4 texel of a texel boundary; on the sphere also u within 1e-4 of the seam, sin theta < 0.05 and
    the side bands of sphere-wo/rotated."""
    rng = np.random.default_rng(seed)
    sl, _ = _point_light()
    scores = []
    if which == "quad":
        pts, idx = _quad(0.0, FLOOR_HALF, True)
        uvs = np.array([(-2.3, -2.3), (3.1, -2.3), (3.1, 3.1), (-2.3, 3.1)], dtype=np.float32)
        for w, h in TEXTURE_SIZES:
            tex = texture_pattern(w, h)
            sd = scenes.SceneData(points=pts, indices=idx, tri_mesh=np.zeros(2, np.uint32), tri_material=np.zeros(2, np.int32), tri_area_light=np.full(2, -1, np.int32),
                                  meshes=[(False, True, False)], materials=[dict(LAMBERT, tex=0)], lights=[sl], uvs=uvs, textures=[tex], name="physics-textured-quad")
            o, d = direct_rays(int(rng.integers(1 << 30)))
            look = lambda r, tex=tex: P.texel_lookup(tex, r["uv"])
            scores.append(_lambert_direct(be, sd, o, d, lambda r: look(r)[0], _same_side, lambda r, ls: look(r)[1] < TEXEL_CUT))
        return _merge(scores)
    tex = texture_pattern(7, 5)
    lin, c = _sphere_transform(rng, "scaled")
    c = c * 0.25 + np.array([0.0, -2.0, 0.0])  # some 5 from the light: nearly half of the sphere is lit
    sd = sphere_scene(dict(LAMBERT, tex=0), c, 1.0, lin, [sl])
    sd.textures = [tex]
    n = 8 * 2000  # candidates; the ledger's sphere_wo_transformed_again leaves a fifth of the lit side visible to the lobe, so the
    o = (c + 4.0 * _unit(rng, n)).astype(np.float32)  # batch is drawn from them by the float64 prediction alone: 1000 lit rows, 1000 dark
    aim = c + (0.8 * rng.uniform(0, 1, (n, 1)) ** (1 / 3) * _unit(rng, n)) @ lin.T
    d = aim - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    r = surface_reference(sd, o, d)
    ls = P.light_sample(_point_light()[1], 0, r["p"], r["n"], np.zeros((n, 2)))
    lit = r["hit"] & _same_side(r, ls) & (P.dot(r["ns"], ls["l"]) > 0)
    rows = np.sort(np.concatenate([np.nonzero(lit)[0][:1000], np.nonzero(~lit)[0][:1000]]))
    o, d = o[rows], d[rows]
    look = lambda r: P.texel_lookup(tex, r["uv"])
    ex = lambda r, ls: (look(r)[1] < TEXEL_CUT) | (np.minimum(r["uv"][:, 0], 1.0 - r["uv"][:, 0]) < 1e-4) | (r["axis"] < AXIS_SCALE) | _side_band(r, ls)
    return _lambert_direct(be, sd, o, d, lambda r: look(r)[0], _same_side, ex)


SMOOTH_TILT = 35.0


def run_direct_smooth(be, which, seed):
    """A Lambert quad pair with tilted vertex normals under the point light at depth 1: kd / pi * I * clamp(ns.l) / d^2 where wo and l
    are on one side of the geometric normal, 0 elsewhere.  Half of the quad (one triangle) carries normals on the far side of its face
    normal, so its n is flipped to them.  `up`: seen from above; `both`: rays from either side."""
    rng = np.random.default_rng(seed)
    sl, _ = _point_light()
    pts, idx = _quad(0.0, FLOOR_HALF, True)
    pts = np.concatenate([pts[idx[0]], pts[idx[1]]])  # two triangles with vertices of their own
    a = np.radians(rng.uniform(5.0, SMOOTH_TILT, (6, 1)))
    side = np.cross(UP, _unit(rng, 6))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    normals = (np.cos(a) * UP + np.sin(a) * side) * rng.uniform(0.3, 3.0, (6, 1))
    normals[3:] *= -1.0
    sd = _mesh_scene(pts.astype(np.float32), [(True, False, False)], [0, 0], normals=normals.astype(np.float32), lights=[sl], name="physics-smooth-quad")
    o, d = direct_rays(int(rng.integers(1 << 30)))
    if which == "both":
        o[::2, 1] *= -1.0
        d[::2, 1] *= -1.0
    kd = P.f64(np.asarray(LAMBERT["a"], dtype=np.float32))
    return _lambert_direct(be, sd, o, d, lambda r: kd[None, :], _same_side, _side_band)


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
    for name in camera_specs():
        out[name] = ("camera", (name,), CAMERA_SEED, CAMERA_CALIBRATION)
    out["camera-jitter/link"] = ("camera-jitter", (), CAMERA_SEED, CAMERA_CALIBRATION)
    for name in SAMPLER_CASES:  # structure only: no toleranced figure, hence nothing to calibrate
        out[name] = ("sampler", (name,), SAMPLER_SEED, ())
    for k in (1, 3):
        for glass in GLASSES:
            for depth in WHITTED_DEPTHS:
                out[f"whitted/{k}-{glass}/d{depth}"] = ("whitted", (k, glass, depth, False), WHITTED_SEED, WHITTED_CALIBRATION)
    for glass, depth in (("clear", 1), ("clear", 16), ("tinted", 3), ("tinted", 16)):
        out[f"whitted-tir/{glass}/d{depth}"] = ("whitted", (1, glass, depth, True), WHITTED_SEED, WHITTED_CALIBRATION)
    for glass in GLASSES:
        out[f"whitted-from-inside/{glass}/d8"] = ("whitted", (3, glass, 8, 20.0), WHITTED_SEED, WHITTED_CALIBRATION)
    for albedo in RR_ALBEDOS:
        out[f"rr-lengths/{albedo}"] = ("rr-lengths", (albedo,), MC_SEED, (MC_SEED + 1, MC_SEED + 2))
    for angle in (40, 75):
        out[f"slab-classes/{angle}"] = ("slab-classes", (angle,), MC_SEED, (MC_SEED + 1, MC_SEED + 2))
    out["clamp/emitter-through-pane"] = ("clamp", (), MC_SEED, (MC_SEED + 1, MC_SEED + 2))
    out["sphere-wo/rotated"] = ("sphere-wo", (), LI_SEED, LI_CALIBRATION)
    for name in SURFACE_CASES:
        out[f"surface/{name}"] = ("surface", (name,), SURFACE_SEED, SURFACE_CALIBRATION)
    for which in ("up", "both"):
        out[f"direct-smooth/{which}"] = ("direct-smooth", (which,), SURFACE_SEED, SURFACE_CALIBRATION)
    for which in ("quad", "sphere"):
        out[f"direct-textured/{which}"] = ("direct-textured", (which,), SURFACE_SEED, SURFACE_CALIBRATION)
    return out


SAMPLER_CASES = {
    "sampler/strata-1d": run_strata_1d,
    "sampler/strata-2d-square": lambda be, seed: run_strata_2d(be, seed, SQUARE_GRIDS),
    "sampler/strata-2d-rect": lambda be, seed: run_strata_2d(be, seed, RECT_GRIDS),
    "sampler/permutations": run_permutations,
    "sampler/uniform": run_uniform,
}


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
    if kind == "camera":
        return run_camera(be, args[0], seed)
    if kind == "camera-jitter":
        return run_camera_jitter(be, seed)
    if kind == "sampler":
        return SAMPLER_CASES[args[0]](be, seed)
    if kind == "whitted":
        return run_whitted(be, args[0], args[1], args[2], seed, tir=args[3])
    if kind == "rr-lengths":
        return run_rr_lengths(be, args[0], seed)
    if kind == "slab-classes":
        return run_slab_classes(be, args[0], seed)
    if kind == "clamp":
        return run_clamp(be, seed)
    if kind == "sphere-wo":
        return run_sphere_wo(be, seed)
    if kind == "surface":
        return run_surface(be, args[0], seed, cache=cache)
    if kind == "direct-smooth":
        return run_direct_smooth(be, args[0], seed)
    if kind == "direct-textured":
        return run_direct_textured(be, args[0], seed)
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
        elif k.endswith("_z"):
            if not v <= Z_MAX:
                bad.append(f"{case_id}:{k} = {v:.2f} > {Z_MAX}")
    if "class_gap" in score and not score["class_gap"] > 100 * tolerance(case_id, "class_abs"):
        bad.append(f"{case_id}: classes {score['class_gap']:.3e} apart, tolerance {tolerance(case_id, 'class_abs'):.3e}")
    return bad


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
    if name == "floor-under-pane":  # the truth is that of infinite plates and unbounded depth: the difference must not matter
        bias = under_pane_bias()
        print(name, "bias bound", bias, "recorded", rec["bias_bound"])
        assert abs(bias - rec["bias_bound"]) <= 1e-5 * bias and bias <= 0.1 * fig["rel_se"]
