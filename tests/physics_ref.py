"""Float64 physics for the shading path: BSDF lobes, Fresnel terms, microfacet distribution, light sampling, polygon
irradiance and directional albedo; the pinhole camera; the structure of the samplers; Whitted's recursion over a stack of
panes; Russian roulette and what it does to path lengths and to per-sample radiance; a floor under a pane; the surface of a
triangle or sphere hit (point, normals, tangent, uv, spawn origin) and the texel an image texture shows there — written from the
published models and the geometry in plain numpy.

Test infrastructure only.  Nothing here imports the oracle or the product, calls their arithmetic or follows their
operation order: every function states the formula of its source (named in its docstring) in float64, so a term that
the oracle and the device both misread disagrees with this file.

Where the reference renderer knowingly differs from the textbook, the difference is an entry of DEVIATIONS and the
functions follow the reference *only while that entry is switched on* (the default).  `textbook(key)` switches one entry
off, `mutated(name)` plants one single-term mistake (MUTATIONS); tests/test_physics.py uses the first to prove that every
entry is live and the second to prove that the comparisons would notice a misread term.

Conventions: arrays are (n, 3) float64, directions point away from the surface (wo towards the viewer, wi towards the
light), local frames have the shading normal on +z, spectra are RGB triples.
"""
import contextlib

import numpy as np

MATTE, GLASS, METAL, GLOSSY = 0, 1, 2, 3
POINT, SPOT, DISTANT, RECT = 0, 1, 2, 3
BX_REFLECTION, BX_TRANSMISSION, BX_DIFFUSE, BX_GLOSSY, BX_SPECULAR = 1, 2, 4, 8, 16

# ----------------------------------------------------------------------------- the deviation ledger
# Each entry: key, the SURVEY §8 quirk it restates (None = found by these tests), where the reference does it
# (file:line under yuki/src of the reference), the sentence that SURVEY's quirk ledger carries, and what the tests assert
# instead of the textbook.  The citations were read in the reference's text; tests/test_physics.py::test_ledger_entry_is_live
# switches every entry off in turn and requires the figure named in `live` (case of tests/physics_cases.py, figure) to fail.
DEVIATIONS = [
    dict(
        key="emission_beta_squared", quirk=2, where="integrators/path.rs:121-129",
        sentence="Emission seen after a specular bounce is weighted by beta twice (beta^2 * Le), not once.",
        asserts="li of an emitter seen through an index-matched pane is (T/0.5)^2 * Le per transmitted sample",
        live=("estimator", "emitter_through_pane"),
    ),
    dict(
        key="nee_consumes_dimensions", quirk=4, where="integrators/path.rs:103-114",
        sentence="Every light consumes two sampler dimensions at every hit whether or not it contributes; the cosine is clamp(ns.l, 0, 1).",
        asserts="a light below the floor leaves the furnace mean intact and shifts every later draw by two dimensions",
        live=("estimator", "dimension_shift"),
    ),
    dict(
        key="lobe_choice_uniform", quirk=9, where="materials/bsdfs/mod.rs:166-198, materials/glass.rs:27-45",
        sentence="Glass is two specular lobes chosen uniformly by u0 < 0.5 with pdf 1/2 each, not one Fresnel-weighted lobe; the remapped u0 is u0*(k-comp).",
        asserts="glass samples: reflection iff u0 < 0.5, pdf exactly 0.5 (pbrt's FresnelSpecular would give pdf F or 1-F)",
        live=("bsdf/glass-1.5/ortho", "s_pdf_abs"),
    ),
    dict(
        key="signed_pdf", quirk=11, where="materials/bsdfs/trowbridge_reitz.rs:76-78",
        sentence="The half-vector pdf is D(wh)*cos(theta_h) without abs: it is negative whenever wo lies below the shading normal.",
        asserts="microfacet sample pdf = sign(cos theta_o) * D*|cos theta_h| / (4 wo.wh)",
        live=("bsdf/metal-0.2/ortho", "s_pdf_rel"),
    ),
    dict(
        key="alpha_clamp", quirk=11, where="materials/bsdfs/trowbridge_reitz.rs:16-20",
        sentence="Trowbridge-Reitz alpha is clamped to at least 1e-3.",
        asserts="metal at alpha 1e-4 evaluates as alpha 1e-3",
        live=("bsdf/metal-0.0001/ortho", "f_rel"),
    ),
    dict(
        key="glossy_alpha_squared", quirk=11, where="materials/glossy.rs:39-49",
        sentence="Glossy uses alpha = r^2, and under remap alpha = roughness_to_alpha(r)^2 (the square is applied after the remap, not to r).",
        asserts="glossy f and pdf with alpha = roughness_to_alpha(r)**2 (remap) or r**2",
        live=("bsdf/glossy-remap-0.4/ortho", "f_rel"),
    ),
    dict(
        key="sigma_radians", quirk=12, where="materials/bsdfs/oren_nayar.rs:17-22, materials/matte.rs:32, scene/pbrt/mod.rs:904-907",
        sentence="Oren-Nayar takes sigma in radians (pbrt: degrees), Lambert iff sigma == 0 exactly; the pbrt loader converts a file's sigma to radians twice.",
        asserts="Oren-Nayar A, B from sigma as given, in radians",
        live=("bsdf/oren-nayar-0.349/ortho", "f_rel"),
    ),
    dict(
        key="fixed_offset", quirk=13, where="interaction.rs:27-59",
        sentence="Rays leave a surface from p +- 1e-3*n (geometric n, side chosen by the direction), shadow rays run to t_max 0.9999 along the unnormalised p1 - o.",
        asserts="shadow ray origin p +- 1e-3*ng, direction p1 - origin (pbrt: error-bound offset, here none for an exact p)",
        live=("light/point", "ray_o_pos"),
    ),
    dict(
        key="no_eta2_transmission", quirk=None, where="materials/bsdfs/specular.rs:83-84",
        sentence="Specular transmission carries no (eta_i/eta_t)^2 radiance factor.",
        asserts="glass transmission f = T*(1-F)/|cos theta_i|",
        live=("bsdf/glass-1.5/ortho", "s_fresnel_abs"),
    ),
    dict(
        key="schlick_signed_cos", quirk=None, where="materials/bsdfs/fresnel.rs:113-115, materials/bsdfs/microfacet.rs:65-67",
        sentence="Schlick's Fresnel is evaluated at the signed cosine wi.faceforward(wh, +z): below the shading normal (1 - cos)^5 exceeds 1 and F exceeds 1.",
        asserts="glossy f with (1 - c)^5 at c = sign(wh.z) * wi.wh",
        live=("bsdf/glossy-0.3/ortho", "f_rel"),
    ),
    dict(
        key="distant_fixed_reach", quirk=None, where="lights/distant_light.rs:31",
        sentence="A distant light's shadow ray ends 10000 units away, not at twice the world radius.",
        asserts="distant light p1 = p + 1e4 * w",
        live=("light/distant", "p1_pos"),
    ),
    dict(
        key="spot_no_tester_when_black", quirk=None, where="lights/spot_light.rs:61-72",
        sentence="A spot light returns no visibility tester when its Li is black (outside the cone); pbrt always returns one.",
        asserts="spot light has-visibility flag = (Li is not black)",
        live=("light/spot", "flag_mismatch"),
    ),
    dict(
        key="camera_window_named_axis", quirk=None, where="camera.rs:73-87",
        sentence="The camera's screen window is +-1 along the axis the field of view names and +-1/aspect along the other; pbrt puts +-1 on the shorter axis.",
        asserts="camera ray direction with the field of view measured along the named axis, whichever is longer",
        live=("camera/x90", "d_angle_abs"),
    ),
    dict(
        key="strata_row_divides_by_ny", quirk=None, where="sampling/stratified.rs:127-128",
        sentence="A 2-D stratum s goes to cell (s % nx, s / ny), not (s % nx, s / nx): with nx != ny cells repeat and values leave [0,1).",
        asserts="the cells floor(u * (nx, ny)) of the spp samples of a pixel are the multiset {(s % nx, s / ny)}",
        live=("sampler/strata-2d-rect", "cells_mismatch"),
    ),
    dict(
        key="uniform_streams_overlap", quirk=None, where="sampling/uniform.rs:81-83",
        sentence="The uniform sampler seeks one per-pixel stream to sample_index * 65536 + dimension, so the draws of consecutive sample indices overlap after 65536 values.",
        asserts="32768 two-dimensional draws into sample index i, the stream continues with the first draws of index i + 1",
        live=("sampler/uniform", "seek_mismatch"),
    ),
    dict(
        key="rr_green_channel", quirk=None, where="integrators/path.rs:163-169",
        sentence="Russian roulette reads the green channel of beta, q = max(0.05, 1 - beta.g), where pbrt reads the largest component.",
        asserts="path lengths in a closed Lambert sphere whose albedo's green is not its largest channel follow q from beta.g",
        live=("rr-lengths/warm", "length_z"),
    ),
    dict(
        key="sphere_wo_transformed_again", quirk=None, where="shapes/sphere.rs:115-116",
        sentence="A sphere builds its SurfaceInteraction with the world-space -ray.d and then transforms it object-to-world, so on a rotated or mirrored sphere wo is transformed once too often.",
        asserts="a rotated Lambert sphere under a point light is lit only where (M wo).n and l.n have the same sign",
        live=("sphere-wo/rotated", "li_zero_mismatch"),
    ),
    dict(
        key="tangent_half_turn", quirk=None, where="shapes/triangle.rs:211-219",
        sentence="With vertex normals a triangle's shading tangent is (normalize(dpdu) x ns) x ns, which is minus dpdu's projection perpendicular to ns: the shading frame is turned half a turn about ns.",
        asserts="the unit tangent of a triangle with vertex normals is -normalize(dpdu - ns (dpdu.ns))",
        live=("surface/normals", "s_abs"),
    ),
    dict(
        key="texel_index_half_texel", quirk=None, where="textures/image_texture.rs:102-108",
        sentence="An image texture's texel index is trunc(max(s*w - 0.5, 0)), not floor(s*w): texel 0 is one and a half texels wide and the last texel half a texel.",
        asserts="a textured matte quad under a point light shows the texel trunc(max(s w - 0.5, 0)) of the float64 uv",
        live=("direct-textured/quad", "li_rel"),
    ),
]
# Read in the reference and found to agree with pbrt-v3, hence no entries: the spot light's falloff (lights/spot_light.rs:38-50:
# smooth (delta^2)^2 between cos_total_width and cos_falloff_start, 0 outside, 1 inside) and the rectangular light's emitting
# side (lights/rectangular_light.rs:48-55: the side its normal (0,-1,0) faces, as DiffuseAreaLight's n.w > 0); of the camera,
# look_at (math/transforms.rs:138-153: right = up x dir, new_up = dir x right, pbrt-v3 §2.7.7 LookAt term for term, so the same
# left-handed camera space) and the raster's y axis (camera.rs:88-93: 1 / (screen_min.y - screen_max.y), downwards as in
# pbrt-v3 §6.2 ProjectiveCamera).  The mutation `camera_y_up` shows that the comparison would notice the second.

DISTANT_WORLD_RADIUS = 10.0  # only what `textbook("distant_fixed_reach")` expects instead of the fixed reach

MUTATIONS = [
    "schlick_exponent_4",  # (1 - cos)^4 for (1 - cos)^5
    "oren_nayar_030",  # A = 1 - s^2 / (2 (s^2 + 0.30))
    "g_dropped",  # masking-shadowing G = 1
    "pdf_without_jacobian",  # half-vector pdf without the 1 / (4 wo.wh)
    "albedo_without_cos",  # directional albedo integrates f, not f cos
    "fresnel_rpar_swapped_eta",  # r_parallel with eta_i and eta_t exchanged (exchanging them in both amplitudes only swaps the two)
    "li_inverse_distance",  # point light Li = I / d
    "rect_pdf_without_cos",  # area-to-solid-angle pdf d^2 / A
    "snell_eta_inverted",  # refraction with eta_t / eta_i
    "sigma_to_degrees",  # Oren-Nayar's sigma converted as if it were wanted in degrees
    "camera_tan_full_fov",  # screen scaled by tan(fov) for tan(fov / 2)
    "camera_y_up",  # raster y counted upwards
    "camera_window_on_shorter_axis",  # the +-1 of the screen window put on the shorter axis whatever the fov names
    "strata_cell_transposed",  # a 2-D stratum's cell read as (row, column)
    "whitted_child_over_pdf",  # a Whitted child weighted f |cos| / pdf with the path tracer's lobe pdf of 1/2
    "whitted_eta2",  # a Whitted transmission child weighted by (eta_i / eta_t)^2
    "rr_from_bounce_3",  # Russian roulette from bounces > 2
    "rr_without_compensation",  # survivors not divided by 1 - q
    "rr_floor_010",  # q = max(0.10, ...)
    "clamp_after_beta",  # the indirect clamp applied to the fully weighted contribution
    "bary_rotated",  # a triangle's barycentric weights applied to (p1, p2, p0)
    "ns_unnormalised",  # the interpolated vertex normal used as it comes
    "swaps_ignored",  # swaps_handedness does not negate the normal
    "n_not_faceforwarded",  # the geometric normal left on its own side of the shading normal
    "tangent_from_dpdv",  # the tangent taken from dpdv
    "sphere_normal_by_m",  # a sphere's normal transformed by M instead of its inverse transpose
    "texel_v_not_flipped",  # image rows counted from the bottom
    "spawn_along_ns",  # the spawn offset taken along the shading normal
]
_MUTATION = None
_OFF = set()


@contextlib.contextmanager
def mutated(name):
    """Plant one single-term mistake in this reference (the power check)."""
    global _MUTATION
    assert name in MUTATIONS, name
    prev, _MUTATION = _MUTATION, name
    try:
        yield
    finally:
        _MUTATION = prev


@contextlib.contextmanager
def textbook(key):
    """Switch one ledger entry off: expect what the textbook does there."""
    assert key in {d["key"] for d in DEVIATIONS}, key
    _OFF.add(key)
    try:
        yield
    finally:
        _OFF.discard(key)


def _m(name):
    return _MUTATION == name


def _on(key):
    return key not in _OFF


# ----------------------------------------------------------------------------- vectors and frames
def f64(a):
    return np.asarray(a, dtype=np.float64)


def dot(a, b):
    return np.sum(f64(a) * f64(b), axis=-1)


def normalize(v):
    v = f64(v)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def frame(ns, dpdu):
    """Shading frame (s, t, n) — pbrt-v3 §9.1 (BSDF constructor): s = normalize(dpdu), t = n x s."""
    n = f64(ns)
    s = normalize(dpdu)
    return s, np.cross(n, s), n


def to_local(v, fr):
    """pbrt-v3 §9.1 BSDF::WorldToLocal."""
    return np.stack([dot(v, fr[0]), dot(v, fr[1]), dot(v, fr[2])], axis=-1)


def to_world(v, fr):
    """pbrt-v3 §9.1 BSDF::LocalToWorld."""
    v = f64(v)
    return fr[0] * v[..., 0:1] + fr[1] * v[..., 1:2] + fr[2] * v[..., 2:3]


# ----------------------------------------------------------------------------- diffuse lobes
def lambert_f(kd):
    """Lambertian BRDF R/pi — pbrt-v3 §8.3."""
    return f64(kd) / np.pi


def oren_nayar_ab(sigma):
    """Oren-Nayar A, B from sigma in radians — pbrt-v3 §8.4.1 (Oren and Nayar 1994, the qualitative model)."""
    sigma = float(sigma)
    if not _on("sigma_radians"):
        sigma = np.radians(sigma)  # pbrt's convention: the parameter is in degrees
    if _m("sigma_to_degrees"):
        sigma = np.degrees(sigma)
    s2 = sigma * sigma
    c = 0.30 if _m("oren_nayar_030") else 0.33
    return 1.0 - s2 / (2.0 * (s2 + c)), 0.45 * s2 / (s2 + 0.09)


def oren_nayar_f(kd, sigma, wo, wi):
    """f = R/pi (A + B max(0, cos(phi_i - phi_o)) sin(alpha) tan(beta)), alpha = max(theta_i, theta_o), beta = min —
    pbrt-v3 §8.4.1 eq. 8.10, local directions."""
    a, b = oren_nayar_ab(sigma)
    wo, wi = f64(wo), f64(wi)
    co, ci = np.abs(wo[:, 2]), np.abs(wi[:, 2])
    so, si = np.sqrt(np.maximum(0.0, 1.0 - co * co)), np.sqrt(np.maximum(0.0, 1.0 - ci * ci))
    with np.errstate(all="ignore"):
        cos_dphi = np.where((so > 0) & (si > 0), (wo[:, 0] * wi[:, 0] + wo[:, 1] * wi[:, 1]) / (so * si), 0.0)
        o_is_alpha = co < ci  # the larger polar angle has the smaller cosine
        sin_alpha = np.where(o_is_alpha, so, si)
        tan_beta = np.where(o_is_alpha, si / ci, so / co)
    return lambert_f(kd)[None, :] * (a + b * np.maximum(0.0, cos_dphi) * sin_alpha * tan_beta)[:, None]


def concentric_disk(u):
    """Shirley and Chiu's concentric map of the unit square onto the unit disk — pbrt-v3 §13.6.2."""
    o = 2.0 * f64(u) - 1.0
    x, y = o[:, 0], o[:, 1]
    with np.errstate(all="ignore"):
        wide = np.abs(x) > np.abs(y)
        r = np.where(wide, x, y)
        theta = np.where(wide, (np.pi / 4.0) * (y / x), np.pi / 2.0 - (np.pi / 4.0) * (x / y))
    theta = np.where((x == 0) & (y == 0), 0.0, theta)
    return np.stack([r * np.cos(theta), r * np.sin(theta)], axis=-1)


def cosine_hemisphere_sample(wo, u):
    """Malley's method: the concentric disk sample lifted to the hemisphere on wo's side — pbrt-v3 §13.6.3."""
    d = concentric_disk(u)
    z = np.sqrt(np.maximum(0.0, 1.0 - d[:, 0] ** 2 - d[:, 1] ** 2))
    return np.stack([d[:, 0], d[:, 1], np.where(f64(wo)[:, 2] < 0, -z, z)], axis=-1)


def cosine_hemisphere_pdf(wo, wi):
    """|cos theta_i| / pi on wo's side, 0 on the other — pbrt-v3 §13.6.3 with BxDF::Pdf §14.1."""
    wo, wi = f64(wo), f64(wi)
    return np.where(wo[:, 2] * wi[:, 2] > 0, np.abs(wi[:, 2]) / np.pi, 0.0)


# ----------------------------------------------------------------------------- Fresnel
def fresnel_dielectric(cos_i, eta_i, eta_t):
    """Unpolarised Fresnel reflectance of a dielectric interface; a negative cosine means the ray arrives from the
    eta_t side — pbrt-v3 §8.2.1 (FrDielectric).  1 under total internal reflection."""
    c = np.clip(f64(cos_i), -1.0, 1.0)
    inside = c <= 0
    ei = np.where(inside, eta_t, eta_i)
    et = np.where(inside, eta_i, eta_t)
    c = np.abs(c)
    sin_t = ei / et * np.sqrt(np.maximum(0.0, 1.0 - c * c))
    tir = sin_t >= 1.0
    cos_t = np.sqrt(np.maximum(0.0, 1.0 - sin_t * sin_t))
    with np.errstate(all="ignore"):
        if _m("fresnel_rpar_swapped_eta"):
            r_par = (ei * c - et * cos_t) / (ei * c + et * cos_t)
        else:
            r_par = (et * c - ei * cos_t) / (et * c + ei * cos_t)
        r_perp = (ei * c - et * cos_t) / (ei * c + et * cos_t)
        f = 0.5 * (r_par * r_par + r_perp * r_perp)
    return np.where(tir, 1.0, f)


def sin_theta_t(cos_i, eta_i, eta_t):
    """Snell's law: sin theta_t for the interface fresnel_dielectric describes — pbrt-v3 §8.2.1."""
    c = np.clip(f64(cos_i), -1.0, 1.0)
    inside = c <= 0
    ratio = np.where(inside, eta_t / eta_i, eta_i / eta_t)
    return ratio * np.sqrt(np.maximum(0.0, 1.0 - c * c))


def fresnel_conductor(cos_i, eta, k, eta_i=1.0):
    """Fresnel reflectance of a conductor with complex index eta + i k under a dielectric eta_i, from the complex
    amplitude coefficients r_s, r_p (Born and Wolf §14.2; pbrt-v3 §8.2.1 FrConductor is their expansion).  (n, 3)."""
    c = np.minimum(np.abs(f64(cos_i)), 1.0)[:, None]
    n = (f64(eta)[None, :] + 1j * f64(k)[None, :]) / eta_i
    s2 = 1.0 - c * c
    root = np.sqrt(n * n - s2)
    r_s = (c - root) / (c + root)
    r_p = (n * n * c - root) / (n * n * c + root)
    return 0.5 * (np.abs(r_s) ** 2 + np.abs(r_p) ** 2)


def fresnel_schlick(cos_i, r0):
    """Schlick's approximation R0 + (1 - R0)(1 - cos)^5 — Schlick 1994; pbrt-v3 §8.5 eq. 8.24."""
    c = np.clip(f64(cos_i), -1.0, 1.0)[:, None]
    e = 4 if _m("schlick_exponent_4") else 5
    r0 = f64(r0)[None, :]
    return r0 + (1.0 - r0) * (1.0 - c) ** e


# ----------------------------------------------------------------------------- Trowbridge-Reitz microfacets
def roughness_to_alpha(r):
    """pbrt-v3 §8.4.2 TrowbridgeReitzDistribution::RoughnessToAlpha: a quartic in ln(max(r, 1e-3))."""
    x = np.log(max(float(r), 1e-3))
    return 1.62142 + 0.819955 * x + 0.1734 * x**2 + 0.0171201 * x**3 + 0.000640711 * x**4


def tr_alpha(alpha):
    return max(float(alpha), 1e-3) if _on("alpha_clamp") else float(alpha)


def tr_d(wh, alpha):
    """Isotropic Trowbridge-Reitz (GGX) D(wh) = 1 / (pi a^2 cos^4 (1 + tan^2/a^2)^2) — pbrt-v3 §8.4.2 eq. 8.12."""
    c2 = f64(wh)[:, 2] ** 2
    with np.errstate(all="ignore"):
        t2 = (1.0 - c2) / c2
        d = 1.0 / (np.pi * alpha * alpha * c2 * c2 * (1.0 + t2 / (alpha * alpha)) ** 2)
    return np.where(c2 > 0, d, 0.0)


def tr_lambda(w, alpha):
    """Lambda(w) = (-1 + sqrt(1 + a^2 tan^2 theta)) / 2 — pbrt-v3 §8.4.3 eq. 8.13 for Trowbridge-Reitz."""
    c2 = f64(w)[:, 2] ** 2
    with np.errstate(all="ignore"):
        t2 = (1.0 - c2) / c2
        lam = 0.5 * (-1.0 + np.sqrt(1.0 + alpha * alpha * t2))
    return np.where(c2 > 0, lam, 0.0)


def tr_g(wo, wi, alpha):
    """Height-correlated masking-shadowing G = 1 / (1 + Lambda(wo) + Lambda(wi)) — pbrt-v3 §8.4.3."""
    if _m("g_dropped"):
        return np.ones(len(wo))
    return 1.0 / (1.0 + tr_lambda(wo, alpha) + tr_lambda(wi, alpha))


def half_vector(wo, wi):
    return normalize(f64(wo) + f64(wi))


def torrance_sparrow_f(wo, wi, alpha, fresnel):
    """f = D(wh) G(wo, wi) F / (4 |cos theta_o| |cos theta_i|) — pbrt-v3 §8.4.4 eq. 8.19.  `fresnel(c, c_signed)` -> (n, 3)
    is given the cosine between wi and the half vector, and the same cosine measured against the half vector turned to +z."""
    wo, wi = f64(wo), f64(wi)
    wh = half_vector(wo, wi)
    c = dot(wi, wh)
    c_signed = np.where(wh[:, 2] < 0, -c, c)
    with np.errstate(all="ignore"):
        s = tr_d(wh, alpha) * tr_g(wo, wi, alpha) / (4.0 * np.abs(wo[:, 2]) * np.abs(wi[:, 2]))
    return s[:, None] * fresnel(c, c_signed)


def half_vector_pdf(wo, wi, alpha):
    """Pdf of wi when wh is drawn from D(wh)|cos theta_h|: D |cos theta_h| / (4 wo.wh) — pbrt-v3 §14.1.1 (the
    half-angle change of variables d wh / d wi = 1 / (4 wo.wh)).  0 across hemispheres."""
    wo, wi = f64(wo), f64(wi)
    wh = half_vector(wo, wi)
    p = tr_d(wh, alpha) * np.abs(wh[:, 2])
    if _on("signed_pdf"):
        p = p * np.sign(wo[:, 2])
    if not _m("pdf_without_jacobian"):
        with np.errstate(all="ignore"):
            p = p / (4.0 * dot(wo, wh))
    return np.where(wo[:, 2] * wi[:, 2] > 0, p, 0.0)


def tr_sample_wh(wo, u, alpha):
    """Half vector for (u0, u1) when the full distribution of normals is sampled: tan^2 theta = a^2 u0 / (1 - u0),
    phi = 2 pi u1, turned into wo's hemisphere — pbrt-v3 §14.1.1 (TrowbridgeReitzDistribution::Sample_wh, sampleVisibleArea off)."""
    u = f64(u)
    t2 = alpha * alpha * u[:, 0] / (1.0 - u[:, 0])
    ct = 1.0 / np.sqrt(1.0 + t2)
    st = np.sqrt(np.maximum(0.0, 1.0 - ct * ct))
    phi = 2.0 * np.pi * u[:, 1]
    wh = np.stack([st * np.cos(phi), st * np.sin(phi), ct], axis=-1)
    return np.where((f64(wo)[:, 2] * wh[:, 2] > 0)[:, None], wh, -wh)


# ----------------------------------------------------------------------------- specular directions
def mirror(wo, n):
    """Reflection of wo about n: -wo + 2 (wo.n) n — pbrt-v3 §8.2.2."""
    wo, n = f64(wo), f64(n)
    return -wo + 2.0 * dot(wo, n)[:, None] * n


def snell(wo, eta_above, eta_below):
    """Refracted local direction through the z = 0 interface (index eta_above over +z, eta_below under it) and the total
    internal reflection mask — pbrt-v3 §8.2.3 (Refract): wt = -eta wo + (eta cos_i - cos_t) n, eta = eta_i / eta_t."""
    wo = f64(wo)
    above = wo[:, 2] > 0
    eta = np.where(above, eta_above / eta_below, eta_below / eta_above)
    if _m("snell_eta_inverted"):
        eta = 1.0 / eta
    n = np.where(above, 1.0, -1.0)
    ci = np.abs(wo[:, 2])
    s2t = eta * eta * np.maximum(0.0, 1.0 - ci * ci)
    tir = s2t >= 1.0
    ct = np.sqrt(np.maximum(0.0, 1.0 - s2t))
    wt = -eta[:, None] * wo
    wt[:, 2] += (eta * ci - ct) * n
    return wt, tir


# ----------------------------------------------------------------------------- materials -> BSDF
def material_alpha(m):
    """Microfacet alpha of a metal or glossy material description (kind, c = roughness, remap)."""
    r = float(np.float32(m["c"]))
    if m["kind"] == GLOSSY and not _on("glossy_alpha_squared"):
        # what a reader of "Glossy squares roughness" might expect instead: the square applied to r before the remap,
        # and no square at all without it (pbrt's alpha = roughness)
        return tr_alpha(roughness_to_alpha(r * r) if m.get("remap") else r)
    a = roughness_to_alpha(r) if m.get("remap") else r
    if m["kind"] == GLOSSY:
        a = a * a
    return tr_alpha(a)


def _spec(v):
    return f64(np.asarray(v, dtype=np.float32))


def lobe_f_local(m, wo, wi):
    """The material's non-specular BRDF for local directions, (n, 3); 0 for glass and for a black matte."""
    n = len(wo)
    kind = m["kind"]
    if kind == MATTE:
        kd = _spec(m["a"])
        if not kd.any():
            return np.zeros((n, 3))
        sigma = float(np.float32(m.get("c", 0.0)))
        if sigma == 0.0:
            return np.broadcast_to(lambert_f(kd), (n, 3)).copy()
        return oren_nayar_f(kd, sigma, wo, wi)
    if kind == METAL:
        eta, k = _spec(m["a"]), _spec(m["b"])
        return torrance_sparrow_f(wo, wi, material_alpha(m), lambda c, cs: fresnel_conductor(c, eta, k))
    if kind == GLOSSY:
        r0 = _spec(m["a"])
        return torrance_sparrow_f(wo, wi, material_alpha(m), lambda c, cs: fresnel_schlick(cs if _on("schlick_signed_cos") else np.abs(c), r0))
    return np.zeros((n, 3))


def bsdf_f(m, ng, ns, dpdu, wo, wi):
    """BSDF::f — pbrt-v3 §9.1: world directions go to the shading frame; reflection lobes count only when wo and wi lie on
    the same side of the *geometric* normal (every lobe with a non-zero f here is a reflection lobe).  -> (f (n, 3), same-side mask)."""
    fr = frame(ns, dpdu)
    reflect = dot(wi, ng) * dot(wo, ng) > 0
    with np.errstate(all="ignore"):
        f = lobe_f_local(m, to_local(wo, fr), to_local(wi, fr))
    return np.where(reflect[:, None], f, 0.0), reflect


def lobe_pdf_local(m, wo, wi):
    """Sampling density of the material's non-specular lobe for local directions."""
    if m["kind"] == MATTE:
        return cosine_hemisphere_pdf(wo, wi)
    return half_vector_pdf(wo, wi, material_alpha(m))


def lobe_type(m):
    """BxDF type bits of the non-specular lobe — pbrt-v3 §8.1 (BxDFType)."""
    return (BX_DIFFUSE if m["kind"] == MATTE else BX_GLOSSY) | BX_REFLECTION


def glass_sample(m, wo_local, u):
    """Specular reflection / transmission of a smooth dielectric — pbrt-v3 §8.2.2-8.2.3, as the two lobes
    SpecularReflection (f = R F / |cos|) and SpecularTransmission (f = T (1 - F) [eta_i^2/eta_t^2] / |cos|).
    -> dict(reflect mask, wi, f, pdf, type, tir mask, fresnel F of the chosen lobe)."""
    wo = f64(wo_local)
    u = f64(u)
    n = len(wo)
    eta = float(np.float32(m["c"]))
    R, T = _spec(m["a"]), _spec(m["b"])
    fr_wo = fresnel_dielectric(wo[:, 2], 1.0, eta)
    wt, tir = snell(wo, 1.0, eta)
    with np.errstate(all="ignore"):
        fr_wt = fresnel_dielectric(wt[:, 2], 1.0, eta)
        f_r = R[None, :] * (fr_wo / np.abs(wo[:, 2]))[:, None]
        f_t = T[None, :] * ((1.0 - fr_wt) / np.abs(wt[:, 2]))[:, None]
    if not _on("no_eta2_transmission"):
        e = np.where(wo[:, 2] > 0, 1.0 / eta, eta)  # eta_i / eta_t along the path
        f_t = f_t * (e * e)[:, None]
    if _on("lobe_choice_uniform"):
        refl = u[:, 0] < 0.5
        pdf = np.full(n, 0.5)
    else:  # one Fresnel-weighted lobe (pbrt-v3 §8.2.4 FresnelSpecular, sampled in §14.1.3)
        refl = u[:, 0] < fr_wo
        pdf = np.where(refl, fr_wo, 1.0 - fr_wo)
    wi = np.where(refl[:, None], wo * np.array([-1.0, -1.0, 1.0]), wt)
    f = np.where(refl[:, None], f_r, f_t)
    typ = np.where(refl, BX_SPECULAR | BX_REFLECTION, BX_SPECULAR | BX_TRANSMISSION)
    none = ~refl & tir
    wi[none] = 0
    f[none] = 0
    return dict(reflect=refl, wi=wi, f=f, pdf=np.where(none, 0.0, pdf), type=np.where(none, 0, typ), tir=tir, none=none,
                fresnel=np.where(refl, fr_wo, fr_wt), sin_t=sin_theta_t(wo[:, 2], 1.0, eta))


# ----------------------------------------------------------------------------- lights
def _apply_point(m, p):
    m = f64(m)
    return f64(p) @ m[:3, :3].T + m[:3, 3]


def shadow_ray(p, ng, p1):
    """The ray from a surface point towards p1: origin moved off the surface, direction p1 - origin (not normalised),
    t_max 0.9999 (pbrt-v3 §3.9.5 Interaction::SpawnRayTo with 1 - ShadowEpsilon; the origin offset follows the ledger)."""
    p, ng, p1 = f64(p), f64(ng), f64(p1)
    if _on("fixed_offset"):
        side = np.where(dot(p1 - p, ng) > 0, 1.0, -1.0)
        o = p + 1e-3 * side[:, None] * ng
    else:
        o = p.copy()  # pbrt offsets by the error bound of p, which is zero for a point given exactly
    return o, p1 - o, 0.9999


def spot_falloff(cos_theta, total_deg, falloff_deg):
    """pbrt-v3 §12.3.1 SpotLight::Falloff: 0 outside the cone, 1 inside the falloff start, (delta^2)^2 between."""
    ct, cf = np.cos(np.radians(total_deg)), np.cos(np.radians(falloff_deg))
    d = np.clip((f64(cos_theta) - ct) / (cf - ct), 0.0, 1.0)
    return np.where(cos_theta < ct, 0.0, d**4)


def light_sample(light, index, p, ng, u):
    """Light::Sample_Li for n surface points — pbrt-v3 §12.3 (point), §12.3.1 (spot), §12.4 (distant), §12.5 + §14.2.2
    (diffuse area light sampled by area, pdf converted to solid angle: d^2 / (|cos| A)).
    `light`: dict(kind, l2w 4x4, I or L, and total/falloff degrees | w | size).
    -> dict(l, li, pdf, has_vis, area_light, p1, ray_o, ray_d, t_max, plus `dist`, `cos_light`, `cos_spot` for conditioning)."""
    p, ng, u = f64(p), f64(ng), f64(u)
    n = len(p)
    kind = light["kind"]
    out = dict(area_light=np.full(n, -1.0), pdf=np.ones(n), has_vis=np.ones(n))
    if kind in (POINT, SPOT):
        pos = _apply_point(light["l2w"], np.zeros(3))
        to = pos[None, :] - p
        d = np.linalg.norm(to, axis=1)
        l = to / d[:, None]
        inten = f64(np.asarray(light["I"], dtype=np.float32))
        li = inten[None, :] / (d if _m("li_inverse_distance") else d * d)[:, None]
        if kind == SPOT:
            w2l = np.linalg.inv(f64(light["l2w"]))
            cos_spot = normalize((-l) @ w2l[:3, :3].T)[:, 2]
            li = li * spot_falloff(cos_spot, light["total"], light["falloff"])[:, None]
            out["cos_spot"] = cos_spot
            if _on("spot_no_tester_when_black"):
                out["has_vis"] = (li.max(axis=1) > 0).astype(np.float64)
        out.update(l=l, li=li, p1=np.broadcast_to(pos, (n, 3)).copy(), dist=d)
    elif kind == DISTANT:
        w = f64(np.asarray(light["w"], dtype=np.float32))
        reach = 1e4 if _on("distant_fixed_reach") else 2.0 * DISTANT_WORLD_RADIUS
        out.update(l=np.broadcast_to(w, (n, 3)).copy(), li=np.broadcast_to(f64(np.asarray(light["L"], dtype=np.float32)), (n, 3)).copy(),
                   p1=p + reach * w[None, :], dist=np.full(n, reach))
    else:
        sx, sy = (float(np.float32(s)) for s in light["size"])
        local = np.stack([(u[:, 0] - 0.5) * sx, np.zeros(n), (u[:, 1] - 0.5) * sy], axis=-1)
        ps = _apply_point(light["l2w"], local)
        nl = f64(light["l2w"])[:3, :3] @ np.array([0.0, -1.0, 0.0])  # rigid transform: normals rotate like vectors
        to = ps - p
        d = np.linalg.norm(to, axis=1)
        wi = to / d[:, None]
        cos_l = -(wi @ nl)
        radiance = f64(np.asarray(light["L"], dtype=np.float32))
        with np.errstate(all="ignore"):
            pdf = d * d / (sx * sy) if _m("rect_pdf_without_cos") else d * d / (np.abs(cos_l) * sx * sy)
        out.update(l=wi, li=np.where((cos_l > 0)[:, None], radiance[None, :], 0.0), pdf=pdf, p1=ps, dist=d, cos_light=cos_l,
                   area_light=np.full(n, float(index)))
    out["ray_o"], out["ray_d"], out["t_max"] = shadow_ray(p, ng, out["p1"])
    return out


def polygon_irradiance(p, n, verts):
    """Irradiance at p (normal n) from a polygon of unit radiance seen from its emitting side: Lambert's formula
    E = 1/2 sum_i theta_i (gamma_i . n), theta_i the angle subtended by edge i and gamma_i the unit normal of the plane
    through p and edge i (Lambert 1760; Arvo 1995, "Applications of irradiance tensors to the simulation of non-Lambertian phenomena", eq. 1).  Vertices in order; the sign is fixed by
    taking the absolute value, valid while the whole polygon lies above the horizon of n."""
    p, n = f64(p), f64(n)
    v = normalize(f64(verts) - p)
    e = 0.0
    for i in range(len(v)):
        a, b = v[i], v[(i + 1) % len(v)]
        theta = np.arccos(np.clip(a @ b, -1.0, 1.0))
        gamma = np.cross(a, b)
        e += theta * (gamma / np.linalg.norm(gamma)) @ n
    return abs(0.5 * e)


# ----------------------------------------------------------------------------- directional albedo
def directional_albedo(m, cos_o, n_mu=1024, n_phi=512):
    """rho(wo) = integral of f(wo, wi) |cos theta_i| d wi over wo's hemisphere by the midpoint rule over (mu = cos theta_i, phi),
    with mu = t^2 so that the cells crowd towards grazing wi less than towards the lobe — pbrt-v3 §8.1.1 (rho_hd).  (3,) RGB.
    At the default grid the result is within 7e-5 of the 4096 x 2048 grid's for every material and angle the tests use
    (alpha >= 0.09), under a fiftieth of the standard error it is compared with."""
    cos_o = float(cos_o)
    wo = np.array([[np.sqrt(1.0 - cos_o * cos_o), 0.0, cos_o]])
    t = (np.arange(n_mu) + 0.5) / n_mu
    mu, dmu = t * t, 2.0 * t / n_mu
    phi = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    total = np.zeros(3)
    for k in range(0, n_mu, 64):  # in slabs: the full grid at once is 2 M directions x several temporaries
        m_, dm_ = mu[k : k + 64, None], dmu[k : k + 64, None]
        s = np.sqrt(1.0 - m_ * m_)
        wi = np.stack([(s * np.cos(phi)[None, :]).ravel(), (s * np.sin(phi)[None, :]).ravel(), np.broadcast_to(m_, (len(m_), n_phi)).ravel()], axis=-1)
        f = lobe_f_local(m, np.broadcast_to(wo, wi.shape), wi)
        w = np.broadcast_to(dm_ * (2.0 * np.pi / n_phi), (len(m_), n_phi)).ravel()
        if not _m("albedo_without_cos"):
            w = w * wi[:, 2]
        total += (f * w[:, None]).sum(axis=0)
    return total


# ----------------------------------------------------------------------------- camera
FOV_X, FOV_Y = 0, 1


def angle_between(a, b):
    """Angle between vectors as atan2(|a x b|, a.b): accurate at angles near 0 and pi, where acos of the dot product is not."""
    a, b = f64(a), f64(b)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), dot(a, b))


def camera_basis(cam):
    """(right, up, forward) of a camera at `position` looking at `target` — pbrt-v3 §2.7.7 (LookAt): forward = normalize(target -
    position), right = normalize(normalize(up) x forward), up' = forward x right; camera space is left-handed, +z forward."""
    fwd = normalize(f64(cam["target"]) - f64(cam["position"]))
    right = normalize(np.cross(normalize(cam["up"]), fwd))
    return right, np.cross(fwd, right), fwd


def camera_window(cam, res):
    """Half extents (wx, wy) of the screen window — pbrt-v3 §6.2 (the window of a ProjectiveCamera) with the ledger's choice of
    the axis that gets +-1; the other axis is scaled by the aspect ratio so that pixels are square."""
    rx, ry = float(res[0]), float(res[1])
    named_x = cam["fov_axis"] == FOV_X
    if not _on("camera_window_named_axis") or _m("camera_window_on_shorter_axis"):
        named_x = rx <= ry  # pbrt: the field of view spans the shorter axis
    return (1.0, ry / rx) if named_x else (rx / ry, 1.0)


def _camera_tan(cam):
    fov = np.radians(float(np.float32(cam["fov_degrees"])))
    return np.tan(fov if _m("camera_tan_full_fov") else 0.5 * fov)


def camera_ray(cam, res, p_film):
    """Pinhole camera — pbrt-v3 §6.2.2 (PerspectiveCamera::GenerateRay without a lens): the ray through raster point p starts
    at the camera position and runs along normalize(forward + x_s t right + y_s t up'), t = tan(fov / 2), where (x_s, y_s) is p
    mapped to the screen window with raster y pointing down.  -> (origin (n, 3), direction (n, 3))."""
    p = f64(p_film)
    right, upv, fwd = camera_basis(cam)
    wx, wy = camera_window(cam, res)
    t = _camera_tan(cam)
    xs = (2.0 * p[:, 0] / float(res[0]) - 1.0) * wx
    ys = (1.0 - 2.0 * p[:, 1] / float(res[1])) * wy
    if _m("camera_y_up"):
        ys = -ys
    d = normalize(fwd[None, :] + (xs * t)[:, None] * right[None, :] + (ys * t)[:, None] * upv[None, :])
    return np.broadcast_to(f64(cam["position"]), d.shape).copy(), d


def camera_raster(cam, res, d):
    """The inverse of camera_ray: the raster point a ray direction passes through."""
    d = f64(d)
    right, upv, fwd = camera_basis(cam)
    wx, wy = camera_window(cam, res)
    t = _camera_tan(cam)
    z = d @ fwd
    xs, ys = (d @ right) / z / t / wx, (d @ upv) / z / t / wy
    if _m("camera_y_up"):
        ys = -ys
    return np.stack([(xs + 1.0) * 0.5 * float(res[0]), (1.0 - ys) * 0.5 * float(res[1])], axis=-1)


def camera_fov_from_rays(cam, res, d_first, d_last):
    """The full angle between the two film edges on the camera's fov axis, from the rays through the centres of the first and the
    last pixel of that axis (any row / column): the screen coordinate (d.axis)/(d.forward) is linear in the raster coordinate and the
    two pixel centres lie 1 - 1/res of the half width from the middle, so the edges' tangent follows by proportion."""
    right, upv, fwd = camera_basis(cam)
    axis, n = (right, res[0]) if cam["fov_axis"] == FOV_X else (upv, res[1])
    s0, s1 = (f64(d_first) @ axis) / (f64(d_first) @ fwd), (f64(d_last) @ axis) / (f64(d_last) @ fwd)
    return 2.0 * np.arctan(0.5 * abs(s1 - s0) / (1.0 - 1.0 / float(n)))


# ----------------------------------------------------------------------------- samplers
def strata_cell(stratum, nx, ny):
    """Cell (x, y) of stratum s in an nx x ny grid — pbrt-v3 §7.3 (StratifiedSample2D numbers the cells row by row: s = y nx + x)."""
    s = np.asarray(stratum, dtype=np.int64)
    x, y = s % nx, s // (ny if _on("strata_row_divides_by_ny") else nx)
    return (y, x) if _m("strata_cell_transposed") else (x, y)


def uniform_moments_z(u):
    """z values of the sample mean and the sample variance of n draws against U[0,1): mean 1/2 with variance 1/(12 n); the variance
    estimate has mean 1/12 and variance (mu_4 - sigma^4)/n = (1/80 - 1/144)/n = 1/(180 n)."""
    u = f64(u).ravel()
    n = len(u)
    return float((u.mean() - 0.5) / np.sqrt(1.0 / 12.0 / n)), float((((u - 0.5) ** 2).mean() - 1.0 / 12.0) / np.sqrt(1.0 / 180.0 / n))


# ----------------------------------------------------------------------------- Whitted over a stack of panes
SPAWN_OFFSET = 1e-3  # the ledger's `fixed_offset`


def _interface(cos_in, inside, eta):
    """(F seen by the arriving ray, F seen from the transmitted direction, cosine of the transmitted ray, total internal reflection)
    at a smooth interface of a pane of index eta in air, for a ray arriving at |cos| = cos_in from inside or outside the glass —
    pbrt-v3 §8.2.1-8.2.3."""
    signed = -cos_in if inside else cos_in  # fresnel_dielectric: a negative cosine arrives from the eta side
    f_in = float(fresnel_dielectric(signed, 1.0, eta))
    sin_t = float(sin_theta_t(signed, 1.0, eta))
    if sin_t >= 1.0:
        return 1.0, 1.0, 0.0, True
    cos_t = np.sqrt(1.0 - sin_t * sin_t)
    return f_in, float(fresnel_dielectric(cos_t if inside else -cos_t, 1.0, eta)), cos_t, False


def whitted_stack(panes, eta, R, T, cos_start, start_y, start_inside, max_depth):
    """Whitted's recursion (Whitted 1980; pbrt-v3 §14.2 WhittedIntegrator::Li with SpecularReflect / SpecularTransmit) over
    horizontal panes [(y_bottom, y_top), ...] of index eta above a matte floor at y = 0, for a ray that starts at height start_y
    going DOWN at |cos| = cos_start to the vertical, in the glass or in air.  Every hit on glass spawns a reflection child of
    weight R F and, unless totally reflected, a transmission child of weight T (1 - F): f |cos|, no pdf, no eta^2 (the ledger's
    `no_eta2_transmission`), while depth + 1 < max_depth.  Children start SPAWN_OFFSET off the surface on their own side (the
    ledger's `fixed_offset`).  The rays stay in their vertical plane of incidence, so a leaf is described by its weight and the
    horizontal distance travelled along the ray's heading.
    -> (RGB weight reaching the background, [(RGB weight, horizontal distance) of every floor hit], closest-hit rays, the
    largest horizontal distance any ray reached)."""
    R, T = f64(R), f64(T)
    faces = sorted([y for pane in panes for y in pane] + [0.0])
    off = SPAWN_OFFSET if _on("fixed_offset") else 0.0
    cos_of, tan_of, iface = {}, {}, {}
    f_in, f_out, cos_t, tir = _interface(cos_start, start_inside, eta)
    cos_of[start_inside] = cos_start
    if not tir:
        cos_of[not start_inside] = cos_t
    for inside, c in cos_of.items():
        tan_of[inside] = np.sqrt(max(0.0, 1.0 - c * c)) / c
        iface[inside] = _interface(c, inside, eta)
    over_pdf = 2.0 if _m("whitted_child_over_pdf") else 1.0
    background, floor, reach = np.zeros(3), [], [0.0]

    def trace(y, up, inside, depth, weight, s):
        ahead = [f for f in faces if (f > y if up else f < y)]
        if not ahead:
            background[:] += weight
            return 1
        hit = min(ahead) if up else max(ahead)
        s = s + abs(hit - y) * tan_of[inside]
        reach[0] = max(reach[0], s)
        if hit == 0.0:
            floor.append((weight, s))
            return 1
        rays = 1
        if depth + 1 < max_depth:
            f_here, f_there, _, total = iface[inside]
            rays += trace(hit + (-off if up else off), not up, inside, depth + 1, weight * R * (f_here * over_pdf), s)
            if not total:
                w = T * ((1.0 - f_there) * over_pdf)
                if not _on("no_eta2_transmission") or _m("whitted_eta2"):
                    w = w * ((eta if inside else 1.0 / eta) ** 2)  # (eta_i / eta_t)^2 along the path
                rays += trace(hit + (off if up else -off), up, not inside, depth + 1, weight * w, s)
        return rays

    n = trace(start_y, False, start_inside, 0, np.ones(3), 0.0)
    return background, floor, n, reach[0]


# ----------------------------------------------------------------------------- Russian roulette
def rr_rule(beta, bounce):
    """Termination probability after the vertex of `bounce` (0 = the camera ray's hit), None when the roulette is not played —
    pbrt-v3 §14.5.4 (PathIntegrator::Li, "Possibly terminate the path with Russian roulette"): from bounces > 3,
    q = max(0.05, 1 - the largest component of beta), survivors divided by 1 - q; the ledger reads green instead."""
    if not bounce > (2 if _m("rr_from_bounce_3") else 3):
        return None
    b = float(beta[1]) if _on("rr_green_channel") else float(np.max(beta))
    return max(0.10 if _m("rr_floor_010") else 0.05, 1.0 - b)


def rr_survive(beta, q):
    return f64(beta) if _m("rr_without_compensation") else f64(beta) / (1.0 - q)


def rr_length_distribution(rho, max_depth):
    """{rays traced: probability} of a path that hits a Lambert surface of albedo rho at every vertex and finds no light: cosine
    sampling makes f cos / pdf = rho exactly, so beta is deterministic and only the roulette ends a path before max_depth."""
    rho = f64(np.asarray(rho, dtype=np.float32))
    beta, alive, out = np.ones(3), 1.0, {}
    for bounce in range(max_depth):
        beta = beta * rho
        q = rr_rule(beta, bounce)
        if q is not None and bounce + 1 < max_depth:
            out[bounce + 1] = alive * q
            alive *= 1.0 - q
            beta = rr_survive(beta, q)
    out[max_depth] = alive
    return {k: v for k, v in out.items() if v > 0}


def slab_path_classes(cos_in, eta, max_depth):
    """[(li / B, probability)] of one path-traced sample through a clear pane (R = T = 1) of index eta in air under a uniform
    background B, no lights: every sequence of the uniform lobe choice (probability 1/2 each, weight F / 0.5 or (1 - F) / 0.5 — the
    ledger's `lobe_choice_uniform`) and every roulette outcome is followed; a path that leaves the pane collects beta B when its
    next ray is traced, one that is ended by the roulette or by max_depth collects nothing.  Equal values are merged."""
    f_in, f_out, cos_t, tir = _interface(cos_in, False, eta)
    assert not tir
    f_glass = _interface(cos_t, True, eta)
    classes = {}

    def add(value, p):
        key = round(value, 12)
        classes[key] = classes.get(key, 0.0) + p

    def trace(bounce, beta, p, inside, escaped):
        if bounce >= max_depth:
            return add(0.0, p)
        if escaped:
            return add(beta, p)
        f_here, f_there = (f_glass[0], f_glass[1]) if inside else (f_in, f_out)
        for reflect in (True, False):
            b = beta * ((f_here if reflect else 1.0 - f_there) / 0.5)
            pr = 0.5 * p
            q = rr_rule(np.full(3, b), bounce)
            if q is not None:
                add(0.0, pr * q)
                pr *= 1.0 - q
                b = float(rr_survive(np.full(3, b), q)[0])
            if pr > 0.0:
                trace(bounce + 1, b, pr, inside if reflect else not inside, escaped=(reflect != inside))

    trace(0, 1.0, 1.0, False, False)
    return sorted(classes.items())


def clamped_emission(beta, le, clamp):
    """Emission found after a specular bounce under the reference's `indirect_clamp` (integrators/path.rs:121-129, a parameter of
    its own; pbrt has none): the radiance of the vertex, which already carries beta once (the ledger's `emission_beta_squared`), is
    clamped per channel, then weighted by beta like every vertex."""
    le = f64(le)
    if _m("clamp_after_beta"):
        return np.minimum(beta * beta * le, clamp)
    inner = beta * le if _on("emission_beta_squared") else le
    return beta * np.minimum(inner, clamp)


# ----------------------------------------------------------------------------- a Lambert floor under a clear pane
def pane_terms(eta, n_vertices, n_mu=4096):
    """Cosine-weighted hemispherical means, by the midpoint rule over mu^2, of what a clear pane of index eta does to light that
    arrives from one side: r[j] / t[j] = the part that returns / passes after exactly j specular vertices (Stokes' sum over the
    inter-reflections, e.g. Born and Wolf §7.6.1 without interference): r[1] = F, r[j] = (1-F)^2 F^(j-2) for odd j >= 3,
    t[j] = (1-F)^2 F^(j-2) for even j.  Their sums are R = 2F / (1+F) and T = 1 - R.  -> (r, t, R mean, T mean)."""
    x = (np.arange(n_mu) + 0.5) / n_mu  # x = mu^2: the cosine-weighted measure 2 mu d mu is d x
    f = fresnel_dielectric(np.sqrt(x), 1.0, eta)
    r, t = np.zeros(n_vertices + 1), np.zeros(n_vertices + 1)
    for j in range(1, n_vertices + 1):
        if j == 1:
            r[j] = f.mean()
        elif j % 2:
            r[j] = ((1.0 - f) ** 2 * f ** (j - 2)).mean()
        else:
            t[j] = ((1.0 - f) ** 2 * f ** (j - 2)).mean()
    big_r = 2.0 * f / (1.0 + f)
    return r, t, float(big_r.mean()), float(1.0 - big_r.mean())


def floor_under_pane(rho, eta, max_depth=None):
    """Radiance, in units of the background's, leaving a Lambert floor of albedo rho under an infinite clear pane: the floor sees
    the background through the pane and itself in it, L = rho (T B + R L), so L = rho T B / (1 - rho R) with the means of pane_terms.
    With `max_depth`: the expectation of a path tracer that traces at most that many rays and starts with the ray that hits the
    floor; the floor's diffuse bounce makes every return to it a renewal, so the truncated value follows by recursion over the bounce
    index of the floor vertex.  (The roulette changes no expectation.)"""
    rho = f64(rho)
    if max_depth is None:
        _, _, rm, tm = pane_terms(eta, 1)
        return rho * tm / (1.0 - rho * rm)
    r, t, _, _ = pane_terms(eta, max_depth)
    value = np.zeros((max_depth + 1, len(rho)))  # value[d]: radiance gathered from a floor vertex hit by the ray of bounce d
    for d in range(max_depth - 1, -1, -1):
        acc = np.zeros(len(rho))
        for j in range(1, max_depth - d):  # the ray after j pane vertices is ray d + j and must still be traced
            acc += t[j] + r[j] * value[d + j]
        value[d] = rho * acc
    return value[0]


# ----------------------------------------------------------------------------- the surface of a hit
# What the integrators read off a hit, from the geometry: the f32 ray and the f32 scene arrays promoted to float64, every hit
# found by solving for it against every primitive.  The scene is a dict of plain arrays: points (nv, 3), indices (nt, 3),
# tri_flags (nt, 3) booleans (has normals, has uvs, swaps handedness: its mesh's), normals (nv, 3) or None, uvs (nv, 2) or None,
# spheres = [(object_to_world 4x4, world_to_object 4x4, radius)].  Source shapes are numbered triangles first, then spheres.
DEFAULT_UVS = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]])  # a triangle of a mesh without uvs (pbrt-v3 §3.6.2 GetUVs)
SPAWN_OFFSET = 1e-3


def _bary(b):
    """The weights of (p0, p1, p2)."""
    return np.roll(b, 1, axis=-1) if _m("bary_rotated") else b


def _unit_or_zero(v):
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        return np.where(n > 0, v / n, 0.0)


def triangle_hits(scene, o, d):
    """Closest triangle hit of every ray by Cramer's rule on o + t d = p2 + b0 (p0 - p2) + b1 (p1 - p2) (Moeller and Trumbore 1997):
    (t, triangle, barycentrics (n, 3)); t = inf where no triangle is hit in front of the origin."""
    o, d = f64(o), f64(d)
    pts, idx = f64(scene["points"]), np.asarray(scene["indices"], dtype=np.int64)
    n = len(o)
    best_t, best_k, best_b = np.full(n, np.inf), np.full(n, -1), np.zeros((n, 3))
    for k in range(len(idx)):
        p0, p1, p2 = pts[idx[k, 0]], pts[idx[k, 1]], pts[idx[k, 2]]
        e0, e1 = p0 - p2, p1 - p2
        m = np.stack([np.broadcast_to(e0, (n, 3)), np.broadcast_to(e1, (n, 3)), -d], axis=-1)  # columns: e0, e1, -d
        det = np.linalg.det(m)
        with np.errstate(all="ignore"):
            sol = np.linalg.solve(np.where((det != 0)[:, None, None], m, np.eye(3)), (o - p2)[:, :, None])[:, :, 0]
        b0, b1, t = sol[:, 0], sol[:, 1], sol[:, 2]
        b2 = 1.0 - b0 - b1
        ok = (det != 0) & (b0 >= 0) & (b1 >= 0) & (b2 >= 0) & (t > 0) & (t < best_t)
        best_t = np.where(ok, t, best_t)
        best_k = np.where(ok, k, best_k)
        best_b = np.where(ok[:, None], np.stack([b0, b1, b2], axis=-1), best_b)
    return best_t, best_k, best_b


def triangle_surface(scene, o, d, tri, b):
    """p, uv, geometric and shading normal and the unit tangent of triangle hits with barycentrics b — pbrt-v3 §3.6.2-3.6.3:
    p = sum b_i p_i and uv = sum b_i uv_i; the face normal is normalize((p0 - p2) x (p1 - p2)), negated under swaps_handedness;
    with vertex normals ns = normalize(sum b_i n_i) and n is the face normal on ns's side; dpdu solves the 2 x 2 uv system and the
    tangent is its normalised projection into the plane perpendicular to ns.  Also the branch each row takes: uv_degenerate (the
    three uvs span no area: no dpdu, any tangent perpendicular to ns will do), ns_zero (the interpolated normal vanishes: ns = n),
    tangent_along_ns (dpdu has no component perpendicular to ns)."""
    d = f64(d)
    pts, idx = f64(scene["points"]), np.asarray(scene["indices"], dtype=np.int64)[tri]
    flags = np.asarray(scene["tri_flags"], dtype=bool)[tri]
    has_n, has_uv, swaps = flags[:, 0], flags[:, 1], flags[:, 2]
    w = _bary(f64(b))
    p0, p1, p2 = pts[idx[:, 0]], pts[idx[:, 1]], pts[idx[:, 2]]
    p = w[:, 0:1] * p0 + w[:, 1:2] * p1 + w[:, 2:3] * p2
    uv3 = np.broadcast_to(DEFAULT_UVS, (len(tri), 3, 2)).copy()
    if scene.get("uvs") is not None:
        uv3 = np.where(has_uv[:, None, None], f64(scene["uvs"])[idx], uv3)
    uv = (w[:, :, None] * uv3).sum(axis=1)
    face = normalize(np.cross(p0 - p2, p1 - p2))
    if not _m("swaps_ignored"):
        face = np.where(swaps[:, None], -face, face)
    # dpdu, dpdv from (p0 - p2, p1 - p2) = (duv02, duv12) (dpdu, dpdv)
    duv02, duv12 = uv3[:, 0] - uv3[:, 2], uv3[:, 1] - uv3[:, 2]
    det = duv02[:, 0] * duv12[:, 1] - duv02[:, 1] * duv12[:, 0]
    uv_degenerate = det == 0
    with np.errstate(all="ignore"):
        dpdu = (duv12[:, 1:2] * (p0 - p2) - duv02[:, 1:2] * (p1 - p2)) / det[:, None]
        dpdv = (-duv12[:, 0:1] * (p0 - p2) + duv02[:, 0:1] * (p1 - p2)) / det[:, None]
    along = np.where(uv_degenerate[:, None], 0.0, dpdv if _m("tangent_from_dpdv") else dpdu)
    ns, n = face.copy(), face.copy()
    ns_zero = np.zeros(len(tri), dtype=bool)
    if scene.get("normals") is not None:
        nsum = (w[:, :, None] * f64(scene["normals"])[idx]).sum(axis=1)
        ns_zero = has_n & (np.linalg.norm(nsum, axis=1) == 0)
        interp = nsum if _m("ns_unnormalised") else _unit_or_zero(nsum)
        ns = np.where((has_n & ~ns_zero)[:, None], interp, face)
        if not _m("n_not_faceforwarded"):
            n = np.where((dot(face, ns) < 0)[:, None], -face, face)
    s = along - ns * (dot(along, ns) / dot(ns, ns))[:, None]
    tangent_along_ns = ~uv_degenerate & (np.linalg.norm(s, axis=1) <= 1e-12 * np.linalg.norm(along, axis=1))
    s = _unit_or_zero(np.where(tangent_along_ns[:, None], 0.0, s))
    if _on("tangent_half_turn"):
        s = np.where(has_n[:, None], -s, s)
    return dict(p=p, uv=uv, n=n, ns=ns, s=s, face=face, wo=-d, has_normals=has_n, uv_degenerate=uv_degenerate, ns_zero=ns_zero, tangent_along_ns=tangent_along_ns,
                edge=np.abs(f64(b)).min(axis=1))


def _linear(m):
    m = f64(m).reshape(4, 4)
    return m[:3, :3], m[:3, 3]


def sphere_hits(scene, o, d):
    """Closest sphere hit: the world ray against the ellipsoid |W x + w| = r (W, w: world_to_object): the smallest positive root of
    the quadratic in t, which is the far root when the origin is inside.  -> (t, sphere, discriminant / b^2, origin inside)."""
    o, d = f64(o), f64(d)
    n = len(o)
    best_t, best_k, best_disc, best_in = np.full(n, np.inf), np.full(n, -1), np.full(n, np.inf), np.zeros(n, dtype=bool)
    for k, (_, w2o, r) in enumerate(scene.get("spheres", ())):
        lin, off = _linear(w2o)
        oo, dd = o @ lin.T + off, d @ lin.T
        a, b, c = dot(dd, dd), 2.0 * dot(oo, dd), dot(oo, oo) - float(r) ** 2
        disc = b * b - 4.0 * a * c
        with np.errstate(all="ignore"):
            root = np.sqrt(disc)
            t0, t1 = (-b - root) / (2.0 * a), (-b + root) / (2.0 * a)
            t = np.where(t0 > 0, t0, t1)
            ok = (disc >= 0) & (t > 0) & (t < best_t)
            rel = disc / (b * b)
        best_t, best_k = np.where(ok, t, best_t), np.where(ok, k, best_k)
        best_disc, best_in = np.where(ok, rel, best_disc), np.where(ok, c < 0, best_in)
    return best_t, best_k, best_disc, best_in


def sphere_surface(scene, o, d, sph, t):
    """p on the ellipsoid, its unit normal (the gradient of |W x + w|^2, W^T (W x + w): outward; inward when the transform swaps
    handedness, pbrt-v3 §3.1.1 / §2.8.3), (u, v) = (phi / 2 pi, (theta - pi) / (0 - pi)) of the object-space point as pbrt-v3 §3.2.3
    parametrises a full sphere (theta_min = pi at z = -r), and the unit tangent, the world image M (-y, x, 0) of the longitude
    direction.  axis = sin theta of the point: the conditioning of u and the tangent near the poles."""
    o, d = f64(o), f64(d)
    n = len(o)
    p = o + t[:, None] * d
    nrm, uv, s, wo, axis = np.zeros((n, 3)), np.zeros((n, 2)), np.zeros((n, 3)), -d.copy(), np.ones(n)
    for k, (o2w, w2o, r) in enumerate(scene.get("spheres", ())):
        rows = sph == k
        if not rows.any():
            continue
        m, _ = _linear(o2w)
        lin, off = _linear(w2o)
        x = p[rows] @ lin.T + off
        grad = x @ m.T if _m("sphere_normal_by_m") else x @ lin
        if np.linalg.det(m) < 0 and not _m("swaps_ignored"):
            grad = -grad
        nrm[rows] = normalize(grad)
        phi = np.arctan2(x[:, 1], x[:, 0])
        phi = np.where(phi < 0, phi + 2.0 * np.pi, phi)
        z = np.clip(x[:, 2] / float(r), -1.0, 1.0)
        uv[rows] = np.stack([phi / (2.0 * np.pi), (np.arccos(z) - np.pi) / (0.0 - np.pi)], axis=-1)
        s[rows] = _unit_or_zero(np.stack([-x[:, 1], x[:, 0], np.zeros(len(x))], axis=-1) @ m.T)
        axis[rows] = np.hypot(x[:, 0], x[:, 1]) / float(r)
        if _on("sphere_wo_transformed_again"):
            wo[rows] = normalize(-d[rows] @ m.T)
    return dict(p=p, uv=uv, n=nrm, ns=nrm.copy(), s=s, wo=wo, axis=axis)


def surface(scene, o, d):
    """The record of every ray's closest hit: hit, t, shape (source order, -1 on a miss), p, n, ns, s (unit tangent), uv, wo, the
    origin of a ray that leaves the hit along d (spawn_origin), and the per-row facts the exclusion predicates and branch counts
    read: is_sphere, edge (smallest barycentric), disc (sphere discriminant / b^2), inside, axis, has_normals, uv_degenerate,
    ns_zero, tangent_along_ns, face."""
    o, d = f64(o), f64(d)
    n = len(o)
    nt = len(scene["indices"])
    tt, tri, b = triangle_hits(scene, o, d) if nt else (np.full(n, np.inf), np.full(n, -1), np.zeros((n, 3)))
    ts, sph, disc, inside = sphere_hits(scene, o, d)
    is_sphere = ts < tt
    t = np.minimum(tt, ts)
    hit = np.isfinite(t)
    out = dict(hit=hit, t=t, is_sphere=is_sphere & hit, shape=np.where(hit, np.where(is_sphere, nt + sph, tri), -1), b=b, disc=disc, inside=inside & is_sphere)
    fields = dict(p=3, uv=2, n=3, ns=3, s=3, wo=3, face=3)
    for k, width in fields.items():
        out[k] = np.zeros((n, width))
    for k in ("has_normals", "uv_degenerate", "ns_zero", "tangent_along_ns"):
        out[k] = np.zeros(n, dtype=bool)
    out["edge"], out["axis"] = np.ones(n), np.ones(n)
    rows = hit & ~is_sphere
    if rows.any():
        r = triangle_surface(scene, o[rows], d[rows], tri[rows], b[rows])
        for k, v in r.items():
            out[k][rows] = v
    rows = hit & is_sphere
    if rows.any():
        r = sphere_surface(scene, o[rows], d[rows], sph[rows], t[rows])
        for k, v in r.items():
            out[k][rows] = v
        out["face"][rows] = r["n"]
    out["origin"] = spawn_origin(out["p"], out["n"], out["ns"], d)
    return out


def spawn_origin(p, n, ns, d):
    """Where a ray along d leaves the surface: the ledger's `fixed_offset`, p +- 1e-3 n with the geometric normal, on d's side."""
    if not _on("fixed_offset"):
        return f64(p)
    along = f64(ns) if _m("spawn_along_ns") else f64(n)
    return f64(p) + SPAWN_OFFSET * np.where(dot(d, along) > 0, 1.0, -1.0)[:, None] * along


def texel_lookup(tex, uv):
    """An image texture at uv — repeat, v flipped (images are stored top row first), point sampled: pbrt-v3 §10.4.1 (ImageTexture
    with the UV mapping) and §10.4.3 with a one-texel box: texel floor(s w) of s in [0, 1).  The ledger's `texel_index_half_texel`
    takes trunc(max(s w - 0.5, 0)) instead.  -> (rgb (n, 3), distance of every row to the nearest texel boundary, in texels)."""
    tex, uv = f64(tex), f64(uv)
    h, w = tex.shape[:2]
    s = uv - np.floor(uv)
    if not _m("texel_v_not_flipped"):
        s = np.stack([s[:, 0], 1.0 - s[:, 1]], axis=-1)
    x = s * np.array([w, h])
    if _on("texel_index_half_texel"):
        x = np.maximum(x - 0.5, 0.0)
    i = np.minimum(np.floor(x).astype(np.int64), np.array([w - 1, h - 1]))
    frac = x - np.floor(x)
    wrap = np.minimum(s, 1.0 - s) * np.array([w, h])  # the repeat's own seam
    boundary = np.minimum(np.minimum(frac, 1.0 - frac), wrap)
    if _on("texel_index_half_texel"):  # texel 0 starts at the seam and runs to s w = 1.5: no boundary at x = 0
        boundary = np.where(s * np.array([w, h]) < 1.0, wrap, boundary)
    return tex[i[:, 1], i[:, 0]], boundary.min(axis=1)
