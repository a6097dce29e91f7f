// yk_geom.h — device geometry: slab test, watertight triangle test, surface
// interaction reconstruction, light sampling.
#pragma once
#include "yk_device.h"

namespace yk {

// Per-ray constants of the watertight test (triangle.rs:59-78 recomputes them per
// triangle; they depend on the ray only, so the values are identical).
struct RayTri {
    int kx, ky, kz;
    float sx, sy, sz;
};
YK_HD RayTri ray_tri_setup(V3 d) {
    RayTri r;
    r.kz = max_dimension(vabs(d));
    r.kx = r.kz < 2 ? r.kz + 1 : 0;
    r.ky = r.kx < 2 ? r.kx + 1 : 0;
    float dx = comp(d, r.kx), dy = comp(d, r.ky), dz = comp(d, r.kz);
    r.sx = -dx / dz;
    r.sy = -dy / dz;
    r.sz = 1.0f / dz;
    return r;
}

struct TriHit {
    float t, b0, b1, b2;
};

// Triangle::intersect up to the barycentrics, shapes/triangle.rs:49-139
YK_HD bool tri_intersect(V3 o, const RayTri& rt, float t_max, V3 p0, V3 p1, V3 p2, TriHit& h) {
    V3 a = p0 - o, b = p1 - o, c = p2 - o;
    V3 p0t = V3{comp(a, rt.kx), comp(a, rt.ky), comp(a, rt.kz)};
    V3 p1t = V3{comp(b, rt.kx), comp(b, rt.ky), comp(b, rt.kz)};
    V3 p2t = V3{comp(c, rt.kx), comp(c, rt.ky), comp(c, rt.kz)};
    p0t.x = p0t.x + rt.sx * p0t.z;
    p0t.y = p0t.y + rt.sy * p0t.z;
    p1t.x = p1t.x + rt.sx * p1t.z;
    p1t.y = p1t.y + rt.sy * p1t.z;
    p2t.x = p2t.x + rt.sx * p2t.z;
    p2t.y = p2t.y + rt.sy * p2t.z;

    float e0 = p1t.x * p2t.y - p1t.y * p2t.x;
    float e1 = p2t.x * p0t.y - p2t.y * p0t.x;
    float e2 = p0t.x * p1t.y - p0t.y * p1t.x;
    if (e0 == 0.0f || e1 == 0.0f || e2 == 0.0f) {  // f64 fallback, triangle.rs:98-105
        double e0d = (double)p1t.x * (double)p2t.y - (double)p1t.y * (double)p2t.x;
        double e1d = (double)p2t.x * (double)p0t.y - (double)p2t.y * (double)p0t.x;
        double e2d = (double)p0t.x * (double)p1t.y - (double)p0t.y * (double)p1t.x;
        e0 = (float)e0d;
        e1 = (float)e1d;
        e2 = (float)e2d;
    }
    // the three rejection tests of triangle.rs:108-131 evaluated without
    // short-circuit branches (same predicates, straight-line v_cmp + s_and/s_or)
    const bool any_neg = (e0 < 0.0f) | (e1 < 0.0f) | (e2 < 0.0f);
    const bool any_pos = (e0 > 0.0f) | (e1 > 0.0f) | (e2 > 0.0f);
    float det = e0 + e1 + e2;
    float p0z = p0t.z * rt.sz;
    float p1z = p1t.z * rt.sz;
    float p2z = p2t.z * rt.sz;
    float t_scaled = e0 * p0z + e1 * p1z + e2 * p2z;
    const float td = t_max * det;
    const bool out_neg = (det < 0.0f) & ((t_scaled >= 0.0f) | (t_scaled < td));
    const bool out_pos = (det > 0.0f) & ((t_scaled <= 0.0f) | (t_scaled > td));
    if ((any_neg & any_pos) | (det == 0.0f) | out_neg | out_pos) return false;
    float inv_det = 1.0f / det;
    h.b0 = e0 * inv_det;
    h.b1 = e1 * inv_det;
    h.b2 = e2 * inv_det;
    h.t = t_scaled * inv_det;
    return true;
}

// Bounds3::slab_test + intersect, math/bounds.rs:176-215.  Returns the entry
// distance through tmin.  The NaN-dropping min/max (0*inf lanes) match Rust's.
YK_HD bool slab(V3 lo, V3 hi, V3 o, V3 inv, float t_max, float& tmin) {
    float t0x = (lo.x - o.x) * inv.x, t0y = (lo.y - o.y) * inv.y, t0z = (lo.z - o.z) * inv.z;
    float t1x = (hi.x - o.x) * inv.x, t1y = (hi.y - o.y) * inv.y, t1z = (hi.z - o.z) * inv.z;
    float nx = fmin_nan(t0x, t1x), ny = fmin_nan(t0y, t1y), nz = fmin_nan(t0z, t1z);
    float fx = fmax_nan(t0x, t1x), fy = fmax_nan(t0y, t1y), fz = fmax_nan(t0z, t1z);
    tmin = fmax_nan(fmax_nan(nx, fmax_nan(ny, nz)), 0.0f);
    float tmax = fmin_nan(fmin_nan(fx, fmin_nan(fy, fz)), t_max);
    return tmin <= tmax;
}

// A box whose test is DEFERRED (the far child: the reference tests it when it pops it, with the
// t_max of that moment) is screened with a relaxed bound when its parent is visited and checked
// exactly (entry distance <= t_max) when popped.  "t_max only shrinks" does not hold in the
// reference: the watertight triangle test accepts t_scaled <= t_max * det and returns
// t = t_scaled / det (triangle.rs:126-139, no conservative t-error test), so a tie hit among
// coplanar triangles can RAISE t_max by a few ulps, and a box culled at visit time by the
// exact bound would pass at pop time.
// LIMIT of the relaxed bound: it holds while t_max rises by no more than 2^-10 relative between the
// visit of a parent and the pop of its deferred child.  One tie hit lifts t_max by at most a few ulps
// (<= ~2^-21 relative), so the bound covers chains of roughly a thousand successive raises on one ray inside
// one such window — thousands of exactly coplanar, overlapping duplicates along a ray are outside it
// (the randomised parity runs, slabs of 160 coplanar triangles each, stay far inside).  Beyond the
// limit a deferred box could be culled that the reference would still enter; nothing else changes.
// (Tools-only builds set the factor to 1.0f to show that a scene exercises the case:
// tools/build_variant.sh exact -DYK_DEFERRED_BOUND_FACTOR=1.0f.)
#ifndef YK_DEFERRED_BOUND_FACTOR
#define YK_DEFERRED_BOUND_FACTOR 1.0009765625f  // 1 + 2^-10
#endif
YK_HD float deferred_t_max(float t_max) { return t_max * YK_DEFERRED_BOUND_FACTOR; }

// SurfaceInteraction after Triangle::intersect, triangle.rs:141-226 +
// interaction.rs:95-132 — the fields the integrator reads.
struct Surface {
    V3 p;       // si.p
    V3 n;       // si.n (geometric, face-forwarded to ns when normals exist)
    V3 ns;      // si.shading.n
    V3 dpdus;   // si.shading.dpdu
    V3 wo;      // si.wo (== -ray.d for triangles; re-normalised through the transform for spheres)
    int material;
    int area_light;
    float u, v;  // si.uv — read only by image textures
};

YK_HD V3 ld3(const float* a, uint32_t i) { return V3{a[3 * i], a[3 * i + 1], a[3 * i + 2]}; }

// Sphere::intersect up to the hit distance, shapes/sphere.rs:38-77.  (orx,ory,orz)/(drx..)
// receive the object-space ray for the caller that goes on to build the surface.
YK_HD bool sphere_hit_t(const DevSphere& sp, V3 o, V3 d, float t_max, float& t_out, V3& ro, V3& rd) {
    ro = xf_point(sp.w2o, o);
    rd = xf_vector(sp.w2o, d);
    float a = rd.x * rd.x + rd.y * rd.y + rd.z * rd.z;
    float b = 2.0f * (rd.x * ro.x + rd.y * ro.y + rd.z * ro.z);
    float c = ro.x * ro.x + ro.y * ro.y + ro.z * ro.z - sp.radius * sp.radius;
    float discrim = b * b - 4.0f * a * c;
    if (discrim < 0.0f) return false;
    float rdisc = sqrtf(discrim);
    float q = b < 0.0f ? -0.5f * (b - rdisc) : -0.5f * (b + rdisc);
    float t0 = q / a;
    float t1 = c / q;
    if (t0 > t1) {
        float tmp = t0;
        t0 = t1;
        t1 = tmp;
    }
    if (t0 > t_max || t1 <= 0.0f) return false;
    float t = t0;
    if (t <= 0.0f) {
        t = t1;
        if (t > t_max) return false;
    }
    t_out = t;
    return true;
}

// Rest of Sphere::intersect (sphere.rs:79-116) + Transform * SurfaceInteraction
// (interaction.rs:141-164): the world-space surface the integrator sees.
YK_HD Surface make_surface_sphere(const DevSphere& sp, V3 ro, V3 rd, float t, V3 world_d, bool want_uv) {
    V3 p = ro + rd * t;  // Ray::point
    p = p * (sp.radius / length(p - V3{0.0f, 0.0f, 0.0f}));
    if (p.x == 0.0f && p.y == 0.0f) p.x = 1e-5f * sp.radius;
    const float phi_max = 2.0f * YK_PI, theta_min = YK_PI, theta_max = 0.0f;
    float theta = det_acosf(rclamp(p.z / sp.radius, -1.0f, 1.0f));
    float su = 0.0f, sv = 0.0f;
    if (want_uv) {  // sphere.rs:95-103; only image textures read the uv
        float phi = det_atan2f(p.y, p.x);
        if (phi < 0.0f) phi += 2.0f * YK_PI;
        su = phi / phi_max;
        sv = (theta - theta_min) / (theta_max - theta_min);
    }
    float z_radius = sqrtf(p.x * p.x + p.y * p.y);
    float inv_z_radius = 1.0f / z_radius;
    float cos_phi = p.x * inv_z_radius;
    float sin_phi = p.y * inv_z_radius;
    V3 dpdu = V3{-phi_max * p.y, phi_max * p.x, 0.0f};
    V3 dpdv = V3{p.z * cos_phi, p.z * sin_phi, -sp.radius * det_sinf(theta)} * (theta_max - theta_min);
    // SurfaceInteraction::new in object space
    V3 n_obj = normalize(cross(dpdu, dpdv));
    if (sp.swaps_handedness) n_obj = -n_obj;
    // &object_to_world * si
    const float* m = sp.o2w;
    const float* mi = sp.w2o;  // inverse of object_to_world
    V3 n = normalize(xf_normal(mi, n_obj));
    V3 sn = normalize(xf_normal(mi, n_obj));
    sn = faceforward_n(sn, n);
    Surface s;
    s.p = xf_point(m, p);
    s.n = n;
    s.dpdus = xf_vector(m, dpdu);
    s.wo = normalize(xf_vector(m, -world_d));
    s.ns = faceforward_n(sn, s.n);
    s.material = sp.material;
    s.area_light = -1;
    s.u = su;
    s.v = sv;
    return s;
}

// SurfaceInteraction of a triangle hit from its vertices (world space), the per-vertex uvs and normals of the mesh
// (read only when the mesh flags say they exist) and the mesh flags: triangle.rs:141-226 + interaction.rs:95-132
struct TriAttr {
    float u0x, u0y, u1x, u1y, u2x, u2y;
    V3 n0, n1, n2;
};
YK_HD Surface make_surface_vals(V3 p0, V3 p1, V3 p2, const TriAttr& at, uint32_t mflags, const TriHit& h) {
    float u0x = 0.0f, u0y = 0.0f, u1x = 1.0f, u1y = 0.0f, u2x = 1.0f, u2y = 1.0f;  // triangle.rs:143-149
    if (mflags & YK_MESH_UVS) {
        u0x = at.u0x; u0y = at.u0y;
        u1x = at.u1x; u1y = at.u1y;
        u2x = at.u2x; u2y = at.u2y;
    }
    float duv02x = u0x - u2x, duv02y = u0y - u2y;
    float duv12x = u1x - u2x, duv12y = u1y - u2y;
    V3 dp02 = p0 - p2, dp12 = p1 - p2;
    float uv_det = duv02x * duv12y - duv02y * duv12x;
    V3 dpdu, dpdv;
    if (uv_det == 0.0f) {
        V3 nn = normalize(cross(p2 - p0, p1 - p0));
        coordinate_system(nn, dpdu, dpdv);
    } else {
        float inv_uv_det = 1.0f / uv_det;
        dpdu = (dp02 * duv12y - dp12 * duv02y) * inv_uv_det;
        dpdv = ((-dp02) * duv12x + dp12 * duv02x) * inv_uv_det;
    }
    (void)dpdv;
    Surface s;
    s.p = p0 * h.b0 + p1 * h.b1 + p2 * h.b2;
    s.u = u0x * h.b0 + u1x * h.b1 + u2x * h.b2;  // uv_hit, triangle.rs:176
    s.v = u0y * h.b0 + u1y * h.b1 + u2y * h.b2;
    V3 n = normalize(cross(dp02, dp12));
    if (mflags & YK_MESH_SWAPS) n = -n;
    s.n = n;
    s.ns = n;
    s.dpdus = dpdu;
    if (mflags & YK_MESH_NORMALS) {
        V3 n0 = at.n0, n1 = at.n1, n2 = at.n2;
        V3 ns;
        V3 nn = normalize(n0 * h.b0 + n1 * h.b1 + n2 * h.b2);
        if (len_sqr(nn) > 0.0f)
            ns = normalize(nn);  // normalised twice, triangle.rs:203-205
        else
            ns = s.n;
        V3 ss = normalize(dpdu);
        V3 ts = cross(ss, ns);
        if (len_sqr(ts) > 0.0f) {
            ts = normalize(ts);
            ss = cross(ts, ns);
        } else {
            coordinate_system(ns, ss, ts);
        }
        // set_shading_geometry, interaction.rs:126-132
        s.ns = normalize(cross(ss, ts));
        s.n = faceforward_n(s.n, s.ns);
        s.dpdus = ss;
    }
    s.material = 0;
    s.area_light = -1;
    return s;
}

// the same through the vertex indices (per-vertex arrays of the scene description)
YK_HD Surface make_surface_core(const DevScene& sc, V3 p0, V3 p1, V3 p2, uint32_t i0, uint32_t i1, uint32_t i2, uint32_t mflags, const TriHit& h) {
    TriAttr at;
    at.u0x = at.u0y = at.u1x = at.u1y = at.u2x = at.u2y = 0.0f;
    at.n0 = at.n1 = at.n2 = V3{0.0f, 0.0f, 0.0f};
    if (mflags & YK_MESH_UVS) {
        at.u0x = sc.uvs[2 * i0]; at.u0y = sc.uvs[2 * i0 + 1];
        at.u1x = sc.uvs[2 * i1]; at.u1y = sc.uvs[2 * i1 + 1];
        at.u2x = sc.uvs[2 * i2]; at.u2y = sc.uvs[2 * i2 + 1];
    }
    if (mflags & YK_MESH_NORMALS) {
        at.n0 = ld3(sc.normals, i0);
        at.n1 = ld3(sc.normals, i1);
        at.n2 = ld3(sc.normals, i2);
    }
    return make_surface_vals(p0, p1, p2, at, mflags, h);
}

YK_HD Surface make_surface(const DevScene& sc, uint32_t tri, const TriHit& h) {
    uint32_t i0 = sc.indices[3 * tri], i1 = sc.indices[3 * tri + 1], i2 = sc.indices[3 * tri + 2];
    Surface s = make_surface_core(sc, ld3(sc.points, i0), ld3(sc.points, i1), ld3(sc.points, i2), i0, i1, i2, sc.mesh_flags[sc.tri_mesh[tri]], h);
    s.material = sc.tri_material[tri];
    s.area_light = sc.tri_area_light[tri];
    return s;
}

// The accepted intersection is recomputed from (ray, shape): same operands, same
// arithmetic as inside the traversal -> same t and barycentrics.
YK_HD Surface hit_surface(const DevScene& sc, uint32_t shape, V3 o, V3 d) {
    if (shape >= sc.n_triangles) {
        const DevSphere& sp = sc.spheres[shape - sc.n_triangles];
        V3 ro, rd;
        float t = 0.0f;
        sphere_hit_t(sp, o, d, __builtin_inff(), t, ro, rd);
        return make_surface_sphere(sp, ro, rd, t, d, sc.texels != nullptr);
    }
    uint32_t i0 = sc.indices[3 * shape], i1 = sc.indices[3 * shape + 1], i2 = sc.indices[3 * shape + 2];
    RayTri rt = ray_tri_setup(d);
    TriHit th = TriHit{0.0f, 0.0f, 0.0f, 0.0f};
    tri_intersect(o, rt, __builtin_inff(), ld3(sc.points, i0), ld3(sc.points, i1), ld3(sc.points, i2), th);
    Surface s = make_surface(sc, shape, th);
    s.wo = -d;
    return s;
}

// Same, addressed by the primitive's slot in leaf order (what the production traversal kernels
// report): the 48-byte traversal record holds the vertices, the area light and the source
// shape, DevScene::prim_shade the vertex indices, material and mesh flags — one dependent
// fetch less than going through indices -> points and tri_mesh -> mesh_flags.
// `want_uv`: also compute a sphere's uv (sphere.rs:95-103); the shading path needs it only for image textures.
// `t_out` (may be NULL): receives the hit distance, Hit.t (the guide pass, k_guides).
// `id_out` (may be NULL): receives the surface id of the hit (k_guides_ids): the source shape and the TriHit's b0, b1, b2 as
// bits — the operands Surface::p is combined from; a sphere has no barycentrics and reports zeros.
YK_HD Surface hit_surface_prim(const DevScene& sc, uint32_t prim, V3 o, V3 d, bool want_uv, float* t_out, uint4* id_out) {
    const float4 v0 = sc.tris[3 * prim], v1 = sc.tris[3 * prim + 1], v2 = sc.tris[3 * prim + 2];
    const uint4 ps = sc.prim_shade[prim];
    const uint32_t src = __float_as_uint(v1.w);
    if (__float_as_uint(v2.w) & YK_PRIM_SPHERE) {
        const DevSphere& sp = sc.spheres[src - sc.n_triangles];
        V3 ro, rd;
        float t = 0.0f;
        sphere_hit_t(sp, o, d, __builtin_inff(), t, ro, rd);
        if (t_out) *t_out = t;
        if (id_out) *id_out = make_uint4(src, 0u, 0u, 0u);
        return make_surface_sphere(sp, ro, rd, t, d, want_uv);
    }
    // per-vertex normals and uvs of the primitive, copied into leaf order at scene creation: their address depends on the
    // hit alone, so they are in flight together with the vertices instead of waiting for the vertex indices (k_shade
    // of an incoherent bounce is a chain of dependent gathers at three waves per SIMD; this removes one link)
    TriAttr at;
    at.u0x = at.u0y = at.u1x = at.u1y = at.u2x = at.u2y = 0.0f;
    at.n0 = at.n1 = at.n2 = V3{0.0f, 0.0f, 0.0f};
    if (sc.prim_attr && (ps.w & (YK_MESH_NORMALS | YK_MESH_UVS))) {
        const float4 a0 = sc.prim_attr[4 * (size_t)prim], a1 = sc.prim_attr[4 * (size_t)prim + 1], a2 = sc.prim_attr[4 * (size_t)prim + 2], a3 = sc.prim_attr[4 * (size_t)prim + 3];
        at.n0 = V3{a0.x, a0.y, a0.z};
        at.n1 = V3{a1.x, a1.y, a1.z};
        at.n2 = V3{a2.x, a2.y, a2.z};
        at.u0x = a0.w; at.u0y = a1.w;
        at.u1x = a2.w; at.u1y = a3.x;
        at.u2x = a3.y; at.u2y = a3.z;
    }
    RayTri rt = ray_tri_setup(d);
    TriHit th = TriHit{0.0f, 0.0f, 0.0f, 0.0f};
    const V3 p0 = V3{v0.x, v0.y, v0.z}, p1 = V3{v1.x, v1.y, v1.z}, p2 = V3{v2.x, v2.y, v2.z};
    tri_intersect(o, rt, __builtin_inff(), p0, p1, p2, th);
    if (t_out) *t_out = th.t;
    if (id_out) *id_out = make_uint4(src, __float_as_uint(th.b0), __float_as_uint(th.b1), __float_as_uint(th.b2));
    Surface s = sc.prim_attr ? make_surface_vals(p0, p1, p2, at, ps.w & 7u, th) : make_surface_core(sc, p0, p1, p2, ps.x, ps.y, ps.z, ps.w & 7u, th);
    s.material = (int)(ps.w >> 6);
    s.area_light = (int)__float_as_uint(v0.w);
    s.wo = -d;
    return s;
}
YK_HD Surface hit_surface_prim(const DevScene& sc, uint32_t prim, V3 o, V3 d, bool want_uv, float* t_out) { return hit_surface_prim(sc, prim, o, d, want_uv, t_out, nullptr); }
YK_HD Surface hit_surface_prim(const DevScene& sc, uint32_t prim, V3 o, V3 d, bool want_uv) { return hit_surface_prim(sc, prim, o, d, want_uv, nullptr, nullptr); }
YK_HD Surface hit_surface_prim(const DevScene& sc, uint32_t prim, V3 o, V3 d) { return hit_surface_prim(sc, prim, o, d, sc.texels != nullptr, nullptr, nullptr); }

// ImageTexture::evaluate, textures/image_texture.rs:81-111: repeat, flip v, point sample.
// `as usize` saturates (NaN and negatives -> 0); the index cannot leave the image.
YK_HD RGB texture_eval(const DevScene& sc, unsigned tex, float u, float v) {
    const uint4 info = sc.tex_info[tex];
    float sx = u - truncf(u);  // f32::fract
    if (sx < 0.0f) sx = 1.0f + sx;
    float sy = v - truncf(v);
    if (sy < 0.0f) sy = 1.0f + sy;
    sy = 1.0f - sy;
    float fx = sx * (float)info.y - 0.5f;
    float fy = sy * (float)info.z - 0.5f;
    unsigned ix = fx > 0.0f ? (unsigned)fminf(fx, 4.0e9f) : 0u;
    unsigned iy = fy > 0.0f ? (unsigned)fminf(fy, 4.0e9f) : 0u;
    size_t idx = (size_t)iy * info.y + ix;
    const size_t last = (size_t)info.y * info.z - 1;
    if (idx > last) idx = last;  // unreachable for finite uv (the reference would panic)
    float4 t = sc.texels[(size_t)info.x + idx];
    return RGB{t.x, t.y, t.z};
}

// Interaction::spawn_ray, interaction.rs:27-40
YK_HD V3 spawn_origin(V3 p, V3 n, V3 d) {
    V3 offset = n * 0.001f;
    return dot(d, n) > 0.0f ? p + offset : p - offset;
}

struct LightSample {
    V3 l;
    RGB li;
    float pdf;
    bool has_vis;
    V3 p1;           // VisibilityTester.p1.p
    int area_light;  // identity of the sampled area light or -1
};

// Whether sample_light reads (ux, uy) for a light of this kind: the point, spot and distant lights have one position or
// direction to offer.  sample_light lets the sample in through this predicate alone, so a caller that asks it and skips the
// draw (sampler_skip_2d) sees what every caller sees.
YK_HD bool light_reads_sample(uint32_t kind) { return kind == YK_LIGHT_RECT; }

// Light::sample_li — point_light.rs:27-50, spot_light.rs:38-80,
// distant_light.rs:24-43, rectangular_light.rs:46-71
YK_HD LightSample sample_light(const DevLight& L, int index, V3 sp, float ux, float uy) {
    if (!light_reads_sample(L.kind)) ux = uy = 0.0f;
    LightSample s;
    s.has_vis = true;
    s.area_light = -1;
    s.pdf = 1.0f;
    V3 lp = V3{L.p[0], L.p[1], L.p[2]};
    RGB li = RGB{L.i[0], L.i[1], L.i[2]};
    if (L.kind == YK_LIGHT_POINT) {
        V3 to_light = lp - sp;
        float dist_sqr = len_sqr(to_light);
        s.li = li / dist_sqr;
        float dist = sqrtf(dist_sqr);
        s.l = to_light / dist;
        s.p1 = lp;
    } else if (L.kind == YK_LIGHT_SPOT) {
        V3 to_light = lp - sp;
        float dist_sqr = len_sqr(to_light);
        float dist = sqrtf(dist_sqr);
        s.l = to_light / dist;
        V3 dir_local = normalize(xf_vector(L.w2l, -s.l));
        float ct = dir_local.z;
        float falloff;
        if (ct < L.cos_total_width)
            falloff = 0.0f;
        else if (ct > L.cos_falloff_start)
            falloff = 1.0f;
        else {
            float delta = (ct - L.cos_total_width) / (L.cos_falloff_start - L.cos_total_width);
            falloff = (delta * delta) * (delta * delta);
        }
        s.li = li * falloff / dist_sqr;
        if (is_black(s.li)) s.has_vis = false;
        s.p1 = lp;
    } else if (L.kind == YK_LIGHT_DISTANT) {
        s.li = li;
        s.l = lp;  // w
        s.p1 = sp + lp * 10000.0f;
    } else {
        V3 p = xf_point(L.s2w, V3{ux, 0.0f, uy});
        V3 n = V3{L.n[0], L.n[1], L.n[2]};
        V3 wi = normalize(p - sp);
        float ndw = dot_nv(n, -wi);
        s.li = ndw > 0.0f ? li : RGB{0.0f, 0.0f, 0.0f};
        s.p1 = p;
        s.area_light = index;
        s.pdf = len_sqr(sp - p) / (fabsf(ndw) * L.area);
        s.l = wi;
    }
    return s;
}

}  // namespace yk
