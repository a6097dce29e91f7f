// yk_motion.h — the film across moves of the GEOMETRY: where a pixel's surface point stood before yk_scene_update moved the
// scene's vertices.  The guide pass writes a surface id beside each guide (yk_render_guides_ids: the source shape and the
// hit's barycentrics); "motion" turns the id and the PREVIOUS vertex array into the previous position of the same surface
// point; yk_history_reproject_moved (yk_temporal.h) projects that position, not the current one, into the previous camera.
//
// The reference clears its film when anything moves, so this file is the rule.  Its arithmetic is yk_denoise.h's and
// yk_temporal.h's:
//   - IEEE-754 binary32, round to nearest, every operation separate (-ffp-contract=off);
//   - a NaN that an operation PRODUCES is 0x7fc00000 (dn_canon); a value that is only copied keeps its bits.
// One text, two instances: the host instance (no context) and k_motion of yk_motion.hip call mo_pixel and agree bit for bit.
//
// What moves: triangles, through their vertices (yk_scene_update), and spheres, through their records
// (yk_scene_apply_edit): a sphere's point keeps its place in the sphere's object space, scaled with the radius.  A call
// without a previous sphere table (MoNoSpheres) takes the spheres as unmoved: a sphere's previous position is its current
// one.  Lights carry no film.
#pragma once
#include "../../include/yuki_hip.h"
#include "yk_denoise.h"
#include "yk_math.h"

#include <type_traits>

namespace yk {

// Everything about a call that does not depend on the pixel.  n_shapes = n_triangles + n_spheres.
struct MoParams {
    uint32_t res_x, res_y;
    uint32_t n_triangles, n_shapes;
};

// What the sphere case reads of sphere k: world_to_object and the radius of the scene's CURRENT table, object_to_world and
// the radius of the table the caller kept from BEFORE the edit.
struct MoSphere {
    float w2o[16], o2w_prev[16];
    float radius, radius_prev;
};
// The call has no previous sphere table: nothing of a sphere is read.
struct MoNoSpheres {};

// Motion, one pixel with surface id (shape, b0, b1, b2) and guide (hit, p).  index(k) reads word k of the scene's index
// array (3 words a triangle), point(v) the three floats of vertex v of the previous vertex array, sphere(k) the MoSphere
// of sphere k.  out = (p_prev, known), the cases in this order:
//   miss          shape == YK_SURFACE_NONE or hit == 0:   the all-zero record;
//   out of range  shape >= n_shapes:                       the all-zero record — the index is never followed: this test
//                                                          stands before the first dependent load;
//   sphere        shape >= n_triangles:                    without a previous table (p as bits, 1); with one,
//                                                          q = xf_point(w2o, p), q = q * (radius_prev / radius) unless the
//                                                          two radii have equal bits, p_prev = xf_point(o2w_prev, q), each
//                                                          component through dn_canon; known = 1;
//   triangle      i0, i1, i2 = index(3 shape ..),          p_prev = P'[i0]*b0 + P'[i1]*b1 + P'[i2]*b2 with the V3 operators:
//                                                          the expression and order of Surface::p (make_surface_vals), each
//                                                          component through dn_canon; known = 1.
// The gather is two hops (id -> three indices -> nine floats).  The three index loads are requested together, then the
// three point loads; none stands under a per-case branch: every lane that is not a triangle asks for triangle 0 instead
// and drops what comes back, as tp_reproject_pixel does for taps outside the film (why).  A scene
// without triangles has no triangle 0: then nothing is loaded (n_triangles is the same for every lane).  The sphere record
// is read the same way: every lane asks for one, sphere 0 where the lane is no sphere, and a scene without spheres reads none.
template <class Index, class Point, class Sphere>
YK_HD void mo_pixel(const MoParams& a, uint32_t shape, float b0, float b1, float b2, float hit, const float* p, const Index& index, const Point& point, const Sphere& sphere, float* out) {
    const bool live = shape != YK_SURFACE_NONE && hit != 0.0f && shape < a.n_shapes;
    const bool tri = live && shape < a.n_triangles;
    V3 q = V3{0.0f, 0.0f, 0.0f};
    if (a.n_triangles != 0u) {
        const size_t t = tri ? (size_t)shape : (size_t)0;
        const uint32_t i0 = index(3 * t), i1 = index(3 * t + 1), i2 = index(3 * t + 2);
        const V3 p0 = point(i0), p1 = point(i1), p2 = point(i2);
        q = p0 * b0 + p1 * b1 + p2 * b2;
    }
    if constexpr (std::is_same<Sphere, MoNoSpheres>::value) {
        out[0] = tri ? dn_canon(q.x) : (live ? p[0] : 0.0f);
        out[1] = tri ? dn_canon(q.y) : (live ? p[1] : 0.0f);
        out[2] = tri ? dn_canon(q.z) : (live ? p[2] : 0.0f);
    } else {
        const bool sph = live && !tri;
        V3 r = V3{0.0f, 0.0f, 0.0f};
        if (a.n_shapes != a.n_triangles) {
            const MoSphere rec = sphere(sph ? shape - a.n_triangles : 0u);
            V3 o = xf_point(rec.w2o, V3{p[0], p[1], p[2]});
            if (__builtin_bit_cast(uint32_t, rec.radius) != __builtin_bit_cast(uint32_t, rec.radius_prev)) o = o * (rec.radius_prev / rec.radius);
            r = xf_point(rec.o2w_prev, o);
        }
        out[0] = tri ? dn_canon(q.x) : (sph ? dn_canon(r.x) : 0.0f);
        out[1] = tri ? dn_canon(q.y) : (sph ? dn_canon(r.y) : 0.0f);
        out[2] = tri ? dn_canon(q.z) : (sph ? dn_canon(r.z) : 0.0f);
    }
    out[3] = live ? 1.0f : 0.0f;
}

}  // namespace yk
