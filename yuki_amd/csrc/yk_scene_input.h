// yk_scene_input.h — the front of scene preparation for geometry that is already in HBM (yk_scene_create_device):
// what check_description and shape_bounds (yk_scene.cpp) do per triangle and per shape, written as functions of one
// element for the gfx950 kernels of yk_scene_input.hip.  The host loops stay the yardstick; the expressions below
// restate them.
//
// Order of the checks.  The host loop walks the triangles in order and, per triangle, tests its three vertex indices,
// its mesh, its material and the range of its area light; the first failure ends it.  That is the minimum of
// 4 * triangle + check over all failures (tri_check).  The area-light rule (-1, or a rectangular light) is a second
// pass on the host, reached only when the first found nothing: it is recorded in a word of its own and read only
// when the first word is clear.  A lane looks its light's kind up only after its own range check has passed.
//
// Non-finite coordinates.  rmin / rmax drop a NaN operand, so a triangle with one NaN coordinate has a finite bound and
// the builder's own test (k_prepare: bounds and centroids) would not see it.  The input stage does: tri_bound says
// whether all nine coordinates it gathered are finite, and geometry that fails takes the host path with reason
// YK_BVH_REASON_NON_FINITE — the same tree, built by the host recursion.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/yuki_hip.h"
#include "yk_math.h"

namespace yk {
namespace inp {

struct Geometry {  // the per-triangle arrays of a yk_scene_desc (device pointers) and the counts they index into
    const uint32_t* indices;
    const uint32_t* tri_mesh;        // may be NULL
    const int32_t* tri_material;     // may be NULL (the host tables' checks refuse that before any kernel runs)
    const int32_t* tri_area_light;   // may be NULL
    uint32_t n_triangles, n_vertices, n_meshes, n_materials, n_lights;
};

enum { kCheckVertex = 0, kCheckMesh = 1, kCheckMaterial = 2, kCheckLight = 3, kCheckNone = 4 };

// What the caller reads back: the two check words and the permutation flag.
struct CheckWords {
    unsigned long long first;   // min over failing triangles of 4 * i + check; all ones = none
    unsigned long long light;   // min of 4 * i over triangles that break the area-light rule; all ones = none
    uint32_t order_bad;         // shape_order is not a permutation
    uint32_t non_finite;        // k_shape_bounds: a triangle has a coordinate that is NaN or infinite
    uint32_t pad[2];
};
const unsigned long long kNoFailure = ~0ull;

// check_description's loop body for triangle i: the first check that fails, in the host's order
YK_HD uint32_t tri_check(const Geometry& g, uint32_t i) {
    const uint32_t* v = g.indices + 3 * (size_t)i;
    const uint32_t v0 = v[0], v1 = v[1], v2 = v[2];
    if ((v0 >= g.n_vertices) | (v1 >= g.n_vertices) | (v2 >= g.n_vertices)) return kCheckVertex;  // one 12-byte load, no branches between
    if (g.tri_mesh && g.tri_mesh[i] >= g.n_meshes) return kCheckMesh;
    if (g.tri_material) {
        const int32_t m = g.tri_material[i];
        if (m < 0 || (uint32_t)m >= g.n_materials) return kCheckMaterial;
    }
    if (g.tri_area_light && g.tri_area_light[i] >= (int32_t)g.n_lights) return kCheckLight;
    return kCheckNone;
}
// Triangle.area_light (triangle.rs:22): -1 or a rectangular light.  Call only where tri_check passed.
YK_HD bool area_light_ok(const Geometry& g, const uint8_t* light_kind, uint32_t i) {
    if (!g.tri_area_light) return true;
    const int32_t al = g.tri_area_light[i];
    return al == -1 || (al >= 0 && light_kind[al] == (uint8_t)YK_LIGHT_RECT);
}

// Triangle::world_bound (triangle.rs:229-235): out = {min.xyz, max.xyz}.  Returns whether all nine coordinates are finite.
YK_HD bool tri_bound(const float* points, const uint32_t* indices, uint32_t i, float (&out)[6]) {
    const uint32_t* v = indices + 3 * (size_t)i;
    const float* p0 = points + 3 * (size_t)v[0];
    const float* p1 = points + 3 * (size_t)v[1];
    const float* p2 = points + 3 * (size_t)v[2];
    const float a[3] = {p0[0], p0[1], p0[2]}, b[3] = {p1[0], p1[1], p1[2]}, c[3] = {p2[0], p2[1], p2[2]};  // three 12-byte gathers
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out[k] = rmin(rmin(a[k], b[k]), c[k]);
        out[3 + k] = rmax(rmax(a[k], b[k]), c[k]);
    }
    const float big = 3.40282347e+38f;  // a NaN fails every comparison
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) finite = finite && __builtin_fabsf(a[k]) <= big && __builtin_fabsf(b[k]) <= big && __builtin_fabsf(c[k]) <= big;
    return finite;
}

// Sphere::world_bound (sphere.rs:121-123): the object-space box [-r, r]^3 through object_to_world — its eight corners in
// the order of transform.rs:194-206, each through xf_point, folded with rmin / rmax from -+FLT_MAX.  out = {min.xyz, max.xyz}.
// One text for creation (yk_scene.cpp), the host route of an edit and k_spheres_in (yk_scene_edit.hip).
YK_HD void sphere_bound(const float* object_to_world, float radius, float (&out)[6]) {
    const float big = 3.40282347e+38f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out[k] = big;
        out[3 + k] = -big;
    }
    // corner c takes the box's maximum on an axis where its bit is set: (0,0,0) (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1)
    const unsigned x_hi = 0xb2u, y_hi = 0xd4u, z_hi = 0xe8u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const V3 q = xf_point(object_to_world, V3{(x_hi >> c) & 1u ? radius : -radius, (y_hi >> c) & 1u ? radius : -radius, (z_hi >> c) & 1u ? radius : -radius});
        const float qq[3] = {q.x, q.y, q.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out[k] = rmin(out[k], qq[k]);
            out[3 + k] = rmax(out[3 + k], qq[k]);
        }
    }
}
// Transform::swaps_handedness (transform.rs:85-91) of a sphere's object_to_world: the sign of the upper 3 x 3 determinant
YK_HD bool swaps_handedness(const float* m) {
    const float det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
    return det < 0.0f;
}

}  // namespace inp
}  // namespace yk
