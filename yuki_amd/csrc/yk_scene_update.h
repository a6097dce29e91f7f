// yk_scene_update.h — the refit rule of yk_scene_update / yk_bvh_refit, written once for the gfx950 kernels of
// yk_scene_update.hip and for the host route (ibid., yk_bvh_refit).
//
// The rule.  A refit keeps the tree's topology and the leaf order and recomputes what depends on coordinates:
//   * a leaf's box is folded from the default bounds, left to right in leaf order, with rmin / rmax — exactly as the
//     builder folds a leaf (yk_bvh_build.h: the fold's order decides the sign of a zero).  A triangle contributes
//     Triangle::world_bound of the new points (inp::tri_bound), a sphere Sphere::world_bound of its record (inp::sphere_bound:
//     as at creation, or as the last yk_scene_apply_edit left it);
//   * an interior node's box is lv::interior_bounds, in child order, once both children are done;
//   * the records follow from the refitted tree through the layout's own code (yk_scene_layout.h / layout_records_host).
// Words 6 and 7 of a node (links, slot, count, axis, leaf flag) are never written.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "yk_bvh_build.h"
#include "yk_scene_input.h"
#include "yk_scene_layout.h"

namespace yk {
namespace upd {

// NaN or infinite: all exponent bits set
YK_HD bool not_finite_bits(uint32_t u) { return (u & 0x7f800000u) == 0x7f800000u; }

// Where a leaf's shapes get their bounds from: a table of six floats per source shape (the host route, yk_bvh_refit) ...
struct TableBound {
    const float* table;
    YK_HD void operator()(uint32_t src, float (&out)[6]) const {
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = table[6 * (size_t)src + k];
    }
};
// ... or the geometry itself (the device route): three 12-byte gathers through the indices, a sphere from its table.
// A source index outside the scene contributes nothing (it cannot happen: the order is a permutation of the shapes).
struct GeometryBound {
    const float* points;
    const uint32_t* indices;
    const float* sphere_bounds;
    uint32_t n_triangles, n_shapes;
    YK_HD void operator()(uint32_t src, float (&out)[6]) const {
        if (src < n_triangles) {
            (void)inp::tri_bound(points, indices, src, out);
        } else if (src < n_shapes) {
            TableBound{sphere_bounds}(src - n_triangles, out);
        } else {
            const lv::Box e = lv::box_empty();
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                out[k] = e.lo[k];
                out[3 + k] = e.hi[k];
            }
        }
    }
};

// The leaf rule: node i (a leaf) gets the fold of its shapes' bounds; its box is written as two 16-byte words that
// carry words 6 and 7 through unchanged.
template <class Bound> YK_HD void refit_leaf(uint32_t* nodes, uint32_t i, const uint32_t* order, const Bound& bound) {
    uint4* w = reinterpret_cast<uint4*>(nodes + 8 * (size_t)i);
    const uint4 hi = w[1];
    const uint32_t first = hi.z, count = hi.w & 0xffffu;
    lv::Box b = lv::box_empty();
    for (uint32_t p = first; p < first + count; ++p) {
        float sb[6];
        bound(order[p], sb);
        lv::box_add(b, sb, sb + 3);
    }
    w[0] = make_uint4(lv::f2u(b.lo[0]), lv::f2u(b.lo[1]), lv::f2u(b.lo[2]), lv::f2u(b.hi[0]));
    w[1] = make_uint4(lv::f2u(b.hi[1]), lv::f2u(b.hi[2]), hi.z, hi.w);
}

}  // namespace upd
}  // namespace yk
