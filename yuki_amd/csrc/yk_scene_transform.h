// yk_scene_transform.h — the rule of yk_scene_transform: a scene's meshes placed by one matrix each, relative to the rest
// pose.  The reference has no animation, so this file is the rule, as yk_motion.h is; what it is made of is the reference's:
// xf_point / xf_normal (yk_math.h) are Transform * Point3 and Transform * Normal as Mesh::new applies them
// (shapes/mesh.rs:27-33), inp::swaps_handedness is Transform::swaps_handedness.  One text, two instances — the host route and
// the kernels of yk_scene_transform.hip — equal bit for bit: binary32, every operation separate (-ffp-contract=off); the
// tree cost in binary64.
//
// The table vertex -> mesh.  Two words a vertex, (min, max) over the meshes of the triangles that index it, starting from
// (XF_NO_MESH, 0): integer minimum and maximum do not depend on the order, so the device's atomics give the host loop's
// words.  min == XF_NO_MESH: no triangle indexes the vertex, it belongs to no mesh and keeps its rest bits; min != max: the
// vertex is shared by two meshes and every transform of the scene is refused; otherwise the vertex's mesh is min.
//
// The kind of a mesh's record (mesh_kind): XF_MOVED unless rest_to_world equals the identity entry by entry with == (as
// Transform::is_identity does: -0 counts as 0, a NaN makes it differ); XF_FLIPS beside it when rest_to_world swaps
// handedness.  A record that is not moved gives the rest pose's BITS and its world_to_rest is never read: computed through
// the identity, -0.0 would come out as +0.0 (-0 * 1 + 0 + 0 + 0) and "nothing moved" would not be byte-exact.
//
// Refusals, as bits of one flag word; where several are set the message is the LOWEST bit's (refusal()):
//   XF_BAD_MATRIX  "transforms: matrix entry not finite"                         either matrix of a moved record (a record
//                                                                                 with a NaN or an infinity is never the identity)
//   XF_BAD_LIT     "transforms: a mesh that carries an area light cannot move"   a moved record, a triangle with tri_area_light >= 0
//   XF_BAD_SHARED  "transforms: vertex shared by two meshes"
//   XF_BAD_POINT   "points: coordinate not finite"                               a RESULT (normals are never tested)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/yuki_hip.h"
#include "yk_device.h"
#include "yk_math.h"
#include "yk_scene_input.h"

namespace yk {
namespace xfm {

enum : uint32_t { XF_MOVED = 1u, XF_FLIPS = 2u };
enum : uint32_t { XF_BAD_MATRIX = 1u, XF_BAD_LIT = 2u, XF_BAD_SHARED = 4u, XF_BAD_POINT = 8u };
static const uint32_t XF_NO_MESH = 0xffffffffu;
static const int XF_RECORD_FLOATS = 32;  // a yk_mesh_transform: rest_to_world, then world_to_rest

inline const char* refusal(uint32_t flag) {
    return (flag & XF_BAD_MATRIX)   ? "transforms: matrix entry not finite"
           : (flag & XF_BAD_LIT)    ? "transforms: a mesh that carries an area light cannot move"
           : (flag & XF_BAD_SHARED) ? "transforms: vertex shared by two meshes"
                                    : "points: coordinate not finite";
}

YK_HD bool not_finite(float f) { return (__builtin_bit_cast(uint32_t, f) & 0x7f800000u) == 0x7f800000u; }

YK_HD bool is_identity(const float* m) {
    bool same = true;
#pragma unroll
    for (int k = 0; k < 16; ++k) same = same && m[k] == ((k % 5) == 0 ? 1.0f : 0.0f);
    return same;
}

// rec: the 32 floats of the mesh's record; lit: the mesh has a triangle that carries an area light.  -> XF_MOVED | XF_FLIPS
// bits; *bad gets the XF_BAD_* bits of the record.
YK_HD uint32_t mesh_kind(const float* rec, bool lit, uint32_t* bad) {
    const bool moved = !is_identity(rec);
    bool wrong = false;
    if (moved) {
#pragma unroll
        for (int k = 0; k < XF_RECORD_FLOATS; ++k) wrong = wrong || not_finite(rec[k]);
    }
    *bad = (wrong ? XF_BAD_MATRIX : 0u) | (moved && lit ? XF_BAD_LIT : 0u);
    return moved ? (XF_MOVED | (inp::swaps_handedness(rec) ? XF_FLIPS : 0u)) : 0u;
}

// the table: one triangle of mesh `mesh` with vertices i0, i1, i2 (the host instance; the device takes atomicMin / atomicMax)
inline void table_add(uint32_t* vertex_mesh, uint32_t v, uint32_t mesh) {
    if (mesh < vertex_mesh[2 * (size_t)v]) vertex_mesh[2 * (size_t)v] = mesh;
    if (mesh > vertex_mesh[2 * (size_t)v + 1]) vertex_mesh[2 * (size_t)v + 1] = mesh;
}
YK_HD bool vertex_shared(uint32_t lo, uint32_t hi) { return lo != XF_NO_MESH && lo != hi; }

// The per-vertex rule.  mesh: the vertex's (the table's min word); kinds: mesh_kind of every record; records: 32 floats a mesh.
YK_HD bool vertex_moves(const uint32_t* kinds, uint32_t n_meshes, uint32_t mesh) { return mesh < n_meshes && (kinds[mesh] & XF_MOVED) != 0u; }
YK_HD V3 vertex_point(const float* records, const uint32_t* kinds, uint32_t n_meshes, uint32_t mesh, V3 rest) {
    if (!vertex_moves(kinds, n_meshes, mesh)) return rest;
    return xf_point(records + XF_RECORD_FLOATS * (size_t)mesh, rest);
}
YK_HD V3 vertex_normal(const float* records, const uint32_t* kinds, uint32_t n_meshes, uint32_t mesh, V3 rest) {
    if (!vertex_moves(kinds, n_meshes, mesh)) return rest;
    return xf_normal(records + XF_RECORD_FLOATS * (size_t)mesh + 16, rest);
}
YK_HD bool point_not_finite(V3 p) { return not_finite(p.x) || not_finite(p.y) || not_finite(p.z); }
// a mesh's flags (YK_MESH_*) from creation's and the kind of its record
YK_HD uint32_t mesh_flags_of(uint32_t created, uint32_t kind) { return (kind & XF_FLIPS) ? (created ^ YK_MESH_SWAPS) : created; }

// The previous position of rest point `rest` under record `rec` (32 floats) for the motion pass: the same two cases.
YK_HD V3 point_under(const float* rec, bool identity, V3 rest) { return identity ? rest : xf_point(rec, rest); }

// ---- tree cost.  nodes: the builder's 32-byte nodes (8 words: min.xyz, max.xyz, link, flags); all of it binary64.
YK_HD double node_area(const uint32_t* nodes, uint32_t i) {
    const uint32_t* w = nodes + 8 * (size_t)i;
    const double dx = (double)__builtin_bit_cast(float, w[3]) - (double)__builtin_bit_cast(float, w[0]);
    const double dy = (double)__builtin_bit_cast(float, w[4]) - (double)__builtin_bit_cast(float, w[1]);
    const double dz = (double)__builtin_bit_cast(float, w[5]) - (double)__builtin_bit_cast(float, w[2]);
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}
// node i's term: into *interior, or — a leaf — A(n) * count(n) into *leaf
YK_HD void cost_term(const uint32_t* nodes, uint32_t i, double* interior, double* leaf) {
    const uint32_t flags = nodes[8 * (size_t)i + 7];
    const double a = node_area(nodes, i);
    *interior = (flags >> 24) != 0u ? 0.0 : a;
    *leaf = (flags >> 24) != 0u ? a * (double)(flags & 0xffffu) : 0.0;
}
YK_HD double cost_of(double interior, double leaf, double root_area) { return root_area > 0.0 ? (interior + leaf) / root_area : 0.0; }
// the host instance: a loop in node order
inline double tree_cost(const uint32_t* nodes, size_t n_nodes) {
    if (n_nodes == 0) return 0.0;
    double interior = 0.0, leaf = 0.0;
    for (size_t i = 0; i < n_nodes; ++i) {
        double a, b;
        cost_term(nodes, (uint32_t)i, &a, &b);
        interior += a;
        leaf += b;
    }
    return cost_of(interior, leaf, node_area(nodes, 0u));
}

}  // namespace xfm
}  // namespace yk
