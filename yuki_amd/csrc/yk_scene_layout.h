// yk_scene_layout.h — the traversal records of a scene as functions of its tree, written once for the gfx950
// kernels of yk_scene_layout.hip ("scene_layout" = 1) and for the host instance of the two order rules (ibid.,
// yk_layout_top_order / yk_layout_wide_slots).  The bytes are the ones the sequential loops of yk_scene_records.cpp
// (layout_records_host) produce; those loops stay the yardstick, the expressions below restate them.
//
// The tree is the reference's depth-first array of 32-byte nodes, read as 8 words a node (yk_bvh_build.h):
// words 0..5 the box, word 6 `a` (second child | first shape), word 7 count | axis << 16 | is_leaf << 24.
//
// Closed forms of the two orders the host loops define by running
//   * interior index: the number of interior nodes before a node in the array — an exclusive scan of !is_leaf.
//   * tree top (cap nodes, breadth first): the host loop admits a child only while the set is below `cap`, looking at
//     the children of the queued nodes in queue order.  Once the set is full nothing is admitted any more, so the
//     rule is a truncation: the k-th interior child met in that order gets id k and is admitted iff k < cap.
//     top_order walks the queue `nt` entries at a time; the ids of a round come from one exclusive scan.
//   * 4-wide collapse: the collapsed nodes are the interior nodes at an even distance from the root (an interior
//     node's grandparent is interior and, by induction, collapsed).  The host loop's stack pops them in ascending
//     array index — it pushes the interior children of a node in descending child order, the children A+1, A.a,
//     B+1, B.a ascend, and the array is pre-order — and a node gives its interior children the next free slots in
//     child order when it is popped.  So with w(X) = the number of interior wide children of a collapsed X (0 for
//     every other node) and E = the exclusive scan of w over the array,
//         slot(child k of X) = 1 + E(X) + |{interior children of X below k}|,   slot(root) = 0,
//     and the collapse has 1 + sum(w) nodes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "yk_bvh_build.h"
#include "yk_device.h"

namespace yk {
namespace lay {

using lv::kNone;

YK_HD bool nd_leaf(const uint32_t* nodes, uint32_t i) { return (nodes[8 * (size_t)i + 7] >> 24) != 0u; }
YK_HD uint32_t nd_a(const uint32_t* nodes, uint32_t i) { return nodes[8 * (size_t)i + 6]; }
YK_HD uint32_t nd_count(const uint32_t* nodes, uint32_t i) { return nodes[8 * (size_t)i + 7] & 0xffffu; }
YK_HD uint32_t nd_axis(const uint32_t* nodes, uint32_t i) { return (nodes[8 * (size_t)i + 7] >> 16) & 0xffu; }

// host: every node's depth (the root's is 1) from the pre-order array, where both children follow their parent
inline std::vector<uint32_t> node_depths(const uint32_t* nodes, size_t n) {
    std::vector<uint32_t> depth(n, 0u);
    depth[0] = 1u;
    for (uint32_t i = 0; i < (uint32_t)n; ++i)
        if (!nd_leaf(nodes, i)) depth[i + 1u] = depth[nd_a(nodes, i)] = depth[i] + 1u;
    return depth;
}

// leaf: the leaf bit and its first slot of the leaf order; interior: its interior index
YK_HD uint32_t ref_of(const uint32_t* nodes, const uint32_t* interior_index, uint32_t i) { return nd_leaf(nodes, i) ? (YK_LEAF_BIT | nd_a(nodes, i)) : interior_index[i]; }

struct NodeWords {  // one 32-byte node as two 16-byte loads
    uint4 lo, hi;   // lo = (min.xyz, max.x)  hi = (max.y, max.z, a, count | axis << 16 | is_leaf << 24)
};
YK_HD NodeWords load_node(const uint32_t* nodes, uint32_t i) {
    const uint4* p = reinterpret_cast<const uint4*>(nodes + 8 * (size_t)i);
    return NodeWords{p[0], p[1]};
}

// DevNode of interior node i as four 16-byte words: both children's boxes bit for bit, the refs, the split axis.
// ref0 / ref1: the children's references (ref_of, or YK_TOP_BIT | id inside a tree top).
YK_HD void dev_node_words(const uint32_t* nodes, uint32_t i, uint32_t ref0, uint32_t ref1, uint4 (&q)[4]) {
    const NodeWords c0 = load_node(nodes, i + 1u), c1 = load_node(nodes, nd_a(nodes, i));
    q[0] = c0.lo;
    q[1] = make_uint4(c0.hi.x, c0.hi.y, c1.lo.x, c1.lo.y);
    q[2] = make_uint4(c1.lo.z, c1.lo.w, c1.hi.x, c1.hi.y);
    q[3] = make_uint4(ref0, ref1 | (nd_axis(nodes, i) << YK_AXIS_SHIFT), 0u, 0u);
}

// ---- tree top ----------------------------------------------------------------------------------------
// order[q]: the reference node at breadth-first position q; id0[q] / id1[q] (may both be NULL): the top id of its
// first / second child, kNone outside the set.  Returns the size of the set.  Exec: lane id and count, a barrier
// and an exclusive scan over the lanes (the device: one wave; the host instance: one lane).
template <class Exec> YK_HD uint32_t top_order(Exec& ex, const uint32_t* nodes, uint32_t cap, uint32_t* order, uint32_t* id0, uint32_t* id1) {
    if (cap == 0u || nd_leaf(nodes, 0u)) return 0u;
    if (ex.tid == 0u) order[0] = 0u;
    ex.sync();
    uint32_t size = 1u, done = 0u;
    while (done < size) {
        const uint32_t end = size < done + ex.nt ? size : done + ex.nt, q = done + ex.tid;
        const bool in = q < end;
        uint32_t c0 = 0u, c1 = 0u;
        bool i0 = false, i1 = false;
        if (in) {
            const uint32_t P = order[q];
            c0 = P + 1u;
            c1 = nd_a(nodes, P);
            i0 = !nd_leaf(nodes, c0);
            i1 = !nd_leaf(nodes, c1);
        }
        uint32_t total;
        const uint32_t t0 = size + ex.scan((i0 ? 1u : 0u) + (i1 ? 1u : 0u), total), t1 = t0 + (i0 ? 1u : 0u);
        const bool a0 = i0 && t0 < cap, a1 = i1 && t1 < cap;
        if (a0) order[t0] = c0;
        if (a1) order[t1] = c1;
        if (in && id0) {
            id0[q] = a0 ? t0 : kNone;
            id1[q] = a1 ? t1 : kNone;
        }
        size = size + total < cap ? size + total : cap;
        done = end;
        ex.sync();
    }
    return size;
}

// ---- 4-wide collapse ----------------------------------------------------------------------------------
YK_HD bool wide_collapsed(const uint32_t* nodes, const uint32_t* depth, uint32_t i) { return !nd_leaf(nodes, i) && ((depth[i] ^ depth[0]) & 1u) == 0u; }
// reference node per slot of collapsed node P: A's children (or A itself, then none), B's children (or B itself, then none)
YK_HD void wide_children(const uint32_t* nodes, uint32_t P, uint32_t (&child)[4]) {
    const uint32_t A = P + 1u, B = nd_a(nodes, P);
    const bool la = nd_leaf(nodes, A), lb = nd_leaf(nodes, B);
    child[0] = la ? A : A + 1u;
    child[1] = la ? YK_REF_NONE : nd_a(nodes, A);
    child[2] = lb ? B : B + 1u;
    child[3] = lb ? YK_REF_NONE : nd_a(nodes, B);
}
// w(i): the slots node i hands out when the host loop pops it
YK_HD uint32_t wide_count(const uint32_t* nodes, const uint32_t* depth, uint32_t i) {
    if (!wide_collapsed(nodes, depth, i)) return 0u;
    uint32_t child[4], n = 0u;
    wide_children(nodes, i, child);
#pragma unroll
    for (int k = 0; k < 4; ++k) n += (child[k] != YK_REF_NONE && !nd_leaf(nodes, child[k])) ? 1u : 0u;
    return n;
}
// refs of collapsed node X (excl = E(X)); slot_of (may be NULL) receives the slot of every interior child
YK_HD void wide_refs(const uint32_t* nodes, uint32_t excl, const uint32_t (&child)[4], uint32_t (&ref)[4], uint32_t* slot_of) {
    uint32_t next = 1u + excl;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (child[k] == YK_REF_NONE) {
            ref[k] = YK_REF_NONE;
        } else if (nd_leaf(nodes, child[k])) {
            ref[k] = YK_LEAF_BIT | nd_a(nodes, child[k]);
        } else {
            ref[k] = next;
            if (slot_of) slot_of[child[k]] = next;
            ++next;
        }
    }
}
// DevNode4 of collapsed node P as eight 16-byte words; an absent child has a zeroed box
YK_HD void dev_node4_words(const uint32_t* nodes, uint32_t P, const uint32_t (&child)[4], const uint32_t (&ref)[4], uint4 (&q)[8]) {
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    NodeWords c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c[k].lo = zero;
        c[k].hi = zero;
        if (child[k] != YK_REF_NONE) c[k] = load_node(nodes, child[k]);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // slots (0, 1), then (2, 3): packed like DevNode
        const NodeWords &u = c[2 * h], &v = c[2 * h + 1];
        q[3 * h + 0] = u.lo;
        q[3 * h + 1] = make_uint4(u.hi.x, u.hi.y, v.lo.x, v.lo.y);
        q[3 * h + 2] = make_uint4(v.lo.z, v.lo.w, v.hi.x, v.hi.y);
    }
    const uint32_t A = P + 1u, B = nd_a(nodes, P);
    const uint32_t axA = nd_leaf(nodes, A) ? 0u : nd_axis(nodes, A), axB = nd_leaf(nodes, B) ? 0u : nd_axis(nodes, B);
    q[6] = make_uint4(ref[0], ref[1], ref[2], ref[3]);
    q[7] = make_uint4(nd_axis(nodes, P) | (axA << 2) | (axB << 4), 0u, 0u, 0u);
}

// ---- primitive records -----------------------------------------------------------------------------------
struct PrimArrays {  // the scene's own device buffers (DevScene) and two small tables
    const uint32_t* indices;
    const float* points;
    const float* normals;
    const float* uvs;
    const uint32_t* tri_mesh;
    const int32_t* tri_material;
    const int32_t* tri_area_light;
    const uint32_t* mesh_flags;
    const DevSphere* spheres;
    const uint8_t* mat_kind;  // device BSDF kind (MK_*) per material
    uint32_t n_triangles;
};
// Leaf-order slot p holding source shape src: tris[3p..], prim_shade[p] and, when attr is given, prim_attr[4p..].
YK_HD void prim_words(const PrimArrays& s, uint32_t src, bool last, uint4 (&tri)[3], uint4& shade, uint4 (&attr)[4], bool want_attr) {
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int k = 0; k < 4; ++k) attr[k] = zero;
    if (src >= s.n_triangles) {  // sphere: only the source index and the flags are read
        const uint32_t mat = (uint32_t)s.spheres[src - s.n_triangles].material, kind = s.mat_kind[mat];
        tri[0] = make_uint4(0u, 0u, 0u, 0xffffffffu);
        tri[1] = make_uint4(0u, 0u, 0u, src);
        tri[2] = make_uint4(0u, 0u, 0u, (last ? YK_PRIM_LAST : 0u) | YK_PRIM_SPHERE | (kind << YK_PRIM_KIND_SHIFT));
        shade = make_uint4(0u, 0u, 0u, (mat << 6) | (kind << 3));
        return;
    }
    const uint32_t vi[3] = {s.indices[3 * (size_t)src], s.indices[3 * (size_t)src + 1], s.indices[3 * (size_t)src + 2]};
    const uint32_t mat = (uint32_t)s.tri_material[src], kind = s.mat_kind[mat], mfl = s.mesh_flags[s.tri_mesh[src]];
    const uint32_t w[3] = {(uint32_t)s.tri_area_light[src], src, (last ? YK_PRIM_LAST : 0u) | (kind << YK_PRIM_KIND_SHIFT)};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* p = s.points + 3 * (size_t)vi[k];
        tri[k] = make_uint4(lv::f2u(p[0]), lv::f2u(p[1]), lv::f2u(p[2]), w[k]);
    }
    shade = make_uint4(vi[0], vi[1], vi[2], (mat << 6) | (kind << 3) | mfl);
    if (!want_attr) return;
    uint32_t nrm[3][3] = {}, uv[3][2] = {};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (mfl & YK_MESH_NORMALS)
            for (int c = 0; c < 3; ++c) nrm[k][c] = lv::f2u(s.normals[3 * (size_t)vi[k] + c]);
        if (mfl & YK_MESH_UVS)
            for (int c = 0; c < 2; ++c) uv[k][c] = lv::f2u(s.uvs[2 * (size_t)vi[k] + c]);
    }
    attr[0] = make_uint4(nrm[0][0], nrm[0][1], nrm[0][2], uv[0][0]);
    attr[1] = make_uint4(nrm[1][0], nrm[1][1], nrm[1][2], uv[0][1]);
    attr[2] = make_uint4(nrm[2][0], nrm[2][1], nrm[2][2], uv[1][0]);
    attr[3] = make_uint4(uv[1][1], uv[2][0], uv[2][1], 0u);
}

}  // namespace lay
}  // namespace yk
