// yk_scene_records.cpp — the device records from a host tree: the sequential loops the device layout (yk_scene_layout.hip)
// is held against, in three sections.  Plain host code: no context, no scene description, no device call.
#include "yk_scene_records.h"

#include <algorithm>
#include <cstring>

#include "yk_kernels.h"

using namespace yk;

// DevNode per interior node, the root ref and the two tree tops
static void layout_nodes(const HostLayoutInput& in, SceneRecords& out) {
    const std::vector<yk_bvh_node>& nodes = in.bvh->nodes;
    // interior index of each reference node = number of interior nodes before it
    std::vector<uint32_t> interior_index(nodes.size());
    uint32_t cnt = 0;
    for (size_t i = 0; i < nodes.size(); ++i) {
        interior_index[i] = cnt;
        if (!nodes[i].is_leaf) ++cnt;
    }
    auto ref_of = [&](uint32_t idx) -> uint32_t { return nodes[idx].is_leaf ? (YK_LEAF_BIT | nodes[idx].a) : interior_index[idx]; };
    std::vector<DevNode>& dn = out.nodes;
    dn.assign(std::max<size_t>(in.n_interior, 1), DevNode());
    for (size_t i = 0; i < nodes.size(); ++i) {
        if (nodes[i].is_leaf) continue;
        const yk_bvh_node& c0 = nodes[i + 1];
        const yk_bvh_node& c1 = nodes[nodes[i].a];
        DevNode& o = dn[interior_index[i]];
        o.q0 = make_float4(c0.bmin[0], c0.bmin[1], c0.bmin[2], c0.bmax[0]);
        o.q1 = make_float4(c0.bmax[1], c0.bmax[2], c1.bmin[0], c1.bmin[1]);
        o.q2 = make_float4(c1.bmin[2], c1.bmax[0], c1.bmax[1], c1.bmax[2]);
        o.q3 = make_uint4(ref_of((uint32_t)i + 1), ref_of(nodes[i].a) | ((uint32_t)nodes[i].axis << YK_AXIS_SHIFT), 0u, 0u);
    }
    // top of the tree, breadth first, for the LDS-resident copies (YK_TOP_BIT refs).  Two sets: the closest-hit kernels
    // keep 8-byte stack entries (ref, entry distance) in LDS and have room for trace_top_nodes() nodes beside them; the
    // any-hit kernel's entries are a bare ref (4 bytes), which leaves room for trace_top_nodes_any() — more than twice as many.
    auto build_top = [&](size_t cap, std::vector<DevNode>& top) {
        top.clear();
        if (nodes[0].is_leaf || cap == 0) return;
        std::vector<uint32_t> order;  // reference node indices, breadth first
        std::vector<uint32_t> top_id(nodes.size(), 0xffffffffu);
        order.push_back(0);
        top_id[0] = 0;
        for (size_t q = 0; q < order.size() && order.size() < cap; ++q) {
            const uint32_t P = order[q];
            for (uint32_t c : {P + 1, nodes[P].a}) {
                if (!nodes[c].is_leaf && order.size() < cap) {
                    top_id[c] = (uint32_t)order.size();
                    order.push_back(c);
                }
            }
        }
        for (uint32_t P : order) {
            DevNode t = dn[interior_index[P]];
            const uint32_t c0 = P + 1, c1 = nodes[P].a;
            if (top_id[c0] != 0xffffffffu) t.q3.x = YK_TOP_BIT | top_id[c0];
            if (top_id[c1] != 0xffffffffu) t.q3.y = YK_TOP_BIT | top_id[c1] | ((uint32_t)nodes[P].axis << YK_AXIS_SHIFT);
            top.push_back(t);
        }
    };
    build_top((size_t)std::min<int64_t>(in.opt.top_nodes, trace_top_nodes()), out.top);
    build_top((size_t)std::min<int64_t>(in.opt.top_nodes, trace_top_nodes_any()), out.top_any);
    out.root_ref = ref_of(0);
}

static void layout_wide(const HostLayoutInput& in, SceneRecords& out) {
    const std::vector<yk_bvh_node>& nodes = in.bvh->nodes;
    // 4-wide collapse (DevNode4): one node per reference interior node reached at even depth
    // below the root.  Built only while the traversal stack of the collapsed tree is
    // guaranteed to fit (the reference asserts on its own stack depth, bvh.rs:172-174).
    std::vector<DevNode4>& dn4 = out.nodes4;
    const bool wide = in.opt.wide_bvh != 0 && !nodes[0].is_leaf && in.bvh->depth <= 64;
    out.wide_auto = wide && in.opt.wide_bvh == 2;
    if (!wide) return;
    dn4.reserve(in.n_interior / 2 + 1);
    struct Todo {
        uint32_t binary;  // reference node index of P
        uint32_t slot;    // DevNode4 index to fill
    };
    std::vector<Todo> stack;
    dn4.emplace_back();
    stack.push_back(Todo{0u, 0u});
    while (!stack.empty()) {
        const Todo td = stack.back();
        stack.pop_back();
        const uint32_t P = td.binary, A = P + 1, B = nodes[P].a;
        uint32_t child[4] = {YK_REF_NONE, YK_REF_NONE, YK_REF_NONE, YK_REF_NONE};  // reference node index per slot
        if (nodes[A].is_leaf) {
            child[0] = A;
        } else {
            child[0] = A + 1;
            child[1] = nodes[A].a;
        }
        if (nodes[B].is_leaf) {
            child[2] = B;
        } else {
            child[2] = B + 1;
            child[3] = nodes[B].a;
        }
        float box[4][6] = {};
        uint32_t ref[4];
        for (int k = 0; k < 4; ++k) {
            ref[k] = YK_REF_NONE;
            if (child[k] == YK_REF_NONE) continue;
            const yk_bvh_node& c = nodes[child[k]];
            for (int a = 0; a < 3; ++a) {
                box[k][a] = c.bmin[a];
                box[k][3 + a] = c.bmax[a];
            }
            if (c.is_leaf) {
                ref[k] = YK_LEAF_BIT | c.a;
            } else {
                ref[k] = (uint32_t)dn4.size();
                dn4.emplace_back();
            }
        }
        // children are expanded so that the first visited subtree (for a positive ray) follows in memory
        for (int k = 3; k >= 0; --k)
            if (ref[k] != YK_REF_NONE && !(ref[k] & YK_LEAF_BIT)) stack.push_back(Todo{child[k], ref[k]});
        DevNode4& o = dn4[td.slot];
        o.q0 = make_float4(box[0][0], box[0][1], box[0][2], box[0][3]);
        o.q1 = make_float4(box[0][4], box[0][5], box[1][0], box[1][1]);
        o.q2 = make_float4(box[1][2], box[1][3], box[1][4], box[1][5]);
        o.q3 = make_float4(box[2][0], box[2][1], box[2][2], box[2][3]);
        o.q4 = make_float4(box[2][4], box[2][5], box[3][0], box[3][1]);
        o.q5 = make_float4(box[3][2], box[3][3], box[3][4], box[3][5]);
        o.q6 = make_uint4(ref[0], ref[1], ref[2], ref[3]);
        const uint32_t axA = nodes[A].is_leaf ? 0u : nodes[A].axis, axB = nodes[B].is_leaf ? 0u : nodes[B].axis;
        o.q7 = make_uint4((uint32_t)nodes[P].axis | (axA << 2) | (axB << 4), 0u, 0u, 0u);
    }
}

// tris / prim_shade / prim_attr in leaf order
static void layout_prims(const HostLayoutInput& in, SceneRecords& out) {
    const HostBvh* bvh = in.bvh;
    const uint32_t nt = in.n_triangles;
    const size_t np = bvh->shape_order.size();
    auto bits = [](uint32_t u) {
        float f;
        std::memcpy(&f, &u, 4);
        return f;
    };
    out.tris.assign(3 * np, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    out.prim_shade.assign(np, make_uint4(0u, 0u, 0u, 0u));
    std::vector<uint8_t> last(np, 0);
    for (const yk_bvh_node& n : bvh->nodes)
        if (n.is_leaf) last[(size_t)n.a + n.count - 1] = 1;
    for (size_t p = 0; p < np; ++p) {
        const uint32_t src = bvh->shape_order[p];
        const uint32_t material = (uint32_t)(src >= nt ? in.sphere_material[src - nt] : in.tri_material[src]), kind = in.mat_kind[material];
        const uint32_t flags = (last[p] ? YK_PRIM_LAST : 0u) | (kind << YK_PRIM_KIND_SHIFT);
        if (src >= nt) {  // sphere: only the source index and the flags are read
            out.tris[3 * p + 0] = make_float4(0.0f, 0.0f, 0.0f, bits(0xffffffffu));
            out.tris[3 * p + 1] = make_float4(0.0f, 0.0f, 0.0f, bits(src));
            out.tris[3 * p + 2] = make_float4(0.0f, 0.0f, 0.0f, bits(flags | YK_PRIM_SPHERE));
            out.prim_shade[p] = make_uint4(0u, 0u, 0u, (material << 6) | (kind << 3));
            continue;
        }
        const uint32_t* vi = in.indices + 3 * (size_t)src;
        const float* p0 = in.points + 3 * (size_t)vi[0];
        const float* p1 = in.points + 3 * (size_t)vi[1];
        const float* p2 = in.points + 3 * (size_t)vi[2];
        out.tris[3 * p + 0] = make_float4(p0[0], p0[1], p0[2], bits((uint32_t)in.tri_area_light[src]));
        out.tris[3 * p + 1] = make_float4(p1[0], p1[1], p1[2], bits(src));
        out.tris[3 * p + 2] = make_float4(p2[0], p2[1], p2[2], bits(flags));
        out.prim_shade[p] = make_uint4(vi[0], vi[1], vi[2], (material << 6) | (kind << 3) | in.mesh_flags[in.tri_mesh[src]]);
    }
    if (!in.normals && !in.uvs) return;
    // leaf-order copy of the per-vertex normals / uvs (yk_device.h: DevScene::prim_attr)
    out.prim_attr.assign(4 * np, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (size_t p = 0; p < np; ++p) {
        const uint32_t src = bvh->shape_order[p];
        if (src >= nt) continue;
        const uint32_t mfl = in.mesh_flags[in.tri_mesh[src]];
        float nrm[3][3] = {}, uv[3][2] = {};
        for (int k = 0; k < 3; ++k) {
            const size_t vi = in.indices[3 * (size_t)src + k];
            if (mfl & YK_MESH_NORMALS)
                for (int c = 0; c < 3; ++c) nrm[k][c] = in.normals[3 * vi + c];
            if (mfl & YK_MESH_UVS)
                for (int c = 0; c < 2; ++c) uv[k][c] = in.uvs[2 * vi + c];
        }
        out.prim_attr[4 * p + 0] = make_float4(nrm[0][0], nrm[0][1], nrm[0][2], uv[0][0]);
        out.prim_attr[4 * p + 1] = make_float4(nrm[1][0], nrm[1][1], nrm[1][2], uv[0][1]);
        out.prim_attr[4 * p + 2] = make_float4(nrm[2][0], nrm[2][1], nrm[2][2], uv[1][0]);
        out.prim_attr[4 * p + 3] = make_float4(uv[1][1], uv[2][0], uv[2][1], 0.0f);
    }
}

SceneRecords layout_records_host(const HostLayoutInput& in) {
    SceneRecords out;
    layout_nodes(in, out);
    layout_wide(in, out);
    layout_prims(in, out);
    return out;
}
