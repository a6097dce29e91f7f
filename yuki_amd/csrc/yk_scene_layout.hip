// yk_scene_layout.hip — "scene_layout" = 1: a scene's traversal records (DevNode, the two LDS tree tops, the
// DevNode4 collapse, tris / prim_shade / prim_attr in leaf order) laid out on the device from the tree in HBM
// (yk_scene_layout.h), and the host instance of the two order rules (yk_layout_top_order, yk_layout_wide_slots).
// The bytes are those of layout_records_host (yk_scene_records.cpp); a failure here leaves its reason and the caller
// lays the records out on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "yk_internal.h"
#include "yk_scan.h"
#include "yk_scene_layout.h"

using namespace yk::lay;
using namespace yk::scan;

namespace {

const int kThreads = 256;

struct HostExec {
    uint32_t tid = 0, nt = 1;
    void sync() {}
    uint32_t scan(uint32_t v, uint32_t& total) {
        total = v;
        return 0u;
    }
};
struct WaveExec {  // one wave of 64 lanes
    uint32_t tid, nt;
    __device__ void sync() { __syncthreads(); }
    __device__ uint32_t scan(uint32_t v, uint32_t& total) {
        const uint32_t inc = wave_incl_scan(v, tid);
        total = __shfl(inc, 63);
        return inc - v;
    }
};

// ------------------------------------------------------------------ what the two scans over the node array (yk_scan.h) add up
struct IsInterior {  // -> interior index
    const uint32_t* __restrict__ nodes;
    __device__ uint32_t operator()(uint32_t i) const { return nd_leaf(nodes, i) ? 0u : 1u; }
};
struct WideCount {  // w(i) -> E (yk_scene_layout.h)
    const uint32_t *__restrict__ nodes, *__restrict__ depth;
    __device__ uint32_t operator()(uint32_t i) const { return wide_count(nodes, depth, i); }
};

// ------------------------------------------------------------------ records
// leaf order -> position in the caller's shape order -> source shape (in place: every lane owns its word)
__global__ void k_apply_order(uint32_t* order, const uint32_t* __restrict__ user, uint32_t np) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < np) order[p] = user[order[p]];
}
// one lane per node: an interior node writes its DevNode, a leaf marks the last slot of its run
__global__ void k_nodes(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ iidx, uint32_t n, uint4* out, uint8_t* last) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (nd_leaf(nodes, i)) {
        last[(size_t)nd_a(nodes, i) + nd_count(nodes, i) - 1u] = 1;
        return;
    }
    uint4 q[4];
    dev_node_words(nodes, i, ref_of(nodes, iidx, i + 1u), ref_of(nodes, iidx, nd_a(nodes, i)), q);
    uint4* o = out + 4 * (size_t)iidx[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = q[k];
}
// block b (one wave) walks the queue of tree top b and writes its nodes; words[2 + b] = its size
__global__ void __launch_bounds__(64) k_tops(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ iidx, uint32_t cap_closest, uint32_t cap_any, uint4* out_closest, uint4* out_any, uint32_t* words) {
    __shared__ uint32_t order[YK_TOP_MAX], id0[YK_TOP_MAX], id1[YK_TOP_MAX];
    const uint32_t cap = blockIdx.x == 0 ? cap_closest : cap_any;
    uint4* out = blockIdx.x == 0 ? out_closest : out_any;
    WaveExec ex{threadIdx.x, blockDim.x};
    const uint32_t size = top_order(ex, nodes, cap, order, id0, id1);
    for (uint32_t q = threadIdx.x; q < size; q += blockDim.x) {
        const uint32_t P = order[q];
        const uint32_t r0 = id0[q] != kNone ? (YK_TOP_BIT | id0[q]) : ref_of(nodes, iidx, P + 1u);
        const uint32_t r1 = id1[q] != kNone ? (YK_TOP_BIT | id1[q]) : ref_of(nodes, iidx, nd_a(nodes, P));
        uint4 w[4];
        dev_node_words(nodes, P, r0, r1, w);
        uint4* o = out + 4 * (size_t)q;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = w[k];
    }
    if (threadIdx.x == 0) words[2 + blockIdx.x] = size;
}
// one lane per collapsed node: the slots of its interior children
__global__ void k_wide_slots(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ depth, const uint32_t* __restrict__ excl, uint32_t n, uint32_t* slot) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !wide_collapsed(nodes, depth, i)) return;
    if (i == 0u) slot[0] = 0u;
    uint32_t child[4], ref[4];
    wide_children(nodes, i, child);
    wide_refs(nodes, excl[i], child, ref, slot);
}
// one lane per collapsed node: its 128-byte record
__global__ void k_wide_nodes(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ depth, const uint32_t* __restrict__ excl, const uint32_t* __restrict__ slot, uint32_t n, uint32_t n4, uint4* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !wide_collapsed(nodes, depth, i)) return;
    const uint32_t me = slot[i];
    if (me >= n4) return;
    uint32_t child[4], ref[4];
    wide_children(nodes, i, child);
    wide_refs(nodes, excl[i], child, ref, nullptr);
    uint4 q[8];
    dev_node4_words(nodes, i, child, ref, q);
    uint4* o = out + 8 * (size_t)me;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = q[k];
}
// one lane per slot of the leaf order
__global__ void k_prims(PrimArrays s, const uint32_t* __restrict__ order, const uint8_t* __restrict__ last, uint32_t np, uint32_t n_shapes_total, uint4* tris, uint4* prim_shade, uint4* prim_attr) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const uint32_t src = order[p];
    if (src >= n_shapes_total) return;  // cannot happen (the order is a permutation of the shapes); guards the gathers
    uint4 tri[3], shade, attr[4];
    prim_words(s, src, last[p] != 0, tri, shade, attr, prim_attr != nullptr);
#pragma unroll
    for (int k = 0; k < 3; ++k) tris[3 * (size_t)p + k] = tri[k];
    prim_shade[p] = shade;
    if (prim_attr) {
#pragma unroll
        for (int k = 0; k < 4; ++k) prim_attr[4 * (size_t)p + k] = attr[k];
    }
}

unsigned blocks(size_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

}  // namespace

// ------------------------------------------------------------------ the device layout
uint32_t layout_scene_device(yk_context* ctx, yk_scene* s, const DeviceTree& tree, const uint32_t* d_user_order, const uint8_t* d_mat_kind, bool has_attr, uint32_t tree_depth, bool* order_applied) {
    const uint32_t n = tree.n_nodes, np = tree.n_shapes;
    if (n == 0 || np == 0 || n > YK_REF_INDEX_MAX || np > YK_REF_INDEX_MAX) return YK_LAYOUT_REASON_DEVICE_ERROR;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const uint32_t* nodes = tree.nodes.as<uint32_t>();
    const uint32_t* depth = tree.depth.as<uint32_t>();
    uint32_t* order = tree.order.as<uint32_t>();
    const bool root_leaf = (tree.root_words[7] >> 24) != 0u;
    const uint32_t n_interior = (n - 1u) / 2u;  // a full binary tree
    const uint32_t cap_closest = (uint32_t)std::min<int64_t>(std::min<int64_t>(s->upd.opt.top_nodes, trace_top_nodes()), YK_TOP_MAX);
    const uint32_t cap_any = (uint32_t)std::min<int64_t>(std::min<int64_t>(s->upd.opt.top_nodes, trace_top_nodes_any()), YK_TOP_MAX);
    const bool wide = s->upd.opt.wide_bvh != 0 && !root_leaf && tree_depth <= 64;

    DevScratch tmp;
    uint32_t *d_index = nullptr, *d_bsum = nullptr, *d_slot = nullptr, *d_words = nullptr;
    uint8_t* d_last = nullptr;
    if (!tmp.get(d_index, n) || !tmp.get(d_bsum, scan_blocks(n)) || !tmp.get(d_last, np) || !tmp.get(d_words, 16) || (wide && !tmp.get(d_slot, n))) return YK_LAYOUT_REASON_OUT_OF_MEMORY;
#define LAY_TRY(expr)                                                                                   \
    do {                                                                                                \
        const hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                         \
            (void)hipStreamSynchronize(st);                                                             \
            return layout_reason_of(e_);                                                                \
        }                                                                                               \
    } while (0)
    LAY_TRY(s->nodes.ensure(std::max<size_t>(n_interior, 1) * sizeof(DevNode)));
    LAY_TRY(s->top_nodes.ensure(std::max<size_t>((size_t)std::min(cap_closest, n_interior) * sizeof(DevNode), 16)));
    LAY_TRY(s->top_nodes_any.ensure(std::max<size_t>((size_t)std::min(cap_any, n_interior) * sizeof(DevNode), 16)));
    LAY_TRY(s->tris.ensure(3 * (size_t)np * sizeof(float4)));
    LAY_TRY(s->prim_shade.ensure((size_t)np * sizeof(uint4)));
    LAY_TRY(s->prim_attr.ensure(has_attr ? 4 * (size_t)np * sizeof(float4) : 16));

    LAY_TRY(hipMemsetAsync(d_words, 0, 16 * sizeof(uint32_t), st));
    LAY_TRY(hipMemsetAsync(d_last, 0, np, st));
    if (d_user_order) {
        k_apply_order<<<blocks(np, kThreads), kThreads, 0, st>>>(order, d_user_order, np);
        LAY_TRY(hipGetLastError());
        *order_applied = true;
    }
    // interior index (absolute: ref_of reads it as the host does), DevNode, last-in-leaf marks
    enqueue_scan(st, IsInterior{nodes}, n, d_index, d_bsum, d_words + 0, true);
    if (n_interior == 0) LAY_TRY(hipMemsetAsync(s->nodes.p, 0, sizeof(DevNode), st));  // a single leaf: one default node
    k_nodes<<<blocks(n, kThreads), kThreads, 0, st>>>(nodes, d_index, n, s->nodes.as<uint4>(), d_last);
    // tree tops (they read the interior index, which the wide scan below overwrites)
    k_tops<<<2, 64, 0, st>>>(nodes, d_index, std::min(cap_closest, n_interior), std::min(cap_any, n_interior), s->top_nodes.as<uint4>(), s->top_nodes_any.as<uint4>(), d_words);
    LAY_TRY(hipGetLastError());
    // primitive records
    PrimArrays pa;
    pa.indices = s->indices.as<uint32_t>();
    pa.points = s->points.as<float>();
    pa.normals = s->normals.as<float>();
    pa.uvs = s->uvs.as<float>();
    pa.tri_mesh = s->tri_mesh.as<uint32_t>();
    pa.tri_material = s->tri_material.as<int32_t>();
    pa.tri_area_light = s->tri_area_light.as<int32_t>();
    pa.mesh_flags = s->mesh_flags.as<uint32_t>();
    pa.spheres = s->spheres.as<DevSphere>();
    pa.mat_kind = d_mat_kind;
    pa.n_triangles = s->n_triangles;
    k_prims<<<blocks(np, kThreads), kThreads, 0, st>>>(pa, order, d_last, np, s->n_triangles + s->n_spheres, s->tris.as<uint4>(), s->prim_shade.as<uint4>(), has_attr ? s->prim_attr.as<uint4>() : nullptr);
    LAY_TRY(hipGetLastError());
    // 4-wide collapse: E over the array, the slots, the records
    uint32_t words[16];
    if (wide) {
        enqueue_scan(st, WideCount{nodes, depth}, n, d_index, d_bsum, d_words + 1, true);
        k_wide_slots<<<blocks(n, kThreads), kThreads, 0, st>>>(nodes, depth, d_index, n, d_slot);
        LAY_TRY(hipGetLastError());
    }
    LAY_TRY(hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, st));
    LAY_TRY(hipStreamSynchronize(st));
    if (words[0] != n_interior) return YK_LAYOUT_REASON_DEVICE_ERROR;
    uint32_t n4 = 0;
    if (wide) {
        n4 = 1u + words[1];
        if (n4 > n_interior) return YK_LAYOUT_REASON_DEVICE_ERROR;
        LAY_TRY(s->nodes4.ensure((size_t)n4 * sizeof(DevNode4)));
        k_wide_nodes<<<blocks(n, kThreads), kThreads, 0, st>>>(nodes, depth, d_index, d_slot, n, n4, s->nodes4.as<uint4>());
        LAY_TRY(hipGetLastError());
        LAY_TRY(hipStreamSynchronize(st));
    } else {
        LAY_TRY(s->nodes4.ensure(16));
    }
#undef LAY_TRY
    set_record_layout(s, n_interior, n4, words[2], words[3], np, has_attr, root_leaf ? (YK_LEAF_BIT | tree.root_words[6]) : 0u, wide && s->upd.opt.wide_bvh == 2);
    return YK_LAYOUT_REASON_NONE;
}

// ------------------------------------------------------------------ the host instance of the two order rules
extern "C" size_t yk_layout_top_order(const yk_bvh_node* nodes, size_t n, uint32_t cap, uint32_t* out_order) try {
    if (!nodes || n == 0 || n > YK_REF_INDEX_MAX || (cap && !out_order)) return 0;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(nodes);
    HostExec ex;
    return top_order(ex, w, cap, out_order, (uint32_t*)nullptr, (uint32_t*)nullptr);
} catch (const std::exception&) {
    return 0;
}

extern "C" size_t yk_layout_wide_slots(const yk_bvh_node* nodes, size_t n, uint32_t* out_slot_per_node) try {
    if (!nodes || n == 0 || n > YK_REF_INDEX_MAX || !out_slot_per_node) return 0;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(nodes);
    for (size_t i = 0; i < n; ++i) out_slot_per_node[i] = kNone;
    if (nd_leaf(w, 0u)) return 0;
    const std::vector<uint32_t> depth = node_depths(w, n);
    std::vector<uint32_t> excl(n);
    uint32_t run = 0u;
    for (uint32_t i = 0; i < (uint32_t)n; ++i) {  // the scan
        excl[i] = run;
        run += wide_count(w, depth.data(), i);
    }
    out_slot_per_node[0] = 0u;
    for (uint32_t i = 0; i < (uint32_t)n; ++i) {  // the lanes of k_wide_slots
        if (!wide_collapsed(w, depth.data(), i)) continue;
        uint32_t child[4], ref[4];
        wide_children(w, i, child);
        wide_refs(w, excl[i], child, ref, out_slot_per_node);
    }
    return 1u + (size_t)run;
} catch (const std::exception&) {
    return 0;
}
