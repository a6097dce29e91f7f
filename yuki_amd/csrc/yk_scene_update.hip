// yk_scene_update.hip — yk_scene_update[_device], the device route (gfx950): a moved mesh keeps its tree, and only what
// depends on coordinates is recomputed (yk_scene_update.h: the rule).  Streaming kernels, one element a lane, 256 lanes
// a block:
//   k_points_finite   the all-or-nothing test over the caller's array, 16-byte loads, one flag word
//   k_leaves          one lane per leaf: the fold of its shapes' bounds from the new points
//   k_level           one launch per tree level, deepest first, one lane per interior node: lv::interior_bounds
//   k_top_levels      the levels at the top of the tree (a block's lanes or fewer each) by ONE block, a barrier between levels
// A kernel boundary is what hands a child's box to its parent: the per-XCD L2s are not coherent, so a parent-pointer climb
// with arrival counters would need an agent-scope release and acquire per step.  Inside k_top_levels every box is written
// and read by one workgroup, on one CU, where the barrier orders them.
// The records are the layout's (layout_scene_device, yk_scene_layout.hip): the same kernels creation runs.
//
// The plan (yk_scene::UpdateState), built by a scene's first update on this route and kept: the tree in HBM (uploaded when
// the host built it), every node's depth (the builder's own, or lay::node_depths), the nodes grouped by depth — a count
// per level with integer atomics, a host scan over the few levels, a scatter; the order inside a level is free — with the
// leaves as the last group, the spheres' bounds and the materials' kinds.  The interior index, the wide slots and the
// last-in-leaf marks are recomputed by the layout on every update (DESIGN.md §3 has the measurement).
// yk_scene_change.cpp calls the route's steps (plan_scene_update, stage_points_device, commit_points_device, refit_scene_device);
// an edit in place runs the same plan, boxes and records after it has rewritten the spheres' bounds or the materials' kinds.
// Also here: yk_bvh_refit, the host instance of the rule.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "yk_scene_route.h"
#include "yk_scene_update.h"

using namespace yk::upd;
using namespace yk::lay;

namespace {

const int kThreads = 256;

// p[head .. head + 4 nvec) is 16-byte aligned; lane 0 of the grid also looks at the floats in front of and behind it
__global__ void __launch_bounds__(kThreads) k_points_finite(const uint32_t* __restrict__ p, size_t n, uint32_t head, size_t nvec, uint32_t* flag) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    bool bad = false;
    if (t < nvec) {
        const uint4 v = reinterpret_cast<const uint4*>(p + head)[t];
        bad = not_finite_bits(v.x) || not_finite_bits(v.y) || not_finite_bits(v.z) || not_finite_bits(v.w);
    }
    if (t == 0) {
        for (uint32_t k = 0; k < head; ++k) bad |= not_finite_bits(p[k]);
        for (size_t k = head + 4 * nvec; k < n; ++k) bad |= not_finite_bits(p[k]);
    }
    if (bad) atomicOr(flag, 1u);
}

// the group of node i: its depth below the root for an interior node, `leaf_group` for a leaf
__device__ uint32_t group_of(const uint32_t* nodes, const uint32_t* depth, uint32_t i, uint32_t leaf_group) { return nd_leaf(nodes, i) ? leaf_group : depth[i] - depth[0]; }
// words[0 .. leaf_group]: nodes per group; words[leaf_group + 1]: set when a depth is not below leaf_group (the plan is refused)
__global__ void __launch_bounds__(kThreads) k_group_count(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ depth, uint32_t n, uint32_t leaf_group, uint32_t* words) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = group_of(nodes, depth, i, leaf_group);
    if (g > leaf_group || (g == leaf_group && !nd_leaf(nodes, i))) {
        atomicOr(&words[leaf_group + 1u], 1u);
        return;
    }
    atomicAdd(&words[g], 1u);
}
// cursor[g]: the next free entry of group g in `list` (starts at the group's offset)
__global__ void __launch_bounds__(kThreads) k_group_scatter(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ depth, uint32_t n, uint32_t leaf_group, uint32_t* cursor, uint32_t* list) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = group_of(nodes, depth, i, leaf_group);
    if (g > leaf_group) return;
    const uint32_t at = atomicAdd(&cursor[g], 1u);
    if (at < n) list[at] = i;
}

__global__ void __launch_bounds__(kThreads) k_leaves(uint32_t* nodes, const uint32_t* __restrict__ list, uint32_t n_leaves, uint32_t n_nodes, const uint32_t* __restrict__ order, GeometryBound bound) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= n_leaves) return;
    const uint32_t i = list[t];
    if (i >= n_nodes) return;  // cannot happen; guards the store
    const uint32_t first = nd_a(nodes, i), count = nd_count(nodes, i);
    if ((uint64_t)first + count > bound.n_shapes) return;  // cannot happen; guards the reads of `order`
    refit_leaf(nodes, i, order, bound);
}

// interior node i of n: both children inside the array
__device__ bool links_ok(const uint32_t* nodes, uint32_t i, uint32_t n) { return i + 1u < n && nd_a(nodes, i) < n; }

__global__ void __launch_bounds__(kThreads) k_level(uint32_t* nodes, const uint32_t* __restrict__ list, uint32_t count, uint32_t n_nodes) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= count) return;
    const uint32_t i = list[t];
    if (links_ok(nodes, i, n_nodes)) lv::interior_bounds(nodes, i);
}

// levels n_top - 1 .. 0, each of at most kThreads nodes (off[d] .. off[d + 1] of `list`), by one block
__global__ void __launch_bounds__(kThreads) k_top_levels(uint32_t* nodes, const uint32_t* __restrict__ list, const uint32_t* __restrict__ off, uint32_t n_top, uint32_t n_nodes) {
    for (uint32_t d = n_top; d-- > 0u;) {
        const uint32_t begin = off[d], count = off[d + 1u] - begin;
        if (threadIdx.x < count) {
            const uint32_t i = list[begin + threadIdx.x];
            if (links_ok(nodes, i, n_nodes)) lv::interior_bounds(nodes, i);
        }
        __threadfence_block();
        __syncthreads();
    }
}

// The plan of the device route.  Returns YK_LAYOUT_REASON_*; a plan that fails is dropped and the next update tries again.
uint32_t build_plan(yk_context* ctx, yk_scene* s) {
    yk_scene::UpdateState& u = s->upd;
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)s->info.n_nodes, np = (uint32_t)s->info.n_shapes;
    if (n == 0 || np == 0 || n > YK_REF_INDEX_MAX || np > YK_REF_INDEX_MAX) return YK_LAYOUT_REASON_DEVICE_ERROR;
    size_t added = 0;
    if (!s->tree_nodes.p || !s->tree_order.p || !u.depth.p) {  // a host-built tree: nodes, depths and order go up, as for the device layout
        const HostBvh* bvh = scene_host_tree(s);
        if (!bvh || bvh->nodes.size() != n || bvh->shape_order.size() != np) return YK_LAYOUT_REASON_DEVICE_ERROR;
        const size_t had = s->tree_nodes.bytes + s->tree_order.bytes + u.depth.bytes;  // nothing, unless a scene kept some of the three
        DeviceTree up;
        const hipError_t e = upload_host_tree(*bvh, up);
        if (e == hipSuccess) adopt_device_tree(s, up, nullptr);  // the host copy stays current
        up.release();  // what the scene held before (resident beside the upload until here), or the failed upload
        ROUTE_TRY(st, e);
        added += s->tree_nodes.bytes + s->tree_order.bytes + u.depth.bytes - had;  // growth only: a tree's buffers have one size
    } else {
        added += u.depth.bytes;  // the builder's own, kept since creation
    }
    {
        const size_t had = u.sphere_b.bytes + u.mat_kind_d.bytes;
        ROUTE_TRY(st, put_host_array(u.sphere_b, u.sphere_bounds.data(), u.sphere_bounds.size() * 4));
        ROUTE_TRY(st, put_host_array(u.mat_kind_d, u.mat_kind.data(), u.mat_kind.size()));
        added += u.sphere_b.bytes + u.mat_kind_d.bytes - had;
    }
    // groups: interior nodes by depth below the root (fewer than the tree's depth), then the leaves
    const uint32_t leaf_group = s->bvh->depth + 1u;
    std::vector<uint32_t> words(leaf_group + 2u, 0u);
    {
        const size_t had = u.words.bytes + u.list.bytes;
        ROUTE_TRY(st, u.words.ensure((words.size() + 1) * 4));  // one more word: the flag of k_points_finite
        ROUTE_TRY(st, u.list.ensure(std::max<size_t>((size_t)n * 4, 16)));
        added += u.words.bytes + u.list.bytes - had;
    }
    uint32_t* d_words = u.words.as<uint32_t>();
    ROUTE_TRY(st, hipMemsetAsync(d_words, 0, (words.size() + 1) * 4, st));
    k_group_count<<<route_blocks(n, kThreads), kThreads, 0, st>>>(s->tree_nodes.as<uint32_t>(), u.depth.as<uint32_t>(), n, leaf_group, d_words);
    ROUTE_TRY(st, hipGetLastError());
    ROUTE_TRY(st, hipMemcpyAsync(words.data(), d_words, words.size() * 4, hipMemcpyDeviceToHost, st));
    ROUTE_TRY(st, hipStreamSynchronize(st));
    if (words[leaf_group + 1u]) return YK_LAYOUT_REASON_DEVICE_ERROR;
    uint32_t n_levels = 0;
    for (uint32_t g = 0; g < leaf_group; ++g)
        if (words[g]) n_levels = g + 1u;
    for (uint32_t g = 0; g < n_levels; ++g)
        if (!words[g]) return YK_LAYOUT_REASON_DEVICE_ERROR;  // a level without nodes above a deeper one: not a tree
    std::vector<uint32_t> off(leaf_group + 2u, 0u);
    uint32_t run = 0;
    for (uint32_t g = 0; g <= leaf_group; ++g) {
        off[g] = run;
        run += words[g];
    }
    off[leaf_group + 1u] = run;
    if (run != n || words[leaf_group] != n - (n - 1u) / 2u) return YK_LAYOUT_REASON_DEVICE_ERROR;
    ROUTE_TRY(st, hipMemcpyAsync(d_words, off.data(), off.size() * 4, hipMemcpyHostToDevice, st));
    k_group_scatter<<<route_blocks(n, kThreads), kThreads, 0, st>>>(s->tree_nodes.as<uint32_t>(), u.depth.as<uint32_t>(), n, leaf_group, d_words, u.list.as<uint32_t>());
    ROUTE_TRY(st, hipGetLastError());
    ROUTE_TRY(st, hipMemcpyAsync(d_words, off.data(), off.size() * 4, hipMemcpyHostToDevice, st));  // the cursors become the offsets again: k_top_levels reads them
    ROUTE_TRY(st, hipStreamSynchronize(st));  // `off` is pageable
    u.level_off.assign(off.begin(), off.begin() + n_levels + 1u);
    u.level_off.push_back(off[leaf_group]);      // [n_levels + 1]: where the leaves begin ...
    u.level_off.push_back(off[leaf_group + 1]);  // [n_levels + 2]: ... and end
    u.info.n_levels = n_levels;
    u.info.plan_bytes += added;
    s->info.device_bytes += added;
    u.planned = true;
    return YK_LAYOUT_REASON_NONE;
}

}  // namespace

uint32_t plan_scene_update(yk_context* ctx, yk_scene* s) {
    (void)hipSetDevice(ctx->device);
    return s->upd.planned ? (uint32_t)YK_LAYOUT_REASON_NONE : build_plan(ctx, s);
}

uint32_t stage_points_device(yk_context* ctx, yk_scene* s, const float* d_points, uint32_t* flag) {
    *flag = 0;
    yk_scene::UpdateState& u = s->upd;
    hipStream_t st = ctx->stream;
    if (!u.planned) return YK_LAYOUT_REASON_DEVICE_ERROR;
    const size_t n_floats = 3 * (size_t)u.n_vertices;
    uint32_t* d_flag = u.words.as<uint32_t>() + (s->bvh->depth + 3u);  // behind the plan's offsets; zero between updates
    const uint32_t head = (uint32_t)std::min<size_t>(n_floats, ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(d_points) & 15u)) & 15u) / 4u);
    const size_t nvec = (n_floats - head) / 4;
    k_points_finite<<<std::max(route_blocks(nvec, kThreads), 1u), kThreads, 0, st>>>(reinterpret_cast<const uint32_t*>(d_points), n_floats, head, nvec, d_flag);
    ROUTE_TRY(st, hipGetLastError());
    ROUTE_TRY(st, hipMemcpyAsync(flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    ROUTE_TRY(st, hipStreamSynchronize(st));
    if (*flag) {
        ROUTE_TRY(st, hipMemsetAsync(d_flag, 0, 4, st));
        ROUTE_TRY(st, hipStreamSynchronize(st));
    }
    return YK_LAYOUT_REASON_NONE;
}

uint32_t commit_points_device(yk_context* ctx, yk_scene* s, const float* d_points, const float* d_normals) {
    hipStream_t st = ctx->stream;
    const size_t bytes = 12 * (size_t)s->upd.n_vertices;
    ROUTE_TRY(st, hipMemcpyAsync(s->points.p, d_points, bytes, hipMemcpyDeviceToDevice, st));
    if (d_normals) ROUTE_TRY(st, hipMemcpyAsync(s->normals.p, d_normals, bytes, hipMemcpyDeviceToDevice, st));
    return YK_LAYOUT_REASON_NONE;
}

uint32_t refit_scene_device(yk_context* ctx, yk_scene* s, bool boxes, double* seconds_boxes, double* seconds_records) {
    yk_scene::UpdateState& u = s->upd;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    if (!u.planned) return YK_LAYOUT_REASON_DEVICE_ERROR;

    // boxes: the leaves, then the levels bottom-up
    double t0 = now_seconds();
    const uint32_t n = (uint32_t)s->info.n_nodes, np = (uint32_t)s->info.n_shapes, n_levels = u.info.n_levels;
    uint32_t* nodes = s->tree_nodes.as<uint32_t>();
    if (boxes) {
        const uint32_t* list = u.list.as<uint32_t>();
        const uint32_t n_leaves = u.level_off[n_levels + 2u] - u.level_off[n_levels + 1u];
        k_leaves<<<route_blocks(n_leaves, kThreads), kThreads, 0, st>>>(nodes, list + u.level_off[n_levels + 1u], n_leaves, n, s->tree_order.as<uint32_t>(),
                                                        GeometryBound{s->points.as<float>(), s->indices.as<uint32_t>(), u.sphere_b.as<float>(), s->n_triangles, np});
        ROUTE_TRY(st, hipGetLastError());
        uint32_t n_top = 0;  // the levels at the top that one block finishes
        while (ctx->update_top_block && n_top < n_levels && u.level_off[n_top + 1u] - u.level_off[n_top] <= (uint32_t)kThreads) ++n_top;
        if (n_top < 2u) n_top = 0;  // one level is one launch either way
        for (uint32_t d = n_levels; d-- > n_top;) {
            const uint32_t count = u.level_off[d + 1u] - u.level_off[d];
            k_level<<<route_blocks(count, kThreads), kThreads, 0, st>>>(nodes, list + u.level_off[d], count, n);
        }
        if (n_top) k_top_levels<<<1, kThreads, 0, st>>>(nodes, list, u.words.as<uint32_t>(), n_top, n);
        ROUTE_TRY(st, hipGetLastError());
    }
    DeviceTree tree;  // borrowed: the buffers stay the scene's
    tree.nodes = s->tree_nodes;
    tree.depth = u.depth;
    tree.order = s->tree_order;
    tree.n_nodes = n;
    tree.n_shapes = np;
    ROUTE_TRY(st, hipMemcpyAsync(tree.root_words, nodes, 32, hipMemcpyDeviceToHost, st));
    ROUTE_TRY(st, hipStreamSynchronize(st));
    *seconds_boxes = boxes ? now_seconds() - t0 : 0.0;

    // records, by the layout's own kernels
    t0 = now_seconds();
    bool order_applied = false;
    const uint32_t r = layout_scene_device(ctx, s, tree, nullptr, u.mat_kind_d.as<uint8_t>(), s->record_bytes[YK_RECORDS_PRIM_ATTR] != 0, s->bvh->depth, &order_applied);
    if (r != YK_LAYOUT_REASON_NONE) return r;
    *seconds_records = now_seconds() - t0;
    yk_bvh_node root;
    std::memcpy(&root, tree.root_words, sizeof(root));
    for (int k = 0; k < 3; ++k) {
        s->info.bounds_min[k] = root.bmin[k];  // bind_records hands them to the kernels
        s->info.bounds_max[k] = root.bmax[k];
    }
    return YK_LAYOUT_REASON_NONE;
}

// ------------------------------------------------------------------ the host instance of the rule
extern "C" yk_status yk_bvh_refit(yk_bvh_node* nodes, size_t n_nodes, const uint32_t* shape_order, size_t n_shapes, const float* shape_bounds) {
    if (!nodes || !shape_order || !shape_bounds || n_nodes == 0 || n_nodes > YK_REF_INDEX_MAX || n_shapes > YK_REF_INDEX_MAX) return YK_ERR_INVALID_ARGUMENT;
    uint32_t* w = reinterpret_cast<uint32_t*>(nodes);
    const uint32_t n = (uint32_t)n_nodes;
    for (uint32_t i = 0; i < n; ++i) {  // every index before anything is written
        if (nd_leaf(w, i)) {
            const uint64_t first = nd_a(w, i), end = first + nd_count(w, i);
            if (end > n_shapes) return YK_ERR_INVALID_ARGUMENT;
            for (uint64_t p = first; p < end; ++p)
                if (shape_order[p] >= n_shapes) return YK_ERR_INVALID_ARGUMENT;
        } else if (i + 1u >= n || nd_a(w, i) <= i || nd_a(w, i) >= n) {
            return YK_ERR_INVALID_ARGUMENT;
        }
    }
    const TableBound bound{shape_bounds};
    for (uint32_t i = n; i-- > 0u;) {  // the array is pre-order: children follow their parent
        if (nd_leaf(w, i))
            refit_leaf(w, i, shape_order, bound);
        else
            lv::interior_bounds(w, i);
    }
    return YK_OK;
}
