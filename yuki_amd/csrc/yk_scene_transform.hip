// yk_scene_transform.hip — yk_scene_transform[_device] on gfx950 (the rule: yk_scene_transform.h), the tree cost, and the
// motion pass that works from matrices (yk_surface_motion_transforms[_device]).  Streaming kernels, one element a lane, 256
// lanes a block; the route's steps are called by yk_scene_change.cpp, which runs yk_scene_update's refit and records after them.
//   k_xf_table_init / k_xf_table / k_xf_shared   once per rest pose: the table vertex -> mesh by integer atomicMin / atomicMax into
//                      two words a vertex (order-independent, hence deterministic), the meshes that carry an area light,
//                      and whether a vertex is shared by two meshes
//   k_xf_meshes        one lane a mesh: the kind of its record, the record's refusals, the counts of moved and flipped meshes
//   k_xf_check         one lane a vertex: computes the result and sets only the flag word — nothing of the scene is written
//   k_xf_write         computes again and writes points and normals: the arithmetic is deterministic, so the two passes agree
//                      and no third copy of the geometry is staged.  20 or 32 bytes a vertex in (8 of the table, 12 of the point,
//                      12 of the normal) and 12 or 24 out; a moved vertex reads its mesh's record, which a block's lanes share
//   k_xf_flags         one lane a mesh: creation's flags with YK_MESH_SWAPS flipped where the record mirrors
//   k_cost_blocks / k_cost_final   the tree cost: every block reduces its nodes' two terms in LDS in a fixed order, one block adds
//                      the partial sums in a fixed order and divides: the same bits on every call
//   k_motion_xf        k_motion (yk_motion.hip) with one more hop: the triangle's mesh, its previous record (64 bytes), and
//                      the three REST points through that record.  The gather discipline is mo_pixel's: the range test stands
//                      before the first dependent load, and no load sits under a per-lane branch.
// Every index a kernel follows is either bounded by the launch (a lane's own element) or tested against its array's length
// before the load or store.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "yk_film_call.h"
#include "yk_film_tile.h"
#include "yk_motion.h"
#include "yk_scene_route.h"
#include "yk_scene_transform.h"
#include "yk_staging.h"

using namespace yk::xfm;

namespace {

const int kThreads = 256;

__global__ void __launch_bounds__(kThreads) k_xf_table_init(uint32_t* vertex_mesh, size_t n_words) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n_words) vertex_mesh[i] = (i & 1u) ? 0u : XF_NO_MESH;
}

__global__ void __launch_bounds__(kThreads) k_xf_table(const uint32_t* __restrict__ indices, const uint32_t* __restrict__ tri_mesh, const int32_t* __restrict__ tri_area_light, uint32_t n_triangles,
                                                       uint32_t n_vertices, uint32_t n_meshes, uint32_t* vertex_mesh, uint32_t* mesh_lit) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= n_triangles) return;
    const uint32_t mesh = tri_mesh[t];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t v = indices[3 * (size_t)t + k];
        if (v >= n_vertices) continue;  // cannot happen (creation checked): guards the stores
        atomicMin(&vertex_mesh[2 * (size_t)v], mesh);
        atomicMax(&vertex_mesh[2 * (size_t)v + 1], mesh);
    }
    if (tri_area_light[t] >= 0 && mesh < n_meshes) atomicOr(&mesh_lit[mesh], 1u);
}

__global__ void __launch_bounds__(kThreads) k_xf_shared(const uint32_t* __restrict__ vertex_mesh, uint32_t n_vertices, uint32_t* flag) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= n_vertices) return;
    const uint2 w = reinterpret_cast<const uint2*>(vertex_mesh)[v];
    if (vertex_shared(w.x, w.y)) atomicOr(flag, XF_BAD_SHARED);
}

// words: the flag, the moved meshes, the flipped meshes
__global__ void __launch_bounds__(kThreads) k_xf_meshes(const float* __restrict__ records, const uint32_t* __restrict__ mesh_lit, uint32_t n_meshes, uint32_t* kinds, uint32_t* words) {
    const uint32_t m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= n_meshes) return;
    float rec[XF_RECORD_FLOATS];
#pragma unroll
    for (int k = 0; k < XF_RECORD_FLOATS; ++k) rec[k] = records[XF_RECORD_FLOATS * (size_t)m + k];
    uint32_t bad;
    const uint32_t kind = mesh_kind(rec, mesh_lit[m] != 0u, &bad);
    kinds[m] = kind;
    if (bad) atomicOr(&words[0], bad);
    if (kind & XF_MOVED) atomicAdd(&words[1], 1u);
    if (kind & XF_FLIPS) atomicAdd(&words[2], 1u);
}

struct XfIo {
    const float* rest_points;
    const float* rest_normals;  // NULL: the scene has no normals array
    const uint32_t* vertex_mesh;
    const float* records;
    const uint32_t* kinds;
    uint32_t n_vertices, n_meshes;
};
__device__ V3 ld3f(const float* p, size_t v) { return V3{p[3 * v], p[3 * v + 1], p[3 * v + 2]}; }

__global__ void __launch_bounds__(kThreads) k_xf_check(XfIo io, uint32_t* flag) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= io.n_vertices) return;
    const uint32_t mesh = io.vertex_mesh[2 * (size_t)v];
    if (!vertex_moves(io.kinds, io.n_meshes, mesh)) return;  // the rest pose's bits: what the scene was given
    if (point_not_finite(vertex_point(io.records, io.kinds, io.n_meshes, mesh, ld3f(io.rest_points, v)))) atomicOr(flag, XF_BAD_POINT);
}

__global__ void __launch_bounds__(kThreads) k_xf_write(XfIo io, float* points, float* normals) {
    const uint32_t v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= io.n_vertices) return;
    const uint32_t mesh = io.vertex_mesh[2 * (size_t)v];
    const V3 p = vertex_point(io.records, io.kinds, io.n_meshes, mesh, ld3f(io.rest_points, v));
    points[3 * (size_t)v] = p.x;
    points[3 * (size_t)v + 1] = p.y;
    points[3 * (size_t)v + 2] = p.z;
    if (io.rest_normals) {
        const V3 n = vertex_normal(io.records, io.kinds, io.n_meshes, mesh, ld3f(io.rest_normals, v));
        normals[3 * (size_t)v] = n.x;
        normals[3 * (size_t)v + 1] = n.y;
        normals[3 * (size_t)v + 2] = n.z;
    }
}

__global__ void __launch_bounds__(kThreads) k_xf_flags(const uint32_t* __restrict__ created, const uint32_t* __restrict__ kinds, uint32_t n_meshes, uint32_t* mesh_flags) {
    const uint32_t m = blockIdx.x * kThreads + threadIdx.x;
    if (m < n_meshes) mesh_flags[m] = mesh_flags_of(created[m], kinds[m]);
}

// ---- tree cost
__device__ void block_sum(double (&a)[kThreads], double (&b)[kThreads]) {  // a fixed tree: the same order on every call
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < half) {
            a[threadIdx.x] += a[threadIdx.x + half];
            b[threadIdx.x] += b[threadIdx.x + half];
        }
    }
    __syncthreads();
}
__global__ void __launch_bounds__(kThreads) k_cost_blocks(const uint32_t* __restrict__ nodes, uint32_t n_nodes, double* partial) {
    __shared__ double a[kThreads], b[kThreads];
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    double interior = 0.0, leaf = 0.0;
    if (i < n_nodes) cost_term(nodes, i, &interior, &leaf);
    a[threadIdx.x] = interior;
    b[threadIdx.x] = leaf;
    block_sum(a, b);
    if (threadIdx.x == 0) {
        partial[2 * (size_t)blockIdx.x] = a[0];
        partial[2 * (size_t)blockIdx.x + 1] = b[0];
    }
}
// one block; out[0] = the cost
__global__ void __launch_bounds__(kThreads) k_cost_final(const double* __restrict__ partial, uint32_t n_blocks, const uint32_t* __restrict__ nodes, double* out) {
    __shared__ double a[kThreads], b[kThreads];
    double interior = 0.0, leaf = 0.0;
    for (uint32_t k = threadIdx.x; k < n_blocks; k += kThreads) {
        interior += partial[2 * (size_t)k];
        leaf += partial[2 * (size_t)k + 1];
    }
    a[threadIdx.x] = interior;
    b[threadIdx.x] = leaf;
    block_sum(a, b);
    if (threadIdx.x == 0) out[0] = cost_of(a[0], b[0], node_area(nodes, 0u));
}

// ---- what yk_scene::TransformState keeps in HBM.  mesh_words: per mesh its lit bit, its kind of the call in progress and its
// flags as creation made them (three runs of max(n_meshes, 1) words), then the four words the stage reads back.
uint32_t mesh_run(const yk_scene* s) { return std::max<uint32_t>(s->n_meshes, 1u); }
uint32_t* lit_of(const yk_scene* s) { return s->xf.mesh_words.as<uint32_t>(); }
uint32_t* kinds_of(const yk_scene* s) { return lit_of(s) + mesh_run(s); }
uint32_t* created_of(const yk_scene* s) { return lit_of(s) + 2 * (size_t)mesh_run(s); }
uint32_t* words_of(const yk_scene* s) { return lit_of(s) + 3 * (size_t)mesh_run(s); }
uint32_t cost_blocks(const yk_scene* s) { return std::max(route_blocks((size_t)s->info.n_nodes, kThreads), 1u); }
size_t kept_bytes(const yk_scene* s) {
    const yk_scene::TransformState& x = s->xf;
    return x.rest_points.bytes + x.rest_normals.bytes + x.vertex_mesh.bytes + x.mesh_words.bytes + x.cost_words.bytes;
}
void release_kept(yk_scene* s) {
    for (DevBuf* b : {&s->xf.rest_points, &s->xf.rest_normals, &s->xf.vertex_mesh, &s->xf.mesh_words, &s->xf.cost_words}) b->release();
}

uint32_t snapshot(yk_context* ctx, yk_scene* s, bool tree_on_device) {
    yk_scene::TransformState& x = s->xf;
    hipStream_t st = ctx->stream;
    const uint32_t nv = s->upd.n_vertices, nt = s->n_triangles, run = mesh_run(s);
    const size_t bytes = 12 * (size_t)nv;
    ROUTE_TRY(st, x.rest_points.ensure(std::max<size_t>(bytes, 16)));
    if (s->upd.has_normals) ROUTE_TRY(st, x.rest_normals.ensure(std::max<size_t>(bytes, 16)));
    ROUTE_TRY(st, x.vertex_mesh.ensure(std::max<size_t>(8 * (size_t)nv, 16)));
    ROUTE_TRY(st, x.mesh_words.ensure((3 * (size_t)run + 4) * 4));
    ROUTE_TRY(st, x.cost_words.ensure((2 * (size_t)cost_blocks(s) + 2) * 8));
    if (bytes) ROUTE_TRY(st, hipMemcpyAsync(x.rest_points.p, s->points.p, bytes, hipMemcpyDeviceToDevice, st));
    if (bytes && s->upd.has_normals) ROUTE_TRY(st, hipMemcpyAsync(x.rest_normals.p, s->normals.p, bytes, hipMemcpyDeviceToDevice, st));
    ROUTE_TRY(st, hipMemsetAsync(x.mesh_words.p, 0, x.mesh_words.bytes, st));
    // no rest pose yet: the scene's flags are creation's (yk_scene_update* resets them)
    ROUTE_TRY(st, hipMemcpyAsync(created_of(s), s->mesh_flags.p, 4 * (size_t)run, hipMemcpyDeviceToDevice, st));
    if (nv) k_xf_table_init<<<route_blocks(2 * (size_t)nv, kThreads), kThreads, 0, st>>>(x.vertex_mesh.as<uint32_t>(), 2 * (size_t)nv);
    if (nt)
        k_xf_table<<<route_blocks(nt, kThreads), kThreads, 0, st>>>(s->indices.as<uint32_t>(), s->tri_mesh.as<uint32_t>(), s->tri_area_light.as<int32_t>(), nt, nv, s->n_meshes, x.vertex_mesh.as<uint32_t>(), lit_of(s));
    if (nv) k_xf_shared<<<route_blocks(nv, kThreads), kThreads, 0, st>>>(x.vertex_mesh.as<uint32_t>(), nv, words_of(s));
    ROUTE_TRY(st, hipGetLastError());
    uint32_t flag = 0;
    ROUTE_TRY(st, hipMemcpyAsync(&flag, words_of(s), 4, hipMemcpyDeviceToHost, st));
    ROUTE_TRY(st, hipMemsetAsync(words_of(s), 0, 16, st));
    ROUTE_TRY(st, hipStreamSynchronize(st));
    x.shared = (flag & XF_BAD_SHARED) != 0u;
    if (tree_on_device) {
        const uint32_t r = tree_cost_device(ctx, s, &x.info.tree_cost_rest);
        if (r != YK_LAYOUT_REASON_NONE) return r;
    } else {  // a host-laid scene on the host route: its tree is on the host, and current
        const HostBvh* bvh = scene_host_tree(s);
        if (!bvh) return YK_LAYOUT_REASON_DEVICE_ERROR;
        x.info.tree_cost_rest = tree_cost(reinterpret_cast<const uint32_t*>(bvh->nodes.data()), bvh->nodes.size());
    }
    x.info.rest_bytes = kept_bytes(s);
    s->info.device_bytes += kept_bytes(s);
    x.active = true;
    return YK_LAYOUT_REASON_NONE;
}

XfIo make_io(const yk_scene* s, const void* d_transforms) {
    XfIo io;
    io.rest_points = s->xf.rest_points.as<float>();
    io.rest_normals = s->upd.has_normals ? s->xf.rest_normals.as<float>() : nullptr;
    io.vertex_mesh = s->xf.vertex_mesh.as<uint32_t>();
    io.records = reinterpret_cast<const float*>(d_transforms);
    io.kinds = kinds_of(s);
    io.n_vertices = s->upd.n_vertices;
    io.n_meshes = s->n_meshes;
    return io;
}

}  // namespace

uint32_t snapshot_rest_device(yk_context* ctx, yk_scene* s, bool tree_on_device) {
    (void)hipSetDevice(ctx->device);
    if (s->xf.active) return YK_LAYOUT_REASON_NONE;
    const uint32_t r = snapshot(ctx, s, tree_on_device);
    if (r != YK_LAYOUT_REASON_NONE) release_kept(s);
    return r;
}

uint32_t tree_cost_device(yk_context* ctx, yk_scene* s, double* cost) {
    hipStream_t st = ctx->stream;
    const uint32_t n = (uint32_t)s->info.n_nodes, n_blocks = cost_blocks(s);
    if (!s->tree_nodes.p || n == 0 || s->xf.cost_words.bytes < (2 * (size_t)n_blocks + 2) * 8) return YK_LAYOUT_REASON_DEVICE_ERROR;
    double* partial = s->xf.cost_words.as<double>();
    double* out = partial + 2 * (size_t)n_blocks;
    k_cost_blocks<<<n_blocks, kThreads, 0, st>>>(s->tree_nodes.as<uint32_t>(), n, partial);
    k_cost_final<<<1, kThreads, 0, st>>>(partial, n_blocks, s->tree_nodes.as<uint32_t>(), out);
    ROUTE_TRY(st, hipGetLastError());
    ROUTE_TRY(st, hipMemcpyAsync(cost, out, 8, hipMemcpyDeviceToHost, st));
    ROUTE_TRY(st, hipStreamSynchronize(st));
    return YK_LAYOUT_REASON_NONE;
}

uint32_t stage_transforms_device(yk_context* ctx, yk_scene* s, const void* d_transforms, uint32_t* flag, uint32_t* counts) {
    *flag = counts[0] = counts[1] = 0;
    hipStream_t st = ctx->stream;
    if (!s->xf.active || !s->xf.rest_points.p) return YK_LAYOUT_REASON_DEVICE_ERROR;
    const XfIo io = make_io(s, d_transforms);
    uint32_t* words = words_of(s);  // zero between calls
    if (io.n_meshes) k_xf_meshes<<<route_blocks(io.n_meshes, kThreads), kThreads, 0, st>>>(io.records, lit_of(s), io.n_meshes, kinds_of(s), words);
    if (io.n_vertices && io.n_meshes) k_xf_check<<<route_blocks(io.n_vertices, kThreads), kThreads, 0, st>>>(io, words);
    ROUTE_TRY(st, hipGetLastError());
    uint32_t got[4] = {};
    ROUTE_TRY(st, hipMemcpyAsync(got, words, 16, hipMemcpyDeviceToHost, st));
    ROUTE_TRY(st, hipMemsetAsync(words, 0, 16, st));
    ROUTE_TRY(st, hipStreamSynchronize(st));
    *flag = got[0] | (s->xf.shared ? (uint32_t)XF_BAD_SHARED : 0u);
    counts[0] = got[1];
    counts[1] = got[2];
    return YK_LAYOUT_REASON_NONE;
}

uint32_t commit_transforms_device(yk_context* ctx, yk_scene* s, const void* d_transforms) {
    hipStream_t st = ctx->stream;
    const XfIo io = make_io(s, d_transforms);
    if (io.n_vertices) k_xf_write<<<route_blocks(io.n_vertices, kThreads), kThreads, 0, st>>>(io, s->points.as<float>(), s->normals.as<float>());
    if (io.n_meshes) k_xf_flags<<<route_blocks(io.n_meshes, kThreads), kThreads, 0, st>>>(created_of(s), kinds_of(s), io.n_meshes, s->mesh_flags.as<uint32_t>());
    ROUTE_TRY(st, hipGetLastError());
    return YK_LAYOUT_REASON_NONE;
}

yk_status drop_rest(yk_context* ctx, yk_scene* s) {
    yk_scene::TransformState& x = s->xf;
    if (!x.active) return YK_OK;
    if (s->on_device) {  // creation's flags are kept beside the rest pose
        HIP_TRY(ctx, hipMemcpy(s->mesh_flags.p, created_of(s), 4 * (size_t)mesh_run(s), hipMemcpyDeviceToDevice));
        s->info.device_bytes -= kept_bytes(s);
        release_kept(s);
    } else {
        s->host.mesh_flags = x.flags_created;
    }
    x.h_rest_points = std::vector<float>();
    x.h_vertex_mesh = std::vector<uint32_t>();
    x.h_mesh_lit = std::vector<uint32_t>();
    x.flags_created = std::vector<uint32_t>();
    x.active = x.shared = false;
    x.info.rest_bytes = 0;
    return YK_OK;
}

// ------------------------------------------------------------------ motion from matrices
namespace {

struct MoXfIo {
    const uint4* ids;          // one uint4 a pixel: (shape, bits of b0, b1, b2)
    const float4* guides;      // two float4 a pixel: (ns, hit), (p, t)
    const uint32_t* indices;   // the scene's own: 3 a triangle
    const uint32_t* tri_mesh;  // the scene's own: 1 a triangle
    const float* rest_points;  // the rest pose (the scene's own points where it was never transformed)
    const float* prev;         // the previous records, 32 floats a mesh; NULL: the scene stood at rest
    uint32_t n_meshes;
    float4* out;
};
// the two sphere tables, as yk_motion.hip reads them
struct MoXfSpheres {
    const float* current;
    const float* prev;
    YK_HD MoSphere operator()(uint32_t k) const {
        const float* c = current + (sizeof(DevSphere) / 4) * (size_t)k;
        const float* p = prev + (sizeof(yk_sphere_desc) / 4) * (size_t)k;
        MoSphere r;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            r.w2o[i] = c[16 + i];
            r.o2w_prev[i] = p[i];
        }
        r.radius = c[32];
        r.radius_prev = p[32];
        return r;
    }
};

// One pixel: mo_pixel with P'[i] = the rest point i under the previous record of the triangle's mesh.  The record is asked for
// after the range test and by every lane alike (triangle 0's where the lane is no triangle; mesh 0's where the mesh is out of
// range, which creation refused); nothing is loaded for a scene without triangles, or of a table the call does not have.
template <class Spheres> YK_HD void mo_xf_pixel(const MoParams& a, const MoXfIo& io, uint32_t shape, float b0, float b1, float b2, float hit, const float* p, const Spheres& spheres, float* out) {
    const bool tri = shape != YK_SURFACE_NONE && hit != 0.0f && shape < a.n_shapes && shape < a.n_triangles;
    float m[16] = {};
    bool identity = true;
    if (a.n_triangles != 0u && io.prev && io.n_meshes != 0u) {
        const uint32_t mesh = io.tri_mesh[tri ? (size_t)shape : (size_t)0];
        const float* rec = io.prev + XF_RECORD_FLOATS * (size_t)(mesh < io.n_meshes ? mesh : 0u);
#pragma unroll
        for (int k = 0; k < 16; ++k) m[k] = rec[k];
        identity = is_identity(m);
    }
    mo_pixel(a, shape, b0, b1, b2, hit, p, [&](size_t k) { return io.indices[k]; },
             [&](uint32_t v) { return point_under(m, identity, V3{io.rest_points[3 * (size_t)v], io.rest_points[3 * (size_t)v + 1], io.rest_points[3 * (size_t)v + 2]}); }, spheres, out);
}

template <class Spheres> __global__ __launch_bounds__(FT_TX* FT_TY) void k_motion_xf(MoXfIo io, MoParams a, Spheres spheres) {
    const uint32_t x = blockIdx.x * FT_TX + threadIdx.x, y = blockIdx.y * FT_TY + threadIdx.y;
    if (x >= a.res_x || y >= a.res_y) return;
    const size_t i = (size_t)y * a.res_x + x;
    const uint4 id = io.ids[i];
    const float4 ga = io.guides[2 * i], gb = io.guides[2 * i + 1];
    const float p[3] = {gb.x, gb.y, gb.z};
    float rec[4];
    mo_xf_pixel(a, io, id.x, __uint_as_float(id.y), __uint_as_float(id.z), __uint_as_float(id.w), ga.w, p, spheres, rec);
    io.out[i] = make_float4(rec[0], rec[1], rec[2], rec[3]);
}

yk_status check_call(const yk_scene* scene, const void* ids, const void* guides, const void* prev_transforms, const void* prev_spheres, uint16_t res_x, uint16_t res_y, const void* out) {
    if (!scene || !ids || !guides || !out || res_x == 0 || res_y == 0) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y;
    if (overlaps(out, n_px * sizeof(yk_motion), ids, n_px * sizeof(yk_surface_id)) || overlaps(out, n_px * sizeof(yk_motion), guides, n_px * sizeof(yk_guide)) ||
        (prev_transforms && overlaps(out, n_px * sizeof(yk_motion), prev_transforms, (size_t)scene->n_meshes * sizeof(yk_mesh_transform))) ||
        (prev_spheres && overlaps(out, n_px * sizeof(yk_motion), prev_spheres, (size_t)scene->n_spheres * sizeof(yk_sphere_desc))))
        return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

MoParams make_params(const yk_scene* scene, uint16_t res_x, uint16_t res_y) {
    MoParams a{};
    a.res_x = res_x;
    a.res_y = res_y;
    a.n_triangles = scene->n_triangles;
    a.n_shapes = scene->n_triangles + scene->n_spheres;
    return a;
}

yk_status enqueue(yk_context* ctx, hipStream_t st, const yk_scene* scene, const void* ids, const void* guides, const void* d_prev, const void* d_prev_spheres, uint16_t res_x, uint16_t res_y, void* out) {
    const MoParams a = make_params(scene, res_x, res_y);
    const bool kept = scene->xf.active;  // a scene in device memory keeps its rest pose there, whichever route made it
    MoXfIo io{reinterpret_cast<const uint4*>(ids), reinterpret_cast<const float4*>(guides), scene->dev.indices, scene->tri_mesh.as<uint32_t>(), kept ? scene->xf.rest_points.as<float>() : scene->points.as<float>(),
              reinterpret_cast<const float*>(d_prev), scene->n_meshes, reinterpret_cast<float4*>(out)};
    if (d_prev_spheres)
        hipLaunchKernelGGL(k_motion_xf<MoXfSpheres>, ft_grid(res_x, res_y), ft_block(), 0, st, io, a, MoXfSpheres{reinterpret_cast<const float*>(scene->dev.spheres), reinterpret_cast<const float*>(d_prev_spheres)});
    else
        hipLaunchKernelGGL(k_motion_xf<MoNoSpheres>, ft_grid(res_x, res_y), ft_block(), 0, st, io, a, MoNoSpheres{});
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

// the rest pose on the host, wherever the scene keeps it
yk_status rest_points_host(const yk_scene* scene, const HostArrays& h, std::vector<float>& fetched, const float** out) {
    const yk_scene::TransformState& x = scene->xf;
    *out = h->points.data();
    if (!x.active) return YK_OK;
    if (!scene->on_device) {
        *out = x.h_rest_points.data();
        return YK_OK;
    }
    fetched.resize(3 * (size_t)scene->upd.n_vertices);
    *out = fetched.data();
    (void)hipSetDevice(scene->device);
    if (!fetched.empty() && hipMemcpy(fetched.data(), x.rest_points.p, fetched.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return YK_ERR_DEVICE;
    }
    return YK_OK;
}

yk_status motion_transforms(yk_context* ctx, const yk_scene* scene, const yk_surface_id* ids, const yk_guide* guides, const yk_mesh_transform* prev, const yk_sphere_desc* prev_spheres, uint16_t res_x,
                            uint16_t res_y, yk_motion* out) {
    const char* name = "yk_surface_motion_transforms";
    if (check_call(scene, ids, guides, prev, prev_spheres, res_x, res_y, out) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + ": bad argument");
    if (scene->n_spheres == 0u) prev_spheres = nullptr;  // nothing to read of it
    const size_t n_px = (size_t)res_x * res_y;
    if (!ctx) {  // the host instance
        const bool kept = scene->xf.active;
        HostArrays h;
        if (yk_status rs = scene_host_arrays(ctx, scene, HOST_INDICES | HOST_TRI_MESH | (kept ? 0u : HOST_POINTS) | (prev_spheres ? HOST_SPHERES : 0u), std::string(name) + ": ", h)) return rs;
        std::vector<float> fetched;
        const float* rest = nullptr;
        if (yk_status rs = rest_points_host(scene, h, fetched, &rest)) return fail(ctx, rs, std::string(name) + ": the rest pose could not be copied back from the device");
        const MoParams a = make_params(scene, res_x, res_y);
        const MoXfIo io{nullptr, nullptr, h->indices.data(), h->tri_mesh.data(), rest, reinterpret_cast<const float*>(prev), scene->n_meshes, nullptr};
        const MoXfSpheres spheres{reinterpret_cast<const float*>(h->spheres.data()), reinterpret_cast<const float*>(prev_spheres)};
        for (size_t i = 0; i < n_px; ++i) {
            float rec[4];
            if (prev_spheres)
                mo_xf_pixel(a, io, ids[i].shape, ids[i].b[0], ids[i].b[1], ids[i].b[2], guides[i].hit, guides[i].p, spheres, rec);
            else
                mo_xf_pixel(a, io, ids[i].shape, ids[i].b[0], ids[i].b[1], ids[i].b[2], guides[i].hit, guides[i].p, MoNoSpheres{}, rec);
            std::memcpy(&out[i], rec, 16);
        }
        return YK_OK;
    }
    YK_LOCK(ctx);
    if (yk_status rs = scene_on_context(ctx, scene, name)) return rs;
    Staging sg(ctx);
    const yk_surface_id* d_ids = sg.upload(ids, n_px);
    const yk_guide* d_guides = sg.upload(guides, n_px);
    const yk_mesh_transform* d_prev = prev ? sg.upload(prev, scene->n_meshes) : nullptr;
    const yk_sphere_desc* d_spheres = prev_spheres ? sg.upload(prev_spheres, scene->n_spheres) : nullptr;
    yk_motion* d_out = sg.output(out, n_px);
    return sg.run([&] { return enqueue(ctx, sg.stream, scene, d_ids, d_guides, d_prev, d_spheres, res_x, res_y, d_out); });
}

}  // namespace

extern "C" {

yk_status yk_surface_motion_transforms(yk_context* ctx, const yk_scene* scene, const yk_surface_id* ids, const yk_guide* guides, const yk_mesh_transform* prev_transforms,
                                       const yk_sphere_desc* prev_spheres, uint16_t res_x, uint16_t res_y, yk_motion* out) try {
    return motion_transforms(ctx, scene, ids, guides, prev_transforms, prev_spheres, res_x, res_y, out);
}
YK_CATCH(ctx)

yk_status yk_surface_motion_transforms_device(yk_context* ctx, const yk_scene* scene, const void* d_ids, const void* d_guides, const void* d_prev_transforms, const void* d_prev_spheres, uint16_t res_x,
                                              uint16_t res_y, void* d_out, void* stream) {
    const char* name = "yk_surface_motion_transforms_device";
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_call(scene, d_ids, d_guides, d_prev_transforms, d_prev_spheres, res_x, res_y, d_out) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + ": bad argument");
    if (yk_status rs = scene_on_context(ctx, scene, name)) return rs;
    // 16-byte loads and stores of the records and the guides, dword loads of the matrices and of the sphere records
    if (misaligned(16, d_ids, d_guides, d_out) || misaligned(4, d_prev_transforms) || misaligned(4, d_prev_spheres))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + ": ids, guides and output must be 16-byte aligned, prev_transforms 4-byte aligned");
    return enqueue(ctx, device_call_stream(ctx, stream), scene, d_ids, d_guides, d_prev_transforms, scene->n_spheres ? d_prev_spheres : nullptr, res_x, res_y, d_out);
}

}  // extern "C"
