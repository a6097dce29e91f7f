// yk_motion.hip — previous positions on gfx950, behind yk_surface_motion[_device]; the per-pixel arithmetic is yk_motion.h's,
// whose host instance these entry points run without a context.
//
// k_motion: one lane per pixel, a block is a 32 x 8 tile of the film (yk_film_tile.h: neighbouring lanes
//   hit neighbouring triangles, so their index and vertex requests share cache lines).  A lane reads its id (one 16-byte
//   load) and its guide (two 16-byte loads), then follows a two-hop gather: three dword index loads requested together,
//   then nine dword vertex loads requested together (a vertex is 12 bytes at a 4-byte aligned address: no wider load is
//   always legal), and writes one 16-byte record.  No load stands under a per-lane branch: a lane that is not a triangle
//   asks for triangle 0 and drops the answer.  No LDS: which vertices a tile touches is not known before the ids are read.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "yk_film_call.h"
#include "yk_film_tile.h"
#include "yk_motion.h"
#include "yk_staging.h"

namespace {

struct MoIo {
    const uint4* ids;         // one uint4 a pixel: (shape, bits of b0, b1, b2)
    const float4* guides;     // two float4 a pixel: (ns, hit), (p, t)
    const uint32_t* indices;  // the scene's own: 3 a triangle
    const float* prev_points; // 3 a vertex
    float4* out;
};
// The two sphere tables of a call with previous spheres: the scene's own DevSphere records (36 floats each, world_to_object
// at float 16, the radius at float 32) and the caller's yk_sphere_desc records (34 floats each, object_to_world first, the
// radius at float 32).  Both tables are 4-byte aligned at least: dword loads, 34 a lane, requested together.
struct MoSpheresIo {
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

// Two instantiations: MoNoSpheres is the pass as it was before spheres could move (yk_surface_motion: the same machine
// code), MoSpheresIo adds the sphere case.
template <class Spheres> __global__ __launch_bounds__(FT_TX* FT_TY) void k_motion(MoIo io, MoParams a, Spheres spheres) {
    const uint32_t x = blockIdx.x * FT_TX + threadIdx.x, y = blockIdx.y * FT_TY + threadIdx.y;
    if (x >= a.res_x || y >= a.res_y) return;
    const size_t i = (size_t)y * a.res_x + x;
    const uint4 id = io.ids[i];
    const float4 ga = io.guides[2 * i], gb = io.guides[2 * i + 1];
    const float p[3] = {gb.x, gb.y, gb.z};
    float rec[4];
    mo_pixel(a, id.x, __uint_as_float(id.y), __uint_as_float(id.z), __uint_as_float(id.w), ga.w, p,
             [&](size_t k) { return io.indices[k]; },
             [&](uint32_t v) { return V3{io.prev_points[3 * (size_t)v], io.prev_points[3 * (size_t)v + 1], io.prev_points[3 * (size_t)v + 2]}; }, spheres, rec);
    io.out[i] = make_float4(rec[0], rec[1], rec[2], rec[3]);
}

// prev_points may be NULL only with a previous sphere table, for a scene without triangles
yk_status check_call(const yk_scene* scene, const void* ids, const void* guides, const float* prev_points, const void* prev_spheres, uint16_t res_x, uint16_t res_y, const void* out) {
    if (!scene || !ids || !guides || !out || res_x == 0 || res_y == 0) return YK_ERR_INVALID_ARGUMENT;
    if (!prev_points && (!prev_spheres || scene->n_triangles != 0u)) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y;
    if (overlaps(out, n_px * sizeof(yk_motion), ids, n_px * sizeof(yk_surface_id)) || overlaps(out, n_px * sizeof(yk_motion), guides, n_px * sizeof(yk_guide)) ||
        (prev_points && overlaps(out, n_px * sizeof(yk_motion), prev_points, (size_t)scene->upd.n_vertices * 12)) ||
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

// d_prev_spheres NULL: the pass without the sphere case
yk_status enqueue(yk_context* ctx, hipStream_t st, const yk_scene* scene, const void* ids, const void* guides, const float* prev_points, const void* d_prev_spheres, uint16_t res_x, uint16_t res_y,
                  void* out) {
    const MoParams a = make_params(scene, res_x, res_y);
    MoIo io{reinterpret_cast<const uint4*>(ids), reinterpret_cast<const float4*>(guides), scene->dev.indices, prev_points, reinterpret_cast<float4*>(out)};
    if (d_prev_spheres)
        hipLaunchKernelGGL(k_motion<MoSpheresIo>, ft_grid(res_x, res_y), ft_block(), 0, st, io, a, MoSpheresIo{reinterpret_cast<const float*>(scene->dev.spheres), reinterpret_cast<const float*>(d_prev_spheres)});
    else
        hipLaunchKernelGGL(k_motion<MoNoSpheres>, ft_grid(res_x, res_y), ft_block(), 0, st, io, a, MoNoSpheres{});
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

// current: the scene's DevSphere table on the host (prev_spheres given), or NULL
void motion_host(const yk_scene* scene, const uint32_t* indices, const yk_surface_id* ids, const yk_guide* guides, const float* prev_points, const DevSphere* current, const yk_sphere_desc* prev_spheres,
                 uint16_t res_x, uint16_t res_y, yk_motion* out) {
    const MoParams a = make_params(scene, res_x, res_y);
    const auto index = [&](size_t k) { return indices[k]; };
    const auto point = [&](uint32_t v) { return V3{prev_points[3 * (size_t)v], prev_points[3 * (size_t)v + 1], prev_points[3 * (size_t)v + 2]}; };
    const MoSpheresIo spheres{reinterpret_cast<const float*>(current), reinterpret_cast<const float*>(prev_spheres)};
    const size_t n_px = (size_t)res_x * res_y;
    for (size_t i = 0; i < n_px; ++i) {
        float rec[4];
        if (prev_spheres)
            mo_pixel(a, ids[i].shape, ids[i].b[0], ids[i].b[1], ids[i].b[2], guides[i].hit, guides[i].p, index, point, spheres, rec);
        else
            mo_pixel(a, ids[i].shape, ids[i].b[0], ids[i].b[1], ids[i].b[2], guides[i].hit, guides[i].p, index, point, MoNoSpheres{}, rec);
        std::memcpy(&out[i], rec, 16);
    }
}

// both host-array entry points; prev_spheres NULL is yk_surface_motion
yk_status surface_motion(yk_context* ctx, const yk_scene* scene, const yk_surface_id* ids, const yk_guide* guides, const float* prev_points, const yk_sphere_desc* prev_spheres, uint16_t res_x,
                         uint16_t res_y, yk_motion* out, const char* name) {
    if (check_call(scene, ids, guides, prev_points, prev_spheres, res_x, res_y, out) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + ": bad argument");
    if (scene->n_spheres == 0u) prev_spheres = nullptr;  // nothing to read of it
    const size_t n_px = (size_t)res_x * res_y;
    if (!ctx) {  // the host instance
        HostArrays h;  // a scene in device memory: its indices and its sphere table live there
        if (yk_status rs = scene_host_arrays(ctx, scene, HOST_INDICES | (prev_spheres ? HOST_SPHERES : 0u), std::string(name) + ": ", h)) return rs;
        motion_host(scene, h->indices.data(), ids, guides, prev_points, h->spheres.data(), prev_spheres, res_x, res_y, out);
        return YK_OK;
    }
    YK_LOCK(ctx);
    if (yk_status rs = scene_on_context(ctx, scene, name)) return rs;
    Staging sg(ctx);
    const yk_surface_id* d_ids = sg.upload(ids, n_px);
    const yk_guide* d_guides = sg.upload(guides, n_px);
    const float* d_points = sg.upload(prev_points, (size_t)scene->upd.n_vertices * 3);
    const yk_sphere_desc* d_spheres = prev_spheres ? sg.upload(prev_spheres, scene->n_spheres) : nullptr;
    yk_motion* d_out = sg.output(out, n_px);
    return sg.run([&] { return enqueue(ctx, sg.stream, scene, d_ids, d_guides, d_points, d_spheres, res_x, res_y, d_out); });
}

yk_status surface_motion_device(yk_context* ctx, const yk_scene* scene, const void* d_ids, const void* d_guides, const float* d_prev_points, const void* d_prev_spheres, uint16_t res_x, uint16_t res_y,
                                void* d_out, void* stream, const char* name) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_call(scene, d_ids, d_guides, d_prev_points, d_prev_spheres, res_x, res_y, d_out) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + ": bad argument");
    if (yk_status rs = scene_on_context(ctx, scene, name)) return rs;
    // 16-byte loads and stores of the records and the guides, dword loads of the vertices and of the sphere records
    if (misaligned(16, d_ids, d_guides, d_out) || misaligned(4, d_prev_points) || misaligned(4, d_prev_spheres))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + ": ids, guides and output must be 16-byte aligned, prev_points 4-byte aligned");
    return enqueue(ctx, device_call_stream(ctx, stream), scene, d_ids, d_guides, d_prev_points, scene->n_spheres ? d_prev_spheres : nullptr, res_x, res_y, d_out);
}

}  // namespace

extern "C" {

yk_status yk_surface_motion(yk_context* ctx, const yk_scene* scene, const yk_surface_id* ids, const yk_guide* guides, const float* prev_points, uint16_t res_x, uint16_t res_y,
                            yk_motion* out) try {
    return surface_motion(ctx, scene, ids, guides, prev_points, nullptr, res_x, res_y, out, "yk_surface_motion");
}
YK_CATCH(ctx)

yk_status yk_surface_motion_device(yk_context* ctx, const yk_scene* scene, const void* d_ids, const void* d_guides, const float* d_prev_points, uint16_t res_x, uint16_t res_y, void* d_out,
                                   void* stream) {
    return surface_motion_device(ctx, scene, d_ids, d_guides, d_prev_points, nullptr, res_x, res_y, d_out, stream, "yk_surface_motion_device");
}

yk_status yk_surface_motion_spheres(yk_context* ctx, const yk_scene* scene, const yk_surface_id* ids, const yk_guide* guides, const float* prev_points, const yk_sphere_desc* prev_spheres,
                                    uint16_t res_x, uint16_t res_y, yk_motion* out) try {
    return surface_motion(ctx, scene, ids, guides, prev_points, prev_spheres, res_x, res_y, out, "yk_surface_motion_spheres");
}
YK_CATCH(ctx)

yk_status yk_surface_motion_spheres_device(yk_context* ctx, const yk_scene* scene, const void* d_ids, const void* d_guides, const float* d_prev_points, const void* d_prev_spheres, uint16_t res_x,
                                           uint16_t res_y, void* d_out, void* stream) {
    return surface_motion_device(ctx, scene, d_ids, d_guides, d_prev_points, d_prev_spheres, res_x, res_y, d_out, stream, "yk_surface_motion_spheres_device");
}

}  // extern "C"
