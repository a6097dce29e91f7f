// yk_albedo.hip — first-hit albedo on gfx950, behind yk_surface_albedo[_device], and its mean over a pixel, behind
// yk_albedo_mean[_device] and the bands of yk_render_albedo_mean (driven from yk_render.cpp); the per-pixel rules are
// yk_albedo.h's, whose host instances these entry points run without a context.  (The demodulated denoise that reads the
// records is in yk_denoise.hip, next to the filter it wraps.)
//
// k_albedo: one lane per pixel, a block is a 32 x 8 tile of the film (yk_film_tile.h: neighbouring lanes
//   hit neighbouring triangles and, on a textured surface, neighbouring texels, so their requests share cache lines).  A
//   lane reads its id (one 16-byte load) and follows a four-hop gather: the shape's material index, mesh and three vertex
//   indices; the material (five dwords of its 44-byte record), the mesh flags and six uv floats; the texture's info (one
//   16-byte load); the texel (one 16-byte load); and writes one 16-byte record.  Every index is clamped into its array and
//   no load stands under a per-lane branch: a lane whose case needs no texture asks for texture 0 and drops the answer.
//   No LDS: which records a tile touches is not known before the ids are read.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "yk_albedo.h"
#include "yk_film_call.h"
#include "yk_film_tile.h"
#include "yk_path_state.h"
#include "yk_staging.h"
#include "yk_wave.h"

namespace {

__global__ __launch_bounds__(FT_TX* FT_TY) void k_albedo(const uint4* __restrict__ ids, DevScene sc, AlParams a, float4* __restrict__ out) {
    const uint32_t x = blockIdx.x * FT_TX + threadIdx.x, y = blockIdx.y * FT_TY + threadIdx.y;
    if (x >= a.res_x || y >= a.res_y) return;
    const size_t i = (size_t)y * a.res_x + x;
    const uint4 id = ids[i];
    float rec[4];
    al_pixel(a, sc, id.x, __uint_as_float(id.y), __uint_as_float(id.z), __uint_as_float(id.w), rec);
    out[i] = make_float4(rec[0], rec[1], rec[2], rec[3]);
}

// k_albedo_mean (yk_albedo_mean[_device], and every band of yk_render_albedo_mean): one lane per OUTPUT pixel, the same
//   32 x 8 tile.  A lane walks its s x s block of the large film's ids row by row (j outer, i inner: al_mean_pixel's
//   summation order), each id a 16-byte load followed by al_pixel's clamped four-hop gather, and writes one 16-byte record.
//   Lanes along x read ids 16*s bytes apart: a wave's 32 lanes of one row cover 512*s contiguous bytes per j, every byte
//   of which some lane uses within the same inner loop, so each line is fetched from HBM once and served from L2 after.
//   a.res_x x a.res_y is the output film (or one band of it); the ids have s*a.res_x records to a row.
__global__ __launch_bounds__(FT_TX* FT_TY) void k_albedo_mean(const uint4* __restrict__ ids_ss, DevScene sc, AlParams a, uint32_t s, float4* __restrict__ out) {
    const uint32_t x = blockIdx.x * FT_TX + threadIdx.x, y = blockIdx.y * FT_TY + threadIdx.y;
    if (x >= a.res_x || y >= a.res_y) return;
    float rec[4];
    al_mean_pixel(a, sc, ids_ss, x, y, s, rec);
    out[(size_t)y * a.res_x + x] = make_float4(rec[0], rec[1], rec[2], rec[3]);
}

// k_ids_band: k_guides_ids' id record alone (the same hit_surface_prim call, so the same bits), for the rays of a band of
//   rows [row0, row0 + rows) of a res_x-wide film, written at (y - row0) * res_x + x of the band's buffer.  The band's tile
//   holds these rows only; a pixel outside them or right of res_x writes nothing, so the index stays inside res_x * rows.
__global__ void k_ids_band(DevScene sc, PathBuffers cur, const int* hit_tri, uint32_t n, const uint32_t* pixel_xy, uint32_t res_x, uint32_t row0, uint32_t rows, uint4* ids) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 rd = cur.rayD[i];
    const uint32_t xy = pixel_xy[path_sample_id(rd)];
    const uint32_t yb = (xy >> 16) - row0, xb = xy & 0xffffu;
    if (yb >= rows || xb >= res_x) return;  // also a row above row0: the difference wraps
    const size_t px = (size_t)yb * res_x + xb;
    const int tri = hit_tri[i];
    uint4 id = make_uint4(YK_SURFACE_NONE, 0u, 0u, 0u);
    if (tri >= 0) {
        float t = 0.0f;
        const float4 ro = cur.rayO[i];
        (void)hit_surface_prim(sc, (uint32_t)tri & YK_HIT_PRIM_MASK, f4_xyz(ro), f4_xyz(rd), sc.texels != nullptr, &t, &id);
    }
    ids[px] = id;
}

yk_status check_call(const yk_scene* scene, const void* ids, uint16_t res_x, uint16_t res_y, const void* out) {
    if (!scene || !ids || !out || res_x == 0 || res_y == 0) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y;
    if (overlaps(out, n_px * sizeof(yk_albedo), ids, n_px * sizeof(yk_surface_id))) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

AlParams make_params(const yk_scene* scene, uint32_t res_x, uint32_t res_y) {
    AlParams a{};
    a.res_x = res_x;
    a.res_y = res_y;
    a.n_triangles = scene->n_triangles;
    a.n_shapes = scene->n_triangles + scene->n_spheres;
    a.n_vertices = scene->upd.n_vertices;
    a.n_meshes = scene->n_meshes;
    a.n_materials = scene->n_materials;
    a.n_textures = scene->n_textures;
    a.has_uvs = scene->upd.has_uvs ? 1u : 0u;
    return a;
}

yk_status enqueue(yk_context* ctx, hipStream_t st, const yk_scene* scene, const void* ids, uint16_t res_x, uint16_t res_y, void* out) {
    const AlParams a = make_params(scene, res_x, res_y);
    hipLaunchKernelGGL(k_albedo, ft_grid(res_x, res_y), ft_block(), 0, st, reinterpret_cast<const uint4*>(ids), scene->dev, a, reinterpret_cast<float4*>(out));
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

// The host instances' view of a scene's shading tables — the arrays al_pixel reads, as host arrays behind a DevScene —
// handed to use(const DevScene&): a host-only scene keeps them, a scene in device memory has them fetched for the call.
template <class Use>
yk_status with_host_tables(yk_context* ctx, const yk_scene* scene, const Use& use) {
    HostArrays h;
    const yk_status rc = scene_host_arrays(ctx, scene, HOST_INDICES | HOST_UVS | HOST_TRI_MESH | HOST_TRI_MATERIAL | HOST_MESH_FLAGS | HOST_MATERIALS | HOST_SPHERES | HOST_TEXTURES, "", h);
    if (rc != YK_OK) return rc;
    DevScene sc{};
    sc.indices = h->indices.data();
    sc.uvs = h->uvs.data();
    sc.tri_mesh = h->tri_mesh.data();
    sc.tri_material = h->tri_material.data();
    sc.mesh_flags = h->mesh_flags.data();
    sc.materials = h->materials.data();
    sc.spheres = h->spheres.data();
    sc.texels = h->texels.data();
    sc.tex_info = h->tex_info.data();
    use(sc);
    return YK_OK;
}

void albedo_host(const yk_scene* scene, const DevScene& sc, const yk_surface_id* ids, uint16_t res_x, uint16_t res_y, yk_albedo* out) {
    const AlParams a = make_params(scene, res_x, res_y);
    const size_t n_px = (size_t)res_x * res_y;
    for (size_t i = 0; i < n_px; ++i) {
        float rec[4];
        al_pixel(a, sc, ids[i].shape, ids[i].b[0], ids[i].b[1], ids[i].b[2], rec);
        std::memcpy(&out[i], rec, 16);
    }
}

// yk_albedo_mean's arguments: the ids are those of the (s * res_x) x (s * res_y) film
yk_status check_mean_call(const yk_scene* scene, const void* ids_ss, uint16_t res_x, uint16_t res_y, uint32_t s, const void* out) {
    if (!scene || !ids_ss || !out || res_x == 0 || res_y == 0) return YK_ERR_INVALID_ARGUMENT;
    if (s < 1u || s > YK_ALBEDO_MEAN_MAX_S || s * res_x > 65535u || s * res_y > 65535u) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y;
    if (overlaps(out, n_px * sizeof(yk_albedo), ids_ss, n_px * s * s * sizeof(yk_surface_id))) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

void albedo_mean_host(const yk_scene* scene, const DevScene& sc, const yk_surface_id* ids_ss, uint16_t res_x, uint16_t res_y, uint32_t s, yk_albedo* out) {
    const AlParams a = make_params(scene, res_x, res_y);
    for (uint32_t y = 0; y < res_y; ++y)
        for (uint32_t x = 0; x < res_x; ++x) {
            float rec[4];
            al_mean_pixel(a, sc, ids_ss, x, y, s, rec);
            std::memcpy(&out[(size_t)y * res_x + x], rec, 16);
        }
}

}  // namespace

namespace yk {
void launch_ids_band(hipStream_t s, const DevScene& sc, PathBuffers cur, const int* hit_tri, uint32_t n, const uint32_t* pixel_xy, uint32_t res_x, uint32_t row0, uint32_t rows, uint4* ids) {
    hipLaunchKernelGGL(k_ids_band, dim3((n + 255u) / 256u), dim3(256), 0, s, sc, cur, hit_tri, n, pixel_xy, res_x, row0, rows, ids);
}
}  // namespace yk

yk_status albedo_mean_enqueue(yk_context* ctx, hipStream_t st, const yk_scene* scene, const void* d_ids_ss, uint32_t res_x, uint32_t rows, uint32_t s, void* d_out) {
    const AlParams a = make_params(scene, res_x, rows);
    hipLaunchKernelGGL(k_albedo_mean, ft_grid(res_x, rows), ft_block(), 0, st, reinterpret_cast<const uint4*>(d_ids_ss), scene->dev, a, s, reinterpret_cast<float4*>(d_out));
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

extern "C" {

yk_status yk_surface_albedo(yk_context* ctx, const yk_scene* scene, const yk_surface_id* ids, uint16_t res_x, uint16_t res_y, yk_albedo* out) try {
    if (check_call(scene, ids, res_x, res_y, out) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_surface_albedo: bad argument");
    const size_t n_px = (size_t)res_x * res_y;
    if (!ctx) return with_host_tables(ctx, scene, [&](const DevScene& sc) { albedo_host(scene, sc, ids, res_x, res_y, out); });  // the host instance
    YK_LOCK(ctx);
    if (yk_status rs = scene_on_context(ctx, scene, "yk_surface_albedo")) return rs;
    Staging sg(ctx);
    const yk_surface_id* d_ids = sg.upload(ids, n_px);
    yk_albedo* d_out = sg.output(out, n_px);
    return sg.run([&] { return enqueue(ctx, sg.stream, scene, d_ids, res_x, res_y, d_out); });
}
YK_CATCH(ctx)

yk_status yk_surface_albedo_device(yk_context* ctx, const yk_scene* scene, const void* d_ids, uint16_t res_x, uint16_t res_y, void* d_out, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_call(scene, d_ids, res_x, res_y, d_out) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_surface_albedo_device: bad argument");
    if (yk_status rs = scene_on_context(ctx, scene, "yk_surface_albedo_device")) return rs;
    if (misaligned(16, d_ids, d_out))  // 16-byte loads and stores of the records
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_surface_albedo_device: ids and output must be 16-byte aligned");
    return enqueue(ctx, device_call_stream(ctx, stream), scene, d_ids, res_x, res_y, d_out);
}

yk_status yk_albedo_mean(yk_context* ctx, const yk_scene* scene, const yk_surface_id* ids_ss, uint16_t res_x, uint16_t res_y, uint32_t s, yk_albedo* out) try {
    if (check_mean_call(scene, ids_ss, res_x, res_y, s, out) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_albedo_mean: bad argument");
    const size_t n_px = (size_t)res_x * res_y;
    if (!ctx) return with_host_tables(ctx, scene, [&](const DevScene& sc) { albedo_mean_host(scene, sc, ids_ss, res_x, res_y, s, out); });  // the host instance
    YK_LOCK(ctx);
    if (yk_status rs = scene_on_context(ctx, scene, "yk_albedo_mean")) return rs;
    Staging sg(ctx);
    const yk_surface_id* d_ids = sg.upload(ids_ss, n_px * s * s);
    yk_albedo* d_out = sg.output(out, n_px);
    return sg.run([&] { return albedo_mean_enqueue(ctx, sg.stream, scene, d_ids, res_x, res_y, s, d_out); });
}
YK_CATCH(ctx)

yk_status yk_albedo_mean_device(yk_context* ctx, const yk_scene* scene, const void* d_ids_ss, uint16_t res_x, uint16_t res_y, uint32_t s, void* d_out, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_mean_call(scene, d_ids_ss, res_x, res_y, s, d_out) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_albedo_mean_device: bad argument");
    if (yk_status rs = scene_on_context(ctx, scene, "yk_albedo_mean_device")) return rs;
    if (misaligned(16, d_ids_ss, d_out)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_albedo_mean_device: ids and output must be 16-byte aligned");
    return albedo_mean_enqueue(ctx, device_call_stream(ctx, stream), scene, d_ids_ss, res_x, res_y, s, d_out);
}

}  // extern "C"
