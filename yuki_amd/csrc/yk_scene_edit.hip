// yk_scene_edit.hip — the sphere table of yk_scene_apply_edit[_device] on the device (gfx950): the caller's yk_sphere_desc
// records, in HBM, become what the scene keeps of its spheres.  One streaming kernel, one sphere a lane, 256 lanes a block:
//   k_spheres_in   reads a 136-byte record (34 consecutive dwords at a 4-byte aligned address, which is all a global load
//                  of any width needs on gfx950: the compiler fetches them as eight 16-byte loads and one 8-byte load),
//                  tests its 33 floats for NaN and infinity and its material for the range,
//                  and writes the 144-byte DevSphere record (nine 16-byte stores), the six floats of Sphere::world_bound
//                  (inp::sphere_bound, three 8-byte stores) and the material index.  A failed test raises a bit of ONE flag
//                  word with an integer atomic; no float atomics, and no load follows an index: the material is compared,
//                  never followed.
// Everything is written to scratch of the caller: the flag is read back before anything of the scene is written
// (stage_spheres_device), and only then the staged tables are copied over the scene's (commit_spheres_device).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "yk_scene_route.h"
#include "yk_scene_update.h"

using namespace yk;
using namespace yk::upd;

namespace {

const int kThreads = 256;
const int kWords = (int)(sizeof(yk_sphere_desc) / 4);  // 34
static_assert(sizeof(yk_sphere_desc) == 136 && sizeof(DevSphere) == 144, "the record sizes k_spheres_in is written for");

__global__ void __launch_bounds__(kThreads) k_spheres_in(const uint32_t* __restrict__ in, uint32_t n_spheres, uint32_t n_materials, uint4* __restrict__ table, float2* __restrict__ bounds,
                                                         int32_t* __restrict__ material, uint32_t* flag) {
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n_spheres) return;
    const uint32_t* p = in + (size_t)kWords * k;
    uint32_t w[kWords];
#pragma unroll
    for (int i = 0; i < kWords; ++i) w[i] = p[i];  // constant indices: the record lives in registers
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 33; ++i) bad = bad || not_finite_bits(w[i]);  // two matrices and the radius
    const int32_t m = (int32_t)w[33];
    const bool bad_material = m < 0 || (uint32_t)m >= n_materials;
    if (bad || bad_material) atomicOr(flag, (bad ? (uint32_t)YK_SPHERES_NOT_FINITE : 0u) | (bad_material ? (uint32_t)YK_SPHERES_MATERIAL : 0u));
    float o2w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) o2w[i] = __uint_as_float(w[i]);
    const float radius = __uint_as_float(w[32]);
    uint4* out = table + 9 * (size_t)k;  // a DevSphere: o2w, w2o, (radius, material, swaps_handedness, pad)
#pragma unroll
    for (int v = 0; v < 8; ++v) out[v] = make_uint4(w[4 * v], w[4 * v + 1], w[4 * v + 2], w[4 * v + 3]);
    out[8] = make_uint4(w[32], w[33], inp::swaps_handedness(o2w) ? 1u : 0u, 0u);
    float b[6];
    inp::sphere_bound(o2w, radius, b);
    float2* ob = bounds + 3 * (size_t)k;
    ob[0] = make_float2(b[0], b[1]);
    ob[1] = make_float2(b[2], b[3]);
    ob[2] = make_float2(b[4], b[5]);
    material[k] = m;
}

}  // namespace

uint32_t stage_spheres_device(yk_context* ctx, yk_scene* s, const void* d_in, DevScratch& tmp, StagedSpheres* staged, uint32_t* flag) {
    *flag = 0;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const uint32_t n = s->n_spheres;
    uint32_t* d_flag = nullptr;
    if (!tmp.get(staged->table, n) || !tmp.get(staged->bounds, 6 * (size_t)n) || !tmp.get(staged->material, n) || !tmp.get(d_flag, 1)) return layout_reason_of(tmp.err);
    ROUTE_TRY(st, hipMemsetAsync(d_flag, 0, 4, st));
    k_spheres_in<<<route_blocks(n, kThreads), kThreads, 0, st>>>(reinterpret_cast<const uint32_t*>(d_in), n, s->n_materials, reinterpret_cast<uint4*>(staged->table), reinterpret_cast<float2*>(staged->bounds),
                                                 staged->material, d_flag);
    ROUTE_TRY(st, hipGetLastError());
    ROUTE_TRY(st, hipMemcpyAsync(flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    ROUTE_TRY(st, hipStreamSynchronize(st));
    return YK_LAYOUT_REASON_NONE;
}

uint32_t commit_spheres_device(yk_context* ctx, yk_scene* s, const StagedSpheres& staged, std::vector<int32_t>* material) {
    yk_scene::UpdateState& u = s->upd;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const size_t n = s->n_spheres;
    if (!u.planned || s->spheres.bytes < n * sizeof(DevSphere) || u.sphere_b.bytes < 24 * n || u.sphere_bounds.size() != 6 * n) return YK_LAYOUT_REASON_DEVICE_ERROR;
    material->resize(n);
    ROUTE_TRY(st, hipMemcpyAsync(s->spheres.p, staged.table, n * sizeof(DevSphere), hipMemcpyDeviceToDevice, st));
    ROUTE_TRY(st, hipMemcpyAsync(u.sphere_b.p, staged.bounds, 24 * n, hipMemcpyDeviceToDevice, st));
    ROUTE_TRY(st, hipMemcpyAsync(u.sphere_bounds.data(), staged.bounds, 24 * n, hipMemcpyDeviceToHost, st));
    ROUTE_TRY(st, hipMemcpyAsync(material->data(), staged.material, 4 * n, hipMemcpyDeviceToHost, st));
    ROUTE_TRY(st, hipStreamSynchronize(st));
    return YK_LAYOUT_REASON_NONE;
}
