// yk_stage_kernels.hip — kernels of the per-stage entry points (yk_stages.cpp): the device math, sampler, BSDF, light and
// surface functions called on arrays for the unit tests, and the packing of caller-supplied rays.  None runs in the render loop.
#include <hip/hip_runtime.h>

#include "yk_device.h"
#include "yk_geom.h"
#include "yk_kernels.h"
#include "yk_rng.h"

namespace yk {

__global__ void k_device_math(int fn, size_t n, const float* a, const float* b, float* out) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (fn >= 11 && fn <= 27) {  // vector functions of yk_math.h / yk_geom.h on triples: a, b = n/3 packed V3, thread 3k handles triple k
        if (i % 3) return;
        V3 va = V3{a[i], a[i + 1], a[i + 2]}, vb = b ? V3{b[i], b[i + 1], b[i + 2]} : V3{0.0f, 0.0f, 0.0f};
        V3 r = V3{0.0f, 0.0f, 0.0f};
        switch (fn) {
            case 11: r.x = dot(va, vb); break;
            case 12: r = cross(va, vb); break;
            case 13: r.x = length(va); break;
            case 14: r = normalize(va); break;
            case 15: r.x = (float)max_dimension(va); break;
            case 16: r = vabs(va); break;
            case 17: r.x = dot_nv(va, vb); break;
            case 18: {  // the permutation Triangle::intersect derives from the ray direction (triangle.rs:60-66)
                RayTri rt = ray_tri_setup(va);
                r = V3{(float)rt.kx, (float)rt.ky, (float)rt.kz};
                break;
            }
            case 19: r = V3{rmin(va.x, vb.x), rmin(va.y, vb.y), rmin(va.z, vb.z)}; break;
            case 20: r = V3{rmax(va.x, vb.x), rmax(va.y, vb.y), rmax(va.z, vb.z)}; break;
            case 21: r = faceforward_v(va, vb); break;
            // the operator traits of Vec3 / Point3 / Normal as the kernels use them (yk_math.h)
            case 22: r = va + vb; break;
            case 23: r = va - vb; break;
            case 24: r = va * vb.x; break;
            case 25: r = va / vb.x; break;
            case 26: r = -va; break;
            case 27: r.x = len_sqr(va); break;
            default: break;
        }
        out[i] = r.x;
        out[i + 1] = r.y;
        out[i + 2] = r.z;
        return;
    }
    float x = a[i], y = b ? b[i] : 0.0f, r;
    switch (fn) {
        case 0: r = det_sinf(x); break;
        case 1: r = det_cosf(x); break;
        case 2: r = det_tanf(x); break;
        case 3: r = det_logf(x); break;
        case 4: r = det_acosf(x); break;
        case 5: r = det_atan2f(x, y); break;
        case 6: r = sqrtf(x); break;
        case 7: r = x / y; break;
        case 8: r = (float)sqrt((double)x); break;
        case 9: r = rmin(x, y); break;
        case 10: r = rmax(x, y); break;
        case 28:  // det_sincosf (the reduction shared by both results): its sine ...
        case 29: {  // ... and its cosine
            float sn, cs;
            det_sincosf(x, sn, cs);
            r = fn == 28 ? sn : cs;
            break;
        }
        default: r = 0.0f;
    }
    out[i] = r;
}

__global__ void k_sampler_sequence(SamplerCfg cfg, uint32_t px, uint32_t py, uint32_t sample_index, const uint8_t* dims, size_t n_draws, float* out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    SamplerState st = sampler_start(cfg, px, py, sample_index, 0);
    for (size_t k = 0; k < n_draws; ++k) {
        if (dims[k] == 1) {
            out[2 * k] = sampler_get_1d(cfg, st);
            out[2 * k + 1] = 0.0f;
        } else {
            float ux, uy;
            sampler_get_2d(cfg, st, ux, uy);
            out[2 * k] = ux;
            out[2 * k + 1] = uy;
        }
    }
}

__global__ void k_bsdf_test(Material m, size_t n, const float* ng, const float* ns, const float* dpdu, const float* wo, const float* wi_or_u,
                            int sample, float* out) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    Frame fr = make_frame(ld3(ng, (uint32_t)i), ld3(ns, (uint32_t)i), ld3(dpdu, (uint32_t)i));
    V3 w = ld3(wo, (uint32_t)i);
    if (!sample) {
        RGB f = bsdf_f(m, fr, w, ld3(wi_or_u, (uint32_t)i));
        out[3 * i] = f.r;
        out[3 * i + 1] = f.g;
        out[3 * i + 2] = f.b;
    } else {
        BsdfSample s = bsdf_sample_f(m, fr, w, wi_or_u[2 * i], wi_or_u[2 * i + 1]);
        out[8 * i + 0] = s.wi.x;
        out[8 * i + 1] = s.wi.y;
        out[8 * i + 2] = s.wi.z;
        out[8 * i + 3] = s.f.r;
        out[8 * i + 4] = s.f.g;
        out[8 * i + 5] = s.f.b;
        out[8 * i + 6] = s.pdf;
        out[8 * i + 7] = (float)s.type;
    }
}

// Light::sample_li + VisibilityTester::ray for n surface points (stage entry yk_light_sample)
__global__ void k_light_test(DevLight L, int index, size_t n, const float* p, const float* ng, const float* u, float* out) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 sp = ld3(p, (uint32_t)i), nn = ld3(ng, (uint32_t)i);
    LightSample ls = sample_light(L, index, sp, u[2 * i], u[2 * i + 1]);
    // p0.spawn_ray_to(p1), interaction.rs:44-59 — as vertex_light does
    V3 offset = nn * 0.001f;
    V3 so = dot(ls.p1 - sp, nn) > 0.0f ? sp + offset : sp - offset;
    V3 sd = ls.p1 - so;
    float* o = out + 18 * i;
    o[0] = ls.l.x; o[1] = ls.l.y; o[2] = ls.l.z;
    o[3] = ls.li.r; o[4] = ls.li.g; o[5] = ls.li.b;
    o[6] = ls.pdf;
    o[7] = ls.has_vis ? 1.0f : 0.0f;
    o[8] = (float)ls.area_light;
    o[9] = ls.p1.x; o[10] = ls.p1.y; o[11] = ls.p1.z;
    o[12] = so.x; o[13] = so.y; o[14] = so.z;
    o[15] = sd.x; o[16] = sd.y; o[17] = sd.z;
}

// The SurfaceInteraction of n closest hits (stage entry yk_surface), YK_SURFACE_FLOATS floats per ray.  hit_word[i] is what
// the render-loop closest-hit kernel reported: -1 or the leaf-order slot | kind bits.  route 0 builds the surface as k_shade,
// the debug integrators and the guide pass do (hit_surface_prim, by slot); route 1 as k_whitted and k_path_debug do
// (hit_surface, by the source shape the slot's record names); t and the barycentrics of route 1 come from the same intersection
// functions hit_surface calls.  A miss is an all-zero record with shape -1.
__global__ void k_surface_test(DevScene sc, size_t n, const float4* rayO, const float4* rayD, const int* hit_word, int route, float* out) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    float* r = out + YK_SURFACE_FLOATS * i;
    for (int k = 0; k < YK_SURFACE_FLOATS; ++k) r[k] = 0.0f;
    r[21] = -1.0f;
    const int h = hit_word[i];
    if (h < 0) return;
    const uint32_t prim = (uint32_t)h & YK_HIT_PRIM_MASK;
    const float4 fo = rayO[i], fd = rayD[i];
    const V3 o = V3{fo.x, fo.y, fo.z}, d = V3{fd.x, fd.y, fd.z};
    Surface sf;
    float t = 0.0f;
    uint4 id = make_uint4(0u, 0u, 0u, 0u);
    if (route == 0) {
        sf = hit_surface_prim(sc, prim, o, d, sc.texels != nullptr, &t, &id);
    } else {
        const uint32_t shape = __float_as_uint(sc.tris[3 * prim + 1].w);
        sf = hit_surface(sc, shape, o, d);
        id.x = shape;
        if (shape >= sc.n_triangles) {
            V3 ro, rd;
            sphere_hit_t(sc.spheres[shape - sc.n_triangles], o, d, __builtin_inff(), t, ro, rd);
        } else {
            const uint32_t i0 = sc.indices[3 * shape], i1 = sc.indices[3 * shape + 1], i2 = sc.indices[3 * shape + 2];
            TriHit th = TriHit{0.0f, 0.0f, 0.0f, 0.0f};
            tri_intersect(o, ray_tri_setup(d), __builtin_inff(), ld3(sc.points, i0), ld3(sc.points, i1), ld3(sc.points, i2), th);
            t = th.t;
            id.y = __float_as_uint(th.b0);
            id.z = __float_as_uint(th.b1);
            id.w = __float_as_uint(th.b2);
        }
    }
    r[0] = 1.0f;
    r[1] = t;
    r[2] = sf.p.x; r[3] = sf.p.y; r[4] = sf.p.z;
    r[5] = sf.n.x; r[6] = sf.n.y; r[7] = sf.n.z;
    r[8] = sf.ns.x; r[9] = sf.ns.y; r[10] = sf.ns.z;
    r[11] = sf.dpdus.x; r[12] = sf.dpdus.y; r[13] = sf.dpdus.z;
    r[14] = sf.wo.x; r[15] = sf.wo.y; r[16] = sf.wo.z;
    r[17] = sf.u; r[18] = sf.v;
    r[19] = (float)sf.material;
    r[20] = (float)sf.area_light;
    r[21] = (float)id.x;
    r[22] = __uint_as_float(id.y); r[23] = __uint_as_float(id.z); r[24] = __uint_as_float(id.w);
    const V3 so = spawn_origin(sf.p, sf.n, d);  // Interaction::spawn_ray for a ray that goes on along d
    r[25] = so.x; r[26] = so.y; r[27] = so.z;
}

__global__ void k_pack_rays(size_t n, const float* o, const float* d, float4* rayO, float4* rayD) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    rayO[i] = make_float4(o[3 * i], o[3 * i + 1], o[3 * i + 2], 0.0f);
    rayD[i] = make_float4(d[3 * i], d[3 * i + 1], d[3 * i + 2], 0.0f);
}
__global__ void k_pack_shadow_rays(size_t n, const float* o, const float* d, const float* t_max, const int* area_light, float4* shO, float4* shD) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    shO[i] = make_float4(o[3 * i], o[3 * i + 1], o[3 * i + 2], t_max[i]);
    shD[i] = make_float4(d[3 * i], d[3 * i + 1], d[3 * i + 2], __uint_as_float((unsigned)(area_light ? area_light[i] : -1)));
}
__global__ void k_unpack_rays(size_t n, const float4* rayO, const float4* rayD, float* o, float* d) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 a = rayO[i], b = rayD[i];
    o[3 * i] = a.x; o[3 * i + 1] = a.y; o[3 * i + 2] = a.z;
    d[3 * i] = b.x; d[3 * i + 1] = b.y; d[3 * i + 2] = b.z;
}

static inline unsigned blocks_for(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

void launch_device_math(hipStream_t s, int fn, size_t n, const float* a, const float* b, float* out) {
    hipLaunchKernelGGL(k_device_math, dim3(blocks_for(n, 256)), dim3(256), 0, s, fn, n, a, b, out);
}
void launch_sampler_sequence(hipStream_t s, const SamplerCfg& cfg, uint32_t px, uint32_t py, uint32_t sample_index, const uint8_t* dims, size_t n_draws,
                             float* out) {
    hipLaunchKernelGGL(k_sampler_sequence, dim3(1), dim3(64), 0, s, cfg, px, py, sample_index, dims, n_draws, out);
}
void launch_light_test(hipStream_t s, const DevLight& L, int index, size_t n, const float* p, const float* ng, const float* u, float* out) {
    hipLaunchKernelGGL(k_light_test, dim3(blocks_for(n, 256)), dim3(256), 0, s, L, index, n, p, ng, u, out);
}
void launch_bsdf_test(hipStream_t s, const Material& m, size_t n, const float* ng, const float* ns, const float* dpdu, const float* wo,
                      const float* wi_or_u, int sample, float* out) {
    hipLaunchKernelGGL(k_bsdf_test, dim3(blocks_for(n, 256)), dim3(256), 0, s, m, n, ng, ns, dpdu, wo, wi_or_u, sample, out);
}
void launch_surface_test(hipStream_t s, const DevScene& sc, size_t n, const float4* rayO, const float4* rayD, const int* hit_word, int route, float* out) {
    hipLaunchKernelGGL(k_surface_test, dim3(blocks_for(n, 256)), dim3(256), 0, s, sc, n, rayO, rayD, hit_word, route, out);
}
void launch_pack_rays(hipStream_t s, size_t n, const float* o, const float* d, float4* rayO, float4* rayD) {
    hipLaunchKernelGGL(k_pack_rays, dim3(blocks_for(n, 256)), dim3(256), 0, s, n, o, d, rayO, rayD);
}
void launch_pack_shadow_rays(hipStream_t s, size_t n, const float* o, const float* d, const float* t_max, const int* area_light, float4* shO,
                             float4* shD) {
    hipLaunchKernelGGL(k_pack_shadow_rays, dim3(blocks_for(n, 256)), dim3(256), 0, s, n, o, d, t_max, area_light, shO, shD);
}
void launch_unpack_rays(hipStream_t s, size_t n, const float4* rayO, const float4* rayD, float* o, float* d) {
    hipLaunchKernelGGL(k_unpack_rays, dim3(blocks_for(n, 256)), dim3(256), 0, s, n, rayO, rayD, o, d);
}

}  // namespace yk
